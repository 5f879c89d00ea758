#!/usr/bin/env python3
"""The velocity modulator and the terrain / reference stage of E environments four ways -> profiles/batch_terrain.json.

For each E in {1, 1024, 4096}, in one process, blocks alternate between

  class    BatchedVelocityModulator.step + BatchedTerrainEstimator.step: 200 back-to-back pairs between two events
  c_call   srbd_vm_modulate_device + srbd_terrain_ref_step_device through ctypes with prebuilt io structs, likewise
  torch    the same maths as plain torch operations on (E, ...) tensors (torch.atan / cos / sin: the device library's,
           so equal to rounding, not to the bit), likewise
  host     E x (srbd_vm_modulate, srbd_terrain_estimate, srbd_reference_assemble) through ctypes, the argument
           pointers built before the clock starts: what a loop that keeps this stage on the host pays per step, before
           its E x 18 doubles are copied up

after a warm-up of each.  The three device kinds are device time between events, so the enqueue cost of back-to-back
calls is inside them: a kind whose time does not move with E is enqueue-bound.  The host kind is wall time.  Three
blocks per kind; the median block is reported per step (both launches together), in us.  One run on one box.

  python scripts/batch_terrain_timing.py [--envs 1 1024 4096] [--commit ID] [--out profiles/batch_terrain.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]

import torch  # noqa: E402  (torch first: one HIP runtime per process)

from quadruped_pympc_amd import _lib  # noqa: E402
from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator  # noqa: E402
from quadruped_pympc_amd.helpers.velocity_modulator import BatchedVelocityModulator  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_terrain.json")
LAUNCHES, WARMUP, BLOCKS, HOST_STEPS = 200, 20, 3, 5
REF_Z = 0.3


def inputs(E):
    rng = np.random.default_rng(E)
    base = rng.uniform(-2, 2, (E, 3))
    hips = base[:, None, :] + rng.uniform(-0.3, 0.3, (E, 4, 3))
    return dict(base_pos=base, com_pos=base + rng.uniform(-0.03, 0.03, (E, 3)), yaws=rng.uniform(-3.0, 3.0, E),
                lin=rng.uniform(-0.3, 0.6, (E, 3)), ang=rng.uniform(-1, 1, (E, 3)), hips=hips,
                feet=hips + rng.uniform(-0.18, 0.18, (E, 4, 3)))


def torch_form(d, state, ref):
    """The modulator, the estimator and the row as plain torch operations; state (E, 3) and ref (E, 24) in place."""
    lin, ang, feet, hips, base = d["lin"], d["ang"], d["feet"], d["hips"], d["base_pos"]
    dist = torch.sqrt(torch.square(feet[..., 0] - hips[..., 0]) + torch.square(feet[..., 1] - hips[..., 1]))
    hit = ~((lin[:, 0] < 0.01) & (lin[:, 1] < 0.01)) & (dist > 0.2).any(dim=1)
    lin = torch.where(hit[:, None], lin * 0.0, lin)
    ang = torch.where(hit[:, None], ang * 0.0, ang)
    c, s = torch.cos(d["yaws"])[:, None], torch.sin(d["yaws"])[:, None]
    v = feet - base[:, None, :]
    r = torch.stack([c * v[..., 0] + s * v[..., 1], -s * v[..., 0] + c * v[..., 1], v[..., 2]], dim=-1)
    front, back, left, right = r[:, 0] - r[:, 1], r[:, 2] - r[:, 3], r[:, 0] - r[:, 2], r[:, 1] - r[:, 3]

    def slope(a, b, axis):
        return (torch.atan(a[:, 2].abs() / (a[:, axis] + 0.001).abs())
                + torch.atan(b[:, 2].abs() / (b[:, axis] + 0.001).abs())) * 0.5

    pitch, roll = slope(left, right, 0), slope(front, back, 1)
    roll = torch.where(front[:, 2] * 0.5 + back[:, 2] * 0.5 < 0, -roll, roll)
    pitch = torch.where(left[:, 2] * 0.5 + right[:, 2] * 0.5 > 0, -pitch, pitch)
    state[:, 0] = 0.0  # roll_activated is off by default
    state[:, 1] = state[:, 1] * 0.99 + pitch * 0.01
    state[:, 2] = state[:, 2] * 0.2 + (feet[..., 2].sum(dim=1) / 4) * 0.8
    roll, pitch = state[:, 0], state[:, 1]
    cr, sr, cp, sp = torch.cos(roll), torch.sin(roll), torch.cos(pitch), torch.sin(pitch)
    v0 = cp * lin[:, 0] + sp * sr * lin[:, 1] + sp * cr * lin[:, 2]
    v1 = cr * lin[:, 1] - sr * lin[:, 2]
    v2 = -sp * lin[:, 0] + cp * sr * lin[:, 1] + cp * cr * lin[:, 2]
    v2 = torch.where(pitch > 0, -v2, v2)
    steep = pitch.abs() > 0.2
    v0, v2 = torch.where(steep, v0 / 2, v0), torch.where(steep, v2 * 2, v2)
    ref[:, 0:2] = 0.0
    ref[:, 2] = (REF_Z + state[:, 2]) - (base[:, 2] - d["com_pos"][:, 2])
    ref[:, 3], ref[:, 4], ref[:, 5] = v0, v1, v2
    ref[:, 6], ref[:, 7], ref[:, 8] = roll, pitch, 0.0
    ref[:, 9:12] = ang


def measure(E):
    x = inputs(E)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    est, vm = BatchedTerrainEstimator(E, REF_Z), BatchedVelocityModulator(E)
    stream = torch.cuda.Stream()
    ref = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    lin = torch.empty((E, 3), dtype=torch.float64, device="cuda")
    ang = torch.empty((E, 3), dtype=torch.float64, device="cuda")
    tstate = torch.zeros((E, 3), dtype=torch.float64, device="cuda")
    vio = _lib.SrbdVmBatchIo(lin=d["lin"].data_ptr(), ang=d["ang"].data_ptr(), feet=d["feet"].data_ptr(),
                             hips=d["hips"].data_ptr(), max_distance=0.2, lin_out=lin.data_ptr(),
                             ang_out=ang.data_ptr())
    tio = _lib.SrbdTerrainRefBatchIo(base_pos=d["base_pos"].data_ptr(), com_pos=d["com_pos"].data_ptr(),
                                     com_pos_offset_w=None, yaws=d["yaws"].data_ptr(), lin=lin.data_ptr(),
                                     ang=ang.data_ptr(), feet=d["feet"].data_ptr(), frg=None, ref_z=REF_Z,
                                     ref=ref.data_ptr(), terrain=None)
    handle, state_ptr = C.c_void_p(stream.cuda_stream), est.state.data_ptr()
    vm_c, terr_c = _lib.lib.srbd_vm_modulate_device, _lib.lib.srbd_terrain_ref_step_device

    def timed(body):
        def run(n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(n):
                body()
            t1.record(stream)
            stream.synchronize()
            return t0.elapsed_time(t1) * 1e3 / n  # us per step
        return run

    def class_step():
        vm.step(d["lin"], d["ang"], d["feet"], d["hips"], out=(lin, ang), stream=stream)
        est.step(d["base_pos"], d["com_pos"], d["yaws"], lin, ang, ref, lift_off=d["feet"], stream=stream)

    def c_call():
        assert vm_c(E, C.byref(vio), handle) == 0 and terr_c(state_ptr, E, C.byref(tio), handle) == 0

    def torch_step():
        with torch.cuda.stream(stream):
            torch_form(d, tstate, ref)

    host = (_lib.SrbdTerrainEst * E)()
    for e in range(E):
        assert _lib.lib.srbd_terrain_est_init(C.byref(host[e])) == 0
    p = _lib.dptr
    lo, ao, rows = np.zeros((E, 3)), np.zeros((E, 3)), np.zeros((E, 12))
    args = [(C.byref(host[e]), p(x["lin"][e]), p(x["ang"][e]), p(x["feet"][e]), p(x["hips"][e]), p(lo[e]), p(ao[e]),
             p(x["base_pos"][e]), float(x["yaws"][e]), float(x["base_pos"][e, 2]), float(x["com_pos"][e, 2]),
             p(rows[e])) for e in range(E)]
    mod, estimate, assemble = (_lib.lib.srbd_vm_modulate, _lib.lib.srbd_terrain_estimate,
                               _lib.lib.srbd_reference_assemble)

    def host_loop(n):
        t0 = time.perf_counter()
        for _ in range(n):
            for g, li, an, ft, hp, l_o, a_o, bp, yaw, bz, cz, row in args:
                mod(0.2, li, an, ft, hp, l_o, a_o)
                estimate(g, bp, yaw, ft, None)
                assemble(g, REF_Z, bz, cz, 0.0, l_o, a_o, row)
        return (time.perf_counter() - t0) * 1e6 / n  # us per step of E environments

    kinds = {"class": timed(class_step), "c_call": timed(c_call), "torch": timed(torch_step), "host": host_loop}
    for k, run in kinds.items():
        run(1 if k == "host" else WARMUP)
    s = {k: [] for k in kinds}
    for _ in range(BLOCKS):
        for k, run in kinds.items():
            s[k].append(run(HOST_STEPS if k == "host" else LAUNCHES))
    row = {"num_envs": E}
    for k, v in s.items():
        m = float(np.median(v))
        row[k] = {"us_per_step": round(m, 2), "blocks": [round(b, 2) for b in v]}
    row["host_over_c_call"] = round(row["host"]["us_per_step"] / row["c_call"]["us_per_step"], 1)
    row["torch_over_c_call"] = round(row["torch"]["us_per_step"] / row["c_call"]["us_per_step"], 1)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git's HEAD of this checkout)")
    args = ap.parse_args()
    rows = [measure(E) for E in args.envs]
    try:
        commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                               capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (not a git checkout)"
    doc = {"workload": {"ref_z": REF_Z, "max_distance": 0.2, "feet": "array", "launches_per_step": 2},
           "device": torch.cuda.get_device_name(0), "commit": commit, "launches": LAUNCHES, "warmup": WARMUP,
           "blocks": BLOCKS, "host_steps": HOST_STEPS,
           "note": "one run on one box; class / c_call / torch: device time between events over back-to-back steps "
                   "(both launches), so enqueue cost is inside; host: wall time of E x 3 ctypes calls with prebuilt "
                   "argument pointers",
           "rows": rows}
    print(f"{'E':>6} {'class':>9} {'c_call':>9} {'torch':>9} {'host':>11}   (us per step)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['class']['us_per_step']:>9} {r['c_call']['us_per_step']:>9} "
              f"{r['torch']['us_per_step']:>9} {r['host']['us_per_step']:>11}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
