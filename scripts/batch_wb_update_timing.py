#!/usr/bin/env python3
"""update_state_and_reference of E environments four ways -> profiles/batch_wb_update.json.

For each E in {1, 1024, 4096}, in a child process of its own (started under ``timeout``), blocks alternate between

  c_chain      (a) the existing C calls through ctypes with prebuilt io structs: srbd_vm_modulate_device,
               srbd_pgg_run_device, srbd_pgg_contact_sequence_device, srbd_frg_step_device,
               srbd_terrain_ref_step_device, srbd_stc_touch_down_device -- and the two (E, 4) row copies of the contact
               bookkeeping a hand-wired loop makes between them
  class_chain  (b) the existing class calls: vm.step, gait.run, gait.compute_contact_sequence, frg.step,
               terrain_est.step, stc_touch_down_device, with the same bookkeeping
  c_fused      (c) srbd_wb_update_device through ctypes with a prebuilt io struct
  class_fused  (d) BatchedWBInterface.update_state_and_reference_device

All optional stages on (start-and-stop too in (c) and (d): the chain has no such call, so (a) and (b) run one stage
less), H = 12, 200 back-to-back control steps on one stream.  Per block both the wall time up to the stream's
synchronisation and the device time between two events; three blocks per kind and round, the median reported per
step in us; two rounds, both reported, so that the run-to-run spread stands beside every ratio.  One run on one box.

  python scripts/batch_wb_update_timing.py [--envs 1 1024 4096] [--commit ID] [--out profiles/batch_wb_update.json]
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
OUT = os.path.join(ROOT, "profiles", "batch_wb_update.json")
STEPS, WARMUP, BLOCKS, ROUNDS = 200, 20, 3, 2
H, LOOKAHEAD, SIM_DT, MPC_DT, REF_Z, CHN, GRAVITY = 12, 3, 0.002, 0.02, 0.3, 0.3, 9.81
CHILD_TIMEOUT = 240


def measure(E):
    import torch  # torch first: one HIP runtime per process

    from quadruped_pympc_amd import _lib
    from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
    from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
    from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
    from quadruped_pympc_amd.helpers.velocity_modulator import BatchedVelocityModulator
    from quadruped_pympc_amd.interfaces.wb_interface_batched import BatchedWBInterface

    rng = np.random.default_rng(E)
    base = rng.uniform(-2, 2, (E, 3))
    hips = base[:, None, :] + rng.uniform(-0.3, 0.3, (E, 4, 3))
    x = dict(com_pos=base + rng.uniform(-0.03, 0.03, (E, 3)), base_pos=base, base_lin_vel=rng.uniform(-0.5, 0.5, (E, 3)),
             euler=rng.uniform(-0.1, 0.1, (E, 3)), base_ang_vel=rng.uniform(-0.5, 0.5, (E, 3)),
             feet=hips + rng.uniform(-0.18, 0.18, (E, 4, 3)), hips=hips, ref_lin=rng.uniform(-0.3, 0.6, (E, 3)),
             ref_ang=rng.uniform(-1, 1, (E, 3)))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    yaws = d["euler"][:, 2].contiguous()
    lift = np.ascontiguousarray(x["feet"])

    def parts():
        return (BatchedPeriodicGaitGenerator(E, 0.65, 1.4, 0, H), BatchedFootholdReferenceGenerator(E, 0.4, 0.3, lift),
                BatchedTerrainEstimator(E, REF_Z))

    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    # (a), (b): one set of state and buffers
    gait, frg, terr = parts()
    vm = BatchedVelocityModulator(E, activated=True)
    lin, ang = torch.empty((E, 3), dtype=f64, device="cuda"), torch.empty((E, 3), dtype=f64, device="cuda")
    contacts = torch.zeros((E, 4, H), dtype=f32, device="cuda")
    cur, prev = torch.ones((E, 4), dtype=f32, device="cuda"), torch.ones((E, 4), dtype=f32, device="cuda")
    flags = torch.empty((E, 4), dtype=f32, device="cuda")
    seeds, ref = torch.empty((E, 4, 3), dtype=f64, device="cuda"), torch.zeros((E, 24), dtype=f64, device="cuda")
    edge, optimize = torch.zeros(E, dtype=i32, device="cuda"), torch.empty(E, dtype=i32, device="cuda")
    dts, lens = np.array([MPC_DT]), np.array([H], dtype=np.int32)
    vio = _lib.SrbdVmBatchIo(lin=d["ref_lin"].data_ptr(), ang=d["ref_ang"].data_ptr(), feet=d["feet"].data_ptr(),
                             hips=d["hips"].data_ptr(), max_distance=0.2, lin_out=lin.data_ptr(),
                             ang_out=ang.data_ptr())
    fio = _lib.SrbdFrgBatchIo(base_pos=d["base_pos"].data_ptr(), yaws=yaws.data_ptr(),
                              base_lin_vel=d["base_lin_vel"].data_ptr(), ref_lin_vel=lin.data_ptr(),
                              hips=d["hips"].data_ptr(), feet=d["feet"].data_ptr(), previous_contact=prev.data_ptr(),
                              current_contact=cur.data_ptr(), pgg=gait.state.data_ptr(), com_pos_offset_w=None,
                              com_height_nominal=CHN, gravity=GRAVITY, seeds=seeds.data_ptr(), ref=ref.data_ptr())
    tio = _lib.SrbdTerrainRefBatchIo(base_pos=d["base_pos"].data_ptr(), com_pos=d["com_pos"].data_ptr(),
                                     com_pos_offset_w=None, yaws=yaws.data_ptr(), lin=lin.data_ptr(),
                                     ang=ang.data_ptr(), feet=None, frg=frg.state.data_ptr(), ref_z=REF_Z,
                                     ref=ref.data_ptr(), terrain=None)
    L = _lib.lib
    pgg_p, frg_p, terr_p = gait.state.data_ptr(), frg.state.data_ptr(), terr.state.data_ptr()

    def bookkeeping():
        with torch.cuda.stream(stream):
            prev.copy_(cur)
            cur.copy_(contacts[:, :, 0])

    def c_chain():
        assert L.srbd_vm_modulate_device(E, C.byref(vio), handle) == 0
        assert L.srbd_pgg_run_device(pgg_p, E, SIM_DT, None, flags.data_ptr(), handle) == 0
        assert L.srbd_pgg_contact_sequence_device(pgg_p, E, H, _lib.dptr(dts), _lib.iptr(lens), 1, contacts.data_ptr(),
                                                  H, handle) == 0
        bookkeeping()
        assert L.srbd_frg_step_device(frg_p, E, C.byref(fio), handle) == 0
        assert L.srbd_terrain_ref_step_device(terr_p, E, C.byref(tio), handle) == 0
        assert L.srbd_stc_touch_down_device(edge.data_ptr(), E, cur.data_ptr(), prev.data_ptr(), contacts.data_ptr(),
                                            H, H, LOOKAHEAD, optimize.data_ptr(), handle) == 0

    def class_chain():
        vm.step(d["ref_lin"], d["ref_ang"], d["feet"], d["hips"], out=(lin, ang), stream=stream)
        gait.run(SIM_DT, stream=stream)
        gait.compute_contact_sequence(dts, lens, out=contacts, stream=stream)
        bookkeeping()
        frg.step(d["base_pos"], yaws, d["base_lin_vel"], lin, d["hips"], d["feet"], prev, cur, gait=gait, ref=ref,
                 out=seeds, stream=stream, com_height_nominal=CHN)
        terr.step(d["base_pos"], d["com_pos"], yaws, lin, ang, ref, frg=frg, stream=stream)
        _lib.stc_touch_down_device(edge, cur, prev, contacts, LOOKAHEAD, horizon=H, out=optimize, stream=stream)

    # (c), (d): the interface on a second set of state
    wb = BatchedWBInterface(E, *parts(), mpc_dt=MPC_DT, horizon=H, ref_z=REF_Z, com_height_nominal=CHN, gravity=GRAVITY,
                            lookahead=LOOKAHEAD, optimize_step_freq=True)
    wb.vm_activated = wb.start_and_stop_activated = True
    order = ("com_pos", "base_pos", "base_lin_vel", "euler", "base_ang_vel", "feet", "hips")
    wb.update_state_and_reference_device(*[d[k] for k in order], SIM_DT, d["ref_lin"], d["ref_ang"], stream=stream)
    io_ref, state_ptrs = wb._io_ref, wb._state_ptrs  # as the call above left them: every pointer set

    def c_fused():
        assert L.srbd_wb_update_device(*state_ptrs, E, io_ref, handle) == 0

    def class_fused():
        wb.update_state_and_reference_device(d["com_pos"], d["base_pos"], d["base_lin_vel"], d["euler"],
                                             d["base_ang_vel"], d["feet"], d["hips"], SIM_DT, d["ref_lin"],
                                             d["ref_ang"], stream=stream)

    def block(body, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        w0 = time.perf_counter()
        t0.record(stream)
        for _ in range(n):
            body()
        t1.record(stream)
        stream.synchronize()
        wall = (time.perf_counter() - w0) * 1e6 / n
        return wall, t0.elapsed_time(t1) * 1e3 / n  # us per step

    kinds = {"c_chain": c_chain, "class_chain": class_chain, "c_fused": c_fused, "class_fused": class_fused}
    for body in kinds.values():
        block(body, WARMUP)
    row = {"num_envs": E, "rounds": []}
    for _ in range(ROUNDS):
        s = {k: [] for k in kinds}
        for _ in range(BLOCKS):
            for k, body in kinds.items():
                s[k].append(block(body, STEPS))
        r = {}
        for k, v in s.items():
            r[k] = {"wall_us_per_step": round(float(np.median([b[0] for b in v])), 2),
                    "device_us_per_step": round(float(np.median([b[1] for b in v])), 2),
                    "wall_blocks": [round(b[0], 2) for b in v], "device_blocks": [round(b[1], 2) for b in v]}
        for num, den, name in (("c_fused", "c_chain", "c_fused_over_c_chain"),
                               ("class_fused", "class_chain", "class_fused_over_class_chain")):
            r[name] = {"wall": round(r[num]["wall_us_per_step"] / r[den]["wall_us_per_step"], 3),
                       "device": round(r[num]["device_us_per_step"] / r[den]["device_us_per_step"], 3)}
        row["rounds"].append(r)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git's HEAD of this checkout)")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("ROW " + json.dumps(measure(args.child)))
        return
    rows = []
    for E in args.envs:  # a fresh process per E, under its own time limit; a failure ends the run
        out = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__),
                              "--child", str(E)], capture_output=True, text=True)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"E = {E}: the child ended with status {out.returncode}; nothing more is started")
        rows.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("ROW ")][-1][4:]))
    try:
        commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                               capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (not a git checkout)"
    doc = {"workload": {"horizon": H, "lookahead": LOOKAHEAD, "stages": "vm, start_stop (fused only), touch_down",
                        "steps_per_block": STEPS},
           "device": rows[0].pop("device") if rows else None, "commit": commit, "warmup": WARMUP, "blocks": BLOCKS,
           "rounds": ROUNDS,
           "note": "one run on one box; wall: host clock from the first enqueue to the stream's synchronisation; "
                   "device: time between two events on the stream; per step, median of the round's blocks; the two "
                   "rounds show the run-to-run spread",
           "rows": rows}
    for r in rows:
        r.pop("device", None)
    print(f"{'E':>6} {'round':>5} {'c_chain':>16} {'class_chain':>16} {'c_fused':>16} {'class_fused':>16}   "
          "(wall / device us per step)")
    for r in rows:
        for i, rd in enumerate(r["rounds"]):
            cells = [f"{rd[k]['wall_us_per_step']:>7} /{rd[k]['device_us_per_step']:>7}"
                     for k in ("c_chain", "class_chain", "c_fused", "class_fused")]
            print(f"{r['num_envs']:>6} {i:>5} " + " ".join(cells))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
