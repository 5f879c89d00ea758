#!/usr/bin/env python3
"""The per-environment reset of the batched loop's device state (srbd_loop_reset_device) against the launch floor and
against what a caller could do without it -> profiles/batch_loop_reset.json.

For each E in {1, 1024, 4096}, in one process, device time between two events over 100 back-to-back calls on one
stream, BLOCKS blocks per kind, the kinds interleaved; median, minimum and maximum block are reported, in us per call:

  reset_L{1,2}_{0,1,100}   srbd_loop_reset_device on all five structs, the trigger words, the warm-start rows (P = 144)
                           and two contact tensors, with 0 %, 1 % (rounded, at least one environment for E >= 100) and
                           100 % of the mask words set to the level
  torch_L{1,2}             the same writes from torch, as a caller of the parent commit could make them without a host
                           wait: torch.where / masked_fill_ with the mask broadcast over each state tensor's views,
                           the warm start and the contact rows (a boolean-mask index would read the mask on the host).
                           Its cost does not depend on the share; its launches are counted from the op list.
  tiny_kernel              a one-element torch kernel, back to back: what a launch that does nothing costs here

A reset rewrites the same words whatever they hold, so the state needs no restoring between calls.  Every block is
enqueued behind a spinning kernel of a few milliseconds, recorded before the first event, so that the 100 calls wait
in the queue and run back to back: without it the rows measure how fast Python enqueues, not the device.

  python scripts/batch_loop_reset_timing.py [--envs 1 1024 4096] [--out profiles/batch_loop_reset.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "batch_loop_reset.json")
CALLS, WARMUP, BLOCKS = 100, 10, 7
P = 144
TORCH_LAUNCHES = {"torch_L1": 6, "torch_L2": 11}


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def measure(E, _lib, torch):
    from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
    from quadruped_pympc_amd.helpers.loop_reset import BatchedLoopReset
    from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
    from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController
    from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

    rng = np.random.default_rng(E)
    gait = BatchedPeriodicGaitGenerator(E, 0.65, 1.4, rng.integers(0, 7, E), 12)
    frg = BatchedFootholdReferenceGenerator(E, 0.46, 0.3, rng.uniform(-0.3, 0.3, (E, 4, 3)))
    stc = BatchedSwingTrajectoryController(E, 0.06, 0.25, 500.0, 10.0)
    terr = BatchedTerrainEstimator(E, ref_z=0.3)
    vfa = BatchedVisualFootholdAdaptation(E)
    vfa.state
    rst = BatchedLoopReset(E, gait=gait, frg=frg, stc=stc, terrain_est=terr, vfa=vfa)
    snap = rst.snapshots
    stream = torch.cuda.Stream()
    feet = torch.from_numpy(rng.uniform(-0.3, 0.3, (E, 4, 3))).cuda()
    best = torch.zeros((E, P), dtype=torch.float32, device="cuda")
    prev, prev_now = (torch.ones((E, 4), dtype=torch.float32, device="cuda") for _ in range(2))

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    t0, t1 = events()  # the spin kernel's rate, once: cycles for about 6 ms
    with torch.cuda.stream(stream):
        t0.record(stream)
        torch.cuda._sleep(1_000_000)
        t1.record(stream)
    stream.synchronize()
    spin = int(6.0 / max(t0.elapsed_time(t1), 1e-3) * 1_000_000)

    def timed(n, body):
        t0, t1 = events()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(spin)
        t0.record(stream)
        for _ in range(n):
            body()
        t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n  # us per call

    one = torch.zeros(1, device="cuda")

    def tiny():
        with torch.cuda.stream(stream):
            one.add_(1.0)

    kinds = {"tiny_kernel": tiny}
    row = {"num_envs": E, "reset_envs": {}}
    handle = C.c_void_p(stream.cuda_stream)
    keep = []
    for level in (1, 2):
        for share in (0, 1, 100):
            n = 0 if share == 0 else E if share == 100 else (max(1, round(0.01 * E)) if E >= 100 else 0)
            m = np.zeros(E, dtype=np.int32)
            m[rng.choice(E, n, replace=False)] = level
            mask = torch.from_numpy(m).cuda()
            io = _lib.SrbdLoopResetIo(mask=mask.data_ptr(), initial_feet=feet.data_ptr(),
                                      rising_edge=stc.rising_edge.data_ptr(), best_params=best.data_ptr(),
                                      num_params=P, n_contact_rows=2)
            io.contact_rows[0], io.contact_rows[1] = prev.data_ptr(), prev_now.data_ptr()
            for name, obj in (("pgg", gait), ("frg", frg), ("stc", stc), ("terrain_est", terr), ("vfa", vfa)):
                setattr(io, name, obj.state.data_ptr())
                setattr(io, name + "_snapshot", snap[name].data_ptr())
            keep.append((mask, io))

            def reset(io=io):
                rc = _lib.lib.srbd_loop_reset_device(E, C.byref(io), handle)
                assert rc == 0, rc

            name = f"reset_L{level}_{share}"
            kinds[name] = reset
            row["reset_envs"][name] = n
    # the torch comparator: the mask broadcast over views of the state tensors
    f64, i32 = torch.float64, torch.int32
    mb = torch.from_numpy(rng.uniform(size=E) < 0.01).cuda()
    m1 = mb[:, None]
    F = _lib.SrbdPgg
    pd, pi = gait.state.view(f64), gait.state.view(i32)
    ph = pd[:, F.phase_signal.offset // 8:F.phase_signal.offset // 8 + 4]
    off = pd[:, F.phase_offset.offset // 8:F.phase_offset.offset // 8 + 4]
    ini = pi[:, F.init.offset // 4:F.init.offset // 4 + 4]
    fd = frg.state.view(f64)
    lo = _lib.SrbdFrg.lift_off.offset // 8
    vi = vfa.state.view(i32)[:, :4]
    feet12 = feet.view(E, 12)
    frg_snap = snap["frg"].view(f64)
    zeros = torch.zeros((E, fd.shape[1] - 51), dtype=f64, device="cuda")

    def torch_l1():
        with torch.cuda.stream(stream):
            torch.where(m1, off, ph, out=ph)            # pgg.reset(): the offsets do not move between resets
            ini.masked_fill_(m1, 0)
            torch.where(m1, feet12, fd[:, lo:lo + 12], out=fd[:, lo:lo + 12])
            vi.masked_fill_(m1, 0)
            prev.masked_fill_(m1, 1.0)
            prev_now.masked_fill_(m1, 1.0)

    def torch_l2():
        with torch.cuda.stream(stream):
            for name, obj in (("pgg", gait), ("stc", stc), ("terrain_est", terr), ("vfa", vfa)):
                torch.where(m1, snap[name], obj.state, out=obj.state)
            fresh = torch.cat([frg_snap[:, :3], feet12.repeat(1, 4), zeros], dim=1)  # repeat, cat
            torch.where(m1, fresh, fd, out=fd)
            stc.rising_edge.masked_fill_(mb, 0)
            best.masked_fill_(m1, 0.0)
            prev.masked_fill_(m1, 1.0)
            prev_now.masked_fill_(m1, 1.0)
            # 4 + 3 + 4 = 11 kernels

    kinds["torch_L1"], kinds["torch_L2"] = torch_l1, torch_l2
    for body in kinds.values():
        timed(WARMUP, body)
    samples = {k: [] for k in kinds}
    for _ in range(BLOCKS):
        for k, body in kinds.items():
            samples[k].append(timed(CALLS, body))
    for k, v in samples.items():
        row[k] = stats(v)
    del keep
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]
    import torch  # torch first: one HIP runtime per process

    from quadruped_pympc_amd import _lib

    rows = [measure(E, _lib, torch) for E in args.envs]
    doc = {"device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "blocks": BLOCKS, "runs": 1,
           "num_params": P, "contact_rows": 2, "torch_launches": TORCH_LAUNCHES,
           "note": "one run on one box; device time between events over back-to-back calls, us per call; median, min "
                   "and max over the blocks, each block queued behind a spinning kernel so that the calls run back to "
                   "back; reset_L<level>_<share %>: srbd_loop_reset_device; torch_L<level>: torch.where / masked_fill_ "
                   "on the state tensors' views", "rows": rows}
    names = [k for k in rows[0] if k not in ("num_envs", "reset_envs")]
    print(f"{'E':>6} " + " ".join(f"{n:>14}" for n in names) + "  (us, median)")
    for r in rows:
        print(f"{r['num_envs']:>6} " + " ".join(f"{r[n]['median']:>14}" for n in names))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
