#!/usr/bin/env python3
"""The foothold reference generator of E environments two ways -> profiles/batch_frg.json.

For each E in {1024, 4096}, in one process, blocks alternate between

  device   srbd_frg_step_device: 200 back-to-back launches between two events on one stream
  host     E x (srbd_frg_update_lift_off, srbd_frg_update_touch_down, srbd_frg_compute) through ctypes, the
           argument pointers built before the clock starts: what a loop that keeps the generators on the host pays
           per step, before its E x 12 doubles are copied up

after a warm-up of each.  The device kind is device time (events, so the launch overhead of back-to-back calls is
inside it); the host kind is wall time.  Three blocks per kind; the median block is reported, per step and per
environment, in us.  One run on one box.

  python scripts/batch_frg_timing.py [--envs 1024 4096] [--commit ID] [--out profiles/batch_frg.json]
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
from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_frg.json")
LAUNCHES, WARMUP, BLOCKS, HOST_STEPS = 200, 20, 3, 5
CHN, GRAVITY = 0.3, 9.81


def inputs(E):
    rng = np.random.default_rng(E)
    rows = (np.arange(E)[:, None] + np.arange(4)[None, :]) % 4
    return dict(base_pos=rng.uniform(-2, 2, (E, 3)), yaws=rng.uniform(-3.0, 3.0, E),
                base_lin_vel=rng.standard_normal((E, 3)) * 0.3, ref_lin_vel=rng.standard_normal((E, 3)) * 0.3,
                hips=rng.uniform(-2, 2, (E, 4, 3)), feet=rng.uniform(-2, 2, (E, 4, 3)),
                prev=(rows < 2).astype(np.float32), cur=((rows + 1) % 4 < 2).astype(np.float32))


def measure(E):
    x = inputs(E)
    stance, height, lift = np.full(E, 0.45), np.full(E, 0.3), x["feet"]
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    gen.gravity_constant = GRAVITY
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    stream = torch.cuda.Stream()
    seeds = torch.empty((E, 4, 3), dtype=torch.float64, device="cuda")
    ref = torch.zeros((E, 24), dtype=torch.float64, device="cuda")

    def device(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(n):
            gen.step(d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"],
                     d["cur"], ref=ref, out=seeds, stream=stream, com_height_nominal=CHN)
        t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n  # us per launch

    host = (_lib.SrbdFrg * E)()
    for e in range(E):
        assert _lib.lib.srbd_frg_init(C.byref(host[e]), 0.45, 0.3, _lib.dptr(np.ascontiguousarray(lift[e]))) == 0
    prev, cur = x["prev"].astype(np.float64), x["cur"].astype(np.float64)
    vel, rvel = np.ascontiguousarray(x["base_lin_vel"][:, :2]), np.ascontiguousarray(x["ref_lin_vel"][:, :2])
    out = np.zeros((E, 4, 3))
    p = _lib.dptr
    args = [(C.byref(host[e]), p(prev[e]), p(cur[e]), p(x["feet"][e]), p(x["base_pos"][e]), float(x["yaws"][e]),
             p(vel[e]), p(rvel[e]), p(x["hips"][e]), p(out[e])) for e in range(E)]
    lo, td, comp = _lib.lib.srbd_frg_update_lift_off, _lib.lib.srbd_frg_update_touch_down, _lib.lib.srbd_frg_compute

    def host_loop(n):
        t0 = time.perf_counter()
        for _ in range(n):
            for g, pv, cu, ft, bp, yaw, v, rv, hp, o in args:
                lo(g, pv, cu, ft, 0, bp, yaw)
                td(g, pv, cu, ft, 0, bp, yaw)
                comp(g, bp, yaw, v, rv, hp, CHN, GRAVITY, None, o)
        return (time.perf_counter() - t0) * 1e6 / n  # us per step of E environments

    device(WARMUP), host_loop(1)
    s = dict(device=[], host=[])
    for _ in range(BLOCKS):
        s["device"].append(device(LAUNCHES))
        s["host"].append(host_loop(HOST_STEPS))
    row = {"num_envs": E}
    for k, v in s.items():
        m = float(np.median(v))
        row[k] = {"us_per_step": round(m, 2), "us_per_env": round(m / E, 4), "blocks": [round(b, 2) for b in v]}
    row["host_over_device"] = round(row["host"]["us_per_step"] / row["device"]["us_per_step"], 1)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git's HEAD of this checkout)")
    args = ap.parse_args()
    rows = [measure(E) for E in args.envs]
    try:
        commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                               capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown (not a git checkout)"
    doc = {"workload": {"com_height_nominal": CHN, "gravity": GRAVITY, "ref_written": True},
           "device": torch.cuda.get_device_name(0), "commit": commit, "launches": LAUNCHES, "warmup": WARMUP,
           "blocks": BLOCKS, "host_steps": HOST_STEPS,
           "note": "one run on one box; device: device time between events over back-to-back launches; host: wall "
                   "time of E x 3 ctypes calls with prebuilt argument pointers",
           "rows": rows}
    print(f"{'E':>6} {'device/step':>12} {'host/step':>11} {'ratio':>8}   (us)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['device']['us_per_step']:>12} {r['host']['us_per_step']:>11} "
              f"{r['host_over_device']:>8}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
