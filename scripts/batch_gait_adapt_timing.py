#!/usr/bin/env python3
"""One gait-adaptive loop step of E environments three ways -> profiles/batch_gait_adapt.json.

For each E in {1, 1024, 4096} (MPPI, zero-order, H = 12, N = 256 samples per environment), in one process:

  host_set  the only way before srbd_batch_set_gait_device: the generator's phases downloaded, the candidate sets
            formed on the host, BatchContext.set_gait (which synchronises and uploads E rows), then step_device
  wrappers  BatchContext.set_gait_device, step_device and _lib.apply_step_frequency (the write-back) on device tensors
  c_call    srbd_batch_set_gait_device, srbd_batch_step_device and srbd_gait_apply_freq_device through ctypes with
            prebuilt io structs

Each kind runs STEPS back-to-back loop steps after a warm-up and is timed as wall time from the first call to the
stream's synchronisation, per step, in us: for the two device kinds that is enqueue plus device time with nothing
waited for in between; the host kind waits inside every set_gait.  Each figure comes from one run; a second run of the
same kind gives the run-to-run spread beside it.  One run on one box.

  python scripts/batch_gait_adapt_timing.py [--envs 1 1024 4096] [--commit ID] [--out profiles/batch_gait_adapt.json]
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
from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator  # noqa: E402
from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController  # noqa: E402
from quadruped_pympc_amd.synthetic import CONFIGS, inputs  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_gait_adapt.json")
STEPS, WARMUP = 100, 10
N, H = 256, 12
AVAIL = np.array([1.4, 2.0, 2.4], np.float32)
PGG_DT, DUTY = 0.02, 0.65


def measure(E):
    w = CONFIGS["c2"]
    cfg = _lib.make_config(num_samples=N, horizon=H, method="mppi", parametrization="zero_order", mass=w.mass,
                           inertia=w.inertia, dts=np.full(H, 0.02, np.float32))
    ctx = _lib.BatchContext(cfg, E)
    state, ref, contact = inputs(w, 3)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()

    def rep(a, dtype):
        return torch.from_numpy(np.array(np.broadcast_to(np.asarray(a, dtype), (E,) + np.shape(a)))).to(dev)

    states, refs, contacts = rep(state, np.float32), rep(ref, np.float32), rep(contact[:, :H], np.float32)
    best = torch.zeros((E, ctx.P), dtype=torch.float32, device=dev)
    seeds = torch.arange(E, dtype=torch.int64, device=dev)
    counters = torch.zeros(E, dtype=torch.int64, device=dev)
    optimize = torch.ones(E, dtype=torch.int32, device=dev)
    gen = BatchedPeriodicGaitGenerator(E, DUTY, 1.3, 0, H)
    stc = BatchedSwingTrajectoryController(E, 0.06, 0.27, 500.0, 10.0)
    fsets = np.broadcast_to(AVAIL, (E, 3)).copy()

    def host_set():
        timings = gen.phase_signal.cpu().numpy().astype(np.float32)  # the download the device form removes
        ctx.set_gait(timings, PGG_DT, DUTY, fsets)
        return ctx.step_device(states, refs, contacts, best, seeds, counters, stream=stream)

    def wrappers():
        ctx.set_gait_device(optimize, AVAIL, PGG_DT, DUTY, pgg=gen.state, stream=stream)
        out = ctx.step_device(states, refs, contacts, best, seeds, counters, stream=stream)
        _lib.apply_step_frequency(optimize, out["best_freq"], gait=gen, stc=stc, stream=stream)

    with torch.cuda.stream(stream):
        o = {k: torch.empty(s, dtype=t, device=dev) for k, s, t in (
            ("grf", (E, 12), torch.float32), ("pred", (E, 24), torch.float32), ("cost", (E,), torch.float32),
            ("index", (E,), torch.int32), ("freq", (E,), torch.float32), ("status", (E,), torch.int32))}
    gio = _lib.BatchGaitIO(pgg=gen.state.data_ptr(), timings=None, nominal_freqs=None, optimize=optimize.data_ptr(),
                           freq_rows=None, available=(C.c_float * _lib.MAX_FREQS)(*AVAIL.tolist()), n_freq=3,
                           pgg_dt=PGG_DT, duty_factor=DUTY, pad=0)
    sio = _lib.BatchDeviceIO(states=states.data_ptr(), refs=refs.data_ptr(), contacts=contacts.data_ptr(), noise=None,
                             seeds=seeds.data_ptr(), counters=counters.data_ptr(), contact_stride=H, pad=0,
                             best_params=best.data_ptr(), grf=o["grf"].data_ptr(),
                             predicted_state=o["pred"].data_ptr(), best_cost=o["cost"].data_ptr(),
                             best_index=o["index"].data_ptr(), best_freq=o["freq"].data_ptr(),
                             status=o["status"].data_ptr(), costs=None)
    handle = C.c_void_p(stream.cuda_stream)
    set_c, step_c, apply_c = (_lib.lib.srbd_batch_set_gait_device, _lib.lib.srbd_batch_step_device,
                              _lib.lib.srbd_gait_apply_freq_device)
    pgg_p, stc_p, opt_p, freq_p = gen.state.data_ptr(), stc.state.data_ptr(), optimize.data_ptr(), o["freq"].data_ptr()

    def c_call():
        assert set_c(ctx.h, C.byref(gio), handle) == 0 and step_c(ctx.h, C.byref(sio), handle) == 0
        assert apply_c(pgg_p, None, stc_p, E, opt_p, freq_p, handle) == 0

    def run(body, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            body()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n  # us per loop step

    row = {"num_envs": E}
    for name, body in (("host_set", host_set), ("wrappers", wrappers), ("c_call", c_call)):
        run(body, WARMUP)
        first, second = run(body, STEPS), run(body, STEPS)
        row[name] = {"us_per_step": round(first, 1), "second_run": round(second, 1),
                     "spread": round(abs(second - first), 1)}
    row["host_set_over_c_call"] = round(row["host_set"]["us_per_step"] / row["c_call"]["us_per_step"], 2)
    ctx.close()
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
    doc = {"workload": {"method": "mppi", "parametrization": "zero_order", "horizon": H, "num_samples": N,
                        "phases_from": "generator state", "launches_per_step": {"set_gait_device": 1, "step": 5,
                                                                                  "write_back": 1}},
           "device": torch.cuda.get_device_name(0), "commit": commit, "steps": STEPS, "warmup": WARMUP,
           "note": "one run on one box; wall time per loop step from the first call to the stream's synchronisation "
                   "over back-to-back steps; us_per_step is the first run, second_run a repeat, spread their difference",
           "rows": rows}
    print(f"{'E':>6} {'host_set':>16} {'wrappers':>16} {'c_call':>16}   (us per loop step, +- second run)")
    for r in rows:
        print(f"{r['num_envs']:>6} " + " ".join(f"{r[k]['us_per_step']:>9} +-{r[k]['spread']:>5}"
                                                for k in ("host_set", "wrappers", "c_call")))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
