#!/usr/bin/env python3
"""The due mask of the batch's controller-interface step (srbd_batch_interface_step_masked_device) against the
unmasked call -> profiles/batch_due.json.

  a  the unmasked srbd_batch_interface_step_device (the parent commit's code: the same kernels, their mask NULL)
  b  the masked call, every environment due
  c  the masked call, one environment in five due, staggered: environment e is due on the calls with
     (call + e) % 5 == 0, the reference's 100 Hz MPC in a 500 Hz loop after per-environment resets
  d  the masked call, no environment due

Shape: batch_interface_timing.py's C2 point (MPPI, zero-order, H 12, N = 10 000 per environment, device draws on the
Philox stream, one sampling iteration) at E = 64 and E = 1024.

Device time of every single call, between two events recorded around it on the stream.  After a warm-up of every
variant, ROUNDS rounds; a round times CALLS back-to-back calls of a, b, c, d and a again, in that order, so the
variants alternate and (a) is measured twice per round.  Per variant p50 and p99 over all its calls.  The margin for
(b) is the spread (a) shows against itself: the largest distance between the per-round medians of its two series.
Every point runs in a child process of its own under a time limit, one after another; the first that fails or times
out ends the run.  One box, one run.

  python scripts/batch_due_timing.py
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]
OUT = os.path.join(ROOT, "profiles", "batch_due.json")
ROUNDS, WARMUP, PERIOD = 6, 10, 5


def child(E):
    import torch

    from quadruped_pympc_amd import _lib as lib
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import mpc_due
    from quadruped_pympc_amd.synthetic import CONFIGS

    w = CONFIGS["c2"]
    H = 12
    cfg = lib.make_config(num_samples=10000, horizon=H, method="mppi", parametrization="zero_order", mass=w.mass,
                          inertia=w.inertia, dts=np.full(H, w.dt, np.float32))
    calls = 40 if E <= 64 else 10
    g = np.random.default_rng(0)
    feet = np.array([0.19, 0.14, 0.0, 0.19, -0.14, 0.0, -0.19, 0.14, 0.0, -0.19, -0.14, 0.0])
    st = np.zeros((E, 24))
    st[:, 2] = 0.3
    st[:, 12:] = feet + 0.01 * g.standard_normal((E, 12))
    rf = st.copy()
    rf[:, 3] = 0.4
    ct = np.ones((E, 4, H), np.float32)
    ct[:, 1, :H // 2] = 0.0
    ct[:, 2, :H // 2] = 0.0
    dev = torch.device("cuda", 0)
    state_in, ref_in, contacts = (torch.from_numpy(a).to(dev) for a in (st, rf, ct))
    b = lib.BatchContext(cfg, E)
    keys = torch.tensor([[100 + e, 0] for e in range(E)], dtype=torch.int64, device=dev)
    prev = torch.ones((E, 4), dtype=torch.float32, device=dev)
    best = torch.zeros((E, b.P), dtype=torch.float32, device=dev)
    phase = torch.arange(E, dtype=torch.int64, device=dev) % PERIOD
    # the masks, made ahead of the timed calls: all, none, and the five of the staggered schedule (500 Hz loop,
    # 100 Hz MPC)
    every = torch.ones(E, dtype=torch.int32, device=dev)
    none = torch.zeros(E, dtype=torch.int32, device=dev)
    staggered = [mpc_due(phase + k, 0.002, 100.0) for k in range(PERIOD)]
    due_share = float(np.mean([m.sum().item() / E for m in staggered]))
    held = {}
    tick = [0]

    def masked(due):
        held["out"] = b.interface_step_masked_device(state_in, ref_in, contacts, keys, prev, best, due,
                                                     out=held.get("out"), iterations=1)

    def a():
        b.interface_step_device(state_in, ref_in, contacts, keys, prev, best, iterations=1)

    def c():
        masked(staggered[tick[0] % PERIOD])
        tick[0] += 1

    variants = {"a": a, "b": lambda: masked(every), "c": c, "d": lambda: masked(none)}

    def series(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * calls)]
        for i in range(calls):
            ev[2 * i].record()
            fn()
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        return [ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(calls)]

    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    order = ("a", "b", "c", "d", "a2")
    rounds = {k: [] for k in order}
    for _ in range(ROUNDS):
        for k in order:
            rounds[k].append(series(variants[k[0]]))
    b.close()

    def stats(per_round):
        flat = np.concatenate(per_round)
        return {"p50_us": float(np.percentile(flat, 50)), "p99_us": float(np.percentile(flat, 99)),
                "round_medians_us": [float(np.median(r)) for r in per_round], "calls": int(flat.size)}

    res = {k: stats(v) for k, v in rounds.items()}
    a_all = stats(rounds["a"] + rounds["a2"])
    meds = res["a"]["round_medians_us"] + res["a2"]["round_medians_us"]
    margin = float(max(meds) - min(meds))
    doc = {"E": E, "calls_per_series": calls, "rounds": ROUNDS, "due_share_c": due_share, "a": a_all,
           "a_first_series": res["a"], "a_second_series": res["a2"], "a_spread_us": margin, "b": res["b"],
           "c": res["c"], "d": res["d"],
           "b_minus_a_p50_us": res["b"]["p50_us"] - a_all["p50_us"],
           "b_within_a_spread": bool(abs(res["b"]["p50_us"] - a_all["p50_us"]) <= margin),
           "c_over_a_p50": res["c"]["p50_us"] / a_all["p50_us"], "d_over_a_p50": res["d"]["p50_us"] / a_all["p50_us"]}
    return doc


PLAN = [(64, 240), (1024, 420)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="E")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(child(int(args.child))), flush=True)
        return 0
    results = []
    for E, limit in PLAN:  # each under its own limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(E)], timeout=limit,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"E={E}: no result within {limit} s; stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"E={E}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"shape": "C2: MPPI, zero-order, H 12, N = 10 000 per environment, device draws (Philox), one sampling "
                    "iteration",
           "method": f"device time of each call between two events around it; {WARMUP} warm-up calls per variant, then "
                     f"{ROUNDS} rounds of calls_per_series back-to-back calls of a, b, c, d, a; p50 and p99 over a "
                     "variant's calls; a_spread_us: the largest distance between the per-round medians of (a)'s two "
                     "series; one run on one box",
           "variants": "a: srbd_batch_interface_step_device; b: srbd_batch_interface_step_masked_device, every "
                       "environment due; c: one in five due, environment e on the calls with (call + e) % 5 == 0; "
                       "d: none due",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0 if len(results) == len(PLAN) else 1


if __name__ == "__main__":
    sys.exit(main())
