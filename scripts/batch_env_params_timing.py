#!/usr/bin/env python3
"""Per-environment robot parameters in a batch (srbd_batch_set_env_params) at the C2 shape (MPPI, zero-order, H 12,
N = 10 000 per environment, Philox device draws) -> profiles/batch_env_params.json.

  hetero E   a batch with per-environment parameters against the same build's homogeneous batch: alternating blocks
             of 100 srbd_batch_step calls, host-to-host p50 over 1 000 steps each after 50 warm-up steps
  seq E      the same heterogeneous batch against E plain contexts created with their own configurations and stepped
             one after another (the only way to get these results without the feature), alternating blocks
  setter     srbd_batch_set_env_params_device at E = 1, 1024, 4096, mask all / mask none: device time between two
             events around 200 calls

Every measurement runs in a child process of its own under a time limit, one after another; the first that fails or
times out ends the run.  Times are made through ctypes with pre-staged argument addresses; the warm starts are fed
back and the counters advance by one per step.

  python scripts/batch_env_params_timing.py
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
OUT = os.path.join(ROOT, "profiles", "batch_env_params.json")
BLOCK, STEPS, WARMUP = 100, 1000, 50


def c2_config(lib, N=10000):
    from quadruped_pympc_amd.synthetic import CONFIGS

    w = CONFIGS["c2"]
    return w, lib.make_config(num_samples=N, horizon=12, method="mppi", parametrization="zero_order", mass=w.mass,
                              inertia=w.inertia, dts=np.full(12, w.dt, np.float32))


def robots(lib, cfg, w, E):
    """Payload, friction, inertia and force-limit randomisation, one draw per environment."""
    r = np.random.default_rng(0)
    scale = r.uniform(0.8, 1.2, E)
    inertia = np.asarray(w.inertia, np.float64).reshape(1, 9) * scale[:, None]
    return lib.make_env_params(E, cfg, mass=w.mass * r.uniform(0.7, 1.3, E), inertia=inertia,
                               mu=r.uniform(0.5, 1.0, E), grf_min=r.choice([0.0, 5.0], E))


def stage(lib, b, w, E):
    from quadruped_pympc_amd.synthetic import inputs

    H = b.cfg.horizon
    for e in range(E):
        s, r, c = inputs(w, e)
        b._states[e], b._refs[e], b._contacts[e] = s, r, c[:, :H]
    b._seeds[...] = 100 + np.arange(E)
    b._counters[...] = 0


def batch_block(lib, b, n):
    a, H, lat = b._addr, b.cfg.horizon, np.empty(n)
    res = C.addressof(b._results)
    for i in range(n):
        b._counters += 1
        t0 = time.perf_counter()
        rc = lib.lib.srbd_batch_step(b.h, a[0], a[1], a[2], H, a[3], None, a[4], a[5], res, None)
        lat[i] = time.perf_counter() - t0
        if rc:
            b.check(rc, "srbd_batch_step")
    return lat * 1e6


def seq_block(lib, ctxs, b, bests, n):
    """n rounds of E sequential srbd_step calls over the batch's staged inputs."""
    E, lat = len(ctxs), np.empty(n)
    st, rf, ct = b._states, b._refs, b._contacts
    for i in range(n):
        ctr = int(b._counters[0]) + 1 + i
        t0 = time.perf_counter()
        for e in range(E):
            bests[e] = ctxs[e].step(st[e], rf[e], ct[e], bests[e], seed=100 + e, counter=ctr)[0]
        lat[i] = time.perf_counter() - t0
    return lat * 1e6


def stats(a):
    return {"p50_us": float(np.percentile(a, 50)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "n": int(a.size)}


def child_hetero(E):
    from quadruped_pympc_amd import _lib as lib

    w, cfg = c2_config(lib)
    homo, het = lib.BatchContext(cfg, E), lib.BatchContext(cfg, E)
    het.set_env_params(robots(lib, cfg, w, E))
    for b in (homo, het):
        stage(lib, b, w, E)
        batch_block(lib, b, WARMUP)
    a, h = [], []
    for _ in range(STEPS // BLOCK):
        a.append(batch_block(lib, homo, BLOCK))
        h.append(batch_block(lib, het, BLOCK))
    a, h = np.concatenate(a), np.concatenate(h)
    homo.close()
    het.close()
    return {"kind": "hetero", "E": E, "homogeneous": stats(a), "per_environment": stats(h),
            "ratio_p50": float(np.percentile(h, 50) / np.percentile(a, 50))}


def child_seq(E):
    from quadruped_pympc_amd import _lib as lib

    w, cfg = c2_config(lib)
    p = robots(lib, cfg, w, E)
    het = lib.BatchContext(cfg, E)
    het.set_env_params(p)
    stage(lib, het, w, E)
    ctxs = [lib.Context(lib.config_with_env_params(cfg, p[e])) for e in range(E)]
    bests = [np.zeros(het.P, np.float32) for _ in range(E)]
    rounds = max(BLOCK, min(STEPS, 20000 // E))  # E sequential steps per round: fewer rounds at large E
    batch_block(lib, het, WARMUP)
    seq_block(lib, ctxs, het, bests, max(2, WARMUP // 5))
    b, s = [], []
    for _ in range(rounds // BLOCK):
        b.append(batch_block(lib, het, BLOCK))
        s.append(seq_block(lib, ctxs, het, bests, BLOCK))
    b, s = np.concatenate(b), np.concatenate(s)
    het.close()
    for c in ctxs:
        c.close()
    return {"kind": "seq", "E": E, "batch_per_environment": stats(b), "sequential_contexts": stats(s),
            "speedup_p50": float(np.percentile(s, 50) / np.percentile(b, 50))}


def child_setter(E):
    import torch

    from quadruped_pympc_amd import _lib as lib

    w, cfg = c2_config(lib, N=64)
    b = lib.BatchContext(cfg, E)
    p = torch.from_numpy(robots(lib, cfg, w, E).view(np.float32).reshape(E, -1).copy()).cuda()
    rej = torch.zeros(E, dtype=torch.int32, device="cuda")
    out = {"kind": "setter", "E": E}
    for name, mask in (("mask_all", torch.ones(E, dtype=torch.int32, device="cuda")),
                       ("mask_none", torch.zeros(E, dtype=torch.int32, device="cuda"))):
        for _ in range(20):
            b.set_env_params_device(p, mask=mask, rejected=rej)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(200):
            b.set_env_params_device(p, mask=mask, rejected=rej)
        t1.record()
        torch.cuda.synchronize()
        out[name + "_us_per_call"] = t0.elapsed_time(t1) * 1e3 / 200
    b.close()
    return out


CHILDREN = {"hetero": child_hetero, "seq": child_seq, "setter": child_setter}
PLAN = [("hetero", 16, 240), ("hetero", 64, 300), ("hetero", 1024, 600), ("seq", 16, 300), ("seq", 64, 420),
        ("setter", 1, 120), ("setter", 1024, 120), ("setter", 4096, 120)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("KIND", "E"))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(CHILDREN[args.child[0]](int(args.child[1]))), flush=True)
        return 0
    results = []
    for kind, E, limit in PLAN:  # each under its own limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(E)], timeout=limit,
                               capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"{kind} E={E}: no result within {limit} s; stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{kind} E={E}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"shape": "C2: MPPI, zero-order, H 12, N = 10 000 per environment, Philox device draws (setter: N = 64)",
           "method": f"host-to-host p50 over alternating blocks of {BLOCK} steps after {WARMUP} warm-up steps; "
                     "one run on one box", "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0 if len(results) == len(PLAN) else 1


if __name__ == "__main__":
    sys.exit(main())
