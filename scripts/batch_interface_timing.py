#!/usr/bin/env python3
"""The batch's controller-interface step (srbd_batch_interface_step_device) against the same work made from the entry
points that existed before it -> profiles/batch_interface.json.

  new    one BatchContext.interface_step_device call per control step
  chain  contacts[:, :, 0] made contiguous, prepare_state_device, then per sampling iteration the key update (Philox: a
         torch op on the counters; the JAX stream: the keys fetched to the host, split there per environment and
         uploaded again -- the round trip splitting keys cost) and step_device / step_cem_device, then the float64
         mask and the contact copy as torch ops

Shapes: C2's (MPPI, zero-order, H 12, N = 10 000 per environment) at E = 1, 64, 1024 with 1 and 2 sampling iterations
on the Philox stream; the same at E = 64, 2 iterations on the JAX stream; the C3 CEM shape (cubic spline S 2, H 16,
N = 10 000 per environment) at E = 64, 2 iterations.

Device time between two events around CALLS back-to-back control steps, BLOCKS interleaved blocks per variant after
a warm-up; the median block with the smallest and largest is reported per variant.  Every point runs in a child
process of its own under a time limit, one after another; the first that fails or times out ends the run.  One box,
one run.

  python scripts/batch_interface_timing.py
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
OUT = os.path.join(ROOT, "profiles", "batch_interface.json")
BLOCKS, WARMUP = 7, 5
SIGMA_RESET = 3.0


def config(lib, shape):
    from quadruped_pympc_amd.synthetic import CONFIGS

    if shape == "c3":
        w = CONFIGS["c3"]
        return lib.make_config(num_samples=10000, horizon=16, method="cem_mppi", parametrization="cubic_spline",
                               num_splines=2, mass=w.mass, inertia=w.inertia, dts=np.full(16, w.dt, np.float32))
    w = CONFIGS["c2"]
    return lib.make_config(num_samples=10000, horizon=12, method="mppi", parametrization="zero_order", mass=w.mass,
                           inertia=w.inertia, dts=np.full(12, w.dt, np.float32))


def child(shape, E, iterations, rng):
    import torch

    from quadruped_pympc_amd import _lib as lib

    cfg = config(lib, shape)
    cem = shape == "c3"
    H = cfg.horizon
    calls = 20 if E <= 64 else 5
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

    def fresh():
        b = (lib.CemBatchContext if cem else lib.BatchContext)(cfg, E)
        if rng != "philox":
            b.set_rng(rng)
        keys = torch.tensor([[100 + e, 0] for e in range(E)], dtype=torch.int64, device=dev)
        if rng != "philox":
            keys[:, 0] = torch.tensor([lib.pack_key(lib.jax_prng_key(42 + e)) & 0x7FFFFFFFFFFFFFFF for e in range(E)])
        prev = torch.ones((E, 4), dtype=torch.float32, device=dev)
        best = torch.zeros((E, b.P), dtype=torch.float32, device=dev)
        sigma = torch.full((E, b.P), SIGMA_RESET, dtype=torch.float32, device=dev) if cem else None
        return b, keys, prev, best, sigma

    bn, kn, pn, bestn, sn = fresh()
    bc, kc, pc, bestc, sc = fresh()

    def new_step():
        return bn.interface_step_device(state_in, ref_in, contacts, kn, pn, bestn, iterations=iterations, sigma=sn,
                                        sigma_reset=SIGMA_RESET if cem else 0.0)["grf"]

    def chain_step():
        cur = contacts[:, :, 0].contiguous()
        states, refs = lib.prepare_state_device(state_in, ref_in, cur, pc, bc.P // 4, bestc)
        for it in range(iterations):
            if rng == "philox":
                kc[:, 1] += 1
            else:  # the host round trip: fetch, split per environment, upload
                h = kc.cpu().numpy().view(np.uint64)
                for e in range(E):
                    k = lib.jax_split(np.array([h[e, 0] >> np.uint64(32), h[e, 0] & np.uint64(0xFFFFFFFF)],
                                               np.uint32), 2, rng == "jax")[0]
                    h[e, 0] = lib.pack_key(k)
                h[:, 1] += np.uint64(1)
                kc.copy_(torch.from_numpy(h.view(np.int64)))
            seeds, counters = kc[:, 0].contiguous(), kc[:, 1].contiguous()
            if cem:
                out = bc.step_cem_device(states, refs, contacts, bestc, sc, seeds, counters,
                                         sigma_reset=SIGMA_RESET if it == 0 else 0.0)
            else:
                out = bc.step_device(states, refs, contacts, bestc, seeds, counters)
        grf = (out["grf"].double().view(E, 4, 3) * cur.double().unsqueeze(2)).view(E, 12)
        pc.copy_(cur)
        return grf

    def block(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / calls

    for fn in (new_step, chain_step):
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    new, chain = [], []
    for _ in range(BLOCKS):
        new.append(block(new_step))
        chain.append(block(chain_step))
    bn.close()
    bc.close()

    def stats(a):
        return {"median_us": float(np.median(a)), "min_us": float(np.min(a)), "max_us": float(np.max(a))}

    return {"shape": shape, "E": E, "iterations": iterations, "rng": rng, "calls_per_block": calls, "blocks": BLOCKS,
            "new": stats(new), "chain": stats(chain),
            "new_over_chain_median": float(np.median(new) / np.median(chain)),
            "new_slower_than_chain_spread": bool(np.median(new) > np.max(chain))}


PLAN = [("c2", 1, 1, "philox", 120), ("c2", 1, 2, "philox", 120), ("c2", 64, 1, "philox", 180),
        ("c2", 64, 2, "philox", 180), ("c2", 1024, 1, "philox", 300), ("c2", 1024, 2, "philox", 300),
        ("c2", 64, 2, "jax", 240), ("c3", 64, 2, "philox", 240)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("SHAPE", "E", "ITERATIONS", "RNG"))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        s, E, it, rng = args.child
        print("RESULT " + json.dumps(child(s, int(E), int(it), rng)), flush=True)
        return 0
    results = []
    for shape, E, it, rng, limit in PLAN:  # each under its own limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, str(E), str(it), rng],
                               timeout=limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(f"{shape} E={E} iterations={it} {rng}: no result within {limit} s; stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{shape} E={E} iterations={it} {rng}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            break
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"shapes": "c2: MPPI, zero-order, H 12, N = 10 000 per environment; c3: CEM-MPPI, cubic spline S 2, H 16, "
                     "N = 10 000 per environment; device draws",
           "method": f"device time between two events around calls_per_block back-to-back control steps, {BLOCKS} "
                     f"interleaved blocks per variant after {WARMUP} warm-up steps each; median, smallest and largest "
                     "block; one run on one box",
           "variants": "new: srbd_batch_interface_step_device; chain: prepare_state_device + key update (jax: through "
                       "the host) + step_device per iteration + torch mask and contact copy",
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return 0 if len(results) == len(PLAN) else 1


if __name__ == "__main__":
    sys.exit(main())
