#!/usr/bin/env python3
"""Batched CEM-MPPI against sequential single-context CEM steps at the C3 shape (CEM, cubic spline S 2, H 16,
N = 10 000 per environment, Philox device draws) -> profiles/batch_cem.json.

For each E in {1, 4, 16, 64}, in one process: blocks of 100 srbd_batch_step_cem calls alternate with blocks of 100
rounds of E sequential srbd_step calls on E plain CEM contexts (what a caller without the batch does), so both see
the same machine state.  Times are host-to-host around the library calls, made through ctypes with pre-staged argument
addresses.  Inputs cycle over 8 pre-staged sets; the warm starts and sigmas are fed back; counters advance by one per
step.  The parent of this feature has no batched CEM, so the sequential rounds of the same build are the baseline.

The device form (srbd_batch_step_cem_device on torch tensors, N = 256) at E in {64, 1024}: the enqueue alone (the
host time of the call, the stream synchronised outside the timed span) and enqueue + synchronise.

  python scripts/batch_cem_timing.py                   # the tables
  python scripts/batch_cem_timing.py --one-shape 16    # 200 batch steps at E = 16 and nothing else: the run to put
                                                       # under `rocprofv3 --kernel-trace --stats`
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]

try:  # torch first: one HIP runtime per process
    import torch
except ImportError:
    torch = None

from quadruped_pympc_amd import _lib  # noqa: E402
from quadruped_pympc_amd.synthetic import CONFIGS, inputs  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_cem.json")
N_SETS, BLOCK, SIGMA0 = 8, 100, 3.0


def c3_config(N=None):
    w = CONFIGS["c3"]
    cfg = _lib.make_config(num_samples=N or 10000, horizon=16, method="cem_mppi", parametrization="cubic_spline",
                           num_splines=2, mass=w.mass, inertia=w.inertia, dts=np.full(16, w.dt, np.float32))
    return w, cfg


class Runner:
    """E environments: one CEM batch context and E plain CEM contexts over the same pre-staged inputs."""

    def __init__(self, E: int, sequential: bool = True, N=None):
        self.w, self.cfg = c3_config(N)
        self.E, self.P, self.H = E, _lib.num_params(self.cfg), self.cfg.horizon
        sets = [[inputs(self.w, s * E + e) for e in range(E)] for s in range(N_SETS)]
        self.states = np.ascontiguousarray([[x[0] for x in ss] for ss in sets], np.float32)      # (sets, E, 24)
        self.refs = np.ascontiguousarray([[x[1] for x in ss] for ss in sets], np.float32)
        self.contacts = np.ascontiguousarray([[x[2][:, :self.H] for x in ss] for ss in sets], np.float32)
        self.seeds = np.arange(100, 100 + E, dtype=np.uint64)
        self.counters = np.zeros(E, np.uint64)
        self.best_b, self.best_s = np.zeros((E, self.P), np.float32), np.zeros((E, self.P), np.float32)
        self.sig_b, self.sig_s = (np.full((E, self.P), SIGMA0, np.float32) for _ in range(2))
        self.res_b, self.res_s = (_lib.SrbdResult * E)(), (_lib.SrbdResult * E)()
        self.batch = _lib.CemBatchContext(self.cfg, E)
        self.ctxs = [_lib.Context(self.cfg) for _ in range(E)] if sequential else []
        self.k_b = self.k_s = 0

    def close(self):
        self.batch.close()
        for c in self.ctxs:
            c.close()

    def batch_steps(self, n: int) -> np.ndarray:
        fn, h = _lib.lib.srbd_batch_step_cem, self.batch.h
        a_best, a_sig = self.best_b.ctypes.data, self.sig_b.ctypes.data
        a_seeds, a_ctr, a_res = self.seeds.ctypes.data, self.counters.ctypes.data, C.addressof(self.res_b)
        lat = np.zeros(n)
        for i in range(n):
            s = self.k_b % N_SETS
            self.counters[:] = self.k_b
            a_st, a_rf, a_ct = self.states[s].ctypes.data, self.refs[s].ctypes.data, self.contacts[s].ctypes.data
            t0 = time.perf_counter_ns()
            rc = fn(h, a_st, a_rf, a_ct, self.H, a_best, a_sig, None, a_seeds, a_ctr, a_res, None)
            lat[i] = (time.perf_counter_ns() - t0) * 1e-3
            self.batch.check(rc, "srbd_batch_step_cem")
            self.k_b += 1
        return lat

    def sequential_rounds(self, n: int) -> np.ndarray:
        fn = _lib.lib.srbd_step
        hs = [c.h for c in self.ctxs]
        a_best = [self.best_s[e].ctypes.data for e in range(self.E)]
        a_sig = [self.sig_s[e].ctypes.data for e in range(self.E)]
        a_res = [C.byref(self.res_s[e]) for e in range(self.E)]
        seeds = [int(x) for x in self.seeds]
        lat = np.zeros(n)
        for i in range(n):
            s = self.k_s % N_SETS
            args = [(self.states[s, e].ctypes.data, self.refs[s, e].ctypes.data, self.contacts[s, e].ctypes.data)
                    for e in range(self.E)]
            t0 = time.perf_counter_ns()
            for e in range(self.E):
                rc = fn(hs[e], args[e][0], args[e][1], args[e][2], self.H, a_best[e], a_sig[e], None, seeds[e],
                        self.k_s, a_res[e], None)
                if rc:
                    self.ctxs[e].check(rc, "srbd_step")
            lat[i] = (time.perf_counter_ns() - t0) * 1e-3
            self.k_s += 1
        return lat


def pct(a, q):
    return round(float(np.percentile(a, q)), 2)


def measure(E: int, steps: int, warmup: int) -> dict:
    r = Runner(E)
    try:
        r.batch_steps(warmup)
        r.sequential_rounds(warmup)
        lb, ls = [], []
        for _ in range((steps + BLOCK - 1) // BLOCK):
            lb.append(r.batch_steps(BLOCK))
            ls.append(r.sequential_rounds(BLOCK))
        # the same inputs, keys and feedback: the same bits
        same = bool(np.array_equal(r.best_b, r.best_s) and np.array_equal(r.sig_b, r.sig_s))
    finally:
        r.close()
    lb, ls = np.concatenate(lb), np.concatenate(ls)
    return {"E": E, "steps": int(lb.size), "batch_p50_us": pct(lb, 50), "batch_p99_us": pct(lb, 99),
            "sequential_p50_us": pct(ls, 50), "sequential_p99_us": pct(ls, 99),
            "speedup_p50": round(pct(ls, 50) / pct(lb, 50), 2), "speedup_p99": round(pct(ls, 99) / pct(lb, 99), 2),
            "batch_us_per_env_p50": round(pct(lb, 50) / E, 2), "best_and_sigma_bit_equal": same}


def measure_device(E: int, steps: int, warmup: int, N: int = 256) -> dict:
    r = Runner(E, sequential=False, N=N)
    try:
        dev = torch.device("cuda", r.cfg.device_id)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        states, refs, contacts = t(r.states[0]), t(r.refs[0]), t(r.contacts[0])
        best, sigma = t(r.best_b), t(r.sig_b)
        seeds = t(r.seeds.view(np.int64))
        counters = torch.zeros(E, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream(dev)
        enq, synced = np.zeros(steps), np.zeros(steps)
        with torch.cuda.stream(stream):
            for i in range(-warmup, 2 * steps):
                counters.add_(1)
                stream.synchronize()
                t0 = time.perf_counter_ns()
                r.batch.step_cem_device(states, refs, contacts, best, sigma, seeds, counters, stream=stream)
                t1 = time.perf_counter_ns()
                stream.synchronize()
                t2 = time.perf_counter_ns()
                if 0 <= i < steps:
                    enq[i] = (t1 - t0) * 1e-3
                elif i >= steps:
                    synced[i - steps] = (t2 - t0) * 1e-3
    finally:
        r.close()
    return {"E": E, "N_per_env": N, "steps": steps, "enqueue_p50_us": pct(enq, 50), "enqueue_p99_us": pct(enq, 99),
            "synced_p50_us": pct(synced, 50), "synced_p99_us": pct(synced, 99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--device-envs", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--one-shape", type=int, default=0, metavar="E")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.one_shape:
        r = Runner(a.one_shape, sequential=False)
        try:
            lat = r.batch_steps(200)
        finally:
            r.close()
        print(json.dumps({"E": a.one_shape, "batch_p50_us": pct(lat, 50)}))
        return
    doc = {"workload": "c3 shape", "shape": {"N_per_env": 10000, "H": 16, "method": "cem_mppi",
                                             "parametrization": "cubic_spline", "S": 2, "rng": "philox"},
           "timing": "host-to-host around the library call (ctypes, pre-staged addresses); blocks of %d batch steps "
                     "alternate with blocks of %d rounds of E sequential srbd_step calls; one run on one machine"
                     % (BLOCK, BLOCK),
           "rows": [measure(E, a.steps, a.warmup) for E in a.envs]}
    if torch is not None and a.device_envs:
        doc["device_form"] = [measure_device(E, a.steps, a.warmup) for E in a.device_envs]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
