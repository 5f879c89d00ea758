#!/usr/bin/env python3
"""Batched environments against sequential single-context steps at the C2 shape (Go2 trot, MPPI zero-order,
N = 10 000 per environment, H = 12, Philox device draws) -> profiles/batch_c2.json.

For each E in {1, 4, 16, 64}, in one process: blocks of 100 srbd_batch_step calls alternate with blocks of 100
rounds of E sequential srbd_step calls on E plain contexts (the path a caller without the batch takes), so both see
the same machine state.  Times are host-to-host around the library calls, made through ctypes with pre-staged
argument addresses (about 1 us of binding cost per call on either side, so a sequential round carries E of them).
Inputs cycle over 8 pre-staged sets; the warm starts are fed back; counters advance by one per step.

  python scripts/bench_batch.py                      # the table
  python scripts/bench_batch.py --gait               # the same comparison with gait-adaptive sampling on both
                                                     # sides (srbd_batch_set_gait / srbd_set_gait, device-drawn
                                                     # frequencies) -> profiles/batch_ga_c2.json
  python scripts/bench_batch.py --cost-terms         # ... with the opt-in cost terms on both sides
                                                     # -> profiles/batch_ext_c2.json
  python scripts/bench_batch.py --one-shape 16       # 200 batch steps at E = 16 and nothing else: the run to put
                                                     # under `rocprofv3 --kernel-trace --stats` (with --gait or
                                                     # --cost-terms: that feature's kernels)
  python scripts/bench_batch.py --kernel-stats run_kernel_stats.csv   # add that run's kernel rows and the rollout
                                                                      # launch's roofline fraction to the JSON
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]

try:  # torch first: one HIP runtime per process
    import torch  # noqa: F401
except ImportError:
    pass

from quadruped_pympc_amd import _lib  # noqa: E402
from quadruped_pympc_amd.synthetic import CONFIGS, inputs  # noqa: E402

OUT = {None: os.path.join(ROOT, "profiles", "batch_c2.json"), "gait": os.path.join(ROOT, "profiles", "batch_ga_c2.json"),
       "cost_terms": os.path.join(ROOT, "profiles", "batch_ext_c2.json")}
# the settings of the feature runs: the leg phases, candidate set and weights the GPU tests use
GA_TIMINGS = [(0.1, 0.6, 0.6, 0.1), (0.0, 0.5, 0.5, 0.0), (0.64, 0.99, 1.0, 0.3)]
GA_FREQS, GA_DUTY = (1.4, 2.0, 2.4), 0.65
COST_TERMS = {"r_force": (0.1, 0.1, 0.001), "w_smooth": 0.01, "w_cone": 5.0}
HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak
N_SETS, BLOCK = 8, 100


def c2_config():
    w = CONFIGS["c2"]
    cfg = _lib.make_config(num_samples=w.num_samples, horizon=w.horizon, method=w.method,
                           parametrization=w.parametrization, mass=w.mass, inertia=w.inertia,
                           dts=np.full(w.horizon, w.dt, np.float32))
    return w, cfg


class Runner:
    """E environments: one batch context and E plain contexts over the same pre-staged inputs."""

    def __init__(self, E: int, sequential: bool = True, feature: str | None = None):
        self.w, self.cfg = c2_config()
        self.E, self.P, self.H = E, _lib.num_params(self.cfg), self.cfg.horizon
        sets = [[inputs(self.w, s * E + e) for e in range(E)] for s in range(N_SETS)]
        self.states = np.ascontiguousarray([[x[0] for x in ss] for ss in sets], np.float32)      # (sets, E, 24)
        self.refs = np.ascontiguousarray([[x[1] for x in ss] for ss in sets], np.float32)
        self.contacts = np.ascontiguousarray([[x[2][:, :self.H] for x in ss] for ss in sets], np.float32)
        self.seeds = np.arange(100, 100 + E, dtype=np.uint64)
        self.counters = np.zeros(E, np.uint64)
        self.best_b = np.zeros((E, self.P), np.float32)
        self.best_s = np.zeros((E, self.P), np.float32)
        self.res_b = (_lib.SrbdResult * E)()
        self.res_s = (_lib.SrbdResult * E)()
        self.batch = _lib.BatchContext(self.cfg, E)
        self.ctxs = [_lib.Context(self.cfg) for _ in range(E)] if sequential else []
        self.k_b = self.k_s = 0
        if feature == "gait":  # the same setting on both sides, once: it holds until changed
            t = np.array([GA_TIMINGS[e % len(GA_TIMINGS)] for e in range(E)], np.float32)
            fs = np.tile(np.array(GA_FREQS, np.float32), (E, 1))
            self.batch.set_gait(t, self.w.dt, GA_DUTY, fs)
            for e, c in enumerate(self.ctxs):
                c.set_gait(t[e], self.w.dt, GA_DUTY, fs[e])
        elif feature == "cost_terms":
            for c in [self.batch] + self.ctxs:
                c.set_cost_terms(COST_TERMS["r_force"], COST_TERMS["w_smooth"], COST_TERMS["w_cone"])

    def close(self):
        self.batch.close()
        for c in self.ctxs:
            c.close()

    def batch_steps(self, n: int) -> np.ndarray:
        fn, h = _lib.lib.srbd_batch_step, self.batch.h
        a_best, a_seeds, a_ctr = self.best_b.ctypes.data, self.seeds.ctypes.data, self.counters.ctypes.data
        a_res = C.addressof(self.res_b)
        lat = np.zeros(n)
        for i in range(n):
            s = self.k_b % N_SETS
            self.counters[:] = self.k_b
            a_st, a_rf, a_ct = self.states[s].ctypes.data, self.refs[s].ctypes.data, self.contacts[s].ctypes.data
            t0 = time.perf_counter_ns()
            rc = fn(h, a_st, a_rf, a_ct, self.H, a_best, None, a_seeds, a_ctr, a_res, None)
            lat[i] = (time.perf_counter_ns() - t0) * 1e-3
            self.batch.check(rc, "srbd_batch_step")
            self.k_b += 1
        return lat

    def sequential_rounds(self, n: int) -> np.ndarray:
        fn = _lib.lib.srbd_step
        hs = [c.h for c in self.ctxs]
        a_best = [self.best_s[e].ctypes.data for e in range(self.E)]
        a_res = [C.byref(self.res_s[e]) for e in range(self.E)]
        seeds = [int(x) for x in self.seeds]
        lat = np.zeros(n)
        for i in range(n):
            s = self.k_s % N_SETS
            args = [(self.states[s, e].ctypes.data, self.refs[s, e].ctypes.data, self.contacts[s, e].ctypes.data)
                    for e in range(self.E)]
            t0 = time.perf_counter_ns()
            for e in range(self.E):
                rc = fn(hs[e], args[e][0], args[e][1], args[e][2], self.H, a_best[e], None, None, seeds[e], self.k_s,
                        a_res[e], None)
                if rc:
                    self.ctxs[e].check(rc, "srbd_step")
            lat[i] = (time.perf_counter_ns() - t0) * 1e-3
            self.k_s += 1
        return lat


def measure(E: int, steps: int, warmup: int, feature: str | None = None) -> dict:
    r = Runner(E, feature=feature)
    try:
        r.batch_steps(warmup)
        r.sequential_rounds(warmup)
        lb, ls = [], []
        for _ in range((steps + BLOCK - 1) // BLOCK):
            lb.append(r.batch_steps(BLOCK))
            ls.append(r.sequential_rounds(BLOCK))
        same = bool(np.array_equal(r.best_b, r.best_s))  # the same inputs, keys and feedback: the same bits
    finally:
        r.close()
    lb, ls = np.concatenate(lb), np.concatenate(ls)
    pct = lambda a, q: round(float(np.percentile(a, q)), 2)  # noqa: E731
    return {"E": E, "steps": int(lb.size), "batch_p50_us": pct(lb, 50), "batch_p99_us": pct(lb, 99),
            "sequential_p50_us": pct(ls, 50), "sequential_p99_us": pct(ls, 99),
            "speedup_p50": round(pct(ls, 50) / pct(lb, 50), 2), "batch_us_per_env_p50": round(pct(lb, 50) / E, 2),
            "warm_starts_bit_equal": same}


def kernel_rows(path: str, E: int, feature: str | None = None) -> dict:
    w, cfg = c2_config()
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "srbd::batch_" in row["Name"]:
                rows.append({"kernel": row["Name"].split("(")[0].replace("void ", ""), "calls": int(row["Calls"]),
                             "avg_us": round(float(row["AverageNs"]) * 1e-3, 3),
                             "min_us": round(float(row["MinNs"]) * 1e-3, 3),
                             "max_us": round(float(row["MaxNs"]) * 1e-3, 3)})
    flag = {None: "", "gait": "--gait ", "cost_terms": "--cost-terms "}[feature]
    out = {"E": E, "source": "rocprofv3 --kernel-trace --stats of `bench_batch.py %s--one-shape %d`" % (flag, E),
           "kernels": rows}
    roll = [r for r in rows if "batch_rollout_" in r["kernel"]]
    if roll:  # bench.py's roofline: each noise row read once + one cost written, per rollout, times E
        algo = E * w.num_samples * (4 * _lib.num_params(cfg) + 4)
        achieved = algo / (roll[0]["avg_us"] * 1e-6) / 1e9
        out["rollout_roofline"] = {"bound": "hbm", "algorithmic_bytes_per_launch": algo, "kernel_us": roll[0]["avg_us"],
                                   "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": round(achieved / HBM_PEAK_GBS, 5)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--one-shape", type=int, default=0, metavar="E")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV")
    ap.add_argument("--kernel-stats-envs", type=int, default=16)
    ap.add_argument("--gait", action="store_true", help="gait-adaptive sampling on both sides")
    ap.add_argument("--cost-terms", action="store_true", help="the opt-in cost terms on both sides")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.gait and a.cost_terms:
        ap.error("--gait with --cost-terms: the batch has no form of that combination")
    feature = "gait" if a.gait else ("cost_terms" if a.cost_terms else None)
    a.out = a.out or OUT[feature]
    if a.one_shape:
        r = Runner(a.one_shape, sequential=False, feature=feature)
        try:
            lat = r.batch_steps(200)
        finally:
            r.close()
        print(json.dumps({"E": a.one_shape, "batch_p50_us": round(float(np.percentile(lat, 50)), 2)}))
        return
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.kernel_stats:
        doc["kernel_trace"] = kernel_rows(a.kernel_stats, a.kernel_stats_envs, feature)
    else:
        w, _ = c2_config()
        doc.update({"workload": w.name, "shape": {"N_per_env": w.num_samples, "H": w.horizon, "method": w.method,
                                                  "parametrization": w.parametrization, "rng": "philox"},
                    "feature": {None: "none (the plain cost, the caller's contact sequences)",
                                "gait": {"gait_adaptive": True, "timings": GA_TIMINGS, "freq_set": GA_FREQS,
                                         "duty": GA_DUTY, "frequencies": "device-drawn"},
                                "cost_terms": COST_TERMS}[feature],
                    "timing": "host-to-host around the library call (ctypes, pre-staged addresses); blocks of %d batch "
                              "steps alternate with blocks of %d rounds of E sequential srbd_step calls" % (BLOCK, BLOCK),
                    "rows": [measure(E, a.steps, a.warmup, feature) for E in a.envs]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
