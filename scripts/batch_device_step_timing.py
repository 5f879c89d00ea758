#!/usr/bin/env python3
"""The batch's device-resident step against its host step (Go2 trot, MPPI zero-order, N = 256 per environment,
H = 12, Philox device draws) -> profiles/batch_device_step.json.

For each E in {64, 1024, 4096}, in one process and on one pair of contexts, blocks of 50 calls alternate between

  host     srbd_batch_step: host arrays in, host arrays out, the call blocks on the published word
  enqueue  srbd_batch_step_device: the time the call takes to enqueue its five launches (the stream is drained
           outside the timed region every 10 calls, so the queue never grows)
  synced   srbd_batch_step_device followed by one hipStreamSynchronize: device arrays in, device arrays ready

until each has 200 samples after 20 warm-up calls each; the p50 (and p10 / p90) of every kind is reported in us.
Times are host-to-host around the library calls, made through ctypes with pre-staged argument addresses and a
pre-built srbd_batch_device_io, so neither side carries binding work.  Warm starts are fed back and the counters
advance every step on both paths (on the device by a torch op outside the timed region).

  python scripts/batch_device_step_timing.py                 # the table and the JSON
  python scripts/batch_device_step_timing.py --one-shape 4096   # 200 synchronised device steps at E = 4096 and
                                                                # nothing else: the run to put under
                                                                # `rocprofv3 --kernel-trace --stats`
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

import torch  # noqa: E402  (torch first: one HIP runtime per process)

from quadruped_pympc_amd import _lib  # noqa: E402
from quadruped_pympc_amd.synthetic import CONFIGS, inputs  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_device_step.json")
N, STEPS, WARMUP, BLOCK, DRAIN = 256, 200, 20, 50, 10


class Runner:
    def __init__(self, E: int):
        w = CONFIGS["c2"]
        self.cfg = _lib.make_config(num_samples=N, horizon=w.horizon, method="mppi", parametrization="zero_order",
                                    mass=w.mass, inertia=w.inertia, dts=np.full(w.horizon, w.dt, np.float32))
        self.E, self.P, self.H = E, _lib.num_params(self.cfg), self.cfg.horizon
        ins = [inputs(w, e % 64) for e in range(E)]
        self.states = np.ascontiguousarray([x[0] for x in ins], np.float32)
        self.refs = np.ascontiguousarray([x[1] for x in ins], np.float32)
        self.contacts = np.ascontiguousarray([x[2][:, :self.H] for x in ins], np.float32)
        self.seeds = np.arange(100, 100 + E, dtype=np.uint64)
        self.counters = np.zeros(E, np.uint64)
        self.best = np.zeros((E, self.P), np.float32)
        self.results = (_lib.SrbdResult * E)()
        self.host = _lib.BatchContext(self.cfg, E)
        self.dev = _lib.BatchContext(self.cfg, E)
        self.stream = torch.cuda.Stream()
        f = dict(dtype=torch.float32, device="cuda")
        with torch.cuda.stream(self.stream):
            self.t = dict(states=torch.from_numpy(self.states).cuda(), refs=torch.from_numpy(self.refs).cuda(),
                          contacts=torch.from_numpy(self.contacts).cuda(),
                          seeds=torch.from_numpy(self.seeds.view(np.int64)).cuda(),
                          counters=torch.zeros(E, dtype=torch.int64, device="cuda"),
                          best_params=torch.zeros((E, self.P), **f), grf=torch.empty((E, 12), **f),
                          predicted_state=torch.empty((E, 24), **f), best_cost=torch.empty(E, **f),
                          best_index=torch.empty(E, dtype=torch.int32, device="cuda"), best_freq=torch.empty(E, **f),
                          status=torch.empty(E, dtype=torch.int32, device="cuda"))
        self.stream.synchronize()
        self.io = _lib.BatchDeviceIO(contact_stride=self.H, noise=None, costs=None,
                                     **{k: v.data_ptr() for k, v in self.t.items()})
        self.io_ref = C.byref(self.io)
        self.hs = C.c_void_p(self.stream.cuda_stream or 1)  # 1: hipStreamLegacy
        self.addr = [a.ctypes.data for a in (self.states, self.refs, self.contacts, self.best, self.seeds,
                                             self.counters)]

    def close(self):
        self.host.close()
        self.dev.close()

    def host_step(self) -> float:
        a = self.addr
        t0 = time.perf_counter()
        rc = _lib.lib.srbd_batch_step(self.host.h, a[0], a[1], a[2], self.H, a[3], None, a[4], a[5],
                                      C.addressof(self.results), None)
        t1 = time.perf_counter()
        self.host.check(rc, "srbd_batch_step")
        self.counters += 1
        return t1 - t0

    def device_step(self, sync: bool) -> float:
        t0 = time.perf_counter()
        rc = _lib.lib.srbd_batch_step_device(self.dev.h, self.io_ref, self.hs)
        if sync:
            self.stream.synchronize()
        t1 = time.perf_counter()
        self.dev.check(rc, "srbd_batch_step_device")
        with torch.cuda.stream(self.stream):
            self.t["counters"] += 1
        return t1 - t0

    def block(self, kind: str, n: int) -> list[float]:
        out = []
        for i in range(n):
            if kind == "host":
                out.append(self.host_step())
            else:
                out.append(self.device_step(kind == "synced"))
                if kind == "enqueue" and (i + 1) % DRAIN == 0:
                    self.stream.synchronize()
        self.stream.synchronize()
        return out


def quantiles(xs):
    a = np.asarray(xs) * 1e6
    return {"p10_us": round(float(np.percentile(a, 10)), 2), "p50_us": round(float(np.percentile(a, 50)), 2),
            "p90_us": round(float(np.percentile(a, 90)), 2), "samples": int(a.size)}


def measure(E: int) -> dict:
    r = Runner(E)
    try:
        kinds = ("host", "enqueue", "synced")
        for k in kinds:
            r.block(k, WARMUP)
        samples = {k: [] for k in kinds}
        for _ in range(STEPS // BLOCK):
            for k in kinds:
                samples[k] += r.block(k, BLOCK)
        status = r.t["status"].cpu().numpy()
        assert np.all(status == 0), "a device step reported a non-zero status"
        return {"num_envs": E, **{k: quantiles(v) for k, v in samples.items()}}
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--one-shape", type=int, default=0)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.one_shape:
        r = Runner(args.one_shape)
        try:
            r.block("synced", STEPS)
        finally:
            r.close()
        return
    rows = [measure(E) for E in args.envs]
    doc = {"workload": {"robot": "go2", "gait": "trot", "method": "mppi", "parametrization": "zero_order",
                        "num_samples": N, "horizon": CONFIGS["c2"].horizon, "rng": "philox"},
           "device": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP, "block": BLOCK, "rows": rows}
    print(f"{'E':>6} {'host p50':>10} {'enqueue p50':>12} {'synced p50':>11}   (us)")
    for row in rows:
        print(f"{row['num_envs']:>6} {row['host']['p50_us']:>10} {row['enqueue']['p50_us']:>12} "
              f"{row['synced']['p50_us']:>11}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
