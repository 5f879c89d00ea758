#!/usr/bin/env python3
"""One control step's producers -- the contact sequences and the prepared states and references of E environments
(Go2 trot, H = 12, MPPI zero-order: 36 warm-start parameters per leg) -- two ways -> profiles/batch_producers.json.

For each E in {64, 1024, 4096}, in one process, blocks of calls alternate between

  host      the route without the device producers: E PeriodicGaitGenerator.run + compute_contact_sequence calls,
            Batched_Sampling_MPC.prepare_state_and_reference (a Python loop over E) and the host-to-device copies of
            the contact sequences, states and references (float32, as the step takes them)
  enqueue   BatchedPeriodicGaitGenerator.run + compute_contact_sequence, the current-contact column made contiguous
            and Batched_Sampling_MPC.prepare_state_and_reference_device: the time the calls take to enqueue (three
            launches and one torch copy; the stream is drained outside the timed region every 10 steps)
  synced    the same followed by one stream synchronise: device arrays in, device arrays ready
  step      srbd_batch_step_device on those arrays (N = 256, Philox draws) followed by one stream synchronise: the
            consumer, for the share of the loop each side takes

until the device kinds have 200 samples after 20 warm-up calls and the host kind 40 after 4 (one host sample at
E = 4096 takes tens of milliseconds).  Times are host-to-host around the Python calls a user makes, so both routes
carry their binding work; p50, p10 and p90 in us.  One run on one box.

  python scripts/batch_producers_timing.py [--envs 64 1024 4096] [--out profiles/batch_producers.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]

import torch  # noqa: E402  (torch first: one HIP runtime per process)

from quadruped_pympc_amd import config as mirror  # noqa: E402
from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC  # noqa: E402
from quadruped_pympc_amd.helpers.periodic_gait_generator import (TROT, BatchedPeriodicGaitGenerator,  # noqa: E402
                                                                 PeriodicGaitGenerator)
from quadruped_pympc_amd.synthetic import CONFIGS, GAITS, reference, robot_state  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_producers.json")
N, H, DT = 256, 12, 0.02
STEPS, WARMUP, BLOCK, DRAIN = 200, 20, 50, 10
HOST_STEPS, HOST_WARMUP, HOST_BLOCK = 40, 4, 10
STATE_KEYS = ("position", "linear_velocity", "orientation", "angular_velocity", "foot_FL", "foot_FR", "foot_RL",
              "foot_RR")
REF_KEYS = ("ref_position", "ref_linear_velocity", "ref_orientation", "ref_angular_velocity", "ref_foot_FL",
            "ref_foot_FR", "ref_foot_RL", "ref_foot_RR")


def config_module():
    cfg = types.ModuleType("batch_producers_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, num_parallel_computations=N, horizon=H, sampling_method="mppi",
                          control_parametrization="zero_order", shift_solution=False, rng="philox", device_id=0)
    return cfg


class Runner:
    def __init__(self, E: int):
        self.E = E
        robot = CONFIGS["c2"].robot
        _, freq, duty = GAITS["trot"]
        self.mpc = Batched_Sampling_MPC(E, config_module())
        self.P = self.mpc.num_control_parameters
        state = np.stack([robot_state(robot, e % 64) for e in range(E)])
        ref = np.stack([reference(robot, s) for s in state])
        # the host route's inputs: what a host simulator hands over
        self.sd = [dict(zip(STATE_KEYS, state[e].reshape(8, 3))) for e in range(E)]
        self.rd = [dict(zip(REF_KEYS, ref[e].reshape(8, 3))) for e in range(E)]
        self.pggs = [PeriodicGaitGenerator(duty, freq, TROT, H) for _ in range(E)]
        self.prev_host = np.ones((E, 4))
        # the device route's: what a device simulator hands over
        self.stream = torch.cuda.Stream()
        with torch.cuda.stream(self.stream):
            self.gen = BatchedPeriodicGaitGenerator(E, duty, freq, TROT, H)
            self.d_state, self.d_ref = torch.from_numpy(state).cuda(), torch.from_numpy(ref).cuda()
            self.d_prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
            self.d_best = torch.zeros((E, self.P), dtype=torch.float32, device="cuda")
            self.d_keys = torch.tensor([[100 + e, 0] for e in range(E)], dtype=torch.int64, device="cuda")
            self.d_seq = torch.empty((E, 4, H), dtype=torch.float32, device="cuda")
        self.stream.synchronize()
        self.last = None

    def close(self):
        self.mpc.close()

    def host_step(self) -> float:
        t0 = time.perf_counter()
        seqs = np.empty((self.E, 4, H), np.float32)
        for e, g in enumerate(self.pggs):
            g.run(DT, g.step_freq)
            seqs[e] = g.compute_contact_sequence([DT], [H])
        current = seqs[:, :, 0]
        states, refs = self.mpc.prepare_state_and_reference(self.sd, self.rd, current, self.prev_host)
        d = (torch.from_numpy(seqs).cuda(), torch.from_numpy(states.astype(np.float32)).cuda(),
             torch.from_numpy(refs.astype(np.float32)).cuda())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.prev_host = current.copy()
        self.last = d
        return t1 - t0

    def device_step(self, sync: bool) -> float:
        s = self.stream
        t0 = time.perf_counter()
        self.gen.run(DT, stream=s)
        seq = self.gen.compute_contact_sequence([DT], [H], out=self.d_seq, stream=s)
        with torch.cuda.stream(s):
            current = seq[:, :, 0].contiguous()
        states, refs = self.mpc.prepare_state_and_reference_device(self.d_state, self.d_ref, current, self.d_prev, s,
                                                                   best_control_parameters=self.d_best)
        if sync:
            s.synchronize()
        t1 = time.perf_counter()
        self.d_prev = current
        self.last = (seq, states, refs)
        return t1 - t0

    def step(self) -> float:
        seq, states, refs = self.last
        t0 = time.perf_counter()
        self.mpc.compute_control_device(states, refs, seq, self.d_best, self.d_keys, stream=self.stream)
        self.stream.synchronize()
        t1 = time.perf_counter()
        with torch.cuda.stream(self.stream):
            self.d_keys[:, 1] += 1
        return t1 - t0

    def block(self, kind: str, n: int) -> list[float]:
        out = []
        for i in range(n):
            if kind == "host":
                out.append(self.host_step())
            elif kind == "step":
                out.append(self.step())
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
        kinds = ("host", "enqueue", "synced", "step")
        r.block("synced", WARMUP)  # the step kind needs device arrays
        for k in kinds:
            r.block(k, HOST_WARMUP if k == "host" else WARMUP)
        samples = {k: [] for k in kinds}
        for _ in range(STEPS // BLOCK):
            for k in kinds:
                if k == "step":
                    r.block("synced", 1)  # fresh device arrays for the consumer
                samples[k] += r.block(k, HOST_BLOCK if k == "host" else BLOCK)
        return {"num_envs": E, **{k: quantiles(v) for k, v in samples.items()}}
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    rows = [measure(E) for E in args.envs]
    doc = {"workload": {"robot": "go2", "gait": "trot", "horizon": H, "params_per_leg": 3 * H, "dt": DT,
                        "step": {"method": "mppi", "parametrization": "zero_order", "num_samples": N,
                                 "rng": "philox"}},
           "device": torch.cuda.get_device_name(0), "steps": STEPS, "warmup": WARMUP, "block": BLOCK,
           "host_steps": HOST_STEPS, "host_warmup": HOST_WARMUP, "host_block": HOST_BLOCK,
           "note": "one run on one box", "rows": rows}
    print(f"{'E':>6} {'host p50':>12} {'enqueue p50':>12} {'synced p50':>11} {'step p50':>10}   (us)")
    for row in rows:
        print(f"{row['num_envs']:>6} {row['host']['p50_us']:>12} {row['enqueue']['p50_us']:>12} "
              f"{row['synced']['p50_us']:>11} {row['step']['p50_us']:>10}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
