#!/usr/bin/env python3
"""The stance and swing leg torques of E environments two ways -> profiles/batch_leg_control.json.

For each E in {1, 256, 1024, 4096} a child process (its own time limit) alternates blocks of

  hip     BatchedSwingTrajectoryController.step: one srbd_stc_step_device launch per step
  c_call  the same launch through the C call alone with a prebuilt argument struct (no tensor checks)
  torch   the same maths written in plain torch on the same tensors, batched over (E, 4): what a user of
          Batched_Sampling_MPC would otherwise run each step (swing clocks kept in a device tensor)

after a warm-up of each.  A block is 1000 back-to-back steps on one stream between two events, so each figure is
the time per step of a loop that never waits for the device: the larger of the device time and the host's enqueue
time.  `host_us` is the wall time per step the host spent enqueueing the same block; where it equals the event
figure the step is bound by the enqueue, not by the kernel.  Three blocks per kind; the median block is reported, in
us per step.  One run on one box.

  python scripts/batch_leg_control_timing.py [--envs 1 256 1024 4096] [--out profiles/batch_leg_control.json]
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

OUT = os.path.join(ROOT, "profiles", "batch_leg_control.json")
STEPS, WARMUP, BLOCKS = 1000, 50, 3
DT, INTERVAL = 0.002, 0.01
CHILD_LIMIT_S = 240


def inputs(E):
    rng = np.random.default_rng(E)
    a = rng.standard_normal((E, 4, 3, 3)) * 0.1
    lift = rng.uniform(-0.4, 0.4, (E, 4, 3))
    return dict(jac=rng.standard_normal((E, 4, 3, 3)) * 0.25, jac_dot=rng.standard_normal((E, 4, 3, 3)) * 0.5,
                mass_matrix=a @ a.transpose(0, 1, 3, 2) + 0.05 * np.eye(3), q_dot=rng.standard_normal((E, 4, 3)),
                foot_pos=lift + rng.uniform(-0.1, 0.1, (E, 4, 3)), foot_vel=rng.standard_normal((E, 4, 3)) * 0.5,
                qfrc_passive=rng.standard_normal((E, 4, 3)) * 0.3, qfrc_bias=rng.standard_normal((E, 4, 3)) * 2.0,
                grfs=rng.standard_normal((E, 4, 3)) * 40.0, lift_off=lift,
                touch_down=lift + rng.uniform(-0.15, 0.15, (E, 4, 3)),
                contact=(rng.uniform(size=(E, 4)) < 0.5).astype(np.float32))


def torch_step(torch, d, clock, height, period, kp, kd, dt):
    """The leg law in plain torch ('bezier_ref', feedback linearisation and friction compensation on): tau,
    des_foot_pos, des_foot_vel, des_joint_vel, apex, full_stance; `clock` (E, 4) is advanced in place."""
    swing = d["contact"] == 0
    clock.copy_(torch.where(swing, torch.where(clock < period, clock + dt, clock), torch.zeros_like(clock)))
    s = (clock / period).clamp(0.0, 1.0)[..., None]
    u = 1.0 - s
    lo, td = d["lift_off"], d["touch_down"]
    z_mid = torch.maximum(lo[..., 2], td[..., 2]) + height
    p3 = torch.stack([0.5 * (lo[..., 0] + td[..., 0]), 0.5 * (lo[..., 1] + td[..., 1]),
                      (64.0 * z_mid - 22.0 * lo[..., 2] - 22.0 * td[..., 2]) / 20.0], -1)
    # P0 = P1 = P2 and P4 = P5 = P6: the degree-6 basis collapses to three weights
    b_lo = u ** 6 + 6 * s * u ** 5 + 15 * s ** 2 * u ** 4
    b_3 = 20 * s ** 3 * u ** 3
    b_td = 15 * s ** 4 * u ** 2 + 6 * s ** 5 * u + s ** 6
    db_3 = 60 * s ** 2 * u ** 3 - 60 * s ** 3 * u ** 2
    db_lo = -30 * s ** 2 * u ** 3 * 2
    db_td = 60 * s ** 3 * u ** 2
    d2b_3 = 120 * s * u ** 3 - 360 * s ** 2 * u ** 2 + 120 * s ** 3 * u
    d2b_lo = -120 * s * u ** 3 + 180 * s ** 2 * u ** 2
    d2b_td = 180 * s ** 2 * u ** 2 - 120 * s ** 3 * u
    T = period[..., None]
    pos = b_lo * lo + b_3 * p3 + b_td * td
    vel = (db_lo * lo + db_3 * p3 + db_td * td) / T
    acc = (d2b_lo * lo + d2b_3 * p3 + d2b_td * td) / (T * T)
    J = d["jac"]
    Jinv = torch.linalg.inv(J)
    fb = kp[..., None] * (pos - d["foot_pos"]) + kd[..., None] * (vel - d["foot_vel"])
    JT = J.transpose(-1, -2)
    w = (acc + fb) - (d["jac_dot"] @ d["q_dot"][..., None])[..., 0]
    tau_swing = (JT @ fb[..., None])[..., 0] + ((d["mass_matrix"] @ Jinv) @ w[..., None])[..., 0] + d["qfrc_bias"]
    tau_stance = -(JT @ d["grfs"][..., None])[..., 0]
    sw = swing[..., None]
    tau = torch.where(sw, tau_swing, tau_stance) - d["qfrc_passive"]
    des_pos = torch.where(sw, pos, td)
    des_vel = torch.where(sw, vel, torch.zeros_like(vel))
    jv = (Jinv @ des_vel[..., None])[..., 0]
    des_joint_vel = d["q_dot"] + (jv - d["q_dot"]).clamp(-10.0, 10.0)
    half = period / 2.0
    apex = (swing & (clock > half - INTERVAL) & (clock < half + INTERVAL)).any(-1).to(torch.int32)
    full = (~swing).all(-1).to(torch.int32)
    return tau, des_pos, des_vel, des_joint_vel, apex, full


def measure(E):
    import torch  # torch first: one HIP runtime per process

    from quadruped_pympc_amd import _lib
    from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController

    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inputs(E).items()}
    height, period_s, kp_s, kd_s = 0.075, 0.3, 500.0, 10.0
    ctl = BatchedSwingTrajectoryController(E, height, period_s, kp_s, kd_s, "bezier_ref")
    args = (d["jac"], d["jac_dot"], d["q_dot"], d["foot_pos"], d["foot_vel"], d["qfrc_passive"], d["qfrc_bias"],
            d["mass_matrix"], d["grfs"], d["touch_down"], d["contact"])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = ctl.step(DT, *args, lift_off=d["lift_off"], apex_interval=INTERVAL)
        clock = torch.zeros((E, 4), dtype=torch.float64, device="cuda")
        period = torch.full((E, 4), period_s, dtype=torch.float64, device="cuda")
        kp, kd = torch.full_like(period, kp_s), torch.full_like(period, kd_s)
        tref = torch_step(torch, d, clock, height, period, kp, kd, DT)
    stream.synchronize()
    # the two paths compute the same step (first step from zero clocks): agreement to rounding
    agree = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)) for a, b in zip(out[:4], tref[:4]))
    assert agree < 1e-9 and bool((out[4] == tref[4]).all()) and bool((out[5] == tref[5]).all()), agree
    names = ("jac", "jac_dot", "mass_matrix", "q_dot", "foot_pos", "foot_vel", "qfrc_passive", "qfrc_bias", "grfs",
             "touch_down", "lift_off", "contact")
    io = _lib.SrbdStcBatchIo(**{k: d[k].data_ptr() for k in names}, frg=None, apex_interval=INTERVAL,
                             tau=out[0].data_ptr(), des_foot_pos=out[1].data_ptr(), des_foot_vel=out[2].data_ptr(),
                             des_joint_vel=out[3].data_ptr(), apex=out[4].data_ptr(), full_stance=out[5].data_ptr())
    handle, state_ptr, io_ref = C.c_void_p(stream.cuda_stream), ctl.state.data_ptr(), C.byref(io)

    def one(kind):
        if kind == "hip":
            ctl.step(DT, *args, lift_off=d["lift_off"], apex_interval=INTERVAL)
        elif kind == "c_call":
            if _lib.lib.srbd_stc_step_device(state_ptr, E, DT, io_ref, handle) != 0:
                raise RuntimeError("srbd_stc_step_device failed")
        else:
            torch_step(torch, d, clock, height, period, kp, kd, DT)

    def block(kind, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            t0.record(stream)
            w0 = time.perf_counter()
            for _ in range(n):
                one(kind)
            host = (time.perf_counter() - w0) * 1e6 / n
            t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n, host  # us per step: stream time, host enqueue time

    kinds = ("hip", "c_call", "torch")
    for k in kinds:
        block(k, WARMUP)
    s = {k: [] for k in kinds}
    for _ in range(BLOCKS):
        for k in kinds:
            s[k].append(block(k, STEPS))
    row = {"num_envs": E, "agreement_rel": agree}
    for k, v in s.items():
        ev, host = [x[0] for x in v], [x[1] for x in v]
        row[k] = {"us_per_step": round(float(np.median(ev)), 2), "host_us": round(float(np.median(host)), 2),
                  "blocks": [round(x, 2) for x in ev]}
    row["torch_over_hip"] = round(row["torch"]["us_per_step"] / row["hip"]["us_per_step"], 1)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1, 256, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print(json.dumps(measure(args.child)))
        return
    rows = []
    for E in args.envs:  # a fresh process per E, each under its own time limit; the first failure ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(E)], capture_output=True,
                           text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"E = {E}: the measuring process ended with status {r.returncode}; nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    device = rows[0].pop("device")
    for r in rows[1:]:
        r.pop("device")
    doc = {"workload": {"generator": "bezier_ref", "feedback_linearization": True, "friction_compensation": True,
                        "dt": DT, "apex_interval": INTERVAL},
           "device": device, "steps_per_block": STEPS, "warmup": WARMUP, "blocks": BLOCKS,
           "note": "one run on one box; us_per_step: stream time between events over back-to-back steps; host_us: wall "
                   "time the host spent enqueueing one step of the same block",
           "rows": rows}
    print(f"{'E':>6} {'hip':>9} {'(host)':>9} {'c_call':>9} {'(host)':>9} {'torch':>9} {'(host)':>9} {'ratio':>7}   (us)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['hip']['us_per_step']:>9} {r['hip']['host_us']:>9} "
              f"{r['c_call']['us_per_step']:>9} {r['c_call']['host_us']:>9} {r['torch']['us_per_step']:>9} "
              f"{r['torch']['host_us']:>9} {r['torch_over_hip']:>7}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
