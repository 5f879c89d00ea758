#!/usr/bin/env python3
"""The swing reflex launch beside the plain leg-controller launch -> profiles/batch_reflex.json.

Device time per call at E = 64 and E = 1024.  Each timed call sits between its own pair of events on a side stream.
The calls go through the C entry points with a prebuilt argument struct (a few us of host time each, no tensor
checks), CHUNK of them at a time behind a spinning kernel whose length is calibrated after a warm launch, so that the
host has enqueued the whole chunk while the device still spins and the events see the device alone.  That is
asserted, not assumed: the host's wall time from the spin's enqueue to the chunk's last record must be below half the
spin, else the script stops.  p50, p10, p90, minimum and maximum over CHUNKS x CHUNK calls, in us:

  reflex_none   srbd_reflex_step_device, 'tracking' mode, two legs of every environment in swing with a small
                tracking error: the detector runs its comparisons and nothing triggers; the no-hit spline
  reflex_all    the same call with every swing leg in early stance (hit moment 0.05 s): the re-planned spline
  stc           srbd_stc_step_device ('bezier_ref') on the same inputs
  tiny_kernel   an empty kernel (srbd_time_launch's is not reachable without a context, so: a one-element torch
                kernel) between the same events: what the event pair itself measures here

dt is 0 in every call, so the clocks and the detector's state stay where the set-up put them and every repetition does
the same work.  `host_us` beside each row is the host's wall time per call while enqueueing.  One run on one box.

  python scripts/batch_reflex_timing.py [--envs 64 1024] [--out profiles/batch_reflex.json]
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

OUT = os.path.join(ROOT, "profiles", "batch_reflex.json")
CHUNKS, CHUNK, WARMUP, SPIN_MS = 6, 50, 20, 10.0
PERIOD, CLOCK, HIT = 0.3, 0.1, 0.05


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = lambda p: round(float(np.percentile(v, p)), 2)  # noqa: E731
    return {"p50": q(50), "p10": q(10), "p90": q(90), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2),
            "n": int(v.size)}


def measure(E, _lib, torch):
    rng = np.random.default_rng(E)
    a = rng.standard_normal((E, 4, 3, 3)) * 0.1
    lift = rng.uniform(-0.4, 0.4, (E, 4, 3))
    contact = np.tile(np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32), (E, 1))
    x = dict(jac=rng.standard_normal((E, 4, 3, 3)) * 0.25, jac_dot=rng.standard_normal((E, 4, 3, 3)) * 0.5,
             mass_matrix=a @ a.transpose(0, 1, 3, 2) + 0.05 * np.eye(3), q_dot=rng.standard_normal((E, 4, 3)),
             foot_pos=lift.copy(), foot_vel=rng.standard_normal((E, 4, 3)) * 0.5,
             qfrc_passive=rng.standard_normal((E, 4, 3)) * 0.3, qfrc_bias=rng.standard_normal((E, 4, 3)) * 2.0,
             grfs=rng.standard_normal((E, 4, 3)) * 40.0, lift_off=lift,
             touch_down=lift + np.array([0.07, 0.01, 0.02]), contact=contact, previous_contact=contact.copy())
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    args = (d["jac"], d["jac_dot"], d["q_dot"], d["foot_pos"], d["foot_vel"], d["qfrc_passive"], d["qfrc_bias"],
            d["mass_matrix"], d["grfs"], d["touch_down"], d["contact"])

    def states(in_reflex):
        g, r = (_lib.SrbdStc * E)(), (_lib.SrbdReflex * E)()
        for e in range(E):
            assert _lib.lib.srbd_stc_init(C.byref(g[e]), 0.06, PERIOD, 500.0, 10.0, _lib.SWING_BEZIER_REF) == 0
            assert _lib.lib.srbd_reflex_init(C.byref(r[e]), 0.15, 0, _lib.REFLEX_TRACKING, 0) == 0
            for l in range(4):
                for k in range(3):
                    r[e].last_des_foot_pos[l][k] = lift[e, l, k]  # the first call sees no tracking error
                if contact[e, l] == 0:
                    g[e].swing_time[l] = CLOCK
                    if in_reflex:
                        r[e].early_stance[l], r[e].has_hitpoint[l], r[e].hitmoments[l] = 1, 1, HIT
                        for k in range(3):
                            r[e].hitpoints[l][k] = lift[e, l, k] + 0.01
        up = lambda s, n: torch.from_numpy(np.frombuffer(bytes(s), np.uint8).reshape(E, n).copy()).cuda()  # noqa: E731
        return up(g, _lib.STC_BYTES), up(r, _lib.REFLEX_BYTES)

    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):  # the spin kernel's rate, from its second launch
        torch.cuda._sleep(1_000_000)
        stream.synchronize()
        t0.record(stream)
        torch.cuda._sleep(10_000_000)
        t1.record(stream)
    stream.synchronize()
    spin = int(SPIN_MS / max(t0.elapsed_time(t1), 1e-3) * 10_000_000)

    def timed(body):
        """body() enqueues one call on `stream`.  Returns the statistics of the device times, with host_us."""
        times, host = [], []
        with torch.cuda.stream(stream):
            for _ in range(WARMUP):
                body()
            stream.synchronize()
            for _ in range(CHUNKS):
                pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                         for _ in range(CHUNK)]
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record(stream)
                torch.cuda._sleep(spin)
                s1.record(stream)
                w0 = time.perf_counter()
                for a_, b_ in pairs:
                    a_.record(stream)
                    body()
                    b_.record(stream)
                wall_ms = (time.perf_counter() - w0) * 1e3
                still_spinning = not s1.query()
                stream.synchronize()
                spun_ms = s0.elapsed_time(s1)
                # device-bound: the host was done while the spin still ran, with a factor of two to spare
                if not (still_spinning and wall_ms < 0.5 * spun_ms):
                    raise SystemExit(f"not device-bound: the host needed {wall_ms:.2f} ms to enqueue {CHUNK} calls, "
                                     f"the spin lasted {spun_ms:.2f} ms")
                times += [a_.elapsed_time(b_) * 1e3 for a_, b_ in pairs]
                host.append(wall_ms * 1e3 / CHUNK)
        out = stats(times)
        out["host_us"] = round(float(np.median(host)), 2)
        return out

    def ptr(t):
        return None if t is None else t.data_ptr()

    def batch_io(o):
        return _lib.SrbdStcBatchIo(jac=ptr(d["jac"]), jac_dot=ptr(d["jac_dot"]), mass_matrix=ptr(d["mass_matrix"]),
                                   q_dot=ptr(d["q_dot"]), foot_pos=ptr(d["foot_pos"]), foot_vel=ptr(d["foot_vel"]),
                                   qfrc_passive=ptr(d["qfrc_passive"]), qfrc_bias=ptr(d["qfrc_bias"]),
                                   grfs=ptr(d["grfs"]), touch_down=ptr(d["touch_down"]), lift_off=ptr(d["lift_off"]),
                                   frg=None, contact=ptr(d["contact"]), apex_interval=0.01, tau=ptr(o["tau"]),
                                   des_foot_pos=ptr(o["des_foot_pos"]), des_foot_vel=ptr(o["des_foot_vel"]),
                                   des_joint_vel=ptr(o["des_joint_vel"]), apex=ptr(o["apex"]),
                                   full_stance=ptr(o["full_stance"]))

    def checked(rc):
        if rc != _lib.OK:
            raise SystemExit(f"the launch failed ({rc})")

    row = {"num_envs": E}
    for name, in_reflex in (("reflex_none", False), ("reflex_all", True)):
        stc, reflex = states(in_reflex)
        out = _lib.reflex_step_device(stc, reflex, 0.0, *args, d["previous_contact"], lift_off=d["lift_off"])
        # the feet a small error away from the desired positions the call wrote: the detector compares, none triggers
        d["foot_pos"].copy_(out["des_foot_pos"] - 0.004)
        torch.cuda.synchronize()
        rio = _lib.SrbdReflexBatchIo(stc=batch_io(out), previous_contact=ptr(d["previous_contact"]))
        row[name] = timed(lambda: checked(_lib.lib.srbd_reflex_step_device(stc.data_ptr(), reflex.data_ptr(), E, 0.0,
                                                                           C.byref(rio), handle)))
        words = reflex.cpu().numpy().view(np.int32)[:, _lib.SrbdReflex.early_stance.offset // 4:][:, :4]
        row[name + "_legs_in_reflex"] = int(words.sum())
    stc, _ = states(False)
    out = _lib.stc_step_device(stc, 0.0, *args, lift_off=d["lift_off"])
    torch.cuda.synchronize()
    sio = batch_io(out)
    row["stc"] = timed(lambda: checked(_lib.lib.srbd_stc_step_device(stc.data_ptr(), E, 0.0, C.byref(sio), handle)))
    one = torch.zeros(1, device="cuda")
    row["tiny_kernel"] = timed(lambda: one.add_(1.0))
    floor = row["tiny_kernel"]["p50"]
    row["reflex_over_stc_beyond_floor"] = {
        k: round((row[k]["p50"] - floor) / max(row["stc"]["p50"] - floor, 1e-3), 2) for k in ("reflex_none", "reflex_all")}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch

    from quadruped_pympc_amd import _lib

    rows = [measure(E, _lib, torch) for E in a.envs]
    doc = {"what": "device time per call between an event pair on a side stream, us; see scripts/batch_reflex_timing.py",
           "device": torch.cuda.get_device_name(0), "calls": CHUNKS * CHUNK, "calls_per_spin": CHUNK,
           "spin_ms": SPIN_MS, "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{'E':>6} {'reflex none':>12} {'reflex all':>11} {'stc':>7} {'tiny':>6}  (us, p50; p10-p90 and host_us below)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['reflex_none']['p50']:>12} {r['reflex_all']['p50']:>11} {r['stc']['p50']:>7} "
              f"{r['tiny_kernel']['p50']:>6}  legs in reflex {r['reflex_none_legs_in_reflex']} / "
              f"{r['reflex_all_legs_in_reflex']}")
        print("       " + "  ".join(f"{k} {r[k]['p10']}-{r[k]['p90']} host {r[k]['host_us']}"
                                    for k in ("reflex_none", "reflex_all", "stc", "tiny_kernel")))


if __name__ == "__main__":
    main()
