#!/usr/bin/env python3
"""Device-resident height scans (srbd_terrain_set_patches_device) and the 'height' strategy behind the apex gate
(srbd_vfa_height_step_scenes_device) on a 16-scene set -> profiles/batch_height_scan.json.

For each E in {64, 1024}, in one process, device time between two events around every single call (REPS calls after
WARMUP, each with its own pair of events on one stream, all of them queued behind a spinning kernel of SPIN_MS so that
the device finds the next call waiting: without it the small rows measure how fast Python enqueues, about 25 us per
call here, not the device); p50, p10, p90, minimum and maximum over the calls, in us:

  scan_points      patches_device, K = 5 patches of 13 x 7 per environment, points (E, 5, 13, 7, 3)
  scan_heights     the same scan, heights (E, 5, 13, 7) alone
  height_step_100  the gated 'height' step with every environment searching (each call on a state array of its own,
                   put back from a saved copy before the timed calls: a search sets `initialized`)
  height_step_0    the gated step with no environment searching (all hold)
  tiny_kernel      a one-element torch kernel between the same events: what the event pair itself measures here

host_route is the way to the same (E, 5, 13, 7, 3) tensor without these calls, with only what the parent commit has:
the centres and scene indices copied to the host, GpuTerrain.patches (the host-array srbd_terrain_patches, which
synchronises) once per scene for the environments standing on it, and the result copied back to the device.  It is host
work and round trips, so it is timed with the host's clock around the whole route (wall_us), REPS_HOST times.

  python scripts/height_scan_timing.py [--envs 64 1024] [--out profiles/batch_height_scan.json]
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
OUT = os.path.join(ROOT, "profiles", "batch_height_scan.json")
REPS, WARMUP, REPS_HOST = 300, 30, 20
SPIN_MS = 30.0
SCENES, K, ROWS, COLS = 16, 5, 13, 7
PERIOD = 0.25


def scenes():
    """16 scenes: stepping stones of four radii, box fields of four densities, four height fields, four flat."""
    from quadruped_pympc_amd.helpers.terrain import stepping_stones_scene

    rng = np.random.default_rng(1)
    out = [stepping_stones_scene(radius=r) for r in (0.10, 0.12, 0.15, 0.18)]
    for n in (10, 20, 40, 80):
        out.append(dict(prims=[dict(type=0, cx=rng.uniform(0, 4), cy=rng.uniform(-0.6, 0.6), cz=0.0,
                                    a=rng.uniform(0.05, 0.2), b=rng.uniform(0.05, 0.2), c=rng.uniform(0.02, 0.1),
                                    yaw=rng.uniform(-3, 3)) for _ in range(n)], has_ground=True, ground_z=0.0))
    for n in (16, 32, 64, 128):
        out.append(dict(prims=[], has_ground=True, ground_z=-0.1,
                        hfield=dict(z=rng.uniform(0, 0.08, (n, n)), x0=-0.5, y0=-1.0, dx=5.0 / n, dy=2.0 / n)))
    out += [dict(prims=[], has_ground=True, ground_z=z) for z in (0.0, 0.01, 0.02, 0.03)]
    assert len(out) == SCENES
    return out


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = lambda p: round(float(np.percentile(v, p)), 2)  # noqa: E731
    return {"p50": q(50), "p10": q(10), "p90": q(90), "min": round(float(v.min()), 2), "max": round(float(v.max()), 2),
            "n": int(v.size)}


def measure(E, tset, singles, _lib, torch):
    rng = np.random.default_rng(E)
    centers = np.stack([rng.uniform(0, 4, (E, K)), rng.uniform(-0.5, 0.5, (E, K)), np.zeros((E, K))], -1)
    yaws = rng.uniform(-3, 3, E)
    ids = (np.arange(E) % SCENES).astype(np.int32)
    up = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731
    c_t, y_t, i_t = up(centers), up(yaws), up(ids)
    stream = torch.cuda.Stream()
    pts = torch.empty((E, K, ROWS, COLS, 3), dtype=torch.float64, device="cuda")
    hts = torch.empty((E, K, ROWS, COLS), dtype=torch.float64, device="cuda")

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):  # the spin kernel's rate, once
        t0.record(stream)
        torch.cuda._sleep(1_000_000)
        t1.record(stream)
    stream.synchronize()
    spin = int(SPIN_MS / max(t0.elapsed_time(t1), 1e-3) * 1_000_000)

    def timed(body, before=None):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        with torch.cuda.stream(stream):
            if before:
                before()
            for i in range(WARMUP):
                body(i)
            if before:
                before()
            torch.cuda._sleep(spin)
            for i, (a, b) in enumerate(pairs):
                a.record(stream)
                body(i)
                b.record(stream)
        stream.synchronize()
        return stats([a.elapsed_time(b) * 1e3 for a, b in pairs])

    row = {"num_envs": E, "rays_per_scan": E * K * ROWS * COLS}
    row["scan_points"] = timed(lambda i: tset.patches_device(c_t, y_t, ROWS, COLS, scene_ids=i_t, stream=stream,
                                                             out=dict(points=pts)))
    row["scan_heights"] = timed(lambda i: tset.patches_device(c_t, y_t, ROWS, COLS, points=False, heights=True,
                                                              scene_ids=i_t, stream=stream, out=dict(heights=hts)))
    one = torch.zeros(1, device="cuda")
    row["tiny_kernel"] = timed(lambda i: one.add_(1.0))

    # the gated step: a diagonal pair at the apex in every environment; searching (not initialized) or holding
    seeds = up(np.concatenate([centers[:, :4, :2], np.zeros((E, 4, 1))], -1))
    contact = up(np.tile(np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32), (E, 1)))
    stc, vfa = (_lib.SrbdStc * E)(), (_lib.SrbdVfa * E)()
    for e in range(E):
        assert _lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, PERIOD, 500.0, 10.0, _lib.SWING_BEZIER_REF) == 0
        assert _lib.lib.srbd_vfa_init(C.byref(vfa[e])) == 0
        stc[e].swing_time[0] = stc[e].swing_time[3] = PERIOD / 2.0
    stc_t = up(np.frombuffer(bytes(stc), dtype=np.uint8).reshape(E, _lib.STC_BYTES))
    saved = up(np.frombuffer(bytes(vfa), dtype=np.uint8).reshape(E, _lib.VFA_BYTES))
    states = saved.repeat(REPS, 1, 1)
    out = dict(footholds=torch.empty((E, 4, 3), dtype=torch.float64, device="cuda"),
               boxes=torch.empty((E, 4, 2, 3), dtype=torch.float64, device="cuda"),
               valid=torch.empty((E, 4), dtype=torch.int32, device="cuda"),
               mode=torch.zeros(E, dtype=torch.int32, device="cuda"))

    def step(i):
        _lib.vfa_height_step_device(states[i], stc_t, seeds, contact, terrain=tset, yaws=y_t, scene_ids=i_t, rows=ROWS,
                                    cols=COLS, out=out, stream=stream)

    row["height_step_100"] = timed(step, lambda: states.copy_(saved.expand_as(states)))
    stream.synchronize()
    assert (out["mode"] == _lib.VFA_SEARCH).all()
    row["height_step_0"] = timed(step)  # every state has searched: all hold
    stream.synchronize()
    assert (out["mode"] == _lib.VFA_HOLD).all()

    # the route without the device calls: host copies, one synchronising host-array call per scene, the copy back
    def host_route():
        c, s = c_t.cpu().numpy(), i_t.cpu().numpy()
        res = np.empty((E, K, ROWS, COLS, 3))
        for k in range(SCENES):
            mine = np.flatnonzero(s == k)
            if mine.size:
                res[mine] = singles[k].patches(c[mine].reshape(-1, 3), np.repeat(yaws[mine], K), ROWS, COLS).reshape(
                    mine.size, K, ROWS, COLS, 3)
        pts.copy_(torch.from_numpy(res))
        torch.cuda.synchronize()

    host_route()
    wall = []
    for _ in range(REPS_HOST):
        t0 = time.perf_counter()
        host_route()
        wall.append((time.perf_counter() - t0) * 1e6)
    row["host_route"] = {"wall_us": stats(wall)}
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]
    import torch  # torch first: one HIP runtime per process

    from quadruped_pympc_amd import _lib
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain, GpuTerrainSet

    sc = scenes()
    tset, singles = GpuTerrainSet(sc), [GpuTerrain(**s) for s in sc]
    try:
        rows = [measure(E, tset, singles, _lib, torch) for E in args.envs]
    finally:
        tset.close()
        for t in singles:
            t.close()
    doc = {"workload": {"scenes": SCENES, "patches_per_env": K, "rows": ROWS, "cols": COLS, "dist": 0.04},
           "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARMUP, "reps_host": REPS_HOST, "runs": 1,
           "spin_ms": SPIN_MS,
           "note": "one box, one run; device time between an event pair around each call, us, the calls queued behind "
                   "a spinning kernel (tiny_kernel: what the pair measures around a one-element kernel); host_route: wall clock of the host-array route with its "
                   "copies, which only needs what the parent commit has",
           "rows": rows}
    print(f"{'E':>6} {'points':>8} {'heights':>8} {'step 100%':>10} {'step 0%':>8} {'tiny':>6} {'host route':>11}  (us, p50)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['scan_points']['p50']:>8} {r['scan_heights']['p50']:>8} "
              f"{r['height_step_100']['p50']:>10} {r['height_step_0']['p50']:>8} {r['tiny_kernel']['p50']:>6} "
              f"{r['host_route']['wall_us']['p50']:>11}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
