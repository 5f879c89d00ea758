#!/usr/bin/env python3
"""The TAMOLS foothold search of E environments (Go2, 13 x 7 patches, the stepping-stones scene) two ways
-> profiles/batch_foothold.json.

For each E in {1, 16, 256, 1024, 4096}, in one process, blocks alternate between

  batch_terrain   srbd_tamols_batch_device, terrain form: 100 back-to-back calls between two events on one stream
  batch_patch     the same in the patch form (the patches of a first terrain call, resident on the device)
  sequential      E srbd_tamols_run_terrain calls (TamolsSearch.run_terrain without scores and patches), host to host:
                  what a loop without the batched call pays per step; repeated until about 100 single calls are timed

after a warm-up of each.  The batched kinds are device times (events, so the launch overhead of back-to-back calls
is inside them); the sequential kind is wall time, each call waiting for its outputs as the API does.  Three blocks
per kind; the median block is reported, per call and per environment, in us.  One run on one box.

  python scripts/batch_foothold_timing.py [--envs 1 16 256 1024 4096] [--out profiles/batch_foothold.json]

--scenes: one scene per environment instead (srbd_tamols_batch_scenes_device) -> profiles/batch_foothold_scenes.json.
At E = 1024 (--envs to change), alternating blocks of the same 100 back-to-back calls on the same inputs:

  shared          srbd_tamols_batch_device on the stepping-stones GpuTerrain (batch_terrain above)
  scenes_1        the scenes call on a set of that one scene, every index 0
  scenes_8        the scenes call on a set of 8 variants of the course (stone spacing, radius and top), round-robin

  python scripts/batch_foothold_timing.py --scenes [--envs 1024] [--out profiles/batch_foothold_scenes.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-pympc-tamols_amd"), ROOT]

import torch  # noqa: E402  (torch first: one HIP runtime per process)

from quadruped_pympc_amd import _lib, config  # noqa: E402
from quadruped_pympc_amd.helpers.terrain import GpuTerrain, GpuTerrainSet, stepping_stones_scene  # noqa: E402
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import TamolsSearch, tamols_params_struct  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "batch_foothold.json")
OUT_SCENES = os.path.join(ROOT, "profiles", "batch_foothold_scenes.json")
CALLS, WARMUP, BLOCKS = 100, 10, 3
FEET = np.array([[0.62, 0.13, 0.0], [0.62, -0.13, 0.0], [0.24, 0.13, 0.0], [0.24, -0.13, 0.0]])


def inputs(E):
    rng = np.random.default_rng(E)
    feet = FEET[None] + np.stack([rng.uniform(0.0, 3.0, E), rng.uniform(-0.3, 0.3, E), np.zeros(E)], 1)[:, None, :]
    seeds = feet + np.array([0.12, 0.0, 0.0]) + rng.uniform(-0.03, 0.03, (E, 4, 3)) * [1, 1, 0]
    return dict(seeds=seeds, hips=feet + [0.0, 0.0, 0.30], vel=np.tile([0.4, 0.05, 0.0], (E, 1)),
                base=feet.mean(1) + [0, 0, 0.3], contact=(rng.uniform(size=(E, 4)) < 0.5).astype(np.float32),
                feet=feet, yaws=rng.uniform(-3.0, 3.0, E))


def measure(E, terrain, search, p):
    inp = inputs(E)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    stream = torch.cuda.Stream()
    common = dict(forward_vel=d["vel"], base_pos=d["base"], contact=d["contact"], feet=d["feet"], stream=stream)
    first = _lib.tamols_batch_device(d["seeds"], d["hips"], p, terrain=terrain, yaws=d["yaws"], want_heightmaps=True,
                                     **common)
    stream.synchronize()
    out = {k: first[k] for k in ("footholds", "boxes", "valid")}
    hms = first["heightmaps"]

    def batch(n, patch):
        form = dict(heightmaps=hms) if patch else dict(terrain=terrain, yaws=d["yaws"])
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(n):
            _lib.tamols_batch_device(d["seeds"], d["hips"], p, out=out, **form, **common)
        t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n  # us per call

    def sequential(reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            for e in range(E):
                search.run_terrain(terrain, inp["yaws"][e], inp["seeds"][e], inp["hips"][e], p,
                                   forward_vel=inp["vel"][e], base_position=inp["base"][e],
                                   current_contact=inp["contact"][e], current_feet_pos=inp["feet"][e],
                                   want_scores=False, want_heightmaps=False)
        return (time.perf_counter() - t0) * 1e6 / reps  # us per E calls

    reps = max(1, CALLS // E)
    batch(WARMUP, False), batch(WARMUP, True), sequential(1 if E > WARMUP else WARMUP // E + 1)
    s = dict(batch_terrain=[], batch_patch=[], sequential=[])
    for _ in range(BLOCKS):
        s["batch_terrain"].append(batch(CALLS, False))
        s["batch_patch"].append(batch(CALLS, True))
        s["sequential"].append(sequential(reps))
    row = {"num_envs": E}
    for k, v in s.items():
        m = float(np.median(v))
        row[k] = {"us_per_call": round(m, 2), "us_per_env": round(m / E, 3), "blocks": [round(x, 2) for x in v]}
    row["sequential_over_batch_terrain"] = round(row["sequential"]["us_per_call"] / row["batch_terrain"]["us_per_call"], 2)
    return row


def measure_scenes(E, p):
    inp = inputs(E)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    stream = torch.cuda.Stream()
    common = dict(forward_vel=d["vel"], base_pos=d["base"], contact=d["contact"], feet=d["feet"], stream=stream)
    variants = [stepping_stones_scene(spacing=0.40 + 0.01 * k, radius=0.15 - 0.005 * k, top=0.05 + 0.005 * k)
                for k in range(8)]
    terrain, one, eight = GpuTerrain(**variants[0]), GpuTerrainSet(variants[:1]), GpuTerrainSet(variants)
    ids = {1: torch.zeros(E, dtype=torch.int32, device="cuda"),
           8: (torch.arange(E, device="cuda") % 8).to(torch.int32).contiguous()}
    forms = dict(shared=dict(terrain=terrain), scenes_1=dict(terrain=one, scene_ids=ids[1]),
                 scenes_8=dict(terrain=eight, scene_ids=ids[8]))
    first = _lib.tamols_batch_device(d["seeds"], d["hips"], p, yaws=d["yaws"], **forms["shared"], **common)
    stream.synchronize()
    out = {k: first[k] for k in ("footholds", "boxes", "valid")}

    def batch(n, kind):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(n):
            _lib.tamols_batch_device(d["seeds"], d["hips"], p, yaws=d["yaws"], out=out, **forms[kind], **common)
        t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n  # us per call

    try:
        for kind in forms:
            batch(WARMUP, kind)
        s = {kind: [] for kind in forms}
        for _ in range(BLOCKS):
            for kind in forms:
                s[kind].append(batch(CALLS, kind))
    finally:
        for t in (terrain, one, eight):
            t.close()
    row = {"num_envs": E}
    for k, v in s.items():
        m = float(np.median(v))
        row[k] = {"us_per_call": round(m, 2), "us_per_env": round(m / E, 3), "blocks": [round(x, 2) for x in v]}
    return row


def main_scenes(args, p):
    rows = [measure_scenes(E, p) for E in (args.envs or [1024])]
    doc = {"workload": {"robot": "go2", "rows": 13, "cols": 7, "scene": "stepping_stones",
                        "scenes_8": "8 variants of the course (spacing, radius, top), assigned round-robin"},
           "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "blocks": BLOCKS,
           "note": "one run on one box; device time between events around back-to-back calls, median block",
           "rows": rows}
    print(f"{'E':>6} {'shared/call':>12} {'scenes S=1':>11} {'scenes S=8':>11}   (us)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['shared']['us_per_call']:>12} {r['scenes_1']['us_per_call']:>11} "
              f"{r['scenes_8']['us_per_call']:>11}")
    out = args.out or OUT_SCENES
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(out, ROOT)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", action="store_true", help="time the one-scene-per-environment call instead")
    args = ap.parse_args()
    p = dict(config.simulation_params["tamols_params"])
    p["h_des"] = 0.25
    p = tamols_params_struct(p, "go2")
    if args.scenes:
        return main_scenes(args, p)
    args.envs = args.envs or [1, 16, 256, 1024, 4096]
    args.out = args.out or OUT
    terrain, search = GpuTerrain.stepping_stones(), TamolsSearch(0)
    try:
        rows = [measure(E, terrain, search, p) for E in args.envs]
    finally:
        search.close()
        terrain.close()
    doc = {"workload": {"robot": "go2", "rows": 13, "cols": 7, "scene": "stepping_stones"},
           "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "blocks": BLOCKS,
           "note": "one run on one box; batch: device time between events; sequential: wall time of E single calls",
           "rows": rows}
    print(f"{'E':>6} {'terrain/call':>13} {'patch/call':>11} {'sequential':>11} {'ratio':>7}   (us)")
    for r in rows:
        print(f"{r['num_envs']:>6} {r['batch_terrain']['us_per_call']:>13} {r['batch_patch']['us_per_call']:>11} "
              f"{r['sequential']['us_per_call']:>11} {r['sequential_over_batch_terrain']:>7}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
