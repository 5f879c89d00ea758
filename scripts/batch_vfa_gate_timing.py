#!/usr/bin/env python3
"""The apex-gated foothold adaptation (srbd_vfa_step_device) against the ungated search (srbd_tamols_batch_device),
terrain form, on the workload of profiles/batch_foothold.json (Go2, 13 x 7 patches, the stepping-stones scene)
-> profiles/batch_vfa_gate.json.

For each E in {1, 1024, 4096}, in one process, device time between two events over 100 back-to-back calls on one
stream, BLOCKS blocks per kind, the kinds interleaved; median, minimum and maximum block are reported, in us per call:

  ungated          srbd_tamols_batch_device: every leg of every environment searched
  gated_0          srbd_vfa_step_device, no environment searching (the gait's share of holding and passing ones)
  gated_trot       the searching share of a trot at the reference's dt (below)
  gated_100        every environment searching
  tiny_kernel      a one-element torch kernel, back to back: what a launch that does nothing costs here

A search sets `initialized`, so a second call on the same state would hold instead of searching.  To time a fixed
share, each of a block's 100 gated calls gets a state array of its own (100 x E x 320 bytes), all of them put back
from a saved copy before the block's first event, so nothing but the calls lies between the events.  The contacts of
`ungated` are the searching environments' (a diagonal pair in swing) where profiles/batch_foothold.json drew them at
random.  Every block is enqueued behind a spinning kernel of a few milliseconds, recorded before the first event, so
that the 100 calls wait in the queue and run back to back: without it the small rows measure how fast Python enqueues
(about 25 us per call here), not the device.

The searching share is computed from the gait, not assumed: the host gate (srbd_vfa_mode / srbd_vfa_commit on the host
PeriodicGaitGenerator's contacts and the host clocks) is stepped over SIM_CYCLES gait cycles of a trot (duty 0.65,
1.4 Hz, swing period 0.25 s, apex window +- 0.01 s, dt 0.004 s) and the steps of each mode are counted.

--ungated-only --pkg-root DIR times only `ungated`, importing the package from DIR: with a build of the parent commit
there, the parent's own ungated call is measured on the same box in the same session (--parent-root does both from
one command, the parent in a child process started before this one touches the device).

  python scripts/batch_vfa_gate_timing.py [--envs 1 1024 4096] [--parent-root DIR] [--out profiles/batch_vfa_gate.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "batch_vfa_gate.json")
CALLS, WARMUP, BLOCKS = 100, 10, 7
FEET = np.array([[0.62, 0.13, 0.0], [0.62, -0.13, 0.0], [0.24, 0.13, 0.0], [0.24, -0.13, 0.0]])
TROT = dict(duty=0.65, freq=1.4, dt=0.004, interval=0.01)
SIM_CYCLES = 50


def inputs(E):  # scripts/batch_foothold_timing.py's
    rng = np.random.default_rng(E)
    feet = FEET[None] + np.stack([rng.uniform(0.0, 3.0, E), rng.uniform(-0.3, 0.3, E), np.zeros(E)], 1)[:, None, :]
    seeds = feet + np.array([0.12, 0.0, 0.0]) + rng.uniform(-0.03, 0.03, (E, 4, 3)) * [1, 1, 0]
    return dict(seeds=seeds, hips=feet + [0.0, 0.0, 0.30], vel=np.tile([0.4, 0.05, 0.0], (E, 1)),
                base=feet.mean(1) + [0, 0, 0.3], contact=(rng.uniform(size=(E, 4)) < 0.5).astype(np.float32),
                feet=feet, yaws=rng.uniform(-3.0, 3.0, E))


def stats(v):
    return {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2),
            "max": round(float(np.max(v)), 2), "blocks": [round(float(x), 2) for x in v]}


def trot_shares(_lib):
    """Steps per mode of the host gate over SIM_CYCLES cycles of the trot, the start-up cycle left out."""
    from quadruped_pympc_amd.helpers.periodic_gait_generator import PeriodicGaitGenerator

    t = TROT
    period = (1.0 - t["duty"]) / t["freq"]
    pgg = PeriodicGaitGenerator(t["duty"], t["freq"], 0, 12)
    stc, vfa = _lib.SrbdStc(), _lib.SrbdVfa()
    assert _lib.lib.srbd_stc_init(C.byref(stc), 0.06, period, 500.0, 10.0, _lib.SWING_BEZIER_REF) == 0
    assert _lib.lib.srbd_vfa_init(C.byref(vfa)) == 0
    per_cycle = 1.0 / (t["freq"] * t["dt"])
    skip, steps = int(2 * per_cycle), int(round((SIM_CYCLES + 2) * per_cycle))
    counts = np.zeros(3, dtype=np.int64)
    seeds, zf, zb, zv = np.zeros(12), np.zeros(12), np.zeros(24), np.ones(4, dtype=np.int32)
    of, ob, ov = np.zeros(12), np.zeros(24), np.zeros(4, dtype=np.int32)
    for k in range(steps):
        contact = np.ascontiguousarray(pgg.run(t["dt"], t["freq"]), dtype=np.float64)
        m = C.c_int32(0)
        assert _lib.lib.srbd_vfa_mode(C.byref(vfa), C.byref(stc), _lib.dptr(contact), t["interval"], C.byref(m)) == 0
        assert _lib.lib.srbd_vfa_commit(C.byref(vfa), m.value, _lib.dptr(seeds), _lib.dptr(zf), _lib.dptr(zb),
                                        _lib.iptr(zv), _lib.dptr(of), _lib.dptr(ob), _lib.iptr(ov)) == 0
        assert _lib.lib.srbd_stc_update_swing_time(C.byref(stc), _lib.dptr(contact), t["dt"]) == 0
        if k >= skip:
            counts[m.value] += 1
    n = int(counts.sum())
    return {"steps": n, "cycles": round(n / per_cycle, 2), "search": counts[_lib.VFA_SEARCH] / n,
            "hold": counts[_lib.VFA_HOLD] / n, "pass": counts[_lib.VFA_PASS] / n,
            "searches_per_cycle": round(counts[_lib.VFA_SEARCH] / (n / per_cycle), 3)}


def gate_state(_lib, E, n_search, hold_share, contact):
    """Structs and contacts that make the first n_search environments (spread over the grid) search and the others hold
    or pass in the gait's proportion."""
    period = (1.0 - TROT["duty"]) / TROT["freq"]
    stc, vfa = (_lib.SrbdStc * E)(), (_lib.SrbdVfa * E)()
    searching = set(np.linspace(0, E - 1, n_search).round().astype(int).tolist()) if n_search else set()
    n_hold = int(round(hold_share * (E - len(searching))))
    k = 0
    for e in range(E):
        assert _lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, period, 500.0, 10.0, _lib.SWING_BEZIER_REF) == 0
        assert _lib.lib.srbd_vfa_init(C.byref(vfa[e])) == 0
        if e in searching:  # a diagonal pair at the apex
            contact[e] = [0.0, 1.0, 1.0, 0.0]
            stc[e].swing_time[0] = stc[e].swing_time[3] = period / 2.0
        elif k < n_hold:  # past the apex, still swinging, searched before
            k += 1
            contact[e] = [0.0, 1.0, 1.0, 0.0]
            stc[e].swing_time[0] = stc[e].swing_time[3] = 0.8 * period
            for l in range(4):
                vfa[e].initialized[l] = 1
        else:  # full stance
            contact[e] = 1.0
    return stc, vfa, len(searching)


def measure(E, terrain, p, _lib, torch, shares, ungated_only):
    inp = inputs(E)
    inp["contact"][:] = [0.0, 1.0, 1.0, 0.0]  # the searching environments' contacts, for the ungated call too
    stream = torch.cuda.Stream()
    up = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731  (a writable copy)
    d = {k: up(v) for k, v in inp.items()}
    first = _lib.tamols_batch_device(d["seeds"], d["hips"], p, terrain=terrain, yaws=d["yaws"], forward_vel=d["vel"],
                                     base_pos=d["base"], contact=d["contact"], feet=d["feet"], stream=stream)
    stream.synchronize()
    out = {k: first[k] for k in ("footholds", "boxes", "valid")}

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    t0, t1 = events()  # the spin kernel's rate, once: cycles for about 6 ms
    with torch.cuda.stream(stream):
        t0.record(stream)
        torch.cuda._sleep(1_000_000)
        t1.record(stream)
    stream.synchronize()
    spin = int(6.0 / max(t0.elapsed_time(t1), 1e-3) * 1_000_000)

    def timed(n, body, before=None):
        t0, t1 = events()
        with torch.cuda.stream(stream):
            if before:
                before()
            torch.cuda._sleep(spin)
        t0.record(stream)
        for i in range(n):
            body(i)
        t1.record(stream)
        stream.synchronize()
        return t0.elapsed_time(t1) * 1e3 / n  # us per call

    def ungated(i=0):
        _lib.tamols_batch_device(d["seeds"], d["hips"], p, terrain=terrain, yaws=d["yaws"], forward_vel=d["vel"],
                                 base_pos=d["base"], contact=d["contact"], feet=d["feet"], out=out, stream=stream)

    kinds = {"ungated": (ungated, None)}
    row = {"num_envs": E}
    if not ungated_only:
        one = torch.zeros(1, device="cuda")

        def tiny(i=0):
            with torch.cuda.stream(stream):
                one.add_(1.0)

        kinds["tiny_kernel"] = (tiny, None)
        n_trot = int(round(shares["search"] * E))
        row["searching_envs"] = {"gated_0": 0, "gated_trot": n_trot, "gated_100": E}
        for name, n_search in (("gated_0", 0), ("gated_trot", n_trot), ("gated_100", E)):
            contact = inp["contact"].copy()
            stc, vfa, _ = gate_state(_lib, E, n_search, shares["hold"] / (shares["hold"] + shares["pass"]), contact)
            stc_t = up(np.frombuffer(bytes(stc), dtype=np.uint8).reshape(E, _lib.STC_BYTES))
            saved = up(np.frombuffer(bytes(vfa), dtype=np.uint8).reshape(E, _lib.VFA_BYTES))
            states, c_t = saved.repeat(CALLS, 1, 1), up(contact)
            g_out = dict(out, mode=torch.zeros(E, dtype=torch.int32, device="cuda"))

            def restore(states=states, saved=saved):
                states.copy_(saved.expand_as(states))

            def gated(i=0, states=states, stc_t=stc_t, c_t=c_t, g_out=g_out):
                _lib.vfa_step_device(states[i], stc_t, d["seeds"], d["hips"], p, c_t, apex_interval=TROT["interval"],
                                     terrain=terrain, yaws=d["yaws"], forward_vel=d["vel"], base_pos=d["base"],
                                     feet=d["feet"], out=g_out, stream=stream)

            kinds[name] = (gated, restore)
            gated()
            stream.synchronize()
            got = np.bincount(g_out["mode"].cpu().numpy(), minlength=3)
            assert got[_lib.VFA_SEARCH] == n_search, (name, got)  # the share that was asked for is the share timed
    for body, before in kinds.values():
        timed(WARMUP, body, before)
    samples = {k: [] for k in kinds}
    for _ in range(BLOCKS):
        for k, (body, before) in kinds.items():
            samples[k].append(timed(CALLS, body, before))
    for k, v in samples.items():
        row[k] = stats(v)
    return row


def run(args):
    sys.path[:0] = [os.path.join(args.pkg_root, "quadruped-pympc-tamols_amd"), args.pkg_root]
    import torch  # torch first: one HIP runtime per process

    from quadruped_pympc_amd import _lib, config
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import tamols_params_struct

    p = dict(config.simulation_params["tamols_params"])
    p["h_des"] = 0.25
    p = tamols_params_struct(p, "go2")
    shares = None if args.ungated_only else trot_shares(_lib)
    terrain = GpuTerrain.stepping_stones()
    try:
        rows = [measure(E, terrain, p, _lib, torch, shares, args.ungated_only) for E in args.envs]
    finally:
        terrain.close()
    return {"device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, args.pkg_root),
            "trot": shares and dict(TROT, **{k: (round(v, 5) if isinstance(v, float) else v) for k, v in shares.items()}),
            "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="*", default=[1, 1024, 4096])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--pkg-root", default=ROOT, help="the checkout whose package and library are imported")
    ap.add_argument("--ungated-only", action="store_true", help="print the ungated rows as JSON and write nothing")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its ungated call is "
                    "timed too, in a child process")
    args = ap.parse_args()
    if args.ungated_only:
        print(json.dumps(run(args)))
        return
    parent = None
    if args.parent_root:  # before this process opens the device; a fresh process, its own package and library
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ungated-only", "--pkg-root",
                                os.path.abspath(args.parent_root), "--envs", *map(str, args.envs)],
                               capture_output=True, text=True, check=True)
        parent = json.loads(child.stdout.strip().splitlines()[-1])
    mine = run(args)
    if parent:  # and once more after, so that the parent's rows bracket this build's in time
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ungated-only", "--pkg-root",
                                os.path.abspath(args.parent_root), "--envs", *map(str, args.envs)],
                               capture_output=True, text=True, check=True)
        again = json.loads(child.stdout.strip().splitlines()[-1])
        for r, a, b in zip(mine["rows"], parent["rows"], again["rows"]):
            r["parent_ungated"] = {"before": a["ungated"], "after": b["ungated"]}
    doc = {"workload": {"robot": "go2", "rows": 13, "cols": 7, "scene": "stepping_stones", "form": "terrain"},
           "device": mine["device"], "calls": CALLS, "warmup": WARMUP, "blocks": BLOCKS, "runs": 1,
           "note": "one run on one box; device time between events over back-to-back calls, us per call; median, min "
                   "and max over the blocks, each block queued behind a spinning kernel so that the calls run back "
                   "to back; parent_ungated: the parent commit's build, child processes before and "
                   "after", "trot": mine["trot"], "rows": mine["rows"]}
    print(f"{'E':>6} {'ungated':>9} {'gated 0%':>9} {'trot':>9} {'100%':>9} {'tiny':>6} {'parent':>15}  (us)")
    for r in doc["rows"]:
        par = r.get("parent_ungated")
        par = f"{par['before']['median']}/{par['after']['median']}" if par else "-"
        print(f"{r['num_envs']:>6} {r['ungated']['median']:>9} {r['gated_0']['median']:>9} "
              f"{r['gated_trot']['median']:>9} {r['gated_100']['median']:>9} {r['tiny_kernel']['median']:>6} {par:>15}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT)}))


if __name__ == "__main__":
    main()
