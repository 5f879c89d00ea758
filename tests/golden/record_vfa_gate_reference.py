#!/usr/bin/env python3
"""Record the reference's apex gate around the foothold adaptation into tests/golden/vfa_gate_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference; no test runs it:

    python tests/golden/record_vfa_gate_reference.py /path/to/reference-checkout

It loads the reference's ``SwingTrajectoryController``, ``PeriodicGaitGenerator`` and ``VisualFootholdAdaptation``
from the checkout, behind a stand-in ``quadruped_pympc`` package (its ``__init__`` and config are not executed) and a
stand-in ``gym_quadruped``.  The fixture holds inputs and the reference's outputs only.

The gate (wb_interface.py:232-246): the statements are read from the checkout's wb_interface.py at recording time and
executed as they stand on a stand-in ``self`` whose ``stc``, ``pgg`` and ``vfa`` are the reference's objects.  Only
``vfa.compute_adaptation`` is replaced, by a stand-in that gives every leg a foothold moved from its seed by a
recorded offset with a box around it, marks one leg infeasible in every second search (that leg keeps its seed at a
recorded height and, as in the reference's own fallback :223-228, no constraint is assigned) and finishes through the
reference's own ``update_footholds_adaptation``.  The search's numerics are pinned by the TAMOLS fixture; this one
pins the state machine.  After the gate every step runs ``update_swing_time``, as compute_stance_and_swing_torque
would (:374), so the gate sees the clocks the last step left.

Per gait (trot, pace, a crawl; dt = 0.004; more than two gait cycles) every step records: the contact flags, the
swing clocks before the gate, the seeds, whether the search ran and what it injected, the returned footholds and
constraints (NaN for None), and ``footholds_adaptation`` and ``initialized`` afterwards.  The recorder refuses to
write unless, for every gait, all three modes occur, a search is directly followed by a hold inside the same apex
window, a hold is ended by full stance, a pass-through overwrites ``footholds_adaptation``, and an infeasible leg
keeps an older box.
"""
from __future__ import annotations

import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "vfa_gate_ref.npz")
LEGS = ("FL", "FR", "RL", "RR")
HORIZON = 12
SIM_DT = 0.004
APEX_INTERVAL = 0.01  # what wb_interface.py:232 passes; checked against the statement's text below
# name, GaitType value, step_freq, duty_factor, steps (config.py gait_params; the crawl's duty factor as configured)
GAITS = [("trot", 0, 1.4, 0.65, 400), ("pace", 1, 1.4, 0.7, 400), ("crawl", 5, 0.5, 0.8, 1100)]
PASS, SEARCH, HOLD = 0, 1, 2  # include/srbd_host.h SRBD_VFA_*


class LegsAttr:
    """Stand-in for gym_quadruped's LegsAttr: four named entries with attribute and item access."""

    def __init__(self, FL, FR, RL, RR):
        self.FL, self.FR, self.RL, self.RR = FL, FR, RL, RR

    def __getitem__(self, name):
        return getattr(self, name)

    def __setitem__(self, name, value):
        setattr(self, name, value)


def load_reference(checkout):
    import enum

    qp = types.ModuleType("quadruped_pympc")
    qp.__path__ = [os.path.join(checkout, "quadruped_pympc")]
    cfg = types.ModuleType("quadruped_pympc.config")
    cfg.simulation_params = {"tamols_params": {}}
    cfg.robot = "go2"
    qp.config = cfg
    gq, gqu, gqq = (types.ModuleType(n) for n in ("gym_quadruped", "gym_quadruped.utils",
                                                   "gym_quadruped.utils.quadruped_utils"))
    gq.__path__, gqu.__path__ = [], []
    gqq.LegsAttr = LegsAttr
    helpers = types.ModuleType("quadruped_pympc.helpers")
    helpers.__path__ = [os.path.join(checkout, "quadruped_pympc", "helpers")]
    utils = types.ModuleType("quadruped_pympc.helpers.quadruped_utils")
    utils.GaitType = enum.Enum("GaitType", [("TROT", 0), ("PACE", 1), ("BOUNDING", 2), ("CIRCULARCRAWL", 3),
                                            ("BFDIAGONALCRAWL", 4), ("BACKDIAGONALCRAWL", 5),
                                            ("FRONTDIAGONALCRAWL", 6), ("FULL_STANCE", 7)])
    sys.modules.update({"quadruped_pympc": qp, "quadruped_pympc.config": cfg, "gym_quadruped": gq,
                        "gym_quadruped.utils": gqu, "gym_quadruped.utils.quadruped_utils": gqq,
                        "quadruped_pympc.helpers": helpers, "quadruped_pympc.helpers.quadruped_utils": utils})
    from quadruped_pympc.helpers.periodic_gait_generator import PeriodicGaitGenerator
    from quadruped_pympc.helpers.swing_trajectory_controller import SwingTrajectoryController
    from quadruped_pympc.helpers.visual_foothold_adaptation import VisualFootholdAdaptation
    return PeriodicGaitGenerator, SwingTrajectoryController, VisualFootholdAdaptation


def gate_statements(checkout):
    """wb_interface.py:232-246 as text, dedented: from the apex condition to get_footholds_adapted."""
    lines = open(os.path.join(checkout, "quadruped_pympc", "interfaces", "wb_interface.py")).read().splitlines()
    block = lines[231:246]
    assert block[0].strip().startswith("if self.stc.check_apex_condition(self.current_contact, interval=0.01)"), block[0]
    assert "self.vfa.initialized == False" in block[0], block[0]
    assert any(b.strip() == "if self.stc.check_full_stance_condition(self.current_contact):" for b in block), block
    assert block[-1].strip() == "ref_feet_pos, ref_feet_constraints = self.vfa.get_footholds_adapted(ref_feet_pos)", block
    return compile(textwrap.dedent("\n".join(block)), "wb_interface.py:232-246", "exec")


def rows(attr):
    return np.array([np.asarray(attr[n], dtype=np.float64) for n in LEGS])


def boxes(attr):
    out = np.full((4, 2, 3), np.nan)
    for i, n in enumerate(LEGS):
        if attr[n] is not None:
            out[i, 0], out[i, 1] = attr[n][0], attr[n][1]
    return out


def record_gait(classes, code, name, gait, freq, duty, steps, rng):
    pgg_class, stc_class, vfa_class = classes
    swing_period = (1.0 - duty) / freq
    pgg = pgg_class(duty_factor=duty, step_freq=freq, gait_type=gait, horizon=HORIZON)
    stc = stc_class(step_height=0.06, swing_period=swing_period, position_gain_fb=500.0, velocity_gain_fb=10.0,
                    generator="bezier_ref")
    vfa = vfa_class(LEGS, adaptation_strategy="tamols")
    me = types.SimpleNamespace(stc=stc, pgg=pgg, vfa=vfa, current_contact=None)
    injected = {}
    searches = [0]

    def compute_adaptation(legs_order, reference_footholds, *args, **kwargs):
        k = searches[0]
        searches[0] += 1
        valid = np.ones(4, dtype=np.int32)
        if k % 2 == 1:
            valid[(k // 2) % 4] = 0
        fh, bx = np.zeros((4, 3)), np.full((4, 2, 3), np.nan)
        for i, leg in enumerate(legs_order):
            seed = np.asarray(reference_footholds[leg], dtype=np.float64)
            if valid[i]:  # VFA:193-222
                cand = seed + rng.uniform(-0.08, 0.08, 3)
                reference_footholds[leg] = cand
                v1, v2 = cand.copy(), cand.copy()
                v1[0] -= 0.05
                v1[1] -= 0.05
                v2[0] += 0.05
                v2[1] += 0.05
                vfa.footholds_constraints[leg] = [v1, v2]
                bx[i, 0], bx[i, 1] = v1, v2
            else:  # VFA:223-228: the seed at its terrain height, no constraint assigned
                reference_footholds[leg][2] = rng.uniform(-0.05, 0.05)
            fh[i] = reference_footholds[leg]
        injected.update(footholds=fh, boxes=bx, valid=valid)
        vfa.update_footholds_adaptation(reference_footholds)
        return True

    vfa.compute_adaptation = compute_adaptation
    hm = types.SimpleNamespace(update_height_map=lambda *a, **k: None)
    heightmaps = LegsAttr(FL=hm, FR=hm, RL=hm, RR=hm)
    hips = np.array([[0.2, 0.15, 0.0], [0.2, -0.15, 0.0], [-0.2, 0.15, 0.0], [-0.2, -0.15, 0.0]])
    rec = {k: [] for k in ("contact", "clocks", "seeds", "searched", "inj_footholds", "inj_boxes", "inj_valid",
                           "footholds", "boxes", "state_footholds", "initialized", "mode")}
    for step in range(steps):
        me.current_contact = pgg.run(SIM_DT, pgg.step_freq)
        base = np.array([0.3 * SIM_DT * step, 0.0, 0.3])
        seeds = hips + base * np.array([1.0, 1.0, 0.0]) + rng.uniform(-0.01, 0.01, (4, 3))
        ref_feet_pos = LegsAttr(**{n: seeds[i].copy() for i, n in enumerate(LEGS)})
        injected.clear()
        scope = dict(self=me, legs_order=LEGS, heightmaps=heightmaps, ref_feet_pos=ref_feet_pos, hip_pos=None,
                     base_lin_vel=np.zeros(3), base_ori_euler_xyz=np.zeros(3), base_ang_vel=np.zeros(3), base_pos=base,
                     feet_pos=None)
        rec["contact"].append(np.asarray(me.current_contact, dtype=np.float64).copy())
        rec["clocks"].append(np.asarray(stc.swing_time, dtype=np.float64).copy())
        rec["seeds"].append(seeds.copy())
        exec(code, {"hasattr": hasattr}, scope)
        searched = bool(injected)
        rec["searched"].append(int(searched))
        rec["inj_footholds"].append(injected["footholds"] if searched else np.full((4, 3), np.nan))
        rec["inj_boxes"].append(injected["boxes"] if searched else np.full((4, 2, 3), np.nan))
        rec["inj_valid"].append(injected["valid"] if searched else np.zeros(4, dtype=np.int32))
        rec["footholds"].append(rows(scope["ref_feet_pos"]))
        rec["boxes"].append(boxes(scope["ref_feet_constraints"]))
        rec["state_footholds"].append(rows(vfa.footholds_adaptation))
        rec["initialized"].append(int(bool(vfa.initialized)))
        rec["mode"].append(SEARCH if searched else HOLD if vfa.initialized else PASS)
        stc.update_swing_time(me.current_contact, LEGS, SIM_DT)
    out = {k: np.array(v) for k, v in rec.items()}
    out["swing_period"] = np.float64(swing_period)
    check_coverage(name, out)
    return out


def check_coverage(name, r):
    mode, contact, clocks = r["mode"], r["contact"], r["clocks"]
    half = float(r["swing_period"]) / 2.0
    full = (contact != 0).all(axis=1)
    apex = ((contact == 0) & (clocks > half - APEX_INTERVAL) & (clocks < half + APEX_INTERVAL)).any(axis=1)
    n = len(mode)
    found = dict(
        modes=set(mode.tolist()) == {PASS, SEARCH, HOLD},
        search_then_hold_in_window=any(mode[i] == SEARCH and mode[i + 1] == HOLD and apex[i + 1] for i in range(n - 1)),
        hold_ended_by_full_stance=any(mode[i] == HOLD and mode[i + 1] == PASS and full[i + 1] for i in range(n - 1)),
        pass_overwrites=any(mode[i] == PASS and mode[i - 1] == HOLD
                            and not np.array_equal(r["state_footholds"][i - 1], r["seeds"][i])
                            and np.array_equal(r["state_footholds"][i], r["seeds"][i]) for i in range(1, n)),
        stale_box=False)
    for i in range(1, n):
        if mode[i] == SEARCH:
            for l in range(4):
                old = r["boxes"][i - 1][l]
                if r["inj_valid"][i][l] == 0 and not np.isnan(old).any() and np.array_equal(r["boxes"][i][l], old):
                    found["stale_box"] = True
    missing = [k for k, v in found.items() if not v]
    if missing:
        raise SystemExit(f"{name}: not covered: {missing} -- refusing to write")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    checkout = sys.argv[1]
    classes = load_reference(checkout)
    code = gate_statements(checkout)
    rng = np.random.default_rng(5)
    data = dict(sim_dt=np.float64(SIM_DT), apex_interval=np.float64(APEX_INTERVAL),
                gait_names=np.array([g[0] for g in GAITS]), gait_types=np.array([g[1] for g in GAITS], dtype=np.int32),
                gait_freqs=np.array([g[2] for g in GAITS]), gait_duties=np.array([g[3] for g in GAITS]),
                numpy_version=np.array(np.__version__))
    summary = []
    for name, gait, freq, duty, steps in GAITS:
        r = record_gait(classes, code, name, gait, freq, duty, steps, rng)
        for k, v in r.items():
            data[f"{name}_{k}"] = v
        counts = np.bincount(r["mode"], minlength=3)
        summary.append(f"{name}: {steps} steps, {counts[SEARCH]} search / {counts[HOLD]} hold / {counts[PASS]} pass")
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: " + "; ".join(summary))


if __name__ == "__main__":
    main()
