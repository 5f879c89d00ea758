#!/usr/bin/env python3
"""Record the reference's reset statements into tests/golden/loop_reset_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference; no test runs it:

    python tests/golden/record_loop_reset_reference.py /path/to/reference-checkout

It loads the reference's ``PeriodicGaitGenerator`` (quadruped_pympc/helpers/periodic_gait_generator.py),
``FootholdReferenceGenerator`` (helpers/foothold_reference_generator.py) and ``VisualFootholdAdaptation``
(helpers/visual_foothold_adaptation.py) from the checkout, behind a stand-in ``quadruped_pympc`` package (its
``__init__`` and config are not executed) and stand-ins for ``gym_quadruped`` and, where it is not installed,
``mujoco`` (imported by the foothold generator's module, not used by what runs here).  The fixture holds inputs and
the reference's field values only.

Gait generator (``reset``, :22-46).  For each of the eight gait types one generator is dirtied -- by 0, 1 and 37
``run(SIM_DT, step_freq)`` calls; by ``set_phase_signal`` with the start-up hold set and two runs, so that it is
still inside the hold; by ``set_full_stance`` after 37 runs; and by a changed ``step_freq`` -- and its fields are
recorded before and after ``reset()``: phase_signal, phase_offset, init, gait_type, previous_gait_type, step_freq,
duty_factor.

``WBInterface.reset`` (wb_interface.py:469-484).  The statements are read from the checkout's wb_interface.py at
recording time and executed as they stand on a stand-in ``self`` whose ``pgg``, ``frg`` and ``vfa`` are the
reference's objects, dirtied first (runs, a lift-off and touch-down update's worth of changed tables, a velocity
history, ``initialized`` set, footholds stored).  Recorded before and after: the generator's fields, the foothold
generator's five tables, its history and scalars, the adaptation's ``initialized`` and footholds, current_contact.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loop_reset_ref.npz")
LEGS = ("FL", "FR", "RL", "RR")
HORIZON = 12
SIM_DT = 0.002
STEP_FREQ, DUTY = 1.4, 0.65
RUNS = (0, 1, 37)
N_WBI = 6


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
    cfg.simulation_params = {"tamols_params": {}, "visual_foothold_adaptation": "tamols"}
    cfg.robot = "go2"
    cfg.gravity_constant = 9.81
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
    mods = {"quadruped_pympc": qp, "quadruped_pympc.config": cfg, "gym_quadruped": gq, "gym_quadruped.utils": gqu,
            "gym_quadruped.utils.quadruped_utils": gqq, "quadruped_pympc.helpers": helpers,
            "quadruped_pympc.helpers.quadruped_utils": utils}
    if importlib.util.find_spec("mujoco") is None:
        mods["mujoco"] = types.ModuleType("mujoco")
    sys.modules.update(mods)
    from quadruped_pympc.helpers.foothold_reference_generator import FootholdReferenceGenerator
    from quadruped_pympc.helpers.periodic_gait_generator import PeriodicGaitGenerator
    from quadruped_pympc.helpers.visual_foothold_adaptation import VisualFootholdAdaptation
    return PeriodicGaitGenerator, FootholdReferenceGenerator, VisualFootholdAdaptation, cfg


def reset_statements(checkout):
    """wb_interface.py:476-483 as text, dedented: the body of WBInterface.reset without its return."""
    lines = open(os.path.join(checkout, "quadruped_pympc", "interfaces", "wb_interface.py")).read().splitlines()
    assert lines[468].strip().startswith("def reset(self, initial_feet_pos"), lines[468]
    block = lines[475:483]
    assert block[0].strip() == "self.pgg.reset()", block[0]
    assert any(b.strip() == "self.frg.lift_off_positions = initial_feet_pos" for b in block), block
    assert any(b.strip() == "self.vfa.reset()" for b in block), block
    assert block[-1].strip() == "self.current_contact = np.array([1, 1, 1, 1])", block[-1]
    return compile(textwrap.dedent("\n".join(block)), "wb_interface.py:476-483", "exec")


def rows(attr):
    return np.array([np.asarray(attr[n], dtype=np.float64) for n in LEGS])


def pgg_fields(g):
    return dict(phase_signal=np.array(g._phase_signal, dtype=np.float64),
                phase_offset=np.array(g.phase_offset, dtype=np.float64),
                init=np.array(g._init, dtype=np.int32), gait_type=np.int32(g.gait_type),
                previous_gait_type=np.int32(g.previous_gait_type), step_freq=np.float64(g.step_freq),
                duty_factor=np.float64(g.duty_factor))


def frg_fields(f):
    hist = np.zeros((20, 2))
    for i, v in enumerate(f.base_vel_hist):
        hist[i] = v
    return dict(lift_off=rows(f.lift_off_positions), lift_off_h=rows(f.lift_off_positions_h),
                touch_down=rows(f.touch_down_positions), touch_down_h=rows(f.touch_down_positions_h),
                last_reference_footholds=rows(f.last_reference_footholds), vel_hist=hist,
                hist_len=np.int32(len(f.base_vel_hist)), stance_time=np.float64(f.stance_time),
                hip_height=np.float64(f.hip_height), hip_offset=np.float64(f.hip_offset))


def vfa_fields(v):
    return dict(initialized=np.int32(bool(v.initialized)), footholds=rows(v.footholds_adaptation))


def main(checkout):
    PGG, FRG, VFA, cfg = load_reference(checkout)
    rng = np.random.default_rng(20261020)
    cases = []  # (dirty name, gait type, before, after)
    for gait in range(8):
        def fresh():
            return PGG(duty_factor=DUTY, step_freq=STEP_FREQ, gait_type=gait, horizon=HORIZON)

        made = []
        for n in RUNS:
            g = fresh()
            for _ in range(n):
                g.run(SIM_DT, g.step_freq)
            made.append((f"run{n}", g))
        g = fresh()  # inside the start-up hold: the phases behind their offsets, the holds set
        g.set_phase_signal(np.array(g.phase_offset) * 0.5, [True] * 4)
        g.run(SIM_DT, g.step_freq)
        g.run(SIM_DT, g.step_freq)
        if gait != 2:  # bounding's rear offsets are 0.0: those two legs leave the hold at the first run
            assert any(g._init), "the hold case left the hold"
        made.append(("hold", g))
        g = fresh()
        for _ in range(37):
            g.run(SIM_DT, g.step_freq)
        g.set_full_stance()
        g.run(SIM_DT, g.step_freq)
        made.append(("full_stance", g))
        g = fresh()
        for _ in range(37):
            g.run(SIM_DT, g.step_freq)
        g.step_freq = 2.4  # what the step-frequency write-back leaves (wb_interface.py:355); reset() keeps it
        made.append(("freq", g))
        for name, g in made:
            before = pgg_fields(g)
            g.reset()
            cases.append((name, gait, before, pgg_fields(g)))
    out = {"pgg_case": np.array([c[0] for c in cases]), "pgg_gait": np.array([c[1] for c in cases], dtype=np.int32)}
    for key in cases[0][2]:
        out[f"pgg_before_{key}"] = np.array([c[2][key] for c in cases])
        out[f"pgg_after_{key}"] = np.array([c[3][key] for c in cases])

    code = reset_statements(checkout)
    wbi = []
    for k in range(N_WBI):
        gait = (0, 1, 5, 3, 7, 2)[k]
        feet0 = LegsAttr(*(rng.uniform(-0.4, 0.4, 3) for _ in LEGS))
        self = types.SimpleNamespace(
            pgg=PGG(duty_factor=DUTY, step_freq=STEP_FREQ, gait_type=gait, horizon=HORIZON),
            frg=FRG(stance_time=0.46, lift_off_positions=feet0, hip_height=0.28),
            vfa=VFA(legs_order=LEGS, adaptation_strategy="tamols"),
            current_contact=np.array([1, 0, 0, 1]))
        for _ in range(23 + 40 * k):
            self.pgg.run(SIM_DT, self.pgg.step_freq)
        for n in LEGS:  # what the lift-off / touch-down updates and compute_footholds_reference leave behind
            for table in (self.frg.lift_off_positions, self.frg.lift_off_positions_h, self.frg.touch_down_positions,
                          self.frg.touch_down_positions_h):
                table[n] = rng.uniform(-0.5, 0.5, 3)
        self.frg.last_reference_footholds = LegsAttr(*(rng.uniform(-0.5, 0.5, 3) for _ in LEGS))
        for _ in range(7 + 5 * k):
            self.frg.base_vel_hist.append(rng.uniform(-1, 1, 2))
        if k % 2 == 0:
            self.vfa.update_footholds_adaptation(LegsAttr(*(rng.uniform(-0.5, 0.5, 3) for _ in LEGS)))
        new_feet = LegsAttr(*(rng.uniform(-0.4, 0.4, 3) for _ in LEGS))
        before = (pgg_fields(self.pgg), frg_fields(self.frg), vfa_fields(self.vfa), np.array(self.current_contact))
        exec(code, {"np": np, "cfg": cfg}, {"self": self, "initial_feet_pos": new_feet})
        after = (pgg_fields(self.pgg), frg_fields(self.frg), vfa_fields(self.vfa), np.array(self.current_contact))
        wbi.append((rows(new_feet), before, after))
    out["wbi_initial_feet"] = np.array([w[0] for w in wbi])
    for when, idx in (("before", 1), ("after", 2)):
        for part, j in (("pgg", 0), ("frg", 1), ("vfa", 2)):
            for key in wbi[0][idx][j]:
                out[f"wbi_{when}_{part}_{key}"] = np.array([w[idx][j][key] for w in wbi])
        out[f"wbi_{when}_current_contact"] = np.array([w[idx][3] for w in wbi], dtype=np.float64)

    # VisualFootholdAdaptation.reset alone (:63-64)
    v = VFA(legs_order=LEGS, adaptation_strategy="tamols")
    held = LegsAttr(*(rng.uniform(-0.5, 0.5, 3) for _ in LEGS))
    v.update_footholds_adaptation(held)
    out["vfa_before_initialized"], out["vfa_before_footholds"] = np.int32(bool(v.initialized)), rows(v.footholds_adaptation)
    v.reset()
    out["vfa_after_initialized"], out["vfa_after_footholds"] = np.int32(bool(v.initialized)), rows(v.footholds_adaptation)
    out["numpy_version"] = np.array(np.__version__)
    assert out["vfa_before_initialized"] == 1 and out["vfa_after_initialized"] == 0
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(cases)} generator cases, {N_WBI} WBInterface.reset cases, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
