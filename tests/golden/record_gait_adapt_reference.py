#!/usr/bin/env python3
"""Record the reference's touch-down trigger and step-frequency write-back into tests/golden/gait_adapt_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference; no test runs it:

    python tests/golden/record_gait_adapt_reference.py /path/to/reference-checkout

It loads the reference's ``SwingTrajectoryController`` (quadruped_pympc/helpers/swing_trajectory_controller.py) and
``PeriodicGaitGenerator`` (quadruped_pympc/helpers/periodic_gait_generator.py) from the checkout, behind a stand-in
``quadruped_pympc`` package (its ``__init__`` and config are not executed) and a stand-in ``gym_quadruped``.  The
fixture holds inputs and the reference's outputs only.

Trigger (``check_touch_down_condition``, :148-165).  Per gait (trot, pace, a crawl) one generator runs GAIT_STEPS
steps of ``run(SIM_DT, step_freq)`` followed by ``compute_contact_sequence``; every step's (current, previous,
sequence) goes to one controller per lookahead (1 and 3), whose returned flag and ``rising_edge_detected`` afterwards
are recorded.  SIM_DT is small enough that every gait passes through full stance between its swings.  Hand-made
sequences follow: an edge with no stable stance yet, stable stance with no edge, an edge consumed once and not twice.
The recorder refuses to write unless, for every gait and lookahead, both return values and both edge transitions
(False -> True, True -> False) occur.

Write-back (wb_interface.py:354-358).  The four statements are read from the checkout's wb_interface.py at recording
time and executed as they stand on a stand-in ``self`` whose ``pgg`` is the reference's generator and whose ``stc`` is
the reference's controller, for ``best_sample_freq`` a float32 scalar over the configured ``step_freq_available``
plus decimals float32 cannot represent, and duty factors 0.65 and 0.5.  Recorded: ``pgg.step_freq``,
``frg.stance_time``, ``stc.swing_period`` as float64 values, and their dtypes' names.  The NumPy version is recorded
too: the products' precision follows its promotion rule.
"""
from __future__ import annotations

import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gait_adapt_ref.npz")
HORIZON = 12
MPC_DT = 0.02
SIM_DT = 0.004
GAIT_STEPS = 400
# name, GaitType value, step_freq, duty_factor (config.py gait_params; the crawl's duty factor as configured)
GAITS = [("trot", 0, 1.4, 0.65), ("pace", 1, 1.4, 0.7), ("crawl", 5, 0.5, 0.8)]
LOOKAHEADS = [1, 3]
FREQS_AVAILABLE = [1.4, 2.0, 2.4]  # config.py mpc_params['step_freq_available']
FREQS_EXTRA = [1.3, 1.1, 0.7, 1.7, 2.3, 3.3, 0.1]
DUTIES = [0.65, 0.5]


def load_reference(checkout):
    qp = types.ModuleType("quadruped_pympc")
    qp.__path__ = [os.path.join(checkout, "quadruped_pympc")]
    cfg = types.ModuleType("quadruped_pympc.config")
    qp.config = cfg
    gq, gqu, gqq = (types.ModuleType(n) for n in ("gym_quadruped", "gym_quadruped.utils",
                                                   "gym_quadruped.utils.quadruped_utils"))
    gq.__path__, gqu.__path__ = [], []
    gqq.LegsAttr = types.SimpleNamespace
    # helpers/quadruped_utils.py imports mujoco; the generator reads only GaitType's values from it (the values of
    # include/srbd_host.h's SRBD_GAIT_* enum)
    import enum

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
    return PeriodicGaitGenerator, SwingTrajectoryController


def write_back_statements(checkout):
    """wb_interface.py:354-358 as text, dedented: the `if optimize_swing == 1:` block."""
    lines = open(os.path.join(checkout, "quadruped_pympc", "interfaces", "wb_interface.py")).read().splitlines()
    block = lines[353:358]
    assert block[0].strip() == "if optimize_swing == 1:" and "regenerate_swing_trajectory_generator" in block[4], block
    return compile(textwrap.dedent("\n".join(block)), "wb_interface.py:354-358", "exec")


def gait_sequences(pgg_class, stc_class):
    cur, prev, seq, look, flag, edge, start, names = [], [], [], [], [], [], [], []
    dts, lens = [MPC_DT], [HORIZON]

    def controller():
        return stc_class(step_height=0.06, swing_period=0.25, position_gain_fb=500.0, velocity_gain_fb=10.0,
                         generator="bezier_ref")

    def feed(name, lookahead, steps):
        stc = controller()
        start.append(len(flag))
        names.append(f"{name}/lookahead{lookahead}")
        flags, edges = [], [False]
        for c, p, s in steps:
            r = stc.check_touch_down_condition(np.array(c, dtype=np.float64), np.array(p, dtype=np.float64),
                                               np.array(s, dtype=np.float64), lookahead=lookahead)
            cur.append(c), prev.append(p), seq.append(s), look.append(lookahead)
            flags.append(int(r)), edges.append(bool(stc.rising_edge_detected))
        flag.extend(flags), edge.extend(edges[1:])
        return flags, edges

    for name, gait, freq, duty in GAITS:
        pgg = pgg_class(duty_factor=duty, step_freq=freq, gait_type=gait, horizon=HORIZON)
        steps, previous = [], np.ones(4)
        for _ in range(GAIT_STEPS):
            current = pgg.run(SIM_DT, pgg.step_freq)
            sequence = pgg.compute_contact_sequence(dts, lens)
            steps.append((current.copy(), previous.copy(), sequence.copy()))
            previous = current
        for lookahead in LOOKAHEADS:
            flags, edges = feed(name, lookahead, steps)
            ups = sum(1 for a, b in zip(edges, edges[1:]) if not a and b)
            downs = sum(1 for a, b in zip(edges, edges[1:]) if a and not b)
            if not (0 in flags and 1 in flags and ups and downs):
                raise SystemExit(f"{name}, lookahead {lookahead}: flags {sorted(set(flags))}, {ups} rising and {downs} "
                                 "falling edge transitions -- refusing to write")

    ones, swing = np.ones(4), np.array([1.0, 0.0, 0.0, 1.0])

    def sequence(columns):  # columns of four flags, padded with full stance to the horizon
        s = np.ones((4, HORIZON))
        for i, col in enumerate(columns):
            s[:, i] = col
        return s

    lift1 = [0.0, 1.0, 1.0, 1.0]
    for lookahead in LOOKAHEADS:
        stable_then_lift = sequence([ones] * lookahead + [lift1])
        unstable = sequence([ones] * (lookahead - 1) + [lift1, lift1])
        all_stance = sequence([])
        # an edge with no stable stance yet (held), then stable: fires once; the same inputs again: not twice
        feed("hand/edge_then_stable", lookahead, [(ones, swing, unstable), (ones, ones, unstable),
                                                  (ones, ones, all_stance), (ones, ones, stable_then_lift),
                                                  (ones, ones, stable_then_lift)])
        # stable stance with no edge: never fires; then a swing step and an edge in the firing step itself
        feed("hand/stable_no_edge", lookahead, [(ones, ones, stable_then_lift), (ones, ones, stable_then_lift),
                                                (swing, ones, stable_then_lift), (ones, swing, stable_then_lift),
                                                (ones, ones, stable_then_lift)])
        # contacts that are not exactly 1 (2.0, 0.5): `== 1` fails for them
        odd = sequence([ones] * lookahead + [[2.0, 1.0, 1.0, 1.0]])
        feed("hand/not_one", lookahead, [(ones, swing, odd), (np.array([2.0, 1, 1, 1]), swing, stable_then_lift),
                                         (ones, np.array([0.5, 1, 1, 1]), sequence([[1, 1, 0.5, 1]] * (lookahead + 1)))])
    start.append(len(flag))
    return dict(td_current=np.array(cur), td_previous=np.array(prev), td_sequence=np.array(seq),
                td_lookahead=np.array(look, dtype=np.int32), td_flag=np.array(flag, dtype=np.int32),
                td_edge_after=np.array(edge, dtype=np.int32), td_start=np.array(start, dtype=np.int64),
                td_names=np.array(names))


def write_back(pgg_class, stc_class, code):
    rows, dtypes = [], set()
    for duty in DUTIES:
        for f in FREQS_AVAILABLE + FREQS_EXTRA:
            best = np.float32(f)
            me = types.SimpleNamespace(
                pgg=pgg_class(duty_factor=duty, step_freq=1.3, gait_type=0, horizon=HORIZON),
                frg=types.SimpleNamespace(stance_time=-1.0), step_height=0.06,
                stc=stc_class(step_height=0.06, swing_period=0.25, position_gain_fb=500.0, velocity_gain_fb=10.0,
                              generator="bezier_ref"))
            exec(code, {"np": np}, {"self": me, "optimize_swing": 1, "best_sample_freq": best})
            got = (me.pgg.step_freq, me.frg.stance_time, me.stc.swing_period)
            dtypes.add(tuple(type(v).__name__ for v in got))
            assert me.stc.swing_generator.swing_period == me.stc.swing_period
            rows.append((duty, best) + tuple(float(v) for v in got))
            # optimize_swing != 1 leaves the three as they were
            exec(code, {"np": np}, {"self": me, "optimize_swing": 0, "best_sample_freq": np.float32(9.0)})
            assert (me.pgg.step_freq, me.frg.stance_time, me.stc.swing_period) == got
    assert len(dtypes) == 1, dtypes
    rows = np.array(rows, dtype=np.float64)
    return dict(wb_duty=rows[:, 0], wb_best_freq=rows[:, 1].astype(np.float32), wb_step_freq=rows[:, 2],
                wb_stance_time=rows[:, 3], wb_swing_period=rows[:, 4], wb_dtypes=np.array(list(dtypes.pop())),
                numpy_version=np.array(np.__version__))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    checkout = sys.argv[1]
    pgg_class, stc_class = load_reference(checkout)
    data = dict(horizon=np.int32(HORIZON), mpc_dt=np.float64(MPC_DT), sim_dt=np.float64(SIM_DT),
                gait_names=np.array([g[0] for g in GAITS]), gait_types=np.array([g[1] for g in GAITS], dtype=np.int32),
                gait_freqs=np.array([g[2] for g in GAITS]), gait_duties=np.array([g[3] for g in GAITS]),
                gait_steps=np.int32(GAIT_STEPS))
    data.update(gait_sequences(pgg_class, stc_class))
    data.update(write_back(pgg_class, stc_class, write_back_statements(checkout)))
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(data['td_flag'])} trigger steps ({int(data['td_flag'].sum())} fired), "
          f"{len(data['wb_duty'])} write-backs, dtypes {list(data['wb_dtypes'])}, NumPy {np.__version__}")


if __name__ == "__main__":
    main()
