#!/usr/bin/env python3
"""Record the reference's ``PeriodicGaitGenerator.update_start_and_stop`` into tests/golden/start_stop_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference; no test runs it:

    python tests/golden/record_start_stop_reference.py /path/to/reference-checkout

It loads the reference's ``PeriodicGaitGenerator`` (quadruped_pympc/helpers/periodic_gait_generator.py) from the
checkout, behind a stand-in ``quadruped_pympc`` package (its ``__init__`` and config are not executed) and a stand-in
``gym_quadruped`` whose ``LegsAttr`` holds four fields, as record_gait_adapt_reference.py does.  The fixture holds
inputs and the reference's outputs only.  Which of ``set_full_stance`` / ``restore_previous_gait`` a call reached (the
action 1 / 2, else 0) is observed by wrapping those two methods of the instance.

Single calls (``case_*``).  Every case stores the generator's words before the call (gait type, previous gait type,
phase signal, phase offset, init), the ten arguments, the action and the words after it.
  - all eleven conjuncts true, from each of the eight gaits, and with the yaw in each of the four quadrants;
  - each of the eleven conjuncts the only false one, twice (two different values), from a walking gait and from full
    stance (the second restores);
  - a restore from full stance to each gait;
  - ``set_full_stance`` on consecutive calls (the second finds full stance and stops again);
  - a command component of 1e-170, whose square underflows: the reference stops;
  - a NaN in each input group.
Sequences (``seq_*``).  Three runs of 40 steps through one generator each: ``update_start_and_stop``, then
``run(dt, step_freq)``, then ``compute_contact_sequence``, with the current contact fed back from the sequence's
column 0 as WBInterface does: a command for 10 steps, none for 18 (the generator stops at the first step that finds
all four feet down, and stands), then a command again (it walks).  After every step the contact sequence (2 H columns
in full stance, H otherwise) and the generator's words are stored.

Condition of the fixture (asserted here, not a measurement): every quantity compared with 0.1, 0.05 or 0.06 lies at
least 1e-9 relative away from its threshold, because the reference's np.cos / np.sin and np.linalg.norm and the
library's yaw_sincos.h and written-out sums agree only to rounding.  The recorder refuses to write otherwise, and
unless every sequence stops and walks again.
"""
from __future__ import annotations

import enum
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "start_stop_ref.npz")
HORIZON = 12
HIP_OFFSET = 0.1
MARGIN = 1e-9
LEGS = ("FL", "FR", "RL", "RR")


class LegsAttr:
    def __init__(self, FL, FR, RL, RR):
        self.FL, self.FR, self.RL, self.RR = FL, FR, RL, RR


def load_reference(checkout):
    qp = types.ModuleType("quadruped_pympc")
    qp.__path__ = [os.path.join(checkout, "quadruped_pympc")]
    cfg = types.ModuleType("quadruped_pympc.config")
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
    return PeriodicGaitGenerator


def watch(pgg):
    """Note which of the two transitions a call reaches."""
    pgg.action = 0
    stop, restore = pgg.set_full_stance, pgg.restore_previous_gait

    def on_stop():
        pgg.action = 1
        stop()

    def on_restore():
        pgg.action = 2
        restore()

    pgg.set_full_stance, pgg.restore_previous_gait = on_stop, on_restore
    return pgg


def words(pgg):
    return (int(pgg.gait_type), int(pgg.previous_gait_type), np.array(pgg._phase_signal, dtype=np.float64),
            np.array(pgg.phase_offset, dtype=np.float64), np.array(pgg._init, dtype=np.int32))


def standing(yaw=0.3, base=(1.5, -0.7, 0.31)):
    """Inputs for which all eleven conjuncts hold: feet under the hips, shifted sideways by the hip offset."""
    base = np.array(base)
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, -s], [s, c]])  # horizontal -> world
    hips_h = np.array([[0.19, 0.05], [0.19, -0.05], [-0.19, 0.05], [-0.19, -0.05]])
    feet_h = hips_h + np.array([[0.012, HIP_OFFSET - 0.008], [-0.015, -HIP_OFFSET + 0.011],
                                [0.007, HIP_OFFSET + 0.013], [-0.004, -HIP_OFFSET - 0.009]])
    hips, feet = np.zeros((4, 3)), np.zeros((4, 3))
    hips[:, :2] = hips_h @ rot.T + base[:2]
    feet[:, :2] = feet_h @ rot.T + base[:2]
    hips[:, 2], feet[:, 2] = 0.3, 0.02
    return dict(feet=feet, hips=hips, base_pos=base, euler=np.array([0.011, -0.017, yaw]),
                lin_vel=np.array([0.02, -0.03, 0.01]), ang_vel=np.array([0.01, 0.04, -0.02]),
                ref_lin=np.zeros(3), ref_ang=np.zeros(3), contact=np.ones(4))


def check_margins(x):
    """The fixture's condition: nothing compared with 0.1, 0.05 or 0.06 sits within MARGIN (relative) of it."""
    yaw = x["euler"][2]
    R = np.array([np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)]).reshape(2, 2)
    sign = (-1.0, 1.0, -1.0, 1.0)
    pairs = [(np.linalg.norm(x["lin_vel"]), 0.1), (np.linalg.norm(x["ang_vel"]), 0.1), (abs(x["euler"][0]), 0.05),
             (abs(x["euler"][1]), 0.05)]
    for l in range(4):
        f = R @ (x["feet"][l, :2] - x["base_pos"][:2])
        f[1] += sign[l] * HIP_OFFSET
        h = R @ (x["hips"][l, :2] - x["base_pos"][:2])
        pairs.append((np.sqrt(np.square(f[0] - h[0]) + np.square(f[1] - h[1])), 0.06))
    for value, limit in pairs:
        assert np.isnan(value) or abs(value - limit) >= MARGIN * limit, (value, limit)


def call(pgg, x):
    check_margins(x)
    pgg.action = 0
    pgg.update_start_and_stop(LegsAttr(*x["feet"].copy()), LegsAttr(*x["hips"].copy()), HIP_OFFSET,
                              x["base_pos"].copy(), x["euler"].copy(), x["lin_vel"].copy(), x["ang_vel"].copy(),
                              x["ref_lin"].copy(), x["ref_ang"].copy(), x["contact"].copy())
    return pgg.action


def generator(cls, gait, previous=None, warm=0, duty=0.65, freq=1.4):
    pgg = watch(cls(duty_factor=duty, step_freq=freq, gait_type=gait, horizon=HORIZON))
    if previous is not None:
        pgg.previous_gait_type = previous
    for _ in range(warm):
        pgg.run(0.013, pgg.step_freq)
    return pgg


def one_false():
    """(conjunct, variant) -> an edit of the standing inputs that makes that conjunct alone false."""
    def edit(key, value):
        def apply(x):
            x[key] = np.array(value, dtype=np.float64)
        return apply

    def foot(l, dx, dy):
        def apply(x):
            c, s = np.cos(x["euler"][2]), np.sin(x["euler"][2])
            x["feet"][l, 0] += c * dx - s * dy
            x["feet"][l, 1] += s * dx + c * dy
        return apply

    def angle(k, v):
        def apply(x):
            x["euler"][k] = v
        return apply

    return [("ref_lin", edit("ref_lin", [0.0, 0.0, 1e-3])), ("ref_lin", edit("ref_lin", [-0.2, 0.0, 0.0])),
            ("ref_ang", edit("ref_ang", [0.0, 1e-150, 0.0])), ("ref_ang", edit("ref_ang", [0.0, 0.0, 0.3])),
            ("lin_vel", edit("lin_vel", [0.09, 0.05, 0.0])), ("lin_vel", edit("lin_vel", [0.0, 0.0, -0.1001])),
            ("ang_vel", edit("ang_vel", [0.0, 0.2, 0.0])), ("ang_vel", edit("ang_vel", [0.06, 0.06, 0.06])),
            ("roll", angle(0, 0.0501)), ("roll", angle(0, -0.2)),
            ("pitch", angle(1, -0.0501)), ("pitch", angle(1, 0.3)),
            ("contact", edit("contact", [1, 1, 0, 1])), ("contact", edit("contact", [1, 1, 1, 2])),
            ("FL", foot(0, 0.07, 0.0)), ("FL", foot(0, 0.0, -0.06)),
            ("FR", foot(1, -0.08, 0.0)), ("FR", foot(1, 0.03, 0.06)),
            ("RL", foot(2, 0.0, 0.09)), ("RL", foot(2, 0.06, 0.0)),
            ("RR", foot(3, 0.0, -0.07)), ("RR", foot(3, -0.05, -0.04))]


def single_calls(cls):
    rows, names = [], []

    def record(name, pgg, x):
        before = words(pgg)
        action = call(pgg, x)
        rows.append((before, x, action, words(pgg)))
        names.append(name)
        return action

    for gait in range(8):  # all true, from every gait (7: already in full stance, stops again)
        assert record(f"all_true/gait{gait}", generator(cls, gait, warm=gait), standing()) == 1
    for yaw in (0.6, 2.2, -2.5, -0.9, 0.0, 3.1):  # the four quadrants and both axes
        assert record(f"all_true/yaw{yaw}", generator(cls, 0, warm=3), standing(yaw)) == 1
    for k, (name, apply) in enumerate(one_false()):
        for gait, previous, want in ((k % 7, None, 0), (7, k % 7, 2)):
            x = standing(yaw=(0.6, 2.2, -2.5, -0.9)[k % 4])
            apply(x)
            assert record(f"one_false/{name}/{k % 2}/from{gait}", generator(cls, gait, previous, warm=2), x) == want
    for gait in range(8):  # restore from full stance to each gait
        x = standing()
        x["ref_lin"] = np.array([0.3, 0.0, 0.0])
        assert record(f"restore/to{gait}", generator(cls, 7, gait), x) == 2
    pgg = generator(cls, 1, warm=5)  # set_full_stance on consecutive calls
    for i in range(3):
        assert record(f"repeat/{i}", pgg, standing()) == 1
    for key, k in (("ref_lin", 0), ("ref_lin", 2), ("ref_ang", 1)):  # squares that underflow: the reference stops
        x = standing()
        x[key][k] = 1e-170
        assert record(f"underflow/{key}{k}", generator(cls, 0, warm=1), x) == 1
    for key in ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang", "contact"):
        for k in range(3 if key == "euler" else 1):  # a NaN in each input group (each Euler angle)
            for gait, previous, want in ((2, None, 0), (7, 4, 2)):
                x = standing()
                x[key].reshape(-1)[k] = np.nan
                assert record(f"nan/{key}{k}/from{gait}", generator(cls, gait, previous), x) == want
    keys = ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang", "contact")
    out = {f"case_{k}": np.array([r[1][k] for r in rows]) for k in keys}
    out.update(case_names=np.array(names), case_action=np.array([r[2] for r in rows], dtype=np.int32))
    for tag, i in (("before", 0), ("after", 3)):
        out[f"case_{tag}_gait"] = np.array([r[i][0] for r in rows], dtype=np.int32)
        out[f"case_{tag}_previous"] = np.array([r[i][1] for r in rows], dtype=np.int32)
        out[f"case_{tag}_phase"] = np.array([r[i][2] for r in rows])
        out[f"case_{tag}_offset"] = np.array([r[i][3] for r in rows])
        out[f"case_{tag}_init"] = np.array([r[i][4] for r in rows], dtype=np.int32)
    return out


SEQUENCES = [  # gait, yaw, simulation dt, contact_sequence_dts, contact_sequence_lenghts, duty factor, step frequency
    (0, 0.4, 0.02, [0.02], [HORIZON], 0.65, 1.4),
    (1, -2.0, 0.016, [0.01, 0.04], [4, HORIZON], 0.7, 1.4),
    (5, 2.9, 0.03, [0.02], [HORIZON], 0.8, 0.5),  # the crawl as configured: a lower duty factor leaves no full stance
]
SEQ_STEPS = 40


def sequences(cls):
    out = {k: [] for k in ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang", "contact",
                           "action", "cols", "contacts", "gait", "previous", "phase", "offset", "init")}
    rng = np.random.default_rng(11)
    for gait, yaw, dt, dts, lens, duty, freq in SEQUENCES:
        pgg = generator(cls, gait, duty=duty, freq=freq)
        current = np.ones(4)
        actions = []
        for i in range(SEQ_STEPS):
            x = standing(yaw + 0.01 * i, base=(0.02 * i, -0.01 * i, 0.3))
            x["feet"][:, :2] += rng.uniform(-0.004, 0.004, (4, 2))
            x["lin_vel"] = rng.uniform(-0.03, 0.03, 3)
            if not 10 <= i < 28:
                x["ref_lin"] = np.array([0.3, 0.0, 0.0])
                x["ref_ang"] = np.array([0.0, 0.0, 0.1])
            x["contact"] = current.copy()
            action = call(pgg, x)
            pgg.run(dt, pgg.step_freq)
            seq = pgg.compute_contact_sequence(dts, lens)
            current = seq[:, 0].copy()
            padded = np.full((4, 2 * HORIZON), -1.0)
            padded[:, :seq.shape[1]] = seq
            g, p, ph, off, ini = words(pgg)
            for k in ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang", "contact"):
                out[k].append(x[k])
            for k, v in (("action", action), ("cols", seq.shape[1]), ("contacts", padded), ("gait", g),
                         ("previous", p), ("phase", ph), ("offset", off), ("init", ini)):
                out[k].append(v)
            actions.append(action)
        if not (1 in actions and 2 in actions and actions[-1] == 0 and actions.count(1) > 3):
            raise SystemExit(f"sequence of gait {gait}: actions {actions} -- refusing to write")
    res = {f"seq_{k}": np.array(v) for k, v in out.items()}
    res.update(seq_gaits=np.array([s[0] for s in SEQUENCES], dtype=np.int32), seq_dt=np.array([s[2] for s in SEQUENCES]),
               seq_duty=np.array([s[5] for s in SEQUENCES]), seq_freq=np.array([s[6] for s in SEQUENCES]),
               seq_steps=np.int32(SEQ_STEPS))
    for n, s in enumerate(SEQUENCES):
        res[f"seq_dts{n}"] = np.array(s[3], dtype=np.float64)
        res[f"seq_lens{n}"] = np.array(s[4], dtype=np.int32)
    return res


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    cls = load_reference(sys.argv[1])
    data = dict(horizon=np.int32(HORIZON), hip_offset=np.float64(HIP_OFFSET), duty_factor=np.float64(0.65),
                step_freq=np.float64(1.4), margin=np.float64(MARGIN), numpy_version=np.array(np.__version__))
    data.update(single_calls(cls))
    data.update(sequences(cls))
    np.savez_compressed(OUT, **data)
    acts = data["case_action"]
    print(f"wrote {OUT}: {len(acts)} single calls (actions 0/1/2: {[int((acts == a).sum()) for a in range(3)]}), "
          f"{len(SEQUENCES)} sequences of {SEQ_STEPS} steps, NumPy {np.__version__}")


if __name__ == "__main__":
    main()
