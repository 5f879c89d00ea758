#!/usr/bin/env python3
"""Record the reference's swing reflexes into tests/golden/reflex_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference and scipy; no test runs it:

    python tests/golden/record_reflex_reference.py /path/to/reference-checkout

It imports the reference's ``EarlyStanceDetector`` (quadruped_pympc/helpers/early_stance_detector.py) and
``SwingTrajectoryController`` with ``generator="scipy"`` (helpers/swing_trajectory_controller.py,
helpers/swing_generators/scipy_swing_trajectory_generator.py) from the checkout, behind a stand-in ``quadruped_pympc``
package (its ``__init__`` and config are not executed; the stand-in config carries the five values the two classes
read) and a stand-in ``gym_quadruped`` whose ``LegsAttr`` is a by-name container.  Whole ticks are composed exactly as
``WBInterface.compute_stance_and_swing_torque`` composes them (quadruped_pympc/interfaces/wb_interface.py:362-415 and
:435-465): ``esd.update_detection`` on the clocks and ``last_des_foot_pos`` the previous tick left, the stance torques,
``update_swing_time``, the swing legs' ``compute_swing_control_cartesian_space`` with the detector's hit moment and hit
point, ``last_des_foot_pos = des_foot_pos``, friction compensation, the desired joint velocities with their
saturation, and the apex / full-stance conditions on the clocks the tick leaves.  The fixture holds inputs and the
reference's outputs only.

The feet are scripted: each tick's foot is the desired foot position the previous tick wrote minus an error vector
whose length the script chooses -- small (no trigger), large (a hit), or one that passes only one of the two
comparisons.  Sequences: a swing with no hit and a clock that passes swing_period; a hit in each of the four legs, then
stance and a fresh swing (the stale hit is cleared on the first swing tick); two legs that would trigger in the same
tick; a hit candidate inside the last 0.07 s; blind and not blind; the height enhancement on through more than six
touch-downs; the detector switched off.  Every trigger comparison stays away from its threshold by more than 1e-6 (the
recorder asserts it, and the test asserts it on the fixture).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reflex_ref.npz")
LEGS = ["FL", "FR", "RL", "RR"]
MAX_COND = 100.0
MAX_JOINT_VEL_DIFFERENCE = 10.0  # wb_interface.py:447
MARGIN = 1e-6
SMALL, LARGE = 0.004, 0.15  # error lengths: far below both thresholds, far above both for the steps used here


class LegsAttr:
    """By-name container with item access, what the two classes use of gym_quadruped's."""

    def __init__(self, FL=None, FR=None, RL=None, RR=None):
        self.FL, self.FR, self.RL, self.RR = FL, FR, RL, RR

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, value):
        setattr(self, key, value)


def load_reference(checkout, sim):
    qp = types.ModuleType("quadruped_pympc")
    qp.__path__ = [os.path.join(checkout, "quadruped_pympc")]
    cfg = types.ModuleType("quadruped_pympc.config")
    cfg.mpc_params = {"type": "sampling"}
    cfg.simulation_params = sim  # mutated per sequence: both classes read it in their constructors
    qp.config = cfg
    gq, gqu, gqq = (types.ModuleType(n) for n in ("gym_quadruped", "gym_quadruped.utils",
                                                   "gym_quadruped.utils.quadruped_utils"))
    gq.__path__, gqu.__path__ = [], []
    gqq.LegsAttr = LegsAttr
    helpers = types.ModuleType("quadruped_pympc.helpers")
    helpers.__path__ = [os.path.join(checkout, "quadruped_pympc", "helpers")]
    sys.modules.update({"quadruped_pympc": qp, "quadruped_pympc.config": cfg, "gym_quadruped": gq,
                        "gym_quadruped.utils": gqu, "gym_quadruped.utils.quadruped_utils": gqq,
                        "quadruped_pympc.helpers": helpers})
    from quadruped_pympc.helpers.early_stance_detector import EarlyStanceDetector
    from quadruped_pympc.helpers.swing_trajectory_controller import SwingTrajectoryController
    return EarlyStanceDetector, SwingTrajectoryController


def jacobian(rng):
    u, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    v, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    j = u @ np.diag(rng.uniform(0.1, 0.4, 3)) @ v.T
    assert np.linalg.cond(j) <= MAX_COND
    return j


def swings(ticks, *intervals):
    """(ticks, 4) contact flags: 1 except inside the (leg, first, last + 1) swing intervals."""
    c = np.ones((ticks, 4))
    for leg, a, b in intervals:
        c[a:b, leg] = 0.0
    return c


# name, parameters, contact schedule, {(tick, leg): error length}, {(tick, leg): touch_down jump}
def sequences():
    pair_a, pair_b = (0, 3), (1, 2)
    out = []
    # a swing with no hit; swing_period 0.295 is no multiple of dt, so the clocks pass it and hold
    out.append(dict(name="no_hit", dt=0.01, period=0.295, blind=False, enhance=False, mode="tracking", step_height=0.06,
                    rmax=0.14, contact=swings(38, (0, 2, 34), (3, 2, 34)), errors={}, jumps={}))
    # a hit in each leg; a second hit candidate in a leg that already triggered (kept); then stance and a fresh swing
    out.append(dict(name="hit_each_leg", dt=0.01, period=0.2, blind=False, enhance=False, mode="tracking",
                    step_height=0.05, rmax=0.12,
                    contact=swings(54, (0, 2, 22), (3, 2, 22), (1, 24, 44), (2, 24, 44), (0, 46, 52), (3, 46, 52)),
                    errors={(8, 0): LARGE, (12, 3): LARGE, (14, 0): LARGE, (29, 1): LARGE, (33, 2): LARGE,
                            # one comparison each: ratio above 0.3 but shorter than 0.1; longer than 0.1 but, against
                            # a touch_down that jumped 0.5 m away, ratio below 0.3
                            (5, 3): 0.05, (27, 2): 0.12},
                    jumps={(27, 2): 0.5}))
    # blind; two legs in the same tick (the lower wins, the other is untouched and, its error gone, cleaned up the
    # tick after); a candidate inside the last 0.07 s; clocks that pass swing_period
    out.append(dict(name="same_tick_blind", dt=0.01, period=0.195, blind=True, enhance=False, mode="tracking",
                    step_height=0.07, rmax=0.16, contact=swings(28, (1, 2, 25), (2, 2, 25)),
                    errors={(9, 1): LARGE, (9, 2): LARGE, (19, 2): LARGE}, jumps={}))
    # the height enhancement through eight touch-downs after one hit: six cycles raised, then the counter returns to
    # -1; both legs of a pair touch down in the same tick (one increment)
    n, sw = 60, []
    for phase in range(8):
        first = 1 + 7 * phase
        sw += [(leg, first, first + 6) for leg in (pair_a if phase % 2 == 0 else pair_b)]
    out.append(dict(name="enhancement", dt=0.02, period=0.12, blind=False, enhance=True, mode="tracking",
                    step_height=0.05, rmax=0.13, contact=swings(n, *sw), errors={(3, 0): LARGE}, jumps={}))
    # the same with the enhancement and blind, a hit in a later phase restarting the count
    out.append(dict(name="enhancement_blind_rehit", dt=0.02, period=0.12, blind=True, enhance=True, mode="tracking",
                    step_height=0.05, rmax=0.13, contact=swings(32, *sw[:8]), errors={(2, 3): LARGE, (17, 0): LARGE},
                    jumps={}))
    # the detector switched off: large errors, nothing triggers
    out.append(dict(name="off", dt=0.01, period=0.2, blind=False, enhance=True, mode=False, step_height=0.05,
                    rmax=0.12, contact=swings(12, (0, 1, 12), (3, 1, 12)), errors={(4, 0): LARGE, (6, 3): LARGE},
                    jumps={}))
    return out


def run_sequence(esd_class, stc_class, sim, seq, rng):
    sim.update({"reflex_trigger_mode": seq["mode"], "reflex_next_steps_height_enhancement": seq["enhance"],
                "visual_foothold_adaptation": "blind" if seq["blind"] else "tamols",
                "reflex_max_step_height": seq["rmax"]})
    kp, kd = 500.0, 10.0
    stc = stc_class(step_height=seq["step_height"], swing_period=seq["period"], position_gain_fb=kp,
                    velocity_gain_fb=kd, generator="scipy")
    esd = esd_class(legs_order=tuple(LEGS))
    dt, contact = seq["dt"], seq["contact"]
    ticks = len(contact)
    # what the simulator provides, constant over the sequence
    jac = np.stack([jacobian(rng) for _ in range(4)])
    jac_dot = rng.standard_normal((4, 3, 3)) * 0.5
    a = rng.standard_normal((4, 3, 3)) * 0.1
    mass = a @ a.transpose(0, 2, 1) + 0.05 * np.eye(3)
    q_dot = rng.standard_normal((4, 3)) * 2.0
    foot_vel = rng.standard_normal((4, 3)) * 0.5
    passive = rng.standard_normal((4, 3)) * 0.3
    bias = rng.standard_normal((4, 3)) * 2.0
    grfs = rng.standard_normal((4, 3)) * np.array([20.0, 20.0, 80.0])
    stand = np.array([[0.3, 0.2, 0.0], [0.3, -0.2, 0.0], [-0.3, 0.2, 0.0], [-0.3, -0.2, 0.0]]) + \
        rng.uniform(-0.02, 0.02, (4, 3))
    stride = np.array([0.07, 0.01, 0.02]) + rng.uniform(-0.005, 0.005, (4, 3))  # shorter than 0.1: no hit at lift-off

    last_des = LegsAttr(*[np.zeros((3,)) for _ in range(4)])  # wb_interface.py's constructor
    previous = np.ones(4)
    rec = {k: [] for k in ("foot_pos", "lift_off", "touch_down", "contact", "previous_contact", "tau", "des_foot_pos",
                           "des_foot_vel", "des_joint_vel", "apex", "full_stance", "swing_time_after", "early_stance",
                           "has_hitpoint", "hitmoments", "hitpoints", "gait_cycles", "height_enhancement", "gen_pos",
                           "gen_vel", "gen_acc", "trigger_ratio", "trigger_norm")}
    for t in range(ticks):
        cur = contact[t]
        lift_off = stand.copy()
        touch_down = stand + stride + 0.001 * np.sin(0.7 * t + np.arange(12).reshape(4, 3))  # the footholds drift
        for (tick, leg), jump in seq["jumps"].items():
            if tick == t:
                touch_down[leg, 0] += jump
        feet = np.zeros((4, 3))
        for l in range(4):
            length = seq["errors"].get((t, l), SMALL)
            d = rng.standard_normal(3)
            feet[l] = last_des[LEGS[l]] - length * d / np.linalg.norm(d)
        # the comparisons of early_stance_detector.py:75 for the swing legs, as NumPy forms them
        ratio, norm = np.full(4, np.nan), np.full(4, np.nan)
        for l in range(4):
            if cur[l] == 0:
                local = (last_des[LEGS[l]] - feet[l]).squeeze()
                norm[l] = np.linalg.norm(local)
                ratio[l] = norm[l] / np.linalg.norm(touch_down[l] - lift_off[l])
        # wb_interface.py:362-365
        esd.update_detection(LegsAttr(*[feet[l] for l in range(4)]), last_des,
                             lift_off=LegsAttr(*[lift_off[l] for l in range(4)]),
                             touch_down=LegsAttr(*[touch_down[l] for l in range(4)]), swing_time=stc.swing_time,
                             swing_period=stc.swing_period, current_contact=cur, previous_contact=previous,
                             mujoco_contact=None, stc=stc)
        # :369-374
        tau = [-np.matmul(jac[l].T, grfs[l]) for l in range(4)]
        stc.update_swing_time(cur, LEGS, dt)
        # :377-408
        des_foot_pos = LegsAttr(*[np.zeros((3,)) for _ in range(4)])
        des_foot_vel = LegsAttr(*[np.zeros((3,)) for _ in range(4)])
        gen = np.zeros((3, 4, 3))
        for leg_id, leg_name in enumerate(LEGS):
            if cur[leg_id] == 0:
                tau[leg_id], des_foot_pos[leg_name], des_foot_vel[leg_name] = \
                    stc.compute_swing_control_cartesian_space(
                        leg_id=leg_id, q_dot=q_dot[leg_id], J=jac[leg_id], J_dot=jac_dot[leg_id],
                        lift_off=lift_off[leg_id], touch_down=touch_down[leg_id], foot_pos=feet[leg_id],
                        foot_vel=foot_vel[leg_id], passive_force=passive[leg_id], h=bias[leg_id],
                        mass_matrix=mass[leg_id], early_stance_hitmoments=esd.hitmoments[leg_name],
                        early_stance_hitpoints=esd.hitpoints[leg_name])
                gen[:, leg_id] = stc.swing_generator.compute_trajectory_references(
                    stc.swing_time[leg_id], lift_off[leg_id], touch_down[leg_id], esd.hitmoments[leg_name],
                    esd.hitpoints[leg_name])
            else:
                des_foot_pos[leg_name] = touch_down[leg_id]
                des_foot_vel[leg_name] = des_foot_vel[leg_name] * 0.0
        last_des = des_foot_pos
        # :411-415
        if stc.use_friction_compensation:
            for l in range(4):
                tau[l] = tau[l] - passive[l]
        # :435-438, :461-465
        des_joint_vel = []
        for l in range(4):
            v = np.linalg.pinv(jac[l]) @ des_foot_vel[LEGS[l]]
            des_joint_vel.append(q_dot[l] + np.clip(v - q_dot[l], -MAX_JOINT_VEL_DIFFERENCE, MAX_JOINT_VEL_DIFFERENCE))
        hp = [esd.hitpoints[n] for n in LEGS]
        for key, value in dict(
                foot_pos=feet, lift_off=lift_off, touch_down=touch_down, contact=cur, previous_contact=previous,
                tau=np.stack(tau), des_foot_pos=np.stack([np.asarray(des_foot_pos[n], dtype=float) for n in LEGS]),
                des_foot_vel=np.stack([np.asarray(des_foot_vel[n], dtype=float) for n in LEGS]),
                des_joint_vel=np.stack(des_joint_vel), apex=int(stc.check_apex_condition(cur, 0.01)),
                full_stance=int(stc.check_full_stance_condition(cur)),
                swing_time_after=np.array([float(x) for x in stc.swing_time]),
                early_stance=np.array([int(bool(esd.early_stance[n])) for n in LEGS]),
                has_hitpoint=np.array([int(p is not None) for p in hp]),
                hitmoments=np.array([float(esd.hitmoments[n]) for n in LEGS]),
                hitpoints=np.stack([np.zeros(3) if p is None else np.asarray(p, dtype=float) for p in hp]),
                gait_cycles=int(esd.gait_cycles_after_reflex_height_enanchement),
                height_enhancement=int(bool(stc.swing_generator.reflex_next_steps_height_enhancement)),
                gen_pos=gen[0], gen_vel=gen[1], gen_acc=gen[2], trigger_ratio=ratio, trigger_norm=norm).items():
            rec[key].append(np.array(value, dtype=np.float64 if np.asarray(value).dtype.kind == "f" else np.int32))
        previous = cur.copy()
    per_seq = dict(jac=jac, jac_dot=jac_dot, mass_matrix=mass, q_dot=q_dot, foot_vel=foot_vel, qfrc_passive=passive,
                   qfrc_bias=bias, grfs=grfs, step_height=seq["step_height"], swing_period=seq["period"],
                   position_gain_fb=kp, velocity_gain_fb=kd, reflex_max_step_height=seq["rmax"],
                   blind=int(seq["blind"]), enhancement=int(seq["enhance"]),
                   trigger_mode=0 if seq["mode"] is False else 1, dt=dt)
    return per_seq, {k: np.stack(v) for k, v in rec.items()}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sim = {}
    esd_class, stc_class = load_reference(os.path.abspath(sys.argv[1]), sim)
    rng = np.random.default_rng(20261)
    seqs = sequences()
    heads, ticks = [], []
    for seq in seqs:
        h, r = run_sequence(esd_class, stc_class, sim, seq, rng)
        heads.append(h)
        ticks.append(r)
    data = {k: np.stack([np.asarray(h[k]) for h in heads]) for k in heads[0]}
    data.update({k: np.concatenate([r[k] for r in ticks]) for k in ticks[0]})
    data["names"] = np.array([s["name"] for s in seqs])
    data["start"] = np.cumsum([0] + [len(r["contact"]) for r in ticks]).astype(np.int32)  # sequence s: start[s]..start[s+1]
    total = int(data["start"][-1])
    assert total <= 300, total

    # the coverage and the margins the tests rely on
    def of(name):
        s = [q["name"] for q in seqs].index(name)
        return slice(int(data["start"][s]), int(data["start"][s + 1]))

    swing = data["contact"] == 0
    ratio, norm = data["trigger_ratio"][swing], data["trigger_norm"][swing]
    assert np.isfinite(ratio).all() and np.isfinite(norm).all()
    assert np.abs(ratio - 0.3).min() > MARGIN and np.abs(norm - 0.1).min() > MARGIN
    assert ((ratio > 0.3) & (norm < 0.1)).any() and ((ratio < 0.3) & (norm > 0.1)).any()
    new_hit = np.diff(data["early_stance"], axis=0, prepend=0) == 1
    assert not data["early_stance"][of("no_hit")].any() and not data["early_stance"][of("off")].any()
    assert (new_hit[of("hit_each_leg")].sum(axis=0) == 1).all()  # each leg once; the second candidate in leg 0 kept
    same = of("same_tick_blind")
    assert new_hit[same][9].tolist() == [0, 1, 0, 0] and data["early_stance"][same][10].tolist() == [0, 1, 0, 0]
    assert data["trigger_ratio"][same][9, 2] > 0.3 and data["trigger_norm"][same][9, 2] > 0.1  # it would have
    assert data["trigger_ratio"][same][19, 2] > 0.3 and not data["early_stance"][same][19, 2]  # the last 0.07 s
    stale = data["has_hitpoint"][of("hit_each_leg")]
    assert stale[45, 0] == 1 and stale[46, 0] == 0  # kept through stance, cleared on the first swing tick
    enh = data["height_enhancement"][of("enhancement")]
    cyc = data["gait_cycles"][of("enhancement")]
    assert enh.max() == 1 and enh[-1] == 0 and cyc.max() == 5 and cyc[-1] == -1 and cyc[0] == -1
    edges = ((data["contact"] == 1) & (data["previous_contact"] == 0)).any(axis=1)[of("enhancement")]
    assert edges.sum() > 6
    past = data["swing_time_after"] > data["swing_period"][np.searchsorted(data["start"], np.arange(total),
                                                                            side="right") - 1][:, None]
    assert past[of("no_hit")].any() and past[of("same_tick_blind")].any()
    assert set(data["blind"]) == {0, 1}
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(seqs)} sequences, {total} ticks, {os.path.getsize(OUT)} bytes, "
          f"margins ratio {np.abs(ratio - 0.3).min():.3g} norm {np.abs(norm - 0.1).min():.3g}, "
          f"hits {int(new_hit.sum())}")


if __name__ == "__main__":
    main()
