#!/usr/bin/env python3
"""Record the reference's stance and swing leg torques into tests/golden/leg_control_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference; no test runs it:

    python tests/golden/record_leg_control_reference.py /path/to/reference-checkout

It puts the checkout on ``sys.path``, imports the reference's ``SwingTrajectoryController``
(quadruped_pympc/helpers/swing_trajectory_controller.py, with its 'bezier_ref' and 'explicit' generators) and composes
it exactly as ``WBInterface.compute_stance_and_swing_torque`` does (quadruped_pympc/interfaces/wb_interface.py:369-415
and :435-465): the stance torques, ``update_swing_time``, the swing legs' ``compute_swing_control_cartesian_space``,
friction compensation, the desired joint velocities with their saturation -- and ``check_apex_condition`` /
``check_full_stance_condition`` on the clocks the step leaves.  The generator's own outputs at every leg's clock are
kept too.  The fixture holds inputs and the reference's outputs only.

Cases: both generators; per leg a clock that ends at 0 (stance), inside the first half, exactly at swing_period / 2,
inside the second half, just past swing_period (advanced there, and held there); touch-down above and below lift-off;
feedback linearisation and friction compensation off in some.  Jacobians are drawn as U diag(s) V.T with singular
values in [0.1, 0.4], and the recorder asserts cond(J) <= 100 for every one, so that the reference's pseudo-inverse
and a plain inverse differ by rounding only.  That cap is a condition of the fixture, not a measurement.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "leg_control_ref.npz")
LEGS = ["FL", "FR", "RL", "RR"]
GENERATORS = ["bezier_ref", "explicit"]  # the fixture's generator codes: SRBD_SWING_BEZIER_REF, SRBD_SWING_EXPLICIT
CASES_PER_GENERATOR = 72
DT = 1.0 / 512.0  # binary: the clocks that must land exactly on swing_period / 2 do
EXACT_PERIODS = [0.25, 0.375, 0.5]
MAX_COND = 100.0
MAX_JOINT_VEL_DIFFERENCE = 10.0  # wb_interface.py:447
# the clock each leg ends the step at, as (kind, contact): the step adds DT to a swing clock below the period
KINDS = ["stance", "first_half", "half", "second_half", "past", "held"]


def jacobian(rng):
    u, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    v, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    j = u @ np.diag(rng.uniform(0.1, 0.4, 3)) @ v.T
    assert np.linalg.cond(j) <= MAX_COND, np.linalg.cond(j)
    return j


def clock_before(kind, period, rng):
    """The clock before the step such that the step's update leaves the kind's clock."""
    if kind == "stance":
        return rng.uniform(0.0, period)  # reset to 0 by the contact
    if kind == "first_half":
        return rng.uniform(0.05, 0.45) * period
    if kind == "half":
        before = period / 2.0 - DT
        assert before + DT == period / 2.0
        return before
    if kind == "second_half":
        return rng.uniform(0.55, 0.95) * period
    if kind == "past":
        return period - 0.5 * DT  # below the period: advanced to period + DT / 2
    return period + 0.25 * DT  # held: not below the period, left alone


def one_case(stc_class, rng, generator, index):
    exact = index % 2 == 0
    period = EXACT_PERIODS[(index // 2) % 3] if exact else float(rng.uniform(0.2, 0.6))
    step_height = float(rng.uniform(0.04, 0.12))
    kp, kd = (500.0, 10.0) if index % 3 else (float(rng.uniform(50, 800)), float(rng.uniform(1, 40)))
    use_fl, use_fc = int(index % 5 != 3), int(index % 7 != 4)
    kinds = [KINDS[(index + 2 * l + (l * index) // 3) % len(KINDS)] for l in range(4)]
    if index % 12 == 11:
        kinds = ["stance"] * 4  # full stance
    contact = np.array([1.0 if k == "stance" else 0.0 for k in kinds])
    before = np.array([clock_before(k, period, rng) for k in kinds])
    jac = np.stack([jacobian(rng) for _ in range(4)])
    jac_dot = rng.standard_normal((4, 3, 3)) * 0.5
    a = rng.standard_normal((4, 3, 3)) * 0.1
    mass = a @ a.transpose(0, 2, 1) + 0.05 * np.eye(3)
    q_dot = rng.standard_normal((4, 3)) * 2.0
    q_dot[index % 4] *= 8.0  # some desired joint velocities saturate
    lift_off = rng.uniform(-0.4, 0.4, (4, 3))
    touch_down = lift_off + rng.uniform(-0.15, 0.15, (4, 3))  # above and below
    foot_pos = lift_off + rng.uniform(-0.1, 0.1, (4, 3))
    foot_vel = rng.standard_normal((4, 3)) * 0.5
    passive = rng.standard_normal((4, 3)) * 0.3
    bias = rng.standard_normal((4, 3)) * 2.0
    grfs = rng.standard_normal((4, 3)) * np.array([20.0, 20.0, 80.0])
    interval = [0.01, 0.02, DT / 2.0][index % 3]

    stc = stc_class(step_height=step_height, swing_period=period, position_gain_fb=kp, velocity_gain_fb=kd,
                    generator=generator)
    stc.use_feedback_linearization = bool(use_fl)
    stc.use_friction_compensation = bool(use_fc)
    stc.swing_time = [float(t) for t in before]

    # wb_interface.py:369-372
    tau = [-np.matmul(jac[l].T, grfs[l]) for l in range(4)]
    # :374
    stc.update_swing_time(contact, LEGS, DT)
    # :377-405
    des_foot_pos = [np.zeros((3,)) for _ in range(4)]
    des_foot_vel = [np.zeros((3,)) for _ in range(4)]
    for leg_id in range(4):
        if contact[leg_id] == 0:
            tau[leg_id], des_foot_pos[leg_id], des_foot_vel[leg_id] = stc.compute_swing_control_cartesian_space(
                leg_id=leg_id, q_dot=q_dot[leg_id], J=jac[leg_id], J_dot=jac_dot[leg_id], lift_off=lift_off[leg_id],
                touch_down=touch_down[leg_id], foot_pos=foot_pos[leg_id], foot_vel=foot_vel[leg_id],
                passive_force=passive[leg_id], h=bias[leg_id], mass_matrix=mass[leg_id], early_stance_hitmoments=-1,
                early_stance_hitpoints=None)
        else:
            des_foot_pos[leg_id] = touch_down[leg_id]
            des_foot_vel[leg_id] = des_foot_vel[leg_id] * 0.0
    # :411-415
    if stc.use_friction_compensation:
        for leg_id in range(4):
            tau[leg_id] = tau[leg_id] - passive[leg_id]
    # :435-438, :461-465
    des_joint_vel = []
    for leg_id in range(4):
        v = np.linalg.pinv(jac[leg_id]) @ des_foot_vel[leg_id]
        difference = np.clip(v - q_dot[leg_id], -MAX_JOINT_VEL_DIFFERENCE, MAX_JOINT_VEL_DIFFERENCE)
        des_joint_vel.append(q_dot[leg_id] + difference)
    # the generator alone, at every leg's clock
    gen = [stc.swing_generator.compute_trajectory_references(stc.swing_time[l], lift_off[l], touch_down[l])
           for l in range(4)]
    return dict(
        generator=GENERATORS.index(generator), step_height=step_height, swing_period=period, position_gain_fb=kp,
        velocity_gain_fb=kd, use_feedback_linearization=use_fl, use_friction_compensation=use_fc,
        swing_time_before=before, contact=contact, dt=DT, apex_interval=interval, jac=jac, jac_dot=jac_dot,
        mass_matrix=mass, q_dot=q_dot, foot_pos=foot_pos, foot_vel=foot_vel, qfrc_passive=passive, qfrc_bias=bias,
        grfs=grfs, lift_off=lift_off, touch_down=touch_down,
        # the reference's outputs
        swing_time_after=np.array([float(t) for t in stc.swing_time]), tau=np.stack(tau),
        des_foot_pos=np.stack(des_foot_pos), des_foot_vel=np.stack(des_foot_vel), des_joint_vel=np.stack(des_joint_vel),
        apex=int(stc.check_apex_condition(contact, interval)), full_stance=int(stc.check_full_stance_condition(contact)),
        gen_pos=np.stack([g[0] for g in gen]), gen_vel=np.stack([g[1] for g in gen]),
        gen_acc=np.stack([g[2] for g in gen]), kinds=np.array([KINDS.index(k) for k in kinds]))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from quadruped_pympc.helpers.swing_trajectory_controller import SwingTrajectoryController

    rng = np.random.default_rng(20260)
    cases = [one_case(SwingTrajectoryController, rng, g, i) for g in GENERATORS for i in range(CASES_PER_GENERATOR)]
    data = {k: np.stack([np.asarray(c[k]) for c in cases]) for k in cases[0]}
    data["kind_names"] = np.array(KINDS)
    data["generator_names"] = np.array(GENERATORS)
    # the coverage the tests rely on
    swing = data["contact"] == 0
    for g in range(len(GENERATORS)):
        of_g = data["generator"] == g
        for k in range(len(KINDS)):
            assert ((data["kinds"] == k) & of_g[:, None]).sum() >= 8, (GENERATORS[g], KINDS[k])
        up = (data["touch_down"][..., 2] > data["lift_off"][..., 2]) & swing & of_g[:, None]
        down = (data["touch_down"][..., 2] < data["lift_off"][..., 2]) & swing & of_g[:, None]
        assert up.sum() >= 20 and down.sum() >= 20
    half = data["kinds"] == KINDS.index("half")
    assert (data["swing_time_after"][half] == (data["swing_period"][:, None] / 2.0 * np.ones((1, 4)))[half]).all()
    past = data["kinds"] == KINDS.index("past")
    assert (data["swing_time_after"][past] > (data["swing_period"][:, None] * np.ones((1, 4)))[past]).all()
    assert data["apex"].min() == 0 and data["apex"].max() == 1
    assert data["full_stance"].min() == 0 and data["full_stance"].max() == 1
    assert (data["use_feedback_linearization"] == 0).any() and (data["use_friction_compensation"] == 0).any()
    saturated = np.abs(data["des_joint_vel"] - data["q_dot"]) == MAX_JOINT_VEL_DIFFERENCE
    assert saturated.any() and not saturated.all()
    assert np.linalg.cond(data["jac"]).max() <= MAX_COND
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes, max cond(J) {np.linalg.cond(data['jac']).max():.2f}")


if __name__ == "__main__":
    main()
