#!/usr/bin/env python3
"""Record the reference's velocity modulator, terrain estimator and reference row into tests/golden/terrain_ref.npz.

TEST INFRASTRUCTURE ONLY.  Run by hand on a machine that has a checkout of the reference and scipy; no test runs it:

    python tests/golden/record_terrain_reference.py /path/to/reference-checkout

It loads the reference's ``TerrainEstimator`` (quadruped_pympc/helpers/terrain_estimator.py) and ``VelocityModulator``
(quadruped_pympc/helpers/velocity_modulator.py) by path, the latter behind a stand-in ``quadruped_pympc.config`` module
(``simulation_params['velocity_modulator']`` and ``robot``), and composes the estimator with the lines of
``WBInterface.update_state_and_reference`` that build the reference row from it
(quadruped_pympc/interfaces/wb_interface.py:250-291), scipy's ``Rotation.from_euler`` included.  The fixture holds
inputs and the reference's outputs only.

Modulator cases (``vm_case``): 0 standing, both entries below 0.01; 1 one negative entry, the other >= 0.01; 2 moving
and no leg beyond 0.2; 3..6 a trigger from leg FL, FR, RL, RR alone; 7 a NaN distance (the other legs inside); 8 a
trigger with negative entries in the command, so that -0.0 appears.

Estimator sequences (``te_kind``) of STEPS steps each, so that the filters carry: 0 random feet, the filters from
zero; 1 the pitch filter seeded above 0.2; 2 seeded below -0.2; 3 roll switched on, both filters seeded; 4 a
denominator of exactly zero with a non-zero numerator at step ZERO_STEP (arctan(inf) = pi / 2); 5 a 0 / 0 at step
ZERO_STEP, whose NaN persists.  The recorder refuses to write unless every case is reached: both signs of each sign
test, pitch > 0 and <= 0, |pitch| above and below 0.2, roll on, the pi / 2 and the persisting NaN.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "terrain_ref.npz")
LEGS = ["FL", "FR", "RL", "RR"]
STEPS = 10
ZERO_STEP = 3
SEQUENCES_PER_KIND = 4
MAX_DISTANCE = 0.2
HIPS = np.array([[0.19, 0.11, 0.3], [0.19, -0.11, 0.3], [-0.19, 0.11, 0.3], [-0.19, -0.11, 0.3]])


def load_reference(checkout):
    """(TerrainEstimator, VelocityModulator) with the reference's two files executed under a stand-in config."""
    qp = types.ModuleType("quadruped_pympc")
    qp.__path__ = []
    cfg = types.ModuleType("quadruped_pympc.config")
    cfg.simulation_params = {"velocity_modulator": True}
    cfg.robot = "go2"
    qp.config = cfg
    sys.modules.update({"quadruped_pympc": qp, "quadruped_pympc.config": cfg})
    mods = []
    for name in ("terrain_estimator", "velocity_modulator"):
        path = os.path.join(checkout, "quadruped_pympc", "helpers", name + ".py")
        spec = importlib.util.spec_from_file_location("reference_" + name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[0].TerrainEstimator, mods[1].VelocityModulator


def legs(table):
    return types.SimpleNamespace(**{k: table[l].copy() for l, k in enumerate(LEGS)})


def modulator_cases(vm_class, rng):
    vm = vm_class()
    assert vm.activated is True and vm.max_distance == MAX_DISTANCE
    rows = []

    def add(case, lin, ang, offsets):
        hips = HIPS + rng.uniform(-0.5, 0.5, 3)
        feet = hips + np.asarray(offsets, dtype=np.float64)
        lin, ang = np.asarray(lin, dtype=np.float64), np.asarray(ang, dtype=np.float64)
        lo, ao = vm.modulate_velocities(lin.copy(), ang.copy(), legs(feet), legs(hips))
        rows.append((case, lin, ang, feet, hips, np.array(lo), np.array(ao)))

    def inside():
        r, a = rng.uniform(0.0, 0.19, 4), rng.uniform(0, 2 * np.pi, 4)
        return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.3, 0.0, 4)], axis=1)

    def beyond(l, off):
        r, a = rng.uniform(0.21, 0.4), rng.uniform(0, 2 * np.pi)
        off[l, 0:2] = r * np.cos(a), r * np.sin(a)
        return off

    for _ in range(6):
        ang = rng.uniform(-1, 1, 3)
        add(0, [rng.uniform(-0.5, 0.0099), rng.uniform(-0.5, 0.0099), 0.0], ang, beyond(int(rng.integers(4)), inside()))
        add(1, [rng.uniform(-0.5, -0.02), rng.uniform(0.01, 0.5), 0.0], ang, beyond(int(rng.integers(4)), inside()))
        add(1, [rng.uniform(0.01, 0.5), rng.uniform(-0.5, -0.02), 0.0], ang, inside())
        add(2, [rng.uniform(0.01, 0.5), rng.uniform(0.01, 0.5), rng.uniform(-0.1, 0.1)], ang, inside())
        for l in range(4):
            add(3 + l, [rng.uniform(0.01, 0.5), rng.uniform(0.01, 0.5), rng.uniform(0.0, 0.1)], np.abs(ang),
                beyond(l, inside()))
        off = inside()
        off[int(rng.integers(4)), int(rng.integers(2))] = np.nan
        add(7, [rng.uniform(0.01, 0.5), rng.uniform(0.01, 0.5), 0.0], ang, off)
        add(8, [rng.uniform(0.01, 0.5), rng.uniform(-0.5, -0.02), -0.05], -np.abs(ang),
            beyond(int(rng.integers(4)), inside()))
    add(0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], inside())
    add(2, [0.01, 0.01, 0.0], [0.0, 0.0, 0.3], inside())  # the early return's own bound: 0.01 is not below 0.01
    cols = list(zip(*rows))
    out = {"vm_case": np.array(cols[0], dtype=np.int32)}
    for name, col in zip(("vm_lin", "vm_ang", "vm_feet", "vm_hips", "vm_lin_out", "vm_ang_out"), cols[1:]):
        out[name] = np.array(col, dtype=np.float64)
    # every case is reached, and does what its name says
    case, lin_out, lin = out["vm_case"], out["vm_lin_out"], out["vm_lin"]
    assert set(case.tolist()) == set(range(9)), sorted(set(case.tolist()))
    same = np.array([np.array_equal(a, b) for a, b in zip(lin_out, lin)])
    assert same[np.isin(case, (0, 2, 7))].all() and not same[np.isin(case, (3, 4, 5, 6, 8))].any()
    assert not same[case == 1].all() and same[case == 1].any()
    assert np.isnan(out["vm_feet"][case == 7]).any()
    assert (np.signbit(lin_out[case == 8]) & (lin_out[case == 8] == 0.0)).any(), "no -0.0 in the modulated command"
    return out


def estimator_sequences(te_class, rng):
    from scipy.spatial.transform import Rotation as R

    seqs = []
    seen = {"roll_neg": 0, "roll_pos": 0, "pitch_neg": 0, "pitch_pos": 0, "pitch>0": 0, "pitch<=0": 0, "|pitch|>0.2": 0,
            "|pitch|<=0.2": 0, "roll_on": 0, "pi/2": 0, "nan_persists": 0}
    for kind in range(6):
        for _ in range(SEQUENCES_PER_KIND):
            te = te_class()
            init = np.zeros(3)
            if kind == 1:
                init[1] = rng.uniform(0.25, 0.5)
            elif kind == 2:
                init[1] = -rng.uniform(0.25, 0.5)
            elif kind == 3:
                te.roll_activated = True
                init[0:2] = rng.uniform(-0.4, 0.4, 2)
                seen["roll_on"] += 1
            init[2] = rng.uniform(-0.1, 0.3)
            te.terrain_roll, te.terrain_pitch, te.terrain_height = (float(v) for v in init)
            ref_z = float(rng.uniform(0.25, 0.6))
            rec = {k: [] for k in ("base", "yaw", "feet", "lin", "ang", "com", "com_off", "terrain", "ref")}
            for step in range(STEPS):
                base = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.2, 0.6)])
                yaw = float(rng.uniform(-3.2, 3.2))
                slope = rng.uniform(-0.6, 0.6, 2)  # the ground's gradient, so that both signs of each test are reached
                c, s = np.cos(yaw), np.sin(yaw)
                feet = np.empty((4, 3))
                for l in range(4):
                    h = HIPS[l, 0:2] + rng.uniform(-0.08, 0.08, 2)
                    feet[l, 0] = base[0] + c * h[0] - s * h[1]
                    feet[l, 1] = base[1] + s * h[0] + c * h[1]
                    feet[l, 2] = slope[0] * h[0] + slope[1] * h[1] + rng.uniform(-0.02, 0.02)
                if kind >= 4 and step == ZERO_STEP:
                    # yaw 0 and base 0: the rotation returns the feet; left x = 0.0 - 0.001, and left x + 0.001 == 0
                    base, yaw = np.zeros(3), 0.0
                    feet[0, 0], feet[2, 0] = 0.0, 0.001
                    if kind == 5:
                        feet[2, 2] = feet[0, 2]  # and left z = 0: 0 / 0
                    else:
                        assert feet[0, 2] != feet[2, 2]
                lin, ang = rng.uniform(-0.6, 0.6, 3), rng.uniform(-1, 1, 3)
                com = base + rng.uniform(-0.03, 0.03, 3)
                com_off = rng.uniform(-0.02, 0.02, 3) if step % 2 else np.zeros(3)
                lift_off = {k: feet[l].copy() for l, k in enumerate(LEGS)}
                # ---- wb_interface.py:250-291, line by line
                terrain_roll, terrain_pitch, terrain_height = te.compute_terrain_estimation(
                    base_position=base, yaw=yaw, feet_pos=lift_off, current_contact=np.ones(4))
                ref_pos = np.array([0, 0, ref_z])
                ref_pos[2] = ref_z + terrain_height
                ref_base_lin_vel = R.from_euler("xyz", [terrain_roll, terrain_pitch, 0]).as_matrix() @ lin
                if terrain_pitch > 0.0:
                    ref_base_lin_vel[2] = -ref_base_lin_vel[2]
                if np.abs(terrain_pitch) > 0.2:
                    ref_base_lin_vel[0] = ref_base_lin_vel[0] / 2.
                    ref_base_lin_vel[2] = ref_base_lin_vel[2] * 2
                ref_pos[2] -= base[2] - (com[2] + com_off[2])
                row = np.concatenate([ref_pos, ref_base_lin_vel, np.array([terrain_roll, terrain_pitch, 0.0]), ang])
                # ----
                for k, v in (("base", base), ("yaw", yaw), ("feet", feet), ("lin", lin), ("ang", ang), ("com", com),
                             ("com_off", com_off), ("terrain", [terrain_roll, terrain_pitch, terrain_height]),
                             ("ref", row)):
                    rec[k].append(np.array(v, dtype=np.float64))
                # which branches this step took (the estimator's sign tests are restated only to count them)
                z = feet[:, 2]
                if not np.isnan(terrain_pitch):
                    seen["roll_neg" if (z[0] - z[1]) * 0.5 + (z[2] - z[3]) * 0.5 < 0 else "roll_pos"] += 1
                    seen["pitch_neg" if (z[0] - z[2]) * 0.5 + (z[1] - z[3]) * 0.5 > 0 else "pitch_pos"] += 1
                    seen["pitch>0" if terrain_pitch > 0.0 else "pitch<=0"] += 1
                    seen["|pitch|>0.2" if np.abs(terrain_pitch) > 0.2 else "|pitch|<=0.2"] += 1
                if kind == 4 and step == ZERO_STEP:
                    before = rec["terrain"][-2][1]
                    raw = (terrain_pitch - before * 0.99) / 0.01  # about +-(pi / 2 + other) / 2: above pi / 4
                    seen["pi/2"] += int(abs(raw) > np.pi / 4)
                if kind == 5 and step == STEPS - 1:
                    seen["nan_persists"] += int(np.isnan(terrain_pitch) and not np.isnan(rec["terrain"][ZERO_STEP - 1][1]))
            seqs.append((kind, int(te.roll_activated), init, ref_z, rec))
    missing = [k for k, n in seen.items() if n == 0]
    assert not missing, f"cases not reached: {missing}"
    out = {"te_kind": np.array([q[0] for q in seqs], dtype=np.int32),
           "te_roll_activated": np.array([q[1] for q in seqs], dtype=np.int32),
           "te_init": np.array([q[2] for q in seqs]), "te_ref_z": np.array([q[3] for q in seqs])}
    for k in ("base", "yaw", "feet", "lin", "ang", "com", "com_off", "terrain", "ref"):
        out["te_" + k] = np.array([q[4][k] for q in seqs], dtype=np.float64)
    return out, seen


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    te_class, vm_class = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261020)
    data = modulator_cases(vm_class, rng)
    te, seen = estimator_sequences(te_class, rng)
    data.update(te)
    data["max_distance"] = np.float64(MAX_DISTANCE)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {data['vm_case'].size} modulator cases, {data['te_kind'].size} sequences of {STEPS} steps; "
          f"{os.path.getsize(OUT)} bytes; reached {seen}")


if __name__ == "__main__":
    main()
