"""srbd_pgg_start_stop (include/srbd_host.h, csrc/srbd_start_stop.h) and the Python mirror's update_start_and_stop
against outputs recorded from the reference's PeriodicGaitGenerator.update_start_and_stop
(tests/golden/start_stop_ref.npz, written by tests/golden/record_start_stop_reference.py).  The fixture keeps every
quantity compared with 0.1, 0.05 or 0.06 at least 1e-9 relative away from its threshold, so the verdicts are compared
exactly; what a verdict writes is assignments and the phase arithmetic pgg_sequences.npz already pins, compared
exactly too."""
import ctypes as C
import os

import numpy as np
import pytest

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.periodic_gait_generator import PeriodicGaitGenerator

REF = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "start_stop_ref.npz"))
ARGS = ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang", "contact")
HIP_OFFSET = float(REF["hip_offset"])
lib = _lib.lib


def struct(gait, previous, phase, offset, init, duty=float(REF["duty_factor"]), freq=float(REF["step_freq"])):
    g = _lib.SrbdPgg()
    assert lib.srbd_pgg_init(C.byref(g), int(gait), duty, freq, int(REF["horizon"])) == 0
    g.previous_gait_type = int(previous)
    for l in range(4):
        g.phase_signal[l], g.phase_offset[l], g.init[l] = float(phase[l]), float(offset[l]), int(init[l])
    return g


def start_stop(g, x):
    a = [np.ascontiguousarray(x[k], dtype=np.float64) for k in ARGS]
    return lib.srbd_pgg_start_stop(C.byref(g), _lib.dptr(a[0]), _lib.dptr(a[1]), HIP_OFFSET,
                                   *[_lib.dptr(v) for v in a[2:]])


def words(g):
    return (g.gait_type, g.previous_gait_type, list(g.phase_signal), list(g.phase_offset), list(g.init))


def test_fixture_holds_the_cases_the_contract_names():
    names = [str(n) for n in REF["case_names"]]
    for conjunct in ("ref_lin", "ref_ang", "lin_vel", "ang_vel", "roll", "pitch", "contact", "FL", "FR", "RL", "RR"):
        assert sum(n.startswith(f"one_false/{conjunct}/") for n in names) >= 2, conjunct
    for gait in range(8):
        assert f"all_true/gait{gait}" in names and f"restore/to{gait}" in names
    assert sum(n.startswith("repeat/") for n in names) >= 2 and any(n.startswith("underflow/") for n in names)
    for group in ARGS:
        assert any(n.startswith(f"nan/{group}") for n in names), group
    yaws = REF["case_euler"][[n.startswith("all_true/yaw") for n in names], 2]
    assert {(bool(np.cos(y) > 0), bool(np.sin(y) > 0)) for y in yaws if np.sin(y) * np.cos(y) != 0} == {
        (True, True), (True, False), (False, True), (False, False)}
    assert set(REF["case_action"].tolist()) == {0, 1, 2} and float(REF["margin"]) == 1e-9


@pytest.mark.parametrize("mirror", [False, True])
def test_single_calls_equal_the_reference(mirror):
    for i, name in enumerate(REF["case_names"]):
        x = {k: REF[f"case_{k}"][i] for k in ARGS}
        before = [REF[f"case_before_{k}"][i] for k in ("gait", "previous", "phase", "offset", "init")]
        if mirror:
            p = PeriodicGaitGenerator(float(REF["duty_factor"]), float(REF["step_freq"]), int(before[0]),
                                      int(REF["horizon"]))
            p.previous_gait_type = int(before[1])
            p.set_phase_signal(before[2], before[4])
            for l in range(4):
                p._g.phase_offset[l] = float(before[3][l])
            action = p.update_start_and_stop(x["feet"], x["hips"], HIP_OFFSET, x["base_pos"], x["euler"], x["lin_vel"],
                                             x["ang_vel"], x["ref_lin"], x["ref_ang"], x["contact"])
            g = p._g
        else:
            g = struct(*before)
            action = start_stop(g, x)
        assert action == REF["case_action"][i], name
        got = words(g)
        assert got[0] == REF["case_after_gait"][i] and got[1] == REF["case_after_previous"][i], name
        assert got[2] == REF["case_after_phase"][i].tolist() and got[3] == REF["case_after_offset"][i].tolist(), name
        assert got[4] == REF["case_after_init"][i].tolist(), name
        if action == 0:  # nothing is written
            assert got == (int(before[0]), int(before[1]), before[2].tolist(), before[3].tolist(), before[4].tolist())


def test_sequences_equal_the_reference_step_for_step():
    """update_start_and_stop, run, compute_contact_sequence: after each step the generator's words and the contact
    sequence are the reference's, exactly; the current contact fed back is column 0 of the sequence."""
    steps, H = int(REF["seq_steps"]), int(REF["horizon"])
    for n, gait in enumerate(REF["seq_gaits"]):
        p = PeriodicGaitGenerator(float(REF["seq_duty"][n]), float(REF["seq_freq"][n]), int(gait), H)
        dts, lens = REF[f"seq_dts{n}"], REF[f"seq_lens{n}"]
        current = np.ones(4)
        for i in range(n * steps, (n + 1) * steps):
            x = {k: REF[f"seq_{k}"][i] for k in ARGS}
            assert np.array_equal(x["contact"], current), i
            action = p.update_start_and_stop(x["feet"], x["hips"], HIP_OFFSET, x["base_pos"], x["euler"], x["lin_vel"],
                                             x["ang_vel"], x["ref_lin"], x["ref_ang"], current)
            assert action == REF["seq_action"][i], i
            p.run(float(REF["seq_dt"][n]), p.step_freq)
            seq = p.compute_contact_sequence(dts, lens)
            cols = int(REF["seq_cols"][i])
            assert seq.shape == (4, cols) and np.array_equal(seq, REF["seq_contacts"][i][:, :cols]), i
            assert p.gait_type == REF["seq_gait"][i] and p.previous_gait_type == REF["seq_previous"][i], i
            assert np.array_equal(p.phase_signal, REF["seq_phase"][i]), i
            assert p.phase_offset == REF["seq_offset"][i].tolist(), i
            assert np.array_equal(p._init.astype(np.int32), REF["seq_init"][i]), i
            current = seq[:, 0].copy()
        acts = REF["seq_action"][n * steps:(n + 1) * steps].tolist()
        assert 1 in acts and 2 in acts and acts[-1] == 0  # walk, stop, stand, walk


def test_invalid_arguments_are_refused_and_nothing_is_written():
    x = {k: np.ascontiguousarray(REF[f"case_{k}"][0], dtype=np.float64) for k in ARGS}
    ptrs = [_lib.dptr(x[k]) for k in ARGS]
    g = struct(0, 0, [0.1, 0.2, 0.3, 0.4], [0.5, 1.0, 1.0, 0.5], [0, 1, 0, 0])
    before = bytes(g)
    assert lib.srbd_pgg_start_stop(None, ptrs[0], ptrs[1], HIP_OFFSET, *ptrs[2:]) == _lib.E_INVALID
    for k in range(len(ptrs)):
        bad = list(ptrs)
        bad[k] = None
        assert lib.srbd_pgg_start_stop(C.byref(g), bad[0], bad[1], HIP_OFFSET, *bad[2:]) == _lib.E_INVALID, ARGS[k]
        assert bytes(g) == before
    p = PeriodicGaitGenerator(0.65, 1.4, 0, 12)
    assert p.start_and_stop_activated is False
    with pytest.raises(ValueError):
        p.update_start_and_stop(np.zeros((3, 3)), x["hips"], HIP_OFFSET, x["base_pos"], x["euler"], x["lin_vel"],
                                x["ang_vel"], x["ref_lin"], x["ref_ang"], x["contact"])
