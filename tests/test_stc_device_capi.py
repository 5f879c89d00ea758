"""C-ABI and bindings of the device-resident leg controller (srbd_stc_step_device, include/srbd_mpc.h;
_lib.stc_step_device; BatchedSwingTrajectoryController).  CPU only: every SRBD_E_INVALID here is decided before a HIP
call, so the dummy pointers are never followed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib, config
from quadruped_pympc_amd.helpers.swing_trajectory_controller import (BatchedSwingTrajectoryController,
                                                                     SwingTrajectoryController)

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
PTR = 0x1000  # non-null, never followed
REQUIRED = ("jac", "jac_dot", "mass_matrix", "q_dot", "foot_pos", "foot_vel", "qfrc_passive", "qfrc_bias", "grfs",
            "touch_down", "contact", "tau", "des_foot_pos", "des_foot_vel")
OPTIONAL = ("des_joint_vel", "apex", "full_stance")
HOST = ("srbd_stc_init", "srbd_stc_set_timing", "srbd_stc_update_swing_time", "srbd_stc_reference", "srbd_stc_step",
        "srbd_stc_apex", "srbd_stc_full_stance")
lib = _lib.lib


def call(d_stc=PTR, num_envs=4, dt=0.002, no_io=False, lift_off=PTR, frg=None, **over):
    f = dict({k: PTR for k in REQUIRED}, **{k: None for k in OPTIONAL}, apex_interval=0.01, lift_off=lift_off, frg=frg)
    f.update(over)
    io = _lib.SrbdStcBatchIo(**f)
    return lib.srbd_stc_step_device(d_stc, num_envs, dt, None if no_io else C.byref(io), None)


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, names in (("srbd_mpc.h", ("srbd_stc_step_device",)), ("srbd_host.h", HOST)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name in names:
            assert name in exported and name in _lib.SIGNATURES, name
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
            assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert callable(_lib.stc_step_device)


def test_struct_sizes_match_the_headers():
    """sizeof as the C compiler sees the two headers, against the ctypes mirrors."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "srbd_mpc.h"\n#include "srbd_host.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(srbd_stc), offsetof(srbd_stc, swing_time), '
           'sizeof(srbd_stc_io), sizeof(srbd_stc_batch_io), offsetof(srbd_stc_batch_io, apex_interval), '
           'offsetof(srbd_stc_io, apex_interval)); return 0; }\n')
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "sizes.c"), os.path.join(tmp, "sizes")
        open(c, "w").write(src)
        subprocess.run(["cc", "-I", INCLUDE, c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_lib.SrbdStc), _lib.SrbdStc.swing_time.offset, C.sizeof(_lib.SrbdStcIo),
                     C.sizeof(_lib.SrbdStcBatchIo), _lib.SrbdStcBatchIo.apex_interval.offset,
                     _lib.SrbdStcIo.apex_interval.offset]
    assert _lib.STC_BYTES == C.sizeof(_lib.SrbdStc) == 80 and _lib.STC_BYTES % 8 == 0
    assert C.sizeof(_lib.SrbdStcBatchIo) == 20 * 8 and _lib.SrbdStcBatchIo.tau.offset == 112
    assert (_lib.SWING_BEZIER_REF, _lib.SWING_EXPLICIT) == (0, 1)


def test_header_states_the_contract():
    text = open(os.path.join(INCLUDE, "srbd_mpc.h")).read()
    doc = text[text.index("The stance and swing leg controller of the device-resident loop"):
               text.index("int srbd_stc_step_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)  # the comment's line breaks
    for phrase in ("Equivalence", "srbd_stc_step (srbd_host.h)", "exactly one launch", "no synchronising HIP",
                   "srbd_prepare_state_device reads it", "legacy null stream", "wb_interface.py:369-415",
                   "bit for bit", "NaNs position for position", "SRBD_E_INVALID (before any HIP call)",
                   "SRBD_E_NODEVICE", "1..4096", "both or neither of lift_off and frg", "np.linalg.pinv",
                   "zero matrix", "Arrays must not overlap"):
        assert phrase in doc, phrase
    host = open(os.path.join(INCLUDE, "srbd_host.h")).read()
    for phrase in ("np.linalg.pinv", "zero matrix", "early-stance detector", "kinodynamic"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", host), phrase


def test_invalid_arguments_refused_before_any_hip_call():
    """With or without a device: INVALID, never NODEVICE, and no pointer is followed."""
    E_INVALID = _lib.E_INVALID
    assert call(d_stc=None) == E_INVALID
    assert call(no_io=True) == E_INVALID
    for name in REQUIRED:
        assert call(**{name: None}) == E_INVALID, name
    assert call(lift_off=None, frg=None) == E_INVALID  # neither
    assert call(lift_off=PTR, frg=PTR) == E_INVALID  # both
    for E in (0, -1, 4097, 2 ** 31 - 1):
        assert call(num_envs=E) == E_INVALID, E
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(dt=bad) == E_INVALID
        assert call(apex_interval=bad) == E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_valid_calls_reach_the_launch():
    """Arguments that pass validation go on to the launch, which finds no device: SRBD_E_NODEVICE, not INVALID."""
    assert call() == _lib.E_NODEVICE
    assert call(num_envs=1, lift_off=None, frg=PTR) == _lib.E_NODEVICE
    assert call(num_envs=4096, des_joint_vel=PTR, apex=PTR, full_stance=PTR) == _lib.E_NODEVICE
    assert call(dt=-0.002, apex_interval=-1.0) == _lib.E_NODEVICE  # finite is all that is asked


# ------------------------------------------------------------------ the wrapper's tensor checks
E = 3


def good():
    f64 = torch.float64
    m, v = (lambda: torch.zeros(E, 4, 3, 3, dtype=f64)), (lambda: torch.zeros(E, 4, 3, dtype=f64))
    return dict(stc=torch.zeros(E, _lib.STC_BYTES, dtype=torch.uint8), dt=0.002, jac=m(), jac_dot=m(), q_dot=v(),
                foot_pos=v(), foot_vel=v(), qfrc_passive=v(), qfrc_bias=v(), mass_matrix=m(), grfs=v(), touch_down=v(),
                contact=torch.ones(E, 4), lift_off=v())


def test_wrapper_refuses_bad_tensors_without_calling_c(monkeypatch):
    calls = []
    monkeypatch.setattr(lib, "srbd_stc_step_device", lambda *a: calls.append(a) or _lib.OK)
    f64 = torch.float64
    bad = [("stc", torch.zeros(E * _lib.STC_BYTES, dtype=torch.uint8), "controller state"),
           ("stc", torch.zeros(E, _lib.STC_BYTES, dtype=torch.int8), "uint8"),
           ("stc", torch.zeros(E, _lib.STC_BYTES - 8, dtype=torch.uint8), "must be"),
           ("jac", torch.zeros(E, 4, 3, 3), "float64"), ("jac", torch.zeros(E, 4, 9, dtype=f64), "must be"),
           ("jac_dot", torch.zeros(E, 4, 3, 3, dtype=f64).transpose(2, 3)[:, :, :, :], "must be|contiguous"),
           ("mass_matrix", torch.zeros(E + 1, 4, 3, 3, dtype=f64), "must be"),
           ("q_dot", torch.zeros(E, 12, dtype=f64), "must be"), ("foot_pos", torch.zeros(E, 4, 3), "float64"),
           ("foot_vel", torch.zeros(E, 3, 4, dtype=f64).transpose(1, 2), "contiguous"),
           ("qfrc_passive", np.zeros((E, 4, 3)), "torch tensor"), ("qfrc_bias", torch.zeros(E, 4, 2, dtype=f64), "must"),
           ("grfs", torch.zeros(E, 12, dtype=f64), "must be"), ("touch_down", torch.zeros(E, 4, 3), "float64"),
           ("contact", torch.ones(E, 4, dtype=f64), "float32"), ("contact", torch.ones(E, 5), "must be"),
           ("lift_off", torch.zeros(E, 4, 3), "float64"), ("lift_off", None, "exactly one"),
           ("frg", torch.zeros(E, _lib.FRG_BYTES, dtype=torch.uint8), "exactly one"),
           ("out", {"tau": torch.zeros(E, 12, dtype=f64)}, "must be"), ("out", {"taus": None}, "unknown output"),
           ("out", {"apex": torch.zeros(E, dtype=torch.int64)}, "int32"),
           ("dt", float("nan"), "finite"), ("apex_interval", float("inf"), "finite")]
    for name, value, match in bad:
        with pytest.raises(ValueError, match=match):
            _lib.stc_step_device(**dict(good(), **{name: value}))
    with pytest.raises(ValueError, match="must be"):  # the frg form checks the state's shape
        _lib.stc_step_device(**dict(good(), lift_off=None, frg=torch.zeros(E, 8, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="cuda"):  # right dtypes and shapes, wrong device: refused, not copied
        _lib.stc_step_device(**good())
    assert not calls


def test_batched_class_argument_checks_are_host_only():
    for n in (0, 4097):
        with pytest.raises(ValueError, match="num_envs"):
            BatchedSwingTrajectoryController(n, 0.06, 0.4, 500, 10)
    with pytest.raises(ValueError, match="step_height"):
        BatchedSwingTrajectoryController(3, [0.06, 0.07], 0.4, 500, 10)
    with pytest.raises(ValueError, match="swing_period"):
        BatchedSwingTrajectoryController(3, 0.06, [0.4] * 4, 500, 10)
    with pytest.raises(ValueError, match="position_gain_fb"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, [500, 400], 10)
    with pytest.raises(ValueError, match="velocity_gain_fb"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, [10] * 2)
    with pytest.raises(ValueError, match="generator"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, 10, ["bezier_ref", "explicit"])
    with pytest.raises(NotImplementedError, match="scipy"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, 10, "scipy")
    with pytest.raises(NotImplementedError, match="scipy"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, 10, ["bezier_ref", "scipy", "explicit"])
    for period in (0.0, float("nan")):
        with pytest.raises(ValueError, match="positive and finite"):
            BatchedSwingTrajectoryController(3, 0.06, [0.4, period, 0.4], 500, 10)
    for method in ("step", "state_dict", "load_state_dict", "regenerate_swing_trajectory_generator"):
        assert callable(getattr(BatchedSwingTrajectoryController, method))
    for method in ("regenerate_swing_trajectory_generator", "compute_swing_control_cartesian_space",
                   "update_swing_time", "check_apex_condition", "check_full_stance_condition"):
        assert callable(getattr(SwingTrajectoryController, method))


def test_batched_class_without_a_device_raises_a_clear_error():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        BatchedSwingTrajectoryController(3, 0.06, [0.4, 0.45, 0.5], 500, 10, ["bezier_ref", "explicit", "explicit"])


def test_config_carries_the_reference_values():
    sp = config.simulation_params
    assert sp["swing_generator"] == "bezier_ref"
    assert (sp["swing_position_gain_fb"], sp["swing_velocity_gain_fb"]) == (500, 10)
    assert sp["step_height"] == 0.3 * config.hip_height
