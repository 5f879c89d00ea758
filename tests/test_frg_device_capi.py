"""C-ABI and bindings of the device-resident foothold reference generator (srbd_frg_step_device, include/srbd_mpc.h;
_lib.frg_step_device; BatchedFootholdReferenceGenerator).  CPU only: every SRBD_E_INVALID here is decided before a HIP
call, so the dummy pointers are never followed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "srbd_mpc.h")
PTR = 0x1000  # non-null, never followed
REQUIRED = ("base_pos", "yaws", "base_lin_vel", "ref_lin_vel", "hips", "feet", "previous_contact", "current_contact",
            "seeds")
OPTIONAL = ("pgg", "com_pos_offset_w", "ref")
lib = _lib.lib


def call(d_frg=PTR, num_envs=4, no_io=False, **over):
    f = dict({k: PTR for k in REQUIRED}, **{k: None for k in OPTIONAL}, com_height_nominal=0.3, gravity=9.81)
    f.update(over)
    io = _lib.SrbdFrgBatchIo(**f)
    return lib.srbd_frg_step_device(d_frg, num_envs, None if no_io else C.byref(io), None)


def test_symbol_exported_bound_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    name = "srbd_frg_step_device"
    assert name in exported and name in _lib.SIGNATURES
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M)
    assert callable(_lib.frg_step_device)
    # the structure's layout: 10 pointers, 2 doubles, 2 pointers
    assert C.sizeof(_lib.SrbdFrgBatchIo) == 14 * 8
    assert _lib.SrbdFrgBatchIo.com_height_nominal.offset == 80 and _lib.SrbdFrgBatchIo.seeds.offset == 96


def test_header_states_the_contract():
    text = open(HEADER).read()
    doc = text[text.index("The foothold reference generator of the device-resident loop"):
               text.index("int srbd_frg_step_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)  # the comment's line breaks
    for phrase in ("Equivalence", "srbd_frg_update_lift_off, srbd_frg_update_touch_down, srbd_frg_compute",
                   "exactly one launch", "no synchronising HIP", "srbd_prepare_state_device reads it",
                   "legacy null stream", "foothold_reference_generator.py:53-199", "wb_interface.py:202-227",
                   "bit for bit", "entries 12..23", "SRBD_E_INVALID (before any HIP call)", "SRBD_E_NODEVICE",
                   "1..4096", "once on the host"):
        assert phrase in doc, phrase


def test_invalid_arguments_refused_before_any_hip_call():
    """With or without a device: INVALID, never NODEVICE, and no pointer is followed."""
    E_INVALID = _lib.E_INVALID
    assert call(d_frg=None) == E_INVALID
    assert call(no_io=True) == E_INVALID
    for name in REQUIRED:
        assert call(**{name: None}) == E_INVALID, name
    for E in (0, -1, 4097, 2 ** 31 - 1):
        assert call(num_envs=E) == E_INVALID, E
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(com_height_nominal=bad) == E_INVALID
        assert call(gravity=bad) == E_INVALID
    for bad in (0.0, -0.0, -9.81):
        assert call(gravity=bad) == E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_valid_calls_reach_the_launch():
    """Arguments that pass validation go on to the launch, which finds no device: SRBD_E_NODEVICE, not INVALID."""
    assert call() == _lib.E_NODEVICE
    assert call(num_envs=1) == _lib.E_NODEVICE
    assert call(num_envs=4096, pgg=PTR, com_pos_offset_w=PTR, ref=PTR) == _lib.E_NODEVICE
    assert call(com_height_nominal=-0.3) == _lib.E_NODEVICE  # a NaN root flows through, as on the host
    assert lib.srbd_frg_step_device(PTR, 4, C.byref(_lib.SrbdFrgBatchIo(
        **{k: PTR for k in REQUIRED}, com_height_nominal=0.3, gravity=9.81)), C.c_void_p(1)) == _lib.E_NODEVICE


# ------------------------------------------------------------------ the wrapper's tensor checks
E = 3


def good():
    f64 = torch.float64
    return dict(frg=torch.zeros(E, _lib.FRG_BYTES, dtype=torch.uint8), base_pos=torch.zeros(E, 3, dtype=f64),
                yaws=torch.zeros(E, dtype=f64), base_lin_vel=torch.zeros(E, 3, dtype=f64),
                ref_lin_vel=torch.zeros(E, 3, dtype=f64), hips=torch.zeros(E, 4, 3, dtype=f64),
                feet=torch.zeros(E, 4, 3, dtype=f64), previous_contact=torch.ones(E, 4),
                current_contact=torch.ones(E, 4), com_height_nominal=0.3, gravity=9.81)


def test_wrapper_refuses_bad_tensors_without_calling_c(monkeypatch):
    calls = []
    monkeypatch.setattr(lib, "srbd_frg_step_device", lambda *a: calls.append(a) or _lib.OK)
    f64 = torch.float64
    bad = [("frg", torch.zeros(E * _lib.FRG_BYTES, dtype=torch.uint8), "generator state"),
           ("frg", torch.zeros(E, _lib.FRG_BYTES, dtype=torch.int8), "uint8"),
           ("frg", torch.zeros(E, _lib.FRG_BYTES - 8, dtype=torch.uint8), "must be"),
           ("base_pos", torch.zeros(E, 3), "float64"), ("base_pos", torch.zeros(E, 2, dtype=f64), "must be"),
           ("yaws", torch.zeros(E, 1, dtype=f64), "must be"), ("base_lin_vel", torch.zeros(E, 2, dtype=f64), "must be"),
           ("ref_lin_vel", torch.zeros(E + 1, 3, dtype=f64), "must be"),
           ("hips", torch.zeros(E, 3, 4, dtype=f64).transpose(1, 2), "contiguous"),
           ("feet", torch.zeros(E, 12, dtype=f64), "must be"),
           ("previous_contact", torch.ones(E, 4, dtype=f64), "float32"),
           ("current_contact", torch.ones(E, 5), "must be"),
           ("pgg", torch.zeros(E, _lib.PGG_BYTES + 1, dtype=torch.uint8), "must be"),
           ("com_pos_offset_w", torch.zeros(E, 3), "float64"), ("ref", torch.zeros(E, 12, dtype=f64), "must be"),
           ("out", torch.zeros(E, 12, dtype=f64), "must be"), ("out", np.zeros((E, 4, 3)), "torch tensor"),
           ("gravity", 0.0, "gravity"), ("gravity", float("nan"), "gravity"),
           ("com_height_nominal", float("inf"), "com_height_nominal")]
    for name, value, match in bad:
        with pytest.raises(ValueError, match=match):
            _lib.frg_step_device(**dict(good(), **{name: value}))
    with pytest.raises(ValueError, match="cuda"):  # right dtypes and shapes, wrong device: refused, not copied
        _lib.frg_step_device(**good())
    assert not calls


def test_batched_class_argument_checks_are_host_only():
    lift = np.zeros((4, 3))
    for n in (0, 4097):
        with pytest.raises(ValueError, match="num_envs"):
            BatchedFootholdReferenceGenerator(n, 0.4, 0.3, lift)
    with pytest.raises(ValueError, match="stance_time"):
        BatchedFootholdReferenceGenerator(3, [0.4, 0.5], 0.3, lift)
    with pytest.raises(ValueError, match="hip_height"):
        BatchedFootholdReferenceGenerator(3, 0.4, [0.3] * 4, lift)
    with pytest.raises(ValueError, match="lift_off_positions"):
        BatchedFootholdReferenceGenerator(3, 0.4, 0.3, np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="finite"):
        BatchedFootholdReferenceGenerator(3, [0.4, float("nan"), 0.4], 0.3, lift)
    for method in ("step", "state_dict", "load_state_dict", "set_stance_time"):
        assert callable(getattr(BatchedFootholdReferenceGenerator, method))


def test_batched_class_without_a_device_raises_a_clear_error():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        BatchedFootholdReferenceGenerator(3, [0.4, 0.45, 0.5], 0.3, np.zeros((3, 4, 3)))
