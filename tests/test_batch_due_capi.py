"""C-ABI and binding of the due mask of the batch's device steps (srbd_batch_step_masked_device,
srbd_batch_step_cem_masked_device, srbd_batch_interface_step_masked_device, include/srbd_mpc.h; mpc_due).  CPU only:
every check here is decided before a device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib
from test_batch_device_capi import fake_io, last_error

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "srbd_mpc.h")
DESIGN = os.path.join(ROOT, "DESIGN.md")
DUE = 0x2000  # a non-null address that is never followed (the checks come first)

DECLARED = {
    "srbd_batch_step_masked_device":
        "int srbd_batch_step_masked_device(srbd_batch* b, const srbd_batch_device_io* io, const int32_t* due, "
        "void* hip_stream);",
    "srbd_batch_step_cem_masked_device":
        "int srbd_batch_step_cem_masked_device(srbd_batch* b, const srbd_batch_device_io* io, "
        "const srbd_batch_cem_io* cem, const int32_t* due, void* hip_stream);",
    "srbd_batch_interface_step_masked_device":
        "int srbd_batch_interface_step_masked_device(srbd_batch* b, const srbd_batch_interface_io* io, "
        "const int32_t* due, void* hip_stream);",
}
P_ = C.c_void_p
BOUND = {
    "srbd_batch_step_masked_device": [P_, C.POINTER(_lib.BatchDeviceIO), P_, P_],
    "srbd_batch_step_cem_masked_device": [P_, C.POINTER(_lib.BatchDeviceIO), C.POINTER(_lib.BatchCemIO), P_, P_],
    "srbd_batch_interface_step_masked_device": [P_, C.POINTER(_lib.BatchInterfaceIO), P_, P_],
}


def flat(text):
    """One line: the comment leaders of the header's block comments and every run of white space folded."""
    return re.sub(r"\s+", " ", re.sub(r"\n \* ?", " ", text))


def fake_iface_io():
    io = _lib.BatchInterfaceIO()
    for name, ctype in _lib.BatchInterfaceIO._fields_:
        if ctype is C.c_void_p and name not in ("gait", "sigma", "costs"):
            setattr(io, name, 0x1000)
    io.contact_stride, io.iterations, io.params_per_leg = 12, 1, 36
    return io


def test_symbols_exported_with_the_declared_signatures():
    """Fails without the feature: the library exports no such symbols."""
    header = flat(open(HEADER).read())
    for name, decl in DECLARED.items():
        assert decl in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
        fn = getattr(_lib.lib, name)
        assert fn.restype == C.c_int and fn.argtypes == _lib.SIGNATURES[name][1] == BOUND[name], name
    assert callable(_lib.BatchContext.step_masked_device) and callable(_lib.BatchContext.interface_step_masked_device)
    assert callable(_lib.CemBatchContext.step_cem_masked_device)


def test_no_field_was_added_to_the_io_structures():
    assert C.sizeof(_lib.BatchDeviceIO) == 8 * 14 + 2 * 4
    assert C.sizeof(_lib.BatchCemIO) == 16
    assert [f[0] for f in _lib.BatchInterfaceIO._fields_][-1] == "costs"
    assert C.sizeof(_lib.BatchInterfaceIO) == 8 * 19 + 4 * 6


def test_step_masked_refusals_name_their_argument():
    lib = _lib.lib
    for name, call in (("srbd_batch_step_masked_device", lambda io, due: lib.srbd_batch_step_masked_device(
                            None, io, due, None)),
                       ("srbd_batch_step_cem_masked_device", lambda io, due: lib.srbd_batch_step_cem_masked_device(
                            None, io, C.byref(_lib.BatchCemIO(sigma=0x1000, sigma_reset=0.0, pad=0)), due, None))):
        unmasked = name.replace("_masked", "")
        assert call(None, DUE) == _lib.E_INVALID
        assert last_error() == name + ": null io"
        assert call(C.byref(fake_io()), None) == _lib.E_INVALID
        msg = last_error()
        assert msg.startswith(name + ": null due") and unmasked + ")" in msg
        assert call(C.byref(fake_io()), DUE) == _lib.E_INVALID
        assert last_error() == name + ": null batch"
        assert call(C.byref(fake_io(grf=None)), DUE) == _lib.E_INVALID
        assert last_error() == name + ": null required pointer: grf"
    assert lib.srbd_batch_step_cem_masked_device(None, C.byref(fake_io()), None, DUE, None) == _lib.E_INVALID
    assert last_error() == "srbd_batch_step_cem_masked_device: null cem"


def test_interface_step_masked_refusals_name_their_argument():
    lib, name = _lib.lib, "srbd_batch_interface_step_masked_device"
    assert lib.srbd_batch_interface_step_masked_device(None, None, DUE, None) == _lib.E_INVALID
    assert last_error() == name + ": null io"
    assert lib.srbd_batch_interface_step_masked_device(None, C.byref(fake_iface_io()), None, None) == _lib.E_INVALID
    msg = last_error()
    assert msg.startswith(name + ": null due") and "srbd_batch_interface_step_device)" in msg
    assert lib.srbd_batch_interface_step_masked_device(None, C.byref(fake_iface_io()), DUE, None) == _lib.E_INVALID
    assert last_error() == name + ": null batch"
    # the unmasked calls' messages keep their names
    assert lib.srbd_batch_interface_step_device(None, C.byref(fake_iface_io()), None) == _lib.E_INVALID
    assert last_error() == "srbd_batch_interface_step_device: null batch"
    assert lib.srbd_batch_step_device(None, C.byref(fake_io()), None) == _lib.E_INVALID
    assert last_error() == "srbd_batch_step_device: null batch"


def test_header_and_design_state_the_contract():
    header, design = flat(open(HEADER).read()), flat(open(DESIGN).read())
    block = header[header.index("The due mask"):header.index("int srbd_batch_step_masked_device(")]
    for phrase in ("neither written nor read", "arrival count", "Out of scope", "quadruped_pympc_wrapper.py :134",
                   "Launches:", "Equivalence", "SRBD_E_INVALID"):
        assert phrase in block, phrase
    section = design[design.index("The due mask"):]
    for phrase in ("neither written nor read", "arrival count"):
        assert phrase in section, phrase
    assert "srbd_batch_step_masked_device" in design[design.index("## 8"):]


# ------------------------------------------------------------------ mpc_due
@pytest.mark.parametrize("dt,hz,period", [(0.002, 100.0, 5), (0.002, 500.0, 1), (0.004, 100.0, 2)])
def test_mpc_due_is_the_references_expression(dt, hz, period):
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import mpc_due

    assert round(1 / (hz * dt)) == period  # 0.004 s at 100 Hz: the quotient 2.5 rounds to the even integer
    step_num = torch.tensor([0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 4999, 5000], dtype=torch.int64)
    due = mpc_due(step_num, dt, hz)
    want = [int(n % round(1 / (hz * dt)) == 0) for n in step_num.tolist()]
    assert due.dtype == torch.int32 and tuple(due.shape) == tuple(step_num.shape) and due.tolist() == want
    assert due[0].item() == 1  # the first step of an episode solves
    assert mpc_due(step_num.to(torch.int32), dt, hz).tolist() == want


# ------------------------------------------------------------------ the bindings' checks of due
E, N, H, P = 3, 100, 12, 144


@pytest.fixture
def hollow_batch(monkeypatch):
    """A BatchContext of E = 3 that owns no srbd_batch; the C functions record their calls."""
    calls = []
    for name in DECLARED:
        monkeypatch.setattr(_lib.lib, name, lambda *a: calls.append(a) or _lib.OK)
    b = _lib.BatchContext.__new__(_lib.BatchContext)
    b.E, b.N, b.P, b.h = E, N, P, None
    b.cfg = _lib.make_config(num_samples=N, horizon=H, method="mppi", parametrization="zero_order", mass=15.0,
                             inertia=np.eye(3), dts=np.full(H, 0.02))
    return b, calls


@pytest.mark.parametrize("due,match", [
    (lambda: torch.ones(E, dtype=torch.int64), "int32"),
    (lambda: torch.ones(E, dtype=torch.float32), "int32"),
    (lambda: torch.ones(E + 1, dtype=torch.int32), "must be"),
    (lambda: torch.ones(E, 1, dtype=torch.bool), "must be"),
    (lambda: torch.ones(2 * E, dtype=torch.int32)[::2], "contiguous"),
    (lambda: np.ones(E, np.int32), "torch tensor"),
    (lambda: torch.ones(E, dtype=torch.int32), "must be on cuda:0"),
    (lambda: torch.ones(E, dtype=torch.bool), "must be on cuda:0"),
])
def test_due_is_checked_before_the_c_call(hollow_batch, due, match):
    b, calls = hollow_batch
    with pytest.raises(ValueError, match=match):
        b.check_due(due())
    assert not calls


def test_controller_classes_take_the_due_keyword():
    import inspect

    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_gait_adaptive_batched import \
        Batched_Sampling_MPC as Batched_GA
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import Batched_SRBDControllerInterface

    for cls in (Batched_Sampling_MPC, Batched_CEM_Sampling_MPC, Batched_GA, Batched_SRBDControllerInterface):
        p = inspect.signature(cls.compute_control_device).parameters["due"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, cls
