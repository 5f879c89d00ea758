"""C-ABI and bindings of the device-resident gait adaptation loop (srbd_stc_touch_down_device,
srbd_batch_set_gait_device, srbd_gait_apply_freq_device, include/srbd_mpc.h; srbd_stc_touch_down, srbd_gait_apply_freq,
include/srbd_host.h).  CPU only: every SRBD_E_INVALID here is decided before a HIP call, so the dummy pointers are
never followed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped-pympc-tamols_amd", "csrc")
PTR = 0x1000  # non-null, never followed
HOST = ("srbd_stc_touch_down", "srbd_gait_apply_freq")
DEVICE = ("srbd_stc_touch_down_device", "srbd_batch_set_gait_device", "srbd_gait_apply_freq_device")
lib = _lib.lib
E_INVALID = _lib.E_INVALID


def trigger(edge=PTR, num_envs=4, current=PTR, previous=PTR, contacts=PTR, stride=12, horizon=12, lookahead=3,
            out=PTR):
    return lib.srbd_stc_touch_down_device(edge, num_envs, current, previous, contacts, stride, horizon, lookahead, out,
                                          None)


def apply(pgg=PTR, frg=PTR, stc=PTR, num_envs=4, optimize=PTR, best=PTR):
    return lib.srbd_gait_apply_freq_device(pgg, frg, stc, num_envs, optimize, best, None)


def set_gait(batch=None, no_io=False, **over):
    f = dict(pgg=PTR, timings=None, nominal_freqs=None, optimize=PTR, freq_rows=None, n_freq=3, pgg_dt=0.02,
             duty_factor=0.65, pad=0)
    f.update(over)
    io = _lib.BatchGaitIO(available=(C.c_float * _lib.MAX_FREQS)(1.4, 2.0, 2.4), **f)
    rc = lib.srbd_batch_set_gait_device(batch, None if no_io else C.byref(io), None)
    return rc, (lib.srbd_batch_last_error(None) or b"").decode()


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, names in (("srbd_mpc.h", DEVICE), ("srbd_host.h", HOST)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name in names:
            assert name in exported and name in _lib.SIGNATURES, name
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
            assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert len(_lib.SIGNATURES["srbd_stc_touch_down_device"][1]) == 10
    assert len(_lib.SIGNATURES["srbd_gait_apply_freq_device"][1]) == 7
    assert len(_lib.SIGNATURES["srbd_stc_touch_down"][1]) == 7 and len(_lib.SIGNATURES["srbd_gait_apply_freq"][1]) == 5
    for fn in (_lib.stc_touch_down_device, _lib.gait_apply_freq_device, _lib.apply_step_frequency,
               _lib.BatchContext.set_gait_device):
        assert callable(fn)
    assert lib.srbd_abi_version() == 1  # additive


def test_struct_matches_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "srbd_mpc.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(srbd_batch_gait_io), '
           'offsetof(srbd_batch_gait_io, available), offsetof(srbd_batch_gait_io, n_freq), '
           'offsetof(srbd_batch_gait_io, duty_factor), SRBD_MAX_FREQS); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "sizes.c"), os.path.join(tmp, "sizes")
        open(c, "w").write(src)
        subprocess.run(["cc", "-I", INCLUDE, c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    io = _lib.BatchGaitIO
    assert sizes == [C.sizeof(io), io.available.offset, io.n_freq.offset, io.duty_factor.offset, _lib.MAX_FREQS]
    assert C.sizeof(io) % 8 == 0


def test_headers_state_the_contract():
    text = open(os.path.join(INCLUDE, "srbd_mpc.h")).read()
    doc = text[text.index("The gait adaptation loop of the device-resident step"):
               text.index("int srbd_gait_apply_freq_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("Equivalence", "byte for byte", "bit for bit", "best_freq included", "exactly one launch",
                   "no synchronising HIP", "legacy null stream", "Stale staging",
                   "srbd_batch_set_gait or srbd_batch_clear_gait", "returns SRBD_E_INVALID", "changes nothing",
                   "swing_trajectory_controller.py:148-165", "wb_interface.py:354-358",
                   "centroidal_nmpc_jax_gait_adaptive.py:687-692", ":834-838", "may block", "1..4096",
                   "SRBD_E_INVALID (before any HIP call)", "SRBD_E_NODEVICE", "both or neither of io->pgg and io->timings",
                   "lookahead outside 1..horizon-1", "ordered exactly as two device steps are"):
        assert phrase in doc, phrase
    host = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(INCLUDE, "srbd_host.h")).read())
    for phrase in ("srbd_stc_touch_down and srbd_gait_apply_freq below", "swing_trajectory_controller.py:148-165",
                   "wb_interface.py:354-358", "NumPy 2", "zero, negative or not finite", "untouched",
                   "lookahead outside 1..horizon-1", "== 1",
                   # the srbd_stc comment keeps its other phrases
                   "np.linalg.pinv", "zero matrix", "early-stance detector", "kinodynamic", "'scipy' generator",
                   "srbd_stc_set_timing is the call it would make"):
        assert phrase in host, phrase
    shared = open(os.path.join(CSRC, "srbd_gait_adapt.h")).read()
    for phrase in ("NumPy 2.2.6", "NEP 50", "STC:148-165", "WBI:354-358", "Deviation", "untouched"):
        assert phrase in shared, phrase


def test_trigger_and_write_back_refusals_before_any_hip_call():
    for name in ("edge", "current", "previous", "contacts", "out"):
        assert trigger(**{name: None}) == E_INVALID, name
    for E in (0, -1, 4097, 2 ** 31 - 1):
        assert trigger(num_envs=E) == E_INVALID, E
        assert apply(num_envs=E) == E_INVALID, E
    for look in (0, -1, 12, 13):
        assert trigger(lookahead=look) == E_INVALID, look
    assert trigger(horizon=1, lookahead=1) == E_INVALID
    assert trigger(horizon=_lib.MAX_HORIZON + 1, stride=64) == E_INVALID
    assert trigger(stride=11) == E_INVALID
    for name in ("pgg", "optimize", "best"):
        assert apply(**{name: None}) == E_INVALID, name


def test_set_gait_device_refusals_before_any_hip_call():
    """Without a batch every call is refused; the message says for what, and the io is judged first."""
    rc, msg = set_gait(no_io=True)
    assert rc == E_INVALID and "null io" in msg
    rc, msg = set_gait(optimize=None)
    assert rc == E_INVALID and "optimize" in msg
    rc, msg = set_gait(pgg=PTR, timings=PTR)  # both
    assert rc == E_INVALID and "exactly one of pgg and timings" in msg
    rc, msg = set_gait(pgg=None, timings=None)  # neither
    assert rc == E_INVALID and "exactly one of pgg and timings" in msg
    rc, msg = set_gait(pgg=None, timings=PTR)  # phases without a nominal frequency
    assert rc == E_INVALID and "nominal_freqs" in msg
    for n in (0, 9, -1):
        rc, msg = set_gait(n_freq=n)
        assert rc == E_INVALID and "n_freq" in msg, n
    rc, msg = set_gait()  # a well-formed io
    assert rc == E_INVALID and "null batch" in msg
    rc, msg = set_gait(pgg=None, timings=PTR, nominal_freqs=PTR, freq_rows=PTR, n_freq=8)
    assert rc == E_INVALID and "null batch" in msg


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_valid_calls_reach_the_launch():
    assert trigger() == _lib.E_NODEVICE
    assert trigger(num_envs=4096, lookahead=11) == _lib.E_NODEVICE
    assert trigger(num_envs=1, lookahead=1, horizon=2, stride=2) == _lib.E_NODEVICE
    assert apply() == _lib.E_NODEVICE
    assert apply(frg=None, stc=None, num_envs=4096) == _lib.E_NODEVICE


# ------------------------------------------------------------------ the wrappers' tensor checks
E = 3


def test_wrappers_refuse_bad_tensors_before_the_device():
    edge = torch.zeros(E, dtype=torch.int32)
    c = torch.ones((E, 4), dtype=torch.float32)
    seq = torch.ones((E, 4, 12), dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        _lib.stc_touch_down_device(edge, c, c, seq)  # well-formed CPU tensors: refused for their device, last
    with pytest.raises(IndexError, match="lookahead"):
        _lib.stc_touch_down_device(edge, c, c, seq, lookahead=12)
    with pytest.raises(IndexError, match="lookahead"):
        _lib.stc_touch_down_device(edge, c, c, seq, lookahead=0)
    with pytest.raises(ValueError, match="rising_edge"):
        _lib.stc_touch_down_device(torch.zeros(0, dtype=torch.int32), c, c, seq)
    with pytest.raises(ValueError, match="rising_edge must be torch.int32"):
        _lib.stc_touch_down_device(edge.long(), c, c, seq)
    with pytest.raises(ValueError, match="current must be"):
        _lib.stc_touch_down_device(edge, c.double(), c, seq)
    with pytest.raises(ValueError, match="contacts must be"):
        _lib.stc_touch_down_device(edge, c, c, torch.ones((E, 3, 12)))
    with pytest.raises(ValueError, match="horizon"):
        _lib.stc_touch_down_device(edge, c, c, seq, horizon=13)
    pgg = torch.zeros((E, _lib.PGG_BYTES), dtype=torch.uint8)
    opt, best = torch.zeros(E, dtype=torch.int32), torch.ones(E, dtype=torch.float32)
    with pytest.raises(ValueError, match="cuda"):
        _lib.gait_apply_freq_device(pgg, opt, best)
    with pytest.raises(ValueError, match="best_freq must be torch.float32"):
        _lib.gait_apply_freq_device(pgg, opt, best.double())
    with pytest.raises(ValueError, match="optimize must be"):
        _lib.gait_apply_freq_device(pgg, opt[:2], best)
    with pytest.raises(ValueError, match="stc must be"):
        _lib.gait_apply_freq_device(pgg, opt, best, stc=torch.zeros((E, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="gait"):
        _lib.apply_step_frequency(opt, best)


def test_batched_controller_needs_a_device_only_for_its_state():
    with pytest.raises(ValueError, match="num_envs"):
        BatchedSwingTrajectoryController(0, 0.06, 0.25, 500.0, 10.0)
    assert hasattr(BatchedSwingTrajectoryController, "check_touch_down_condition")
