"""C-ABI and bindings of the device-resident velocity modulator and terrain / reference stage
(srbd_vm_modulate_device, srbd_terrain_ref_step_device, include/srbd_mpc.h; _lib.vm_modulate_device,
_lib.terrain_ref_step_device; BatchedVelocityModulator, BatchedTerrainEstimator).  CPU only: every SRBD_E_INVALID here
is decided before a HIP call, so the dummy pointers are never followed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
from quadruped_pympc_amd.helpers.velocity_modulator import BatchedVelocityModulator

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
PTR = 0x1000  # non-null, never followed
TERR_REQUIRED = ("base_pos", "com_pos", "yaws", "lin", "ang", "ref")
VM_REQUIRED = ("lin", "ang", "feet", "hips", "lin_out", "ang_out")
HOST = ("srbd_vm_modulate", "srbd_terrain_est_init", "srbd_terrain_estimate", "srbd_reference_assemble",
        "srbd_selftest_atan")
DEVICE = ("srbd_vm_modulate_device", "srbd_terrain_ref_step_device")
lib = _lib.lib


def terr(d_terrain=PTR, num_envs=4, no_io=False, feet=PTR, frg=None, ref_z=0.3, **over):
    f = dict({k: PTR for k in TERR_REQUIRED}, com_pos_offset_w=None, terrain=None, feet=feet, frg=frg, ref_z=ref_z)
    f.update(over)
    io = _lib.SrbdTerrainRefBatchIo(**f)
    return lib.srbd_terrain_ref_step_device(d_terrain, num_envs, None if no_io else C.byref(io), None)


def vm(num_envs=4, no_io=False, max_distance=0.2, **over):
    f = dict({k: PTR for k in VM_REQUIRED}, max_distance=max_distance)
    f.update(over)
    io = _lib.SrbdVmBatchIo(**f)
    return lib.srbd_vm_modulate_device(num_envs, None if no_io else C.byref(io), None)


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, names in (("srbd_mpc.h", DEVICE), ("srbd_host.h", HOST)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name in names:
            assert name in exported and name in _lib.SIGNATURES, name
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
            assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert callable(_lib.vm_modulate_device) and callable(_lib.terrain_ref_step_device)


def test_struct_sizes_match_the_headers():
    """sizeof as the C compiler sees the two headers, against the ctypes mirrors."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "srbd_mpc.h"\n#include "srbd_host.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(srbd_terrain_est), '
           'offsetof(srbd_terrain_est, height), offsetof(srbd_terrain_est, pitch_activated), '
           'sizeof(srbd_vm_batch_io), offsetof(srbd_vm_batch_io, max_distance), sizeof(srbd_terrain_ref_batch_io), '
           'offsetof(srbd_terrain_ref_batch_io, ref_z)); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "sizes.c"), os.path.join(tmp, "sizes")
        open(c, "w").write(src)
        subprocess.run(["cc", "-I", INCLUDE, c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_lib.SrbdTerrainEst), _lib.SrbdTerrainEst.height.offset,
                     _lib.SrbdTerrainEst.pitch_activated.offset, C.sizeof(_lib.SrbdVmBatchIo),
                     _lib.SrbdVmBatchIo.max_distance.offset, C.sizeof(_lib.SrbdTerrainRefBatchIo),
                     _lib.SrbdTerrainRefBatchIo.ref_z.offset]
    assert _lib.TERRAIN_EST_BYTES == C.sizeof(_lib.SrbdTerrainEst) == 32 and _lib.TERRAIN_EST_BYTES % 8 == 0
    assert C.sizeof(_lib.SrbdVmBatchIo) == 7 * 8 and C.sizeof(_lib.SrbdTerrainRefBatchIo) == 11 * 8


def test_header_states_the_contract():
    text = open(os.path.join(INCLUDE, "srbd_mpc.h")).read()
    doc = text[text.index("The velocity modulator and the terrain estimate with the reference row"):
               text.index("int srbd_terrain_ref_step_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)  # the comment's line breaks
    for phrase in ("Equivalence", "srbd_terrain_estimate(g,", "srbd_reference_assemble(g,", "exactly one launch",
                   "no synchronising HIP", "legacy null stream", "wb_interface.py:250-291", "bit for bit",
                   "NaNs position for position", "SRBD_E_INVALID (before any HIP call)", "SRBD_E_NODEVICE", "1..4096",
                   "both or neither of feet and frg", "entries 12..23 are not written", "Arrays must not overlap"):
        assert phrase in doc, phrase
    host = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(INCLUDE, "srbd_host.h")).read())
    for phrase in ("update_start_and_stop", "early-stance detector", "kinodynamic", "no abs", "within 1 ulp",
                   "srbd_terrain is the ray-cast terrain handle"):
        assert phrase in host, phrase


def test_invalid_arguments_refused_before_any_hip_call():
    """With or without a device: INVALID, never NODEVICE, and no pointer is followed."""
    E_INVALID = _lib.E_INVALID
    assert terr(d_terrain=None) == E_INVALID
    assert terr(no_io=True) == E_INVALID
    for name in TERR_REQUIRED:
        assert terr(**{name: None}) == E_INVALID, name
    assert terr(feet=None, frg=None) == E_INVALID  # neither
    assert terr(feet=PTR, frg=PTR) == E_INVALID  # both
    for E in (0, -1, 4097, 2 ** 31 - 1):
        assert terr(num_envs=E) == E_INVALID, E
        assert vm(num_envs=E) == E_INVALID, E
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert terr(ref_z=bad) == E_INVALID
    assert vm(no_io=True) == E_INVALID
    for name in VM_REQUIRED:
        assert vm(**{name: None}) == E_INVALID, name
    assert vm(max_distance=float("nan")) == E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_valid_calls_reach_the_launch():
    """Arguments that pass validation go on to the launch, which finds no device: SRBD_E_NODEVICE, not INVALID."""
    assert terr() == _lib.E_NODEVICE
    assert terr(num_envs=1, feet=None, frg=PTR) == _lib.E_NODEVICE
    assert terr(num_envs=4096, com_pos_offset_w=PTR, terrain=PTR, ref_z=-1.0) == _lib.E_NODEVICE
    assert vm() == _lib.E_NODEVICE
    assert vm(num_envs=4096, max_distance=float("inf")) == _lib.E_NODEVICE


# ------------------------------------------------------------------ the wrappers' tensor checks
E = 3


def tensors():
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    return dict(terrain=torch.zeros((E, _lib.TERRAIN_EST_BYTES), dtype=torch.uint8), base_pos=z(E, 3),
                com_pos=z(E, 3), yaws=z(E), lin=z(E, 3), ang=z(E, 3), ref=z(E, 24))


def wrapper(t, **kw):
    kw.setdefault("lift_off", torch.zeros((E, 4, 3), dtype=torch.float64))
    return _lib.terrain_ref_step_device(t["terrain"], t["base_pos"], t["com_pos"], t["yaws"], t["lin"], t["ang"],
                                        t["ref"], kw.pop("ref_z", 0.3), **kw)


def test_wrapper_refuses_bad_tensors_before_the_device():
    t = tensors()
    with pytest.raises(ValueError, match="cuda"):
        wrapper(t)  # well-formed CPU tensors: refused for their device, last
    with pytest.raises(ValueError, match="exactly one"):
        wrapper(t, lift_off=None)
    with pytest.raises(ValueError, match="exactly one"):
        wrapper(t, frg=torch.zeros((E, _lib.FRG_BYTES), dtype=torch.uint8))
    with pytest.raises(ValueError, match="ref_z"):
        wrapper(t, ref_z=float("nan"))
    with pytest.raises(ValueError, match="ref must be"):
        wrapper(dict(t, ref=torch.zeros((E, 12), dtype=torch.float64)))
    with pytest.raises(ValueError, match="yaws must be torch.float64"):
        wrapper(dict(t, yaws=torch.zeros(E, dtype=torch.float32)))
    with pytest.raises(ValueError, match="estimator state"):
        wrapper(dict(t, terrain=torch.zeros((0, _lib.TERRAIN_EST_BYTES), dtype=torch.uint8)))
    with pytest.raises(ValueError, match="frg must be"):
        wrapper(t, lift_off=None, frg=torch.zeros((E, 8), dtype=torch.uint8))
    z = torch.zeros((E, 3), dtype=torch.float64)
    legs = torch.zeros((E, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="cuda"):
        _lib.vm_modulate_device(z, z, legs, legs)
    with pytest.raises(ValueError, match="hips must be"):
        _lib.vm_modulate_device(z, z, legs, z)
    with pytest.raises(ValueError, match="NaN"):
        _lib.vm_modulate_device(z, z, legs, legs, float("nan"))
    with pytest.raises(ValueError, match="lin must be"):
        _lib.vm_modulate_device(torch.zeros((0, 3), dtype=torch.float64), z, legs, legs)


def test_batched_classes_check_their_arguments_on_the_host():
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="num_envs"):
            BatchedTerrainEstimator(bad, 0.3)
        with pytest.raises(ValueError, match="num_envs"):
            BatchedVelocityModulator(bad)
    with pytest.raises(ValueError, match="ref_z"):
        BatchedTerrainEstimator(2, float("inf"))
    with pytest.raises(ValueError, match="roll_activated"):
        BatchedTerrainEstimator(2, 0.3, roll_activated=[True, False, True])
    vm_ = BatchedVelocityModulator(E)
    assert vm_.activated is True and vm_.max_distance == 0.2
    off = BatchedVelocityModulator(E, activated=False)
    z = torch.zeros((E, 3), dtype=torch.float64)
    lin, ang = off.step(z, z, None, None)  # switched off: the command as given, no device needed
    assert lin is z and ang is z
