"""C-ABI and bindings of the per-environment reset on the device (srbd_loop_reset_device, include/srbd_mpc.h;
_lib.loop_reset_device; helpers/loop_reset.py BatchedLoopReset).  CPU only: every SRBD_E_INVALID here is decided before
a HIP call, so the dummy pointers are never followed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.loop_reset import BatchedLoopReset, mask_words
from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
PTR = 0x1000  # non-null, 8-byte aligned, never followed
lib = _lib.lib
E_INVALID = _lib.E_INVALID
NAMES = ("pgg", "frg", "stc", "terrain_est", "vfa")


def call(num_envs=4, no_io=False, rows=0, **over):
    f = dict(mask=PTR, initial_feet=PTR, rising_edge=PTR, best_params=PTR, num_params=36, n_contact_rows=rows)
    for n in NAMES:
        f[n] = f[n + "_snapshot"] = PTR
    f.update(over)
    row_ptrs = f.pop("contact_rows", [PTR] * max(0, min(rows, 4)))
    io = _lib.SrbdLoopResetIo(**f)
    for i, p in enumerate(row_ptrs):
        io.contact_rows[i] = p
    rc = lib.srbd_loop_reset_device(num_envs, None if no_io else C.byref(io), None)
    return rc, _lib.last_error(None)


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, name, nargs in (("srbd_mpc.h", "srbd_loop_reset_device", 3), ("srbd_host.h", "srbd_loop_reset", 15)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        assert name in exported and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert lib.srbd_abi_version() == 1  # additive
    assert (_lib.RESET_REFERENCE, _lib.RESET_EPISODE) == (1, 2)


def test_io_struct_layout_matches_the_header():
    """sizeof and every field offset of srbd_loop_reset_io as the C compiler lays it out."""
    fields = [n for n, _ in _lib.SrbdLoopResetIo._fields_]
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"srbd_host.h\"\n#include \"srbd_mpc.h\"\nint main(void){\n"
    src += 'printf("%zu\\n", sizeof(srbd_loop_reset_io));\n'
    for n in fields:
        src += f'printf("%zu\\n", offsetof(srbd_loop_reset_io, {n}));\n'
    src += "return 0;}\n"
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.SrbdLoopResetIo) == 18 * 8 + 8
    assert got[1:] == [getattr(_lib.SrbdLoopResetIo, n).offset for n in fields]
    assert fields[:2] == ["mask", "initial_feet"] and fields[-2:] == ["num_params", "n_contact_rows"]


def test_invalid_arguments_refused_before_any_hip_call_with_a_message():
    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc == E_INVALID and msg.startswith("srbd_loop_reset_device: ") and what in msg, (kw, rc, msg)

    for E in (0, -1, 4097, 2 ** 31 - 1):
        refused("num_envs", num_envs=E)
    refused("null io", no_io=True)
    refused("null mask", mask=None)
    for n in (-1, 5, 2 ** 31 - 1):
        refused("n_contact_rows", rows=n, contact_rows=[PTR] * 4)
    refused("null contact row", rows=3, contact_rows=[PTR, None, PTR])
    refused("initial_feet", initial_feet=None)
    for n in NAMES:  # stricter than the host call: a struct without its snapshot, whatever the levels are
        refused("without its snapshot", **{n + "_snapshot": None})
    for bad in (0, -1, -(2 ** 31)):
        refused("num_params", num_params=bad)
    for n in NAMES:
        refused("8-byte aligned", **{n: PTR + 4})
        refused("8-byte aligned", **{n + "_snapshot": PTR + 2})


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_valid_calls_reach_the_launch():
    assert call()[0] == _lib.E_NODEVICE
    assert call(num_envs=1)[0] == _lib.E_NODEVICE and call(num_envs=4096, rows=4)[0] == _lib.E_NODEVICE
    for n in NAMES:  # every piece is optional, with its snapshot
        assert call(**{n: None, n + "_snapshot": None})[0] == _lib.E_NODEVICE, n
        assert call(**{n: None})[0] == _lib.E_NODEVICE, n  # a snapshot alone is ignored
    assert call(frg=None, initial_feet=None)[0] == _lib.E_NODEVICE
    assert call(best_params=None, num_params=0, rising_edge=None)[0] == _lib.E_NODEVICE
    none = {n: None for n in NAMES}
    assert call(initial_feet=None, best_params=None, rising_edge=None, **none)[0] == _lib.E_NODEVICE


def test_wrapper_checks_its_arguments_on_the_host():
    E = 5
    mask = torch.zeros(E, dtype=torch.int32)
    pgg = torch.zeros((E, _lib.PGG_BYTES), dtype=torch.uint8)
    frg = torch.zeros((E, _lib.FRG_BYTES), dtype=torch.uint8)
    feet = torch.zeros((E, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="cuda"):  # well-formed host tensors: refused for their device, last
        _lib.loop_reset_device(mask, feet, pgg=pgg, frg=frg, snapshots={"pgg": pgg.clone(), "frg": frg.clone()})
    with pytest.raises(ValueError, match="mask must be"):
        _lib.loop_reset_device(torch.zeros((E, 1), dtype=torch.int32))
    with pytest.raises(ValueError, match="mask must be torch.int32"):
        _lib.loop_reset_device(torch.zeros(E, dtype=torch.int64))
    with pytest.raises(ValueError, match="pgg is given without its snapshot"):
        _lib.loop_reset_device(mask, pgg=pgg)
    with pytest.raises(ValueError, match="unknown snapshot 'gait'"):
        _lib.loop_reset_device(mask, pgg=pgg, snapshots={"gait": pgg})
    with pytest.raises(ValueError, match="frg is given without initial_feet"):
        _lib.loop_reset_device(mask, frg=frg, snapshots={"frg": frg})
    with pytest.raises(ValueError, match=r"snapshots\['pgg'\] must be"):
        _lib.loop_reset_device(mask, pgg=pgg, snapshots={"pgg": pgg[:3]})
    with pytest.raises(ValueError, match="initial_feet must be"):
        _lib.loop_reset_device(mask, feet[:, :3], frg=frg, snapshots={"frg": frg})
    with pytest.raises(ValueError, match="best_params must be"):
        _lib.loop_reset_device(mask, best_params=torch.zeros(E, dtype=torch.float32))
    with pytest.raises(ValueError, match="at most 4 contact rows"):
        _lib.loop_reset_device(mask, contact_rows=[torch.ones((E, 4))] * 5)
    with pytest.raises(ValueError, match=r"contact_rows\[1\] must be"):
        _lib.loop_reset_device(mask, contact_rows=[torch.ones((E, 4)), torch.ones((E, 3))])
    with pytest.raises(ValueError, match="bool, int32 or int64"):
        mask_words(torch.zeros(E), E)
    with pytest.raises(ValueError, match=r"mask must be \(5,\)"):
        mask_words(torch.zeros(4, dtype=torch.bool), E)
    assert mask_words(mask, E) is mask  # an int32 mask is passed as it is


class _Part:
    def __init__(self, n):
        self.num_envs = n

    @property
    def state(self):
        raise AssertionError("the state is not touched before the sizes are checked")


def test_class_refuses_mismatched_num_envs_and_has_the_documented_surface():
    for bad in (0, -1, 4097):
        with pytest.raises(ValueError, match="num_envs must be 1..4096"):
            BatchedLoopReset(bad)
    for name in ("gait", "frg", "stc", "terrain_est", "vfa"):
        with pytest.raises(ValueError, match="holds 3 environments, expected 4"):
            BatchedLoopReset(4, **{name: _Part(3)})
    assert BatchedLoopReset(4).snapshots == {}  # nothing given: no device is touched
    assert list(inspect.signature(BatchedLoopReset.__init__).parameters)[1:] == ["num_envs", "gait", "frg", "stc",
                                                                                 "terrain_est", "vfa"]
    sig = inspect.signature(BatchedLoopReset.reset)
    assert list(sig.parameters)[1:3] == ["mask", "initial_feet"] and sig.parameters["initial_feet"].default is None
    for name in ("best_control_parameters", "contact_rows", "stream"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    for cls in (BatchedPeriodicGaitGenerator, BatchedVisualFootholdAdaptation):
        p = inspect.signature(cls.reset).parameters
        assert p["mask"].default is None and p["mask"].kind is inspect.Parameter.KEYWORD_ONLY
        assert list(p)[1] == "stream"  # the positional argument the parent had


def test_header_states_the_contract():
    text = open(os.path.join(INCLUDE, "srbd_mpc.h")).read()
    doc = text[text.index("Restarting single environments of the batched loop"):text.index("int srbd_loop_reset_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("simulation/simulation.py:773-781", "wb_interface.py:469-484", "no byte of environment e is written",
                   "none of its inputs is read", "SRBD_RESET_EPISODE", "SRBD_RESET_REFERENCE", "step_freq left alone",
                   "that table only", "contact_rows", "whatever the mask holds", "one wave per environment",
                   "wave-uniform", "No LDS, no atomics, no scratch", "byte for byte", "exactly one launch",
                   "no synchronising HIP call", "touches no srbd_batch", "SRBD_E_INVALID (before any HIP call",
                   "num_envs outside 1..4096", "n_contact_rows outside 0..4", "Out of scope", "compacting"):
        assert phrase.lower() in doc.lower(), phrase
    host = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(INCLUDE, "srbd_host.h")).read())
    for phrase in ("srbd_loop_reset", "wb_interface.py:477-479", "a level outside {1, 2}", "frg without initial_feet",
                   "best_params with num_params < 1"):
        assert phrase in host, phrase
