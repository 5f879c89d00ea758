"""C-ABI and bindings of the swing reflexes (srbd_reflex_* of include/srbd_host.h, srbd_reflex_step_device of
include/srbd_mpc.h; _lib.reflex_step_device; ReflexSwingTrajectoryController,
BatchedReflexSwingTrajectoryController).  CPU only: every SRBD_E_INVALID here is decided before a HIP call, so the
dummy pointers are never followed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib, config
from quadruped_pympc_amd.helpers.early_stance_detector import EarlyStanceDetector
from quadruped_pympc_amd.helpers.swing_trajectory_controller import (BatchedReflexSwingTrajectoryController,
                                                                     BatchedSwingTrajectoryController,
                                                                     ReflexSwingTrajectoryController,
                                                                     SwingTrajectoryController)

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
PTR = 0x1000  # non-null, never followed
REQUIRED = ("jac", "jac_dot", "mass_matrix", "q_dot", "foot_pos", "foot_vel", "qfrc_passive", "qfrc_bias", "grfs",
            "touch_down", "contact", "tau", "des_foot_pos", "des_foot_vel")
OPTIONAL = ("des_joint_vel", "apex", "full_stance")
HOST = ("srbd_reflex_init", "srbd_reflex_detect", "srbd_reflex_reference", "srbd_reflex_step")
lib = _lib.lib
p = _lib.dptr


def call(d_stc=PTR, d_reflex=PTR, num_envs=4, dt=0.002, no_io=False, lift_off=PTR, frg=None, previous_contact=PTR,
         **over):
    f = dict({k: PTR for k in REQUIRED}, **{k: None for k in OPTIONAL}, apex_interval=0.01, lift_off=lift_off, frg=frg)
    f.update(over)
    io = _lib.SrbdReflexBatchIo(stc=_lib.SrbdStcBatchIo(**f), previous_contact=previous_contact)
    return lib.srbd_reflex_step_device(d_stc, d_reflex, num_envs, dt, None if no_io else C.byref(io), None)


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, names in (("srbd_mpc.h", ("srbd_reflex_step_device",)), ("srbd_host.h", HOST)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name in names:
            assert name in exported and name in _lib.SIGNATURES, name
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
            assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert callable(_lib.reflex_step_device) and lib.srbd_abi_version() == 1


def test_struct_sizes_match_the_headers():
    """sizeof and offsets as the C compiler sees the two headers, against the ctypes mirror; the old struct as it was."""
    fields = ("hitmoments", "hitpoints", "last_des_foot_pos", "has_hitpoint", "early_stance", "trigger_mode",
              "gait_cycles", "reserved")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "srbd_mpc.h"\n#include "srbd_host.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu", sizeof(srbd_reflex), sizeof(srbd_stc), '
           'sizeof(srbd_reflex_batch_io), offsetof(srbd_reflex_batch_io, previous_contact));\n' +
           "".join(f'printf(" %zu", offsetof(srbd_reflex, {f}));\n' for f in fields) + 'return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "sizes.c"), os.path.join(tmp, "sizes")
        open(c, "w").write(src)
        subprocess.run(["cc", "-I", INCLUDE, c, "-o", exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_lib.SrbdReflex), C.sizeof(_lib.SrbdStc), C.sizeof(_lib.SrbdReflexBatchIo),
                     _lib.SrbdReflexBatchIo.previous_contact.offset] + \
        [getattr(_lib.SrbdReflex, f).offset for f in fields]
    assert _lib.REFLEX_BYTES == C.sizeof(_lib.SrbdReflex) == 320 and _lib.REFLEX_BYTES % 8 == 0
    assert _lib.STC_BYTES == 80 and (_lib.SWING_BEZIER_REF, _lib.SWING_EXPLICIT) == (0, 1)
    # doubles first, then int32 words, and every byte accounted for by a named field
    assert sum(C.sizeof(t) for _, t in _lib.SrbdReflex._fields_) == 320
    assert _lib.SrbdReflex.has_hitpoint.offset == 32 * 8
    assert (_lib.REFLEX_OFF, _lib.REFLEX_TRACKING, _lib.REFLEX_GEOM_CONTACT) == (0, 1, 2)


def test_init_values_and_refusals():
    r = _lib.SrbdReflex()
    C.memset(C.byref(r), 0xAB, C.sizeof(r))
    assert lib.srbd_reflex_init(C.byref(r), 0.16, 5, _lib.REFLEX_TRACKING, 7) == _lib.OK
    assert (r.reflex_max_step_height, r.early_stance_time_threshold, r.relative_tracking_error_threshold,
            r.absolute_min_distance_error_threshold) == (0.16, 0.07, 0.3, 0.1)
    assert list(r.hitmoments) == [-1.0] * 4 and list(r.has_hitpoint) == [0] * 4 and list(r.early_stance) == [0] * 4
    assert bytes(r.hitpoints) == bytes(96) and bytes(r.last_des_foot_pos) == bytes(96)
    assert (r.trigger_mode, r.blind, r.use_height_enhancement, r.height_enhancement, r.gait_cycles,
            r.max_gait_cycles, list(r.reserved)) == (1, 1, 1, 0, -1, 6, [0, 0])
    before = bytes(r)
    assert lib.srbd_reflex_init(None, 0.16, 0, 1, 0) == _lib.E_INVALID
    for height in (float("nan"), float("inf")):
        assert lib.srbd_reflex_init(C.byref(r), height, 0, 1, 0) == _lib.E_INVALID
    for mode in (_lib.REFLEX_GEOM_CONTACT, 3, -1):  # 'geom_contact' among the refused
        assert lib.srbd_reflex_init(C.byref(r), 0.16, 0, mode, 0) == _lib.E_INVALID
    assert bytes(r) == before  # nothing written on refusal


def host_call(g=None, r=None, previous=True, dt=0.002, no_io=False, **over):
    """srbd_reflex_step on zero arrays with one thing wrong; returns (rc, both structs' bytes before and after)."""
    g0, r0 = _lib.SrbdStc(), _lib.SrbdReflex()
    assert lib.srbd_stc_init(C.byref(g0), 0.06, 0.3, 500.0, 10.0, 0) == 0
    assert lib.srbd_reflex_init(C.byref(r0), 0.15, 0, 1, 1) == 0
    g = g0 if g is None else g
    r = r0 if r is None else r
    arrays = {k: np.zeros(36 if k in ("jac", "jac_dot", "mass_matrix") else 12) for k in REQUIRED + ("lift_off",)}
    arrays["contact"] = np.zeros(4)
    f = dict({k: p(v) for k, v in arrays.items()}, apex_interval=0.01)
    f.update(over)
    io = _lib.SrbdStcIo(**f)
    prev = np.ones(4)
    before = bytes(g) + bytes(r)
    rc = lib.srbd_reflex_step(C.byref(g) if g is not False else None, C.byref(r) if r is not False else None,
                              None if no_io else C.byref(io), p(prev) if previous else None, dt)
    return rc, before, bytes(g) + bytes(r) if g is not False and r is not False else before, arrays


def test_host_step_refusals_write_nothing():
    rc, before, after, _ = host_call()
    assert rc == _lib.OK and before != after  # the valid call runs (and moves the clocks)
    bad = [dict(g=False), dict(r=False), dict(no_io=True), dict(previous=False), dict(dt=float("nan")),
           dict(dt=float("inf")), dict(apex_interval=float("nan"))]
    bad += [{k: None} for k in REQUIRED + ("lift_off",)]
    for kw in bad:
        rc, before, after, arrays = host_call(**kw)
        assert rc == _lib.E_INVALID and before == after, kw
        assert not any(v.any() for k, v in arrays.items() if k in ("tau", "des_foot_pos", "des_foot_vel")), kw

    def stc(period):
        g = _lib.SrbdStc()
        assert lib.srbd_stc_init(C.byref(g), 0.06, 0.3, 500.0, 10.0, 0) == 0
        g.swing_period = period
        return g

    def reflex(**fields):
        r = _lib.SrbdReflex()
        assert lib.srbd_reflex_init(C.byref(r), 0.15, 0, 1, 0) == 0
        for k, v in fields.items():
            setattr(r, k, v)
        return r

    for kw in [dict(g=stc(0.0)), dict(g=stc(-0.3)), dict(g=stc(float("nan"))), dict(g=stc(float("inf"))),
               dict(r=reflex(trigger_mode=_lib.REFLEX_GEOM_CONTACT)), dict(r=reflex(trigger_mode=9)),
               dict(r=reflex(reflex_max_step_height=float("nan"))),
               dict(r=reflex(reflex_max_step_height=float("-inf")))]:
        rc, before, after, arrays = host_call(**kw)
        assert rc == _lib.E_INVALID and before == after
        assert not arrays["tau"].any()
        g, r = kw.get("g", stc(0.3)), kw.get("r", reflex())
        v = np.zeros(3)
        assert lib.srbd_reflex_reference(C.byref(g), C.byref(r), 0, p(v), p(v), p(v), p(v), p(v)) == _lib.E_INVALID
    # the generator code of the srbd_stc is not read by this path
    g = stc(0.3)
    g.generator = 77
    assert host_call(g=g)[0] == _lib.OK
    g, r, v = stc(0.3), reflex(), np.zeros(3)
    for leg in (-1, 4):
        assert lib.srbd_reflex_reference(C.byref(g), C.byref(r), leg, p(v), p(v), p(v), p(v), p(v)) == _lib.E_INVALID
    z4, z12 = np.zeros(4), np.zeros(12)
    assert lib.srbd_reflex_detect(None, p(z12), p(z12), p(z12), p(z4), 0.3, p(z4), p(z4)) == _lib.E_INVALID
    assert lib.srbd_reflex_detect(C.byref(reflex(trigger_mode=2)), p(z12), p(z12), p(z12), p(z4), 0.3, p(z4),
                                  p(z4)) == _lib.E_INVALID
    assert lib.srbd_reflex_detect(C.byref(r), p(z12), p(z12), p(z12), p(z4), 0.3, None, p(z4)) == _lib.E_INVALID


def test_header_states_the_contract():
    text = open(os.path.join(INCLUDE, "srbd_mpc.h")).read()
    doc = text[text.index("The swing reflex path of the device-resident loop"):
               text.index("int srbd_reflex_step_device")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("Equivalence", "srbd_reflex_step (srbd_host.h)", "exactly one launch", "no synchronising HIP",
                   "srbd_prepare_state_device reads it", "legacy null stream", "wb_interface.py:362-415",
                   "early_stance_detector.py:36-128", "scipy_swing_trajectory_generator.py:25-122", "bit for bit",
                   "NaNs position for position", "SRBD_E_INVALID (before any HIP call)", "SRBD_E_NODEVICE", "1..4096",
                   "both or neither of lift_off and frg", "'geom_contact'", "previous_contact", "scipy raises",
                   "Arrays must not overlap", "srbd_loop_reset_device does not know d_reflex"):
        assert phrase in doc, phrase
    host = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(INCLUDE, "srbd_host.h")).read())
    for phrase in ("early-stance detector", "kinodynamic", "'scipy' generator", "have entry points of their own, below",
                   "sizeof 320", "the legs after the first that triggers are not touched at all",
                   "norm(local) / norm(disp) > 0.3 and norm(local) > 0.1", "Deviation", "SRBD_REFLEX_GEOM_CONTACT",
                   "sizeof 80"):
        assert phrase in host, phrase


def test_invalid_arguments_refused_before_any_hip_call():
    """With or without a device: INVALID, never NODEVICE, and no pointer is followed."""
    E_INVALID = _lib.E_INVALID
    assert call(d_stc=None) == E_INVALID
    assert call(d_reflex=None) == E_INVALID
    assert call(no_io=True) == E_INVALID
    assert call(previous_contact=None) == E_INVALID
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
    return dict(stc=torch.zeros(E, _lib.STC_BYTES, dtype=torch.uint8),
                reflex=torch.zeros(E, _lib.REFLEX_BYTES, dtype=torch.uint8), dt=0.002, jac=m(), jac_dot=m(), q_dot=v(),
                foot_pos=v(), foot_vel=v(), qfrc_passive=v(), qfrc_bias=v(), mass_matrix=m(), grfs=v(), touch_down=v(),
                contact=torch.ones(E, 4), previous_contact=torch.ones(E, 4), lift_off=v())


def test_wrapper_refuses_bad_tensors_without_calling_c(monkeypatch):
    calls = []
    monkeypatch.setattr(lib, "srbd_reflex_step_device", lambda *a: calls.append(a) or _lib.OK)
    f64 = torch.float64
    bad = [("stc", torch.zeros(E * _lib.STC_BYTES, dtype=torch.uint8), "controller state"),
           ("stc", torch.zeros(E, _lib.STC_BYTES, dtype=torch.int8), "uint8"),
           ("reflex", torch.zeros(E, _lib.REFLEX_BYTES - 8, dtype=torch.uint8), "must be"),
           ("reflex", torch.zeros(E + 1, _lib.REFLEX_BYTES, dtype=torch.uint8), "must be"),
           ("reflex", torch.zeros(E, _lib.REFLEX_BYTES, dtype=torch.int32), "uint8"),
           ("reflex", bytes(E * _lib.REFLEX_BYTES), "torch tensor"),
           ("previous_contact", torch.ones(E, 4, dtype=f64), "float32"),
           ("previous_contact", torch.ones(E, 5), "must be"), ("previous_contact", None, "torch tensor"),
           ("jac", torch.zeros(E, 4, 3, 3), "float64"), ("jac", torch.zeros(E, 4, 9, dtype=f64), "must be"),
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
            _lib.reflex_step_device(**dict(good(), **{name: value}))
    with pytest.raises(ValueError, match="must be"):  # the frg form checks the state's shape
        _lib.reflex_step_device(**dict(good(), lift_off=None, frg=torch.zeros(E, 8, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="cuda"):  # right dtypes and shapes, wrong device: refused, not copied
        _lib.reflex_step_device(**good())
    assert not calls


def test_class_argument_checks_are_host_only():
    B = BatchedReflexSwingTrajectoryController
    assert issubclass(B, BatchedSwingTrajectoryController)
    assert issubclass(ReflexSwingTrajectoryController, SwingTrajectoryController)
    for n in (0, 4097):
        with pytest.raises(ValueError, match="num_envs"):
            B(n, 0.06, 0.4, 500, 10, reflex_max_step_height=0.15)
    with pytest.raises(ValueError, match="reflex_max_step_height"):
        B(3, 0.06, 0.4, 500, 10, reflex_max_step_height=[0.15, 0.16])
    with pytest.raises(ValueError, match="blind"):
        B(3, 0.06, 0.4, 500, 10, reflex_max_step_height=0.15, blind=[True, False])
    for height in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            B(3, 0.06, 0.4, 500, 10, reflex_max_step_height=[0.15, height, 0.15])
        with pytest.raises(ValueError, match="finite"):
            ReflexSwingTrajectoryController(0.06, 0.4, 500, 10, reflex_max_step_height=height)
    for cls, args in ((B, (3, 0.06, 0.4, 500, 10)), (ReflexSwingTrajectoryController, (0.06, 0.4, 500, 10))):
        with pytest.raises(NotImplementedError, match="geom_contact"):
            cls(*args, reflex_max_step_height=0.15, reflex_trigger_mode="geom_contact")
        with pytest.raises(ValueError, match="reflex_trigger_mode"):
            cls(*args, reflex_max_step_height=0.15, reflex_trigger_mode="contact")
        with pytest.raises(TypeError):
            cls(*args)  # reflex_max_step_height has no default
    with pytest.raises(ValueError, match="step_height"):
        B(3, [0.06, 0.07], 0.4, 500, 10, reflex_max_step_height=0.15)
    with pytest.raises(ValueError, match="positive and finite"):
        B(3, 0.06, [0.4, 0.0, 0.4], 500, 10, reflex_max_step_height=0.15)
    with pytest.raises(ValueError, match="scipy"):
        ReflexSwingTrajectoryController(0.06, 0.4, 500, 10, "bezier_ref", reflex_max_step_height=0.15)
    for method in ("step", "state_dict", "load_state_dict", "reset", "regenerate_swing_trajectory_generator",
                   "check_touch_down_condition"):
        assert callable(getattr(B, method))
    c = ReflexSwingTrajectoryController(0.06, 0.4, 500, 10, reflex_max_step_height=0.15, blind=True)
    assert c.generator == "scipy" and isinstance(c.esd, EarlyStanceDetector) and c.esd._r is c._r
    assert c.blind_locomotion and c.reflex_max_step_height == 0.15 and not c.reflex_next_steps_height_enhancement
    assert c.esd.trigger_mode == "tracking" and c.esd.activated
    assert list(c.esd.hitmoments) == [-1.0] * 4 and list(c.esd.hitpoints) == [None] * 4
    off = ReflexSwingTrajectoryController(0.06, 0.4, 500, 10, reflex_max_step_height=0.15, reflex_trigger_mode=False)
    assert off.esd.trigger_mode is False and not off.esd.activated


def test_scipy_on_the_old_classes_still_raises():
    with pytest.raises(NotImplementedError, match="scipy"):
        SwingTrajectoryController(0.06, 0.4, 500, 10, "scipy")
    with pytest.raises(NotImplementedError, match="scipy"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, 10, "scipy")
    with pytest.raises(NotImplementedError, match="ReflexSwingTrajectoryController"):
        BatchedSwingTrajectoryController(3, 0.06, 0.4, 500, 10, ["bezier_ref", "scipy", "explicit"])


def test_batched_class_without_a_device_raises_a_clear_error():
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        BatchedReflexSwingTrajectoryController(3, 0.06, [0.4, 0.45, 0.5], 500, 10, reflex_max_step_height=0.15)


def test_config_carries_the_reference_values():
    sp = config.simulation_params
    assert sp["reflex_trigger_mode"] == "tracking"
    assert sp["reflex_max_step_height"] == 0.5 * config.hip_height
    assert sp["reflex_next_steps_height_enhancement"] is False
    d = EarlyStanceDetector()  # the reference's constructor: everything from the config
    assert d.trigger_mode == "tracking" and not d.use_reflex_next_steps_height_enhancement
    assert (d.early_stance_time_threshold, d.relative_tracking_error_threshold,
            d.absolute_min_distance_error_threshold, d.max_gait_cycles_height_enhancement,
            d.gait_cycles_after_reflex_height_enanchement) == (0.07, 0.3, 0.1, 6, -1)
    assert d._r.reflex_max_step_height == sp["reflex_max_step_height"] and d._r.blind == 0
