"""C-ABI of the batched environments (srbd_batch_*, include/srbd_mpc.h): exports, bindings, argument checks and the
configurations a batch refuses.  CPU only: every rejection is decided before a device is looked for."""
import ctypes as C
import sys
import types

import numpy as np
import pytest

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd import config as mirror

BATCH_FUNCS = ("srbd_batch_create", "srbd_batch_destroy", "srbd_batch_last_error", "srbd_batch_num_envs",
               "srbd_batch_set_rng", "srbd_batch_step", "srbd_batch_copy_costs")


def make_cfg(N=100, method="mppi", world_size=1, rank=0):
    return _lib.make_config(num_samples=N, horizon=12, method=method, parametrization="zero_order", mass=15.0,
                            inertia=np.eye(3), dts=np.full(12, 0.02), rank=rank, world_size=world_size)


def create(cfg, num_envs):
    h = C.c_void_p()
    rc = _lib.lib.srbd_batch_create(C.byref(cfg), num_envs, C.byref(h))
    if rc == _lib.OK:  # a device is visible and the configuration is valid
        _lib.lib.srbd_batch_destroy(h)
    return rc


def test_symbols_exported_and_bound():
    for name in BATCH_FUNCS:
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert hasattr(_lib, "BatchContext")


@pytest.mark.parametrize("what,cfg,num_envs", [
    ("num_envs 0", make_cfg(), 0),
    ("num_envs 4097", make_cfg(), 4097),
    ("N 16385", make_cfg(N=16385), 4),
    ("CEM", make_cfg(method="cem_mppi"), 4),
    ("world_size 2", make_cfg(N=1024, world_size=2), 4),
])
def test_create_rejects(what, cfg, num_envs):
    assert create(cfg, num_envs) == _lib.E_INVALID, what
    msg = _lib.lib.srbd_batch_last_error(None)
    assert msg and len(msg) > 0


def test_limits_themselves_pass_validation():
    """num_envs 4096 and N 16 384 are in range: with no device the call gets as far as looking for one."""
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert create(make_cfg(N=16384), 1) == _lib.E_NODEVICE
    assert create(make_cfg(N=64), 4096) == _lib.E_NODEVICE


def test_null_arguments():
    lib = _lib.lib
    h = C.c_void_p()
    cfg = make_cfg()
    assert lib.srbd_batch_create(None, 2, C.byref(h)) == _lib.E_INVALID
    assert lib.srbd_batch_create(C.byref(cfg), 2, None) == _lib.E_INVALID
    lib.srbd_batch_destroy(None)  # a no-op
    assert lib.srbd_batch_num_envs(None) == _lib.E_INVALID
    assert lib.srbd_batch_set_rng(None, _lib.RNG_PHILOX) == _lib.E_INVALID
    assert lib.srbd_batch_copy_costs(None, None) == _lib.E_INVALID
    buf = np.zeros(1024, np.float32).ctypes.data
    assert lib.srbd_batch_step(None, buf, buf, buf, 12, buf, None, buf, buf, buf, None) == _lib.E_INVALID
    assert lib.srbd_batch_last_error(None) is not None


def test_no_device_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert create(make_cfg(), 4) == _lib.E_NODEVICE
    with pytest.raises(RuntimeError, match="srbd_batch_create"):
        _lib.BatchContext(make_cfg(), 4)


def test_controller_refuses_cem(monkeypatch):
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC

    cfg = types.ModuleType("cem_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, sampling_method="cem_mppi")
    called = []
    monkeypatch.setattr(_lib.lib, "srbd_batch_create", lambda *a: called.append(a) or _lib.E_INVALID)
    with pytest.raises(NotImplementedError, match="cem_mppi"):
        Batched_Sampling_MPC(4, cfg)
    assert not called


def test_controller_shapes_and_keys():
    """Construction is host-only: (E, P) warm starts, one master key per environment, advanced as the single
    class advances its key."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip import Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC

    b = Batched_Sampling_MPC(3)
    one = Sampling_MPC()
    assert b.best_control_parameters.shape == (3, one.num_control_parameters)
    assert b.master_keys.shape == (3, 2) and b.rng == one.rng
    k0 = np.array(b.master_keys)
    b.with_newkey()
    for e in range(3):
        one.master_key = k0[e]
        np.testing.assert_array_equal(b.master_keys[e], one.with_newkey().master_key)
