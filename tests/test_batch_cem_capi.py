"""C-ABI of the batched CEM-MPPI environments (srbd_batch_create_cem, srbd_batch_step_cem,
srbd_batch_step_cem_device, include/srbd_mpc.h): exports, bindings and the refusals.  CPU only: every rejection is
decided before a device is looked for."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd import config as mirror

CEM_FUNCS = ("srbd_batch_create_cem", "srbd_batch_step_cem", "srbd_batch_step_cem_device")


def make_cfg(N=100, method="cem_mppi", num_elite=10, world_size=1, rank=0):
    return _lib.make_config(num_samples=N, horizon=12, method=method, parametrization="zero_order", mass=15.0,
                            inertia=np.eye(3), dts=np.full(12, 0.02), num_elite=num_elite, rank=rank,
                            world_size=world_size)


def create(cfg, num_envs):
    h = C.c_void_p()
    rc = _lib.lib.srbd_batch_create_cem(C.byref(cfg), num_envs, C.byref(h))
    if rc == _lib.OK:  # a device is visible and the configuration is valid
        _lib.lib.srbd_batch_destroy(h)
    return rc


def config_module(**mpc):
    cfg = types.ModuleType("cem_test_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, **mpc)
    return cfg


def test_symbols_exported_and_bound():
    for name in CEM_FUNCS:
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert issubclass(_lib.CemBatchContext, _lib.BatchContext)
    assert C.sizeof(_lib.BatchCemIO) == 16  # { float* sigma; float sigma_reset; int32_t pad; }


@pytest.mark.parametrize("what,cfg,num_envs", [
    ("MPPI", make_cfg(method="mppi"), 4),
    ("random sampling", make_cfg(method="random_sampling"), 4),
    ("num_elite 1", make_cfg(num_elite=1), 4),
    ("num_elite 17", make_cfg(num_elite=17), 4),
    ("num_envs 0", make_cfg(), 0),
    ("num_envs 4097", make_cfg(), 4097),
    ("N 16385", make_cfg(N=16385), 4),
    ("world_size 2", make_cfg(N=1024, world_size=2), 4),
])
def test_create_cem_rejects(what, cfg, num_envs):
    assert create(cfg, num_envs) == _lib.E_INVALID, what
    msg = _lib.lib.srbd_batch_last_error(None)
    assert msg and len(msg) > 0


def test_valid_config_reaches_the_device_lookup():
    """A valid CEM configuration, the limits included: with no device the call gets as far as looking for one."""
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert create(make_cfg(), 4) == _lib.E_NODEVICE
    assert create(make_cfg(N=16384, num_elite=16), 1) == _lib.E_NODEVICE
    assert create(make_cfg(N=64, num_elite=2), 4096) == _lib.E_NODEVICE
    with pytest.raises(RuntimeError, match="srbd_batch_create_cem"):
        _lib.CemBatchContext(make_cfg(), 4)


def test_plain_create_still_refuses_cem_and_names_the_new_call():
    h = C.c_void_p()
    cfg = make_cfg()
    assert _lib.lib.srbd_batch_create(C.byref(cfg), 4, C.byref(h)) == _lib.E_INVALID
    assert b"srbd_batch_create_cem" in _lib.lib.srbd_batch_last_error(None)


def test_null_arguments():
    lib = _lib.lib
    h = C.c_void_p()
    cfg = make_cfg()
    assert lib.srbd_batch_create_cem(None, 2, C.byref(h)) == _lib.E_INVALID
    assert lib.srbd_batch_create_cem(C.byref(cfg), 2, None) == _lib.E_INVALID
    buf = np.zeros(1024, np.float32).ctypes.data
    assert lib.srbd_batch_step_cem(None, buf, buf, buf, 12, buf, buf, None, buf, buf, buf, None) == _lib.E_INVALID
    io = _lib.BatchDeviceIO(**{name: buf for name, _ in _lib.BatchDeviceIO._fields_
                               if name not in ("contact_stride", "pad", "noise", "costs")})
    io.contact_stride = 12
    cem = _lib.BatchCemIO(sigma=buf, sigma_reset=0.0, pad=0)
    # each refusal by its own message (the text of the calling thread: b is NULL), under the entry point's name
    assert lib.srbd_batch_step_cem_device(None, C.byref(io), C.byref(cem), None) == _lib.E_INVALID
    assert lib.srbd_batch_last_error(None) == b"srbd_batch_step_cem_device: null batch"
    assert lib.srbd_batch_step_cem_device(None, None, C.byref(cem), None) == _lib.E_INVALID
    assert lib.srbd_batch_last_error(None) == b"srbd_batch_step_cem_device: null io"
    assert lib.srbd_batch_step_cem_device(None, C.byref(io), None, None) == _lib.E_INVALID
    assert lib.srbd_batch_last_error(None) == b"srbd_batch_step_cem_device: null cem"
    io_no_grf = _lib.BatchDeviceIO.from_buffer_copy(io)
    io_no_grf.grf = None
    assert lib.srbd_batch_step_cem_device(None, C.byref(io_no_grf), C.byref(cem), None) == _lib.E_INVALID
    assert lib.srbd_batch_last_error(None) == b"srbd_batch_step_cem_device: null required pointer: grf"
    assert lib.srbd_batch_step_device(None, None, None) == _lib.E_INVALID  # the sibling keeps its own name
    assert lib.srbd_batch_last_error(None) == b"srbd_batch_step_device: null io"
    for bad in (-1.0, float("inf"), float("nan")):
        cem_bad = _lib.BatchCemIO(sigma=buf, sigma_reset=bad, pad=0)
        assert lib.srbd_batch_step_cem_device(None, C.byref(io), C.byref(cem_bad), None) == _lib.E_INVALID
        assert b"sigma_reset" in lib.srbd_batch_last_error(None)
    no_sigma = _lib.BatchCemIO(sigma=None, sigma_reset=3.0, pad=0)
    assert lib.srbd_batch_step_cem_device(None, C.byref(io), C.byref(no_sigma), None) == _lib.E_INVALID
    assert b"sigma" in lib.srbd_batch_last_error(None)


# ------------------------------------------------------------------ CemBatchContext.step_cem_device's sigma checks
E, N, H, P = 3, 100, 12, 144


@pytest.fixture
def hollow_cem_batch(monkeypatch):
    """A CemBatchContext of E = 3, N = 100, H = 12 that owns no srbd_batch; the C function records its calls."""
    calls = []
    monkeypatch.setattr(_lib.lib, "srbd_batch_step_cem_device", lambda *a: calls.append(a) or _lib.OK)
    b = _lib.CemBatchContext.__new__(_lib.CemBatchContext)
    b.E, b.N, b.P, b.h = E, N, P, None
    b.cfg = make_cfg(N=N)
    return b, calls


def good_args():
    return dict(states=torch.zeros(E, 24), refs=torch.zeros(E, 24), contacts=torch.ones(E, 4, H),
                best=torch.zeros(E, P), sigma=torch.ones(E, P), seeds=torch.zeros(E, dtype=torch.int64),
                counters=torch.zeros(E, dtype=torch.int64))


BAD_SIGMA = [
    (dict(sigma=np.ones((E, P), np.float32)), "sigma must be a torch tensor"),
    (dict(sigma=torch.ones(E, P, dtype=torch.float64)), "sigma must be torch.float32"),
    (dict(sigma=torch.ones(E, P + 12)), "sigma must be"),
    (dict(sigma=torch.ones(P)), "sigma must be"),
    (dict(sigma=torch.ones(P, E).t()), "sigma must be contiguous"),
    (dict(sigma_reset=-1.0), "sigma_reset"),
    (dict(sigma_reset=float("inf")), "sigma_reset"),
    (dict(sigma_reset=float("nan")), "sigma_reset"),
    (dict(best=torch.zeros(E, P + 12)), "best must be"),  # the plain step's checks still run
]


@pytest.mark.parametrize("bad,match", BAD_SIGMA, ids=[str(i) for i in range(len(BAD_SIGMA))])
def test_step_cem_device_refuses_bad_arguments_before_the_c_call(hollow_cem_batch, bad, match):
    b, calls = hollow_cem_batch
    with pytest.raises(ValueError, match=match):
        b.step_cem_device(**dict(good_args(), **bad))
    assert not calls


def test_step_cem_device_refuses_cpu_tensors_before_the_c_call(hollow_cem_batch):
    """Right dtypes and shapes, wrong device: every tensor here lives on the CPU."""
    b, calls = hollow_cem_batch
    with pytest.raises(ValueError, match="must be on cuda:0"):
        b.step_cem_device(**good_args())
    assert not calls


def test_cem_controller_refuses_other_methods(monkeypatch):
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC

    called = []
    monkeypatch.setattr(_lib.lib, "srbd_batch_create_cem", lambda *a: called.append(a) or _lib.E_INVALID)
    for method in ("mppi", "random_sampling"):
        with pytest.raises(ValueError, match="cem_mppi"):
            Batched_CEM_Sampling_MPC(4, config_module(sampling_method=method))
    assert not called


def test_cem_controller_shapes():
    """Construction is host-only: (E, P) sigma at the configured constant, with_newsigma broadcasting."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC

    cfg = config_module(sampling_method="cem_mppi")
    c = Batched_CEM_Sampling_MPC(3, cfg)
    P = c.num_control_parameters
    assert c.sigma_cem_mppi.shape == (3, P) and c.sigma_cem_mppi.dtype == np.float32
    assert (c.sigma_cem_mppi == np.float32(cfg.mpc_params["sigma_cem_mppi"])).all()
    assert c.sigma_reset_value == float(cfg.mpc_params["sigma_cem_mppi"])
    row = np.linspace(0.2, 5.0, P).astype(np.float32)
    assert c.with_newsigma(row) is c
    np.testing.assert_array_equal(c.get_sigma(), np.tile(row, (3, 1)))
    c.with_newsigma(1.5)
    assert (c.get_sigma() == np.float32(1.5)).all() and c.get_sigma().shape == (3, P)


def test_existing_classes_still_refuse_cem(monkeypatch):
    from quadruped_pympc_amd.controllers.sampling import centroidal_nmpc_hip_batched as plain
    from quadruped_pympc_amd.controllers.sampling import centroidal_nmpc_hip_gait_adaptive_batched as ga

    called = []
    monkeypatch.setattr(_lib.lib, "srbd_batch_create", lambda *a: called.append(a) or _lib.E_INVALID)
    monkeypatch.setattr(_lib.lib, "srbd_batch_create_cem", lambda *a: called.append(a) or _lib.E_INVALID)
    for cls in (plain.Batched_Sampling_MPC, ga.Batched_Sampling_MPC):
        with pytest.raises(NotImplementedError, match="cem_mppi") as ei:
            cls(4, config_module(sampling_method="cem_mppi"))
        assert "Batched_CEM_Sampling_MPC" in str(ei.value)
    assert not called
