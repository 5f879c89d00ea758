"""C-ABI of the per-environment robot and cost parameters of a batch (srbd_batch_set_env_params,
srbd_batch_set_env_params_device, srbd_batch_get_env_params, srbd_batch_clear_env_params, include/srbd_mpc.h): exports,
bindings, the record's layout, make_env_params' roundings and the refusals decided before a device is looked for.
CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quadruped_pympc_amd import _lib

ENV_FUNCS = ("srbd_batch_set_env_params", "srbd_batch_set_env_params_device", "srbd_batch_get_env_params",
             "srbd_batch_clear_env_params")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "srbd_mpc.h")


def make_cfg(mass=15.0, **kw):
    return _lib.make_config(num_samples=100, horizon=12, method="mppi", parametrization="zero_order", mass=mass,
                            inertia=np.diag([0.1, 0.3, 0.4]), dts=np.full(12, 0.02), **kw)


def test_symbols_exported_and_bound():
    for name in ENV_FUNCS:
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    for cls in (_lib.BatchContext, _lib.CemBatchContext):
        for method in ("set_env_params", "set_env_params_device", "get_env_params", "clear_env_params"):
            assert callable(getattr(cls, method))


def test_record_layout():
    """39 packed floats; the ctypes struct and the numpy dtype agree field by field."""
    assert C.sizeof(_lib.EnvParams) == 156
    assert _lib.ENV_PARAMS_DTYPE.itemsize == 156
    for name, _ in _lib.EnvParams._fields_:
        assert getattr(_lib.EnvParams, name).offset == _lib.ENV_PARAMS_DTYPE.fields[name][1], name
    assert [n for n, _ in _lib.EnvParams._fields_][:7] == ["mass", "mg", "grf_min", "grf_max", "mu", "inertia",
                                                           "q_diag"]
    assert _lib.EnvParams.inertia.offset == 20 and _lib.EnvParams.q_diag.offset == 56


# float32(10.012999534606934) * float32(9.81) = 98.22753 but float32(float64(m) * 9.81) = 98.22752: the third mass
# tells make_config's rounding (the double product rounded once) from a float32 product
MASSES = [15.0, 12.453, 10.012999534606934]


def test_make_env_params_rounds_as_make_config():
    m3 = np.float32(MASSES[2])
    assert np.float32(m3 * np.float32(9.81)) != np.float32(float(m3) * 9.81)
    base = make_cfg()
    p = _lib.make_env_params(3, base, mass=MASSES)
    for e, m in enumerate(MASSES):
        cfg = make_cfg(mass=m)
        assert np.float32(p["mass"][e]).tobytes() == np.float32(cfg.mass).tobytes()
        assert np.float32(p["mg"][e]).tobytes() == np.float32(cfg.mg).tobytes()
        assert np.float32(p["grf_max"][e]).tobytes() == np.float32(cfg.grf_max).tobytes()
        got = _lib.config_with_env_params(base, p[e])
        assert bytes(got) == bytes(cfg)


def test_make_env_params_defaults_and_broadcast():
    base = make_cfg(mu=0.7, grf_min=2.0)
    p = _lib.make_env_params(4, base)
    assert p.shape == (4,) and p.dtype == _lib.ENV_PARAMS_DTYPE
    for e in range(4):
        assert bytes(_lib.config_with_env_params(base, p[e])) == bytes(base)
    q = np.arange(24, dtype=np.float32)
    p = _lib.make_env_params(2, base, mu=[0.3, 1.0], grf_max=200.0, inertia=np.eye(3), q_diag=q)
    np.testing.assert_array_equal(p["mu"], np.array([0.3, 1.0], np.float32))
    np.testing.assert_array_equal(p["grf_max"], np.float32(200.0))
    np.testing.assert_array_equal(p["grf_min"], np.float32(2.0))
    np.testing.assert_array_equal(p["inertia"][1], np.eye(3, dtype=np.float32).reshape(9))
    np.testing.assert_array_equal(p["q_diag"][0], q)
    assert np.float32(p["mg"][0]).tobytes() == np.float32(base.mg).tobytes()  # mass not given: the configuration's
    with pytest.raises(ValueError, match="mu"):
        _lib.make_env_params(2, base, mu=[0.3, 0.5, 0.8])
    with pytest.raises(ValueError, match="inertia"):
        _lib.make_env_params(2, base, inertia=np.zeros((3, 9)))


def test_null_arguments_are_refused_before_any_device_call():
    lib = _lib.lib
    buf = np.zeros(64, np.float32).ctypes.data
    assert lib.srbd_batch_set_env_params(None, buf, None) == _lib.E_INVALID
    assert b"srbd_batch_set_env_params" in lib.srbd_batch_last_error(None)
    assert lib.srbd_batch_set_env_params_device(None, buf, None, None, None) == _lib.E_INVALID
    assert b"srbd_batch_set_env_params_device" in lib.srbd_batch_last_error(None)
    assert lib.srbd_batch_get_env_params(None, buf) == _lib.E_INVALID
    assert lib.srbd_batch_clear_env_params(None) == _lib.E_INVALID


def test_header_states_the_rules():
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    assert "typedef struct srbd_env_params" in text
    # the equivalence: srbd_step on srbd_create(cfg_e), every output bit for bit
    assert re.search(r"environment e returns exactly what srbd_step returns on srbd_create\(cfg_e\)", text)
    assert "every output bit for bit" in text
    # the refusal rule and the per-environment validation
    assert "Refusal rule" in text and "SRBD_E_INVALID with a message" in text
    assert "names that environment in srbd_batch_last_error and changes nothing" in text
    assert "d_rejected[e] = 1" in text
    assert "4-byte aligned" in text
    # the robot moved to the per-environment list of the batch's header comment
    shared = text[text.index("Shared: the srbd_config"):text.index("Per environment: everything per step")]
    assert "robot" not in shared and "bounds" not in shared
