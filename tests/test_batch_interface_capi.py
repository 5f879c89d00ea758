"""C-ABI of the batch's controller-interface step (srbd_batch_interface_step_device, srbd_selftest_interface_keys,
include/srbd_mpc.h): exports, bindings, the refusals that need no device, and the key schedule's host twin against
the jax.random oracle (both counter layouts) and against counter + 1 (Philox).  CPU only."""
import ctypes as C

import numpy as np
import pytest

from oracle import jax_random_oracle as jro
from quadruped_pympc_amd import _lib

FUNCS = ("srbd_batch_interface_step_device", "srbd_selftest_interface_keys")
U64 = 0xFFFFFFFFFFFFFFFF


def test_symbols_exported_and_bound():
    for name in FUNCS:
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.srbd_abi_version() == 1
    assert _lib.MAX_IFACE_ITERS == 8
    # 3 pointers, 4 ints, gait, 4 pointers, float + int, 11 pointers
    assert C.sizeof(_lib.BatchInterfaceIO) == 3 * 8 + 16 + 8 + 4 * 8 + 8 + 11 * 8
    assert _lib.BatchInterfaceIO.gait.offset == 40 and _lib.BatchInterfaceIO.sigma_reset.offset == 80


def test_null_batch_and_null_io_are_refused_without_a_device():
    io = _lib.BatchInterfaceIO()
    assert _lib.lib.srbd_batch_interface_step_device(None, C.byref(io), None) == _lib.E_INVALID
    assert b"null batch" in _lib.lib.srbd_batch_last_error(None)
    assert _lib.lib.srbd_batch_interface_step_device(None, None, None) == _lib.E_INVALID


def _keys(n):
    """n keys with the edge values first: 0, all ones, a counter at 2^64 - 1."""
    rng = np.random.default_rng(5)
    k = rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    edge = np.array([[0, 0], [U64, U64], [42, U64], [U64, 0], [0x0123456789ABCDEF, 7]], dtype=np.uint64)
    k[:min(n, len(edge))] = edge[:n] if n < len(edge) else edge
    return k


def _expected(keys, rng, iterations):
    """The schedule of srbd_interface_step in Python integers: (advanced keys, step keys)."""
    n = keys.shape[0]
    steps = np.zeros((iterations, n, 2), np.uint64)
    out = np.array(keys)
    for e in range(n):
        k0, k1 = int(keys[e, 0]), int(keys[e, 1])
        for i in range(iterations):
            if rng != "philox":
                a = jro.split(np.array([k0 >> 32, k0 & 0xFFFFFFFF], np.uint32), 2, partitionable=rng == "jax")[0]
                k0 = (int(a[0]) << 32) | int(a[1])
            k1 = (k1 + 1) & U64
            steps[i, e] = (k0, k1)
        out[e] = (k0, k1)
    return out, steps


@pytest.mark.parametrize("rng", ["philox", "jax", "jax_legacy"])
@pytest.mark.parametrize("iterations", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 65])
def test_key_schedule_equals_the_oracle(rng, iterations, n):
    keys = _keys(n)
    if n == 1:  # the single key: every edge value in turn
        for row in _keys(5):
            got, steps = _lib.interface_keys_host(row.reshape(1, 2), rng, iterations)
            want, want_steps = _expected(row.reshape(1, 2), rng, iterations)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(steps, want_steps)
        return
    got, steps = _lib.interface_keys_host(keys, rng, iterations)
    want, want_steps = _expected(keys, rng, iterations)
    np.testing.assert_array_equal(steps, want_steps)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, steps[-1])  # keys_io after the call is the last row of step_keys
    if rng == "philox":
        np.testing.assert_array_equal(got[:, 0], keys[:, 0])  # the seed stays
        assert int(got[2, 1]) == (iterations - 1)  # 2^64 - 1 wraps as uint64
    else:
        assert int(got[2, 1]) == (iterations - 1) and np.all(got[5:, 0] != keys[5:, 0])


def test_key_schedule_refusals():
    k = np.zeros((1, 2), np.uint64)
    s = np.zeros((8, 1, 2), np.uint64)
    f = _lib.lib.srbd_selftest_interface_keys
    assert f(None, 1, 0, 1, s.ctypes.data) == _lib.E_INVALID
    assert f(k.ctypes.data, 1, 0, 1, None) == _lib.E_INVALID
    assert f(k.ctypes.data, 0, 0, 1, s.ctypes.data) == _lib.E_INVALID
    assert f(k.ctypes.data, 1, 3, 1, s.ctypes.data) == _lib.E_INVALID
    assert f(k.ctypes.data, 1, 0, 0, s.ctypes.data) == _lib.E_INVALID
    assert f(k.ctypes.data, 1, 0, 9, s.ctypes.data) == _lib.E_INVALID
    assert not k.any() and not s.any()
