"""C-ABI and bindings of the batched, device-resident TAMOLS foothold search (srbd_tamols_batch_device,
include/srbd_mpc.h; _lib.tamols_batch_device; BatchedVisualFootholdAdaptation).  CPU only: every SRBD_E_INVALID here
is decided before a HIP call, so the dummy pointers are never followed.  Also the host twin of the kernel's yaw
cos / sin (csrc/yaw_sincos.h) against libm."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import (BatchedVisualFootholdAdaptation,
                                                                    tamols_params_struct)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "srbd_mpc.h")
PTR = 0x1000  # non-null, never followed
lib = _lib.lib
PARAMS = tamols_params_struct({}, "go2")
# the yaws of tests/test_gpu_tamols_batch.py (its exact comparisons need libm's cos / sin of them correctly rounded)
GPU_TEST_YAWS = (0.0, 0.3, -1.2, 2.5, -0.7, 3.1, 1.0, -2.9)


def call(terrain=None, num_envs=4, params=PARAMS, **over):
    f = dict(seeds=PTR, hips=PTR, forward_vel=None, base_pos=None, contact=None, feet=None,
             yaws=PTR if terrain else None, heightmaps=None if terrain else PTR, rows=13, cols=7, dist_x=0.04,
             dist_y=0.04, ray_z=10.0, footholds=PTR, boxes=PTR, valid=PTR, seed_heights=None, scores=None,
             heightmaps_out=None, ref=None)
    f.update(over)
    io = _lib.TamolsBatchIO(**f)
    return lib.srbd_tamols_batch_device(terrain, None if params is None else C.byref(params), num_envs, C.byref(io),
                                        None)


def test_symbol_exported_bound_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for name in ("srbd_tamols_batch_device", "srbd_selftest_yaw_sincos"):
        assert name in exported
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert callable(_lib.tamols_batch_device)
    # the structure's layout: 8 pointers, 2 int32, 3 doubles, 7 pointers
    assert C.sizeof(_lib.TamolsBatchIO) == 8 * 8 + 8 + 3 * 8 + 7 * 8
    assert _lib.TamolsBatchIO.rows.offset == 64 and _lib.TamolsBatchIO.footholds.offset == 96


@pytest.mark.parametrize("terrain", [None, PTR], ids=["patch", "terrain"])
def test_invalid_arguments_refused_before_any_hip_call(terrain):
    E_INVALID = _lib.E_INVALID
    for name in ("seeds", "hips", "footholds", "boxes", "valid"):
        assert call(terrain, **{name: None}) == E_INVALID, name
    assert call(terrain, params=None) == E_INVALID
    assert lib.srbd_tamols_batch_device(terrain, C.byref(PARAMS), 4, None, None) == E_INVALID
    for E in (0, -1, 4097, 2 ** 31 - 1):
        assert call(terrain, num_envs=E) == E_INVALID, E
    for rows, cols in ((0, 7), (13, 0), (-1, -1), (17, 19), (321, 1), (1, 321), (65536, 65536)):
        assert call(terrain, rows=rows, cols=cols) == E_INVALID, (rows, cols)
    if terrain:
        assert call(terrain, yaws=None) == E_INVALID
        for bad in (0.0, -0.04, float("nan")):
            assert call(terrain, dist_x=bad) == E_INVALID
            assert call(terrain, dist_y=bad) == E_INVALID
    else:
        assert call(terrain, heightmaps=None) == E_INVALID
        assert call(terrain, heightmaps_out=PTR) == E_INVALID


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the dummy pointers would be followed")
def test_limits_pass_validation_and_reach_the_launch():
    """E = 4096 and 16 x 20 are inside the range: with no device the launch itself reports SRBD_E_NODEVICE.  (The
    terrain form reads the terrain object's device fields on the host, so only the patch form runs with a dummy.)"""
    assert call(None, num_envs=4096, rows=16, cols=20) == _lib.E_NODEVICE
    assert call(None, num_envs=1, rows=1, cols=1) == _lib.E_NODEVICE
    assert call(None, num_envs=4096, rows=20, cols=16, forward_vel=PTR, base_pos=PTR, contact=PTR, feet=PTR,
                seed_heights=PTR, scores=PTR, ref=PTR) == _lib.E_NODEVICE


def test_python_class_constructs_on_the_host_and_checks_its_arguments():
    torch = pytest.importorskip("torch")
    vfa = BatchedVisualFootholdAdaptation(300)
    assert vfa.num_envs == 300
    p = vfa._params()
    from quadruped_pympc_amd import config  # the active configuration without a reference package installed

    want = tamols_params_struct(config.simulation_params["tamols_params"], config.robot)
    assert isinstance(p, _lib.TamolsParams) and bytes(p) == bytes(want)
    assert vfa._params() is p
    vfa.tamols_params = dict(vfa.tamols_params, weight_deviation=3.0)
    assert vfa._params().w_dev == 3.0
    for E in (0, 4097):
        with pytest.raises(ValueError):
            BatchedVisualFootholdAdaptation(E)
    seeds = torch.zeros((300, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="cuda"):  # host tensors are refused, not copied
        vfa.compute_adaptation_device(seeds, seeds.clone(), None, None, None, None,
                                      heightmaps=torch.zeros((300, 4, 2, 2, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="300 environments"):
        vfa.compute_adaptation_device(seeds[:5], seeds[:5], None, None, None, None,
                                      heightmaps=torch.zeros((5, 4, 2, 2, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="either terrain"):
        _lib.tamols_batch_device(seeds, seeds, p)
    with pytest.raises(ValueError, match="1..320"):
        _lib.tamols_batch_device(seeds, seeds, p, heightmaps=torch.zeros((300, 4, 17, 19, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        _lib.tamols_batch_device(seeds.float(), seeds, p,
                                 heightmaps=torch.zeros((300, 4, 2, 2, 3), dtype=torch.float64))


def yaw_cs(yaws):
    y = np.ascontiguousarray(yaws, dtype=np.float64)
    out = np.zeros((y.size, 2))
    assert lib.srbd_selftest_yaw_sincos(y.ctypes.data, y.size, out.ctypes.data) == 0
    return out


def test_yaw_sincos_against_libm():
    """The kernel's cos / sin of a yaw (host twin, the same float64 operations) are the correctly rounded values; libm's
    are within one ulp of the true ones, so the two differ by at most one ulp of libm's value, and agree on all but a
    small share of a grid.  On the GPU tests' yaws and on the special values they are equal."""
    got = yaw_cs(GPU_TEST_YAWS)
    for (c, s), y in zip(got, GPU_TEST_YAWS):
        assert c.tobytes() == np.float64(math.cos(y)).tobytes() and s.tobytes() == np.float64(math.sin(y)).tobytes(), y
    z = yaw_cs([0.0, -0.0, np.inf, -np.inf, np.nan])
    assert z[0].tolist() == [1.0, 0.0] and z[1, 0] == 1.0 and z[1, 1] == 0.0 and np.signbit(z[1, 1])
    assert not np.signbit(z[0, 1]) and np.isnan(z[2:]).all()
    grid = np.concatenate([np.linspace(-7.0, 7.0, 20001), np.linspace(-700.0, 700.0, 5001),
                           np.arange(-8, 9) * (math.pi / 2), [1e-300, 5e-324, 1e5, -3e5]])
    got = yaw_cs(grid)
    want = np.array([[math.cos(v), math.sin(v)] for v in grid])
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    share = np.mean(np.any(got != want, axis=1))
    print(f"yaws whose libm cos or sin is not the correctly rounded value: {share:.4%}")
    assert share < 0.02  # libm's documented error is below an ulp; a large share would be a defect here
