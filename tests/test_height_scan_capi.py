"""C-ABI and bindings of the device-resident height scans and the 'height' strategy behind the apex gate
(srbd_terrain_patches_device, srbd_terrain_set_patches_device, srbd_vfa_height_step_device,
srbd_vfa_height_step_scenes_device, include/srbd_mpc.h; the host twin srbd_vfa_height_search, include/srbd_host.h;
_lib.terrain_patches_device / vfa_height_step_device; GpuTerrain.patches_device, GpuTerrainSet.patches_device,
BatchedVisualFootholdAdaptation(adaptation_strategy='height')).  CPU only: every SRBD_E_INVALID here is decided before a
HIP call and before a handle is followed, so the dummy pointers are never read."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.terrain import GpuTerrain, GpuTerrainSet, PatchHeightMap
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
PTR = 0x1000  # non-null, 4-byte aligned, never followed
lib = _lib.lib
DEVICE_NAMES = ("srbd_terrain_patches_device", "srbd_terrain_set_patches_device", "srbd_vfa_height_step_device",
                "srbd_vfa_height_step_scenes_device")
NAN, INF = float("nan"), float("inf")


def terrain_error():
    msg = lib.srbd_terrain_last_error(None)
    return msg.decode() if msg else ""


def set_error():
    msg = lib.srbd_terrain_set_last_error(None)
    return msg.decode() if msg else ""


def test_symbols_exported_bound_and_declared():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for header, names in (("srbd_mpc.h", DEVICE_NAMES), ("srbd_host.h", ("srbd_vfa_height_search",))):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
        for name in names:
            assert name in exported, name
            assert name in _lib.SIGNATURES, name
            assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
            assert re.search(r"^int " + name + r"\s*\(", text, flags=re.M), name
    assert lib.srbd_abi_version() == 1
    for cls in (GpuTerrain, GpuTerrainSet):
        assert callable(cls.patches_device)


def test_patch_io_struct_layout():
    S = _lib.PatchBatchIO
    offsets = dict(centers=0, yaws=8, patches_per_env=16, rows=20, cols=24, dist_x=32, dist_y=40, ray_z=48, points=56,
                   heights=64)
    assert C.sizeof(S) == 72 and [n for n, _ in S._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(S, name).offset == off, name


# ------------------------------------------------------------------ srbd_terrain_patches_device / _set_patches_device
def patch_io(**over):
    f = dict(centers=PTR, yaws=PTR, patches_per_env=5, rows=13, cols=7, dist_x=0.04, dist_y=0.04, ray_z=10.0,
             points=PTR, heights=None)
    f.update(over)
    return _lib.PatchBatchIO(**f)


PATCH_IO_CASES = [(dict(centers=None), "centers"), (dict(yaws=None), "yaws"),
                  (dict(points=None, heights=None), "both null"),
                  (dict(patches_per_env=0), "patches_per_env"), (dict(patches_per_env=17), "patches_per_env"),
                  (dict(patches_per_env=-1), "patches_per_env"),
                  (dict(rows=0), "rows"), (dict(cols=0), "cols"), (dict(rows=-3), "rows"), (dict(cols=-1), "cols"),
                  (dict(rows=17, cols=20), "rows * cols"), (dict(rows=321, cols=1), "rows * cols"),
                  (dict(rows=2 ** 31 - 1, cols=2 ** 31 - 1), "rows * cols"),
                  (dict(dist_x=0.0), "dist_x"), (dict(dist_x=-0.04), "dist_x"), (dict(dist_x=NAN), "dist_x"),
                  (dict(dist_x=INF), "dist_x"), (dict(dist_y=0.0), "dist_y"), (dict(dist_y=NAN), "dist_y"),
                  (dict(dist_y=INF), "dist_y"), (dict(ray_z=NAN), "ray_z"), (dict(ray_z=INF), "ray_z"),
                  (dict(ray_z=-INF), "ray_z")]


def test_patches_device_refuses_bad_arguments_with_a_message():
    fn, what = lib.srbd_terrain_patches_device, "srbd_terrain_patches_device"
    assert fn(None, 3, C.byref(patch_io()), None) == _lib.E_INVALID
    assert what in terrain_error() and "null terrain" in terrain_error()
    assert fn(PTR, 3, None, None) == _lib.E_INVALID and "null io" in terrain_error()
    for n in (0, -1, 4097, 2 ** 31 - 1):
        assert fn(PTR, n, C.byref(patch_io()), None) == _lib.E_INVALID, n
        assert "num_envs" in terrain_error() and "1..4096" in terrain_error()
    for over, why in PATCH_IO_CASES:
        assert fn(PTR, 3, C.byref(patch_io(**over)), None) == _lib.E_INVALID, over
        assert what in terrain_error() and why in terrain_error(), (over, terrain_error())
    # heights alone, points alone and the 320-ray lattice are not refused for their arguments: the next check follows
    # the handle, which this test cannot offer -- see tests/test_gpu_height_scan.py


def test_set_patches_device_refuses_bad_arguments_with_a_message():
    fn, what = lib.srbd_terrain_set_patches_device, "srbd_terrain_set_patches_device"
    assert fn(None, PTR, 3, C.byref(patch_io()), None) == _lib.E_INVALID
    assert what in set_error() and "null set" in set_error()
    assert fn(PTR, None, 3, C.byref(patch_io()), None) == _lib.E_INVALID and "null d_scene" in set_error()
    for odd in (PTR + 1, PTR + 2, PTR + 3):
        assert fn(PTR, odd, 3, C.byref(patch_io()), None) == _lib.E_INVALID, odd
        assert "d_scene" in set_error() and "aligned" in set_error()
    assert fn(PTR, PTR, 3, None, None) == _lib.E_INVALID and "null io" in set_error()
    for n in (0, -1, 4097):
        assert fn(PTR, PTR, n, C.byref(patch_io()), None) == _lib.E_INVALID, n
        assert "num_envs" in set_error()
    for over, why in PATCH_IO_CASES:
        assert fn(PTR, PTR, 3, C.byref(patch_io(**over)), None) == _lib.E_INVALID, over
        assert what in set_error() and why in set_error(), (over, set_error())


# ------------------------------------------------------------------ srbd_vfa_height_step_device / _scenes_device
def step_io(**over):
    f = dict(seeds=PTR, hips=None, forward_vel=None, base_pos=None, contact=PTR, feet=None, yaws=PTR, heightmaps=None,
             rows=13, cols=7, dist_x=0.04, dist_y=0.04, ray_z=10.0, footholds=PTR, boxes=PTR, valid=PTR,
             seed_heights=None, scores=None, heightmaps_out=None, ref=None)
    f.update(over)
    return _lib.TamolsBatchIO(**f)


STEP_IO_CASES = [(dict(contact=None), "contact"), (dict(seeds=None), "seeds"), (dict(footholds=None), "footholds"),
                 (dict(boxes=None), "boxes"), (dict(valid=None), "valid"), (dict(yaws=None), "yaws"),
                 (dict(heightmaps=PTR), "heightmaps"), (dict(rows=0), "rows"), (dict(cols=0), "cols"),
                 (dict(rows=17, cols=20), "rows * cols"), (dict(dist_x=0.0), "dist_x"), (dict(dist_x=NAN), "dist_x"),
                 (dict(dist_y=-1.0), "dist_y"), (dict(dist_y=NAN), "dist_y")]


def test_height_step_refuses_bad_arguments_with_a_message():
    fn, what = lib.srbd_vfa_height_step_device, "srbd_vfa_height_step_device"
    a = step_io()
    assert fn(PTR, PTR, None, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID
    assert what in terrain_error() and "null terrain" in terrain_error()
    assert fn(None, PTR, PTR, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "d_vfa" in terrain_error()
    assert fn(PTR, None, PTR, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "d_stc" in terrain_error()
    assert fn(PTR, PTR, PTR, 3, None, 0.01, None, None) == _lib.E_INVALID and "null io" in terrain_error()
    for bad in (NAN, INF, -INF):
        assert fn(PTR, PTR, PTR, 3, C.byref(a), bad, None, None) == _lib.E_INVALID
        assert "apex_interval" in terrain_error()
    for n in (0, -1, 4097):
        assert fn(PTR, PTR, PTR, n, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "num_envs" in terrain_error()
    for over, why in STEP_IO_CASES:
        assert fn(PTR, PTR, PTR, 3, C.byref(step_io(**over)), 0.01, None, None) == _lib.E_INVALID, over
        assert what in terrain_error() and why in terrain_error(), (over, terrain_error())


def test_height_step_scenes_refuses_bad_arguments_with_a_message():
    fn, what = lib.srbd_vfa_height_step_scenes_device, "srbd_vfa_height_step_scenes_device"
    a = step_io()
    assert fn(PTR, PTR, None, PTR, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID
    assert what in set_error() and "null set" in set_error()
    assert fn(PTR, PTR, PTR, None, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "null d_scene" in set_error()
    assert fn(PTR, PTR, PTR, PTR + 2, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "aligned" in set_error()
    assert fn(None, PTR, PTR, PTR, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "d_vfa" in set_error()
    assert fn(PTR, None, PTR, PTR, 3, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "d_stc" in set_error()
    assert fn(PTR, PTR, PTR, PTR, 3, C.byref(a), NAN, None, None) == _lib.E_INVALID and "apex_interval" in set_error()
    assert fn(PTR, PTR, PTR, PTR, 4097, C.byref(a), 0.01, None, None) == _lib.E_INVALID and "num_envs" in set_error()
    for over, why in STEP_IO_CASES:
        assert fn(PTR, PTR, PTR, PTR, 3, C.byref(step_io(**over)), 0.01, None, None) == _lib.E_INVALID, over
        assert what in set_error() and why in set_error(), (over, set_error())


# ------------------------------------------------------------------ the wrappers' checks
E, K = 3, 2


def fake_set(device_id=0):
    return types.SimpleNamespace(h=C.c_void_p(PTR), num_scenes=2, device_id=device_id)


def fake_terrain():
    return types.SimpleNamespace(h=C.c_void_p(PTR))


def raising(name):
    def f(*a):
        raise AssertionError(f"{name} was called")
    return f


def test_patches_device_wrappers_refuse_bad_tensors_without_calling_c(monkeypatch):
    torch = pytest.importorskip("torch")
    for name in DEVICE_NAMES:
        monkeypatch.setattr(lib, name, raising(name))
    f64 = torch.float64
    centers, yaws = torch.zeros(E, K, 3, dtype=f64), torch.zeros(E, dtype=f64)
    ids = torch.zeros(E, dtype=torch.int32)
    one = lambda **kw: GpuTerrain.patches_device(fake_terrain(), **dict(dict(centers=centers, yaws=yaws), **kw))  # noqa: E731
    many = lambda **kw: GpuTerrainSet.patches_device(fake_set(), **dict(dict(centers=centers, yaws=yaws, scene_ids=ids), **kw))  # noqa: E731
    bad = [(dict(centers=centers.numpy()), "torch tensor"), (dict(centers=centers.float()), "float64"),
           (dict(centers=torch.zeros(E, 3, dtype=f64)), "centers must be"),
           (dict(centers=torch.zeros(E, K, 2, dtype=f64)), "must be"),
           (dict(centers=torch.zeros(E, 17, 3, dtype=f64)), "1..16"),
           (dict(centers=torch.zeros(0, K, 3, dtype=f64)), "1..4096"),
           (dict(centers=torch.zeros(E, K, 6, dtype=f64)[:, :, ::2]), "contiguous"),
           (dict(yaws=yaws.float()), "float64"), (dict(yaws=torch.zeros(E + 1, dtype=f64)), "yaws must be"),
           (dict(yaws=torch.zeros(E, K, dtype=f64)), "yaws must be"), (dict(yaws=[0.0] * E), "torch tensor"),
           (dict(rows=0), "1..320"), (dict(rows=17, cols=20), "1..320"), (dict(dist_x=0.0), "positive and finite"),
           (dict(dist_y=INF), "positive and finite"), (dict(ray_z=NAN), "ray_z"),
           (dict(points=False, heights=False), "points, heights or both"),
           (dict(out=dict(heights=torch.zeros(E, K, 13, 6, dtype=f64))), "must be"),
           (dict(out=dict(height=torch.zeros(1, dtype=f64))), "unknown output"),
           (dict(), "cuda")]  # all right but on the host: refused, not copied
    for kw, match in bad:
        for f in (one, many):
            with pytest.raises(ValueError, match=match):
                f(**kw)
    for kw, match in [(dict(scene_ids=ids.long()), "int32"), (dict(scene_ids=ids.numpy()), "torch tensor"),
                      (dict(scene_ids=torch.zeros(E + 1, dtype=torch.int32)), "must be"),
                      (dict(scene_ids=None), "needs scene_ids")]:
        with pytest.raises(ValueError, match=match):
            many(**kw)
    with pytest.raises(ValueError, match="single GpuTerrain"):
        _lib.terrain_patches_device(fake_terrain(), centers, yaws, scene_ids=ids)


def test_height_strategy_wrapper_refuses_bad_arguments_without_calling_c(monkeypatch):
    torch = pytest.importorskip("torch")
    for name in DEVICE_NAMES + ("srbd_vfa_step_device", "srbd_vfa_step_scenes_device"):
        monkeypatch.setattr(lib, name, raising(name))
    f64 = torch.float64
    seeds, hips, yaws = torch.zeros(E, 4, 3, dtype=f64), torch.zeros(E, 4, 3, dtype=f64), torch.zeros(E, dtype=f64)
    contact = torch.ones(E, 4)
    vfa, stc = torch.zeros(E, _lib.VFA_BYTES, dtype=torch.uint8), torch.zeros(E, _lib.STC_BYTES, dtype=torch.uint8)
    assert BatchedVisualFootholdAdaptation(E).adaptation_strategy == "tamols"  # today's behaviour is the default
    with pytest.raises(ValueError, match="adaptation_strategy"):
        BatchedVisualFootholdAdaptation(E, adaptation_strategy="nearest")
    with pytest.raises(ImportError):
        BatchedVisualFootholdAdaptation(E, adaptation_strategy="vfa")
    b = BatchedVisualFootholdAdaptation(E, adaptation_strategy="height")
    b._state = vfa  # the gate's state on the host: the checks come before any device is touched
    step = lambda **kw: b.step_device(seeds, hips, None, None, contact, None, stc=stc, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="no patch form"):
        step(heightmaps=torch.zeros(E, 4, 2, 2, 3, dtype=f64))
    with pytest.raises(ValueError, match="no patch form"):
        step(terrain=fake_terrain(), yaws=yaws, heightmaps=torch.zeros(E, 4, 2, 2, 3, dtype=f64))
    with pytest.raises(ValueError, match="needs a terrain"):
        step(yaws=yaws)
    with pytest.raises(ValueError, match="needs yaws"):
        step(terrain=fake_terrain())
    with pytest.raises(ValueError, match="needs scene_ids"):
        step(terrain=fake_set(), yaws=yaws)
    with pytest.raises(ValueError, match="single GpuTerrain"):
        step(terrain=fake_terrain(), yaws=yaws, scene_ids=torch.zeros(E, dtype=torch.int32))
    with pytest.raises(ValueError, match="1..320"):
        step(terrain=fake_terrain(), yaws=yaws, rows=17, cols=20)
    with pytest.raises(ValueError, match="no scores"):
        step(terrain=fake_terrain(), yaws=yaws, want_scores=True)
    with pytest.raises(ValueError, match="float64"):
        step(terrain=fake_terrain(), yaws=yaws.float())
    with pytest.raises(ValueError, match="contact flags"):
        b.step_device(seeds, hips, None, None, None, None, stc=stc, terrain=fake_terrain(), yaws=yaws)
    with pytest.raises(ValueError, match="cuda"):  # all right but on the host
        step(terrain=fake_terrain(), yaws=yaws)
    with pytest.raises(ValueError, match="step_device"):
        b.compute_adaptation_device(seeds, hips, None, None, None, None, terrain=fake_terrain(), yaws=yaws)


# ------------------------------------------------------------------ srbd_vfa_height_search against numpy
def get_height(patch, seed):
    """PatchHeightMap.get_height (helpers/terrain.py) on a (rows, cols, 3) patch: the reference's lookup."""
    hm = PatchHeightMap(None)
    hm.data = np.asarray(patch, dtype=np.float64)[:, :, None, :]
    return hm.get_height(seed)


def height_search(patch, seed):
    patch = np.ascontiguousarray(patch, dtype=np.float64)
    f, v = np.full(3, -7.0), C.c_int32(-7)
    seed = np.ascontiguousarray(seed, dtype=np.float64)
    assert lib.srbd_vfa_height_search(_lib.dptr(patch), patch.shape[0], patch.shape[1], _lib.dptr(seed), _lib.dptr(f),
                                      C.byref(v)) == _lib.OK
    return f, v.value


def check_search(patch, seed, what):
    f, v = height_search(patch, seed)
    want = np.array([seed[0], seed[1], get_height(patch, seed)])
    np.testing.assert_array_equal(f, want, err_msg=what)
    assert np.where(np.isnan(want), 0, f).tobytes() == np.where(np.isnan(want), 0, want).tobytes(), what
    assert v == (0 if np.isnan(want[2]) else 1), what
    return f, v


def test_height_search_on_random_patches():
    rng = np.random.default_rng(5)
    for rows, cols in ((1, 1), (3, 5), (13, 7), (16, 20)):
        for trial in range(25):
            hm = PatchHeightMap(lambda x, y: 0.1 * np.sin(7 * x) + 0.05 * np.cos(5 * y), rows, cols)
            patch = hm.update_height_map(rng.uniform(-1, 1, 3), rng.uniform(-3, 3))[:, :, 0, :]
            seed = patch[rows // 2, cols // 2] + rng.uniform(-0.3, 0.3, 3)
            f, v = check_search(patch, seed, f"{rows}x{cols} trial {trial}")
            assert v == 1 and np.isfinite(f).all()


def test_height_search_ties_nan_points_and_misses():
    # two equidistant points: the lower index wins, whichever way round the heights are
    for z in ((1.0, 2.0), (2.0, 1.0)):
        patch = np.array([[[9.0, 0.0, 5.0], [-0.5, 0.0, z[0]], [0.5, 0.0, z[1]], [0.5, 0.0, 7.0]]])
        f, v = check_search(patch, [0.0, 0.0, 3.0], f"tie {z}")
        assert f[2] == z[0] + 0.02 and v == 1
    # a NaN patch point wins numpy's argmin at its first occurrence: before and after the true minimum, and two of them
    base = np.array([[[1.0, 0.0, 1.0], [0.1, 0.0, 2.0], [2.0, 0.0, 3.0], [3.0, 0.0, 4.0]]])
    for at, coord in ((0, 0), (2, 1), (3, 0)):
        patch = base.copy()
        patch[0, at, coord] = np.nan
        f, v = check_search(patch, [0.0, 0.0, 0.0], f"NaN point at {at}")
        assert f[2] == base[0, at, 2] + 0.02 and v == 1
    patch = base.copy()
    patch[0, 3, 0] = patch[0, 2, 1] = np.nan
    assert check_search(patch, [0.0, 0.0, 0.0], "two NaN points")[0][2] == 3.02
    # a NaN seed: every distance is NaN, the first point wins
    assert check_search(base, [np.nan, 0.0, 0.0], "NaN seed")[0][2] == 1.02
    # the nearest point is a miss (z NaN): z NaN and valid 0; a miss elsewhere changes nothing
    patch = base.copy()
    patch[0, 1, 2] = np.nan
    f, v = check_search(patch, [0.0, 0.0, 0.0], "miss at the nearest point")
    assert np.isnan(f[2]) and v == 0 and f[0] == 0.0 and f[1] == 0.0
    patch = base.copy()
    patch[0, 0, 2] = np.nan
    f, v = check_search(patch, [0.0, 0.0, 0.0], "miss elsewhere")
    assert f[2] == 2.02 and v == 1
    # the seed's own z is not read
    assert height_search(base, [0.0, 0.0, 1e300])[0].tolist() == [0.0, 0.0, 2.02]


def test_height_search_refuses_bad_arguments():
    p, s, f, v = np.zeros((1, 1, 3)), np.zeros(3), np.full(3, 4.0), C.c_int32(4)
    d = _lib.dptr
    for args in ((None, 1, 1, d(s), d(f), C.byref(v)), (d(p), 1, 1, None, d(f), C.byref(v)),
                 (d(p), 1, 1, d(s), None, C.byref(v)), (d(p), 1, 1, d(s), d(f), None),
                 (d(p), 0, 1, d(s), d(f), C.byref(v)), (d(p), 1, -1, d(s), d(f), C.byref(v)),
                 (d(p), 17, 20, d(s), d(f), C.byref(v))):
        assert lib.srbd_vfa_height_search(*args) == _lib.E_INVALID
    assert f.tolist() == [4.0] * 3 and v.value == 4
