"""C-ABI and bindings of the device-resident set of terrain scenes and the searches with one scene per environment
(srbd_terrain_set_*, srbd_tamols_batch_scenes_device, srbd_vfa_step_scenes_device, include/srbd_mpc.h;
_lib.TerrainScene, _lib.tamols_batch_device / vfa_step_device with scene_ids; helpers.terrain.GpuTerrainSet).  CPU only:
every SRBD_E_INVALID here is decided before a HIP call, so the dummy pointers are never followed."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.helpers.terrain import GpuTerrainSet
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import (BatchedVisualFootholdAdaptation,
                                                                    tamols_params_struct)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "srbd_mpc.h")
PTR = 0x1000  # non-null, never followed
lib = _lib.lib
PARAMS = tamols_params_struct({}, "go2")
NAMES = ("srbd_terrain_set_create", "srbd_terrain_set_destroy", "srbd_terrain_set_last_error",
         "srbd_terrain_set_num_scenes", "srbd_tamols_batch_scenes_device", "srbd_vfa_step_scenes_device")


def last_error():
    msg = lib.srbd_terrain_set_last_error(None)
    return msg.decode() if msg else ""


def test_symbols_exported_bound_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\sT\s(\w+)$", dyn.stdout, flags=re.M))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        assert re.search(r"^(int|void|const char\*) ?" + name + r"\s*\(", text, flags=re.M), name
    assert lib.srbd_abi_version() == 1


def test_scene_struct_layout():
    S = _lib.TerrainScene
    assert C.sizeof(S) == 80
    offsets = dict(prims=0, nprims=8, has_ground=12, ground_z=16, hfield=24, hf_nx=32, hf_ny=36, hf_x0=40, hf_y0=48,
                   hf_dx=56, hf_dy=64, miss_z=72)
    assert [n for n, _ in S._fields_] == list(offsets)
    for name, off in offsets.items():
        assert getattr(S, name).offset == off, name


def scene(**over):
    f = dict(prims=None, nprims=0, has_ground=1, ground_z=0.0, hfield=None, hf_nx=0, hf_ny=0, hf_x0=0.0, hf_y0=0.0,
             hf_dx=0.0, hf_dy=0.0, miss_z=float("nan"))
    f.update(over)
    return _lib.TerrainScene(**f)


def create(scenes, n=None, out=True):
    arr = (_lib.TerrainScene * max(1, len(scenes)))(*scenes) if scenes is not None else None
    h = C.c_void_p()
    rc = lib.srbd_terrain_set_create(0, arr, len(scenes) if n is None else n, C.byref(h) if out else None)
    assert not h.value or rc == _lib.OK
    if h.value:
        lib.srbd_terrain_set_destroy(h)
    return rc


def test_create_refuses_bad_counts_and_pointers_with_a_message():
    for n in (0, -1, 4097, 2 ** 31 - 1):
        assert create([scene()], n=n) == _lib.E_INVALID, n
        assert "1..4096" in last_error()
    assert create(None, n=1) == _lib.E_INVALID and "scenes" in last_error()
    assert create([scene()], out=False) == _lib.E_INVALID and "out" in last_error()


def test_create_refuses_a_bad_scene_by_its_index():
    """Each thing srbd_terrain_create refuses, on the scene at index 2 of 3, before a device is looked for."""
    one = (_lib.TerrainPrim * 1)(_lib.TerrainPrim(_lib.PRIM_BOX, 0, 0, 0, 0, 1, 1, 1, 0))
    odd = (_lib.TerrainPrim * 2)(_lib.TerrainPrim(_lib.PRIM_CYLINDER, 0, 0, 0, 0, 1, 0, 1, 0),
                                 _lib.TerrainPrim(7, 0, 0, 0, 0, 1, 1, 1, 0))
    z = np.zeros((2, 2))
    hf = dict(hfield=_lib.dptr(z), hf_nx=2, hf_ny=2, hf_dx=0.1, hf_dy=0.1)
    good = [scene(prims=one, nprims=1), scene(**hf)]
    bad = [(dict(nprims=-1), "bad arguments"), (dict(nprims=1, prims=None), "bad arguments"),
           (dict(prims=odd, nprims=2), "unknown primitive type"),
           (dict(hf, hf_nx=1), "height field"), (dict(hf, hf_ny=1), "height field"),
           (dict(hf, hf_dx=0.0), "height field"), (dict(hf, hf_dy=-0.1), "height field"),
           (dict(hf, hf_dx=float("nan")), "height field")]
    for over, why in bad:
        assert create(good + [scene(**over)]) == _lib.E_INVALID, over
        msg = last_error()
        assert "scene 2" in msg and why in msg, (over, msg)
    # the first bad scene is the one named
    assert create([scene(nprims=-1), scene(nprims=-1), scene()]) == _lib.E_INVALID and "scene 0" in last_error()
    # height-field points that together do not fit the index type (no height is read before the refusal)
    big = dict(hf, hf_nx=40000, hf_ny=40000)
    assert create([scene(**big), scene(**big)]) == _lib.E_INVALID
    assert "scene 1" in last_error() and "2^31" in last_error()


@pytest.mark.skipif(_lib.device_count() > 0, reason="with a device the set would be created")
def test_no_device_is_reported():
    z = np.zeros((2, 2))
    assert create([scene(), scene(hfield=_lib.dptr(z), hf_nx=2, hf_ny=2, hf_dx=0.1, hf_dy=0.1)]) == _lib.E_NODEVICE
    assert "no HIP device" in last_error()
    with pytest.raises(RuntimeError, match="srbd_terrain_set_create"):
        GpuTerrainSet([dict(prims=[], has_ground=True), dict(prims=[], has_ground=False)])


def test_python_set_checks_its_scenes_on_the_host():
    with pytest.raises(RuntimeError, match="1..4096"):
        GpuTerrainSet([])
    with pytest.raises(ValueError, match="scene 1: unknown keys"):
        GpuTerrainSet([dict(prims=[]), dict(prims=[], ground=True)])
    with pytest.raises(RuntimeError, match="scene 1: unknown primitive type"):
        GpuTerrainSet([dict(prims=[]), dict(prims=[dict(type=5, cx=0, cy=0, cz=0, a=1, c=1)])])


def io(**over):
    f = dict(seeds=PTR, hips=PTR, forward_vel=None, base_pos=None, contact=PTR, feet=None, yaws=PTR, heightmaps=None,
             rows=13, cols=7, dist_x=0.04, dist_y=0.04, ray_z=10.0, footholds=PTR, boxes=PTR, valid=PTR,
             seed_heights=None, scores=None, heightmaps_out=None, ref=None)
    f.update(over)
    return _lib.TamolsBatchIO(**f)


def test_null_set_is_refused_with_a_message_and_null_handles_are_harmless():
    a = io()
    assert lib.srbd_tamols_batch_scenes_device(None, PTR, C.byref(PARAMS), 4, C.byref(a), None) == _lib.E_INVALID
    assert "srbd_tamols_batch_scenes_device" in last_error() and "null set" in last_error()
    assert lib.srbd_vfa_step_scenes_device(PTR, PTR, None, PTR, C.byref(PARAMS), 4, C.byref(a), 0.01, None,
                                           None) == _lib.E_INVALID
    assert "srbd_vfa_step_scenes_device" in last_error() and "null set" in last_error()
    lib.srbd_terrain_set_destroy(None)
    assert lib.srbd_terrain_set_num_scenes(None) == _lib.E_INVALID


# ------------------------------------------------------------------ the wrappers' checks
E = 3


def fake_set(device_id=0):
    return types.SimpleNamespace(h=C.c_void_p(PTR), num_scenes=2, device_id=device_id)


def fake_terrain():
    return types.SimpleNamespace(h=C.c_void_p(PTR))


def test_wrappers_refuse_bad_scene_arguments_without_calling_c(monkeypatch):
    torch = pytest.importorskip("torch")
    calls = []
    for name in ("srbd_tamols_batch_device", "srbd_tamols_batch_scenes_device", "srbd_vfa_step_device",
                 "srbd_vfa_step_scenes_device"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append(_n) or _lib.OK)
    f64 = torch.float64
    seeds, hips, yaws = torch.zeros(E, 4, 3, dtype=f64), torch.zeros(E, 4, 3, dtype=f64), torch.zeros(E, dtype=f64)
    contact = torch.ones(E, 4)
    ids = torch.zeros(E, dtype=torch.int32)
    hms = torch.zeros(E, 4, 2, 2, 3, dtype=f64)
    vfa, stc = torch.zeros(E, _lib.VFA_BYTES, dtype=torch.uint8), torch.zeros(E, _lib.STC_BYTES, dtype=torch.uint8)
    batched = BatchedVisualFootholdAdaptation(E)

    def calls_of(**kw):
        yield lambda: _lib.tamols_batch_device(seeds, hips, PARAMS, **kw)
        yield lambda: _lib.vfa_step_device(vfa, stc, seeds, hips, PARAMS, contact, **kw)
        yield lambda: batched.compute_adaptation_device(seeds, hips, None, None, None, None, **kw)

    bad = [(dict(terrain=fake_set(), yaws=yaws), "needs scene_ids"),
           (dict(terrain=fake_terrain(), yaws=yaws, scene_ids=ids), "single GpuTerrain"),
           (dict(heightmaps=hms, scene_ids=ids), "no scenes"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=ids.long()), "int32"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=ids.numpy()), "torch tensor"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=torch.zeros(E + 1, dtype=torch.int32)), "must be"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=torch.zeros(E, 1, dtype=torch.int32)), "must be"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=torch.zeros(2 * E, dtype=torch.int32)[::2]), "contiguous"),
           (dict(terrain=fake_set(), yaws=yaws, scene_ids=ids), "cuda")]  # all right but on the host: not copied
    for kw, match in bad:
        for f in calls_of(**kw):
            with pytest.raises(ValueError, match=match):
                f()
    batched._state = vfa  # the gate's state on the host: the checks come before any device is touched
    with pytest.raises(ValueError, match="needs scene_ids"):
        batched.step_device(seeds, hips, None, None, contact, None, stc=stc, terrain=fake_set(), yaws=yaws)
    assert not calls


@pytest.mark.gpu
def test_scene_ids_on_another_device_than_the_set_are_refused(monkeypatch):
    torch = pytest.importorskip("torch")
    calls = []
    monkeypatch.setattr(lib, "srbd_tamols_batch_scenes_device", lambda *a: calls.append(a) or _lib.OK)
    f64 = torch.float64
    seeds = torch.zeros(E, 4, 3, dtype=f64, device="cuda:0")
    with pytest.raises(ValueError, match="set's device"):
        _lib.tamols_batch_device(seeds, seeds.clone(), PARAMS, terrain=fake_set(device_id=1),
                                 yaws=torch.zeros(E, dtype=f64, device="cuda:0"),
                                 scene_ids=torch.zeros(E, dtype=torch.int32, device="cuda:0"))
    assert not calls
