"""Device-resident height scans (GpuTerrain.patches_device, GpuTerrainSet.patches_device) and the 'height' strategy
behind the apex gate (_lib.vfa_height_step_device, BatchedVisualFootholdAdaptation(adaptation_strategy='height'))
against their equivalence contracts.  The scans: byte for byte heightmaps_out of srbd_tamols_batch_scenes_device for the
same centres (which tests/test_gpu_terrain_set.py and tests/test_gpu_tamols_batch.py pin to the single calls and the
oracle) and, on yaws whose libm cos / sin are the device's, the host-array GpuTerrain.patches.  The gated step: the host
chain srbd_vfa_mode -> srbd_vfa_height_search on the scans -> srbd_vfa_commit.  Every comparison is exact, NaNs position
for position; no tolerance appears here."""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
SENT = 7.25  # sentinel of the not-to-be-written entries
INTERVAL = 0.01
LATTICES = [(1, 1), (3, 5), (13, 7), (16, 20)]
SHAPES = [(3, 5), (3, 1), (1, 5), (1, 1)]  # (E, K)
YAW_SEED, YAW_DRAWS = 3, 8


def scenes():
    """Flat ground; yawed boxes over ground; cylinders without ground (a miss is NaN); a height field."""
    rng = np.random.default_rng(21)
    boxes = [dict(type=0, cx=rng.uniform(-0.5, 1.5), cy=rng.uniform(-0.6, 0.6), cz=0.0, a=rng.uniform(0.03, 0.2),
                  b=rng.uniform(0.03, 0.2), c=rng.uniform(0.01, 0.1), yaw=rng.uniform(-3, 3)) for _ in range(40)]
    cyls = [dict(type=1, cx=rng.uniform(-0.5, 1.5), cy=rng.uniform(-0.6, 0.6), cz=0.0, a=rng.uniform(0.05, 0.2),
                 b=0.0, c=rng.uniform(0.01, 0.1), yaw=0.0) for _ in range(30)]
    hf = dict(z=rng.uniform(0.0, 0.08, (23, 17)), x0=-0.7, y0=-0.9, dx=0.11, dy=0.13)
    return [dict(prims=[], has_ground=True, ground_z=0.015), dict(prims=boxes, has_ground=True, ground_z=-0.02),
            dict(prims=cyls, has_ground=False), dict(prims=[], has_ground=False, miss_z=-1.0, hfield=hf)]


EMPTY = dict(prims=(), has_ground=False)
IDS = {3: [1, 3, 2], 1: [2]}


def yaws_checked():
    """YAW_DRAWS yaws of seed YAW_SEED, yaw 0 first, and which of them numpy's cos / sin agree on with the device's
    (srbd_selftest_yaw_sincos, the kernel's host twin), bit for bit."""
    from quadruped_pympc_amd import _lib

    yaws = np.concatenate([[0.0], np.random.default_rng(YAW_SEED).uniform(-3.1, 3.1, YAW_DRAWS - 1)])
    cs = np.zeros((len(yaws), 2))
    assert _lib.lib.srbd_selftest_yaw_sincos(_lib.dptr(yaws), len(yaws), _lib.dptr(cs)) == _lib.OK
    agree = np.array([cs[i, 0].tobytes() == np.cos(yaws[i]).tobytes() and cs[i, 1].tobytes() == np.sin(yaws[i]).tobytes()
                      for i in range(len(yaws))])
    return yaws, agree


def test_yaw_seed_keeps_at_least_half_of_the_draws():
    """CPU: the drawn yaws of the host-array comparison below; at most half may be filtered out."""
    yaws, agree = yaws_checked()
    assert yaws[0] == 0.0 and agree[0]
    assert agree.sum() * 2 >= len(yaws), agree


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


@pytest.fixture(scope="module")
def world(lib):
    """The four-scene set, a GpuTerrain of each scene and of the empty scene, closed at the end."""
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain, GpuTerrainSet

    sc = scenes()
    w = dict(scenes=sc, set=GpuTerrainSet(sc), single=[GpuTerrain(**s) for s in sc], empty=GpuTerrain(**EMPTY))
    yield w
    w["set"].close()
    for t in w["single"] + [w["empty"]]:
        t.close()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)  # NaNs position for position
    if want.dtype.kind == "f":  # a NaN's sign and payload are not part of the contract
        nan = np.isnan(want)
        assert np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes(), what


def centers_of(E, K, seed=0):
    rng = np.random.default_rng(100 * E + K + seed)
    c = np.stack([rng.uniform(-0.3, 1.3, (E, K)), rng.uniform(-0.5, 0.5, (E, K)), rng.uniform(-1, 1, (E, K))], -1)
    yaws = np.array([0.0, 0.3, -1.2, 2.5])[:E] if E > 1 else np.array([-0.7])
    return c, yaws


def ids_tensor(ids):
    return torch.tensor(list(ids), dtype=torch.int32, device="cuda")


_scans = {}


def scan(world, E, K, rows, cols):
    """patches_device on the set for the case's centres, computed once and shared: (centres, yaws, points, heights)."""
    key = (E, K, rows, cols)
    if key not in _scans:
        c, yaws = centers_of(E, K)
        pts, h = world["set"].patches_device(cuda(c), cuda(yaws), rows, cols, points=True, heights=True,
                                             scene_ids=ids_tensor(IDS[E]))
        torch.cuda.synchronize()
        _scans[key] = (c, yaws, pts.cpu().numpy(), h.cpu().numpy())
    return _scans[key]


def tamols_patches(lib, terrain, c, yaws, rows, cols, scene_ids=None):
    """heightmaps_out of the batched TAMOLS search with the centres as seeds, four at a time (the last repeated)."""
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import tamols_params_struct

    E, K = c.shape[:2]
    out = np.zeros((E, K, rows, cols, 3))
    for k0 in range(0, K, 4):
        idx = [min(k, K - 1) for k in range(k0, k0 + 4)]
        seeds = cuda(c[:, idx])
        kw = {} if scene_ids is None else dict(scene_ids=ids_tensor(scene_ids))
        got = lib.tamols_batch_device(seeds, seeds + torch.tensor([0.0, 0.0, 0.3], device="cuda", dtype=torch.float64),
                                      tamols_params_struct({}, "go2"), terrain=terrain, yaws=cuda(yaws), rows=rows,
                                      cols=cols, want_heightmaps=True, **kw)
        torch.cuda.synchronize()
        n = min(4, K - k0)
        out[:, k0:k0 + n] = got["heightmaps"].cpu().numpy()[:, :n]
    return out


# ------------------------------------------------------------------ 1: the scans against the TAMOLS launch's patches
@gpu
@pytest.mark.parametrize("E,K", SHAPES)
@pytest.mark.parametrize("rows,cols", LATTICES)
def test_scan_equals_the_search_launch_patches(lib, world, E, K, rows, cols):
    c, yaws, pts, h = scan(world, E, K, rows, cols)
    want = tamols_patches(lib, world["set"], c, yaws, rows, cols, scene_ids=IDS[E])
    same_bits(pts, want, f"E={E} K={K} {rows}x{cols}: points")
    same_bits(h, pts[..., 2], "heights is points[..., 2]")
    # each output alone writes the same bytes, into the caller's tensor
    d = dict(centers=cuda(c), yaws=cuda(yaws), rows=rows, cols=cols, scene_ids=ids_tensor(IDS[E]))
    only_h = torch.full((E, K, rows, cols), SENT, dtype=torch.float64, device="cuda")
    assert world["set"].patches_device(points=False, heights=True, out=dict(heights=only_h), **d) is only_h
    only_p = world["set"].patches_device(**d)
    torch.cuda.synchronize()
    same_bits(only_h, h, "heights alone")
    same_bits(only_p, pts, "points alone")
    if rows >= 13 and E == 3:  # the scenes do differ, rays miss where there is no ground, and hit elsewhere
        assert np.isnan(h[2]).any() and np.isfinite(h[0]).all() and len({h[e].tobytes() for e in range(E)}) == E


@gpu
@pytest.mark.parametrize("s", range(4))
def test_shared_scene_form_equals_a_one_scene_set(lib, world, s):
    from quadruped_pympc_amd.helpers.terrain import GpuTerrainSet

    E, K, rows, cols = 3, 5, 13, 7
    c, yaws = centers_of(E, K, seed=s)
    one = GpuTerrainSet([world["scenes"][s]])
    a = world["single"][s].patches_device(cuda(c), cuda(yaws), rows, cols, points=True, heights=True)
    b = one.patches_device(cuda(c), cuda(yaws), rows, cols, points=True, heights=True, scene_ids=ids_tensor([0] * E))
    torch.cuda.synchronize()
    same_bits(a[0], b[0], f"scene {s}: points")
    same_bits(a[1], b[1], f"scene {s}: heights")
    same_bits(a[0], tamols_patches(lib, world["single"][s], c, yaws, rows, cols), f"scene {s}: srbd_tamols_batch_device")
    one.close()


# ------------------------------------------------------------------ 2: the host-array call, on yaws libm agrees on
@gpu
@pytest.mark.parametrize("rows,cols", LATTICES)
def test_scan_equals_the_host_array_patches(lib, world, rows, cols):
    yaws, agree = yaws_checked()
    yaws = yaws[agree]
    assert yaws[0] == 0.0 and len(yaws) * 2 >= YAW_DRAWS
    E, K = len(yaws), 5
    ids = [e % 4 for e in range(E)]
    c = centers_of(E, K)[0]
    got = world["set"].patches_device(cuda(c), cuda(yaws), rows, cols, scene_ids=ids_tensor(ids))
    torch.cuda.synchronize()
    for e in range(E):
        want = world["single"][ids[e]].patches(c[e], np.full(K, yaws[e]), rows, cols)
        same_bits(got[e], want, f"environment {e} (scene {ids[e]}, yaw {yaws[e]}) {rows}x{cols}")


# ------------------------------------------------------------------ 3: bad indices, NaN centres
@gpu
def test_bad_indices_scan_the_empty_scene_and_environments_are_independent(lib, world):
    E, K, rows, cols = 3, 5, 13, 7
    c, yaws, pts, h = scan(world, E, K, rows, cols)
    empty = world["empty"].patches_device(cuda(c), cuda(yaws), rows, cols).cpu().numpy()
    assert np.isnan(empty[..., 2]).all()
    for bad in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        ids = list(IDS[E])
        ids[1] = bad
        got = world["set"].patches_device(cuda(c), cuda(yaws), rows, cols, scene_ids=ids_tensor(ids)).cpu().numpy()
        same_bits(got[1], empty[1], f"index {bad}: the empty scene's output")
        same_bits(got[[0, 2]], pts[[0, 2]], f"index {bad}: the others")
    for poison in ("centre", "yaw"):
        c2, y2 = c.copy(), yaws.copy()
        if poison == "centre":
            c2[1, 2, 0] = np.nan
        else:
            y2[1] = np.nan
        got = world["set"].patches_device(cuda(c2), cuda(y2), rows, cols, scene_ids=ids_tensor(IDS[E])).cpu().numpy()
        same_bits(got[[0, 2]], pts[[0, 2]], f"NaN {poison}: the others")
        assert np.isnan(got[1, 2, ..., 0]).all()
        if poison == "centre":
            same_bits(got[1, [0, 1, 3, 4]], pts[1, [0, 1, 3, 4]], "NaN centre: the environment's other patches")


# ------------------------------------------------------------------ 4: the gated 'height' step
# What each environment's clocks and contacts are at each of the 12 calls: 'apex' (one leg in swing at half its
# period), 'swing' (that leg early in its swing) or 'stance' (all four legs down, which releases a held search).
PLAN = ["swing swing apex swing apex swing stance swing apex swing stance swing".split(),   # P P S H H H P P S H P P
        "apex swing swing stance swing swing apex apex swing swing swing stance".split(),   # S H H P P P S H H H H P
        "swing stance swing swing apex swing stance apex swing stance swing apex".split()]  # P P P P S H P S H P P S
PERIOD = 0.25
CALLS = 12


def gate_inputs(lib, E, k):
    """Call k's srbd_stc structs, contact flags and seeds (which move with k, so a held foothold is not the seed)."""
    stc = (lib.SrbdStc * E)()
    contact = np.ones((E, 4), dtype=np.float32)
    for e in range(E):
        assert lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, PERIOD, 500.0, 10.0, lib.SWING_BEZIER_REF) == 0
        what, leg = PLAN[e][k], (e + 1) % 4
        if what != "stance":
            contact[e, leg] = 0.0
            stc[e].swing_time[leg] = PERIOD / 2.0 if what == "apex" else 0.02
    c, yaws = centers_of(E, 4, seed=7)
    return stc, contact, c + [0.013 * k, -0.007 * k, 0.0], yaws


def host_chain(lib, vfa, stc, contact, seeds, patches):
    """The contract's right-hand side on host structs (stepped in place): srbd_vfa_mode, srbd_vfa_height_search on the
    scans of a searching environment, srbd_vfa_commit with NaN boxes."""
    E = len(vfa)
    rows, cols = patches.shape[2:4]
    p, ip = lib.dptr, lib.iptr
    want = dict(footholds=np.zeros((E, 4, 3)), boxes=np.zeros((E, 4, 2, 3)), valid=np.zeros((E, 4), np.int32),
                mode=np.zeros(E, np.int32), seed_heights=np.full((E, 4), SENT),
                heightmaps=np.full((E, 4, rows, cols, 3), SENT))
    for e in range(E):
        m = C.c_int32(-1)
        ct = np.ascontiguousarray(contact[e], dtype=np.float64)
        assert lib.lib.srbd_vfa_mode(C.byref(vfa[e]), C.byref(stc[e]), p(ct), INTERVAL, C.byref(m)) == 0
        sf = sb = sv = None
        if m.value == lib.VFA_SEARCH:
            sf, sb, sv = np.zeros((4, 3)), np.full((4, 2, 3), np.nan), np.zeros(4, np.int32)
            for leg in range(4):
                v = C.c_int32(-1)
                assert lib.lib.srbd_vfa_height_search(p(np.ascontiguousarray(patches[e, leg])), rows, cols,
                                                      p(np.ascontiguousarray(seeds[e, leg])), p(sf[leg]), C.byref(v)) == 0
                sv[leg] = v.value
            want["seed_heights"][e] = sf[:, 2]
            want["heightmaps"][e] = patches[e]
        assert lib.lib.srbd_vfa_commit(C.byref(vfa[e]), m.value, p(np.ascontiguousarray(seeds[e])), p(sf), p(sb), ip(sv),
                                       p(want["footholds"][e]), p(want["boxes"][e]), ip(want["valid"][e])) == 0
        want["mode"][e] = m.value
    want["ref"] = np.concatenate([np.full((E, 12), SENT), want["footholds"].reshape(E, 12)], axis=1)
    return want


def initial_state(lib, E):
    """srbd_vfa_init structs, some legs holding a box already (as after a TAMOLS search): what a miss must keep."""
    vfa = (lib.SrbdVfa * E)()
    for e in range(E):
        assert lib.lib.srbd_vfa_init(C.byref(vfa[e])) == 0
        for k in range(6):
            vfa[e].boxes[6 * ((e + 2) % 4) + k] = 0.1 * k - e
    return vfa


def struct_tensor(structs, nbytes):
    return cuda(np.frombuffer(bytes(structs), dtype=np.uint8).reshape(len(structs), nbytes).copy())


def device_call(lib, terrain, ids, vfa_t, stc, contact, seeds, yaws, rows, cols, step=None):
    """One gated call with every optional output prefilled with the sentinel; `step`: the class's step_device."""
    E = len(stc)
    out = dict(seed_heights=torch.full((E, 4), SENT, dtype=torch.float64, device="cuda"),
               heightmaps=torch.full((E, 4, rows, cols, 3), SENT, dtype=torch.float64, device="cuda"))
    ref = torch.full((E, 24), SENT, dtype=torch.float64, device="cuda")
    kw = dict(terrain=terrain, yaws=cuda(yaws), rows=rows, cols=cols, ref=ref, out=out)
    if ids is not None:
        kw["scene_ids"] = ids_tensor(ids)
    stc_t = struct_tensor(stc, lib.STC_BYTES)
    if step is None:
        got = lib.vfa_height_step_device(vfa_t, stc_t, cuda(seeds), cuda(contact), apex_interval=INTERVAL, **kw)
    else:
        f, b, v, m = step(cuda(seeds), None, None, None, cuda(contact), None, stc=stc_t, apex_interval=INTERVAL, **kw)
        got = dict(out, footholds=f, boxes=b, valid=v, mode=m)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in got.items()}
    res["ref"] = ref.cpu().numpy()
    res["state"] = vfa_t.cpu().numpy().copy()
    assert stc_t.cpu().numpy().tobytes() == bytes(stc), "d_stc is read only"
    return res


_sequences = {}


def sequence(lib, world, E, rows, cols):
    """The 12 calls on the set, each checked against the host chain; the per-call device results, shared."""
    key = (E, rows, cols)
    if key in _sequences:
        return _sequences[key]
    vfa = initial_state(lib, E)
    vfa_t = struct_tensor(vfa, lib.VFA_BYTES)
    seen, results = set(), []
    for k in range(CALLS):
        stc, contact, seeds, yaws = gate_inputs(lib, E, k)
        patches = world["set"].patches_device(cuda(seeds), cuda(yaws), rows, cols,
                                              scene_ids=ids_tensor(IDS[E])).cpu().numpy()
        want = host_chain(lib, vfa, stc, contact, seeds, patches)
        got = device_call(lib, world["set"], IDS[E], vfa_t, stc, contact, seeds, yaws, rows, cols)
        for name, w in want.items():
            same_bits(got[name], w, f"call {k}: {name}")
        assert got["state"].tobytes() == bytes(vfa), f"call {k}: srbd_vfa bytes"
        seen.add(tuple(want["mode"].tolist()))
        results.append(got)
    _sequences[key] = results
    modes = np.array([r["mode"] for r in results])
    for e in range(E):  # every environment passes, searches, holds and releases, at calls of its own
        assert set(modes[:, e].tolist()) == {lib.VFA_PASS, lib.VFA_SEARCH, lib.VFA_HOLD}, modes[:, e]
    assert E == 1 or len(seen) > 4
    return results


@gpu
@pytest.mark.parametrize("E,rows,cols", [(E, r, c) for E in (3, 1) for r, c in LATTICES])
def test_gated_height_step_equals_the_host_chain(lib, world, E, rows, cols):
    results = sequence(lib, world, E, rows, cols)
    if E == 3 and rows * cols > 1:
        valid = np.concatenate([r["valid"][r["mode"] == lib.VFA_SEARCH] for r in results])
        assert (valid == 1).any(), "some searching leg's ray hit"


@gpu
def test_scenes_form_equals_the_shared_form_scene_by_scene(lib, world):
    E, rows, cols = 3, 13, 7
    results = sequence(lib, world, E, rows, cols)
    for s in sorted(set(IDS[E])):
        mine = [e for e in range(E) if IDS[E][e] == s]
        vfa_t = struct_tensor(initial_state(lib, E), lib.VFA_BYTES)
        for k in range(CALLS):
            stc, contact, seeds, yaws = gate_inputs(lib, E, k)
            got = device_call(lib, world["single"][s], None, vfa_t, stc, contact, seeds, yaws, rows, cols)
            for name in ("footholds", "boxes", "valid", "mode", "seed_heights", "heightmaps", "ref", "state"):
                same_bits(got[name][mine], results[k][name][mine], f"scene {s}, call {k}: {name}")


# ------------------------------------------------------------------ 5: the class, and a reset
@gpu
def test_class_with_the_height_strategy_and_a_loop_reset(lib, world):
    from quadruped_pympc_amd.helpers.loop_reset import BatchedLoopReset
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

    E, rows, cols = 3, 13, 7
    results = sequence(lib, world, E, rows, cols)
    b = BatchedVisualFootholdAdaptation(E, adaptation_strategy="height")
    b.load_state_dict(initial_state(lib, E))
    reset = BatchedLoopReset(E, vfa=b)
    for k in range(CALLS):
        stc, contact, seeds, yaws = gate_inputs(lib, E, k)
        got = device_call(lib, world["set"], IDS[E], b.state, stc, contact, seeds, yaws, rows, cols, step=b.step_device)
        for name in ("footholds", "boxes", "valid", "mode", "seed_heights", "heightmaps", "ref", "state"):
            same_bits(got[name], results[k][name], f"call {k}: {name}")
    # all three made to hold (environment 2 still holds call 11's search); a reset of environment 0: it passes its seeds
    # through again, the others hold
    stc, contact, seeds, yaws = gate_inputs(lib, E, 0)
    stc[0].swing_time[1] = PERIOD / 2.0
    first = device_call(lib, world["set"], IDS[E], b.state, stc, contact, seeds, yaws, rows, cols, step=b.step_device)
    assert first["mode"].tolist() == [lib.VFA_SEARCH, lib.VFA_SEARCH, lib.VFA_HOLD]
    reset.reset(torch.tensor([True, False, False], device="cuda"))
    stc, contact, seeds2, yaws = gate_inputs(lib, E, 1)  # 'swing' for environments 0 and 1, 'stance' for 2
    contact[2, 3] = 0.0
    stc[2].swing_time[3] = 0.02
    after = device_call(lib, world["set"], IDS[E], b.state, stc, contact, seeds2, yaws, rows, cols, step=b.step_device)
    assert after["mode"].tolist() == [lib.VFA_PASS, lib.VFA_HOLD, lib.VFA_HOLD]
    same_bits(after["footholds"][0], seeds2[0], "the restarted environment returns its seeds")
    same_bits(after["footholds"][1:], first["footholds"][1:], "the others hold their searches")
    assert not np.array_equal(after["footholds"][1], seeds2[1])


# ------------------------------------------------------------------ 6: one launch, no synchronisation
@gpu
def test_calls_return_while_their_stream_is_busy(lib, world):
    E, K, rows, cols = 3, 5, 13, 7
    c, yaws, pts, h = scan(world, E, K, rows, cols)
    results = sequence(lib, world, E, rows, cols)
    stc, contact, seeds, yaws4 = gate_inputs(lib, E, 0)
    stc[0].swing_time[1] = PERIOD / 2.0  # environment 0 searches
    d = dict(c=cuda(c), yaws=cuda(yaws), ids=ids_tensor(IDS[E]), seeds=cuda(seeds), contact=cuda(contact),
             yaws4=cuda(yaws4), stc=struct_tensor(stc, lib.STC_BYTES),
             vfa=struct_tensor(initial_state(lib, E), lib.VFA_BYTES))
    produced = torch.zeros_like(d["c"])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(50_000_000)  # tens of milliseconds of device time ahead of everything below
        produced.copy_(d["c"])          # the centres exist only once the stream gets here
        got = world["set"].patches_device(produced, d["yaws"], rows, cols, points=True, heights=True,
                                          scene_ids=d["ids"], stream=s)
        step = lib.vfa_height_step_device(d["vfa"], d["stc"], d["seeds"], d["contact"], terrain=world["set"],
                                          yaws=d["yaws4"], scene_ids=d["ids"], rows=rows, cols=cols, stream=s)
        busy = not s.query()
    assert busy, "a call waited for the device"
    s.synchronize()
    same_bits(got[0], pts, "stream order: points")
    same_bits(got[1], h, "stream order: heights")
    assert step["mode"].tolist() == [lib.VFA_SEARCH, lib.VFA_SEARCH, lib.VFA_PASS]
    same_bits(step["footholds"][1], results[0]["footholds"][1], "stream order: the searched footholds")
