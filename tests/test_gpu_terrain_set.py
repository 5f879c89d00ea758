"""One terrain scene per environment (srbd_terrain_set_*, srbd_tamols_batch_scenes_device,
srbd_vfa_step_scenes_device; GpuTerrainSet with scene_ids) against its equivalence contract: every output of
environment e holds the bytes the shared-scene call (tamols_batch_device / vfa_step_device on a GpuTerrain, which
tests/test_gpu_tamols_batch.py and tests/test_gpu_vfa_gate_device.py pin to the single-environment calls, the oracles
and the host gate) writes for that environment's inputs on a GpuTerrain built from the same scene dict.  The expected
values are that call run over all E inputs once per scene, keeping the rows whose id is that scene; they never come from
the new path.  Every comparison is exact, NaNs position for position."""
import numpy as np
import pytest
import torch

from oracle import terrain_oracle
from test_gpu_tamols_batch import FEET, batch_call, cuda, hfield_scene, inputs, same, stacked_boxes_scene
from test_gpu_vfa_gate_device import INTERVAL, SENT, gate_state, same_bits, struct_tensor

from quadruped_pympc_amd import config as mirror

pytestmark = pytest.mark.gpu
ALL = ("vel", "base", "contact", "feet")
EMPTY = dict(prims=(), has_ground=False)  # what an index outside the set stands on (miss_z NaN)


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


@pytest.fixture(scope="module")
def params():
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import tamols_params_struct

    p = dict(mirror.simulation_params["tamols_params"])
    p["h_des"] = 0.25
    return tamols_params_struct(p, "go2")


def hfield2_scene():
    """A second height field of another shape, origin and spacing than hfield_scene's 48 x 40."""
    rng = np.random.default_rng(13)
    return dict(prims=[], has_ground=True, ground_z=-0.3,
                hfield=dict(z=rng.uniform(0.0, 0.08, (7, 9)), x0=0.2, y0=-0.45, dx=0.37, dy=0.12))


def raised_scene():
    """stacked_boxes_scene's primitives, the same xy region, every top 0.03 m higher."""
    s = stacked_boxes_scene()
    return dict(s, prims=[dict(q, cz=q["cz"] + 0.03) for q in s["prims"]])


@pytest.fixture(scope="module")
def world(lib):
    """The scene dicts by name and a cache of the GpuTerrain of each (the reference side), closed at the end."""
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain, stepping_stones_scene

    scenes = dict(stones=stepping_stones_scene(), hfield=hfield_scene(), hfield2=hfield2_scene(),
                  ground=dict(prims=[], has_ground=True), stacked=stacked_boxes_scene(),
                  stacked_noground=stacked_boxes_scene(False), bare=dict(prims=[], has_ground=True, ground_z=-0.02),
                  raised=raised_scene(), empty=EMPTY)
    made = {}

    def terrain(name):
        if name not in made:
            made[name] = GpuTerrain(**scenes[name])
        return made[name]

    yield scenes, terrain
    for t in made.values():
        t.close()


def make_set(world, names):
    from quadruped_pympc_amd.helpers.terrain import GpuTerrainSet

    s = GpuTerrainSet([world[0][n] for n in names])
    assert s.num_scenes == len(names)
    return s


def names_of(names, ids):
    """The scene every environment stands on: its set entry, or the empty scene for an index outside the set."""
    return [names[i] if 0 <= i < len(names) else "empty" for i in ids]


def expected(lib, world, per_env, p, inp, rows, cols, use=ALL):
    """The shared-scene call over all E inputs once per scene, the rows of each scene's environments kept."""
    want = None
    per_env = np.array(per_env)
    for name in sorted(set(per_env)):
        got = batch_call(lib, world[1](name), p, inp, rows, cols, use=use)
        if want is None:
            want = {k: np.full_like(v, 0) for k, v in got.items()}
        for k, v in got.items():
            want[k][per_env == name] = v[per_env == name]
    return want


def scenes_call(lib, tset, ids, p, inp, rows, cols, use=ALL, **kw):
    return batch_call(lib, tset, p, inp, rows, cols, use=use,
                      scene_ids=torch.tensor(list(ids), dtype=torch.int32, device="cuda"), **kw)


def test_mixed_scenes(lib, world, params):
    names = ["stones", "hfield", "hfield2", "ground", "stacked_noground"]
    ids = [3, 0, 4, 1, 2, 0, 4, 2, 1]
    E = len(ids)
    inp = inputs(E, 501)
    inp["seeds"][2, :, :2] = (FEET + [0.12, 0, 0])[:, :2]  # one of the stacked environments on the pile
    want = expected(lib, world, names_of(names, ids), params, inp, 13, 7)
    tset = make_set(world, names)
    ref = torch.full((E, 24), SENT, dtype=torch.float64, device="cuda")
    got = scenes_call(lib, tset, ids, params, inp, 13, 7, ref=ref)
    same(got, want, "mixed scenes")
    np.testing.assert_array_equal(ref[:, 12:].cpu().numpy(), want["footholds"].reshape(E, 12))
    assert (ref[:, :12] == SENT).all()
    # the scenes do differ under these inputs, and rays miss where there is no ground
    assert np.isnan(want["heightmaps"][[2, 6], ..., 2]).any() and want["valid"].any()
    assert len({want["heightmaps"][e, ..., 2].tobytes() for e in range(E)}) >= 5
    tset.close()


def test_slice_boundaries(lib, world, params):
    """Scene 1 holds more primitives within reach than the culled list, so its rays walk the whole scene from global
    memory: exactly its own slice of the concatenated arrays, with an empty-primitive scene before it and a scene of
    higher tops over the same region behind it."""
    names = ["bare", "stacked", "raised"]
    E = 5
    inp = inputs(E, 31)
    inp["seeds"][:, :, :2] = (FEET + [0.12, 0, 0])[None, :, :2] + np.random.default_rng(2).uniform(-0.02, 0.02, (E, 4, 2))
    inp["hips"] = inp["seeds"] + [-0.12, 0.0, 0.30]
    pr, more = world[0]["stacked"]["prims"], world[0]["raised"]["prims"]
    differs = False
    for e in range(E):
        sx, sy = inp["seeds"][e, 0, :2]
        assert sum(np.hypot(q["cx"] - sx, q["cy"] - sy) < 0.26 for q in pr) > 128
        kw = dict(has_ground=True, ground_z=world[0]["stacked"]["ground_z"])
        alone = terrain_oracle.patches(pr, inp["seeds"][e], np.full(4, inp["yaws"][e]), 13, 7, 0.04, 0.04, 10.0, **kw)
        union = terrain_oracle.patches(pr + more, inp["seeds"][e], np.full(4, inp["yaws"][e]), 13, 7, 0.04, 0.04, 10.0,
                                       **kw)
        differs = differs or not np.array_equal(alone[..., 2], union[..., 2])
    assert differs, "walking scene 2's primitives too must change a ray's height"
    tset = make_set(world, names)
    for ids in ([1] * E, [1, 2, 1, 0, 2]):
        want = expected(lib, world, names_of(names, ids), params, inp, 13, 7)
        same(scenes_call(lib, tset, ids, params, inp, 13, 7), want, f"slices {ids}")
    tset.close()


def test_single_scene_equals_the_shared_scene_call(lib, world, params):
    E = 67
    inp = inputs(E, 167)
    want = batch_call(lib, world[1]("stones"), params, inp, 13, 7)
    tset = make_set(world, ["stones"])
    same(scenes_call(lib, tset, [0] * E, params, inp, 13, 7), want, "S = 1")
    assert want["valid"].any() and np.isfinite(want["scores"]).any()
    tset.close()


@pytest.mark.parametrize("rows,cols", [(1, 1), (16, 20)])
def test_patch_shapes(lib, world, params, rows, cols):
    names = ["stones", "hfield"]
    ids = [1, 0, 0, 1, 0]
    inp = inputs(5, 7 * rows + cols)
    want = expected(lib, world, names_of(names, ids), params, inp, rows, cols)
    tset = make_set(world, names)
    same(scenes_call(lib, tset, ids, params, inp, rows, cols), want, f"{rows}x{cols}")
    tset.close()


def test_bad_indices_run_on_the_empty_scene(lib, world, params):
    names = ["stones", "hfield", "stacked"]
    ids = [2, -1, len(names), 0, 2 ** 31 - 1]
    inp = inputs(5, 77)
    per_env = names_of(names, ids)
    assert per_env == ["stacked", "empty", "empty", "stones", "empty"]
    want = expected(lib, world, per_env, params, inp, 13, 7)
    assert np.isnan(want["heightmaps"][[1, 2, 4], ..., 2]).all() and not want["valid"][[1, 2, 4]].any()
    tset = make_set(world, names)
    same(scenes_call(lib, tset, ids, params, inp, 13, 7), want, "bad indices")
    tset.close()


@pytest.mark.parametrize("use", [(), ALL])
def test_optional_inputs(lib, world, params, use):
    names = ["stones", "hfield2"]
    ids = [0, 1, 1, 0, 1]
    inp = inputs(5, 41)
    inp["vel"][1] = [-0.3, 0.0, 0.0]
    inp["contact"][3] = 1.0
    want = expected(lib, world, names_of(names, ids), params, inp, 13, 7, use=use)
    tset = make_set(world, names)
    same(scenes_call(lib, tset, ids, params, inp, 13, 7, use=use), want, str(use))
    tset.close()


def test_stream_order(lib, world, params):
    """Two calls on one non-default stream, the ids rewritten between them by a torch operation on that stream, nothing
    synchronised until the end: the second call follows the new ids."""
    names = ["stones", "hfield", "ground"]
    first, second = [0, 1, 2, 0, 1], [2, 2, 0, 1, 7]
    E = len(first)
    inp = inputs(E, 91)
    want = [expected(lib, world, names_of(names, ids), params, inp, 13, 7) for ids in (first, second)]
    assert want[0]["heightmaps"].tobytes() != want[1]["heightmaps"].tobytes()
    tset = make_set(world, names)
    d = {k: cuda(v) for k, v in inp.items()}
    ids = torch.tensor(first, dtype=torch.int32, device="cuda")
    new = torch.tensor(second, dtype=torch.int32, device="cuda")
    done = torch.tensor([True] * E, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(side):
        for k in range(2):
            got.append(lib.tamols_batch_device(d["seeds"], d["hips"], params, terrain=tset, yaws=d["yaws"],
                                               scene_ids=ids, forward_vel=d["vel"], base_pos=d["base"],
                                               contact=d["contact"], feet=d["feet"], want_seed_heights=True,
                                               want_scores=True, want_heightmaps=True, stream=side))
            if k == 0:
                ids.copy_(torch.where(done, new, ids))  # as a reset does, in stream order (no host round trip)
    side.synchronize()
    for k in range(2):
        same({n: v.cpu().numpy() for n, v in got[k].items()}, want[k], f"call {k}")
    tset.close()


# ------------------------------------------------------------------ the gate
def gated_call(lib, terrain, p, d, stc_t, vfa_t, rows, cols, scene_ids=None):
    """vfa_step_device with every optional output prefilled with the sentinel; `terrain` a GpuTerrain or, with
    scene_ids, a set."""
    E = d["seeds"].shape[0]
    out = dict(seed_heights=torch.full((E, 4), SENT, dtype=torch.float64, device="cuda"),
               scores=torch.full((E, 4, rows * cols), SENT, dtype=torch.float64, device="cuda"),
               heightmaps=torch.full((E, 4, rows, cols, 3), SENT, dtype=torch.float64, device="cuda"))
    ref = torch.full((E, 24), SENT, dtype=torch.float64, device="cuda")
    kw = {} if scene_ids is None else dict(scene_ids=scene_ids)
    got = lib.vfa_step_device(vfa_t, stc_t, d["seeds"], d["hips"], p, d["contact"], apex_interval=INTERVAL,
                              forward_vel=d["vel"], base_pos=d["base"], feet=d["feet"], ref=ref, out=out,
                              terrain=terrain, yaws=d["yaws"], rows=rows, cols=cols, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in got.items()}
    res["ref"] = ref.cpu().numpy()
    res["state"] = vfa_t.cpu().numpy().copy()
    return res


def test_gate(lib, world, params):
    """SEARCH, HOLD and PASS environments on three scenes, two control steps in a row (the searching environments hold
    in the second), against vfa_step_device per scene: outputs, mode and the srbd_vfa structs.  A HOLD and a PASS
    environment carry an index outside the set and match all the same: they read neither the index nor the set."""
    names = ["stones", "hfield", "stacked"]
    E, rows, cols = 8, 13, 7
    ids = [1, 99, 0, 2, 2, 0, -1, 1]  # gate_state's plan: e % 4 = 0 searches, 1 holds, 2 and 3 pass
    inp = inputs(E, 611)
    stc, vfa, inp["contact"] = gate_state(lib, E, inp, 612)
    d = {k: cuda(v) for k, v in inp.items()}
    stc_t = struct_tensor(stc, lib.STC_BYTES)
    per_env = np.array([names[i] if 0 <= i < len(names) else names[0] for i in ids])  # any scene: they do not search
    # expected: per scene, its own copy of the state through both steps
    want = [None, None]
    for name in sorted(set(per_env)):
        state = struct_tensor(vfa, lib.VFA_BYTES)
        for k in range(2):
            got = gated_call(lib, world[1](name), params, d, stc_t, state, rows, cols)
            if want[k] is None:
                want[k] = {n: np.zeros_like(v) for n, v in got.items()}
            for n, v in got.items():
                want[k][n][per_env == name] = v[per_env == name]
    m0, m1 = want[0]["mode"], want[1]["mode"]
    assert set(m0.tolist()) == {lib.VFA_SEARCH, lib.VFA_HOLD, lib.VFA_PASS}
    assert m0[1] == lib.VFA_HOLD and m0[6] == lib.VFA_PASS and (m1[m0 == lib.VFA_SEARCH] == lib.VFA_HOLD).all()
    tset = make_set(world, names)
    state = struct_tensor(vfa, lib.VFA_BYTES)
    ids_t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    for k in range(2):
        got = gated_call(lib, tset, params, d, stc_t, state, rows, cols, scene_ids=ids_t)
        for n, w in want[k].items():
            same_bits(got[n], w, f"step {k}: {n}")
        for n in ("seed_heights", "scores", "heightmaps"):
            assert (got[n][[1, 6]] == SENT).all(), n
            assert k == 1 or not (got[n][m0 == lib.VFA_SEARCH] == SENT).any(), n
    assert stc_t.cpu().numpy().tobytes() == bytes(stc)
    tset.close()
