"""The TAMOLS kernels against the reference's own scores (tests/golden/tamols_ref_*.npz, recorded from the reference's
``VisualFootholdAdaptation.compute_adaptation(strategy='tamols')`` by oracle/record_tamols_reference.py).

Every recorded case runs through every entry point: ``TamolsSearch.run`` (the caller's patch, scan path),
``TamolsSearch.run_terrain`` with the lattice bracket and with SRBD_TAMOLS_LATTICE=0 (every point scanned), and
``_lib.tamols_batch_device`` in its patch and terrain forms with the case at environments 0 and 2 of 3 beside a
different environment.  The cases cover the patch shapes at which the kernels change path (1x1, 1x7, 13x1, 3x5, 13x7,
16x16, 16x20), three robots' reach bounds, non-zero nominal-kinematic weights and every branch of the cost; the
recorder asserted that, and that every winner leads by more than 1e-6 and no nearest-neighbour query is a tie, so an
argmin or inf / NaN mismatch is an error and not rounding.

Tolerances are test_gpu_tamols.py's: finite scores atol 1e-9 (the closed-form plane fit against SVD lstsq), footholds
and boxes atol 1e-12; inf and NaN positions, validity and the raycast patches are exact.  Each run prints its largest
finite-score difference (pytest -s shows it).
"""
import numpy as np
import pytest
import torch

from tamols_ref import TAMOLS_REF_CASES, tamols_ref_case

pytestmark = pytest.mark.gpu
ATOL_SCORE, ATOL_POS = 1e-9, 1e-12


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


@pytest.fixture(scope="module")
def search(lib):
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import TamolsSearch

    s = TamolsSearch(0)
    yield s
    s.close()


@pytest.fixture
def case(request, lib):
    """(recorded case, its TamolsParams, its scene on the device)."""
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import tamols_params_struct

    c = tamols_ref_case(request.param)
    ter = GpuTerrain(**c["scene"])
    yield c, tamols_params_struct(c["params"], c["robot"]), ter
    ter.close()


def against_the_reference(got, c, what, heightmaps=False):
    ref = c["scores"]
    scores = np.asarray(got["scores"]).reshape(ref.shape)
    fin = np.isfinite(ref)
    diff = float(np.max(np.abs(scores[fin] - ref[fin]))) if fin.any() else 0.0
    print(f"\n{what} {c['name']}: largest finite-score difference {diff:.3e} over {int(fin.sum())} scores")
    np.testing.assert_array_equal(np.isposinf(scores), np.isposinf(ref), err_msg=f"{what}: inf positions")
    np.testing.assert_array_equal(np.isnan(scores), np.isnan(ref), err_msg=f"{what}: NaN positions")
    assert not np.isneginf(scores).any()
    np.testing.assert_allclose(scores[fin], ref[fin], rtol=0, atol=ATOL_SCORE, err_msg=f"{what}: scores")
    valid = c["valid"]
    np.testing.assert_array_equal(np.asarray(got["valid"]).astype(bool), valid, err_msg=f"{what}: valid")
    np.testing.assert_allclose(got["footholds"], c["footholds"], rtol=0, atol=ATOL_POS, err_msg=f"{what}: footholds")
    np.testing.assert_allclose(got["boxes"][valid], c["boxes"][valid], rtol=0, atol=ATOL_POS, err_msg=f"{what}: boxes")
    if heightmaps:
        np.testing.assert_array_equal(got["heightmaps"], c["patches"], err_msg=f"{what}: raycast patches")


def optional(c):
    return dict(forward_vel=c["vel"], base_position=c["base"],
                current_contact=None if c["contact"] is None else c["contact"].astype(np.int32),
                current_feet_pos=c["feet"])


@pytest.mark.parametrize("case", TAMOLS_REF_CASES, indirect=True)
def test_run_on_the_recorded_patch(search, case):
    c, p, _ = case
    got = search.run(c["patches"], c["seeds"], c["hips"], p, **optional(c))
    against_the_reference(got, c, "run")


@pytest.mark.parametrize("lattice", ["1", "0"])
@pytest.mark.parametrize("case", TAMOLS_REF_CASES, indirect=True)
def test_run_terrain(monkeypatch, search, case, lattice):
    c, p, ter = case
    monkeypatch.setenv("SRBD_TAMOLS_LATTICE", lattice)
    got = search.run_terrain(ter, c["yaw"], c["seeds"], c["hips"], p, rows=c["rows"], cols=c["cols"],
                             dist_x=c["dist_x"], dist_y=c["dist_y"], ray_z=c["ray_z"], **optional(c))
    against_the_reference(got, c, f"run_terrain lattice={lattice}", heightmaps=True)


def cuda(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def batch_of_three(c):
    """The case at environments 0 and 2; environment 1 is a different problem over the same scene (other seeds, hips,
    yaw, velocity, base, contact, feet and patches), so a wrong per-environment stride reads or writes its data."""
    def three(a, other):
        return None if a is None else np.stack([a, other(np.asarray(a, dtype=np.float64)), a])

    shift = np.array([0.07, -0.03, 0.0])
    return dict(
        seeds=three(c["seeds"], lambda a: a + shift), hips=three(c["hips"], lambda a: a + shift + [0.01, 0.02, 0.015]),
        yaws=np.array([c["yaw"], c["yaw"] + 0.4, c["yaw"]]),
        vel=three(c["vel"], lambda a: 0.5 * a + [0.05, -0.02, 0.0]), base=three(c["base"], lambda a: a + shift),
        contact=three(c["contact"], lambda a: 1.0 - a), feet=three(c["feet"], lambda a: a + shift[::-1]),
        patches=three(c["patches"], lambda a: a + [0.013, -0.007, 0.004]))


@pytest.mark.parametrize("form", ["patch", "terrain"])
@pytest.mark.parametrize("case", TAMOLS_REF_CASES, indirect=True)
def test_batch_device(lib, case, form):
    c, p, ter = case
    b = batch_of_three(c)
    if form == "patch":
        how = dict(heightmaps=cuda(b["patches"]))
    else:
        how = dict(terrain=ter, yaws=cuda(b["yaws"]), rows=c["rows"], cols=c["cols"], dist_x=c["dist_x"],
                   dist_y=c["dist_y"], ray_z=c["ray_z"], want_heightmaps=True)
    out = lib.tamols_batch_device(cuda(b["seeds"]), cuda(b["hips"]), p, forward_vel=cuda(b["vel"]),
                                  base_pos=cuda(b["base"]), contact=cuda(b["contact"], np.float32),
                                  feet=cuda(b["feet"]), want_scores=True, **how)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for e in (0, 2):
        against_the_reference({k: v[e] for k, v in out.items()}, c, f"batch {form} form, environment {e}",
                              heightmaps=form == "terrain")
