"""oracle/tamols_oracle.py against the reference's own TAMOLS foothold search.

tests/golden/tamols_ref_*.npz hold what the reference's ``VisualFootholdAdaptation.compute_adaptation
(strategy='tamols')`` computed (every candidate's score, the footholds, the boxes, validity) on the recorded inputs;
oracle/record_tamols_reference.py wrote them from a checkout of the reference and asserted the case set's branch
coverage, winner margins and absence of nearest-neighbour ties.  The oracle runs the reference's numpy operations, so
the comparison is bit for bit (inf and NaN positions included), in both nearest-neighbour modes.
"""
import numpy as np
import pytest

from oracle.tamols_oracle import DEFAULT_PARAMS, TamolsOracle
from tamols_ref import TAMOLS_REF_CASES, tamols_ref_case, tamols_ref_config

SHAPES = {(1, 1), (1, 7), (13, 1), (3, 5), (13, 7), (16, 16), (16, 20)}


def test_the_case_list_is_the_recorded_one():
    import glob
    import os

    cfg = tamols_ref_config()
    assert tuple(cfg["cases"]) == TAMOLS_REF_CASES
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    files = {os.path.basename(f)[len("tamols_ref_"):-4] for f in glob.glob(os.path.join(here, "tamols_ref_*.npz"))}
    assert files == set(TAMOLS_REF_CASES) | {"config"}
    cases = [tamols_ref_case(n) for n in TAMOLS_REF_CASES]
    assert {(c["rows"], c["cols"]) for c in cases} >= SHAPES
    assert {c["robot"] for c in cases} >= {"go2", "aliengo", "b2"}
    assert sum(c["params"]["weight_nominal_kinematic"] in (1.0, 3.0) and c["params"]["h_des"] != 0.25
               for c in cases) >= 2
    assert any(not c["valid"].any() for c in cases) and any(c["valid"].any() and not c["valid"].all() for c in cases)
    assert any(np.isnan(c["patches"][..., 2]).any() and np.isnan(c["scores"]).any() for c in cases)
    assert any(len(c["scene"]["prims"]) > 128 for c in cases)


def test_mirrored_params_equal_the_references_config():
    """``config.simulation_params['tamols_params']`` and ``config.robot`` of the mirror against the reference's
    config.py, read as data by the recorder; an entry the reference gives by name (h_des = hip_height) equals the
    mirror's variable of that name.  The oracle's defaults are the same numbers."""
    from quadruped_pympc_amd import config as mirror

    cfg = tamols_ref_config()
    ref, ours = cfg["tamols_params"], mirror.simulation_params["tamols_params"]
    assert set(ref) == set(ours)
    named = 0
    for k, v in ref.items():
        if isinstance(v, dict) and set(v) == {"name"}:
            assert ours[k] == getattr(mirror, v["name"]), k
            named += 1
        else:
            assert ours[k] == v and type(ours[k]) is type(v), k
            if k in DEFAULT_PARAMS:
                assert DEFAULT_PARAMS[k] == v, k
    assert named == 1 and ref["h_des"] == {"name": "hip_height"}
    assert cfg["robot"] == mirror.robot


@pytest.mark.parametrize("nn", ["kdtree", "first"])
@pytest.mark.parametrize("name", TAMOLS_REF_CASES)
def test_oracle_equals_the_reference(name, nn):
    c = tamols_ref_case(name)
    orc = TamolsOracle(c["params"], c["robot"], nn=nn)
    fh, boxes, valid, scores = orc.compute(c["patches"].reshape(4, c["rows"], c["cols"], 1, 3), c["seeds"], c["hips"],
                                           c["vel"], c["base"], c["contact"], c["feet"])
    np.testing.assert_array_equal(scores, c["scores"])  # inf and NaN positions included
    np.testing.assert_array_equal(valid, c["valid"])
    np.testing.assert_array_equal(fh, c["footholds"])
    np.testing.assert_array_equal(boxes[valid], c["boxes"][valid])
    assert np.isnan(boxes[~valid]).all() and np.isnan(c["boxes"][~valid]).all()


@pytest.mark.parametrize("name", TAMOLS_REF_CASES)
def test_recorded_patches_are_the_terrain_oracles(name):
    """The patch the reference was fed is oracle/terrain_oracle.patches of the recorded scene (what the GPU's terrain
    form must raycast), and every feasible leg's winner leads by more than 1e-6."""
    from oracle import terrain_oracle

    c = tamols_ref_case(name)
    sc = c["scene"]
    got = terrain_oracle.patches(sc["prims"], c["seeds"], np.full(4, c["yaw"]), c["rows"], c["cols"], c["dist_x"],
                                 c["dist_y"], c["ray_z"], has_ground=sc["has_ground"], ground_z=sc["ground_z"],
                                 hfield=sc["hfield"], miss_z=sc["miss_z"])
    np.testing.assert_array_equal(got, c["patches"])
    for leg in range(4):
        s = np.sort(c["scores"][leg][np.isfinite(c["scores"][leg])])
        assert c["valid"][leg] == (s.size > 0)
        assert s.size < 2 or s[1] - s[0] > 1e-6
