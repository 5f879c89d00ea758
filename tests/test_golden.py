"""Golden fixtures (tests/golden/*.npz, made by tests/golden/make_golden.py) on CPU.

* the numpy oracle reproduces every fixture bit for bit (guards the oracle against drift),
* the C oracle reproduces the costs (same f32 evaluation order; a few ulp at most),
* the product's host merge (srbd_make_record_host + srbd_finish_host) fed with the fixture's
  costs reproduces the fixture's step outputs,
* the product's prepare_state_and_reference and PeriodicGaitGenerator reproduce theirs,
* the TAMOLS oracle reproduces its fixture.
"""
import glob
import os

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle.srbd_ga_oracle import GaitAdaptiveOracle
from oracle.srbd_oracle import SamplingMPCOracle
from oracle.tamols_oracle import TamolsOracle
from quadruped_pympc_amd import _lib
from quadruped_pympc_amd.config import HIP_HEIGHTS, simulation_params
from quadruped_pympc_amd.helpers.periodic_gait_generator import PeriodicGaitGenerator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SRBD = sorted(glob.glob(os.path.join(GOLDEN, "srbd_c*.npz")))  # the oracle's; srbd_ref_*.npz are the reference's
GA = sorted(glob.glob(os.path.join(GOLDEN, "ga_*.npz")))
f32 = np.float32
METHODS = {"random_sampling": 0, "mppi": 1, "cem_mppi": 2}
PARS = {"zero_order": 0, "linear_spline": 1, "cubic_spline": 2}


def load(path):
    return dict(np.load(path, allow_pickle=False))


def oracle_for(g):
    o = SamplingMPCOracle(mass=float(g["mass"]), inertia=g["inertia"], horizon=int(g["horizon"]),
                          num_samples=int(g["num_samples"]), method=str(g["method"]),
                          parametrization=str(g["parametrization"]), num_splines=int(g["num_splines"]))
    o.robot.dts = g["dts"]
    return o


def test_fixtures_present():
    assert len(SRBD) >= 5
    assert len(GA) >= 2


@pytest.mark.parametrize("path", GA, ids=os.path.basename)
def test_ga_oracle_reproduces_fixture(path):
    g = load(path)
    o = GaitAdaptiveOracle(pgg_dt=float(g["pgg_dt"]), mass=float(g["mass"]), inertia=g["inertia"],
                           horizon=int(g["horizon"]), num_samples=int(g["num_samples"]), method=str(g["method"]),
                           parametrization=str(g["parametrization"]), num_splines=int(g["num_splines"]))
    out = o.compute_control_ga(g["state"], g["ref"], g["contact"], g["best_in"], g["noise"], g["freqs"],
                               g["timing"])
    for k in ("costs", "best", "grf", "pred"):
        np.testing.assert_array_equal(out[k], g[k])
    assert out["best_index"] == int(g["best_index"]) and out["best_freq"] == g["best_freq"]


@pytest.mark.parametrize("path", SRBD, ids=os.path.basename)
def test_numpy_oracle_reproduces_fixture(path):
    g = load(path)
    o = oracle_for(g)
    out = o.compute_control(g["state"], g["ref"], g["contact"], g["best_in"], g["noise"])
    np.testing.assert_array_equal(out["costs"], g["costs"])
    np.testing.assert_array_equal(out["best"], g["best"])
    np.testing.assert_array_equal(out["grf"], g["grf"])
    np.testing.assert_array_equal(out["pred"], g["pred"])
    assert out["best_index"] == int(g["best_index"])
    if g["sigma"].size:
        np.testing.assert_array_equal(out["sigma"], g["sigma"])


@pytest.mark.parametrize("path", SRBD, ids=os.path.basename)
def test_c_oracle_reproduces_fixture_costs(path):
    g = load(path)
    H = int(g["horizon"])
    cfg = co.make_cfg(N=int(g["num_samples"]), H=H, method=METHODS[str(g["method"])],
                      param_kind=PARS[str(g["parametrization"])], mass=float(g["mass"]), inertia=g["inertia"],
                      dts=g["dts"])
    c = co.rollout_costs(cfg, g["state"], g["ref"], g["contact"], g["best_in"], g["noise"])
    c = np.where(np.isfinite(c), c, f32(1e6))
    np.testing.assert_allclose(c, g["costs"], rtol=2e-6, atol=1e-4)


@pytest.mark.parametrize("path", SRBD, ids=os.path.basename)
def test_host_merge_reproduces_fixture(path):
    g = load(path)
    N, H = int(g["num_samples"]), int(g["horizon"])
    cfg = _lib.make_config(num_samples=N, horizon=H, method=str(g["method"]),
                           parametrization=str(g["parametrization"]), mass=float(g["mass"]), inertia=g["inertia"],
                           dts=g["dts"])
    world = 2
    spans = [_lib.shard_rows(N, r, world) for r in range(world)]
    recs = [_lib.make_record_host(cfg, r, world, g["costs"][a:a + n], g["noise"][a:a + n])
            for r, (a, n) in enumerate(spans)]
    sigma = g["sigma_in"] if g["sigma_in"].size else None
    best, ns, res = _lib.finish_host(cfg, np.concatenate(recs), g["state"], g["contact"], g["best_in"], sigma)
    assert res.best_index == int(g["best_index"])
    np.testing.assert_allclose(best, g["best"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(np.array(res.grf), g["grf"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(np.array(res.predicted_state), g["pred"], rtol=1e-5, atol=1e-5)
    if sigma is not None:
        np.testing.assert_allclose(ns, g["sigma"], rtol=1e-5, atol=1e-6)


def test_prepare_state_fixture():
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip import Sampling_MPC
    from test_host_logic import cfg_module

    g = load(os.path.join(GOLDEN, "prepare_state.npz"))
    m = Sampling_MPC(cfg_module(sampling_method="mppi", control_parametrization="zero_order"))
    sk = ("position", "linear_velocity", "orientation", "angular_velocity", "foot_FL", "foot_FR", "foot_RL", "foot_RR")
    rk = ("ref_position", "ref_linear_velocity", "ref_orientation", "ref_angular_velocity", "ref_foot_FL",
          "ref_foot_FR", "ref_foot_RL", "ref_foot_RR")
    for i in range(g["state_in"].shape[0]):
        sc = {k: g["state_in"][i, 3 * j:3 * j + 3] for j, k in enumerate(sk)}
        rs = {k: g["ref_in"][i, 3 * j:3 * j + 3].reshape((1, 3) if "foot" in k else (3,)) for j, k in enumerate(rk)}
        m.best_control_parameters = g["best_in"][i].copy()
        s, r = m.prepare_state_and_reference(sc, rs, g["current_contact"][i], g["previous_contact"][i])
        np.testing.assert_array_equal(s, g["state"][i])
        np.testing.assert_array_equal(r, g["ref"][i])
        np.testing.assert_array_equal(m.best_control_parameters, g["best"][i])


def test_pgg_fixture():
    g = load(os.path.join(GOLDEN, "pgg_sequences.npz"))
    for gait in (0, 1, 2, 5):
        duty, freq = g[f"gait{gait}_params"]
        pgg = PeriodicGaitGenerator(duty, freq, gait, 12)
        for k in range(g[f"gait{gait}"].shape[0]):
            for _ in range(5):
                pgg.run(0.002, freq)
            np.testing.assert_array_equal(pgg.compute_contact_sequence([0.01, 0.02], [2, 12]), g[f"gait{gait}"][k])


def test_tamols_oracle_fixture():
    g = load(os.path.join(GOLDEN, "tamols_go2.npz"))
    params = dict(simulation_params["tamols_params"])
    params["h_des"] = HIP_HEIGHTS["go2"]
    orc = TamolsOracle(params, "go2")
    for name in ("flat", "stepping_stones_medium"):
        fh, boxes, valid, scores = orc.compute(g[f"{name}_heightmaps"], g[f"{name}_seeds"], g[f"{name}_hips"],
                                               g[f"{name}_vel"], g[f"{name}_base"], g[f"{name}_contact"],
                                               g[f"{name}_feet"])
        np.testing.assert_array_equal(fh, g[f"{name}_footholds"])
        np.testing.assert_array_equal(valid, g[f"{name}_valid"])
        np.testing.assert_array_equal(scores, g[f"{name}_scores"])
    assert np.isfinite(g["stepping_stones_medium_scores"]).any() and np.isinf(g["stepping_stones_medium_scores"]).any()
