"""GPU path vs the reference's own recorded outputs (tests/golden/srbd_ref_*.npz, prepare_state_ref.npz).

The fixtures are what the reference's sampling controller returned when oracle/record_srbd_reference.py executed it
from a checkout under a numpy stand-in for jax (program logic under IEEE float32 numpy evaluation plus the exact
noise stream; not XLA's rounding or reduction order).  Nothing here reads that checkout or the oracle.

Tolerances as tests/test_gpu_parity.py: costs rtol 2e-5 atol 1e-3; GRFs rtol 1e-4 atol 5e-3; parameters rtol 1e-4
atol 1e-3; predicted state rtol 1e-5 atol 1e-4; sigma rtol 1e-4 atol 1e-5.  Saturated rows as a set, best_index and
best_freq exactly.  Every step is a single one at N <= 192.
"""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = sorted(glob.glob(os.path.join(GOLDEN, "srbd_ref_*.npz")))
BASE = [p for p in REF if "srbd_ref_ga_" not in p]
GA = [p for p in REF if "srbd_ref_ga_" in p]
f32 = np.float32
SATURATED = f32(1000000)


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def load(name_or_path):
    path = name_or_path if os.sep in name_or_path else os.path.join(GOLDEN, f"srbd_ref_{name_or_path}.npz")
    return dict(np.load(path, allow_pickle=False))


def config(lib, g, graph=True):
    return lib.make_config(num_samples=int(g["num_samples"]), horizon=int(g["horizon"]), method=str(g["method"]),
                           parametrization=str(g["parametrization"]), num_splines=int(g["num_splines"]),
                           mass=float(g["mass"]), inertia=g["inertia"], dts=g["dts"], grf_min=float(g["grf_min"]),
                           grf_max=float(g["grf_max"]), mu=float(g["mu"]), sigma_mppi=float(g["sigma_mppi"]),
                           sigma_random_sampling=tuple(g["sigma_rs"]), use_graph=graph)


def compare(g, best, ns, res, costs, what=""):
    np.testing.assert_array_equal(costs == SATURATED, g["costs"] == SATURATED, err_msg=f"{what} saturated rows")
    np.testing.assert_allclose(costs, g["costs"], rtol=2e-5, atol=1e-3, err_msg=f"{what} costs")
    assert res.best_index == int(g["best_index"]), what
    np.testing.assert_allclose(np.array(res.grf), g["grf"], rtol=1e-4, atol=5e-3, err_msg=f"{what} grf")
    np.testing.assert_allclose(best, g["best"], rtol=1e-4, atol=1e-3, err_msg=f"{what} parameters")
    np.testing.assert_allclose(np.array(res.predicted_state), g["pred"], rtol=1e-5, atol=1e-4, err_msg=f"{what} pred")
    if g["sigma"].size:
        np.testing.assert_allclose(ns, g["sigma"], rtol=1e-4, atol=1e-5, err_msg=f"{what} sigma")


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("path", BASE, ids=os.path.basename)
def test_gpu_step_matches_reference(lib, path, graph):
    g = load(path)
    ctx = lib.Context(config(lib, g, graph))
    try:
        sigma = g["sigma_in"] if g["sigma_in"].size else None
        best, ns, res, costs = ctx.step(g["state"], g["ref"], g["contact"], g["best_in"], sigma=sigma,
                                        noise=g["noise"], want_costs=True)
    finally:
        ctx.close()
    compare(g, best, ns, res, costs)


@pytest.mark.parametrize("path", GA, ids=os.path.basename)
def test_gpu_gait_adaptive_step_matches_reference(lib, path):
    g = load(path)
    ctx = lib.Context(config(lib, g))
    try:
        ctx.set_gait(g["timing"], float(g["pgg_dt"]), float(g["duty"]), g["freq_set"], g["freqs"])
        best, ns, res, costs = ctx.step(g["state"], g["ref"], g["contact"], g["best_in"], noise=g["noise"],
                                        want_costs=True)
    finally:
        ctx.close()
    compare(g, best, ns, res, costs)
    assert res.best_freq == g["best_freq"]


@pytest.mark.parametrize("name", ["c1_rs_zo_h10", "c2_mppi_zo_h12", "c3_cem_cubic_h16"])
def test_gpu_key_driven_step_matches_reference(lib, name):
    """Key -> draws -> rollout -> reduction on the device, from the reference's key alone (no injected noise)."""
    from quadruped_pympc_amd._lib import pack_key

    g = load(name)
    ctx = lib.Context(config(lib, g))
    try:
        ctx.set_rng("jax")
        sigma = g["sigma_in"] if g["sigma_in"].size else None
        best, ns, res, costs = ctx.step(g["state"], g["ref"], g["contact"], g["best_in"], sigma=sigma,
                                        seed=pack_key(g["key"]), counter=0, want_costs=True)
    finally:
        ctx.close()
    compare(g, best, ns, res, costs, what="key-driven")


def test_gpu_batch_step_matches_reference(lib):
    """E = 3 environments of srbd_batch_step, each against its own fixture (one configuration, three states)."""
    gs = [load(f"batch3_mppi_zo_h12_e{e}") for e in range(3)]
    for g in gs[1:]:
        for k in ("num_samples", "horizon", "mass", "inertia", "dts", "mu", "grf_min", "grf_max", "sigma_mppi"):
            np.testing.assert_array_equal(g[k], gs[0][k])
    b = lib.BatchContext(config(lib, gs[0]), 3)
    try:
        best, results, costs = b.step(np.stack([g["state"] for g in gs]), np.stack([g["ref"] for g in gs]),
                                      np.stack([g["contact"] for g in gs]), np.stack([g["best_in"] for g in gs]),
                                      noise=np.stack([g["noise"] for g in gs]), want_costs=True)
    finally:
        b.close()
    for e, g in enumerate(gs):
        compare(g, best[e], None, results[e], costs[e], what=f"environment {e}")


def test_gpu_prepare_state_device_matches_reference(lib):
    import torch

    g = dict(np.load(os.path.join(GOLDEN, "prepare_state_ref.npz"), allow_pickle=False))
    E = g["state_in"].shape[0]
    assert E == 16
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(state_in=g["state_in"], ref_in=g["ref_in"], cur=g["current_contact"].astype(f32),
              prev=g["previous_contact"].astype(f32), best=g["best_in"].astype(f32)).items()}
    states, refs = lib.prepare_state_device(d["state_in"], d["ref_in"], d["cur"], d["prev"],
                                            int(g["params_per_leg"]), d["best"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(states.cpu().numpy(), g["state"].astype(f32))
    np.testing.assert_array_equal(refs.cpu().numpy(), g["ref"].astype(f32))
    np.testing.assert_array_equal(d["best"].cpu().numpy(), g["best"])
