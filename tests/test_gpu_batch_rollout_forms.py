"""Every compile-time form launch_batch_rollout, launch_batch_rollout_ga and launch_batch_pack can select
(csrc/srbd_batch.hip), each against one plain ``Context`` per environment, bit for bit: best, sigma (CEM), costs, GRFs,
predicted state, best index and best frequency.  E = 2 (the second environment's offsets), N = 160 (three leaves, the
last partly filled: the valid path and the padding rows), two differing environments (states, contact phases with a
swing leg, warm starts, seeds).  Expected values never come from the batch."""

import numpy as np
import pytest
import torch

import test_gpu_batch_cem as tcem
import test_gpu_batch_device as tdev
import test_gpu_batch_env_params as tenv
import test_gpu_batch_features as tfeat
from helpers import product_cfg

pytestmark = pytest.mark.gpu

E, N = 2, 160
# the specialised shapes of launch_batch_rollout and one generic shape per parametrization
PLAIN = [
    ("zo_h10", dict(par="zero_order", H=10)),
    ("zo_h12", dict(par="zero_order", H=12)),
    ("zo_h16", dict(par="zero_order", H=16)),
    ("zo_h7", dict(par="zero_order", H=7)),
    ("lin_s2_h12", dict(par="linear_spline", H=12, S=2)),
    ("lin_s2_h16", dict(par="linear_spline", H=16, S=2)),
    ("lin_s3_h7", dict(par="linear_spline", H=7, S=3)),
    ("cub_s2_h12", dict(par="cubic_spline", H=12, S=2)),
    ("cub_s2_h16", dict(par="cubic_spline", H=16, S=2)),
    ("cub_s3_h7", dict(par="cubic_spline", H=7, S=3)),
]
# launch_batch_rollout_ga's: it fixes the horizon alone, so the spline shapes need no S of their own
GA = PLAIN
# the shapes with a kernel of their own under per-environment parameters: the flagship's and the generic ones
ENV = [s for s in PLAIN if s[0] in ("zo_h12", "zo_h7", "lin_s3_h7", "cub_s3_h7")]
VARIANTS = ["plain", "terms", "cem", "cem_terms"]


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def run_plain(lib, kw, variant, noise, envt):
    cem, terms = variant.startswith("cem"), variant.endswith("terms")
    t = tcem if cem else tfeat
    cases = t.env_cases(E, N=N, **kw) if cem else t.env_cases(E, N=N, method="mppi", **kw)
    seeds, counters = t.default_keys(E)
    cfg = product_cfg(cases[0])
    p = tenv.env_params(lib, cases, shift=1) if envt else None  # shift 1: both environments differ from the shared robot
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(c), p[e]) if envt else product_cfg(c))
            for e, c in enumerate(cases)]
    b = (lib.CemBatchContext if cem else lib.BatchContext)(cfg, E)
    try:
        if terms:
            for x in ctxs:
                x.set_cost_terms(**tcem.TERMS)
            b.set_cost_terms(**tcem.TERMS)
        if envt:
            b.set_env_params(p)
        want = t.single_steps(lib, cases, seeds, counters, noise=noise, ctxs=ctxs)
        got = t.batch_step(b, cases, seeds, counters, noise=noise)
    finally:
        b.close()
        for x in ctxs:
            x.close()
    for e in range(E):
        t.assert_same(got[e], want[e], f"env {e}")
    assert got[0]["costs"].tobytes() != got[1]["costs"].tobytes()  # the environments do differ


@pytest.mark.parametrize("noise", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,kw", PLAIN, ids=[s[0] for s in PLAIN])
def test_plain_forms(lib, name, kw, variant, noise):
    run_plain(lib, kw, variant, noise, envt=False)


@pytest.mark.parametrize("noise", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,kw", ENV, ids=[s[0] for s in ENV])
def test_plain_forms_env_params(lib, name, kw, variant, noise):
    run_plain(lib, kw, variant, noise, envt=True)


@pytest.mark.parametrize("injected", [False, True], ids=["philox", "injected"])
@pytest.mark.parametrize("name,kw", GA, ids=[s[0] for s in GA])
def test_gait_adaptive_forms(lib, name, kw, injected):
    tfeat.run_ga(lib, tfeat.env_cases(E, N=N, method="mppi", **kw), injected=injected)


@pytest.mark.parametrize("name,kw", ENV, ids=[s[0] for s in ENV])
def test_gait_adaptive_forms_env_params(lib, name, kw):
    cases = tfeat.env_cases(E, N=N, method="mppi", **kw)
    p = tenv.env_params(lib, cases, shift=1)
    seeds, counters = tfeat.default_keys(E)
    t, fs = tfeat.timings_of(E), tfeat.sets_of(cases, E)
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(c), p[e])) for e, c in enumerate(cases)]
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        want = tfeat.single_steps(lib, cases, seeds, counters, gait=(t, fs, None), ctxs=ctxs)
        b.set_env_params(p)
        b.set_gait(t, tfeat.PGG_DT, tfeat.GA_DUTY, fs)
        got = tfeat.batch_step(b, cases, seeds, counters)
    finally:
        b.close()
        for x in ctxs:
            x.close()
    for e in range(E):
        tfeat.assert_same(got[e], want[e], f"env {e}")


@pytest.mark.parametrize("envt", [False, True], ids=["shared", "env_params"])
@pytest.mark.parametrize("cem", [False, True], ids=["mppi", "cem"])
def test_device_resident_step_pack_forms(lib, cem, envt):
    """The four pack kernels: the device-resident step's outputs are the single contexts' (through the host form of
    the same batch they would be the batch's own, so the expected values are the contexts')."""
    t = tcem if cem else tfeat
    kw = dict(par="zero_order", H=12)
    cases = t.env_cases(E, N=N, **kw) if cem else t.env_cases(E, N=N, method="mppi", **kw)
    seeds, counters = t.default_keys(E)
    p = tenv.env_params(lib, cases, shift=1) if envt else None
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(c), p[e]) if envt else product_cfg(c))
            for e, c in enumerate(cases)]
    b = (lib.CemBatchContext if cem else lib.BatchContext)(product_cfg(cases[0]), E)
    try:
        want = t.single_steps(lib, cases, seeds, counters, ctxs=ctxs)
        if envt:
            b.set_env_params(p)
        if cem:
            got = tcem.device_form(b, cases, seeds, counters, tcem.dev(tcem.stack(cases, "sigma")), 0.0,
                                   torch.cuda.Stream())
        else:
            got = tdev.device_step(b, tdev.arrays_of(cases), *tdev.default_keys(E))  # the same keys, as uint64 arrays
    finally:
        b.close()
        for x in ctxs:
            x.close()
    for e in range(E):
        w = want[e]
        for k, wk in (("best", "best"), ("grf", "grf"), ("predicted_state", "pred"), ("costs", "costs")):
            assert np.asarray(got[k][e], np.float32).tobytes() == w[wk].tobytes(), f"env {e} {k}"
        if cem:
            assert np.asarray(got["sigma"][e], np.float32).tobytes() == w["sigma"].tobytes(), f"env {e} sigma"
        assert np.float32(got["best_cost"][e]).tobytes() == w["best_cost"].tobytes(), f"env {e}"
        assert int(got["best_index"][e]) == w["best_index"] and int(got["status"][e]) == 0, f"env {e}"
