"""Gait-adaptive sampling and the opt-in cost terms in a batch (srbd_batch_set_gait, srbd_batch_clear_gait,
srbd_batch_set_cost_terms): environment e of a batch step against a plain ``Context`` that received ``set_gait`` /
``set_cost_terms`` with environment e's values and was stepped with environment e's inputs (bit for bit), and against
the CPU oracles with injected noise (the tolerances and the near-tie rule of tests/test_gpu_ga.py and
tests/test_gpu_cost_terms.py, restated).  Expected values never come from the batch itself."""
import numpy as np
import pytest

from helpers import f32, make_case, product_cfg
from oracle.srbd_ga_oracle import GA_DUTY, GaitAdaptiveOracle, freq_set

pytestmark = pytest.mark.gpu

COST_RTOL, COST_ATOL = 2e-5, 1e-3
AVAIL = (1.4, 2.0, 2.4)
TIMINGS = [(0.1, 0.6, 0.6, 0.1), (0.0, 0.5, 0.5, 0.0), (0.64, 0.99, 1.0, 0.3)]  # tests/test_gpu_ga.py
TERMS = {"r_force": (0.1, 0.1, 0.001), "w_smooth": 0.01, "w_cone": 5.0}  # tests/test_gpu_cost_terms.py
PGG_DT = 0.02


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def env_cases(E, wkey="c2", **kw):
    """Environment e's case: its own state, reference, contact phase, warm start and noise."""
    return [make_case(wkey, seed=e, k=e, **kw) for e in range(E)]


def stack(cases, key):
    return np.stack([c[key] for c in cases])


def result_dict(best, res, costs):
    return dict(best=np.array(best, f32), grf=np.array(res.grf, f32), pred=np.array(res.predicted_state, f32),
                best_cost=f32(res.best_cost), best_index=int(res.best_index), best_freq=f32(res.best_freq),
                costs=costs)


def assert_same(got, want, what=""):
    for k in ("best", "grf", "pred", "costs"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    assert got["best_cost"].tobytes() == want["best_cost"].tobytes(), what
    assert got["best_index"] == want["best_index"], what
    assert got["best_freq"].tobytes() == want["best_freq"].tobytes(), what


def timings_of(E):
    return np.array([TIMINGS[e % len(TIMINGS)] for e in range(E)], f32)


def default_keys(E):
    return [100 + e for e in range(E)], [7 + 2 * e for e in range(E)]


def single_steps(lib, cases, seeds, counters, *, gait=None, terms=None, rng=None, noise=False, bests=None, ctxs=None):
    """The expected values: a plain Context of the cases' configuration, given environment e's setting and stepped
    with environment e's inputs.  gait: (timings (E, 4), freq_sets (E, n), freq_rows (E, N) or None) or None."""
    own = ctxs is None
    ctx = None
    if own:
        ctx = lib.Context(product_cfg(cases[0]))
        if rng:
            ctx.set_rng(rng)
    try:
        out = []
        for e, c in enumerate(cases):
            x = ctx if own else ctxs[e]
            if terms is not None:
                x.set_cost_terms(terms["r_force"], terms["w_smooth"], terms["w_cone"])
            if gait is not None:
                t, fs, rows = gait
                x.set_gait(t[e], PGG_DT, GA_DUTY, fs[e], None if rows is None else rows[e])
            best, _, res, costs = x.step(c["state"], c["ref"], c["contact"], c["best"] if bests is None else bests[e],
                                         noise=c["noise"] if noise else None, seed=int(seeds[e]),
                                         counter=int(counters[e]), want_costs=True)
            out.append(result_dict(best, res, costs))
    finally:
        if own:
            ctx.close()
    return out


def batch_step(b, cases, seeds, counters, noise=False, bests=None):
    best, results, costs = b.step(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                  stack(cases, "best") if bests is None else bests,
                                  noise=stack(cases, "noise") if noise else None, seeds=seeds, counters=counters,
                                  want_costs=True)
    return [result_dict(best[e], results[e], costs[e]) for e in range(len(cases))]


def sets_of(cases, E):
    """Every environment's candidate set as the controller forms it (oracle freq_set), nominal 1.65."""
    method = cases[0]["orc"].method  # the oracle's method code
    return np.stack([freq_set(method, AVAIL, 1.65, 1) for _ in range(E)]).astype(f32)


def run_ga(lib, cases, *, rng=None, seeds=None, counters=None, injected=False, fs=None):
    """One gait-adaptive batch step against E gait-adaptive single steps; returns the batch's results."""
    E = len(cases)
    s0, c0 = default_keys(E)
    seeds = s0 if seeds is None else seeds
    counters = c0 if counters is None else counters
    t = timings_of(E)
    fs = sets_of(cases, E) if fs is None else fs
    rows = None
    if injected:
        N = cases[0]["w"].num_samples
        rows = np.stack([np.random.default_rng(50 + e).choice(fs[e], N) for e in range(E)]).astype(f32)
    want = single_steps(lib, cases, seeds, counters, gait=(t, fs, rows), rng=rng, noise=injected)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        if rng:
            b.set_rng(rng)
        b.set_gait(t, PGG_DT, GA_DUTY, fs, rows)
        got = batch_step(b, cases, seeds, counters, noise=injected)
    finally:
        b.close()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
        assert got[e]["best_freq"] in fs[e]
    return got


# the smallest shape that still exercises the part named beside it
GA_SHAPES = [
    ("zo_h12_n257_mppi", dict(N=257, method="mppi", par="zero_order", H=12)),  # one level above the leaves
    ("zo_h12_n257_rs", dict(N=257, method="random_sampling", par="zero_order", H=12)),  # the key reduction
    ("zo_h16_n130", dict(N=130, method="mppi", par="zero_order", H=16)),
    ("zo_h10_n257_rs", dict(N=257, method="random_sampling", par="zero_order", H=10)),
    ("lin_s2_h12_n300", dict(N=300, method="mppi", par="linear_spline", H=12, S=2)),  # per-leg spline coefficients
    ("cub_s2_h16_n300", dict(N=300, method="mppi", par="cubic_spline", H=16, S=2)),
    ("zo_h8_n130", dict(N=130, method="mppi", par="zero_order", H=8)),  # the generic, non-specialised form
    ("zo_h12_n1", dict(N=1, method="mppi", par="zero_order", H=12)),    # a single row
    ("zo_h12_n65", dict(N=65, method="mppi", par="zero_order", H=12)),  # a second leaf of one row
]
COST_SHAPES = [
    ("zo_h12_n257_mppi", dict(N=257, method="mppi", par="zero_order", H=12)),  # the rolling prefetch window
    ("zo_h12_n257_rs", dict(N=257, method="random_sampling", par="zero_order", H=12)),
    ("zo_h16_n130", dict(N=130, method="mppi", par="zero_order", H=16)),
    ("lin_s2_h12_n300", dict(N=300, method="mppi", par="linear_spline", H=12, S=2)),
    ("cub_s2_h16_n300", dict(N=300, method="mppi", par="cubic_spline", H=16, S=2)),
    ("zo_h8_n130", dict(N=130, method="mppi", par="zero_order", H=8)),  # the generic form
    ("zo_h12_n1", dict(N=1, method="mppi", par="zero_order", H=12)),
]


# ------------------------------------------------------------------ gait-adaptive sampling
@pytest.mark.parametrize("name,kw", GA_SHAPES, ids=[s[0] for s in GA_SHAPES])
def test_ga_bit_equal_device_draws(lib, name, kw):
    """Device-drawn frequencies, Philox: keyed by environment e's seed and counter."""
    got = run_ga(lib, env_cases(3, **kw))
    if kw["N"] >= 130:  # the environments drew different rows
        assert not np.array_equal(got[0]["costs"], got[1]["costs"])


@pytest.mark.parametrize("name,kw", GA_SHAPES[:2], ids=[s[0] for s in GA_SHAPES[:2]])
def test_ga_bit_equal_jax_stream(lib, name, kw):
    """Device-drawn frequencies with rng='jax': jax.random.choice on environment e's key."""
    E = 3
    seeds = [lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)]
    run_ga(lib, env_cases(E, **kw), rng="jax", seeds=seeds)


@pytest.mark.parametrize("name,kw", GA_SHAPES[:2] + GA_SHAPES[4:5], ids=[s[0] for s in GA_SHAPES[:2] + GA_SHAPES[4:5]])
def test_ga_bit_equal_injected_rows(lib, name, kw):
    """Injected per-row frequencies (environment e's rows at e x ldn) with injected noise."""
    run_ga(lib, env_cases(3, **kw), injected=True)


def test_ga_per_environment_frequency_sets(lib):
    """Random sampling: environment 1 gets a one-value set (optimize_swing false: n x nominal) and its best_freq is
    that value; environments 0 and 2 are what they are when environment 1 has the full set."""
    E = 3
    cases = env_cases(E, N=257, method="random_sampling", par="zero_order", H=12)
    full = sets_of(cases, E)
    assert len(set(full[1].tolist())) == len(AVAIL)
    one = full.copy()
    one[1] = freq_set(cases[1]["orc"].method, AVAIL, 1.65, 0)
    assert set(one[1].tolist()) == {f32(1.65)}
    got_full = run_ga(lib, cases, fs=full)
    got_one = run_ga(lib, cases, fs=one)
    assert got_one[1]["best_freq"].tobytes() == f32(1.65).tobytes()
    for e in (0, 2):
        assert_same(got_one[e], got_full[e], f"env {e}")
    assert not np.array_equal(got_one[1]["costs"], got_full[1]["costs"])


def test_ga_oracle_parity(lib):
    """Injected noise and frequencies against oracle.srbd_ga_oracle: per-sample costs to tolerance; the oracle's
    reduction fed with the GPU's costs reproduces the step; best_freq is the best row's injected frequency."""
    E = 3
    cases = env_cases(E, N=300, method="mppi", par="zero_order", H=12)
    t, fs = timings_of(E), sets_of(cases, E)
    rows = np.stack([np.random.default_rng(e).choice(fs[e], 300) for e in range(E)]).astype(f32)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_gait(t, PGG_DT, GA_DUTY, fs, rows)
        got = batch_step(b, cases, [42] * E, [3] * E, noise=True)
    finally:
        b.close()
    for e, (case, g) in enumerate(zip(cases, got)):
        w = case["w"]
        o = GaitAdaptiveOracle(pgg_dt=PGG_DT, mass=w.mass, inertia=w.inertia, horizon=w.horizon,
                               num_samples=w.num_samples, method=w.method, parametrization=w.parametrization,
                               num_splines=w.num_splines)
        params = (case["best"][None, :] + case["noise"]).astype(f32)
        ref_costs = o.saturate(o.rollout_costs_ga(case["state"], case["ref"], params, t[e], rows[e]))
        np.testing.assert_allclose(g["costs"], ref_costs, rtol=COST_RTOL, atol=COST_ATOL)
        r = o.reduce(case["state"], case["contact"], case["best"], case["noise"], g["costs"])
        assert g["best_index"] == r["best_index"]
        np.testing.assert_allclose(g["best"], r["best"], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(g["grf"], r["grf"], rtol=1e-5, atol=1e-3)
        assert g["best_freq"] == rows[e][g["best_index"]]


def test_clear_gait_returns_to_the_plain_step(lib):
    E = 3
    seeds, counters = default_keys(E)
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    plain = single_steps(lib, cases, seeds, counters)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_gait(timings_of(E), PGG_DT, GA_DUTY, sets_of(cases, E))
        ga = batch_step(b, cases, seeds, counters)
        b.clear_gait()
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert ga[e]["best_freq"] in np.array(AVAIL, f32)
        assert not np.array_equal(ga[e]["costs"], plain[e]["costs"])
        assert_same(got[e], plain[e], f"env {e}")
        assert got[e]["best_freq"] == 0.0


def test_ga_feedback_three_steps(lib):
    """Three consecutive steps, set_gait before each with advanced leg phases and the returned best fed back,
    against three single contexts: refilling the staged inputs keeps the gait fields."""
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    seeds = [100 + e for e in range(E)]
    fs = sets_of(cases, E)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    ctxs = [lib.Context(product_cfg(cases[0])) for _ in range(E)]
    try:
        bb = stack(cases, "best")
        for it in range(3):
            t = ((timings_of(E) + f32(0.033) * it) % f32(1.0)).astype(f32)
            counters = [7 + 2 * e + it for e in range(E)]
            b.set_gait(t, PGG_DT, GA_DUTY, fs)
            got = batch_step(b, cases, seeds, counters, bests=bb)
            want = single_steps(lib, cases, seeds, counters, gait=(t, fs, None), bests=bb, ctxs=ctxs)
            for e in range(E):
                assert_same(got[e], want[e], f"step {it} env {e}")
            bb = np.stack([w["best"] for w in want])
    finally:
        b.close()
        for c in ctxs:
            c.close()


def test_ga_more_environments_than_leaves(lib):
    """E = 40 at N = 65, device draws: 80 rollout blocks, 40 merge blocks counting themselves; a second step shows the
    arrival count was reset."""
    E = 40
    cases = env_cases(E, N=65, method="mppi", par="zero_order", H=12)
    seeds, counters = default_keys(E)
    t, fs = timings_of(E), sets_of(cases, E)
    want = single_steps(lib, cases, seeds, counters, gait=(t, fs, None))
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_gait(t, PGG_DT, GA_DUTY, fs)
        first = batch_step(b, cases, seeds, counters)
        second = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(first[e], want[e], f"env {e}")
        assert_same(second[e], want[e], f"second step env {e}")


# ------------------------------------------------------------------ opt-in cost terms
def run_terms(lib, cases, terms):
    E = len(cases)
    seeds, counters = default_keys(E)
    want = single_steps(lib, cases, seeds, counters, terms=terms)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_cost_terms(terms["r_force"], terms["w_smooth"], terms["w_cone"])
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
    return got


@pytest.mark.parametrize("name,kw", COST_SHAPES, ids=[s[0] for s in COST_SHAPES])
def test_cost_terms_bit_equal(lib, name, kw):
    cases = env_cases(3, **kw)
    got = run_terms(lib, cases, TERMS)
    if kw["N"] > 1:  # the terms are in the cost
        seeds, counters = default_keys(3)
        plain = single_steps(lib, cases[:1], seeds[:1], counters[:1])[0]
        assert np.mean(got[0]["costs"] > plain["costs"]) > 0.9


def test_cost_terms_oracle_parity(lib):
    E = 3
    cases = env_cases(E, N=300, method="mppi", par="zero_order", H=12)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_cost_terms(TERMS["r_force"], TERMS["w_smooth"], TERMS["w_cone"])
        got = batch_step(b, cases, [1] * E, [2] * E, noise=True)
    finally:
        b.close()
    for case, g in zip(cases, got):
        o = case["orc"]
        params = (case["best"][None, :] + case["noise"]).astype(f32)
        ref = o.saturate(o.rollout_costs(case["state"], case["ref"], params, case["contact"], cost_terms=TERMS))
        np.testing.assert_allclose(g["costs"], ref, rtol=2e-5, atol=1e-3)
        plain = o.saturate(o.rollout_costs(case["state"], case["ref"], params, case["contact"]))
        assert np.mean(ref > plain) > 0.9


def test_zero_weights_are_the_plain_step_and_invalid_weights_change_nothing(lib):
    E = 3
    seeds, counters = default_keys(E)
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    plain = single_steps(lib, cases, seeds, counters)
    with_terms = single_steps(lib, cases, seeds, counters, terms=TERMS)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_cost_terms((0.0, 0.0, 0.0), 0.0, 0.0)
        zero = batch_step(b, cases, seeds, counters)
        b.set_cost_terms(TERMS["r_force"], TERMS["w_smooth"], TERMS["w_cone"])
        with pytest.raises(RuntimeError, match="finite"):
            b.set_cost_terms((0.1, -1.0, 0.0), 0.0, 0.0)
        with pytest.raises(RuntimeError, match="finite"):
            b.set_cost_terms((0.1, 0.1, 0.1), float("nan"), 0.0)
        with pytest.raises(RuntimeError, match="finite"):
            b.set_cost_terms((0.1, 0.1, 0.1), 0.0, float("inf"))
        kept = batch_step(b, cases, seeds, counters)
        b.set_cost_terms((0.0, 0.0, 0.0), 0.0, 0.0)
        cleared = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(zero[e], plain[e], f"zero weights env {e}")
        assert_same(kept[e], with_terms[e], f"after the refused weights env {e}")
        assert_same(cleared[e], plain[e], f"cleared env {e}")


def test_gait_adaptive_with_cost_terms_is_refused_in_either_order(lib):
    E = 3
    seeds, counters = default_keys(E)
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    t, fs = timings_of(E), sets_of(cases, E)
    with_terms = single_steps(lib, cases, seeds, counters, terms=TERMS)
    with_gait = single_steps(lib, cases, seeds, counters, gait=(t, fs, None))
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_cost_terms(TERMS["r_force"], TERMS["w_smooth"], TERMS["w_cone"])
        with pytest.raises(RuntimeError, match="no batch form"):
            b.set_gait(t, PGG_DT, GA_DUTY, fs)
        kept_terms = batch_step(b, cases, seeds, counters)
        b.set_cost_terms((0.0, 0.0, 0.0), 0.0, 0.0)
        b.set_gait(t, PGG_DT, GA_DUTY, fs)
        with pytest.raises(RuntimeError, match="no batch form"):
            b.set_cost_terms(TERMS["r_force"], TERMS["w_smooth"], TERMS["w_cone"])
        b.set_cost_terms((0.0, 0.0, 0.0), 0.0, 0.0)  # zero weights activate nothing
        kept_gait = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(kept_terms[e], with_terms[e], f"cost terms kept, env {e}")
        assert_same(kept_gait[e], with_gait[e], f"gait kept, env {e}")


# ------------------------------------------------------------------ controller class
def test_gait_adaptive_controller_class(lib):
    """The gait-adaptive Batched_Sampling_MPC at E = 2 over two with_newkey / compute_control rounds against two
    centroidal_nmpc_hip_gait_adaptive.Sampling_MPC objects given the same starting keys."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_gait_adaptive import Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_gait_adaptive_batched import \
        Batched_Sampling_MPC

    E = 2
    batched = Batched_Sampling_MPC(E)
    singles = [Sampling_MPC() for _ in range(E)]
    cases = env_cases(E, N=batched.num_parallel_computations, method=batched.sampling_method,
                      par=batched.control_parametrization, H=batched.horizon)
    nominal, swing = [1.65, 1.4], [1, 0]
    try:
        for e in range(E):
            singles[e].master_key = np.array(batched.master_keys[e])
        bb = np.array(batched.best_control_parameters)
        for it in range(2):
            t = ((timings_of(E) + f32(0.05) * it) % f32(1.0)).astype(f32)
            batched.with_newkey()
            out = batched.compute_control(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"), bb,
                                          batched.get_key(), t, nominal, swing)
            assert np.asarray(out[5]).shape == (E,)
            for e in range(E):
                s = singles[e].with_newkey()
                np.testing.assert_array_equal(batched.master_keys[e], s.master_key)
                ref = s.compute_control(cases[e]["state"], cases[e]["ref"], cases[e]["contact"], bb[e], s.get_key(),
                                        t[e], nominal[e], swing[e])
                for i in (0, 1, 2, 3):  # GRFs, footholds, predicted state, best parameters
                    np.testing.assert_array_equal(out[i][e], ref[i], err_msg=f"round {it} env {e} item {i}")
                assert f32(out[4][e]).tobytes() == f32(ref[4]).tobytes()
                assert f32(out[5][e]).tobytes() == f32(ref[5]).tobytes() and f32(ref[5]) != 0
                np.testing.assert_array_equal(np.asarray(out[6])[e], np.asarray(ref[6]))
            bb = out[3]
    finally:
        batched.close()
        for s in singles:
            s.close()
