"""Batched environments on the GPU (srbd_batch_step): environment e of a batch step against a plain ``Context`` of
the same configuration stepped with environment e's inputs (bit for bit), and against the CPU oracle with injected
noise (the tolerances and the near-tie rule of the single-step parity tests).  Expected values never come from the
batch itself."""
import numpy as np
import pytest

from helpers import f32, make_case, product_cfg

pytestmark = pytest.mark.gpu

COST_RTOL, COST_ATOL = 2e-5, 1e-3


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
                best_cost=f32(res.best_cost), best_index=int(res.best_index), costs=costs)


def single_steps(lib, cases, seeds, counters, rng=None, noise=False, bests=None, ctx=None):
    """The parent's code path: one plain Context of the cases' configuration, stepped once per environment."""
    own = ctx is None
    if own:
        ctx = lib.Context(product_cfg(cases[0]))
        if rng:
            ctx.set_rng(rng)
    try:
        out = []
        for e, c in enumerate(cases):
            best, _, res, costs = ctx.step(c["state"], c["ref"], c["contact"], c["best"] if bests is None else bests[e],
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


def assert_same(got, want, what=""):
    for k in ("best", "grf", "pred", "costs"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    assert got["best_cost"].tobytes() == want["best_cost"].tobytes(), what
    assert got["best_index"] == want["best_index"], what


def run_bit_equal(lib, cases, rng=None, seeds=None, counters=None):
    E = len(cases)
    seeds = [100 + e for e in range(E)] if seeds is None else seeds
    counters = [7 + 2 * e for e in range(E)] if counters is None else counters
    want = single_steps(lib, cases, seeds, counters, rng=rng)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        if rng:
            b.set_rng(rng)
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
    return got


# the smallest shape that still exercises the part named beside it
DEVICE_DRAW_SHAPES = [
    # 34 leaves: two level-1 nodes, the second with two children; the last leaf holds one row
    ("zo_h12_n2113", 3, dict(N=2113, method="mppi", par="zero_order", H=12)),
    ("zo_h12_n1", 3, dict(N=1, method="mppi", par="zero_order", H=12)),      # a single row
    ("zo_h12_n65", 3, dict(N=65, method="mppi", par="zero_order", H=12)),    # a second leaf of one row
    ("zo_h12_n257", 3, dict(N=257, method="mppi", par="zero_order", H=12)),  # exactly one level above the leaves
    # the key reduction; H 10's specialised shape
    ("rs_h10_n257", 3, dict(wkey="c1", N=257, method="random_sampling", par="zero_order", H=10)),
    ("lin_s2_h12_n700", 3, dict(N=700, method="mppi", par="linear_spline", H=12, S=2)),  # spline decode
    ("cub_s2_h16_n700", 3, dict(N=700, method="mppi", par="cubic_spline", H=16, S=2)),   # H 16: no LDS stage
    ("zo_h8_n300", 3, dict(N=300, method="mppi", par="zero_order", H=8)),    # the generic, non-specialised shape
    ("c2_n10000_e4", 4, dict(N=10000, method="mppi", par="zero_order", H=12)),  # C2 itself: 157 leaves
]


@pytest.mark.parametrize("name,E,kw", DEVICE_DRAW_SHAPES, ids=[s[0] for s in DEVICE_DRAW_SHAPES])
def test_bit_equal_device_draws(lib, name, E, kw):
    run_bit_equal(lib, env_cases(E, **kw))


def test_device_draws_are_draw_noise_rows(lib):
    """Environment e's device draws are srbd_draw_noise(seed_e, counter_e): a batch step on those rows injected
    equals the batch step that draws on the device."""
    E, seeds, counters = 3, [100, 101, 102], [7, 9, 11]
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    ctx = lib.Context(product_cfg(cases[0]))
    try:
        rows = [ctx.draw_noise(seeds[e], counters[e]) for e in range(E)]
    finally:
        ctx.close()
    for e in range(E):
        assert not rows[e][0].any() and rows[e][1:].any()
        cases[e] = dict(cases[e], noise=rows[e])
    assert not np.array_equal(rows[0], rows[1])
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        drawn = batch_step(b, cases, seeds, counters)
        injected = batch_step(b, cases, seeds, counters, noise=True)
    finally:
        b.close()
    for e in range(E):
        assert_same(drawn[e], injected[e], f"env {e}")


@pytest.mark.parametrize("rng", ["jax", "jax_legacy"])
def test_bit_equal_jax_streams(lib, rng):
    """The per-environment key reaches the threefry path."""
    E = 3
    seeds = [lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)]
    got = run_bit_equal(lib, env_cases(E, N=257, method="mppi", par="zero_order", H=12), rng=rng, seeds=seeds)
    assert not np.array_equal(got[0]["costs"], got[1]["costs"])


# ---- oracle parity with injected noise: test_gpu_parity.py's checks, restated
def check_reduction(case, g):
    o = case["orc"]
    r = o.reduce(case["state"], case["contact"], case["best"], case["noise"], g["costs"])
    assert r["best_index"] == g["best_index"]
    np.testing.assert_allclose(g["best"], r["best"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g["grf"], r["grf"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(g["pred"], r["pred"], rtol=1e-5, atol=1e-5)


def check_end_to_end(case, g):
    ref = case["orc"].compute_control(case["state"], case["ref"], case["contact"], case["best"], case["noise"])
    np.testing.assert_allclose(g["costs"], ref["costs"], rtol=COST_RTOL, atol=COST_ATOL)
    try:
        np.testing.assert_allclose(g["grf"], ref["grf"], rtol=1e-4, atol=5e-3)
        np.testing.assert_allclose(g["best"], ref["best"], rtol=1e-4, atol=1e-3)
    except AssertionError:
        # near tie: the selection flipped on costs equal to tolerance; the GPU is then consistent with the
        # oracle's reduction applied to the GPU's own costs
        c = ref["costs"]
        assert g["costs"][g["best_index"]] <= c.min() * (1 + COST_RTOL) + COST_ATOL
        check_reduction(case, g)


@pytest.mark.parametrize("kw", [dict(N=700, method="mppi", par="zero_order", H=12),
                                dict(wkey="c3", N=700, method="random_sampling", par="cubic_spline", H=10)],
                         ids=["mppi_zo_h12", "rs_cubic_h10"])
def test_oracle_parity_injected_noise(lib, kw):
    E = 3
    cases = env_cases(E, **kw)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        got = batch_step(b, cases, [42] * E, [1] * E, noise=True)
    finally:
        b.close()
    for e in range(E):
        check_end_to_end(cases[e], got[e])
        check_reduction(cases[e], got[e])


def test_isolation(lib):
    """A NaN state and an all-swing contact sequence in environment 1 change nothing in environments 0 and 2."""
    E, seeds, counters = 3, [100, 101, 102], [7, 9, 11]
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    clean = single_steps(lib, cases, seeds, counters)
    cases[1] = dict(cases[1], state=np.full(24, np.nan, f32), contact=np.zeros_like(cases[1]["contact"]))
    poisoned = single_steps(lib, [cases[1]], seeds[1:2], counters[1:2])[0]
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    assert_same(got[0], clean[0], "env 0")
    assert_same(got[2], clean[2], "env 2")
    for k in ("best", "grf", "pred", "costs"):  # NaNs compare by bits
        assert got[1][k].tobytes() == poisoned[k].tobytes(), k
    assert got[1]["best_index"] == poisoned["best_index"]
    assert got[1]["best_cost"].tobytes() == poisoned["best_cost"].tobytes()


def test_feedback_four_steps(lib):
    """Four consecutive steps, the returned best fed back and the counters advanced by one; the last step skips a
    counter (what a draw made ahead would have predicted).  Staging reuse and the arrival count's reset."""
    E = 3
    cases = env_cases(E, N=2113, method="mppi", par="zero_order", H=12)
    seeds = [100 + e for e in range(E)]
    b = lib.BatchContext(product_cfg(cases[0]), E)
    ctxs = [lib.Context(product_cfg(cases[0])) for _ in range(E)]
    try:
        bb = stack(cases, "best")
        sb = [c["best"] for c in cases]
        for it in range(4):
            counters = [7 + 2 * e + it + (1 if it == 3 else 0) for e in range(E)]
            got = batch_step(b, cases, seeds, counters, bests=bb)
            for e in range(E):
                want = single_steps(lib, [cases[e]], [seeds[e]], [counters[e]], bests=[sb[e]], ctx=ctxs[e])[0]
                assert_same(got[e], want, f"step {it} env {e}")
                sb[e] = want["best"]
            bb = np.stack([g["best"] for g in got])
    finally:
        b.close()
        for c in ctxs:
            c.close()


def test_single_environment(lib):
    run_bit_equal(lib, env_cases(1, N=257, method="mppi", par="zero_order", H=12))


def test_more_environments_than_leaves(lib):
    """E = 40 at N = 65: 80 rollout blocks, 40 merge blocks counting themselves."""
    run_bit_equal(lib, env_cases(40, N=65, method="mppi", par="zero_order", H=12))


def test_largest_batch_allocates(lib):
    """E = 4096 at N = 64, created and destroyed: the allocation sizes are computed in 64 bits."""
    case = make_case("c2", N=64, method="mppi", par="zero_order", H=12)
    b = lib.BatchContext(product_cfg(case), 4096)
    try:
        assert lib.lib.srbd_batch_num_envs(b.h) == 4096
    finally:
        b.close()


def test_controller_class(lib):
    """Batched_Sampling_MPC at E = 2 over three with_newkey / compute_control rounds against two Sampling_MPC
    objects given the same starting keys."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip import Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC

    E = 2
    batched = Batched_Sampling_MPC(E)
    singles = [Sampling_MPC() for _ in range(E)]
    cases = env_cases(E, N=batched.num_parallel_computations, method=batched.sampling_method,
                      par=batched.control_parametrization, H=batched.horizon)
    try:
        for e in range(E):
            singles[e].master_key = np.array(batched.master_keys[e])
        bb = np.array(batched.best_control_parameters)
        for it in range(3):
            batched.with_newkey()
            out = batched.compute_control(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"), bb,
                                          batched.get_key())
            for e in range(E):
                s = singles[e].with_newkey()
                np.testing.assert_array_equal(batched.master_keys[e], s.master_key)
                ref = s.compute_control(cases[e]["state"], cases[e]["ref"], cases[e]["contact"], bb[e], s.get_key())
                for i in (0, 1, 2, 3):  # GRFs, footholds, predicted state, best parameters
                    np.testing.assert_array_equal(out[i][e], ref[i], err_msg=f"round {it} env {e} item {i}")
                assert f32(out[4][e]).tobytes() == f32(ref[4]).tobytes()
                assert out[5][e] == ref[5]
                np.testing.assert_array_equal(np.asarray(out[6])[e], np.asarray(ref[6]))
            bb = out[3]
    finally:
        batched.close()
        for s in singles:
            s.close()
