"""Batched CEM-MPPI on the GPU (srbd_batch_create_cem, srbd_batch_step_cem, srbd_batch_step_cem_device): environment e
of a batch step against a plain ``Context`` of the same configuration stepped with environment e's inputs and sigma
(bit for bit, the new sigma included), the device form against the host form (bytewise), and the CPU oracle with
injected noise (the tolerances and the near-tie rule of the single-step parity tests, sigma with the tolerances
tests/test_gpu_parity.py uses for it).  Expected values never come from the batch itself."""
import types

import numpy as np
import pytest
import torch

from helpers import f32, make_case, product_cfg

pytestmark = pytest.mark.gpu

COST_RTOL, COST_ATOL = 2e-5, 1e-3
TERMS = {"r_force": (0.1, 0.1, 0.001), "w_smooth": 0.01, "w_cone": 5.0}  # tests/test_gpu_cost_terms.py
KEYS = ("best", "sigma", "grf", "pred", "costs")


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def env_cases(E, wkey="c2", **kw):
    """Environment e's case: its own state, reference, contact phase, warm start, noise -- and its own sigma, per
    column in [0.2, 5] (the clamp's range), so a sigma read from another environment or column shows."""
    kw.setdefault("method", "cem_mppi")
    cases = [make_case(wkey, seed=e, k=e, **kw) for e in range(E)]
    for e, c in enumerate(cases):
        c["sigma"] = np.random.default_rng(1000 + e).uniform(0.2, 5.0, c["orc"].P).astype(f32)
    return cases


def stack(cases, key):
    return np.stack([c[key] for c in cases])


def default_keys(E):
    return [100 + e for e in range(E)], [7 + 2 * e for e in range(E)]


def result_dict(best, sigma, res, costs):
    return dict(best=np.array(best, f32), sigma=np.array(sigma, f32), grf=np.array(res.grf, f32),
                pred=np.array(res.predicted_state, f32), best_cost=f32(res.best_cost),
                best_index=int(res.best_index), costs=costs)


def single_steps(lib, cases, seeds, counters, rng=None, noise=False, bests=None, sigmas=None, ctxs=None, terms=None):
    """The expected values: one plain Context of the cases' configuration per call, stepped once per environment."""
    out = []
    for e, c in enumerate(cases):
        ctx = lib.Context(product_cfg(c)) if ctxs is None else ctxs[e]
        try:
            if ctxs is None and rng:
                ctx.set_rng(rng)
            if ctxs is None and terms:
                ctx.set_cost_terms(**terms)
            best, sigma, res, costs = ctx.step(c["state"], c["ref"], c["contact"],
                                               c["best"] if bests is None else bests[e],
                                               sigma=c["sigma"] if sigmas is None else sigmas[e],
                                               noise=c["noise"] if noise else None, seed=int(seeds[e]),
                                               counter=int(counters[e]), want_costs=True)
            out.append(result_dict(best, sigma, res, costs))
        finally:
            if ctxs is None:
                ctx.close()
    return out


def batch_step(b, cases, seeds, counters, noise=False, bests=None, sigmas=None):
    best, sigma, results, costs = b.step_cem(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                             stack(cases, "best") if bests is None else bests,
                                             stack(cases, "sigma") if sigmas is None else sigmas,
                                             noise=stack(cases, "noise") if noise else None, seeds=seeds,
                                             counters=counters, want_costs=True)
    return [result_dict(best[e], sigma[e], results[e], costs[e]) for e in range(len(cases))]


def assert_same(got, want, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
        assert got[k].tobytes() == want[k].tobytes(), f"{what} {k}"
    assert got["best_cost"].tobytes() == want["best_cost"].tobytes(), what
    assert got["best_index"] == want["best_index"], what


def run_bit_equal(lib, cases, rng=None, seeds=None, noise=False, terms=None):
    E = len(cases)
    s0, counters = default_keys(E)
    seeds = s0 if seeds is None else seeds
    want = single_steps(lib, cases, seeds, counters, rng=rng, noise=noise, terms=terms)
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        if rng:
            b.set_rng(rng)
        if terms:
            b.set_cost_terms(**terms)
        got = batch_step(b, cases, seeds, counters, noise=noise)
    finally:
        b.close()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
        assert np.isfinite(got[e]["sigma"]).all()
    return got


# the smallest shape that still reaches the part named beside it
SHAPES = [
    ("zo_h12_n700", 3, dict(N=700, par="zero_order", H=12)),   # the LDS-staged form: sigma from its LDS copy
    ("zo_h12_n8", 3, dict(N=8, par="zero_order", H=12)),       # fewer rows than num_elite: KEY_NONE elites
    ("zo_h12_n65", 3, dict(N=65, par="zero_order", H=12)),     # a second leaf of one row
    ("zo_h16_n300", 3, dict(N=300, par="zero_order", H=16)),   # specialised, no LDS stage: sigma at the slot load
    ("zo_h8_n300", 3, dict(N=300, par="zero_order", H=8)),     # the generic path: sigma at the read
    ("lin_s2_h12_n700", 3, dict(N=700, par="linear_spline", H=12, S=2)),
    ("lin_s2_h16_n300", 3, dict(wkey="c3", N=300, par="linear_spline", H=16, S=2)),  # the other H 16 form
    ("cub_s2_h16_n700", 3, dict(wkey="c3", N=700, par="cubic_spline", H=16, S=2)),  # C3's decode, windowed loads
    ("zo_h12_n16384_e2", 2, dict(N=16384, par="zero_order", H=12)),  # 256 records: the merge's largest top-K
]


@pytest.mark.parametrize("name,E,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_bit_equal_device_draws(lib, name, E, kw):
    got = run_bit_equal(lib, env_cases(E, **kw))
    assert not np.array_equal(got[0]["sigma"], got[1]["sigma"])


@pytest.mark.parametrize("rng", ["jax", "jax_legacy"])
def test_bit_equal_jax_streams(lib, rng):
    E = 3
    seeds = [lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)]
    run_bit_equal(lib, env_cases(E, N=257, par="zero_order", H=12), rng=rng, seeds=seeds)


def test_bit_equal_injected_noise(lib):
    """noise_scaled = 1: the rows are used as given, whatever sigma is."""
    run_bit_equal(lib, env_cases(3, N=257, par="zero_order", H=12), noise=True)


def test_bit_equal_cost_terms(lib):
    """srbd_batch_set_cost_terms on a CEM batch: the kernel's form with the opt-in terms."""
    run_bit_equal(lib, env_cases(3, wkey="c3", N=300, par="cubic_spline", H=16, S=2), terms=TERMS)


# ---- oracle parity with injected noise: test_gpu_parity.py's checks, restated with sigma
def check_reduction(case, g):
    o = case["orc"]
    r = o.reduce(case["state"], case["contact"], case["best"], case["noise"], g["costs"])
    assert r["best_index"] == g["best_index"]
    np.testing.assert_allclose(g["best"], r["best"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(g["grf"], r["grf"], rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(g["pred"], r["pred"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g["sigma"], r["sigma"], rtol=1e-5, atol=1e-5, equal_nan=True)


def check_end_to_end(case, g):
    ref = case["orc"].compute_control(case["state"], case["ref"], case["contact"], case["best"], case["noise"])
    np.testing.assert_allclose(g["costs"], ref["costs"], rtol=COST_RTOL, atol=COST_ATOL)
    try:
        np.testing.assert_allclose(g["grf"], ref["grf"], rtol=1e-4, atol=5e-3)
        np.testing.assert_allclose(g["best"], ref["best"], rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(g["sigma"], ref["sigma"], rtol=1e-4, atol=1e-5, equal_nan=True)
    except AssertionError:
        # near tie: the selection flipped on costs equal to tolerance; the GPU is then consistent with the
        # oracle's reduction applied to the GPU's own costs
        c = ref["costs"]
        assert g["costs"][g["best_index"]] <= c.min() * (1 + COST_RTOL) + COST_ATOL
        check_reduction(case, g)


@pytest.mark.parametrize("kw", [dict(N=700, par="zero_order", H=12),
                                dict(wkey="c3", N=700, par="cubic_spline", H=16, S=2)],
                         ids=["zo_h12", "cubic_h16"])
def test_oracle_parity_injected_noise(lib, kw):
    E = 3
    cases = [make_case(kw.get("wkey", "c2"), seed=e, k=e, method="cem_mppi",
                       **{k: v for k, v in kw.items() if k != "wkey"}) for e in range(E)]
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        got = batch_step(b, cases, [42] * E, [1] * E, noise=True)
    finally:
        b.close()
    for e in range(E):
        check_end_to_end(cases[e], got[e])
        check_reduction(cases[e], got[e])


# ---- the device form: the host form's bytes
DEV_FIELDS = ("best", "sigma", "grf", "predicted_state", "best_cost", "best_index", "best_freq", "status", "costs")


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:  # the keys: reinterpreted, as the library reinterprets them back
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def host_form(b, cases, seeds, counters, sigmas):
    best, sigma, res, costs = b.step_cem(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                         stack(cases, "best"), sigmas, seeds=seeds, counters=counters,
                                         want_costs=True)
    return dict(best=best, sigma=sigma, grf=np.array([r.grf[:] for r in res], f32),
                predicted_state=np.array([r.predicted_state[:] for r in res], f32),
                best_cost=np.array([r.best_cost for r in res], f32),
                best_index=np.array([r.best_index for r in res], np.int32),
                best_freq=np.array([r.best_freq for r in res], f32),
                status=np.array([r.status for r in res], np.int32), costs=costs)


def unaligned(a):
    """A contiguous device view of `a` that starts one float past a 16-byte boundary: the dword path."""
    flat = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
    v = flat[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def device_form(b, cases, seeds, counters, sigma_tensor, sigma_reset, stream):
    best = dev(stack(cases, "best"))
    with torch.cuda.stream(stream):
        out = b.step_cem_device(dev(stack(cases, "state")), dev(stack(cases, "ref")), dev(stack(cases, "contact")),
                                best, sigma_tensor, dev(np.asarray(seeds, np.uint64)),
                                dev(np.asarray(counters, np.uint64)), sigma_reset=sigma_reset, want_costs=True,
                                stream=stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["best"], got["sigma"] = best.cpu().numpy(), sigma_tensor.cpu().numpy()
    return got


@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("reset", [0.0, 3.0], ids=["read", "reset3"])
@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "dword"])
def test_device_form_equals_host_form(lib, E, reset, aligned):
    cases = env_cases(E, N=130, par="zero_order", H=12)
    seeds, counters = default_keys(E)
    given = stack(cases, "sigma")
    bh, bd = lib.CemBatchContext(product_cfg(cases[0]), E), lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        want = host_form(bh, cases, seeds, counters, np.full_like(given, reset) if reset else given)
        # with a reset the tensor is only written: what it held (another sigma) must not matter
        st = dev(given) if aligned else unaligned(given)
        got = device_form(bd, cases, seeds, counters, st, reset, torch.cuda.Stream())
        for k in DEV_FIELDS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert got[k].tobytes() == want[k].tobytes(), k
        np.testing.assert_array_equal(bd.copy_costs(), want["costs"])  # that step's costs
    finally:
        bh.close()
        bd.close()
    assert np.all(want["status"] == 0)


def test_iteration_loop(lib):
    """3 control steps x 2 sampling iterations at E = 4 on the device form: sigma reset on iteration 0, best, sigma
    and the advanced counters fed back; four plain contexts stepped the same way are the expected values."""
    E, RESET = 4, 3.0
    cases = env_cases(E, N=300, par="zero_order", H=12)
    seeds = [100 + e for e in range(E)]
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    ctxs = [lib.Context(product_cfg(cases[0])) for _ in range(E)]
    stream = torch.cuda.Stream()
    try:
        best = dev(stack(cases, "best"))
        sigma = dev(stack(cases, "sigma"))
        sb = [c["best"] for c in cases]
        ss = [c["sigma"] for c in cases]
        states, refs, contacts = dev(stack(cases, "state")), dev(stack(cases, "ref")), dev(stack(cases, "contact"))
        ctr = 0
        for step in range(3):
            for it in range(2):
                ctr += 1
                counters = [ctr + 5 * e for e in range(E)]
                with torch.cuda.stream(stream):
                    out = b.step_cem_device(states, refs, contacts, best, sigma, dev(np.asarray(seeds, np.uint64)),
                                            dev(np.asarray(counters, np.uint64)),
                                            sigma_reset=RESET if it == 0 else 0.0, want_costs=True, stream=stream)
                torch.cuda.synchronize()
                if it == 0:
                    ss = [np.full_like(s, RESET) for s in ss]
                want = single_steps(lib, cases, seeds, counters, bests=sb, sigmas=ss, ctxs=ctxs)
                gb, gs = best.cpu().numpy(), sigma.cpu().numpy()
                for e in range(E):
                    what = f"step {step} iteration {it} env {e}"
                    assert gb[e].tobytes() == want[e]["best"].tobytes(), what
                    assert gs[e].tobytes() == want[e]["sigma"].tobytes(), what
                    assert out["grf"][e].cpu().numpy().tobytes() == want[e]["grf"].tobytes(), what
                    assert out["predicted_state"][e].cpu().numpy().tobytes() == want[e]["pred"].tobytes(), what
                    assert out["costs"][e].cpu().numpy().tobytes() == want[e]["costs"].tobytes(), what
                    assert out["best_cost"][e].cpu().numpy().tobytes() == want[e]["best_cost"].tobytes(), what
                    assert int(out["best_index"][e]) == want[e]["best_index"], what
                sb = [w["best"] for w in want]
                ss = [w["sigma"] for w in want]
    finally:
        b.close()
        for c in ctxs:
            c.close()


def test_isolation(lib):
    """A NaN state in environment 1, an all-swing contact sequence in 2 and sigma at the 0.2 clamp in 3 change
    nothing in environments 0 and 4: their bytes equal a run without those three."""
    E = 5
    seeds, counters = default_keys(E)
    cases = env_cases(E, N=257, par="zero_order", H=12)
    clean = single_steps(lib, cases, seeds, counters)
    cases[1] = dict(cases[1], state=np.full(24, np.nan, f32))
    cases[2] = dict(cases[2], contact=np.zeros_like(cases[2]["contact"]))
    cases[3] = dict(cases[3], sigma=np.full_like(cases[3]["sigma"], 0.2))
    odd = single_steps(lib, cases[1:4], seeds[1:4], counters[1:4])
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    assert_same(got[0], clean[0], "env 0")
    assert_same(got[4], clean[4], "env 4")
    for e in (1, 2, 3):  # NaNs compare by bits
        for k in KEYS:
            assert got[e][k].tobytes() == odd[e - 1][k].tobytes(), (e, k)
        assert got[e]["best_index"] == odd[e - 1]["best_index"]
        assert got[e]["best_cost"].tobytes() == odd[e - 1]["best_cost"].tobytes()


def test_largest_batch_steps(lib):
    """E = 4096 at N = 64 allocates and steps; environments 0, 2047 and 4095 against single contexts."""
    E, spot = 4096, (0, 2047, 4095)
    base = env_cases(3, N=64, par="zero_order", H=12)
    cases = [base[e % 3] for e in range(E)]
    for i, e in enumerate(spot):
        cases[e] = base[i]
    seeds = [100 + e for e in range(E)]
    counters = [7 + (e % 11) for e in range(E)]
    want = single_steps(lib, [cases[e] for e in spot], [seeds[e] for e in spot], [counters[e] for e in spot])
    b = lib.CemBatchContext(product_cfg(base[0]), E)
    try:
        assert lib.lib.srbd_batch_num_envs(b.h) == E
        best, sigma, results, costs = b.step_cem(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                                 stack(cases, "best"), stack(cases, "sigma"), seeds=seeds,
                                                 counters=counters, want_costs=True)
    finally:
        b.close()
    for i, e in enumerate(spot):
        assert_same(result_dict(best[e], sigma[e], results[e], costs[e]), want[i], f"env {e}")


def test_mixing_rules(lib):
    """A plain step on a CEM batch and a _cem step on an MPPI batch are refused and change nothing."""
    E = 2
    seeds, counters = default_keys(E)
    cases = env_cases(E, N=130, par="zero_order", H=12)
    arrays = (stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"))
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        want = batch_step(b, cases, seeds, counters)
        best0 = stack(cases, "best")
        b._best[...] = best0
        with pytest.raises(RuntimeError, match="sigma is part of the step"):
            b.step(*arrays, best0, seeds=seeds, counters=counters)
        np.testing.assert_array_equal(b._best, best0)
        tb, ts = dev(best0), dev(stack(cases, "sigma"))
        with pytest.raises(RuntimeError, match="sigma is part of the step"):
            b.step_device(dev(arrays[0]), dev(arrays[1]), dev(arrays[2]), tb, dev(np.asarray(seeds, np.uint64)),
                          dev(np.asarray(counters, np.uint64)))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(tb.cpu().numpy(), best0)
        np.testing.assert_array_equal(b.copy_costs(), np.stack([w["costs"] for w in want]))  # the last step's still
        with pytest.raises(RuntimeError, match="gait-adaptive CEM"):
            b.set_gait(np.zeros((E, 4), f32), 0.02, 0.65, np.full((E, 1), 1.4, f32))
        again = batch_step(b, cases, seeds, counters)  # and the batch still steps exactly
        for e in range(E):
            assert_same(again[e], want[e], f"env {e}")
    finally:
        b.close()
    mppi = [make_case("c2", seed=e, k=e, N=130, method="mppi", par="zero_order", H=12) for e in range(E)]
    m = lib.BatchContext(product_cfg(mppi[0]), E)
    try:
        buf = np.zeros((E, m.P), f32)
        res = (lib.SrbdResult * E)()
        a = [np.ascontiguousarray(x, dtype=f32) for x in (stack(mppi, "state"), stack(mppi, "ref"),
                                                          stack(mppi, "contact"))]
        ks, kc = np.asarray(seeds, np.uint64), np.asarray(counters, np.uint64)
        import ctypes as C
        rc = lib.lib.srbd_batch_step_cem(m.h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 12,
                                         buf.ctypes.data, buf.ctypes.data, None, ks.ctypes.data, kc.ctypes.data,
                                         C.addressof(res), None)
        assert rc == lib.E_INVALID and b"not a CEM batch" in lib.lib.srbd_batch_last_error(m.h)
        assert not buf.any()
        # the device form on the MPPI batch: refused before anything is enqueued, so nothing is written
        E_, P_ = E, m.P
        t = dict(states=dev(a[0]), refs=dev(a[1]), contacts=dev(a[2]), best=dev(stack(mppi, "best")),
                 seeds=dev(ks), counters=dev(kc))
        out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in (
            ("grf", (E_, 12), torch.float32), ("predicted_state", (E_, 24), torch.float32),
            ("best_cost", (E_,), torch.float32), ("best_index", (E_,), torch.int32),
            ("best_freq", (E_,), torch.float32), ("status", (E_,), torch.int32))}
        sig = torch.full((E_, P_), 3.0, dtype=torch.float32, device="cuda")
        io = lib.BatchDeviceIO(states=t["states"].data_ptr(), refs=t["refs"].data_ptr(),
                               contacts=t["contacts"].data_ptr(), noise=None, seeds=t["seeds"].data_ptr(),
                               counters=t["counters"].data_ptr(), contact_stride=12, pad=0,
                               best_params=t["best"].data_ptr(), costs=None,
                               **{k: v.data_ptr() for k, v in out.items()})
        cem = lib.BatchCemIO(sigma=sig.data_ptr(), sigma_reset=0.0, pad=0)
        rc = lib.lib.srbd_batch_step_cem_device(m.h, C.byref(io), C.byref(cem), None)
        assert rc == lib.E_INVALID
        assert lib.lib.srbd_batch_last_error(m.h) == b"srbd_batch_step_cem_device: not a CEM batch (srbd_batch_create_cem)"
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t["best"].cpu().numpy(), stack(mppi, "best"))
        assert (sig == 3.0).all() and all((v == 77).all() for v in out.values())
        good = m.step(a[0], a[1], a[2], stack(mppi, "best"), seeds=seeds, counters=counters)  # and it still steps
        assert np.isfinite(good[0]).all()
    finally:
        m.close()


def test_device_form_refuses_sigma_on_another_device(lib):
    """sigma on the CPU beside device tensors: ValueError, nothing enqueued (best unchanged)."""
    E = 2
    cases = env_cases(E, N=130, par="zero_order", H=12)
    seeds, counters = default_keys(E)
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        best = dev(stack(cases, "best"))
        with pytest.raises(ValueError, match="sigma must be on cuda"):
            b.step_cem_device(dev(stack(cases, "state")), dev(stack(cases, "ref")), dev(stack(cases, "contact")), best,
                              torch.from_numpy(stack(cases, "sigma")), dev(np.asarray(seeds, np.uint64)),
                              dev(np.asarray(counters, np.uint64)))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(best.cpu().numpy(), stack(cases, "best"))
    finally:
        b.close()


def cem_config(**mpc):
    from quadruped_pympc_amd import config as mirror

    cfg = types.ModuleType("cem_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, sampling_method="cem_mppi", num_parallel_computations=700,
                          num_sampling_iterations=2, **mpc)
    return cfg


@pytest.mark.parametrize("rng", ["philox", "jax"])
def test_controller_device_form(lib, rng):
    """Batched_CEM_Sampling_MPC.compute_control_device driven as its module docstring shows -- two control steps of
    two sampling iterations, sigma_reset on the first and None afterwards, keys advanced on the host and uploaded --
    against compute_control (the host form) of a second controller given the same keys, best and sigma.  Every
    member of the 8-tuple is compared; the JAX stream also checks that both forms number their calls alike."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC

    E = 3
    cfg = cem_config(rng=rng)
    cd, ch = Batched_CEM_Sampling_MPC(E, cfg), Batched_CEM_Sampling_MPC(E, cfg)
    cases = env_cases(E, N=700, par=cd.control_parametrization, H=cd.horizon)
    stream = torch.cuda.Stream()
    try:
        states, refs, contacts = dev(stack(cases, "state")), dev(stack(cases, "ref")), dev(stack(cases, "contact"))
        best = dev(np.array(cd.best_control_parameters))
        sigma = torch.empty((E, cd.num_control_parameters), dtype=torch.float32, device="cuda")
        hb = np.array(ch.best_control_parameters)
        for step in range(2):
            for it in range(cd.num_sampling_iterations):
                cd.with_newkey()
                ch.with_newkey()
                np.testing.assert_array_equal(cd.get_key(), ch.get_key())
                if rng == "philox":
                    keys = dev(np.asarray(cd.get_key(), np.uint64))
                else:
                    keys = dev(np.array([lib.pack_key(k) for k in cd.get_key()], np.uint64))
                with torch.cuda.stream(stream):
                    out = cd.compute_control_device(states, refs, contacts, best, keys, sigma, stream=stream,
                                                    sigma_reset=cd.sigma_reset_value if it == 0 else None)
                torch.cuda.synchronize()
                if it == 0:
                    ch.with_newsigma(cfg.mpc_params["sigma_cem_mppi"])
                ref = ch.compute_control(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"), hb,
                                         ch.get_key(), ch.get_sigma())
                what = f"step {step} iteration {it}"
                assert len(out) == 8 and len(ref) == 8
                assert out[3] is best and out[7] is sigma  # updated in place and returned
                for i in (0, 1, 2, 3, 4, 7):  # GRFs, footholds, predicted states, best, best costs, sigma
                    g = out[i].cpu().numpy()
                    assert g.dtype == ref[i].dtype and g.tobytes() == ref[i].tobytes(), f"{what} item {i}"
                np.testing.assert_array_equal(out[5].cpu().numpy(), ref[5], err_msg=what)
                np.testing.assert_array_equal(np.asarray(out[6]), np.asarray(ref[6]), err_msg=what)
                hb = ref[3]
                ch.with_newsigma(ref[7])
        assert cd._calls == ch._calls == 4
    finally:
        cd.close()
        ch.close()


def test_controller_class(lib):
    """Batched_CEM_Sampling_MPC at E = 2 against two Sampling_MPC objects driven as SRBDControllerInterface drives
    them: per control step two sampling iterations, with_newkey each, with_newsigma(configured constant) on the
    first, the returned best and sigma fed back.  Every member of the 8-tuple is compared."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip import Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC

    cfg = cem_config()
    E = 2
    batched = Batched_CEM_Sampling_MPC(E, cfg)
    singles = [Sampling_MPC(cfg) for _ in range(E)]
    cases = env_cases(E, N=700, par=batched.control_parametrization, H=batched.horizon)
    try:
        for e in range(E):
            singles[e].master_key = np.array(batched.master_keys[e])
        bb = np.array(batched.best_control_parameters)
        for step in range(2):
            for it in range(batched.num_sampling_iterations):
                batched.with_newkey()
                if it == 0:
                    batched.with_newsigma(cfg.mpc_params["sigma_cem_mppi"])
                out = batched.compute_control(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                              bb, batched.get_key(), batched.get_sigma())
                assert len(out) == 8
                for e in range(E):
                    s = singles[e].with_newkey()
                    if it == 0:
                        s.with_newsigma(cfg.mpc_params["sigma_cem_mppi"])
                    np.testing.assert_array_equal(batched.master_keys[e], s.master_key)
                    ref = s.compute_control(cases[e]["state"], cases[e]["ref"], cases[e]["contact"], bb[e],
                                            s.get_key(), s.get_sigma())
                    assert len(ref) == 8
                    what = f"step {step} iteration {it} env {e}"
                    for i in (0, 1, 2, 3, 7):  # GRFs, footholds, predicted state, best parameters, sigma
                        np.testing.assert_array_equal(out[i][e], ref[i], err_msg=f"{what} item {i}")
                    assert f32(out[4][e]).tobytes() == f32(ref[4]).tobytes(), what
                    assert out[5][e] == ref[5], what
                    np.testing.assert_array_equal(np.asarray(out[6])[e], np.asarray(ref[6]), err_msg=what)
                    s.with_newsigma(ref[7])
                bb = out[3]
                batched.with_newsigma(out[7])
    finally:
        batched.close()
        for s in singles:
            s.close()
