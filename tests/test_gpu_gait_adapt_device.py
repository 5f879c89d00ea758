"""The device-resident gait adaptation loop (srbd_stc_touch_down_device, srbd_batch_set_gait_device,
srbd_gait_apply_freq_device, include/srbd_mpc.h; BatchContext.set_gait_device,
BatchedSwingTrajectoryController.check_touch_down_condition, the gait-adaptive Batched_Sampling_MPC's
compute_control_device and apply_step_frequency) against the host forms: srbd_stc_touch_down and srbd_gait_apply_freq
(include/srbd_host.h), which tests/test_gait_adapt_host.py pins to the recorded reference, and srbd_batch_set_gait.  The
contract is bit equality, so every comparison is exact and no tolerance appears here.  Expected values never come from
the device-side calls under test."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from helpers import f32, make_case, product_cfg
from quadruped_pympc_amd import config as mirror

pytestmark = pytest.mark.gpu

REF = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gait_adapt_ref.npz")))
H = int(REF["horizon"])
AVAIL = np.array([1.4, 2.0, 2.4], f32)
PGG_DT, GA_DUTY = 0.02, 0.65
N = 130  # three leaves, the last one partial


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. the trigger
def gait_rows(lookahead):
    """The fixture's three gait sequences recorded with this lookahead: (first row, rows, first firing row)."""
    out = []
    for i, name in enumerate(REF["td_names"]):
        if not str(name).startswith("hand/") and str(name).endswith(f"lookahead{lookahead}"):
            a, b = int(REF["td_start"][i]), int(REF["td_start"][i + 1])
            fire = a + int(np.flatnonzero(REF["td_flag"][a:b] == 1)[1])  # the second firing: an edge precedes it
            out.append((a, b, fire))
    assert len(out) == 3
    return out


@pytest.mark.parametrize("lookahead", [1, 3])
@pytest.mark.parametrize("E", [1, 3, 65, 4096])
def test_trigger_equals_the_host_function(lib, E, lookahead):
    """Environment e walks the fixture's inputs of gait e % 3 (trot 1.4 Hz, pace 1.4 Hz, crawl 0.5 Hz), shifted so that
    it fires 4 + (e + e // 3) % 8 steps in; its edge state starts as the reference left it one row earlier."""
    steps, rows = 14, gait_rows(lookahead)
    first = np.array([rows[e % 3][2] - 4 - (e + e // 3) % 8 for e in range(E)])
    assert all(rows[e % 3][0] < first[e] and first[e] + steps <= rows[e % 3][1] for e in range(E))
    edge0 = REF["td_edge_after"][first - 1].astype(np.int32)
    # the host side first: the expected flags and edge states, and the scenario's condition
    edges = [C.c_int32(int(v)) for v in edge0]
    want_flag, want_edge = np.zeros((steps, E), np.int32), np.zeros((steps, E), np.int32)
    for k in range(steps):
        for e in range(E):
            i = first[e] + k
            cur, prev, seq = (np.ascontiguousarray(REF[n][i], np.float64) for n in ("td_current", "td_previous",
                                                                                    "td_sequence"))
            want_flag[k, e] = lib.lib.srbd_stc_touch_down(C.byref(edges[e]), lib.dptr(cur), lib.dptr(prev),
                                                          lib.dptr(seq), H, H, lookahead)
            want_edge[k, e] = edges[e].value
    assert (want_flag >= 0).all() and want_flag.sum() >= E  # every environment fires
    if E > 1:
        mixed = [k for k in range(steps) if 0 < want_flag[k].sum() < E]
        assert mixed, "some environment must fire while another does not at the same step"
    idx = first[None, :] + np.arange(steps)[:, None]
    cur, prev = cuda(REF["td_current"][idx].astype(f32)), cuda(REF["td_previous"][idx].astype(f32))
    seq = torch.full((steps, E, 4, H + 3), 7.0, dtype=torch.float32, device="cuda")  # a stride beyond the horizon
    seq[:, :, :, :H] = cuda(REF["td_sequence"][idx].astype(f32))
    edge = cuda(edge0)
    got_flag, got_edge = [], []
    for k in range(steps):
        got_flag.append(lib.stc_touch_down_device(edge, cur[k], prev[k], seq[k], lookahead, horizon=H))
        got_edge.append(edge.clone())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.stack(got_flag).cpu().numpy(), want_flag)
    np.testing.assert_array_equal(torch.stack(got_edge).cpu().numpy(), want_edge)


def test_trigger_class_carries_its_edge_state(lib):
    from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController

    E = 3
    stc = BatchedSwingTrajectoryController(E, 0.06, 0.25, 500.0, 10.0)
    ones = torch.ones((E, 4), dtype=torch.float32, device="cuda")
    prev = ones.clone()
    prev[1, 2] = 0.0  # environment 1 has just touched down
    seq = torch.ones((E, 4, H), dtype=torch.float32, device="cuda")
    seq[:, 0, 4:] = 0.0  # stable for four columns: lookahead 3 does not fire yet
    flags = stc.check_touch_down_condition(ones, prev, seq)
    assert flags.dtype == torch.int32 and flags.is_cuda and flags.cpu().tolist() == [0, 0, 0]
    sd = stc.state_dict()
    assert sd.rising_edge.tolist() == [0, 1, 0]
    other = BatchedSwingTrajectoryController(E, 0.06, 0.25, 500.0, 10.0)
    other.load_state_dict(sd)
    seq[:, 0, 3] = 0.0
    assert other.check_touch_down_condition(ones, ones, seq).cpu().tolist() == [0, 1, 0]
    assert other.rising_edge.cpu().tolist() == [0, 0, 0]
    other.load_state_dict(bytes(sd))  # a plain byte string carries no edge
    assert other.rising_edge.cpu().tolist() == [0, 0, 0]


# ------------------------------------------------------------------ 2. the write-back
def host_structs(lib, E, rng):
    duties = (0.65, 0.5, 0.7)
    pgg, frg, stc = (lib.SrbdPgg * E)(), (lib.SrbdFrg * E)(), (lib.SrbdStc * E)()
    for e in range(E):
        assert lib.lib.srbd_pgg_init(C.byref(pgg[e]), e % 7, duties[e % 3], 1.3 + 0.01 * (e % 5), H) == 0
        assert lib.lib.srbd_frg_init(C.byref(frg[e]), 0.3 + 0.01 * (e % 4), 0.25, lib.dptr(rng.uniform(-1, 1, 12))) == 0
        assert lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, 0.2 + 0.01 * (e % 6), 500.0, 10.0, e % 2) == 0
    return pgg, frg, stc


def as_tensor(structs):
    n = len(structs)
    return cuda(np.frombuffer(bytes(structs), np.uint8).reshape(n, -1).copy())


@pytest.mark.parametrize("E", [1, 3, 65, 4096])
def test_write_back_equals_the_host_function(lib, E):
    rng = np.random.default_rng(E)
    freqs = np.concatenate([REF["wb_best_freq"], np.array([0.0, -1.4, np.nan, np.inf, -np.inf], f32)])
    best = freqs[(np.arange(E) * 7 + 3) % len(freqs)].astype(f32)
    optimize = np.array([(1, 1, 0, 1, 2)[e % 5] for e in range(E)], np.int32)
    if E == 1:
        optimize[:] = 1
    d_opt, d_best = cuda(optimize), cuda(best)
    for use_frg, use_stc in ((True, True), (False, True), (True, False), (False, False)):
        pgg, frg, stc = host_structs(lib, E, rng)
        before = [bytes(x) for x in (pgg, frg, stc)]
        d_pgg, d_frg, d_stc = as_tensor(pgg), as_tensor(frg), as_tensor(stc)
        wrote = np.zeros(E, np.int32)
        for e in range(E):
            wrote[e] = lib.lib.srbd_gait_apply_freq(C.byref(pgg[e]), C.byref(frg[e]) if use_frg else None,
                                                    C.byref(stc[e]) if use_stc else None, int(optimize[e]),
                                                    float(best[e]))
        assert (wrote >= 0).all()
        if E > 1:
            assert 0 < wrote.sum() < E  # written and untouched environments side by side
        lib.gait_apply_freq_device(d_pgg, d_opt, d_best, frg=d_frg if use_frg else None,
                                   stc=d_stc if use_stc else None)
        torch.cuda.synchronize()
        for name, t, host, b0, used in (("pgg", d_pgg, pgg, before[0], True), ("frg", d_frg, frg, before[1], use_frg),
                                        ("stc", d_stc, stc, before[2], use_stc)):
            got = t.cpu().numpy().tobytes()
            assert got == bytes(host), (name, use_frg, use_stc)
            if not used:
                assert got == b0, name
        # untouched environments: optimize != 1 or a bad frequency
        size = C.sizeof(lib.SrbdPgg)
        for e in np.flatnonzero(wrote == 0):
            assert d_pgg[e].cpu().numpy().tobytes() == before[0][e * size:(e + 1) * size], e
        assert all(wrote[e] == 0 for e in range(E) if optimize[e] != 1 or not (np.isfinite(best[e]) and best[e] > 0))


# ------------------------------------------------------------------ 3. the gait fields
def env_cases(E, **kw):
    return [make_case("c2", seed=e, k=e, N=N, H=H, **kw) for e in range(E)]


def stack(cases, key):
    return np.stack([c[key] for c in cases])


def device_step(b, cases, seeds, counters, noise=False, stream=None):
    """One step_device with the cases' inputs; the outputs as host arrays after a synchronisation."""
    best = cuda(stack(cases, "best"))
    out = b.step_device(cuda(stack(cases, "state")), cuda(stack(cases, "ref")), cuda(stack(cases, "contact")), best,
                        cuda(np.asarray(seeds, np.uint64).view(np.int64)),
                        cuda(np.asarray(counters, np.uint64).view(np.int64)),
                        noise=cuda(stack(cases, "noise")) if noise else None, want_costs=True, stream=stream)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["best"] = best.cpu().numpy()
    return res


def assert_same_step(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"


def host_sets(method, optimize, nominal):
    """Sampling_MPC._freq_set per environment."""
    if method == "random_sampling":
        return np.stack([np.where(bool(o), AVAIL, f32(n)).astype(f32) for o, n in zip(optimize, nominal)])
    return np.stack([AVAIL for _ in optimize])


def keys_for(lib, rng, E):
    if rng == "philox":
        return [100 + e for e in range(E)], [7 + 2 * e for e in range(E)]
    return [lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)], [1] * E


GAIT_CASES = [
    # name, E, method, parametrization, rng, phases from, injected rows
    ("mppi_zo_philox_pgg_e3", 3, "mppi", "zero_order", "philox", "pgg", False),
    ("rs_zo_philox_pgg_e3", 3, "random_sampling", "zero_order", "philox", "pgg", False),
    ("rs_zo_philox_timings_e65", 65, "random_sampling", "zero_order", "philox", "timings", False),
    ("mppi_lin_philox_timings_e3", 3, "mppi", "linear_spline", "philox", "timings", False),
    ("rs_lin_jax_pgg_e3", 3, "random_sampling", "linear_spline", "jax", "pgg", False),
    ("mppi_zo_jax_timings_e1", 1, "mppi", "zero_order", "jax", "timings", False),
    ("rs_zo_philox_pgg_nominal_e1", 1, "random_sampling", "zero_order", "philox", "pgg+nominal", False),
    ("mppi_zo_injected_timings_e3", 3, "mppi", "zero_order", "philox", "timings", True),
    ("rs_lin_injected_pgg_e65", 65, "random_sampling", "linear_spline", "philox", "pgg", True),
]


@pytest.mark.parametrize("name,E,method,par,rng,source,injected", GAIT_CASES, ids=[c[0] for c in GAIT_CASES])
def test_set_gait_device_equals_host_set_gait(lib, name, E, method, par, rng, source, injected):
    from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator

    cases = env_cases(E, method=method, par=par)
    seeds, counters = keys_for(lib, rng, E)
    gen_rng = np.random.default_rng(11)
    # phases that float32 does not represent, step frequencies outside the candidate set
    phases = gen_rng.uniform(0.0, 1.0, (E, 4))
    step_freq = 1.3 + 0.05 * (np.arange(E) % 4)
    optimize = np.array([(1, 0, 2)[e % 3] for e in range(E)], np.int32)  # 2: bool(optimize_swing) is true
    if E == 1:
        optimize[:] = 0 if "nominal" in source else 1
    rows = None
    if injected:
        rows = np.stack([np.random.default_rng(50 + e).choice(AVAIL, N) for e in range(E)]).astype(f32)
    gen = nominal_t = timings_t = None
    if source.startswith("pgg"):
        gen = BatchedPeriodicGaitGenerator(E, 0.65, step_freq, [e % 3 for e in range(E)], H)
        gen.set_phase_signal(phases)
        nominal = step_freq.astype(f32)
        if "nominal" in source:  # an explicit nominal frequency goes before the generator's
            nominal = np.full(E, 1.65, f32)
            nominal_t = cuda(nominal)
    else:
        nominal = step_freq.astype(f32)
        timings_t, nominal_t = cuda(phases.astype(f32)), cuda(nominal)
    a, b = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        for x in (a, b):
            if rng != "philox":
                x.set_rng(rng)
        # the expected values: the host set_gait with the values the device form is documented to use
        b.set_gait(phases.astype(f32), PGG_DT, GA_DUTY, host_sets(method, optimize, nominal), rows)
        want = device_step(b, cases, seeds, counters, noise=injected)
        a.set_gait_device(cuda(optimize), AVAIL, PGG_DT, GA_DUTY, pgg=None if gen is None else gen.state,
                          timings=timings_t, nominal_freqs=nominal_t, freq_rows=None if rows is None else cuda(rows))
        got = device_step(a, cases, seeds, counters, noise=injected)
        assert_same_step(got, want, name)
        assert (want["status"] == 0).all()
        if method == "random_sampling" and not injected:
            for e in np.flatnonzero(optimize == 0):  # a one-value set: the nominal frequency comes back
                assert got["best_freq"][e] == nominal[e]
        if injected:
            assert all(got["best_freq"][e] in AVAIL for e in range(E))
        # a second set with other values replaces the first (the rows too)
        optimize2 = (1 - (optimize != 0)).astype(np.int32)
        rows2 = None if rows is None else rows[::-1].copy()
        b.set_gait(phases[:, ::-1].astype(f32), PGG_DT, GA_DUTY, host_sets(method, optimize2, nominal), rows2)
        want2 = device_step(b, cases, seeds, counters, noise=injected)
        a.set_gait_device(cuda(optimize2), AVAIL, PGG_DT, GA_DUTY, timings=cuda(phases[:, ::-1].astype(f32)),
                          nominal_freqs=cuda(nominal), freq_rows=None if rows2 is None else cuda(rows2))
        assert_same_step(device_step(a, cases, seeds, counters, noise=injected), want2, name + " (second set)")
    finally:
        a.close()
        b.close()


def test_set_gait_device_refusals_with_a_batch(lib):
    cases = env_cases(2, method="mppi", par="zero_order")
    b = lib.BatchContext(product_cfg(cases[0]), 2)
    try:
        opt = torch.ones(2, dtype=torch.int32, device="cuda")
        t, nom = torch.zeros((2, 4), device="cuda"), torch.ones(2, device="cuda")
        with pytest.raises(ValueError, match="exactly one"):
            b.set_gait_device(opt, AVAIL, PGG_DT, GA_DUTY)
        with pytest.raises(ValueError, match="nominal_freqs"):
            b.set_gait_device(opt, AVAIL, PGG_DT, GA_DUTY, timings=t)
        with pytest.raises(ValueError, match="available"):
            b.set_gait_device(opt, np.ones(9), PGG_DT, GA_DUTY, timings=t, nominal_freqs=nom)
        with pytest.raises(ValueError, match="optimize must be torch.int32"):
            b.set_gait_device(opt.long(), AVAIL, PGG_DT, GA_DUTY, timings=t, nominal_freqs=nom)
        with pytest.raises(ValueError, match="timings must be"):
            b.set_gait_device(opt, AVAIL, PGG_DT, GA_DUTY, timings=t[:, :3].contiguous(), nominal_freqs=nom)
        with pytest.raises(ValueError, match="must be on"):
            b.set_gait_device(opt.cpu(), AVAIL, PGG_DT, GA_DUTY, timings=t, nominal_freqs=nom)
        b.set_cost_terms((0.1, 0.1, 0.001), 0.01, 5.0)
        with pytest.raises(RuntimeError, match="cost terms"):
            b.set_gait_device(opt, AVAIL, PGG_DT, GA_DUTY, timings=t, nominal_freqs=nom)
    finally:
        b.close()


# ------------------------------------------------------------------ 4. stream order
def test_set_on_one_stream_step_on_another(lib):
    E = 3
    cases = env_cases(E, method="random_sampling", par="zero_order")
    seeds, counters = keys_for(lib, "philox", E)
    optimize = cuda(np.array([1, 0, 1], np.int32))
    timings = cuda(np.random.default_rng(3).uniform(0, 1, (E, 4)).astype(f32))
    nominal = cuda(np.array([1.3, 1.35, 1.45], f32))
    rows = cuda(np.stack([np.random.default_rng(60 + e).choice(AVAIL, N) for e in range(E)]).astype(f32))
    a, b = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_gait_device(optimize, AVAIL, PGG_DT, GA_DUTY, timings=timings, nominal_freqs=nominal, freq_rows=rows)
        want = device_step(b, cases, seeds, counters, noise=True)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a.set_gait_device(optimize, AVAIL, PGG_DT, GA_DUTY, timings=timings, nominal_freqs=nominal, freq_rows=rows,
                          stream=s1)
        got = device_step(a, cases, seeds, counters, noise=True, stream=s2)
        assert_same_step(got, want, "two streams")
        # and back: a set on the second stream follows the step on it, a step on the first follows that set
        a.set_gait_device(optimize, AVAIL, PGG_DT, GA_DUTY, timings=timings, nominal_freqs=nominal, freq_rows=rows,
                          stream=s2)
        assert_same_step(device_step(a, cases, seeds, counters, noise=True, stream=s1), want, "streams swapped")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. stale staging
def host_step(b, cases, seeds, counters):
    best, results, costs = b.step(stack(cases, "state"), stack(cases, "ref"), stack(cases, "contact"),
                                  stack(cases, "best"), seeds=seeds, counters=counters, want_costs=True)
    return dict(best=best, costs=costs, grf=np.array([r.grf[:] for r in results], f32),
                best_cost=np.array([r.best_cost for r in results], f32),
                best_freq=np.array([r.best_freq for r in results], f32))


def test_host_step_refused_while_the_staging_is_stale(lib):
    E = 3
    cases = env_cases(E, method="mppi", par="zero_order")
    seeds, counters = keys_for(lib, "philox", E)
    timings = np.random.default_rng(4).uniform(0, 1, (E, 4)).astype(f32)
    nominal, optimize = np.array([1.3, 1.35, 1.45], f32), np.ones(E, np.int32)
    a, fresh = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        plain = host_step(fresh, cases, seeds, counters)
        fresh.set_gait(timings, PGG_DT, GA_DUTY, host_sets("mppi", optimize, nominal))
        adaptive = host_step(fresh, cases, seeds, counters)
        assert (plain["best_freq"] == 0).all() and all(f in AVAIL for f in adaptive["best_freq"])

        def set_on_device():
            a.set_gait_device(cuda(optimize), AVAIL, PGG_DT, GA_DUTY, timings=cuda(timings), nominal_freqs=cuda(nominal))

        set_on_device()
        a._best[...] = 5.0  # the host step's staging: a refused step must not rewrite it
        with pytest.raises(RuntimeError, match="srbd_batch_set_gait or srbd_batch_clear_gait") as err:
            host_step(a, cases, seeds, counters)
        assert "(-1)" in str(err.value) and "stale" in str(err.value)
        # the device step is not affected, and the refusal changed nothing
        got = device_step(a, cases, seeds, counters)
        assert got["best"].tobytes() == adaptive["best"].tobytes()
        assert got["best_freq"].tobytes() == adaptive["best_freq"].tobytes()
        with pytest.raises(RuntimeError, match="srbd_batch_set_gait or srbd_batch_clear_gait"):
            host_step(a, cases, seeds, counters)
        a.clear_gait()
        after_clear = host_step(a, cases, seeds, counters)
        for k in plain:
            assert after_clear[k].tobytes() == plain[k].tobytes(), f"after clear_gait: {k}"
        set_on_device()
        with pytest.raises(RuntimeError, match="stale"):
            host_step(a, cases, seeds, counters)
        a.set_gait(timings, PGG_DT, GA_DUTY, host_sets("mppi", optimize, nominal))
        after_set = host_step(a, cases, seeds, counters)
        for k in adaptive:
            assert after_set[k].tobytes() == adaptive[k].tobytes(), f"after set_gait: {k}"
    finally:
        a.close()
        fresh.close()


# ------------------------------------------------------------------ 6. the closed loop
def config_with(**mpc):
    cfg = types.ModuleType("gait_adapt_device_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, **mpc)
    return cfg


def test_closed_loop_equals_the_host_driven_loop(lib):
    """60 steps of run -> contact sequence -> trigger -> set_gait_device -> step_device -> apply with nothing read
    back in between, against the same loop driven per environment by the host functions (host set_gait, the device
    step).  The step frequencies start at 1.3, outside step_freq_available, so every adaptation shows."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import \
        Batched_Sampling_MPC as Batched_Base
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_gait_adaptive_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
    from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController

    E, steps, dt, lookahead = 3, 60, 0.02, 3
    gaits, duty = [0, 1, 5], [0.65, 0.7, 0.8]  # trot, pace, a crawl (whose full-stance gaps are shorter than 3 columns)
    cfg = config_with(num_parallel_computations=N, horizon=H, sampling_method="random_sampling",
                      control_parametrization="zero_order", shift_solution=False, rng="philox", device_id=0,
                      step_freq_available=[1.4, 2.0, 2.4])
    on_dev, on_host = Batched_Sampling_MPC(E, cfg), Batched_Sampling_MPC(E, cfg)
    assert on_dev.dt == PGG_DT
    cases = env_cases(E, method="random_sampling", par="zero_order")
    states, refs = cuda(stack(cases, "state")), cuda(stack(cases, "ref"))
    best0 = stack(cases, "best")
    keys = np.stack([[[100 + e, k] for e in range(E)] for k in range(steps)]).astype(np.uint64)
    d_keys = cuda(keys.view(np.int64))
    rng = np.random.default_rng(8)
    try:
        # ---- the host-driven loop: host structs, host trigger, host set_gait, host write-back
        pgg, frg, stc = (lib.SrbdPgg * E)(), (lib.SrbdFrg * E)(), (lib.SrbdStc * E)()
        for e in range(E):
            assert lib.lib.srbd_pgg_init(C.byref(pgg[e]), gaits[e], duty[e], 1.3, H) == 0
            assert lib.lib.srbd_frg_init(C.byref(frg[e]), 0.5, 0.25, lib.dptr(rng.uniform(-1, 1, 12))) == 0
            assert lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, 0.27, 500.0, 10.0, 0) == 0
        frg0 = bytes(frg)
        edges = [C.c_int32(0) for _ in range(E)]
        dts, lens = np.array([dt]), np.array([H], np.int32)
        previous = np.ones((E, 4))
        best_t = cuda(best0)
        want, fired = [], np.zeros(E, int)
        for k in range(steps):
            current, seqs, optimize = np.zeros((E, 4)), np.zeros((E, 4, H)), np.zeros(E, np.int32)
            for e in range(E):
                assert lib.lib.srbd_pgg_run(C.byref(pgg[e]), dt, pgg[e].step_freq, lib.dptr(current[e])) == 0
                assert lib.lib.srbd_pgg_contact_sequence(C.byref(pgg[e]), lib.dptr(dts), lib.iptr(lens), 1,
                                                         lib.dptr(seqs[e]), 4 * H) == H
                optimize[e] = lib.lib.srbd_stc_touch_down(C.byref(edges[e]), lib.dptr(current[e]),
                                                          lib.dptr(previous[e]), lib.dptr(seqs[e]), H, H, lookahead)
            assert (optimize >= 0).all()
            fired += optimize
            timings = np.array([list(pgg[e].phase_signal) for e in range(E)]).astype(f32)
            nominal = np.array([pgg[e].step_freq for e in range(E)]).astype(f32)
            on_host.context.set_gait(timings, PGG_DT, GA_DUTY, on_host.freq_sets(nominal, optimize))
            out = Batched_Base.compute_control_device(on_host, states, refs, cuda(seqs.astype(f32)), best_t, d_keys[k])
            torch.cuda.synchronize()
            freq = out[5].cpu().numpy()
            assert freq.dtype == f32
            for e in range(E):
                assert lib.lib.srbd_gait_apply_freq(C.byref(pgg[e]), C.byref(frg[e]), C.byref(stc[e]),
                                                    int(optimize[e]), float(freq[e])) >= 0
            want.append(dict(contact=current.astype(f32), seq=seqs.astype(f32), optimize=optimize.copy(),
                             edge=np.array([x.value for x in edges], np.int32), grf=out[0].cpu().numpy(),
                             pred=out[2].cpu().numpy(), best=best_t.cpu().numpy(), cost=out[4].cpu().numpy(),
                             freq=freq, costs=np.asarray(out[6]), pgg=bytes(pgg), frg=bytes(frg), stc=bytes(stc)))
            previous = current
        # the scenario's condition, on the host values
        assert (fired >= 2).sum() >= 2, f"the host trigger must fire twice in two environments, fired {fired}"
        adapted = [e for e in range(E) if fired[e] >= 2]
        for e in adapted:
            assert pgg[e].step_freq != 1.3 and f32(pgg[e].step_freq) in AVAIL
        assert any(w["optimize"].sum() not in (0, E) for w in want)

        # ---- the device loop: nothing read back until the end
        gen = BatchedPeriodicGaitGenerator(E, duty, 1.3, gaits, H)
        ctl = BatchedSwingTrajectoryController(E, 0.06, 0.27, 500.0, 10.0)
        d_frg = cuda(np.frombuffer(frg0, np.uint8).reshape(E, -1).copy())
        best_t = cuda(best0)
        d_prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got = []
        for k in range(steps):
            current = gen.run(dt)
            seq = gen.compute_contact_sequence([dt], [H])
            optimize = ctl.check_touch_down_condition(current, d_prev, seq, lookahead=lookahead)
            out = on_dev.compute_control_device(states, refs, seq, best_t, d_keys[k], gait=gen,
                                                optimize_swings=optimize)
            on_dev.apply_step_frequency(optimize, out[5], gait=gen, frg=d_frg, stc=ctl)
            got.append(dict(contact=current, seq=seq, optimize=optimize, edge=ctl.rising_edge.clone(), grf=out[0],
                            pred=out[2], best=best_t.clone(), cost=out[4], freq=out[5],
                            pgg=gen.state.clone(), frg=d_frg.clone(), stc=ctl.state.clone()))
            d_prev = current
        torch.cuda.synchronize()
        for k in range(steps):
            for name in ("contact", "seq", "optimize", "edge", "grf", "pred", "best", "cost", "freq"):
                g, w = got[k][name].cpu().numpy(), want[k][name]
                assert g.dtype == w.dtype and g.shape == w.shape, f"step {k} {name}"
                assert g.tobytes() == w.tobytes(), f"step {k} {name}"
            for name in ("pgg", "frg", "stc"):
                assert got[k][name].cpu().numpy().tobytes() == want[k][name], f"step {k}: {name} state"
        # the last step's costs rows (fetched lazily from the device batch)
        np.testing.assert_array_equal(on_dev.context.copy_costs(), want[-1]["costs"])
    finally:
        on_dev.close()
        on_host.close()
