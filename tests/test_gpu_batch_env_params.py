"""Per-environment robot and cost parameters of a batch on the GPU (srbd_batch_set_env_params and its device form,
include/srbd_mpc.h): environment e of a batch step against a plain ``Context`` created from the batch's configuration
with environment e's seven fields (bit for bit, every output), the device step and the device setter against the host
forms (bytewise), and the CPU oracle of each environment's robot with injected noise (the tolerances and the near-tie
rule of tests/test_gpu_batch.py).  Expected values never come from the batch itself."""

import numpy as np
import pytest
import torch

import test_gpu_batch_cem as tcem
import test_gpu_batch_device as tdev
import test_gpu_batch_features as tfeat
from helpers import f32, product_cfg
from oracle.srbd_oracle import SamplingMPCOracle
from test_gpu_batch import assert_same, batch_step, check_end_to_end, check_reduction, env_cases, result_dict

pytestmark = pytest.mark.gpu

MUS = (0.3, 0.5, 0.8, 1.0)


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def env_params(lib, cases, shift=0):
    """Environment e's robot, all distinct: mass w.mass (0.7 + 0.15 e), inertia scaled by (0.8 + 0.1 e) plus a small
    symmetric off-diagonal, mu from MUS, grf_max from the mass, grf_min 0 / 5, q_diag perturbed per entry and the
    feet weights q_diag[12:] non-zero in environment 1.  Environment 0 keeps the configuration's own values.
    shift: another draw of the same kind (e -> e + shift) for the tests that change parameters."""
    E, w, cfg = len(cases), cases[0]["w"], product_cfg(cases[0])
    I0 = np.asarray(w.inertia, np.float64).reshape(3, 3)
    q0 = np.array(cfg.q_diag[:], np.float64)
    mass, inertia, mu, grf_min, q = [], [], [], [], []
    for e in range(E):
        k = e + shift
        mass.append(w.mass * (0.7 + 0.15 * k))
        off = np.zeros((3, 3))
        off[0, 1] = off[1, 0] = 0.002 * (k + 1)
        off[1, 2] = off[2, 1] = -0.001 * (k + 1)
        inertia.append(I0 * (0.8 + 0.1 * k) + off)
        mu.append(MUS[k % 4])
        grf_min.append((0.0, 5.0)[k % 2])
        qe = q0 * (1.0 + 0.03 * (k + 1) * np.cos(np.arange(24) + k))
        qe[12:] = 3.0 + 0.25 * np.arange(12) if k == 1 else 0.0
        q.append(qe)
    p = lib.make_env_params(E, cfg, mass=mass, inertia=np.array(inertia), mu=mu, grf_min=grf_min, q_diag=np.array(q))
    if shift == 0:
        p[0] = lib.make_env_params(1, cfg)[0]
    return p


def single_steps(lib, cases, params, seeds, counters, noise=False):
    """The expected values: one plain Context per environment, created from the cases' configuration with that
    environment's fields, stepped with that environment's inputs."""
    out = []
    for e, c in enumerate(cases):
        ctx = lib.Context(lib.config_with_env_params(product_cfg(c), params[e]))
        try:
            best, _, res, costs = ctx.step(c["state"], c["ref"], c["contact"], c["best"],
                                           noise=c["noise"] if noise else None, seed=int(seeds[e]),
                                           counter=int(counters[e]), want_costs=True)
            assert res.status == 0
            out.append(result_dict(best, res, costs))
        finally:
            ctx.close()
    return out


def keys_of(E):
    return [100 + e for e in range(E)], [7 + 2 * e for e in range(E)]


def run_bit_equal(lib, cases):
    E = len(cases)
    seeds, counters = keys_of(E)
    p = env_params(lib, cases)
    want = single_steps(lib, cases, p, seeds, counters)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_env_params(p)
        got = batch_step(b, cases, seeds, counters)
        back = b.get_env_params()
    finally:
        b.close()
    assert back.tobytes() == p.tobytes()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
    return got


SHAPES = [
    ("zo_h12_n65", 3, dict(N=65, method="mppi", par="zero_order", H=12)),      # a second leaf of one row
    ("zo_h12_n2113", 3, dict(N=2113, method="mppi", par="zero_order", H=12)),  # two level-1 nodes
    ("rs_h10_n257", 3, dict(wkey="c1", N=257, method="random_sampling", par="zero_order", H=10)),
    ("lin_s2_h12_n700", 3, dict(N=700, method="mppi", par="linear_spline", H=12, S=2)),
    ("cub_s2_h16_n700", 3, dict(N=700, method="mppi", par="cubic_spline", H=16, S=2)),
    ("zo_h8_n300", 3, dict(N=300, method="mppi", par="zero_order", H=8)),      # the generic shape
    ("zo_h12_n64_e5", 5, dict(N=64, method="mppi", par="zero_order", H=12)),   # more environments than leaves
]


@pytest.mark.parametrize("name,E,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_bit_equal_device_draws(lib, name, E, kw):
    run_bit_equal(lib, env_cases(E, **kw))


@pytest.mark.parametrize("kw", [dict(wkey="c3", N=700, par="cubic_spline", H=16, S=2),
                                dict(N=257, par="zero_order", H=12)], ids=["cub_s2_h16_n700", "zo_h12_n257"])
def test_cem_two_steps_sigma_fed_back(lib, kw):
    E = 3
    cases = tcem.env_cases(E, **kw)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(cases[e]), p[e])) for e in range(E)]
    b = lib.CemBatchContext(product_cfg(cases[0]), E)
    try:
        b.set_env_params(p)
        bests = sigmas = None
        for it in range(2):
            ctr = [c + it for c in counters]
            want = tcem.single_steps(lib, cases, seeds, ctr, bests=bests, sigmas=sigmas, ctxs=ctxs)
            got = tcem.batch_step(b, cases, seeds, ctr, bests=None if bests is None else np.stack(bests),
                                  sigmas=None if sigmas is None else np.stack(sigmas))
            for e in range(E):
                tcem.assert_same(got[e], want[e], f"step {it} env {e}")
            bests, sigmas = [w["best"] for w in want], [w["sigma"] for w in want]
        assert not np.array_equal(sigmas[0], sigmas[1])
    finally:
        b.close()
        for c in ctxs:
            c.close()


def test_gait_adaptive_device_drawn_frequencies(lib):
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    t, fs = tfeat.timings_of(E), tfeat.sets_of(cases, E)
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(cases[e]), p[e])) for e in range(E)]
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        want = tfeat.single_steps(lib, cases, seeds, counters, gait=(t, fs, None), ctxs=ctxs)
        b.set_env_params(p)
        b.set_gait(t, tfeat.PGG_DT, tfeat.GA_DUTY, fs)
        got = tfeat.batch_step(b, cases, seeds, counters)
    finally:
        b.close()
        for c in ctxs:
            c.close()
    for e in range(E):
        tfeat.assert_same(got[e], want[e], f"env {e}")  # best_freq included
        assert got[e]["best_freq"] in fs[e]


def test_cost_terms(lib):
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    terms = tfeat.TERMS
    ctxs = [lib.Context(lib.config_with_env_params(product_cfg(cases[e]), p[e])) for e in range(E)]
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        want = tfeat.single_steps(lib, cases, seeds, counters, terms=terms, ctxs=ctxs)
        b.set_cost_terms(terms["r_force"], terms["w_smooth"], terms["w_cone"])
        b.set_env_params(p)
        got = tfeat.batch_step(b, cases, seeds, counters)
    finally:
        b.close()
        for c in ctxs:
            c.close()
    for e in range(E):
        tfeat.assert_same(got[e], want[e], f"env {e}")


def params_tensor(p, as_float=True):
    a = np.ascontiguousarray(p)
    if as_float:
        return torch.from_numpy(a.view(np.float32).reshape(len(p), -1).copy()).cuda()
    return torch.from_numpy(a.view(np.uint8).reshape(len(p), -1).copy()).cuda()


def test_host_step_equals_device_step(lib):
    E = 3
    cases = env_cases(E, N=700, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = tdev.default_keys(E)
    arr = tdev.arrays_of(cases)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_env_params(p)
        want = tdev.host_step(b, arr, seeds, counters)
        got = tdev.device_step(b, arr, seeds, counters)
    finally:
        b.close()
    tdev.assert_same(got, want, "device step")
    assert (want["status"] == 0).all()


def test_device_setter_equals_host_setter(lib):
    E = 4
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p, p2 = env_params(lib, cases), env_params(lib, cases, shift=2)
    seeds, counters = tdev.default_keys(E)
    arr = tdev.arrays_of(cases)
    cfg = product_cfg(cases[0])
    hb, db = lib.BatchContext(cfg, E), lib.BatchContext(cfg, E)
    try:
        # every environment, from a float32 tensor
        hb.set_env_params(p)
        rejected = torch.full((E,), 7, dtype=torch.int32, device="cuda")
        db.set_env_params_device(params_tensor(p), rejected=rejected)
        assert db.get_env_params().tobytes() == p.tobytes()
        assert rejected.cpu().tolist() == [0] * E
        want = tdev.host_step(hb, arr, seeds, counters)
        tdev.assert_same(tdev.device_step(db, arr, seeds, counters), want, "device-set, device step")
        tdev.assert_same(tdev.host_step(db, arr, seeds, counters), want, "device-set, host step")
        # masked, from a uint8 tensor: environments 1 and 3 re-drawn, 0 and 2 keep theirs; their rows of the tensor
        # are NaN and must not be read; environment 3's record is invalid (grf_max < grf_min) and is rejected
        mask = np.array([0, 1, 0, 1], np.int32)
        bad = p2.copy()
        bad["grf_max"][3] = 1.0
        bad["grf_min"][3] = 2.0
        poisoned = bad.copy()
        poisoned.view(np.float32).reshape(E, -1)[[0, 2]] = np.nan
        expect = p.copy()
        expect[1] = p2[1]
        hb.set_env_params(expect)
        db.set_env_params_device(params_tensor(poisoned, as_float=False), mask=torch.from_numpy(mask).cuda(),
                                 rejected=rejected)
        assert rejected.cpu().tolist() == [0, 0, 0, 1]
        assert db.get_env_params().tobytes() == expect.tobytes()
        want = tdev.host_step(hb, arr, seeds, counters)
        tdev.assert_same(tdev.device_step(db, arr, seeds, counters), want, "masked device-set")
        assert expect[1].tobytes() != p[1].tobytes() and expect[3].tobytes() == p[3].tobytes()
    finally:
        hb.close()
        db.close()


def test_device_setter_on_one_stream_step_on_another(lib):
    """The device setter joins the device calls' event protocol: a step on another stream follows the setter's
    launch, and a setter on another stream follows the previous step's reads of the records.  Expected values: the
    same calls on one stream, on another batch."""
    E = 3
    cases = env_cases(E, N=64, method="mppi", par="zero_order", H=12)
    tp, tp2 = params_tensor(env_params(lib, cases)), params_tensor(env_params(lib, cases, shift=2))
    seeds, counters = tdev.default_keys(E)
    arr = tdev.arrays_of(cases)
    cfg = product_cfg(cases[0])
    one, two = lib.BatchContext(cfg, E), lib.BatchContext(cfg, E)
    try:
        one.set_env_params_device(tp)
        want = tdev.device_step(one, arr, seeds, counters)
        one.set_env_params_device(tp2)
        want2 = tdev.device_step(one, arr, seeds, counters)
        assert want["costs"].tobytes() != want2["costs"].tobytes()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        two.set_env_params_device(tp, stream=s1)
        tdev.assert_same(tdev.device_step(two, arr, seeds, counters, stream=s2), want, "set on s1, step on s2")
        # and back, nothing synchronised in between: the step on s2 reads the first records, the setter on s1 follows
        # those reads, and the next step on s2 follows the setter
        best = tdev.dev(arr["best"])
        ins = [tdev.dev(arr[k]) for k in ("states", "refs", "contacts")]
        keys = [tdev.dev(seeds, torch.int64), tdev.dev(counters, torch.int64)]
        torch.cuda.synchronize()
        with torch.cuda.stream(s2):
            torch.cuda._sleep(50_000_000)  # holds the step back, so an unordered setter would overtake it
        out = two.step_device(*ins, best, *keys, want_costs=True, stream=s2)
        two.set_env_params_device(tp2, stream=s1)
        got2 = tdev.device_step(two, arr, seeds, counters, stream=s2)
        tdev.assert_same(tdev.to_host(out, best), want, "step on s2, then set on s1")
        tdev.assert_same(got2, want2, "set on s1, then step on s2")
    finally:
        one.close()
        two.close()


def test_device_setter_argument_checks(lib):
    E = 2
    cases = env_cases(E, N=64, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        good = params_tensor(p)
        with pytest.raises(ValueError, match="params must be on"):
            b.set_env_params_device(good.cpu())
        with pytest.raises(ValueError, match="torch.uint8 or torch.float32"):
            b.set_env_params_device(good.double())
        with pytest.raises(ValueError, match="params must be"):
            b.set_env_params_device(good[:, :38].contiguous())
        with pytest.raises(ValueError, match="mask must be"):
            b.set_env_params_device(good, mask=torch.zeros(E, dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError, match="rejected must be"):
            b.set_env_params_device(good, rejected=torch.zeros(E + 1, dtype=torch.int32, device="cuda"))
        # the C call refuses a pointer that is not 4-byte aligned, before anything is enqueued
        raw = torch.zeros(E * 156 + 8, dtype=torch.uint8, device="cuda")
        rc = lib.lib.srbd_batch_set_env_params_device(b.h, raw.data_ptr() + 1, None, None, None)
        assert rc == lib.E_INVALID and b"4-byte aligned" in lib.lib.srbd_batch_last_error(b.h)
        assert b.get_env_params().tobytes() == lib.make_env_params(E, b.cfg).tobytes()  # nothing was set
    finally:
        b.close()


def test_oracle_parity_injected_noise(lib):
    """Not only self-consistency: each environment against the numpy oracle of its own robot and Q."""
    E = 3
    cases = env_cases(E, N=700, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    w = cases[0]["w"]
    for e in range(E):
        orc = SamplingMPCOracle(mass=float(p["mass"][e]), inertia=p["inertia"][e].reshape(3, 3), horizon=w.horizon,
                                num_samples=w.num_samples, method=w.method, parametrization=w.parametrization,
                                num_splines=w.num_splines, mu=float(p["mu"][e]), grf_min=float(p["grf_min"][e]),
                                grf_max=float(p["grf_max"][e]))
        orc.Q = np.array(p["q_diag"][e], f32)
        cases[e] = dict(cases[e], orc=orc)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_env_params(p)
        got = batch_step(b, cases, [42] * E, [1] * E, noise=True)
    finally:
        b.close()
    for e in range(E):
        check_end_to_end(cases[e], got[e])
        check_reduction(cases[e], got[e])


@pytest.mark.parametrize("poison", ["singular_inertia", "nan_mass"])
def test_isolation(lib, poison):
    """A singular inertia or a NaN mass in environment 1 changes no byte of environments 0 and 2."""
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    bad = p.copy()
    if poison == "singular_inertia":
        bad["inertia"][1] = 0.0
    else:
        bad["mass"][1] = np.nan
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        b.set_env_params(p)
        sane = batch_step(b, cases, seeds, counters)
        b.set_env_params(bad)
        got = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in (0, 2):
        assert_same(got[e], sane[e], f"env {e}")
    assert got[1]["costs"].tobytes() != sane[1]["costs"].tobytes()
    want = single_steps(lib, cases, p, seeds, counters)  # and the sane batch is the contexts' step
    for e in range(E):
        assert_same(sane[e], want[e], f"env {e}")


def test_clear_returns_to_the_shared_robot(lib):
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    cfg = product_cfg(cases[0])
    fresh, b = lib.BatchContext(cfg, E), lib.BatchContext(cfg, E)
    try:
        want = batch_step(fresh, cases, seeds, counters)
        b.set_env_params(p)
        with_params = batch_step(b, cases, seeds, counters)
        b.clear_env_params()
        got = batch_step(b, cases, seeds, counters)
        assert b.get_env_params().tobytes() == lib.make_env_params(E, cfg).tobytes()
    finally:
        fresh.close()
        b.close()
    for e in range(E):
        assert_same(got[e], want[e], f"env {e}")
    assert_same(with_params[0], want[0], "env 0 keeps the configuration's robot")
    assert not np.array_equal(with_params[1]["costs"], want[1]["costs"])


def test_refusals_change_nothing(lib):
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    p = env_params(lib, cases)
    seeds, counters = keys_of(E)
    b = lib.BatchContext(product_cfg(cases[0]), E)
    try:
        assert lib.lib.srbd_batch_set_env_params(b.h, None, None) == lib.E_INVALID
        assert lib.lib.srbd_batch_set_env_params_device(b.h, None, None, None, None) == lib.E_INVALID
        assert lib.lib.srbd_batch_get_env_params(b.h, None) == lib.E_INVALID
        b.set_env_params(p)
        before = batch_step(b, cases, seeds, counters)
        for field, value in (("grf_max", -1.0), ("mu", -0.1), ("grf_min", np.nan)):
            bad = env_params(lib, cases, shift=1)
            bad[field][2] = value
            with pytest.raises(RuntimeError, match="environment 2"):
                b.set_env_params(bad)
        masked_out = env_params(lib, cases, shift=1)
        masked_out["mu"][2] = -1.0
        b.set_env_params(masked_out, mask=[False, False, False])  # an unselected record is not checked
        assert b.get_env_params().tobytes() == p.tobytes()
        after = batch_step(b, cases, seeds, counters)
    finally:
        b.close()
    for e in range(E):
        assert_same(after[e], before[e], f"env {e}")


def test_controller_class(lib):
    """Batched_Sampling_MPC.set_robot_parameters followed by compute_control_device equals the _lib path."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC

    E = 2
    mpc = Batched_Sampling_MPC(E)
    cases = env_cases(E, N=mpc.num_parallel_computations, method=mpc.sampling_method, par=mpc.control_parametrization,
                      H=mpc.horizon)
    masses, mus = [9.5, 17.25], [0.4, 0.9]
    arr = tdev.arrays_of(cases)
    if mpc.rng == "philox":  # (seed, counter) per environment
        seeds, counters = tdev.default_keys(E)
        keys = np.stack([seeds, counters], axis=1)
    else:  # the JAX streams: the packed keys; the controller's call count numbers the step
        keys = seeds = np.array([lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)], np.uint64)
        counters = np.full(E, 1, np.uint64)
    try:
        cfg = mpc.context.cfg
        mpc.set_robot_parameters(mass=masses, mu=mus)
        p = lib.make_env_params(E, cfg, mass=masses, mu=mus)
        assert mpc.context.get_env_params().tobytes() == p.tobytes()
        b = lib.BatchContext(cfg, E)
        try:
            if mpc.rng != "philox":
                b.set_rng(mpc.rng)
            b.set_env_params(p)
            want = tdev.host_step(b, arr, seeds, counters)
        finally:
            b.close()
        best = tdev.dev(arr["best"])
        out = mpc.compute_control_device(tdev.dev(arr["states"]), tdev.dev(arr["refs"]), tdev.dev(arr["contacts"]),
                                         best, tdev.dev(keys, torch.int64))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out[0].cpu().numpy(), want["grf"])
        np.testing.assert_array_equal(out[2].cpu().numpy(), want["predicted_state"])
        np.testing.assert_array_equal(out[3].cpu().numpy(), want["best"])
        np.testing.assert_array_equal(out[4].cpu().numpy(), want["best_cost"])
        mpc.clear_robot_parameters()
        assert mpc.context.get_env_params().tobytes() == lib.make_env_params(E, cfg).tobytes()
    finally:
        mpc.close()
