"""The batch's device-resident step (srbd_batch_step_device, BatchContext.step_device) against the host path
(srbd_batch_step, BatchContext.step) on a second BatchContext of the same configuration given the same inputs.  The
contract is bit equality of every output array -- best parameters, GRFs, predicted states, best cost / index /
frequency, status and the per-sample costs -- so every comparison is exact (NaNs by their bytes).  Expected values
never come from the device path itself."""
import numpy as np
import pytest
import torch

from helpers import f32, make_case, product_cfg
from oracle.srbd_ga_oracle import GA_DUTY, freq_set

pytestmark = pytest.mark.gpu

AVAIL = (1.4, 2.0, 2.4)
TIMINGS = [(0.1, 0.6, 0.6, 0.1), (0.0, 0.5, 0.5, 0.0), (0.64, 0.99, 1.0, 0.3)]  # tests/test_gpu_ga.py
TERMS = {"r_force": (0.1, 0.1, 0.001), "w_smooth": 0.01, "w_cone": 5.0}  # tests/test_gpu_cost_terms.py
PGG_DT = 0.02
FIELDS = ("best", "grf", "predicted_state", "best_cost", "best_index", "best_freq", "status", "costs")


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


def default_keys(E):
    return np.array([100 + e for e in range(E)], np.uint64), np.array([7 + 2 * e for e in range(E)], np.uint64)


def arrays_of(cases, noise=False):
    return dict(states=stack(cases, "state"), refs=stack(cases, "ref"), contacts=stack(cases, "contact"),
                best=stack(cases, "best"), noise=stack(cases, "noise") if noise else None)


def dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:  # the keys: reinterpreted, as the library reinterprets them back
        assert dtype == torch.int64
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def host_step(b, arr, seeds, counters):
    """The expected values: BatchContext.step, every field as an array over the environments."""
    best, res, costs = b.step(arr["states"], arr["refs"], arr["contacts"], arr["best"], noise=arr["noise"],
                              seeds=seeds, counters=counters, want_costs=True)
    return dict(best=best, grf=np.array([r.grf[:] for r in res], f32),
                predicted_state=np.array([r.predicted_state[:] for r in res], f32),
                best_cost=np.array([r.best_cost for r in res], f32),
                best_index=np.array([r.best_index for r in res], np.int32),
                best_freq=np.array([r.best_freq for r in res], f32),
                status=np.array([r.status for r in res], np.int32), costs=costs)


def device_step(b, arr, seeds, counters, contact_stride=None, stream=None):
    """One device step from host arrays: uploaded, stepped, synchronised and read back."""
    contacts = arr["contacts"]
    if contact_stride is not None:  # the columns past H are never read: fill them with something that would show
        pad = np.full(contacts.shape[:2] + (contact_stride,), 7.0, f32)
        pad[:, :, :contacts.shape[2]] = contacts
        contacts = pad
    best = dev(arr["best"])
    out = b.step_device(dev(arr["states"]), dev(arr["refs"]), dev(contacts), best, dev(seeds, torch.int64),
                        dev(counters, torch.int64), noise=None if arr["noise"] is None else dev(arr["noise"]),
                        want_costs=True, stream=stream)
    torch.cuda.synchronize()
    return to_host(out, best)


def to_host(out, best):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["best"] = best.cpu().numpy()
    return got


def assert_same(got, want, what=""):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{what} {k}"
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
        assert got[k].tobytes() == want[k].tobytes(), f"{what} {k}"


def run_pair(lib, cases, *, cfg=None, rng=None, seeds=None, counters=None, noise=False, contact_stride=None,
             setup=None, arr=None):
    """One device step on one context against one host step on another; returns (device, host) results."""
    E = len(cases)
    s0, c0 = default_keys(E)
    seeds = s0 if seeds is None else seeds
    counters = c0 if counters is None else counters
    cfg = product_cfg(cases[0]) if cfg is None else cfg
    arr = arrays_of(cases, noise) if arr is None else arr
    bh, bd = lib.BatchContext(cfg, E), lib.BatchContext(cfg, E)
    try:
        for b in (bh, bd):
            if rng:
                b.set_rng(rng)
            if setup:
                setup(b)
        want = host_step(bh, arr, seeds, counters)
        got = device_step(bd, arr, seeds, counters, contact_stride)
        assert_same(got, want)
        # srbd_batch_copy_costs after a device step: that step's costs
        np.testing.assert_array_equal(bd.copy_costs(), want["costs"])
    finally:
        bh.close()
        bd.close()
    assert np.all(want["status"] == 0)
    return got, want


# the smallest shape that still reaches the part named beside it
SHAPES = [
    ("zo_h12_n1", 3, dict(N=1, method="mppi", par="zero_order", H=12)),      # a single row
    ("zo_h12_n65", 3, dict(N=65, method="mppi", par="zero_order", H=12)),    # a second leaf of one row
    ("zo_h12_n257", 3, dict(N=257, method="mppi", par="zero_order", H=12)),  # one level above the leaves
    ("zo_h8_n130", 3, dict(N=130, method="mppi", par="zero_order", H=8)),    # the generic, non-specialised shape
    ("lin_s2_h12_n700", 3, dict(N=700, method="mppi", par="linear_spline", H=12, S=2)),
    ("cub_s2_h16_n700", 3, dict(N=700, method="mppi", par="cubic_spline", H=16, S=2)),
    ("zo_h10_n257_rs", 3, dict(N=257, method="random_sampling", par="zero_order", H=10)),  # the key reduction
    ("zo_h12_n257_e1", 1, dict(N=257, method="mppi", par="zero_order", H=12)),  # one environment
]


@pytest.mark.parametrize("name,E,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_device_step_bit_equal_device_draws(lib, name, E, kw):
    got, _ = run_pair(lib, env_cases(E, **kw))
    if E > 1 and kw["N"] >= 65:  # the environments drew different rows
        assert not np.array_equal(got["costs"][0], got["costs"][1])


def test_device_step_bit_equal_jax_stream(lib):
    E = 3
    seeds = np.array([lib.pack_key(lib.jax_split(lib.jax_prng_key(e))[0]) for e in range(E)], np.uint64)
    run_pair(lib, env_cases(E, N=257, method="mppi", par="zero_order", H=12), rng="jax", seeds=seeds)


def test_device_step_bit_equal_injected_noise_and_wider_contact_stride(lib):
    """The transpose reads the caller's noise in place; contacts come with 20 columns per leg, 12 of them used."""
    cases = env_cases(3, N=130, method="mppi", par="zero_order", H=12)
    assert cases[0]["contact"].shape == (4, 12)
    run_pair(lib, cases, noise=True, contact_stride=20)


def test_device_step_takes_arrays_that_are_not_16_byte_aligned(lib):
    """states, refs and best as contiguous views one float into a larger allocation: the kernels' dword path."""
    E = 3
    cases = env_cases(E, N=130, method="mppi", par="zero_order", H=12)
    arr = arrays_of(cases)
    seeds, counters = default_keys(E)

    def shifted(a):
        flat = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        v = flat[1:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    bh, bd = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        want = host_step(bh, arr, seeds, counters)
        best = shifted(arr["best"])
        out = bd.step_device(shifted(arr["states"]), shifted(arr["refs"]), dev(arr["contacts"]), best,
                             dev(seeds, torch.int64), dev(counters, torch.int64), want_costs=True)
        torch.cuda.synchronize()
        assert_same(to_host(out, best), want)
    finally:
        bh.close()
        bd.close()


# ------------------------------------------------------------------ values the pack kernel must reproduce
def test_nan_state_and_all_swing_contacts_stay_in_their_environment(lib):
    """Environment 0 has a NaN state, environment 1 never touches the ground (fzref = mg / 0 = inf), environment 2 is
    ordinary: every output equals the host path's, and environment 2 returns what it returns beside ordinary ones."""
    kw = dict(N=257, method="mppi", par="zero_order", H=12)
    cases = env_cases(3, **kw)
    plain, _ = run_pair(lib, cases)
    odd = [dict(c) for c in cases]
    odd[0]["state"] = cases[0]["state"].copy()
    odd[0]["state"][4] = np.nan
    odd[1]["contact"] = np.zeros_like(cases[1]["contact"])
    got, want = run_pair(lib, odd)
    assert np.all(want["costs"][0] == f32(1000000.0)) and np.isnan(want["predicted_state"][0]).any()
    for k in FIELDS:
        assert got[k][2].tobytes() == plain[k][2].tobytes(), k


def foot_cost(state, ref, q, fused):
    """fill_input's cost_feet in strict float32, or as a compiler contracting a * b + c to FMA would form it: the
    outer product and the add in float64 (exact product, one rounding of the sum), then rounded once."""
    cf = f32(0)
    for i in range(12):
        e = f32(state[12 + i] - ref[12 + i])
        t = f32(e * q[i])
        cf = f32(np.float64(t) * np.float64(e) + np.float64(cf)) if fused else f32(cf + f32(t * e))
    return cf


def test_foot_cost_sum_is_unfused(lib):
    """Non-zero foot weights and random foot errors: cost_feet enters every sample's cost as the last add, so a pack
    kernel that contracted the sum to FMA would change the costs.  The seed is chosen (on the CPU) so that the strict
    and the contracted sums differ for an environment, and the test shows that this difference reaches the costs."""
    E, kw = 3, dict(N=257, method="mppi", par="zero_order", H=12)
    cases = env_cases(E, **kw)
    rng = np.random.default_rng(1)
    q = rng.uniform(1e3, 1e5, 12).astype(f32)
    err = rng.uniform(-0.4, 0.4, (E, 12)).astype(f32)
    for e, c in enumerate(cases):  # the reference's feet enter nothing but cost_feet: the rollouts are the plain case's
        c["ref"] = c["ref"].copy()
        c["ref"][12:] = c["state"][12:] + err[e]
    strict = np.array([foot_cost(c["state"], c["ref"], q, False) for c in cases], f32)
    fused = np.array([foot_cost(c["state"], c["ref"], q, True) for c in cases], f32)
    differ = np.flatnonzero(strict != fused)
    assert differ.size >= 1, "the seed must give a case that detects a contraction"
    # the costs without the foot term (weights 0: cost + 0), from the host path
    _, bare = run_pair(lib, cases)
    cfg = product_cfg(cases[0])
    for i in range(12):
        cfg.q_diag[12 + i] = float(q[i])
    got, want = run_pair(lib, cases, cfg=cfg)
    for e in range(E):  # the emulation is the host's sum
        np.testing.assert_array_equal(want["costs"][e], (bare["costs"][e] + strict[e]).astype(f32))
    e = int(differ[0])
    assert np.any((bare["costs"][e] + fused[e]).astype(f32) != want["costs"][e])
    assert_same(got, want)


# ------------------------------------------------------------------ gait-adaptive sampling, cost terms
def timings_of(E, shift=0.0):
    t = np.array([TIMINGS[e % len(TIMINGS)] for e in range(E)], f32)
    return ((t + f32(shift)) % f32(1.0)).astype(f32)


def sets_of(cases, E):
    method = cases[0]["orc"].method
    return np.stack([freq_set(method, AVAIL, 1.65, 1) for _ in range(E)]).astype(f32)


@pytest.mark.parametrize("injected", [False, True], ids=["device_draws", "injected_rows"])
def test_gait_adaptive_device_steps_follow_set_gait(lib, injected):
    """The device step is the first step after set_gait (the gait fields reach the device without a host step), and
    a second set_gait between two device steps holds for the second: best_freq and everything else equal the host
    path's, which receives the same two settings."""
    E, N = 3, 257
    cases = env_cases(E, N=N, method="mppi", par="zero_order", H=12)
    fs = sets_of(cases, E)
    seeds, counters = default_keys(E)
    arr = arrays_of(cases, noise=injected)
    bh, bd = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        for it in range(2):
            t = timings_of(E, 0.21 * it)
            rows = None
            if injected:
                rows = np.stack([np.random.default_rng(50 + e + 10 * it).choice(fs[e], N)
                                 for e in range(E)]).astype(f32)
            bh.set_gait(t, PGG_DT, GA_DUTY, fs, rows)
            bd.set_gait(t, PGG_DT, GA_DUTY, fs, rows)
            want = host_step(bh, arr, seeds, counters + np.uint64(it))
            got = device_step(bd, arr, seeds, counters + np.uint64(it))
            assert_same(got, want, f"step {it}")
            assert np.all(np.isin(want["best_freq"], fs)) and np.all(want["best_freq"] != 0)
            arr = dict(arr, best=want["best"])
    finally:
        bh.close()
        bd.close()


def test_cost_terms_device_step(lib):
    cases = env_cases(3, N=257, method="mppi", par="zero_order", H=12)
    plain, _ = run_pair(lib, cases)
    got, _ = run_pair(lib, cases,
                      setup=lambda b: b.set_cost_terms(TERMS["r_force"], TERMS["w_smooth"], TERMS["w_cone"]))
    assert np.mean(got["costs"] > plain["costs"]) > 0.9  # the terms are in the cost


# ------------------------------------------------------------------ streams and closed loops
def closed_loop(lib, stream):
    """Three steps with best on the device, the counters advanced by a torch op and no synchronisation in between,
    against three host steps fed back through host arrays."""
    E, steps = 3, 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    arr = arrays_of(cases)
    seeds, counters = default_keys(E)
    bh, bd = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        want, hb = [], arr["best"]
        for it in range(steps):
            want.append(host_step(bh, dict(arr, best=hb), seeds, counters + np.uint64(it)))
            hb = want[-1]["best"]
        # uploads on the default stream, complete before the loop's stream starts
        up = {k: dev(arr[k]) for k in ("states", "refs", "contacts", "best")}
        d_seeds, d_ctr = dev(seeds, torch.int64), dev(counters, torch.int64)
        torch.cuda.synchronize()
        outs, bests, sums = [], [], []
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            best = up["best"].clone()
            for it in range(steps):
                # the inputs are produced by torch ops on this stream right before the call ...
                states, refs = up["states"] + 0.0, up["refs"] * 1.0
                out = bd.step_device(states, refs, up["contacts"], best, d_seeds, d_ctr, want_costs=True,
                                     stream=stream)
                # ... and the outputs consumed by torch ops on it right after
                sums.append(out["grf"].sum(dim=1))
                bests.append(best.clone())
                outs.append(out)
                d_ctr = d_ctr + 1
        (stream if stream is not None else torch.cuda.current_stream()).synchronize()
        for it in range(steps):
            assert_same(to_host(outs[it], bests[it]), want[it], f"step {it}")
            np.testing.assert_array_equal(sums[it].cpu().numpy(),
                                          torch.from_numpy(want[it]["grf"]).cuda().sum(dim=1).cpu().numpy())
    finally:
        bh.close()
        bd.close()


def test_closed_loop_three_steps_without_synchronisation(lib):
    closed_loop(lib, None)


def test_closed_loop_on_a_side_stream(lib):
    closed_loop(lib, torch.cuda.Stream())


def test_device_and_host_steps_interleave_on_one_context(lib):
    """Device step, host step, device step on one context (the internal buffers are shared; the device steps run on
    torch's stream, the host step on the batch's own): each equals its counterpart on a host-only context."""
    E = 3
    cases = env_cases(E, N=257, method="mppi", par="zero_order", H=12)
    arr = arrays_of(cases)
    seeds, counters = default_keys(E)
    bh, bd = lib.BatchContext(product_cfg(cases[0]), E), lib.BatchContext(product_cfg(cases[0]), E)
    try:
        best = arr["best"]
        for it, kind in enumerate(("device", "host", "device")):
            a, c = dict(arr, best=best), counters + np.uint64(it)
            want = host_step(bh, a, seeds, c)
            if kind == "host":
                got = host_step(bd, a, seeds, c)
            else:
                best_t = dev(a["best"])
                out = bd.step_device(dev(a["states"]), dev(a["refs"]), dev(a["contacts"]), best_t,
                                     dev(seeds, torch.int64), dev(c, torch.int64), want_costs=True)
                if it == 0:  # the host step that follows waits for this one by itself
                    nxt = dict(arr, best=want["best"])
                    want2 = host_step(bh, nxt, seeds, counters + np.uint64(1))
                    got2 = host_step(bd, nxt, seeds, counters + np.uint64(1))
                    assert_same(got2, want2, "host step right behind a device step")
                torch.cuda.synchronize()
                got = to_host(out, best_t)
            assert_same(got, want, f"step {it} ({kind})")
            best = want["best"]
    finally:
        bh.close()
        bd.close()


def test_contact_stride_below_horizon_is_refused(lib):
    import ctypes as C

    cases = env_cases(1, N=65, method="mppi", par="zero_order", H=12)
    b = lib.BatchContext(product_cfg(cases[0]), 1)
    try:
        io = lib.BatchDeviceIO()
        for name, _ in lib.BatchDeviceIO._fields_:
            if name not in ("contact_stride", "pad", "noise", "costs"):
                setattr(io, name, 0x1000)  # never followed: the call returns before anything is enqueued
        io.contact_stride = 11
        assert lib.lib.srbd_batch_step_device(b.h, C.byref(io), None) == lib.E_INVALID
        assert b"contact_stride" in lib.lib.srbd_batch_last_error(b.h)
    finally:
        b.close()


# ------------------------------------------------------------------ controller class
def test_controller_compute_control_device(lib):
    """Batched_Sampling_MPC.compute_control_device against compute_control of a second controller, two rounds with
    the returned parameters fed back (on the device, and through host arrays)."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC

    E = 2
    on_dev, on_host = Batched_Sampling_MPC(E), Batched_Sampling_MPC(E)
    cases = env_cases(E, N=on_dev.num_parallel_computations, method=on_dev.sampling_method,
                      par=on_dev.control_parametrization, H=on_dev.horizon)
    arr = arrays_of(cases)
    try:
        best_t, hb = dev(arr["best"]), arr["best"]
        states, refs, contacts = dev(arr["states"]), dev(arr["refs"]), dev(arr["contacts"])
        for it in range(2):
            on_host.with_newkey()
            keys = np.array(on_host.get_key())
            ref = on_host.compute_control(arr["states"], arr["refs"], arr["contacts"], hb, keys)
            if on_dev.rng == "philox":  # (seed, counter) per environment
                d_keys = dev(keys.astype(np.uint64), torch.int64)
            else:  # the JAX streams: the packed keys, split on the host
                d_keys = dev(np.array([lib.pack_key(k) for k in keys], np.uint64), torch.int64)
            out = on_dev.compute_control_device(states, refs, contacts, best_t, d_keys)
            torch.cuda.synchronize()
            assert out[3] is best_t
            for i in (0, 1, 2, 3, 4):  # GRFs, footholds, predicted states, best parameters, best costs
                np.testing.assert_array_equal(out[i].cpu().numpy(), np.asarray(ref[i]), err_msg=f"round {it} item {i}")
            np.testing.assert_array_equal(out[5].cpu().numpy(), np.asarray(ref[5]))
            np.testing.assert_array_equal(np.asarray(out[6]), np.asarray(ref[6]))
            hb = ref[3]
    finally:
        on_dev.close()
        on_host.close()
