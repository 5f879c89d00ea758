"""GPU: the batch's controller-interface step (srbd_batch_interface_step_device, include/srbd_mpc.h) against E single
contexts, each running the host srbd_interface_step on the same inputs: every output array, best_params, sigma, keys,
previous_contact, states / refs and the float64 masked GRFs byte for byte, over 12 consecutive steps of a trot whose
lift-offs and touch-downs fall inside them.  The gait-adaptive form, the per-environment parameters and the cost terms
are pinned to the chain of existing device calls with the keys advanced on the host.  Expected values never come from
the call under test."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

from helpers import f32, make_case, product_cfg

pytestmark = pytest.mark.gpu

STEPS = 12
STEP_DT = 0.04       # 12 steps cover 0.67 of the 1.4 Hz trot's period: every leg lifts off or touches down inside
SIGMA_RESET = 3.0
TERMS = {"r_force": (0.1, 0.1, 0.001), "w_smooth": 0.01, "w_cone": 5.0}  # tests/test_gpu_cost_terms.py
OUT_KEYS = ("states", "refs", "grf", "footholds", "grf_raw", "predicted_state", "best_cost", "best_index", "status",
            "costs")
STATE_KEYS = ("keys", "previous_contact", "best", "sigma")
FEET = np.array([[0.19, 0.14, 0.0], [0.19, -0.14, 0.0], [-0.19, 0.14, 0.0], [-0.19, -0.14, 0.0]])


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def dev(a, dtype=None):
    """A numpy array on the device; uint64 keys travel as their int64 bit patterns."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    t = torch.from_numpy(a).cuda()
    assert dtype is None or t.dtype == dtype
    return t


def case_of(N=192, method="mppi", par="zero_order", H=12, S=2):
    return make_case("c2", N=N, method=method, par=par, H=H, S=S)


# ------------------------------------------------------------------ inputs (all formed on the CPU)
def contact_steps(E, H, steps=STEPS):
    """(steps, E, 4, H) float32 from the host gait generator: a trot, environment e shifted by e steps of 7 ms."""
    from quadruped_pympc_amd.helpers.periodic_gait_generator import PeriodicGaitGenerator

    out = np.zeros((steps, E, 4, H), f32)
    dts, lens = np.array([0.02]), np.array([H])
    for e in range(E):
        pgg = PeriodicGaitGenerator(0.65, 1.4, 0, H)
        for _ in range(40 + (e % 16)):  # past the start-up hold
            pgg.run(0.007, pgg.step_freq)
        for k in range(steps):
            pgg.run(STEP_DT, pgg.step_freq)
            out[k, e] = np.asarray(pgg.compute_contact_sequence(dts, lens))[:, :H]
    return out


def assert_contact_coverage(contacts):
    """A condition on the inputs: some environment lifts a leg off (previous 1, current 0) and one touches down."""
    cur = contacts[:, :, :, 0]
    prev = np.concatenate([np.ones_like(cur[:1]), cur[:-1]])
    assert np.any((prev == 1) & (cur == 0)), "no lift-off inside the steps"
    assert np.any((prev == 0) & (cur == 1)), "no touch-down inside the steps"


def state_steps(E, steps=STEPS):
    """(steps, E, 24) float64 state_in and ref_in, srbd_prepare_state's layouts."""
    rng = np.random.default_rng(11)
    st = np.zeros((steps, E, 24))
    rf = np.zeros((steps, E, 24))
    st[:, :, 0:3] = np.array([0.0, 0.0, 0.3]) + 0.01 * rng.standard_normal((steps, E, 3))
    st[:, :, 3:6] = 0.1 * rng.standard_normal((steps, E, 3))
    st[:, :, 6:9] = 0.05 * rng.standard_normal((steps, E, 3))
    st[:, :, 9:12] = 0.1 * rng.standard_normal((steps, E, 3))
    st[:, :, 12:] = FEET.reshape(12) + 0.01 * rng.standard_normal((steps, E, 12))
    rf[:, :, 0:3] = [0.0, 0.0, 0.3]
    rf[:, :, 3:6] = [0.4, 0.0, 0.0]
    rf[:, :, 12:] = (FEET + [0.05, 0.0, 0.0]).reshape(12) + 0.01 * rng.standard_normal((steps, E, 12))
    return st, rf


def initial_keys(lib, E, rng):
    if rng == "philox":
        return np.array([[100 + e, 7 + 2 * e] for e in range(E)], np.uint64)
    return np.array([[lib.pack_key(lib.jax_prng_key(42 + e)), 3 * e] for e in range(E)], np.uint64)


def initial_best(E, P):
    return (0.5 * np.random.default_rng(3).standard_normal((E, P))).astype(f32)


# ------------------------------------------------------------------ the yardstick: E x srbd_interface_step
class HostChain:
    """E single contexts and the state srbd_interface_step carries: keys, previous contact, warm start, sigma."""

    def __init__(self, lib, case, E, rng, keys, best, env_cfgs=None, terms=None):
        self.lib, self.E, self.rng = lib, E, rng
        self.H, self.cem = case["w"].horizon, case["w"].method == "cem_mppi"
        self.ctxs = []
        for e in range(E):
            ctx = lib.Context(product_cfg(case) if env_cfgs is None else env_cfgs[e])
            if rng != "philox":
                ctx.set_rng(rng)
            if terms:
                ctx.set_cost_terms(**terms)
            self.ctxs.append(ctx)
        self.P = self.ctxs[0].P
        self.keys = np.array(keys, np.uint64)
        self.prev = np.ones((E, 4))
        self.best = np.array(best, f32)
        self.sigma = np.full((E, self.P), np.nan, f32) if self.cem else None

    def close(self):
        for c in self.ctxs:
            c.close()

    def step(self, state_in, ref_in, contacts, iterations):
        lib, E, H = self.lib, self.E, self.H
        out = {k: [] for k in OUT_KEYS}
        for e in range(E):
            io = lib.InterfaceIO()
            np.ctypeslib.as_array(io.state_in)[:] = state_in[e]
            np.ctypeslib.as_array(io.ref_in)[:] = ref_in[e]
            np.ctypeslib.as_array(io.current_contact)[:] = contacts[e][:, 0]
            np.ctypeslib.as_array(io.previous_contact)[:] = self.prev[e]
            io.sigma_reset = SIGMA_RESET
            io.key[0], io.key[1] = int(self.keys[e, 0]), int(self.keys[e, 1])
            io.horizon, io.iterations, io.rng, io.cem = H, iterations, lib.RNG_CODES[self.rng], int(self.cem)
            cs = np.ascontiguousarray(contacts[e][:, :H], f32)
            res = lib.SrbdResult()
            rc = lib.lib.srbd_interface_step(self.ctxs[e].h, C.addressof(io), cs.ctypes.data, None, H,
                                             self.best[e].ctypes.data, self.P // 4,
                                             self.sigma[e].ctypes.data if self.cem else None, C.byref(res))
            assert rc == lib.OK, (rc, lib.last_error(self.ctxs[e].h))
            self.keys[e] = (io.key[0], io.key[1])
            self.prev[e] = contacts[e][:, 0]
            out["states"].append(np.array(io.state_out[:], np.float64).astype(f32))
            out["refs"].append(np.array(io.ref_out[:], np.float64).astype(f32))
            out["grf"].append(np.array(io.grf[:], np.float64))
            out["footholds"].append(np.array(ref_in[e][12:], np.float64))
            out["grf_raw"].append(np.array(res.grf[:], f32))
            out["predicted_state"].append(np.array(res.predicted_state[:], f32))
            out["best_cost"].append(f32(res.best_cost))
            out["best_index"].append(np.int32(res.best_index))
            out["status"].append(np.int32(res.status))
            out["costs"].append(self.ctxs[e].copy_costs())
        out = {k: np.stack(v) for k, v in out.items()}
        out.update(keys=self.keys.copy(), previous_contact=self.prev.astype(f32), best=self.best.copy(),
                   sigma=None if self.sigma is None else self.sigma.copy())
        return out


# ------------------------------------------------------------------ the call under test
class DeviceLoop:
    """One batch and the device tensors the call updates in place."""

    def __init__(self, lib, case, E, rng, keys, best, setup=None):
        self.lib, self.E = lib, E
        self.cem = case["w"].method == "cem_mppi"
        self.b = (lib.CemBatchContext if self.cem else lib.BatchContext)(product_cfg(case), E)
        if rng != "philox":
            self.b.set_rng(rng)
        if setup:
            setup(self.b)
        self.keys = dev(np.array(keys, np.uint64), torch.int64)
        self.prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
        self.best = dev(np.array(best, f32))
        self.sigma = torch.full((E, self.b.P), float("nan"), dtype=torch.float32, device="cuda") if self.cem else None

    def close(self):
        self.b.close()

    def enqueue(self, state_in, ref_in, contacts, iterations, gait_io=None, stream=None):
        return self.b.interface_step_device(state_in, ref_in, contacts, self.keys, self.prev, self.best,
                                            iterations=iterations, sigma=self.sigma,
                                            sigma_reset=SIGMA_RESET if self.cem else 0.0, gait_io=gait_io,
                                            want_costs=True, stream=stream)

    def collect(self, out):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got.update(keys=self.keys.cpu().numpy().view(np.uint64), previous_contact=self.prev.cpu().numpy(),
                   best=self.best.cpu().numpy(), sigma=None if self.sigma is None else self.sigma.cpu().numpy())
        return got

    def step(self, state_in, ref_in, contacts, iterations, gait_io=None):
        return self.collect(self.enqueue(dev(state_in), dev(ref_in), dev(contacts), iterations, gait_io))


def assert_same(got, want, what="", keys=OUT_KEYS + STATE_KEYS):
    for k in keys:
        if want.get(k) is None:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {k}: {g.dtype}{g.shape} / {w.dtype}{w.shape}"
        if g.tobytes() != w.tobytes():
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {k}")
            raise AssertionError(f"{what} {k}: equal values, different bytes")


def run_against_host(lib, E, method, rng, iterations, N=192, par="zero_order", H=12, S=2, steps=STEPS):
    case = case_of(N, method, par, H, S)
    contacts = contact_steps(E, H, steps)
    if steps == STEPS:
        assert_contact_coverage(contacts)
    st, rf = state_steps(E, steps)
    keys, best = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    host, loop = HostChain(lib, case, E, rng, keys, best), DeviceLoop(lib, case, E, rng, keys, best)
    try:
        for k in range(steps):
            want = host.step(st[k], rf[k], contacts[k], iterations)
            got = loop.step(st[k], rf[k], contacts[k], iterations)
            assert_same(got, want, f"step {k}")
            if method == "cem_mppi":
                assert np.isfinite(got["sigma"]).all()
        assert np.all(got["status"] == 0)
    finally:
        host.close()
        loop.close()


@pytest.mark.parametrize("rng", ["philox", "jax", "jax_legacy"])
@pytest.mark.parametrize("method", ["random_sampling", "mppi", "cem_mppi"])
def test_methods_and_streams(lib, method, rng):
    run_against_host(lib, 3, method, rng, 2)


@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("method,rng", [("mppi", "philox"), ("cem_mppi", "jax")])
def test_iterations(lib, method, rng, iterations):
    run_against_host(lib, 3, method, rng, iterations)


@pytest.mark.parametrize("name,E,kw", [
    ("e1", 1, {}),
    ("e65", 65, {}),                                   # crosses a wave of the one-lane-per-(environment, leg) kernels
    ("n1000", 3, dict(N=1000)),                        # not a leaf multiple
    ("h5", 3, dict(H=5)),                              # the generic rollout
    ("cubic_s2", 3, dict(par="cubic_spline", S=2)),
    ("cem_e65", 65, dict(method="cem_mppi")),
], ids=lambda v: v if isinstance(v, str) else "")
def test_shapes(lib, name, E, kw):
    kw = dict(kw)
    run_against_host(lib, E, kw.pop("method", "mppi"), "philox", 2, **kw)


def test_cem_sigma_is_reset_at_iteration_0_only(lib):
    """iterations = 2 equals the host call with iterations 2, and differs from a chain that resets sigma before both
    iterations (two host calls of one iteration each: the same keys, prepare_state and steps, the other schedule)."""
    E, rng = 3, "philox"
    case = case_of(method="cem_mppi")
    contacts, (st, rf) = contact_steps(E, 12, 1), state_steps(E, 1)
    keys, best = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    right, wrong = HostChain(lib, case, E, rng, keys, best), HostChain(lib, case, E, rng, keys, best)
    loop = DeviceLoop(lib, case, E, rng, keys, best)
    try:
        want = right.step(st[0], rf[0], contacts[0], 2)
        wrong.step(st[0], rf[0], contacts[0], 1)
        other = wrong.step(st[0], rf[0], contacts[0], 1)
        got = loop.step(st[0], rf[0], contacts[0], 2)
        assert_same(got, want)
        np.testing.assert_array_equal(other["keys"], want["keys"])  # the same draws: only the schedule differs
        assert other["sigma"].tobytes() != got["sigma"].tobytes()
        assert other["best"].tobytes() != got["best"].tobytes()
    finally:
        right.close()
        wrong.close()
        loop.close()


# ------------------------------------------------------------------ against the chain of existing device calls
def advance_keys(keys, rng, iterations):
    """The key rule stated here, in Python integers, with oracle/jax_random_oracle.py's split -- not the library's
    schedule: Philox counter + 1; JAX key = split(key)[0], call count + 1 -> (keys, step keys (iterations, E, 2))."""
    from oracle import jax_random_oracle as jro

    E = keys.shape[0]
    out, steps = np.array(keys, np.uint64), np.zeros((iterations, E, 2), np.uint64)
    for e in range(E):
        k0, k1 = int(keys[e, 0]), int(keys[e, 1])
        for i in range(iterations):
            if rng != "philox":
                a = jro.split(np.array([k0 >> 32, k0 & 0xFFFFFFFF], np.uint32), 2, partitionable=rng == "jax")[0]
                k0 = (int(a[0]) << 32) | int(a[1])
            k1 = (k1 + 1) & 0xFFFFFFFFFFFFFFFF
            steps[i, e] = (k0, k1)
        out[e] = (k0, k1)
    return out, steps


def device_chain_step(lib, b, rng, st, rf, contacts, keys, prev, best, iterations, gait=None):
    """prepare_state_device (+ set_gait_device) + iterations x step_device with the keys advanced on the host + the
    mask in numpy: the existing entry points.  keys, prev (numpy) and best (tensor) are updated in place."""
    cur = np.ascontiguousarray(contacts[:, :, 0])
    states, refs = lib.prepare_state_device(dev(st), dev(rf), dev(cur), dev(prev), b.P // 4, best)
    if gait is not None:
        b.set_gait_device(**gait)
    new_keys, step_keys = advance_keys(keys, rng, iterations)
    for i in range(iterations):
        out = b.step_device(states, refs, dev(contacts), best, dev(step_keys[i, :, 0].copy(), torch.int64),
                            dev(step_keys[i, :, 1].copy(), torch.int64), want_costs=True)
    torch.cuda.synchronize()
    keys[...] = new_keys
    prev[...] = cur
    want = {k: v.cpu().numpy() for k, v in out.items()}
    want["grf_raw"] = want.pop("grf")
    want["grf"] = (want["grf_raw"].astype(np.float64).reshape(-1, 4, 3) * cur.astype(np.float64)[:, :, None]).reshape(-1, 12)
    want.update(states=states.cpu().numpy(), refs=refs.cpu().numpy(), footholds=np.array(rf[:, 12:]),
                keys=keys.copy(), previous_contact=prev.astype(f32), best=best.cpu().numpy(), sigma=None)
    return want


def run_against_device_chain(lib, method, rng, setup=None, with_gait=False, E=3, iterations=2):
    case = case_of(method=method)
    contacts = contact_steps(E, 12)
    assert_contact_coverage(contacts)
    st, rf = state_steps(E)
    keys0, best0 = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    loop = DeviceLoop(lib, case, E, rng, keys0, best0, setup)
    ref = lib.BatchContext(product_cfg(case), E)
    try:
        if rng != "philox":
            ref.set_rng(rng)
        if setup:
            setup(ref)
        keys, prev, best = np.array(keys0), np.ones((E, 4), f32), dev(best0)
        for k in range(STEPS):
            gait = gait_io = None
            if with_gait:
                g = np.random.default_rng(70 + k)
                gait = dict(optimize=dev(g.integers(0, 2, E).astype(np.int32)), available=[1.3, 1.4, 1.5],
                            pgg_dt=0.02, duty=0.65, timings=dev(g.uniform(0, 1, (E, 4)).astype(f32)),
                            nominal_freqs=dev(np.full(E, 1.4, f32)))
                gait_io = loop.b.make_gait_io(gait["optimize"], gait["available"], gait["pgg_dt"], gait["duty"],
                                              timings=gait["timings"], nominal_freqs=gait["nominal_freqs"])
            want = device_chain_step(lib, ref, rng, st[k], rf[k], contacts[k], keys, prev, best, iterations, gait)
            got = loop.step(st[k], rf[k], contacts[k], iterations, gait_io)
            assert_same(got, want, f"step {k}", keys=OUT_KEYS + STATE_KEYS + ("best_freq",))
            if with_gait:
                assert np.all(np.isin(got["best_freq"], f32([1.3, 1.4, 1.5])))
    finally:
        loop.close()
        ref.close()


@pytest.mark.parametrize("method,rng", [("mppi", "philox"), ("random_sampling", "jax")])
def test_gait_adaptive(lib, method, rng):
    run_against_device_chain(lib, method, rng, with_gait=True)


def test_per_environment_parameters(lib):
    def setup(b):
        b.set_env_params(lib.make_env_params(b.E, b.cfg, mass=[12.0, 15.0, 19.0], mu=[0.4, 0.5, 0.7]))

    run_against_device_chain(lib, "mppi", "philox", setup)


def test_cost_terms(lib):
    run_against_device_chain(lib, "mppi", "philox", lambda b: b.set_cost_terms(**TERMS))


def test_environments_are_independent(lib):
    """A NaN state in environment 1 of 3 changes no byte of environments 0 and 2; environment 1's keys and
    previous_contact still advance."""
    E, rng = 3, "philox"
    case = case_of()
    contacts, (st, rf) = contact_steps(E, 12, 2), state_steps(E, 2)
    keys, best = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    clean, dirty = DeviceLoop(lib, case, E, rng, keys, best), DeviceLoop(lib, case, E, rng, keys, best)
    try:
        bad = st.copy()
        bad[:, 1, :] = np.nan
        for k in range(2):
            a = clean.step(st[k], rf[k], contacts[k], 2)
            b = dirty.step(bad[k], rf[k], contacts[k], 2)
            for key in OUT_KEYS + ("keys", "previous_contact", "best"):
                assert a[key][[0, 2]].tobytes() == b[key][[0, 2]].tobytes(), f"step {k} {key}"
            np.testing.assert_array_equal(b["keys"][1], a["keys"][1])
            np.testing.assert_array_equal(b["previous_contact"][1], contacts[k][1][:, 0])
        assert np.isnan(b["states"][1]).any()
    finally:
        clean.close()
        dirty.close()


# ------------------------------------------------------------------ the raw call: poison, refusals
def raw_tensors(lib, b, E, rows, stride, cem, poison=True):
    """Every array of the call with `rows` >= E rows, NaN / 0xFF beyond E rows and beyond column H of contacts."""
    P, N = b.P, b.N

    def f(shape, dtype=torch.float32):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        if dtype in (torch.int32, torch.int64):
            t.fill_(-1)
        else:
            t.fill_(float("nan"))
        return t

    t = dict(state_in=f((rows, 24), torch.float64), ref_in=f((rows, 24), torch.float64),
             contacts=f((rows, 4, stride)), keys=f((rows, 2), torch.int64), previous_contact=f((rows, 4)),
             best_params=f((rows, P)), states=f((rows, 24)), refs=f((rows, 24)), grf=f((rows, 12), torch.float64),
             footholds=f((rows, 12), torch.float64), grf_raw=f((rows, 12)), predicted_state=f((rows, 24)),
             best_cost=f((rows,)), best_index=f((rows,), torch.int32), best_freq=f((rows,)),
             status=f((rows,), torch.int32), costs=f((rows, N)))
    if cem:
        t["sigma"] = f((rows, P))
    return t


def raw_io(lib, t, iterations, stride, P, sigma_reset=0.0, gait=None):
    def p(k):
        return None if t.get(k) is None else t[k].data_ptr()

    return lib.BatchInterfaceIO(
        state_in=p("state_in"), ref_in=p("ref_in"), contacts=p("contacts"), contact_stride=stride,
        iterations=iterations, params_per_leg=P // 4, pad=0, gait=None if gait is None else C.pointer(gait),
        keys=p("keys"), previous_contact=p("previous_contact"), best_params=p("best_params"), sigma=p("sigma"),
        sigma_reset=sigma_reset, pad2=0, states=p("states"), refs=p("refs"), grf=p("grf"), footholds=p("footholds"),
        grf_raw=p("grf_raw"), predicted_state=p("predicted_state"), best_cost=p("best_cost"),
        best_index=p("best_index"), best_freq=p("best_freq"), status=p("status"), costs=p("costs"))


def fill_inputs(lib, t, E, H, rng, P):
    contacts, (st, rf) = contact_steps(E, H, 1), state_steps(E, 1)
    t["state_in"][:E] = dev(st[0])
    t["ref_in"][:E] = dev(rf[0])
    t["contacts"][:E, :, :H] = dev(contacts[0])
    t["keys"][:E] = dev(initial_keys(lib, E, rng), torch.int64)
    t["previous_contact"][:E] = 1.0
    t["best_params"][:E] = dev(initial_best(E, P))
    return st[0], rf[0], contacts[0]


def call(lib, b, io):
    return lib.lib.srbd_batch_interface_step_device(b.h, C.byref(io), C.c_void_p(1))


@pytest.mark.parametrize("method", ["mppi", "cem_mppi"])
def test_nothing_outside_the_documented_outputs_is_written(lib, method):
    E, rows, H, stride, rng = 3, 5, 12, 15, "philox"
    case = case_of(method=method)
    cem = method == "cem_mppi"
    b = (lib.CemBatchContext if cem else lib.BatchContext)(product_cfg(case), E)
    host = None
    try:
        t = raw_tensors(lib, b, E, rows, stride, cem)
        st, rf, contacts = fill_inputs(lib, t, E, H, rng, b.P)
        before = {k: v.clone() for k, v in t.items()}
        torch.cuda.synchronize()
        assert call(lib, b, raw_io(lib, t, 2, stride, b.P, SIGMA_RESET if cem else 0.0)) == lib.OK
        torch.cuda.synchronize()
        for k in ("state_in", "ref_in", "contacts"):  # inputs: unchanged, poison included
            assert t[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), k
        for k, v in t.items():  # every array: the rows beyond E keep their poison
            assert v[E:].cpu().numpy().tobytes() == before[k][E:].cpu().numpy().tobytes(), k
        # and the first E rows are the host call's
        host = HostChain(lib, case, E, rng, initial_keys(lib, E, rng), initial_best(E, b.P))
        want = host.step(st, rf, contacts, 2)
        got = {k: t[k][:E].cpu().numpy() for k in OUT_KEYS}
        got.update(keys=t["keys"][:E].cpu().numpy().view(np.uint64), previous_contact=t["previous_contact"][:E].cpu().numpy(),
                   best=t["best_params"][:E].cpu().numpy(), sigma=t["sigma"][:E].cpu().numpy() if cem else None)
        assert_same(got, want)
    finally:
        b.close()
        if host:
            host.close()


def test_stream_order_and_no_host_synchronisation(lib):
    """Enqueued on a side stream behind a long kernel and the copy that produces `contacts`: the call returns while the
    stream is still busy, and the results equal the synchronous run's."""
    E, rng = 3, "jax"
    case = case_of()
    contacts, (st, rf) = contact_steps(E, 12, 1), state_steps(E, 1)
    keys, best = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    sync, side = DeviceLoop(lib, case, E, rng, keys, best), DeviceLoop(lib, case, E, rng, keys, best)
    try:
        want = sync.step(st[0], rf[0], contacts[0], 2)
        s = torch.cuda.Stream()
        src, st_d, rf_d = dev(contacts[0]), dev(st[0]), dev(rf[0])
        produced = torch.zeros_like(src)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(50_000_000)  # tens of milliseconds of device time ahead of everything below
            produced.copy_(src)             # `contacts` exists only once the stream gets here
            out = side.enqueue(st_d, rf_d, produced, 2, stream=s)
            busy = not s.query()
        assert busy, "the call waited for the device"
        s.synchronize()
        assert_same(side.collect(out), want)
    finally:
        sync.close()
        side.close()


def test_switching_streams_between_calls_is_ordered(lib):
    """Two consecutive calls on two streams with no host wait between them, the first held back by a long kernel: the
    second waits on the batch's event, which lies behind the first call's epilogue, so it reads the previous_contact
    (and keys, warm starts) the first call left.  The inputs hold a leg that swings through both steps: with the
    initial ones as previous contact its warm start would be zeroed."""
    E, rng = 3, "philox"
    case = case_of()
    contacts, (st, rf) = contact_steps(E, 12)[4:6], state_steps(E, 2)  # two steps inside a swing phase
    assert np.any((contacts[0][:, :, 0] == 0) & (contacts[1][:, :, 0] == 0))
    keys, best = initial_keys(lib, E, rng), initial_best(E, case["orc"].P)
    sync, side = DeviceLoop(lib, case, E, rng, keys, best), DeviceLoop(lib, case, E, rng, keys, best)
    try:
        sync.step(st[0], rf[0], contacts[0], 2)
        want = sync.step(st[1], rf[1], contacts[1], 2)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        ins = [(dev(st[k]), dev(rf[k]), dev(contacts[k])) for k in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            torch.cuda._sleep(50_000_000)
            first = side.enqueue(*ins[0], 2, stream=sa)
        with torch.cuda.stream(sb):
            out = side.enqueue(*ins[1], 2, stream=sb)
        assert_same(side.collect(out), want)
        assert first["grf"].shape == (E, 12)
    finally:
        sync.close()
        side.close()


def test_refusals_change_nothing(lib):
    E, H, rng = 3, 12, "philox"
    plain = lib.BatchContext(product_cfg(case_of()), E)
    cemb = lib.CemBatchContext(product_cfg(case_of(method="cem_mppi")), E)
    try:
        def refused(b, cem, why, mutate=None, iterations=2, stride=H, ppl=None, sigma_reset=None, gait=None):
            t = raw_tensors(lib, b, E, E, max(stride, H), cem)
            fill_inputs(lib, t, E, H, rng, b.P)
            if mutate:
                mutate(t)
            io = raw_io(lib, t, iterations, stride, b.P, (SIGMA_RESET if cem else 0.0) if sigma_reset is None
                        else sigma_reset, gait)
            if ppl is not None:
                io.params_per_leg = ppl
            keep = {k: t[k].clone() for k in ("keys", "best_params", "previous_contact") if t.get(k) is not None}
            torch.cuda.synchronize()
            assert call(lib, b, io) == lib.E_INVALID, why
            msg = lib.lib.srbd_batch_last_error(b.h).decode()
            assert why in msg, (why, msg)
            torch.cuda.synchronize()
            for k, v in keep.items():
                assert t[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (why, k)

        assert lib.lib.srbd_batch_interface_step_device(plain.h, None, C.c_void_p(1)) == lib.E_INVALID
        assert "null io" in lib.lib.srbd_batch_last_error(plain.h).decode()
        for name in ("state_in", "ref_in", "contacts", "keys", "previous_contact", "best_params", "states", "refs",
                     "grf", "footholds", "grf_raw", "predicted_state", "best_cost", "best_index", "best_freq",
                     "status"):
            refused(plain, False, name, lambda t, n=name: t.__setitem__(n, None))
        refused(cemb, True, "sigma", lambda t: t.__setitem__("sigma", None))
        refused(plain, False, "iterations", iterations=0)
        refused(plain, False, "iterations", iterations=9)
        refused(plain, False, "contact_stride", stride=H - 1)
        refused(plain, False, "params_per_leg", ppl=0)
        refused(plain, False, "params_per_leg", ppl=plain.P // 4 + 1)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused(cemb, True, "sigma_reset", sigma_reset=bad)
        opt = torch.zeros(E, dtype=torch.int32, device="cuda")
        tim = torch.zeros((E, 4), dtype=torch.float32, device="cuda")
        nom = torch.full((E,), 1.4, dtype=torch.float32, device="cuda")
        gait = plain.make_gait_io(opt, [1.3, 1.4], 0.02, 0.65, timings=tim, nominal_freqs=nom)
        refused(cemb, True, "gait on a CEM batch", gait=gait)
        plain.set_cost_terms(**TERMS)
        refused(plain, False, "gait together with active cost terms", gait=gait)
        plain.set_cost_terms()
        bad_gait = plain.make_gait_io(opt, [1.3, 1.4], 0.02, 0.65, timings=tim, nominal_freqs=nom)
        bad_gait.n_freq = 9  # a refusal of the underlying gait setter
        refused(plain, False, "n_freq", gait=bad_gait)
        # costs may be NULL, and a refused batch still steps
        t = raw_tensors(lib, plain, E, E, H, False)
        fill_inputs(lib, t, E, H, rng, plain.P)
        t["costs"] = None
        assert call(lib, plain, raw_io(lib, t, 1, H, plain.P)) == lib.OK
        torch.cuda.synchronize()
        assert np.isfinite(t["grf"].cpu().numpy()).all()
    finally:
        plain.close()
        cemb.close()


# ------------------------------------------------------------------ the Python class
def _cfg(**mp):
    from quadruped_pympc_amd import config as base

    c = types.SimpleNamespace(**{k: copy.deepcopy(getattr(base, k)) for k in
                                 ("robot", "mass", "inertia", "hip_height", "gravity_constant", "mpc_params",
                                  "simulation_params")})
    c.mpc_params.update(device_id=0, grf_max=c.mass * 9.81, **mp)
    return c


def _dicts(st, rf):
    legs = ("FL", "FR", "RL", "RR")
    sc = {"position": st[0:3].copy(), "linear_velocity": st[3:6].copy(), "orientation": st[6:9].copy(),
          "angular_velocity": st[9:12].copy()}
    rs = {"ref_position": rf[0:3].copy(), "ref_linear_velocity": rf[3:6].copy(), "ref_orientation": rf[6:9].copy(),
          "ref_angular_velocity": rf[9:12].copy()}
    for i, n in enumerate(legs):
        sc["foot_" + n] = st[12 + 3 * i:15 + 3 * i].copy()
        rs["ref_foot_" + n] = rf[12 + 3 * i:15 + 3 * i].copy().reshape(1, 3)
    return sc, rs


@pytest.mark.parametrize("kind,rng", [("plain", "jax"), ("gait_adaptive", "philox"), ("cem", "jax_legacy")])
def test_python_class_equals_single_interfaces(lib, kind, rng):
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_cem_batched import Batched_CEM_Sampling_MPC
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_gait_adaptive_batched import (
        Batched_Sampling_MPC as Batched_GA)
    from quadruped_pympc_amd.interfaces.srbd_controller_interface import SRBDControllerInterface
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import Batched_SRBDControllerInterface

    E, H = 3, 12
    mp = dict(sampling_method="cem_mppi" if kind == "cem" else "mppi", control_parametrization="zero_order",
              num_parallel_computations=192, horizon=H, num_sampling_iterations=2,
              rng="jax" if rng == "jax_legacy" else rng, jax_threefry_partitionable=rng != "jax_legacy",
              optimize_step_freq=kind == "gait_adaptive", shift_solution=False)
    cls = {"plain": Batched_Sampling_MPC, "gait_adaptive": Batched_GA, "cem": Batched_CEM_Sampling_MPC}[kind]
    ctrl = cls(E, _cfg(**mp))
    iface = Batched_SRBDControllerInterface(ctrl)
    # a fresh interface holds its state at once: previous_contact_mpc ones, keys the controller's
    assert iface.previous_contact_mpc.dtype == torch.float32 and tuple(iface.previous_contact_mpc.shape) == (E, 4)
    assert iface.previous_contact_mpc.is_cuda and bool((iface.previous_contact_mpc == 1).all())
    assert tuple(iface.keys.shape) == (E, 2) and iface.keys.is_cuda
    k0 = iface.keys.cpu().numpy().view(np.uint64)
    if rng == "philox":
        np.testing.assert_array_equal(k0, np.asarray(ctrl.master_keys, np.uint64))
    else:
        assert [int(v) for v in k0[:, 0]] == [lib.pack_key(k) for k in ctrl.master_keys] and not k0[:, 1].any()
    assert tuple(iface.best_control_parameters.shape) == (E, ctrl.num_control_parameters)
    assert (iface.sigma_cem_mppi is not None) == (kind == "cem") and iface.last_device_result is None
    singles = [SRBDControllerInterface(_cfg(**mp)) for _ in range(E)]
    contacts = contact_steps(E, H)
    assert_contact_coverage(contacts)
    st, rf = state_steps(E)
    try:
        for e, s in enumerate(singles):
            s.controller.master_key = np.array(ctrl.master_keys[e])
        for k in range(STEPS):
            g = np.random.default_rng(90 + k)
            phases, swing = g.uniform(0, 1, (E, 4)), g.integers(0, 2, E)
            kw = {}
            if kind == "gait_adaptive":
                kw = dict(timings=dev(phases.astype(f32)), nominal_step_frequencies=dev(np.full(E, 1.4, f32)),
                          optimize_swings=dev(swing.astype(np.int32)))
            out = iface.compute_control_device(dev(st[k]), dev(rf[k]), dev(contacts[k]), **kw)
            torch.cuda.synchronize()
            grf, fh = out[0].cpu().numpy(), out[1].cpu().numpy()
            keys = iface.keys.cpu().numpy().view(np.uint64)
            for e, s in enumerate(singles):
                sc, rs = _dicts(st[k, e], rf[k, e])
                r = s.compute_control(sc, rs, contacts[k, e].astype(np.float64), None, phases[e], 1.4, int(swing[e]))
                want = np.concatenate([np.asarray(r[0][n], np.float64) for n in ("FL", "FR", "RL", "RR")])
                assert grf[e].tobytes() == want.tobytes(), f"step {k} env {e} grf"
                np.testing.assert_array_equal(fh[e], rf[k, e, 12:])
                np.testing.assert_array_equal(iface.previous_contact_mpc[e].cpu().numpy(),
                                              np.asarray(s.previous_contact_mpc, f32))
                c1 = s.controller
                if rng == "philox":
                    np.testing.assert_array_equal(keys[e], np.asarray(c1.master_key, np.uint64))
                else:
                    assert int(keys[e, 0]) == lib.pack_key(c1.master_key) and int(keys[e, 1]) == c1._calls
                if kind == "gait_adaptive":
                    assert f32(out[3][e].item()) == f32(r[5])
        assert ctrl._calls == 2 * STEPS
        # reset(mask) restores only the masked rows
        before = iface.previous_contact_mpc.clone()
        iface.previous_contact_mpc[:] = 0.0
        iface.reset(dev(np.array([0, 1, 0], np.int32)))
        np.testing.assert_array_equal(iface.previous_contact_mpc.cpu().numpy(), [[0] * 4, [1] * 4, [0] * 4])
        iface.reset()
        assert bool((iface.previous_contact_mpc == 1).all()) and before.shape == (E, 4)
    finally:
        ctrl.close()
        for s in singles:
            s.controller.close()


def test_python_class_refuses_shift_solution(lib):
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import Batched_SRBDControllerInterface

    ctrl = Batched_Sampling_MPC(2, _cfg(sampling_method="mppi", num_parallel_computations=192, shift_solution=True))
    with pytest.raises(NotImplementedError):
        Batched_SRBDControllerInterface(ctrl)
