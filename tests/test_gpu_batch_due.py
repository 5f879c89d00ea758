"""GPU: the due mask of the batch's device steps (srbd_batch_step_masked_device, srbd_batch_step_cem_masked_device,
srbd_batch_interface_step_masked_device, include/srbd_mpc.h).  Every comparison is of bytes: a due environment holds
what the unmasked call leaves for it on a second batch with the same inputs, an environment that is not due holds its
pre-call bytes -- the in / out state unchanged, the outputs still the sentinel.  A staggered schedule is compared with
E batches of one environment stepped by the unmasked call on their due ticks only, and the arrival count is checked by
a host step behind a masked call.  Expected values never come from the call under test.

The shapes are the smallest that exercise the skips: E = 5 and N = 130 (three leaves per environment, the last with two
valid rows), so every launch has blocks of due and of skipped environments side by side."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_batch_interface as ti
from helpers import f32, product_cfg
from test_gpu_batch_interface import dev, lib  # noqa: F401  (lib: module fixture)

pytestmark = pytest.mark.gpu

E, N = 5, 130
SIGMA_RESET = ti.SIGMA_RESET
MASKS = {"all": [1, 1, 1, 1, 1], "none": [0, 0, 0, 0, 0], "one": [0, 0, 1, 0, 0], "alternate": [1, 0, 1, 0, 1]}
SENT_F, SENT_I = -12345.678, -77  # the outputs' sentinel pattern

# name -> the batch: method, parametrization, horizon, key stream, sampling iterations, io->gait, the settings
CONFIGS = {
    "mppi_zo_philox": dict(method="mppi", par="zero_order", H=12, rng="philox", it=1),
    "rs_linear_jax": dict(method="random_sampling", par="linear_spline", H=12, rng="jax", it=1),
    "cem_cubic_h16": dict(method="cem_mppi", par="cubic_spline", H=16, rng="philox", it=2),
    "gait_zo": dict(method="mppi", par="zero_order", H=12, rng="philox", it=1, gait=True),
    "cost_terms": dict(method="mppi", par="zero_order", H=12, rng="philox", it=1, terms=True),
    "env_params": dict(method="mppi", par="zero_order", H=12, rng="jax_legacy", it=1, envp=True),
}
IFACE_STATE = ("keys", "previous_contact", "best", "sigma")
IFACE_OUT = ("states", "refs", "grf", "footholds", "grf_raw", "predicted_state", "best_cost", "best_index", "best_freq",
             "status", "costs")
STEP_OUT = ("grf", "predicted_state", "best_cost", "best_index", "best_freq", "status", "costs")


def case_of(cfg):
    return ti.case_of(N, cfg["method"], cfg["par"], cfg["H"], 2)


def make_batch(lib, cfg, num_envs=E, env=None):
    """A batch of the configuration with its settings; env: the one environment of E whose parameters an E = 1 batch
    takes."""
    cem = cfg["method"] == "cem_mppi"
    b = (lib.CemBatchContext if cem else lib.BatchContext)(product_cfg(case_of(cfg)), num_envs)
    if cfg["rng"] != "philox":
        b.set_rng(cfg["rng"])
    if cfg.get("terms"):
        b.set_cost_terms(**ti.TERMS)
    if cfg.get("envp"):
        mass, mu = np.array([12.0, 15.0, 19.0, 13.0, 17.0]), np.array([0.4, 0.5, 0.7, 0.6, 0.45])
        sel = slice(None) if env is None else slice(env, env + 1)
        b.set_env_params(lib.make_env_params(num_envs, b.cfg, mass=mass[sel], mu=mu[sel]))
    return b


def sentinel_out(P, rows=E, step=False):
    """The output dict of a call, every row the sentinel."""
    def f(shape, dtype=torch.float32):
        return torch.full(shape, SENT_I if dtype == torch.int32 else SENT_F, dtype=dtype, device="cuda")

    out = dict(grf=f((rows, 12)) if step else f((rows, 12), torch.float64), predicted_state=f((rows, 24)),
               best_cost=f((rows,)), best_index=f((rows,), torch.int32), best_freq=f((rows,)),
               status=f((rows,), torch.int32), costs=f((rows, N)))
    if not step:
        out.update(states=f((rows, 24)), refs=f((rows, 24)), footholds=f((rows, 12), torch.float64),
                   grf_raw=f((rows, 12)))
    return out


def iface_inputs(lib, cfg, P, ticks=1):
    """numpy inputs of `ticks` interface calls and the in / out state ahead of the first: real keys, a previous
    contact that differs from the current one (the lift-off zeroing runs), a warm start and, CEM, a sigma."""
    H = cfg["H"]
    contacts = ti.contact_steps(E, H, ticks + 1)
    st, rf = ti.state_steps(E, ticks)
    state = dict(keys=ti.initial_keys(lib, E, cfg["rng"]), previous_contact=contacts[0][:, :, 0].copy(),
                 best=ti.initial_best(E, P),
                 sigma=np.full((E, P), 2.0, f32) if cfg["method"] == "cem_mppi" else None)
    return dict(state_in=st, ref_in=rf, contacts=contacts[1:]), state


def gait_of(b, tick, rows=slice(None)):
    """The gait setting of a tick, the rows of an E = 1 batch or all -> (BatchGaitIO, the tensors it points to)."""
    g = np.random.default_rng(70 + tick)
    optimize, timings = g.integers(0, 2, E).astype(np.int32), g.uniform(0, 1, (E, 4)).astype(f32)
    alive = (dev(optimize[rows]), dev(timings[rows]), dev(np.full(E, 1.4, f32)[rows]))
    return b.make_gait_io(alive[0], [1.3, 1.4, 1.5], 0.02, 0.65, timings=alive[1], nominal_freqs=alive[2]), alive


class Loop:
    """One batch and the device tensors of the interface call: the in / out state and one held output dict."""

    def __init__(self, lib, cfg, state, num_envs=E, env=None):
        self.cfg, self.env = cfg, env
        self.rows = slice(None) if env is None else slice(env, env + 1)
        self.b = make_batch(lib, cfg, num_envs, env)
        r = self.rows
        self.keys = dev(np.array(state["keys"][r], np.uint64), torch.int64)
        self.prev = dev(np.array(state["previous_contact"][r], f32))
        self.best = dev(np.array(state["best"][r], f32))
        self.sigma = None if state["sigma"] is None else dev(np.array(state["sigma"][r], f32))
        self.out = sentinel_out(self.b.P, num_envs)

    def close(self):
        self.b.close()

    def call(self, inp, tick, due=None):
        """due None: the unmasked call (its outputs copied into the held dict afterwards); else the masked call
        writing into the held dict."""
        r, cfg = self.rows, self.cfg
        gait_io, alive = gait_of(self.b, tick, r) if cfg.get("gait") else (None, None)  # alive until the wait below
        kw = dict(iterations=cfg["it"], sigma=self.sigma, sigma_reset=SIGMA_RESET if self.sigma is not None else 0.0,
                  gait_io=gait_io, want_costs=True)
        args = (dev(inp["state_in"][tick][r]), dev(inp["ref_in"][tick][r]), dev(inp["contacts"][tick][r]), self.keys,
                self.prev, self.best)
        if due is None:
            out = self.b.interface_step_device(*args, **kw)
            for k, v in out.items():
                self.out[k].copy_(v)
        else:
            got = self.b.interface_step_masked_device(*args, due, out=self.out, **kw)
            assert got is self.out
        torch.cuda.synchronize()
        del alive

    def snapshot(self):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy().copy() for k, v in self.out.items()}
        got.update(keys=self.keys.cpu().numpy().view(np.uint64).copy(), previous_contact=self.prev.cpu().numpy(),
                   best=self.best.cpu().numpy(), sigma=None if self.sigma is None else self.sigma.cpu().numpy(),
                   batch_costs=self.b.copy_costs())
        return got


def assert_rows(got, want, rows, what, keys):
    """Rows `rows` of every array named: the same bytes."""
    for k in keys:
        if want.get(k) is None:
            assert got.get(k) is None, k
            continue
        g, w = np.ascontiguousarray(got[k][rows]), np.ascontiguousarray(want[k][rows])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {k}"
        if g.tobytes() != w.tobytes():
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {k} rows {rows}")
            raise AssertionError(f"{what} {k}: equal values, different bytes")


# ------------------------------------------------------------------ single-call parity, the interface step
_unmasked = {}


def unmasked_reference(lib, name):
    """Batch B of a configuration, computed once: the inputs, the pre-call bytes and what the unmasked
    srbd_batch_interface_step_device leaves."""
    if name not in _unmasked:
        cfg = CONFIGS[name]
        probe = make_batch(lib, cfg)
        P = probe.P
        probe.close()
        inp, state = iface_inputs(lib, cfg, P)
        loop = Loop(lib, cfg, state)
        try:
            before = {k: v.cpu().numpy().copy() for k, v in loop.out.items()}
            before.update(state)
            loop.call(inp, 0)
            _unmasked[name] = (inp, state, before, loop.snapshot())
        finally:
            loop.close()
    return _unmasked[name]


def masked_run(lib, name, mask, inp, state, as_bool=False):
    """Batch A: one masked interface call on the inputs; the snapshot behind it."""
    loop = Loop(lib, CONFIGS[name], state)
    try:
        due = dev(np.array(mask, np.int32))
        loop.call(inp, 0, due.bool() if as_bool else due)
        return loop.snapshot()
    finally:
        loop.close()


def check_single_call(got, want, before, mask, what):
    due = np.flatnonzero(np.array(mask) != 0)
    held = np.flatnonzero(np.array(mask) == 0)
    assert_rows(got, want, due, what + " due", IFACE_STATE + IFACE_OUT)
    assert_rows(got, before, held, what + " not due", IFACE_STATE + IFACE_OUT)
    # the batch's own costs rows: the solve's for a due environment, untouched (zero since create) otherwise
    assert_rows(got, want, due, what + " due", ("batch_costs",))
    assert not got["batch_costs"][held].any(), what + ": costs row of an environment that is not due"


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_interface_step_single_call(lib, name, mask):
    inp, state, before, want = unmasked_reference(lib, name)
    got = masked_run(lib, name, MASKS[mask], inp, state)
    if any(MASKS[mask]):
        assert np.all(got["status"][np.array(MASKS[mask]) != 0] == 0)
    check_single_call(got, want, before, MASKS[mask], f"{name} {mask}")


def test_bool_mask_is_the_int32_mask(lib):
    inp, state, before, want = unmasked_reference(lib, "mppi_zo_philox")
    got = masked_run(lib, "mppi_zo_philox", MASKS["alternate"], inp, state, as_bool=True)
    check_single_call(got, want, before, MASKS["alternate"], "bool")


@pytest.mark.parametrize("name", ["mppi_zo_philox", "cem_cubic_h16", "gait_zo"])
def test_nan_inputs_of_environments_not_due_change_nothing(lib, name):
    """state_in, ref_in and contacts of the environments that are not due are NaN: the due rows are the clean run's
    (the unmasked call's), the others untouched."""
    inp, state, before, want = unmasked_reference(lib, name)
    mask = MASKS["alternate"]
    held = np.array(mask) == 0
    bad = {k: v.copy() for k, v in inp.items()}
    for k in bad:
        bad[k][:, held] = np.nan
    got = masked_run(lib, name, mask, bad, state)
    check_single_call(got, want, before, mask, f"{name} nan")


# ------------------------------------------------------------------ single-call parity, the step and its CEM form
STEP_CASES = {
    "mppi_draws": dict(cfg="mppi_zo_philox", noise=False),
    "mppi_injected_noise": dict(cfg="mppi_zo_philox", noise=True),  # the transpose in place of the draws
    "linear_jax": dict(cfg="rs_linear_jax", noise=False),
    "cem": dict(cfg="cem_cubic_h16", noise=False),
    "cem_sigma_reset": dict(cfg="cem_cubic_h16", noise=False, reset=SIGMA_RESET),
}
_step_ref = {}


def step_tensors(lib, cfg, P, noise):
    H = cfg["H"]
    st, rf = ti.state_steps(E, 1)
    keys = ti.initial_keys(lib, E, cfg["rng"])
    t = dict(states=dev(st[0].astype(f32)), refs=dev(rf[0].astype(f32)), contacts=dev(ti.contact_steps(E, H, 1)[0]),
             best=dev(ti.initial_best(E, P)), seeds=dev(keys[:, 0].copy(), torch.int64),
             counters=dev(keys[:, 1].copy(), torch.int64))
    if cfg["method"] == "cem_mppi":
        t["sigma"] = dev(np.full((E, P), 2.0, f32))
    if noise:
        z = np.random.default_rng(5).standard_normal((E, N, P)).astype(f32)
        z[:, 0] = 0.0
        t["noise"] = dev(z)
    return t


def run_step(lib, case, mask):
    """One step of a fresh batch -- unmasked (mask None) or masked into a sentinel dict -> (before, after), numpy."""
    cfg = CONFIGS[case["cfg"]]
    b = make_batch(lib, cfg)
    try:
        t = step_tensors(lib, cfg, b.P, case["noise"])
        out = sentinel_out(b.P, step=True)
        snap = lambda: dict({k: v.cpu().numpy().copy() for k, v in out.items()},  # noqa: E731
                            best=t["best"].cpu().numpy(), sigma=t["sigma"].cpu().numpy() if "sigma" in t else None)
        before = snap()
        args = [t["states"], t["refs"], t["contacts"], t["best"]] + ([t["sigma"]] if "sigma" in t else []) + \
            [t["seeds"], t["counters"]]
        kw = dict(noise=t.get("noise"), want_costs=True)
        if "sigma" in t:
            kw["sigma_reset"] = case.get("reset", 0.0)
        if mask is None:
            res = (b.step_cem_device if "sigma" in t else b.step_device)(*args, **kw)
            for k, v in res.items():
                out[k].copy_(v)
        else:
            fn = b.step_cem_masked_device if "sigma" in t else b.step_masked_device
            assert fn(*args, dev(np.array(mask, np.int32)), out=out, **kw) is out
        torch.cuda.synchronize()
        after = snap()
        after["batch_costs"] = b.copy_costs()
        return before, after
    finally:
        b.close()


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_single_call(lib, name, mask):
    case = STEP_CASES[name]
    if name not in _step_ref:
        _step_ref[name] = run_step(lib, case, None)[1]
    want = _step_ref[name]
    before, got = run_step(lib, case, MASKS[mask])
    due, held = np.flatnonzero(np.array(MASKS[mask]) != 0), np.flatnonzero(np.array(MASKS[mask]) == 0)
    keys = STEP_OUT + ("best", "sigma")
    assert_rows(got, want, due, f"{name} {mask} due", keys + ("batch_costs",))
    assert_rows(got, before, held, f"{name} {mask} not due", keys)
    assert not got["batch_costs"][held].any()


# ------------------------------------------------------------------ the staggered schedule
TICKS, PERIOD = 12, 5
PHASES = np.arange(E)


@pytest.mark.parametrize("name", ["mppi_zo_philox", "rs_linear_jax", "cem_cubic_h16", "gait_zo", "env_params"])
def test_staggered_schedule_against_single_environment_batches(lib, name):
    """12 ticks, MPC period 5, environment e at phase e: one environment is due per tick, each two or three times (the
    tick with none due is the single-call tests' "none" mask).  Batch A makes one
    masked call per tick into one held dict; environment e also runs alone on a batch of one environment, stepped by
    the unmasked call on its due ticks only.  Afterwards every in / out row and every held output row agree."""
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import mpc_due

    cfg = CONFIGS[name]
    probe = make_batch(lib, cfg)
    P = probe.P
    probe.close()
    inp, state = iface_inputs(lib, cfg, P, TICKS)
    batch = Loop(lib, cfg, state)
    singles = [Loop(lib, cfg, state, 1, e) for e in range(E)]
    try:
        solved = np.zeros(E, int)
        for tick in range(TICKS):
            step_num = dev((tick + PHASES).astype(np.int64))
            due = mpc_due(step_num, 0.002, 100.0)
            want_due = ((tick + PHASES) % PERIOD == 0)
            assert due.dtype == torch.int32 and due.cpu().numpy().tolist() == want_due.astype(int).tolist()
            batch.call(inp, tick, due)
            for e in np.flatnonzero(want_due):
                singles[e].call(inp, tick)
                solved[e] += 1
        assert np.all(solved >= 2)
        got = batch.snapshot()
        for e in range(E):
            want = singles[e].snapshot()
            for k in IFACE_STATE + IFACE_OUT + ("batch_costs",):
                if want[k] is None:
                    continue
                assert got[k][e].tobytes() == want[k][0].tobytes(), f"{name} environment {e} {k}"
        assert np.all(got["status"] == 0)
    finally:
        batch.close()
        for s in singles:
            s.close()


# ------------------------------------------------------------------ the arrival count and the sequence word survive
def host_then_device(lib, b, cfg):
    """A host srbd_batch_step and an unmasked device step behind it, on fixed inputs -> their outputs as numpy."""
    H = cfg["H"]
    st, rf = ti.state_steps(E, 1)
    contacts = ti.contact_steps(E, H, 1)[0]
    keys, best0 = ti.initial_keys(lib, E, cfg["rng"]), ti.initial_best(E, b.P)
    best, results, costs = b.step(st[0].astype(f32), rf[0].astype(f32), contacts, best0, seeds=keys[:, 0],
                                  counters=keys[:, 1], want_costs=True)
    host = dict(best=best, costs=costs, grf=np.array([r.grf[:] for r in results], f32),
                pred=np.array([r.predicted_state[:] for r in results], f32),
                cost=np.array([r.best_cost for r in results], f32), status=np.array([r.status for r in results]))
    tb = dev(best0)
    out = b.step_device(dev(st[0].astype(f32)), dev(rf[0].astype(f32)), dev(contacts), tb,
                        dev(keys[:, 0].copy(), torch.int64), dev(keys[:, 1].copy(), torch.int64), want_costs=True)
    torch.cuda.synchronize()
    device = {k: v.cpu().numpy() for k, v in out.items()}
    device["best"] = tb.cpu().numpy()
    return host, device


@pytest.mark.parametrize("mask", ["none", "one"])
def test_host_step_and_device_step_follow_a_masked_call(lib, mask):
    """Behind a masked call with no environment due, and behind a partial one, the merge blocks' arrival count is
    zero and the sequence word published: a host srbd_batch_step on the same batch returns (it waits on that word),
    with the bytes of a batch that never saw a masked call, and so does an unmasked device step.  One run of each."""
    cfg = CONFIGS["mppi_zo_philox"]
    inp, state = iface_inputs(lib, cfg, 12 * cfg["H"])
    fresh = make_batch(lib, cfg)
    masked = Loop(lib, cfg, state)
    try:
        assert masked.b.P == 12 * cfg["H"]
        masked.call(inp, 0, dev(np.array(MASKS[mask], np.int32)))
        got_host, got_dev = host_then_device(lib, masked.b, cfg)
        want_host, want_dev = host_then_device(lib, fresh, cfg)
        for got, want in ((got_host, want_host), (got_dev, want_dev)):
            for k in want:
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
        assert np.all(want_host["status"] == 0)
    finally:
        fresh.close()
        masked.close()


# ------------------------------------------------------------------ the raw call's refusal, on a live batch
def test_null_due_is_refused_before_anything_is_enqueued(lib):
    cfg = CONFIGS["mppi_zo_philox"]
    b = make_batch(lib, cfg)
    try:
        t = ti.raw_tensors(lib, b, E, E, cfg["H"], False)
        before = {k: v.clone() for k, v in t.items()}
        io = ti.raw_io(lib, t, 1, cfg["H"], b.P)
        rc = lib.lib.srbd_batch_interface_step_masked_device(b.h, C.byref(io), None, C.c_void_p(1))
        assert rc == lib.E_INVALID
        msg = lib.lib.srbd_batch_last_error(b.h).decode()
        assert "null due" in msg and "srbd_batch_interface_step_device" in msg
        torch.cuda.synchronize()
        for k, v in t.items():
            assert v.cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), k
    finally:
        b.close()


# ------------------------------------------------------------------ the Python layer
def test_controller_interface_holds_the_rows_of_environments_not_due(lib):
    """Batched_SRBDControllerInterface.compute_control_device(due=): the rows of an environment that is not due are
    the previous call's, those of a due one change; compute_plan_device behind it gives, for a due environment, the
    cost the next step's row 0 has (the warm start rolled out from the held prepared rows)."""
    import test_gpu_batch_plan as tp
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.interfaces.srbd_controller_interface_batched import Batched_SRBDControllerInterface

    n_env, H = 3, 12
    ctrl = Batched_Sampling_MPC(n_env, tp._controller_cfg(
        sampling_method="mppi", control_parametrization="zero_order", num_parallel_computations=tp.N, horizon=H,
        num_sampling_iterations=1, rng="philox", optimize_step_freq=False, shift_solution=False))
    iface = Batched_SRBDControllerInterface(ctrl)
    cases = tp.env_cases(n_env, **tp.SHAPES["zo_h12"])
    st = dev(tp.stack(cases, "state").astype(np.float64))
    rf = dev(tp.stack(cases, "ref").astype(np.float64))
    ct = dev(tp.stack(cases, "contact"))
    every = torch.ones(n_env, dtype=torch.int32, device="cuda")
    due = dev(np.array([1, 0, 1], np.int32))
    names = ("grf", "footholds", "predicted_state", "best_freq", "best_cost")
    first = iface.compute_control_device(st, rf, ct, due=every)
    torch.cuda.synchronize()
    held = {n: t.cpu().numpy().copy() for n, t in zip(names, first)}
    keys0 = iface.keys.cpu().numpy().copy()
    best0 = iface.best_control_parameters.cpu().numpy().copy()
    second = iface.compute_control_device(st, rf, ct, due=due)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(first[:3], second[:3]))  # one persistent dict
    now = {n: t.cpu().numpy() for n, t in zip(names, second)}
    for n in ("grf", "footholds", "predicted_state", "best_cost"):
        assert now[n][1].tobytes() == held[n][1].tobytes(), n
    keys1 = iface.keys.cpu().numpy()
    assert keys1[1].tolist() == keys0[1].tolist() and keys1[0, 1] == keys0[0, 1] + 1 and keys1[2, 1] == keys0[2, 1] + 1
    best1 = iface.best_control_parameters.cpu().numpy()
    assert best1[1].tobytes() == best0[1].tobytes() and best1[0].tobytes() != best0[0].tobytes()
    assert now["predicted_state"][0].tobytes() != held["predicted_state"][0].tobytes()
    plan = iface.compute_plan_device(want=("plan_cost",))["plan_cost"].clone()
    nxt = iface.compute_control_device(st, rf, ct, due=due)
    torch.cuda.synchronize()
    costs = np.asarray(nxt[-1])
    for e in (0, 2):
        assert f32(plan[e].item()).tobytes() == f32(costs[e, 0]).tobytes(), e
    ctrl.close()
