"""The device producers (srbd_pgg_run_device, srbd_pgg_contact_sequence_device, srbd_prepare_state_device;
BatchedPeriodicGaitGenerator, Batched_Sampling_MPC.prepare_state_and_reference_device) against the host producers
(srbd_pgg_run, srbd_pgg_contact_sequence, srbd_prepare_state, include/srbd_host.h), which the CPU tests pin to
oracle/pgg_oracle.py and the golden fixtures.  The contract is bit equality -- the generator state's bytes after
every call, the contact flags, the float32 states and references -- so every comparison is exact and no tolerance
appears here.  Expected values never come from the device path."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import config as mirror
from quadruped_pympc_amd.helpers.periodic_gait_generator import (FULL_STANCE, BatchedPeriodicGaitGenerator,
                                                                 PeriodicGaitGenerator)

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(7.0)


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


# ------------------------------------------------------------------ the host side: E srbd_pgg structs
class HostGenerators:
    """E host generators stepped by the host C functions: the expected state bytes and contact flags."""

    def __init__(self, lib, gaits, duty, freq, H):
        self.lib, self.E, self.H = lib, len(gaits), H
        self.g = (lib.SrbdPgg * self.E)()
        for e in range(self.E):
            assert lib.lib.srbd_pgg_init(C.byref(self.g[e]), int(gaits[e]), float(duty[e]), float(freq[e]), H) == 0

    def bytes(self):
        return bytes(self.g)

    def set_phase_signal(self, phase, init):
        for e in range(self.E):
            ph = np.ascontiguousarray(phase[e], np.float64)
            ini = None if init is None else np.ascontiguousarray(init[e], np.int32)
            assert self.lib.lib.srbd_pgg_set_phase_signal(C.byref(self.g[e]), self.lib.dptr(ph),
                                                          self.lib.iptr(ini)) == 0

    def reset(self):
        for e in range(self.E):
            self.lib.lib.srbd_pgg_reset(C.byref(self.g[e]))

    def run(self, dt, freqs=None):
        out = np.zeros((self.E, 4))
        for e in range(self.E):
            f = self.g[e].step_freq if freqs is None else float(freqs[e])
            assert self.lib.lib.srbd_pgg_run(C.byref(self.g[e]), float(dt), f, self.lib.dptr(out[e])) == 0
        return out.astype(f32)

    def contact_sequence(self, dts, lens):
        """(E, 4, H): the host's sequence; a FULL_STANCE environment's 2 H columns of ones cut to H."""
        H = self.H
        d, l = np.asarray(dts, np.float64), np.asarray(lens, np.int32)
        out = np.zeros((self.E, 4, H), f32)
        buf = np.zeros(8 * H)
        for e in range(self.E):
            cols = self.lib.lib.srbd_pgg_contact_sequence(C.byref(self.g[e]), self.lib.dptr(d), self.lib.iptr(l),
                                                          d.size, self.lib.dptr(buf), buf.size)
            assert cols == (2 * H if self.g[e].gait_type == FULL_STANCE else H)
            out[e] = buf[:4 * cols].reshape(4, cols)[:, :H]
        return out


def environments(E, gait0, seed):
    """Per environment: the eight gait types walked with stride 3 from gait0, its own duty factor and frequency."""
    rng = np.random.default_rng(seed)
    gaits = np.array([(gait0 + 3 * e) % 8 for e in range(E)], np.int32)
    return gaits, rng.uniform(0.5, 0.8, E), rng.uniform(1.0, 2.6, E), rng


def dts_of(kind, H):
    if kind == "uniform":
        return [0.02], [H]
    if kind == "c5":  # the C5 fixture's non-uniform discretisation: two fine steps, then the MPC's dt
        return [0.01, 0.02], [2, H]
    assert kind == "per_step"  # n_dts = H: one step per segment
    return list(0.005 * (1 + np.arange(H) % 7)), list(range(1, H + 1))


def same_state(gen, host, what):
    got = bytes(gen.state_dict())
    assert got == host.bytes(), f"generator state differs from the host's after {what}"


# E: a partial wave, a partial block, more than one block; H: 1, the generic 10, 12, the maximum;
# the stride H or H + 3; dt 0.002 (the simulation's) and 0.02 (the MPC's); step frequencies given and NULL
LOOPS = [
    ("e1_trot_h12", 1, 0, 12, 0, 0.02, False, "uniform"),
    ("e1_full_stance_h32", 1, 7, 32, 3, 0.002, True, "per_step"),
    ("e5_h1", 5, 7, 1, 3, 0.02, True, "uniform"),
    ("e5_h10", 5, 1, 10, 0, 0.002, False, "c5"),
    ("e67_h10", 67, 7, 10, 3, 0.02, False, "per_step"),
    ("e67_h32", 67, 2, 32, 0, 0.002, True, "c5"),
    ("e300_h12", 300, 7, 12, 3, 0.02, True, "c5"),
    ("e300_h12_sim_dt", 300, 0, 12, 0, 0.002, False, "uniform"),
    ("e300_h32", 300, 5, 32, 3, 0.02, False, "per_step"),
]


@pytest.mark.parametrize("name,E,gait0,H,pad,dt,given,kind", LOOPS, ids=[c[0] for c in LOOPS])
def test_forty_steps_of_run_and_contact_sequence(lib, name, E, gait0, H, pad, dt, given, kind):
    gaits, duty, freq, rng = environments(E, gait0, seed=E + H)
    host = HostGenerators(lib, gaits, duty, freq, H)
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    same_state(gen, host, "construction")
    # the start-up hold on some legs of some environments, at phases below and above their offsets
    phase = rng.uniform(0.0, 1.0, (E, 4))
    init = (rng.uniform(0.0, 1.0, (E, 4)) < 0.4).astype(np.int32) * rng.integers(1, 3, (E, 4)).astype(np.int32)
    host.set_phase_signal(phase, init)
    gen.set_phase_signal(phase, init)
    same_state(gen, host, "set_phase_signal")
    freqs = rng.uniform(1.0, 2.6, E) if given else None
    d_freqs = torch.from_numpy(freqs).cuda() if given else None
    dts, lens = dts_of(kind, H)
    buf = torch.full((E, 4, H + pad), float(SENTINEL), dtype=torch.float32, device="cuda")
    held, released, wrapped = 0, 0, 0
    for step in range(40):
        before = np.array([list(g.phase_signal) for g in host.g])
        want = host.run(dt, freqs)
        got = gen.run(dt, d_freqs)
        assert got.dtype == torch.float32 and tuple(got.shape) == (E, 4)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"run, step {step}")
        same_state(gen, host, f"run {step}")
        inits = np.array([list(g.init) for g in host.g])
        held += int((inits != 0).sum())
        released += int(((init != 0) & (inits == 0)).sum()) if step == 39 else 0
        wrapped += int((np.array([list(g.phase_signal) for g in host.g]) < before).sum())
        want_seq = host.contact_sequence(dts, lens)
        out = gen.compute_contact_sequence(dts, lens, out=buf)
        assert out is buf
        seq = buf.cpu().numpy()
        np.testing.assert_array_equal(seq[:, :, :H], want_seq, err_msg=f"contact sequence, step {step}")
        assert np.all(seq[:, :, H:] == SENTINEL), "columns at and beyond H were written"
        same_state(gen, host, f"contact sequence {step}")
    full = np.flatnonzero(gaits == FULL_STANCE)
    for e in full:  # reset by its contact sequence: the phases are the offsets again, the holds cleared
        assert list(host.g[e].phase_signal) == list(host.g[e].phase_offset) and not any(host.g[e].init)
    if E >= 67:  # what the loop is there to cover did occur (host values)
        assert full.size and held and released and (wrapped or dt < 0.01)
        assert len(set(gaits.tolist())) == 8


def test_allocated_sequence_and_reset(lib):
    E, H = 5, 12
    gaits, duty, freq, rng = environments(E, 3, seed=3)
    host = HostGenerators(lib, gaits, duty, freq, H)
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    for _ in range(3):
        host.run(0.02)
        gen.run(0.02)
    seq = gen.compute_contact_sequence([0.02], [H])
    assert tuple(seq.shape) == (E, 4, H) and seq.dtype == torch.float32 and seq.is_contiguous()
    np.testing.assert_array_equal(seq.cpu().numpy(), host.contact_sequence([0.02], [H]))
    same_state(gen, host, "three runs and a sequence")
    host.reset()
    gen.reset()
    same_state(gen, host, "reset")
    np.testing.assert_array_equal(gen.phase_signal.cpu().numpy(), [list(g.phase_signal) for g in host.g])
    np.testing.assert_array_equal(gen.init.cpu().numpy(), np.zeros((E, 4), np.int32))
    with pytest.raises(IndexError):  # the reference's loop would run past its dts
        gen.compute_contact_sequence([0.02], [5])
    same_state(gen, host, "a refused sequence")


def test_large_and_exact_increments(lib):
    """dt * step_freq = 2.5 (more than two wraps in one step), an increment that lands exactly on 1.0 (Python's
    1.0 % 1.0 = 0.0), and a negative dt (the remainder takes the divisor's sign)."""
    E, H = 5, 12
    gaits = np.array([0, 1, 2, 3, 4], np.int32)
    duty = np.full(E, 0.6)
    freq = np.array([125.0, 25.0, 1.4, 2.0, 1.7])
    assert 0.02 * freq[0] == 2.5 and 0.02 * freq[1] == 0.5
    host = HostGenerators(lib, gaits, duty, freq, H)
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    phase = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.5, 0.0, 0.25], [0.0, 0.01, 0.5, 0.99], [0.3, 0.3, 0.3, 0.3],
                      [0.75, 0.5, 0.25, 0.0]])
    host.set_phase_signal(phase, None)
    gen.set_phase_signal(phase)
    zeros = 0
    for step, dt in enumerate([0.02, 0.02, -0.02, 0.02, -0.02, -0.02]):
        want = host.run(dt)
        np.testing.assert_array_equal(gen.run(dt).cpu().numpy(), want, err_msg=f"step {step}")
        same_state(gen, host, f"run {step}")
        zeros += int(sum(p == 0.0 for p in host.g[1].phase_signal))
        np.testing.assert_array_equal(gen.compute_contact_sequence([0.02], [H]).cpu().numpy(),
                                      host.contact_sequence([0.02], [H]))
        same_state(gen, host, f"contact sequence {step}")
    assert zeros >= 2  # 0.5 + 0.5 did land on 1.0 -> 0.0


def test_explicit_null_stream_handle(lib):
    """The C calls with the legacy null stream named by its handle (hipStreamLegacy) and by NULL."""
    E, H = 5, 10
    gaits, duty, freq, _ = environments(E, 0, seed=9)
    host = HostGenerators(lib, gaits, duty, freq, H)
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    out = torch.zeros((E, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for handle in (C.c_void_p(1), None):
        assert lib.lib.srbd_pgg_run_device(gen.state.data_ptr(), E, 0.02, None, out.data_ptr(), handle) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), host.run(0.02))
        same_state(gen, host, "run on the null stream")


# ------------------------------------------------------------------ prepare_state
def contact_patterns(E):
    """(previous, current) of leg l of environment e walks stance->stance, stance->swing (lift-off),
    swing->stance, swing->swing: with E >= 4 every leg sees all four."""
    k = (np.arange(E)[:, None] + np.arange(4)[None, :]) % 4
    prev = np.isin(k, (0, 1)).astype(f32)
    cur = np.isin(k, (0, 2)).astype(f32)
    return prev, cur


def host_prepare(lib, state_in, ref_in, cur, prev, ppl, best):
    E = state_in.shape[0]
    states, refs = np.zeros((E, 24)), np.zeros((E, 24))
    best = None if best is None else best.copy()
    for e in range(E):
        row = None if best is None else np.ascontiguousarray(best[e, :4 * ppl])
        rc = lib.lib.srbd_prepare_state(lib.dptr(np.ascontiguousarray(state_in[e])),
                                        lib.dptr(np.ascontiguousarray(ref_in[e])),
                                        lib.dptr(cur[e].astype(np.float64)), lib.dptr(prev[e].astype(np.float64)),
                                        ppl, lib.fptr(row), lib.dptr(states[e]), lib.dptr(refs[e]))
        assert rc == 0
        if best is not None:
            best[e, :4 * ppl] = row
    return states.astype(f32), refs.astype(f32), best


# params_per_leg / P of zero-order H12, linear S2, cubic S2 H16, and a P with entries past the four legs'
PARAMS = [(36, 144), (9, 36), (24, 96), (9, 41)]


@pytest.mark.parametrize("ppl,P", PARAMS, ids=[f"ppl{a}_p{b}" for a, b in PARAMS])
@pytest.mark.parametrize("E", [1, 5, 67, 300])
def test_prepare_state_bit_equal(lib, E, ppl, P):
    rng = np.random.default_rng(100 * E + P)
    state_in = rng.standard_normal((E, 24)) * 10.0 ** rng.integers(-3, 3, (E, 24))
    ref_in = rng.standard_normal((E, 24))
    nan_env = E // 2
    if E > 1:
        state_in[nan_env, 4] = np.nan  # stays in its environment
        state_in[E - 1, 1] = 1e-40     # below float32's normal range: the cast's subnormal
        ref_in[E - 1, 20] = -3e-42
    prev, cur = contact_patterns(E)
    best = (rng.standard_normal((E, P)) + 3.0).astype(f32)
    want_s, want_r, want_b = host_prepare(lib, state_in, ref_in, cur, prev, ppl, best)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
         dict(state_in=state_in, ref_in=ref_in, cur=cur, prev=prev, best=best).items()}
    for with_best in (True, False):
        best_t = d["best"].clone() if with_best else None
        states, refs = lib.prepare_state_device(d["state_in"], d["ref_in"], d["cur"], d["prev"],
                                                ppl if with_best else 0, best_t)
        for got, want, what in ((states, want_s, "states"), (refs, want_r, "refs")):
            got = got.cpu().numpy()
            assert got.dtype == f32 and got.shape == (E, 24)
            np.testing.assert_array_equal(got, want, err_msg=what)
            assert got.tobytes() == want.tobytes(), what
        if with_best:
            np.testing.assert_array_equal(best_t.cpu().numpy(), want_b)
    # the cases are in the inputs: swing feet replaced, lift-off legs zeroed and nothing else
    lift = (prev == 1) & (cur == 0)
    assert lift.any() and (want_b[:, :4 * ppl].reshape(E, 4, ppl) == 0).all(axis=2).tolist() == lift.tolist()
    assert (want_b[:, 4 * ppl:] != 0).all()
    if E > 1:
        assert np.isnan(want_s[nan_env, 4]) and np.isfinite(np.delete(want_s, nan_env, axis=0)).all()
        assert want_s[E - 1, 1] != 0 and abs(want_s[E - 1, 1]) < np.finfo(f32).tiny


# ------------------------------------------------------------------ streams
def test_producers_on_a_side_stream_behind_a_fill(lib):
    """The three launches enqueued on a side stream right behind a fill kernel of their output buffer, with no
    synchronisation in between: stream order alone makes the result the host's."""
    E, H, pad, ppl, P = 67, 12, 3, 36, 144
    gaits, duty, freq, rng = environments(E, 7, seed=21)
    host = HostGenerators(lib, gaits, duty, freq, H)
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    state_in, ref_in = rng.standard_normal((E, 24)), rng.standard_normal((E, 24))
    best = (rng.standard_normal((E, P)) + 3.0).astype(f32)
    prev = rng.integers(0, 2, (E, 4)).astype(f32)
    d_state, d_ref = torch.from_numpy(state_in).cuda(), torch.from_numpy(ref_in).cuda()
    d_best, d_prev = torch.from_numpy(best).cuda(), torch.from_numpy(prev).cuda()
    buf = torch.zeros((E, 4, H + pad), dtype=torch.float32, device="cuda")
    flags = torch.zeros((E, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf.fill_(float(SENTINEL))
        flags.fill_(float(SENTINEL))
        got_run = lib.pgg_run_device(gen.state, 0.02, out=flags, stream=side)
        gen.compute_contact_sequence([0.01, 0.02], [2, H], out=buf, stream=side)
        cur = buf[:, :, 0].contiguous()
        states, refs = lib.prepare_state_device(d_state, d_ref, cur, d_prev, ppl, d_best, stream=side)
    side.synchronize()
    want_run = host.run(0.02)
    want_seq = host.contact_sequence([0.01, 0.02], [2, H])
    want_s, want_r, want_b = host_prepare(lib, state_in, ref_in, want_seq[:, :, 0], prev, ppl, best)
    np.testing.assert_array_equal(got_run.cpu().numpy(), want_run)
    seq = buf.cpu().numpy()
    np.testing.assert_array_equal(seq[:, :, :H], want_seq)
    assert np.all(seq[:, :, H:] == SENTINEL)
    np.testing.assert_array_equal(states.cpu().numpy(), want_s)
    np.testing.assert_array_equal(refs.cpu().numpy(), want_r)
    np.testing.assert_array_equal(d_best.cpu().numpy(), want_b)
    same_state(gen, host, "the side stream's run and sequence")


# ------------------------------------------------------------------ end to end
STATE_KEYS = ("position", "linear_velocity", "orientation", "angular_velocity", "foot_FL", "foot_FR", "foot_RL",
              "foot_RR")
REF_KEYS = ("ref_position", "ref_linear_velocity", "ref_orientation", "ref_angular_velocity", "ref_foot_FL",
            "ref_foot_FR", "ref_foot_RL", "ref_foot_RR")


def config_with(**mpc):
    cfg = types.ModuleType("producers_device_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, **mpc)
    return cfg


def test_device_loop_equals_host_loop(lib):
    """run -> contact sequence -> prepare_state_and_reference_device -> compute_control_device for six steps with
    nothing read back in between, against E host PeriodicGaitGenerator objects, the host
    prepare_state_and_reference and compute_control: every output of every step, bit for bit."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.synthetic import CONFIGS, reference, robot_state

    E, N, H, steps, dt = 5, 256, 12, 6, 0.02
    cfg = config_with(num_parallel_computations=N, horizon=H, sampling_method="mppi",
                      control_parametrization="zero_order", shift_solution=False, rng="philox", device_id=0)
    on_dev, on_host = Batched_Sampling_MPC(E, cfg), Batched_Sampling_MPC(E, cfg)
    assert on_dev.num_control_parameters == 144 and on_dev.num_control_parameters_single_leg == 36
    robot = CONFIGS["c2"].robot
    gaits = [0, 1, 2, 7, 3]  # trot, pace, bounding, full stance, crawl
    duty, freq = [0.65, 0.7, 0.65, 0.65, 0.8], [1.4, 2.0, 2.4, 1.4, 1.0]
    start = np.array([[0.62, 0.1, 0.1, 0.6], [0.68, 0.3, 0.66, 0.3], [0.5, 0.5, 0.63, 0.6], [0.0, 0.5, 0.5, 0.0],
                      [0.78, 0.25, 0.75, 0.5]])  # legs about to pass their duty factor: lift-offs within the steps
    pggs = [PeriodicGaitGenerator(duty[e], freq[e], gaits[e], H) for e in range(E)]
    for e in range(E):
        pggs[e].set_phase_signal(start[e])
    gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
    gen.set_phase_signal(start)
    try:
        rng = np.random.default_rng(5)
        state_in = np.stack([[robot_state(robot, 10 * k + e) for e in range(E)] for k in range(steps)])
        ref_in = np.stack([[reference(robot, s) for s in state_in[k]] for k in range(steps)])
        ref_in[:, :, 12:] += rng.uniform(-0.05, 0.05, (steps, E, 12))  # the swing feet's substitution shows
        # the host loop
        want, lifts = [], 0
        previous = np.ones((E, 4))
        on_host.best_control_parameters = (rng.standard_normal((E, 144)) * 0.5).astype(f32)
        best0 = on_host.best_control_parameters.copy()
        for k in range(steps):
            seqs = []
            for e in range(E):
                pggs[e].run(dt, pggs[e].step_freq)
                seqs.append(pggs[e].compute_contact_sequence([dt], [H])[:, :H])
            seqs = np.stack(seqs)
            current = seqs[:, :, 0].copy()
            lifts += int(((previous == 1) & (current == 0)).sum())
            sd = [dict(zip(STATE_KEYS, state_in[k, e].reshape(8, 3))) for e in range(E)]
            rd = [dict(zip(REF_KEYS, ref_in[k, e].reshape(8, 3))) for e in range(E)]
            states, refs = on_host.prepare_state_and_reference(sd, rd, current, previous)
            zeroed = on_host.best_control_parameters.copy()
            on_host.with_newkey()
            keys = np.array(on_host.get_key())
            out = on_host.compute_control(states, refs, seqs, on_host.best_control_parameters, keys)
            on_host.best_control_parameters = out[3]
            want.append(dict(seq=seqs.astype(f32), states=states.astype(f32), refs=refs.astype(f32), zeroed=zeroed,
                             keys=keys.copy(), grf=out[0], pred=out[2], best=out[3].copy(), cost=out[4],
                             pgg=b"".join(bytes(p._g) for p in pggs)))
            previous = current
        assert lifts >= 3, "the scenario must contain lift-offs"
        # the device loop: everything uploaded first, then six steps enqueued with no synchronisation
        d_state, d_ref = torch.from_numpy(state_in).cuda(), torch.from_numpy(ref_in).cuda()
        d_keys = torch.from_numpy(np.stack([w["keys"] for w in want]).astype(np.uint64).view(np.int64)).cuda()
        best_t = torch.from_numpy(best0).cuda()
        d_prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got = []
        for k in range(steps):
            gen.run(dt)
            seq = gen.compute_contact_sequence([dt], [H])
            current = seq[:, :, 0].contiguous()
            states, refs = on_dev.prepare_state_and_reference_device(d_state[k], d_ref[k], current, d_prev,
                                                                     best_control_parameters=best_t)
            zeroed = best_t.clone()
            out = on_dev.compute_control_device(states, refs, seq, best_t, d_keys[k])
            assert out[3] is best_t
            got.append(dict(seq=seq, states=states, refs=refs, zeroed=zeroed, grf=out[0], pred=out[2],
                            best=best_t.clone(), cost=out[4], pgg=gen.state.clone()))
            d_prev = current
        torch.cuda.synchronize()
        for k in range(steps):
            for name in ("seq", "states", "refs", "zeroed", "grf", "pred", "best", "cost"):
                g, w = got[k][name].cpu().numpy(), np.asarray(want[k][name])
                assert g.dtype == w.dtype and g.shape == w.shape, f"step {k} {name}"
                np.testing.assert_array_equal(g, w, err_msg=f"step {k} {name}")
            assert got[k]["pgg"].cpu().numpy().tobytes() == want[k]["pgg"], f"step {k}: generator state"
    finally:
        on_dev.close()
        on_host.close()


def test_device_generators_match_reference_recording(lib):
    """srbd_pgg_run_device / srbd_pgg_contact_sequence_device, E = 8 with one gait type each, against
    tests/golden/pgg_ref.npz (the reference's numpy PeriodicGaitGenerator, recorded).  Exact equality."""
    import os

    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgg_ref.npz"),
                     allow_pickle=False))
    E, H = 8, 12
    params = np.stack([g[f"gait{e}_params"] for e in range(E)])
    gen = BatchedPeriodicGaitGenerator(E, params[:, 0], params[:, 1], np.arange(E, dtype=np.int32), H)
    runs = np.stack([g[f"gait{e}_runs"] for e in range(E)], axis=2)              # (60, 5, E, 4)
    want = {"uniform": np.stack([g[f"gait{e}_uniform"][:, :, :H] for e in range(E)], axis=1),
            "nonuniform": np.stack([g[f"gait{e}_nonuniform"][:, :, :H] for e in range(E)], axis=1)}
    got_runs, got = [], {"uniform": [], "nonuniform": []}
    for k in range(60):
        got_runs.append([gen.run(0.002) for _ in range(5)])
        got["uniform"].append(gen.compute_contact_sequence([0.02], [H]))
        got["nonuniform"].append(gen.compute_contact_sequence([0.01, 0.02], [2, H]))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.stack([torch.stack(r) for r in got_runs]).cpu().numpy(), runs.astype(f32))
    for kind in want:
        np.testing.assert_array_equal(torch.stack(got[kind]).cpu().numpy(), want[kind].astype(f32), err_msg=kind)
