"""The per-environment reset of the loop's device state (srbd_loop_reset_device; BatchedLoopReset; the ``mask=``
keyword of the two classes' own resets) against the host call srbd_loop_reset (include/srbd_host.h), which
tests/test_loop_reset_host.py pins to the reference's statements and to fresh constructor calls.  The contract is byte
equality, so every comparison is exact and no tolerance appears here.  Expected values never come from the device
path under test."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import config as mirror
from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
from quadruped_pympc_amd.helpers.loop_reset import BatchedLoopReset
from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController
from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

pytestmark = pytest.mark.gpu
f32 = np.float32
DT, H, P = 0.02, 12, 144
DIRTY_STEPS = 45
NAMES = ("pgg", "frg", "stc", "terrain_est", "vfa")


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def struct_types(lib):
    return dict(pgg=lib.SrbdPgg, frg=lib.SrbdFrg, stc=lib.SrbdStc, terrain_est=lib.SrbdTerrainEst, vfa=lib.SrbdVfa)


class World:
    """The five Batched classes of E environments and a BatchedLoopReset built right after them, then dirtied by 45
    steps of the real producers on synthetic inputs: the velocity ring wrapped, swing clocks running, the terrain
    filter moved, step_freq / stance_time / swing_period rewritten by apply_step_frequency for every other
    environment, and vfa.initialized set with held footholds for a third of them."""

    def __init__(self, lib, E, seed=0, steps=DIRTY_STEPS):
        from test_gpu_stc_device import args_of, draw_inputs

        rng = np.random.default_rng(1000 + seed)
        self.lib, self.E = lib, E
        self.gaits = rng.integers(0, 7, E)
        self.duty, self.freq = rng.uniform(0.55, 0.8, E), rng.uniform(1.0, 2.4, E)
        self.period = (1.0 - self.duty) / self.freq
        self.lift = rng.uniform(-0.3, 0.3, (E, 4, 3))
        self.gait = BatchedPeriodicGaitGenerator(E, self.duty, self.freq, self.gaits, H)
        self.frg = BatchedFootholdReferenceGenerator(E, self.duty / self.freq, 0.3, self.lift)
        self.stc = BatchedSwingTrajectoryController(E, 0.06, self.period, 500.0, 10.0)
        self.terr = BatchedTerrainEstimator(E, ref_z=0.3)
        self.vfa = BatchedVisualFootholdAdaptation(E)
        self.vfa.state  # built here, so that the snapshot below holds srbd_vfa_init structs
        self.reset = BatchedLoopReset(E, gait=self.gait, frg=self.frg, stc=self.stc, terrain_est=self.terr,
                                      vfa=self.vfa)
        self.parts = dict(pgg=self.gait, frg=self.frg, stc=self.stc, terrain_est=self.terr, vfa=self.vfa)
        x = draw_inputs(rng, E, 0)
        dyn = {k: cuda(v) for k, v in x.items()}
        base, com = cuda(rng.uniform(-1, 1, (E, 3))), cuda(rng.uniform(-1, 1, (E, 3)))
        yaws, vel = cuda(rng.uniform(-3, 3, E)), cuda(rng.standard_normal((E, 3)) * 0.3)
        ref_vel, ang = cuda(np.tile([0.4, 0.0, 0.0], (E, 1))), cuda(np.zeros((E, 3)))
        hips, feet = cuda(rng.uniform(-0.4, 0.4, (E, 4, 3))), cuda(rng.uniform(-0.4, 0.4, (E, 4, 3)))
        ref = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
        prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
        for k in range(steps):
            c = self.gait.run(DT)
            seeds = self.frg.step(base, yaws, vel, ref_vel, hips, feet, prev, c, gait=self.gait, ref=ref,
                                  com_height_nominal=0.3)
            self.terr.step(base, com, yaws, ref_vel, ang, ref, frg=self.frg)
            self.stc.step(DT, *args_of(dict(dyn, contact=c, touch_down=seeds)), frg=self.frg)
            if k == 20:
                lib.apply_step_frequency(cuda((np.arange(E) % 2).astype(np.int32)),
                                         cuda(np.where(np.arange(E) % 4 < 2, 2.0, 2.4).astype(f32)), gait=self.gait,
                                         frg=self.frg, stc=self.stc)
            prev = c
        held = self.vfa.state_dict()
        for e in range(0, E, 3):
            held[e].initialized[:] = [1] * 4
            held[e].footholds[:] = rng.uniform(-0.5, 0.5, 12).tolist()
            held[e].valid[:] = [1, 0, 1, 1]
        self.vfa.load_state_dict(held)
        self.stc.rising_edge.copy_(cuda((np.arange(E) % 3 != 0).astype(np.int32)))
        self.prev = prev.clone()
        self.best = cuda(rng.standard_normal((E, P)).astype(f32))
        self.other = cuda(rng.uniform(0, 1, (E, 4)).astype(f32))  # a second contact tensor of the caller's
        torch.cuda.synchronize()
        self.dirty = self.download()
        self.snap = {n: t.cpu().numpy().copy() for n, t in self.reset.snapshots.items()}
        ring = np.frombuffer(self.dirty["frg"].tobytes(), dtype=np.int32).reshape(E, -1)[:, -2:]
        if steps > 20:
            assert (ring[:, 0] == 20).all(), "the velocity ring must have wrapped"
            clocks = np.frombuffer(self.dirty["stc"].tobytes(), dtype=np.float64).reshape(E, -1)[:, -4:]
            assert (clocks != 0).any() or E < 4, "swing clocks must be running"
            assert self.dirty["pgg"].tobytes() != self.snap["pgg"].tobytes()

    def tensors(self):
        return dict({n: p.state for n, p in self.parts.items()}, edge=self.stc.rising_edge, best=self.best,
                    prev=self.prev, other=self.other)

    def download(self):
        return {n: t.cpu().numpy().copy() for n, t in self.tensors().items()}

    def restore(self):
        for n, t in self.tensors().items():
            t.copy_(torch.from_numpy(self.dirty[n]))

    def host(self, mask, feet, skip=(), rows=("prev", "other"), best=True, edge=True):
        """srbd_loop_reset applied per environment to the dirty bytes: the expected bytes of every tensor."""
        lib, want = self.lib, {n: v.copy() for n, v in self.dirty.items()}
        types_ = struct_types(lib)
        for e in np.flatnonzero(mask):
            level = 2 if mask[e] == 2 else 1
            s = {n: types_[n].from_buffer_copy(self.dirty[n][e].tobytes()) for n in NAMES if n not in skip}
            z = {n: types_[n].from_buffer_copy(self.snap[n][e].tobytes()) for n in s}
            ed, be = want["edge"][e:e + 1], want["best"][e]
            args = [C.byref(s[n]) if n in s else None for n in NAMES] + [C.byref(z[n]) if n in z else None for n in NAMES]
            rc = lib.lib.srbd_loop_reset(level, lib.dptr(np.ascontiguousarray(feet[e])), *args,
                                         ed.ctypes.data_as(lib._IP) if edge else None,
                                         be.ctypes.data_as(lib._FP) if best else None, P if best else 0)
            assert rc == lib.OK
            for n in s:
                want[n][e] = np.frombuffer(bytes(s[n]), dtype=np.uint8)
            for r in rows:
                want[r][e] = 1.0
        return want

    def apply(self, mask, feet, skip=(), rows=("prev", "other"), best=True, edge=True, stream=None, feet_t=None,
              snapshots=None):
        """One srbd_loop_reset_device call through _lib on the world's tensors."""
        t = self.tensors()
        states = {n: t[n] for n in NAMES if n not in skip}
        snaps = snapshots or self.reset.snapshots
        self.lib.loop_reset_device(cuda(mask.astype(np.int32)), cuda(feet) if feet_t is None else feet_t,
                                   snapshots={n: snaps[n] for n in states}, rising_edge=t["edge"] if edge else None,
                                   best_params=t["best"] if best else None, contact_rows=[t[r] for r in rows],
                                   stream=stream, **states)


WORLDS = {}


def world(lib, E):
    if E not in WORLDS:
        WORLDS[E] = World(lib, E, seed=E)
    w = WORLDS[E]
    w.restore()
    return w


def masks(E, kind, seed=3):
    if kind == "mixed":
        m = np.random.default_rng(seed).choice([0, 1, 2, 7], E).astype(np.int32)
        if E >= 3:
            m[:3] = [2, 0, 7]  # every level present, the last environment reset
            m[-1] = 2 if E > 3 else m[-1]
        return m
    return np.full(E, dict(zeros=0, ones=1, twos=2)[kind], dtype=np.int32)


def same(got, want, what):
    for n in want:
        assert got[n].tobytes() == want[n].tobytes(), f"{what}: {n} differs from the host's bytes"


CASES = [(E, k) for E in (1, 3, 65) for k in ("zeros", "ones", "twos", "mixed")] + [(4096, "mixed")]


@pytest.mark.parametrize("E,kind", CASES)
def test_device_equals_host(lib, E, kind):
    w = world(lib, E)
    mask = masks(E, kind)
    feet = np.random.default_rng(E).uniform(-0.4, 0.4, (E, 4, 3))
    w.apply(mask, feet)
    torch.cuda.synchronize()
    got = w.download()
    same(got, w.host(mask, feet), f"E={E} {kind}")
    if kind == "zeros":
        same(got, w.dirty, "all zero")
    if kind == "twos":  # the episode reset is the constructor's bytes, whatever the 45 steps left
        for n in ("pgg", "stc", "terrain_est", "vfa"):
            assert got[n].tobytes() == w.snap[n].tobytes(), n
        fresh = BatchedFootholdReferenceGenerator(E, w.duty / w.freq, 0.3, feet)
        assert got["frg"].tobytes() == bytes(fresh.state_dict())
        assert not got["edge"].any() and not got["best"].any() and (got["prev"] == 1).all()


def test_unreset_environments_are_neither_written_nor_read(lib):
    E = 65
    w = world(lib, E)
    mask = masks(E, "mixed")
    off = mask == 0
    assert off.sum() >= 5 and (~off).sum() >= 5
    feet = np.random.default_rng(8).uniform(-0.4, 0.4, (E, 4, 3))
    want = w.host(mask, feet)
    poisoned = feet.copy()
    poisoned[off] = np.nan
    snaps = {n: t.clone() for n, t in w.reset.snapshots.items()}
    for t in snaps.values():
        t[cuda(off)] = 0xFF  # all-ones bytes: NaN in every double
    w.best[cuda(off)] = float("nan")
    dirty_best = w.best.cpu().numpy().copy()
    w.apply(mask, poisoned, snapshots=snaps)
    torch.cuda.synchronize()
    got = w.download()
    for n in got:
        ref = dirty_best if n == "best" else w.dirty[n]
        assert got[n][off].tobytes() == ref[off].tobytes(), f"{n}: an unreset environment's bytes changed"
        assert got[n][~off].tobytes() == want[n][~off].tobytes(), f"{n}: a reset environment differs"
    for n in ("frg", "pgg", "stc", "terrain_est"):  # no NaN reached a reset environment
        assert not np.isnan(np.frombuffer(got[n][~off].tobytes(), dtype=np.float64)).any(), n
    assert not np.isnan(got["best"][~off]).any()


def test_environments_are_independent(lib):
    E = 65
    w = world(lib, E)
    rng = np.random.default_rng(12)
    feet = rng.uniform(-0.4, 0.4, (E, 4, 3))
    a = np.zeros(E, dtype=np.int32)
    a[rng.choice(E, 20, replace=False)] = rng.choice([1, 2], 20)
    both = a.copy()
    free = np.flatnonzero(a == 0)
    both[free[::2]] = rng.choice([1, 2, 7], free[::2].size)
    w.apply(a, feet)
    torch.cuda.synchronize()
    alone = w.download()
    w.restore()
    w.apply(both, feet)
    torch.cuda.synchronize()
    union = w.download()
    sel = a != 0
    for n in alone:
        assert alone[n][sel].tobytes() == union[n][sel].tobytes(), n
    same(alone, w.host(a, feet), "A alone")


@pytest.mark.parametrize("missing", NAMES + ("edge", "best", "rows"))
def test_each_piece_is_optional(lib, missing):
    E = 3
    w = world(lib, E)
    mask = np.array([2, 7, 2], dtype=np.int32)
    feet = np.random.default_rng(4).uniform(-0.4, 0.4, (E, 4, 3))
    kw = dict(skip=(missing,) if missing in NAMES else (), edge=missing != "edge", best=missing != "best",
              rows=() if missing == "rows" else ("prev", "other"))
    w.apply(mask, feet, **kw)
    torch.cuda.synchronize()
    got = w.download()
    same(got, w.host(mask, feet, **kw), f"without {missing}")
    key = dict(edge="edge", best="best", rows="prev").get(missing, missing)
    assert got[key].tobytes() == w.dirty[key].tobytes(), "the piece left out must not change"


def test_class_reset_and_bool_and_int64_masks(lib):
    E = 65
    w = world(lib, E)
    rng = np.random.default_rng(5)
    feet = rng.uniform(-0.4, 0.4, (E, 4, 3))
    mask = masks(E, "mixed")
    w.reset.reset(cuda(mask.astype(np.int64)), cuda(feet), best_control_parameters=w.best,
                  contact_rows=(w.prev, w.other))
    torch.cuda.synchronize()
    same(w.download(), w.host(mask, feet), "int64 mask through the class")
    w.restore()
    flags = mask != 0
    w.reset.reset(cuda(flags), cuda(feet), best_control_parameters=w.best, contact_rows=(w.prev,))
    torch.cuda.synchronize()
    same(w.download(), w.host(flags.astype(np.int32), feet, rows=("prev",)), "bool mask: the reference's level")


def test_own_resets_with_and_without_a_mask(lib):
    """reset(mask=None) keeps the parent's bytes (every environment: phases = offsets, holds cleared; initialized
    cleared); with a mask only the named environments, by the host call's bytes."""
    E = 65
    w = world(lib, E)
    types_ = struct_types(lib)
    w.gait.reset()
    w.vfa.reset()
    torch.cuda.synchronize()
    got = w.download()
    for n, fn in (("pgg", lib.lib.srbd_pgg_reset), ("vfa", lib.lib.srbd_vfa_reset)):
        arr = (types_[n] * E).from_buffer_copy(w.dirty[n].tobytes())
        for e in range(E):
            assert fn(C.byref(arr[e])) == lib.OK
        assert got[n].tobytes() == bytes(arr), n
    for n in ("frg", "stc", "terrain_est", "edge", "best", "prev"):
        assert got[n].tobytes() == w.dirty[n].tobytes(), n
    w.restore()
    mask = masks(E, "mixed")
    w.gait.reset(mask=cuda(mask))
    w.vfa.reset(mask=cuda(mask != 0))
    torch.cuda.synchronize()
    got = w.download()
    one = (mask != 0).astype(np.int32)  # a 2 in the classes' own mask is still the reference's level
    feet = np.zeros((E, 4, 3))
    want = w.host(one, feet, skip=("frg", "stc", "terrain_est"), rows=(), best=False, edge=False)
    same(got, want, "own resets with a mask")


def test_stream_order_and_no_host_wait(lib):
    """The call on a side stream behind an event from a producer (the gait generator's run on another stream) and
    ahead of a consumer (the next run), nothing synchronised in between: the serial run's bytes.  torch's
    synchronisation check is armed around the call: a host wait inside it would raise."""
    E = 65
    w = world(lib, E)
    mask = masks(E, "mixed")
    feet = np.random.default_rng(6).uniform(-0.4, 0.4, (E, 4, 3))
    d_feet = cuda(feet)
    d_mask64 = cuda(mask.astype(np.int64))

    def run(streams):
        w.restore()
        torch.cuda.synchronize()
        a, b = streams
        big = torch.empty(1 << 25, dtype=torch.float64, device="cuda")  # 256 MiB: the fill outlasts the enqueue
        with torch.cuda.stream(a):
            big.fill_(1.0)
            w.gait.run(DT, stream=a)
            done = torch.cuda.Event()
            done.record(a)
        with torch.cuda.stream(b):
            b.wait_event(done)
            torch.cuda.set_sync_debug_mode("error")
            try:
                w.reset.reset(d_mask64, d_feet, best_control_parameters=w.best, contact_rows=(w.prev,), stream=b)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            c = w.gait.run(DT, stream=b)
        torch.cuda.synchronize()
        return dict(w.download(), contact=c.cpu().numpy())

    main = torch.cuda.current_stream()
    serial = run((main, main))
    side = run((torch.cuda.Stream(), torch.cuda.Stream()))
    same(side, serial, "side streams")
    # and the serial run is the host's: run, reset, run
    types_ = struct_types(lib)
    w.restore()
    w.gait.run(DT)
    torch.cuda.synchronize()
    w.dirty, keep = w.download(), w.dirty
    try:
        want = w.host(mask, feet, rows=("prev",))
    finally:
        w.dirty = keep
    arr = (types_["pgg"] * E).from_buffer_copy(want["pgg"].tobytes())
    contact = np.zeros((E, 4))
    for e in range(E):
        assert lib.lib.srbd_pgg_run(C.byref(arr[e]), DT, arr[e].step_freq, lib.dptr(contact[e])) == lib.OK
    assert serial["pgg"].tobytes() == bytes(arr)
    np.testing.assert_array_equal(serial["contact"], contact.astype(f32))
    for n in ("frg", "stc", "terrain_est", "vfa", "edge", "best", "prev"):
        assert serial[n].tobytes() == want[n].tobytes(), n


def config_with(**mpc):
    cfg = types.ModuleType("loop_reset_device_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, **mpc)
    return cfg


def test_episode_equivalence_in_the_closed_loop(lib):
    """45 steps of the device loop, a level-2 reset of a third of the environments with new feet, 30 further steps:
    the reset environments are, bit for bit at every step, freshly constructed classes of exactly those environments
    running the same 30 inputs; the others equal a run with no reset at all."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.synthetic import CONFIGS, reference, robot_state
    from test_gpu_stc_device import args_of, draw_inputs

    E, N, K0, K1 = 6, 64, 45, 30
    A = np.array([1, 4])
    B = np.array([0, 2, 3, 5])
    K = K0 + K1
    cfg = config_with(num_parallel_computations=N, horizon=H, sampling_method="mppi",
                      control_parametrization="zero_order", shift_solution=False, rng="philox", device_id=0)
    robot = CONFIGS["c2"].robot
    rng = np.random.default_rng(77)
    gaits = np.array([0, 1, 0, 5, 0, 2])
    duty, freq = np.array([0.65, 0.7, 0.6, 0.8, 0.65, 0.65]), np.array([1.4, 2.0, 2.0, 1.0, 2.4, 1.4])
    state_in = np.stack([[robot_state(robot, 10 * k + e) for e in range(E)] for k in range(K)])
    ref_in = np.stack([[reference(robot, s) for s in state_in[k]] for k in range(K)])
    hips = state_in[:, :, 12:].reshape(K, E, 4, 3) + rng.uniform(-0.03, 0.03, (K, E, 4, 3))
    hips[..., 2] += 0.3
    lift = state_in[0, :, 12:].reshape(E, 4, 3)
    new_feet = state_in[K0, :, 12:].reshape(E, 4, 3) + rng.uniform(-0.02, 0.02, (E, 4, 3))
    keys = np.stack([np.full((K, E), 99, dtype=np.int64), np.tile(np.arange(1, K + 1)[:, None], (1, E))], axis=2)
    dyn = draw_inputs(rng, E, 0)

    def run(envs, steps, feet0, ctrl, reset_at=None):
        """The loop for the environments `envs` over the input steps `steps`; returns every step's bytes."""
        n = len(envs)
        gait = BatchedPeriodicGaitGenerator(n, duty[envs], freq[envs], gaits[envs], H)
        frg = BatchedFootholdReferenceGenerator(n, duty[envs] / freq[envs], 0.3, feet0[envs])
        stc = BatchedSwingTrajectoryController(n, 0.06, (1.0 - duty[envs]) / freq[envs], 500.0, 10.0)
        terr = BatchedTerrainEstimator(n, ref_z=0.3)
        rst = BatchedLoopReset(n, gait=gait, frg=frg, stc=stc, terrain_est=terr)
        d = {k: cuda(v[envs]) for k, v in dyn.items()}
        best = torch.zeros((n, P), dtype=torch.float32, device="cuda")
        prev = torch.ones((n, 4), dtype=torch.float32, device="cuda")
        rec = []
        for k in steps:
            if k == reset_at:
                m = np.zeros(n, dtype=np.int32)
                m[A] = 2
                rst.reset(cuda(m), cuda(new_feet[envs]), best_control_parameters=best, contact_rows=(prev,))
            s = cuda(state_in[k][envs])
            ref = cuda(ref_in[k][envs])
            gait.run(DT)
            seq = gait.compute_contact_sequence([DT], [H])
            cur = seq[:, :, 0].contiguous()
            seeds = frg.step(s[:, 0:3].contiguous(), s[:, 8].contiguous(), s[:, 3:6].contiguous(),
                             ref[:, 3:6].contiguous(), cuda(hips[k][envs]), s[:, 12:].reshape(n, 4, 3).contiguous(),
                             prev, cur, gait=gait, ref=ref, com_height_nominal=0.3)
            terr.step(s[:, 0:3].contiguous(), s[:, 0:3].contiguous(), s[:, 8].contiguous(),
                      ref_in_t(ref_in[k][envs], 3), ref_in_t(ref_in[k][envs], 9), ref, frg=frg)
            states, refs = ctrl.prepare_state_and_reference_device(s, ref, cur, prev, best_control_parameters=best)
            out = ctrl.compute_control_device(states, refs, seq, best, cuda(keys[k][envs]))
            grf = out[0].double().view(n, 4, 3).contiguous()
            tau = stc.step(DT, *args_of(dict(d, contact=cur, touch_down=seeds, grfs=grf)), frg=frg)[0]
            rec.append([t.clone() for t in (gait.state, frg.state, stc.state, terr.state, ref, out[0], tau, best)])
            prev = cur
        torch.cuda.synchronize()
        return [[t.cpu().numpy() for t in r] for r in rec]

    def ref_in_t(r, o):
        return cuda(r[:, o:o + 3])

    big, small = Batched_Sampling_MPC(E, cfg), Batched_Sampling_MPC(len(A), cfg)
    try:
        everyone = np.arange(E)
        with_reset = run(everyone, range(K), lift, big, reset_at=K0)
        without = run(everyone, range(K), lift, big)
        fresh = run(A, range(K0, K), new_feet, small)
    finally:
        big.close()
        small.close()
    names = ("pgg", "frg", "stc", "terrain_est", "ref", "grf", "tau", "best")
    assert any(np.abs(r[5]).max() > 0 for r in with_reset), "the MPC must return forces"
    for k in range(K):
        for i, n in enumerate(names):
            got, base = with_reset[k][i], without[k][i]
            assert got[B].tobytes() == base[B].tobytes(), f"step {k}: {n} of an unreset environment"
            if k < K0:
                assert got[A].tobytes() == base[A].tobytes(), f"step {k}: {n} before the reset"
            else:
                assert got[A].tobytes() == fresh[k - K0][i].tobytes(), f"step {k}: {n} after the episode reset"
    assert any(with_reset[k][1][A].tobytes() != without[k][1][A].tobytes() for k in range(K0, K)), "the reset must show"
