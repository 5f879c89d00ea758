"""The device-resident swing reflexes (srbd_reflex_step_device; BatchedReflexSwingTrajectoryController) against the
host function srbd_reflex_step (include/srbd_host.h), which tests/test_reflex_host.py pins to the recorded reference.
The contract is bit equality -- both structs' bytes after every tick and all six outputs -- so every comparison is
exact and no tolerance appears here.  Expected values never come from the device path."""
import ctypes as C

import numpy as np
import pytest
import torch

from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedReflexSwingTrajectoryController

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 7.0
DT = 0.02
INTERVAL = 0.03
TICKS = 40
SMALL, LARGE = 0.004, 0.15  # scripted foot errors: far below both trigger thresholds, far above both
INPUTS = ("jac", "jac_dot", "mass_matrix", "q_dot", "foot_pos", "foot_vel", "qfrc_passive", "qfrc_bias", "grfs",
          "lift_off", "touch_down")
VECTORS = ("tau", "des_foot_pos", "des_foot_vel", "des_joint_vel")
FLAGS = ("apex", "full_stance")


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


class Host:
    """E host (srbd_stc, srbd_reflex) pairs stepped by srbd_reflex_step: the expected bytes and outputs.  An environment
    the host call refuses keeps its bytes and the sentinel in its output rows."""

    def __init__(self, lib, E, seed):
        rng = np.random.default_rng(seed)
        self.lib, self.E, self.rng = lib, E, rng
        self.period = np.array([0.23, 0.3, 0.37])[np.arange(E) % 3] + rng.uniform(0.0, 0.015, E)
        self.g, self.r = (lib.SrbdStc * E)(), (lib.SrbdReflex * E)()
        for e in range(E):
            assert lib.lib.srbd_stc_init(C.byref(self.g[e]), rng.uniform(0.04, 0.08), self.period[e],
                                         rng.uniform(100, 800), rng.uniform(2, 30), e % 2) == 0
            self.g[e].use_feedback_linearization = int(e % 5 != 3)
            self.g[e].use_friction_compensation = int(e % 7 != 4)
            mode = lib.REFLEX_OFF if e % 11 == 5 else lib.REFLEX_TRACKING
            assert lib.lib.srbd_reflex_init(C.byref(self.r[e]), rng.uniform(0.1, 0.2), e % 2, mode,
                                            int(e % 3 == 0)) == 0
        self.refused = set()

    def refuse(self, e, how):
        if how == "period":
            self.g[e].swing_period = 0.0
        else:
            self.r[e].trigger_mode = self.lib.REFLEX_GEOM_CONTACT
        self.refused.add(e)

    def last_des(self):
        return np.array([[row[:] for row in r.last_des_foot_pos] for r in self.r])

    def step(self, x, previous, dt=DT, interval=INTERVAL):
        p, E = self.lib.dptr, self.E
        out = {k: np.full((E, 4, 3), SENTINEL) for k in VECTORS}
        out.update({k: np.full(E, int(SENTINEL), np.int32) for k in FLAGS})
        contact, prev = x["contact"].astype(np.float64), previous.astype(np.float64)
        for e in range(E):
            io = self.lib.SrbdStcIo(apex_interval=interval, contact=p(contact[e]),
                                    apex=self.lib.iptr(out["apex"][e:e + 1]),
                                    full_stance=self.lib.iptr(out["full_stance"][e:e + 1]),
                                    **{k: p(x[k][e]) for k in INPUTS}, **{k: p(out[k][e]) for k in VECTORS})
            rc = self.lib.lib.srbd_reflex_step(C.byref(self.g[e]), C.byref(self.r[e]), C.byref(io), p(prev[e]), dt)
            assert rc == (self.lib.E_INVALID if e in self.refused else 0), e
        return out


def contacts(E, k):
    """Tick k's contact flags: legs (0, 3) and (1, 2) swing in turn, 12 ticks each with two ticks of full stance
    between, environment e running the script shifted by 3 e ticks -- so a wave holds stance legs, legs in the
    detection window, legs inside the last 0.07 s and clocks past the shorter periods at once."""
    phase = (k + 3 * np.arange(E)) % 28
    c = np.ones((E, 4), f32)
    a, b = phase < 12, (phase >= 14) & (phase < 26)
    c[a, 0] = c[a, 3] = 0.0
    c[b, 1] = c[b, 2] = 0.0
    return c


def draw_inputs(host, k, nan_env=None):
    """One tick's inputs.  The feet are the desired positions the previous tick wrote minus a scripted error: large
    -- a hit candidate -- in leg (e + k // 5) % 4 of environment e at the ticks k % 5 == e % 5, and in a second leg of
    every fourth environment in the same tick (two legs that would trigger together)."""
    rng, E = host.rng, host.E
    a = rng.standard_normal((E, 4, 3, 3)) * 0.1
    lift = np.array([[0.3, 0.2, 0.0], [0.3, -0.2, 0.0], [-0.3, 0.2, 0.0], [-0.3, -0.2, 0.0]]) + \
        rng.uniform(-0.01, 0.01, (E, 4, 3))
    length = np.full((E, 4), SMALL)
    for e in range(E):
        if k % 5 == e % 5:
            length[e, (e + k // 5) % 4] = LARGE
            if e % 4 == 1:
                length[e, (e + k // 5 + 1) % 4] = LARGE
                length[e, (e + k // 5 + 3) % 4] = LARGE
    d = rng.standard_normal((E, 4, 3))
    feet = host.last_des() - length[..., None] * d / np.linalg.norm(d, axis=-1, keepdims=True)
    x = dict(jac=rng.standard_normal((E, 4, 3, 3)) * 0.25, jac_dot=rng.standard_normal((E, 4, 3, 3)) * 0.5,
             mass_matrix=a @ a.transpose(0, 1, 3, 2) + 0.05 * np.eye(3), q_dot=rng.standard_normal((E, 4, 3)) * 6.0,
             foot_pos=feet, foot_vel=rng.standard_normal((E, 4, 3)) * 0.5,
             qfrc_passive=rng.standard_normal((E, 4, 3)) * 0.3, qfrc_bias=rng.standard_normal((E, 4, 3)) * 2.0,
             grfs=rng.standard_normal((E, 4, 3)) * 40.0, lift_off=lift,
             touch_down=lift + np.array([0.07, 0.01, 0.02]) + rng.uniform(-0.005, 0.005, (E, 4, 3)),
             contact=contacts(E, k))
    if nan_env is not None:
        x["foot_pos"][nan_env] = np.nan
        x["q_dot"][nan_env] = np.nan
        if k >= 6:
            x["lift_off"][nan_env, :, 2] = np.nan
            x["grfs"][nan_env] = np.inf
    return x


def upload(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)  # NaNs position for position
    nan = np.isnan(want)  # a NaN's sign and payload are not part of the contract (x86 and the GPU make different ones)
    assert np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes(), what


def same_structs(lib, stc, reflex, host, what):
    """Both device arrays against the host structs, byte for byte; the doubles of a NaN field position for position."""
    for got, want, size, name in ((stc, bytes(host.g), lib.STC_BYTES, "srbd_stc"),
                                  (reflex, bytes(host.r), lib.REFLEX_BYTES, "srbd_reflex")):
        raw = got.cpu().numpy().tobytes()
        if raw == want:
            continue
        a = np.frombuffer(raw, np.uint8).reshape(host.E, size)
        b = np.frombuffer(want, np.uint8).reshape(host.E, size)
        for e in np.flatnonzero((a != b).any(axis=1)):
            ints = 256 if size == lib.REFLEX_BYTES else 0  # the reflex struct's int32 words start at byte 256
            da, db = a[e].view(np.float64), b[e].view(np.float64)
            both_nan = np.repeat(np.isnan(da) & np.isnan(db), 8)
            if ints:
                both_nan[ints:] = False
            assert (a[e] == b[e])[~both_nan].all(), f"{name}[{e}] differs from the host's, {what}"


def args_of(d):
    return (d["jac"], d["jac_dot"], d["q_dot"], d["foot_pos"], d["foot_vel"], d["qfrc_passive"], d["qfrc_bias"],
            d["mass_matrix"], d["grfs"], d["touch_down"], d["contact"])


# a single environment (optional outputs NULL); one quad short of a wave (lift_off through the foothold generator's
# state); a partial last block with mixed quads, a NaN environment, two refused ones, on a side stream
@pytest.mark.parametrize("E", [1, 3, 67])
def test_forty_ticks_bit_equal(lib, E):
    host = Host(lib, E, seed=100 + E)
    nan_env = 7 if E == 67 else None
    if E == 67:
        host.refuse(13, "period")
        host.refuse(29, "geom_contact")
    stc = torch.from_numpy(np.frombuffer(bytes(host.g), np.uint8).reshape(E, lib.STC_BYTES).copy()).cuda()
    reflex = torch.from_numpy(np.frombuffer(bytes(host.r), np.uint8).reshape(E, lib.REFLEX_BYTES).copy()).cuda()
    frg = BatchedFootholdReferenceGenerator(E, 0.4, 0.3, np.zeros((4, 3))) if E == 3 else None
    minimal = E == 1
    guard = {k: torch.full((E + 2, 4, 3), SENTINEL, dtype=torch.float64, device="cuda") for k in VECTORS}
    guard.update({k: torch.full((E + 2,), int(SENTINEL), dtype=torch.int32, device="cuda") for k in FLAGS})
    names = VECTORS[:3] if minimal else tuple(guard)
    out = {k: guard[k][1:E + 1] for k in names}
    stream = torch.cuda.Stream() if E == 67 else None
    previous = np.ones((E, 4), f32)
    hits, flags_on, stale, cycles = np.zeros(4, int), 0, 0, set()
    for k in range(TICKS):
        x = draw_inputs(host, k, nan_env)
        before = np.array([r.early_stance[:] for r in host.r])
        had = np.array([r.has_hitpoint[:] for r in host.r])
        want = host.step(x, previous)
        d = upload(dict(x, previous_contact=previous))
        if frg is not None:
            frg.lift_off_positions.copy_(d["lift_off"])
        torch.cuda.synchronize()
        got = lib.reflex_step_device(stc, reflex, DT, *args_of(d), d["previous_contact"],
                                     lift_off=None if frg is not None else d["lift_off"],
                                     frg=None if frg is None else frg.state, apex_interval=INTERVAL, out=out,
                                     want_joint_vel=not minimal, want_flags=not minimal, stream=stream)
        if stream is not None:
            stream.synchronize()
        assert set(got) == set(names)
        for name in names:
            assert got[name].data_ptr() == out[name].data_ptr()
            same_bits(got[name], want[name], f"{name}, tick {k}")
        same_structs(lib, stc, reflex, host, f"tick {k}")
        for name, t in guard.items():
            edge = t.cpu().numpy()
            assert (edge[0] == SENTINEL).all() and (edge[E + 1] == SENTINEL).all(), f"a guard row of {name} was written"
            if name not in names:
                assert (edge == SENTINEL).all(), f"{name} was written though NULL"
        after = np.array([r.early_stance[:] for r in host.r])
        new = (after == 1) & (before == 0)
        hits += new.sum(axis=0)
        stale += int(((had == 1) & (np.array([r.has_hitpoint[:] for r in host.r]) == 0)).sum())
        flags_on += sum(r.height_enhancement for r in host.r)
        cycles |= {r.gait_cycles for r in host.r}
        assert new.sum(axis=1).max() <= 1, "at most one leg triggers per tick and environment"
        previous = x["contact"]
    assert hits.sum() > 0, "the script must produce hits"
    if E == 67:
        assert (hits > 0).all() and stale > 0 and flags_on > 0 and {-1, 0, 1, 2} <= cycles
        for e in host.refused:  # left as found, rows unwritten
            assert (want["tau"][e] == SENTINEL).all() and list(host.g[e].swing_time) == [0.0] * 4
        swing = x["contact"][nan_env] == 0
        assert np.isnan(want["tau"][nan_env][swing]).all() and np.isfinite(want["tau"][nan_env + 1]).all()
        clocks = np.array([list(g.swing_time) for g in host.g])
        assert (clocks > host.period[:, None]).any(), "a swing clock must pass its period"


def test_nan_environment_changes_nothing_in_its_neighbours(lib):
    E, nan_env = 6, 2
    runs = {}
    for bad in (True, False):
        host = Host(lib, E, seed=77)
        stc = torch.from_numpy(np.frombuffer(bytes(host.g), np.uint8).reshape(E, lib.STC_BYTES).copy()).cuda()
        reflex = torch.from_numpy(np.frombuffer(bytes(host.r), np.uint8).reshape(E, lib.REFLEX_BYTES).copy()).cuda()
        previous, rows = np.ones((E, 4), f32), []
        for k in range(10):
            x = draw_inputs(host, k, nan_env if bad else None)
            host.step(x, previous)
            d = upload(dict(x, previous_contact=previous))
            got = lib.reflex_step_device(stc, reflex, DT, *args_of(d), d["previous_contact"], lift_off=d["lift_off"],
                                         apex_interval=INTERVAL)
            rows.append((stc.cpu().numpy().copy(), reflex.cpu().numpy().copy(),
                         {n: t.cpu().numpy().copy() for n, t in got.items()}))
            previous = x["contact"]
        runs[bad] = rows
    for (s1, r1, o1), (s2, r2, o2) in zip(runs[True], runs[False]):
        keep = np.arange(E) != nan_env
        assert s1[keep].tobytes() == s2[keep].tobytes() and r1[keep].tobytes() == r2[keep].tobytes()
        for n in o1:
            assert o1[n][keep].tobytes() == o2[n][keep].tobytes(), n


def test_class_loop_with_step_frequency_and_masked_reset(lib):
    """BatchedReflexSwingTrajectoryController in a short loop with apply_step_frequency on its srbd_stc state and a
    masked reset of its reflex state, against the host chain srbd_gait_apply_freq -> srbd_reflex_step."""
    E = 5
    host = Host(lib, E, seed=5)
    ctl = BatchedReflexSwingTrajectoryController(E, 0.06, host.period, 500.0, 10.0, reflex_max_step_height=0.15)
    assert tuple(ctl.reflex_state.shape) == (E, lib.REFLEX_BYTES) and tuple(ctl.state.shape) == (E, lib.STC_BYTES)
    st = ctl.state_dict()
    assert set(st) == {"stc", "reflex"} and len(st["stc"]) == E and len(st["reflex"]) == E
    first = bytes(st["reflex"])
    # the host twins of what the constructor built, then both sides loaded with the varied structs of `host`
    for e in range(E):
        g, r = lib.SrbdStc(), lib.SrbdReflex()
        assert lib.lib.srbd_stc_init(C.byref(g), 0.06, host.period[e], 500.0, 10.0, 0) == 0
        assert lib.lib.srbd_reflex_init(C.byref(r), 0.15, 0, lib.REFLEX_TRACKING, 0) == 0
        assert bytes(st["stc"][e]) == bytes(g) and bytes(st["reflex"][e]) == bytes(r)
    for e in range(E):
        st["stc"][e], st["reflex"][e] = host.g[e], host.r[e]
    ctl.load_state_dict(st)
    for half in (st["stc"], bytes(st["stc"]), {"stc": st["stc"]}):  # one half alone is refused, not loaded
        with pytest.raises(ValueError, match="reflex"):
            ctl.load_state_dict(half)
    with pytest.raises(ValueError, match="srbd_reflex structs expected"):
        ctl.load_state_dict({"stc": st["stc"], "reflex": bytes(st["reflex"])[8:]})
    gait = BatchedPeriodicGaitGenerator(E, 0.65, 1.4, 0, 12)
    pgg = gait.state_dict()
    previous, ptrs = np.ones((E, 4), f32), None
    for k in range(24):
        x = draw_inputs(host, k)
        if k in (6, 15):  # wb_interface.py:354-358 ahead of the tick: environments 1 and 3 re-timed
            optimize = np.array([0, 1, 0, 1, 0], np.int32)
            freq = np.array([1.4, 2.0, 1.4, 2.4 if k == 6 else 1.7, 1.4], f32)
            lib.apply_step_frequency(torch.from_numpy(optimize).cuda(), torch.from_numpy(freq).cuda(), gait=gait,
                                     stc=ctl)
            for e in range(E):
                assert lib.lib.srbd_gait_apply_freq(C.byref(pgg[e]), None, C.byref(host.g[e]), int(optimize[e]),
                                                    float(freq[e])) == int(optimize[e])
        if k == 12:  # an episode ends in environments 0 and 3: their reflex structs back to the constructor's bytes
            mask = torch.tensor([True, False, False, True, False]).cuda()
            ctl.reset(mask)
            for e in (0, 3):
                C.memmove(C.byref(host.r[e]), first[e * lib.REFLEX_BYTES:(e + 1) * lib.REFLEX_BYTES], lib.REFLEX_BYTES)
        want = host.step(x, previous)
        d = upload(dict(x, previous_contact=previous))
        got = ctl.step(DT, *args_of(d), d["previous_contact"], lift_off=d["lift_off"], apex_interval=INTERVAL)
        assert [tuple(t.shape) for t in got] == [(E, 4, 3)] * 4 + [(E,)] * 2
        now = [t.data_ptr() for t in got]
        assert ptrs is None or now == ptrs, "the output tensors are allocated once"
        ptrs = now
        for t, name in zip(got, VECTORS + FLAGS):
            same_bits(t, want[name], f"{name}, tick {k}")
        same_structs(lib, ctl.state, ctl.reflex_state, host, f"tick {k}")
        previous = x["contact"]
    assert any(r.has_hitpoint[l] for r in host.r for l in range(4)) or any(r.gait_cycles == 0 for r in host.r)
    saved = ctl.state_dict()
    assert first != bytes(saved["reflex"])
    ctl.reset(torch.ones(E, dtype=torch.bool, device="cuda"))
    assert bytes(ctl.state_dict()["reflex"]) == first  # every environment back to the constructor's bytes
    ctl.load_state_dict({k: bytes(v) for k, v in saved.items()})  # byte strings are taken too
    again = ctl.state_dict()
    assert bytes(again["reflex"]) == bytes(saved["reflex"]) and bytes(again["stc"]) == bytes(saved["stc"])
    with pytest.raises(ValueError, match="cuda"):  # host tensors are refused, not copied
        ctl.step(DT, *[t.cpu() for t in args_of(d)], d["previous_contact"].cpu(), lift_off=d["lift_off"].cpu())
