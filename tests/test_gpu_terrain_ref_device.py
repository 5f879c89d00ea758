"""The device-resident velocity modulator and terrain / reference stage (srbd_vm_modulate_device,
srbd_terrain_ref_step_device; BatchedVelocityModulator, BatchedTerrainEstimator) against the host functions
srbd_vm_modulate, srbd_terrain_estimate and srbd_reference_assemble (include/srbd_host.h), which
tests/test_terrain_host.py pins to the recorded reference.  The contract is bit equality -- the estimator state's bytes
after every step and entries 0..11 of every reference row -- so every comparison is exact and no tolerance appears
here.  Expected values never come from the device path."""
import ctypes as C

import numpy as np
import pytest
import torch

from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
from quadruped_pympc_amd.helpers.velocity_modulator import BatchedVelocityModulator

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 7.0
REF_Z = 0.31
CHN, GRAVITY = 0.3, 9.81
HIPS = np.array([[0.19, 0.11, 0.3], [0.19, -0.11, 0.3], [-0.19, 0.11, 0.3], [-0.19, -0.11, 0.3]])


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


class HostEstimators:
    """E host srbd_terrain_est structs stepped by srbd_terrain_estimate and srbd_reference_assemble."""

    def __init__(self, lib, roll_on, init=None):
        self.lib, self.E = lib, len(roll_on)
        self.g = (lib.SrbdTerrainEst * self.E)()
        for e in range(self.E):
            assert lib.lib.srbd_terrain_est_init(C.byref(self.g[e])) == 0
            self.g[e].roll_activated = int(roll_on[e])
            if init is not None:
                self.g[e].roll, self.g[e].pitch, self.g[e].height = init[e]

    def bytes(self):
        return bytes(self.g)

    def step(self, x, feet, off=None, ref_z=REF_Z):
        """(rows (E, 12), terrain (E, 3)) from the step's inputs and the feet (E, 4, 3) the estimator is given."""
        p, fn = self.lib.dptr, self.lib.lib
        rows, terrain = np.zeros((self.E, 12)), np.zeros((self.E, 3))
        for e in range(self.E):
            g = C.byref(self.g[e])
            assert fn.srbd_terrain_estimate(g, p(x["base_pos"][e]), float(x["yaws"][e]),
                                            p(np.ascontiguousarray(feet[e])), p(terrain[e])) == 0
            assert fn.srbd_reference_assemble(g, ref_z, float(x["base_pos"][e, 2]), float(x["com_pos"][e, 2]),
                                              0.0 if off is None else float(off[e, 2]), p(x["lin"][e]), p(x["ang"][e]),
                                              p(rows[e])) == 0
        return rows, terrain


def host_modulate(lib, x, limit=0.2):
    lo, ao = np.zeros_like(x["lin"]), np.zeros_like(x["ang"])
    for e in range(x["lin"].shape[0]):
        assert lib.lib.srbd_vm_modulate(limit, lib.dptr(x["lin"][e]), lib.dptr(x["ang"][e]), lib.dptr(x["feet"][e]),
                                        lib.dptr(x["hips"][e]), lib.dptr(lo[e]), lib.dptr(ao[e])) == 0
    return lo, ao


def draw_inputs(rng, E):
    """One step's random inputs: feet under the hips on a sloped ground (so both signs of both tests and both sides of
    0.2 are met over the environments), some legs beyond the modulator's 0.2, commands of both signs."""
    base = rng.uniform(-2, 2, (E, 3))
    yaws = rng.uniform(-4.0, 4.0, E)
    c, s = np.cos(yaws)[:, None], np.sin(yaws)[:, None]
    local = HIPS[None, :, 0:2] + rng.uniform(-0.15, 0.15, (E, 4, 2))
    slope = rng.uniform(-1.5, 1.5, (E, 1, 2))
    feet = np.empty((E, 4, 3))
    feet[..., 0] = base[:, None, 0] + c * local[..., 0] - s * local[..., 1]
    feet[..., 1] = base[:, None, 1] + s * local[..., 0] + c * local[..., 1]
    feet[..., 2] = (slope * local).sum(-1) + rng.uniform(-0.02, 0.02, (E, 4))
    hips = np.empty((E, 4, 3))
    hips[..., 0] = base[:, None, 0] + c * HIPS[None, :, 0] - s * HIPS[None, :, 1]
    hips[..., 1] = base[:, None, 1] + s * HIPS[None, :, 0] + c * HIPS[None, :, 1]
    hips[..., 2] = base[:, None, 2]
    return dict(base_pos=base, com_pos=base + rng.uniform(-0.03, 0.03, (E, 3)), yaws=yaws,
                lin=rng.uniform(-0.3, 0.6, (E, 3)), ang=rng.uniform(-1, 1, (E, 3)), feet=feet, hips=hips)


def upload(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)  # NaNs position for position
    nan = np.isnan(want)  # a NaN's sign and payload are not part of the contract (x86 and the GPU make different ones)
    assert np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes(), what


def same_state(lib, est, host, what):
    """The struct bytes, the three doubles' NaNs compared by position."""
    got = np.frombuffer(bytes(est.state_dict()), dtype=np.float64).reshape(-1, 4)
    want = np.frombuffer(host.bytes(), dtype=np.float64).reshape(-1, 4)
    same_bits(got[:, :3].copy(), want[:, :3].copy(), f"filter words after {what}")
    assert got[:, 3].tobytes() == want[:, 3].tobytes(), f"switches after {what}"


def estimators(lib, E, seed):
    rng = np.random.default_rng(seed)
    roll_on = np.arange(E) % 3 == 1
    est = BatchedTerrainEstimator(E, REF_Z, roll_activated=roll_on)
    st = est.state_dict()
    init = np.stack([rng.uniform(-0.4, 0.4, E), rng.uniform(-0.4, 0.4, E), rng.uniform(-0.1, 0.3, E)], axis=1)
    init[np.arange(E) % 4 == 0] = 0.0  # some from the constructor's zeros
    for e in range(E):
        st[e].roll, st[e].pitch, st[e].height = init[e]
    est.load_state_dict(st)
    host = HostEstimators(lib, roll_on, init)
    assert bytes(est.state_dict()) == host.bytes(), "construction"
    return est, host, rng


# a single environment, a partial quad group, one environment past a wave (a partial block), sixteen full blocks
@pytest.mark.parametrize("E", [1, 3, 65, 4096])
def test_eight_steps_bit_equal(lib, E):
    est, host, rng = estimators(lib, E, seed=E)
    guard = torch.full((E + 2, 24), SENTINEL, dtype=torch.float64, device="cuda")
    tguard = torch.full((E + 2, 3), SENTINEL, dtype=torch.float64, device="cuda")
    ref, tout = guard[1:E + 1], tguard[1:E + 1]
    with_off = E != 3  # com_pos_offset_w NULL at E = 3
    pitches = []
    for k in range(8):
        x = draw_inputs(rng, E)
        off = rng.uniform(-0.02, 0.02, (E, 3)) if with_off else None
        if k == 2:  # a zero denominator (environment 0) -- pi / 2
            x["base_pos"][0], x["yaws"][0] = 0.0, 0.0
            x["feet"][0, 0, 0], x["feet"][0, 2, 0] = 0.0, 0.001
        want, want_t = host.step(x, x["feet"], off)
        d = upload(x)
        est.step(d["base_pos"], d["com_pos"], d["yaws"], d["lin"], d["ang"], ref, lift_off=d["feet"],
                 com_pos_offset_w=None if off is None else torch.from_numpy(off).cuda(), out=tout)
        g = guard.cpu().numpy()
        same_bits(g[1:E + 1, :12].copy(), want, f"ref 0..11, step {k}")
        assert (g[1:E + 1, 12:] == SENTINEL).all() and (g[0] == SENTINEL).all() and (g[-1] == SENTINEL).all()
        tg = tguard.cpu().numpy()
        same_bits(tg[1:E + 1].copy(), want_t, f"terrain, step {k}")
        assert (tg[0] == SENTINEL).all() and (tg[-1] == SENTINEL).all()
        same_state(lib, est, host, f"step {k}")
        pitches.append(want_t[:, 1])
    p = np.concatenate(pitches)
    if E >= 65:  # the inputs reach both quirks' two sides
        assert (p > 0).any() and (p <= 0).any() and (np.abs(p) > 0.2).any() and (np.abs(p) <= 0.2).any()


def test_nan_environment_changes_nothing_in_its_neighbours(lib):
    E, bad = 9, 4
    est_a, host, rng = estimators(lib, E, seed=77)
    est_b, _, _ = estimators(lib, E, seed=77)
    ref_a = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    ref_b = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    for k in range(3):
        x = draw_inputs(rng, E)
        y = {n: v.copy() for n, v in x.items()}
        y["feet"][bad] = np.nan
        want, _ = host.step(y, y["feet"])
        a, b = upload(x), upload(y)
        est_a.step(a["base_pos"], a["com_pos"], a["yaws"], a["lin"], a["ang"], ref_a, lift_off=a["feet"])
        est_b.step(b["base_pos"], b["com_pos"], b["yaws"], b["lin"], b["ang"], ref_b, lift_off=b["feet"])
        ra, rb = ref_a.cpu().numpy(), ref_b.cpu().numpy()
        keep = np.arange(E) != bad
        assert ra[keep].tobytes() == rb[keep].tobytes(), f"step {k}"
        same_bits(rb[:, :12].copy(), want, f"the NaN run, step {k}")
        assert np.isnan(rb[bad, [2, 3, 5, 7]]).all()
        same_state(lib, est_b, host, f"the NaN run, step {k}")


def test_feet_through_the_generator_state_equal_feet_through_an_array(lib):
    E = 7
    est_a, host, rng = estimators(lib, E, seed=5)
    est_b, _, _ = estimators(lib, E, seed=5)
    x = draw_inputs(rng, E)
    frg = BatchedFootholdReferenceGenerator(E, 0.4, 0.3, x["feet"])  # its lift-off table starts as these feet
    d = upload(x)
    ref_a = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    ref_b = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    est_a.step(d["base_pos"], d["com_pos"], d["yaws"], d["lin"], d["ang"], ref_a, lift_off=d["feet"])
    est_b.step(d["base_pos"], d["com_pos"], d["yaws"], d["lin"], d["ang"], ref_b, frg=frg)
    want, _ = host.step(x, x["feet"])
    same_bits(ref_a[:, :12].contiguous(), want, "array")
    same_bits(ref_b[:, :12].contiguous(), want, "generator state")
    assert bytes(est_a.state_dict()) == bytes(est_b.state_dict())
    with pytest.raises(ValueError, match="exactly one"):
        est_b.step(d["base_pos"], d["com_pos"], d["yaws"], d["lin"], d["ang"], ref_b, frg=frg, lift_off=d["feet"])


def modulator_inputs(rng, E):
    x = draw_inputs(rng, E)
    x["feet"][..., :2] = x["hips"][..., :2] + rng.uniform(-0.2, 0.2, (E, 4, 2))  # about one leg in five beyond 0.2
    x["lin"][np.arange(E) % 5 == 0, :2] = rng.uniform(-0.3, 0.0099, (len(range(0, E, 5)), 2))  # standing
    x["feet"][np.arange(E) % 7 == 3, 1, 0] = np.nan  # a NaN distance
    return x


@pytest.mark.parametrize("E", [1, 3, 65, 4096])
def test_modulator_bit_equal(lib, E):
    rng = np.random.default_rng(100 + E)
    vm = BatchedVelocityModulator(E)
    guard = [torch.full((E + 2, 3), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)]
    for k in range(2):
        x = modulator_inputs(rng, E)
        want_l, want_a = host_modulate(lib, x)
        d = upload(x)
        got = vm.step(d["lin"], d["ang"], d["feet"], d["hips"], out=(guard[0][1:E + 1], guard[1][1:E + 1]))
        same_bits(got[0].contiguous(), want_l, f"lin, step {k}")
        same_bits(got[1].contiguous(), want_a, f"ang, step {k}")
        for g in guard:
            g = g.cpu().numpy()
            assert (g[0] == SENTINEL).all() and (g[-1] == SENTINEL).all()
        if E >= 65:
            hit = (want_l == 0).all(axis=1)
            assert hit.any() and not hit.all() and np.signbit(want_l[hit]).any()
    lin2, ang2 = vm.step(d["lin"], d["ang"], d["feet"], d["hips"])  # allocated outputs
    same_bits(lin2, want_l, "allocated lin")
    same_bits(ang2, want_a, "allocated ang")


def test_modulated_command_feeds_the_foothold_generator(lib):
    """srbd_vm_modulate_device -> srbd_frg_step_device with nothing read back in between: the seeds are those of
    srbd_vm_modulate -> srbd_frg_update_lift_off / _touch_down / _compute on the host."""
    E = 6
    rng = np.random.default_rng(31)
    x = modulator_inputs(rng, E)
    x["feet"] = np.nan_to_num(x["feet"], nan=0.1)  # the generator's state is compared as bytes: no NaN in it
    vel = rng.uniform(-0.5, 0.5, (E, 3))
    frg = BatchedFootholdReferenceGenerator(E, 0.4, 0.3, x["feet"])
    g = (lib.SrbdFrg * E)()
    prev, cur = np.ones((E, 4)), np.ones((E, 4))
    cur[:, 1] = 0.0
    want_l, _ = host_modulate(lib, x)
    want = np.zeros((E, 4, 3))
    p, fn = lib.dptr, lib.lib
    for e in range(E):
        assert fn.srbd_frg_init(C.byref(g[e]), 0.4, 0.3, p(x["feet"][e])) == 0
        args = (C.byref(g[e]), p(prev[e]), p(cur[e]), p(x["feet"][e]), 0, p(x["base_pos"][e]), float(x["yaws"][e]))
        assert fn.srbd_frg_update_lift_off(*args) == 0 and fn.srbd_frg_update_touch_down(*args) == 0
        assert fn.srbd_frg_compute(C.byref(g[e]), p(x["base_pos"][e]), float(x["yaws"][e]),
                                   p(np.ascontiguousarray(vel[e, :2])), p(np.ascontiguousarray(want_l[e, :2])),
                                   p(x["hips"][e]), CHN, frg.gravity_constant, None, p(want[e])) == 0
    d = upload(x)
    lin, _ = BatchedVelocityModulator(E).step(d["lin"], d["ang"], d["feet"], d["hips"])
    seeds = frg.step(d["base_pos"], d["yaws"], torch.from_numpy(vel).cuda(), lin, d["hips"], d["feet"],
                     torch.from_numpy(prev.astype(f32)).cuda(), torch.from_numpy(cur.astype(f32)).cuda(),
                     com_height_nominal=CHN)
    same_bits(seeds, want, "seeds")
    assert bytes(frg.state_dict()) == bytes(g)


def test_side_stream_behind_a_long_fill(lib):
    """Both launches enqueued on a side stream right behind a long fill of their outputs, with no synchronisation in
    between: stream order alone makes the result the host's."""
    E = 67
    est, host, rng = estimators(lib, E, seed=21)
    x = modulator_inputs(rng, E)
    x["feet"] = np.nan_to_num(x["feet"], nan=0.1)
    d = upload(x)
    big = torch.zeros((1 << 24,), dtype=torch.float64, device="cuda")  # 128 MiB: the fill outlasts the enqueue
    ref = big[:E * 24].view(E, 24)
    lin, ang = big[E * 24:E * 27].view(E, 3), big[E * 27:E * 30].view(E, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big.fill_(SENTINEL)
        BatchedVelocityModulator(E).step(d["lin"], d["ang"], d["feet"], d["hips"], out=(lin, ang), stream=side)
        est.step(d["base_pos"], d["com_pos"], d["yaws"], lin, ang, ref, lift_off=d["feet"], stream=side)
    side.synchronize()
    x["lin"], x["ang"] = host_modulate(lib, x)
    want, _ = host.step(x, x["feet"])
    same_bits(lin.contiguous(), x["lin"], "lin")
    r = ref.cpu().numpy()
    same_bits(r[:, :12].copy(), want, "ref 0..11")
    assert (r[:, 12:] == SENTINEL).all()
    same_state(lib, est, host, "the side stream's step")


def test_classes_against_the_c_calls_and_state_dict_round_trip(lib):
    E = 5
    est, host, rng = estimators(lib, E, seed=3)
    raw, _, _ = estimators(lib, E, seed=3)
    x = draw_inputs(rng, E)
    d = upload(x)
    ref_a = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    ref_b = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    assert est.step(d["base_pos"], d["com_pos"], d["yaws"], d["lin"], d["ang"], ref_a, lift_off=d["feet"]) is ref_a
    for handle in (C.c_void_p(1),):  # the legacy null stream named by its handle
        io = lib.SrbdTerrainRefBatchIo(base_pos=d["base_pos"].data_ptr(), com_pos=d["com_pos"].data_ptr(),
                                       com_pos_offset_w=None, yaws=d["yaws"].data_ptr(), lin=d["lin"].data_ptr(),
                                       ang=d["ang"].data_ptr(), feet=d["feet"].data_ptr(), frg=None, ref_z=REF_Z,
                                       ref=ref_b.data_ptr(), terrain=None)
        torch.cuda.synchronize()
        assert lib.lib.srbd_terrain_ref_step_device(raw.state.data_ptr(), E, C.byref(io), handle) == 0
        torch.cuda.synchronize()
    assert ref_a.cpu().numpy().tobytes() == ref_b.cpu().numpy().tobytes()
    assert bytes(est.state_dict()) == bytes(raw.state_dict())
    want, _ = host.step(x, x["feet"])
    same_bits(ref_a[:, :12].contiguous(), want, "class step")
    same_bits(est.terrain_pitch.contiguous(), np.array([g.pitch for g in host.g]), "pitch view")
    # a round trip through bytes into a fresh estimator, which then steps like the first
    saved = bytes(est.state_dict())
    fresh = BatchedTerrainEstimator(E, REF_Z)
    fresh.load_state_dict(saved)
    assert bytes(fresh.state_dict()) == saved
    with pytest.raises(ValueError, match="structs expected"):
        fresh.load_state_dict(saved[:-8])
    x2 = draw_inputs(rng, E)
    d2 = upload(x2)
    for e_, r_ in ((est, ref_a), (fresh, ref_b)):
        e_.step(d2["base_pos"], d2["com_pos"], d2["yaws"], d2["lin"], d2["ang"], r_, lift_off=d2["feet"])
    assert ref_a.cpu().numpy().tobytes() == ref_b.cpu().numpy().tobytes()
    host.step(x2, x2["feet"])
    same_state(lib, fresh, host, "the round trip")


def test_loop_modulator_generator_terrain_prepare(lib):
    """modulate -> srbd_frg_step_device -> terrain / reference (feet through the generator's state) ->
    srbd_prepare_state_device for four steps at E = 3 with nothing read back in between, against the same chain of
    host functions: the float32 states and references bit for bit."""
    E, steps = 3, 4
    rng = np.random.default_rng(12)
    first = draw_inputs(rng, E)
    frg = BatchedFootholdReferenceGenerator(E, 0.4, 0.3, first["feet"])
    est, host, _ = estimators(lib, E, seed=8)
    vm = BatchedVelocityModulator(E)
    g = (lib.SrbdFrg * E)()
    p, fn = lib.dptr, lib.lib
    for e in range(E):
        assert fn.srbd_frg_init(C.byref(g[e]), 0.4, 0.3, p(first["feet"][e])) == 0
    ref = torch.zeros((E, 24), dtype=torch.float64, device="cuda")
    prev = np.ones((E, 4), dtype=f32)
    got, want = [], []
    for k in range(steps):
        x = first if k == 0 else draw_inputs(rng, E)
        vel = rng.uniform(-0.5, 0.5, (E, 3))
        state = rng.uniform(-1, 1, (E, 24))
        cur = ((k + np.arange(E)[:, None] + np.arange(4)[None, :]) % 4 < 2).astype(f32)
        # the host chain
        lin, ang = host_modulate(lib, x)
        row = np.zeros((E, 24))
        for e in range(E):
            args = (C.byref(g[e]), p(prev[e].astype(np.float64)), p(cur[e].astype(np.float64)), p(x["feet"][e]), 0,
                    p(x["base_pos"][e]), float(x["yaws"][e]))
            assert fn.srbd_frg_update_lift_off(*args) == 0 and fn.srbd_frg_update_touch_down(*args) == 0
            seeds = np.zeros((4, 3))
            assert fn.srbd_frg_compute(C.byref(g[e]), p(x["base_pos"][e]), float(x["yaws"][e]),
                                       p(np.ascontiguousarray(vel[e, :2])), p(np.ascontiguousarray(lin[e, :2])),
                                       p(x["hips"][e]), CHN, frg.gravity_constant, None, p(seeds)) == 0
            row[e, 12:] = seeds.ravel()
        lift = np.array([np.array(g[e].lift_off) for e in range(E)])
        row[:, :12], _ = host.step(dict(x, lin=lin, ang=ang), lift)
        so, ro = np.zeros((E, 24)), np.zeros((E, 24))
        for e in range(E):
            assert fn.srbd_prepare_state(p(state[e]), p(row[e]), p(cur[e].astype(np.float64)),
                                         p(prev[e].astype(np.float64)), 0, None, p(so[e]), p(ro[e])) == 0
        want.append((so.astype(f32), ro.astype(f32)))
        # the device chain
        d = upload(x)
        d_prev, d_cur = torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda()
        dl, da = vm.step(d["lin"], d["ang"], d["feet"], d["hips"])
        frg.step(d["base_pos"], d["yaws"], torch.from_numpy(vel).cuda(), dl, d["hips"], d["feet"], d_prev, d_cur,
                 ref=ref, com_height_nominal=CHN)
        est.step(d["base_pos"], d["com_pos"], d["yaws"], dl, da, ref, frg=frg)
        states, refs = lib.prepare_state_device(torch.from_numpy(state).cuda(), ref, d_cur, d_prev)
        got.append((states, refs))
        prev = cur
    torch.cuda.synchronize()
    for k in range(steps):
        same_bits(got[k][0], want[k][0], f"states, step {k}")
        same_bits(got[k][1], want[k][1], f"refs, step {k}")
    assert bytes(frg.state_dict()) == bytes(g)
    same_state(lib, est, host, "the loop")
