"""The device-resident foothold reference generator (srbd_frg_step_device; BatchedFootholdReferenceGenerator) against
the host functions (srbd_frg_update_lift_off, srbd_frg_update_touch_down, srbd_frg_compute, include/srbd_host.h),
which tests/test_frg_host.py pins to the NumPy restatement of the reference.  The contract is bit equality -- the
generator state's bytes after every step and the seeds -- so every comparison is exact and no tolerance appears
here.  Expected values never come from the device path."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import config as mirror
from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
from quadruped_pympc_amd.helpers.periodic_gait_generator import (FULL_STANCE, BatchedPeriodicGaitGenerator,
                                                                 PeriodicGaitGenerator)

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 7.0
CHN = 0.3


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


class HostGenerators:
    """E host srbd_frg structs stepped by the three host C calls: the expected state bytes and seeds."""

    def __init__(self, lib, stance, height, lift, gravity):
        self.lib, self.E, self.gravity = lib, len(stance), gravity
        self.g = (lib.SrbdFrg * self.E)()
        for e in range(self.E):
            assert lib.lib.srbd_frg_init(C.byref(self.g[e]), float(stance[e]), float(height[e]),
                                         lib.dptr(np.ascontiguousarray(lift[e]))) == 0

    def bytes(self):
        return bytes(self.g)

    def step(self, x, full=None, off=None, chn=CHN):
        """x: the step's inputs (float64 arrays, contacts widened); returns the seeds (E, 4, 3)."""
        p, fn = self.lib.dptr, self.lib.lib
        out = np.zeros((self.E, 4, 3))
        prev, cur = x["prev"].astype(np.float64), x["cur"].astype(np.float64)
        for e in range(self.E):
            g = C.byref(self.g[e])
            fs = int(bool(full is not None and full[e]))
            base, yaw = p(x["base_pos"][e]), float(x["yaws"][e])
            assert fn.srbd_frg_update_lift_off(g, p(prev[e]), p(cur[e]), p(x["feet"][e]), fs, base, yaw) == 0
            assert fn.srbd_frg_update_touch_down(g, p(prev[e]), p(cur[e]), p(x["feet"][e]), fs, base, yaw) == 0
            assert fn.srbd_frg_compute(g, base, yaw, p(np.ascontiguousarray(x["base_lin_vel"][e, :2])),
                                       p(np.ascontiguousarray(x["ref_lin_vel"][e, :2])), p(x["hips"][e]), chn,
                                       self.gravity, None if off is None else p(off[e]), p(out[e])) == 0
        return out


def environments(E, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.2, 0.6, E), rng.uniform(0.2, 0.4, E), rng.uniform(-0.3, 0.3, (E, 4, 3)), rng


def draw_inputs(rng, E, k):
    """One step's random inputs: velocities of three magnitudes, so that both limits are reached and missed, and
    the scripted contacts (frg_model.contact_script's period-4 pattern 1 1 0 0, in which every leg meets all four
    (previous, current) pairs), environment e running it shifted by e rows."""
    scale = np.array([0.02, 0.3, 6.0])[rng.integers(0, 3, (E, 1))]
    shift = np.arange(E) % 4
    rows = (k + shift[:, None] + np.arange(4)[None, :]) % 4
    return dict(base_pos=rng.uniform(-2, 2, (E, 3)), yaws=rng.uniform(-4.0, 4.0, E),
                base_lin_vel=rng.standard_normal((E, 3)) * scale, ref_lin_vel=rng.standard_normal((E, 3)) * scale,
                hips=rng.uniform(-2, 2, (E, 4, 3)), feet=rng.uniform(-2, 2, (E, 4, 3)),
                prev=(rows < 2).astype(f32), cur=((rows + 1) % 4 < 2).astype(f32))


def upload(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}


def pgg_bytes(lib, gaits):
    g = (lib.SrbdPgg * len(gaits))()
    for e, gait in enumerate(gaits):
        assert lib.lib.srbd_pgg_init(C.byref(g[e]), int(gait), 0.65, 1.4, 12) == 0
    raw = np.frombuffer(bytes(g), dtype=np.uint8).reshape(len(gaits), lib.PGG_BYTES).copy()
    return torch.from_numpy(raw).cuda()


def same_state(gen, host, what):
    assert bytes(gen.state_dict()) == host.bytes(), f"generator state differs from the host's after {what}"


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got, want, err_msg=what)
    assert got.tobytes() == want.tobytes(), what


# a single environment, a partial wave, a partial block, more than one block
@pytest.mark.parametrize("E", [1, 5, 67, 300])
def test_forty_five_steps_bit_equal(lib, E):
    steps = 45  # the ring fills and wraps twice
    stance, height, lift, rng = environments(E, seed=E)
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    host = HostGenerators(lib, stance, height, lift, gen.gravity_constant)
    same_state(gen, host, "construction")
    odd = E % 2 == 1  # the optional inputs are given for odd E, NULL otherwise
    gaits = np.where(np.arange(E) % 3 == 0, FULL_STANCE, np.arange(E) % 7).astype(np.int32)
    pgg = pgg_bytes(lib, gaits) if odd else None
    full = (gaits == FULL_STANCE) if odd else None
    guarded = torch.full((E + 2, 4, 3), SENTINEL, dtype=torch.float64, device="cuda")
    ref = torch.full((E, 24), SENTINEL, dtype=torch.float64, device="cuda")
    pairs = set()
    for k in range(steps):
        x = draw_inputs(rng, E, k)
        off = rng.uniform(-0.05, 0.05, (E, 3)) if odd else None
        pairs |= {(l, int(x["prev"][0, l]), int(x["cur"][0, l])) for l in range(4)}
        want = host.step(x, full, off)
        d = upload(x)
        got = gen.step(d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"],
                       d["cur"], gait=pgg, com_pos_offset_w=None if off is None else torch.from_numpy(off).cuda(),
                       ref=ref, out=guarded[1:E + 1], com_height_nominal=CHN)
        assert got.data_ptr() == guarded[1:E + 1].data_ptr()
        same_bits(got, want, f"seeds, step {k}")
        same_state(gen, host, f"step {k}")
        r = ref.cpu().numpy()
        same_bits(r[:, 12:].reshape(E, 4, 3), want, f"ref 12..23, step {k}")
        assert (r[:, :12] == SENTINEL).all(), "ref entries 0..11 were written"
        edge = guarded.cpu().numpy()
        assert (edge[0] == SENTINEL).all() and (edge[E + 1] == SENTINEL).all(), "a guard row was written"
    assert host.g[0].hist_len == 20 and host.g[0].hist_head == steps % 20
    assert pairs == {(l, p, c) for l in range(4) for p in (0, 1) for c in (0, 1)}
    same_bits(gen.last_reference_footholds, want, "last_reference_footholds view")
    if odd:
        assert full.any() and (E == 1 or not full.all())


def test_allocated_output_state_dict_and_stance_time(lib):
    E = 5
    stance, height, lift, rng = environments(E, seed=50)
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    host = HostGenerators(lib, stance, height, lift, gen.gravity_constant)
    for k in range(3):
        x = draw_inputs(rng, E, k)
        d = upload(x)
        got = gen.step(d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"],
                       d["cur"], com_height_nominal=CHN)
        assert tuple(got.shape) == (E, 4, 3) and got.dtype == torch.float64 and got.is_contiguous()
        same_bits(got, host.step(x), f"step {k}")
    saved = gen.state_dict()
    new_stance = rng.uniform(0.2, 0.6, E)
    gen.set_stance_time(torch.from_numpy(new_stance).cuda())  # wb_interface.py:356
    for e in range(E):
        host.g[e].stance_time = new_stance[e]
    same_state(gen, host, "set_stance_time")
    x = draw_inputs(rng, E, 3)
    d = upload(x)
    args = (d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"], d["cur"])
    same_bits(gen.step(*args, com_height_nominal=CHN), host.step(x), "after set_stance_time")
    same_state(gen, host, "a step after set_stance_time")
    gen.load_state_dict(saved)
    assert bytes(gen.state_dict()) == bytes(saved)
    with pytest.raises(ValueError, match="cuda"):  # host tensors are refused, not copied
        gen.step(*[t.cpu() for t in args])


def test_nan_environment_changes_nothing_in_its_neighbours(lib):
    E, bad = 5, 2
    stance, height, lift, rng = environments(E, seed=77)
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    host = HostGenerators(lib, stance, height, lift, gen.gravity_constant)
    size = lib.FRG_BYTES
    for k in range(6):
        x = draw_inputs(rng, E, k)
        x["base_lin_vel"][bad] = np.nan
        if k >= 2:
            x["yaws"][bad] = np.nan
            x["feet"][bad, k % 4] = np.nan
            x["base_pos"][bad, 1] = np.inf
        want = host.step(x)
        d = upload(x)
        got = gen.step(d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"],
                       d["cur"], com_height_nominal=CHN).cpu().numpy()
        np.testing.assert_array_equal(got, want)  # NaNs position for position
        assert np.isnan(want[bad, :, :2]).all() and np.isfinite(np.delete(want, bad, axis=0)).all()
        raw, exp = bytes(gen.state_dict()), host.bytes()
        for e in range(E):
            a, b = raw[e * size:(e + 1) * size], exp[e * size:(e + 1) * size]
            if e != bad:
                assert a == b, f"environment {e}, step {k}"
        ga = np.frombuffer(raw[bad * size:(bad + 1) * size - 8], dtype=np.float64)
        gb = np.frombuffer(exp[bad * size:(bad + 1) * size - 8], dtype=np.float64)
        np.testing.assert_array_equal(ga, gb)
        assert raw[(bad + 1) * size - 8:(bad + 1) * size] == exp[(bad + 1) * size - 8:(bad + 1) * size]


def test_side_stream_behind_a_long_fill(lib):
    """The launch enqueued on a side stream right behind long fills of its outputs, with no synchronisation in
    between: stream order alone makes the result the host's."""
    E = 67
    stance, height, lift, rng = environments(E, seed=21)
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    host = HostGenerators(lib, stance, height, lift, gen.gravity_constant)
    x = draw_inputs(rng, E, 1)
    d = upload(x)
    big = torch.zeros((1 << 24,), dtype=torch.float64, device="cuda")  # 128 MiB: the fill outlasts the enqueue
    seeds = big[:E * 12].view(E, 4, 3)
    ref = big[E * 12:E * 36].view(E, 24)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big.fill_(SENTINEL)
        got = gen.step(d["base_pos"], d["yaws"], d["base_lin_vel"], d["ref_lin_vel"], d["hips"], d["feet"], d["prev"],
                       d["cur"], ref=ref, out=seeds, stream=side, com_height_nominal=CHN)
    side.synchronize()
    want = host.step(x)
    same_bits(got, want, "seeds")
    r = ref.cpu().numpy()
    same_bits(r[:, 12:].reshape(E, 4, 3), want, "ref 12..23")
    assert (r[:, :12] == SENTINEL).all()
    same_state(gen, host, "the side stream's step")


def test_explicit_null_stream_handle(lib):
    """The C call with the legacy null stream named by its handle (hipStreamLegacy) and by NULL."""
    E = 5
    stance, height, lift, rng = environments(E, seed=9)
    gen = BatchedFootholdReferenceGenerator(E, stance, height, lift)
    host = HostGenerators(lib, stance, height, lift, gen.gravity_constant)
    seeds = torch.zeros((E, 4, 3), dtype=torch.float64, device="cuda")
    for k, handle in enumerate((C.c_void_p(1), None)):
        x = draw_inputs(rng, E, k)
        d = upload(x)
        io = lib.SrbdFrgBatchIo(base_pos=d["base_pos"].data_ptr(), yaws=d["yaws"].data_ptr(),
                                base_lin_vel=d["base_lin_vel"].data_ptr(), ref_lin_vel=d["ref_lin_vel"].data_ptr(),
                                hips=d["hips"].data_ptr(), feet=d["feet"].data_ptr(),
                                previous_contact=d["prev"].data_ptr(), current_contact=d["cur"].data_ptr(),
                                pgg=None, com_pos_offset_w=None, com_height_nominal=CHN,
                                gravity=gen.gravity_constant, seeds=seeds.data_ptr(), ref=None)
        torch.cuda.synchronize()
        assert lib.lib.srbd_frg_step_device(gen.state.data_ptr(), E, C.byref(io), handle) == 0
        torch.cuda.synchronize()
        same_bits(seeds, host.step(x), f"handle {handle}")
        same_state(gen, host, "a step on the null stream")


# ------------------------------------------------------------------ end to end
def config_with(**mpc):
    cfg = types.ModuleType("frg_device_config")
    for k in dir(mirror):
        if not k.startswith("__"):
            setattr(cfg, k, getattr(mirror, k))
    cfg.mpc_params = dict(mirror.mpc_params, **mpc)
    return cfg


def test_flat_ground_loop_equals_the_loop_fed_from_the_host(lib):
    """gait generator -> foothold reference generator (writing ref 12..23) -> prepare_state_and_reference_device ->
    compute_control_device for six steps on flat ground with nothing read back in between, against the same loop whose
    contacts and reference feet come from the host generators and the host srbd_frg functions: the GRFs bit for bit."""
    from quadruped_pympc_amd.controllers.sampling.centroidal_nmpc_hip_batched import Batched_Sampling_MPC
    from quadruped_pympc_amd.synthetic import CONFIGS, reference, robot_state

    E, N, H, steps, dt = 5, 128, 12, 6, 0.02
    cfg = config_with(num_parallel_computations=N, horizon=H, sampling_method="mppi",
                      control_parametrization="zero_order", shift_solution=False, rng="philox", device_id=0)
    on_dev, on_host = Batched_Sampling_MPC(E, cfg), Batched_Sampling_MPC(E, cfg)
    robot = CONFIGS["c2"].robot
    gaits = [0, 1, 2, 7, 3]  # trot, pace, bounding, full stance, crawl
    duty, freq = [0.65, 0.7, 0.65, 0.65, 0.8], [1.4, 2.0, 2.4, 1.4, 1.0]
    start = np.array([[0.62, 0.1, 0.1, 0.6], [0.68, 0.3, 0.66, 0.3], [0.5, 0.5, 0.63, 0.6], [0.0, 0.5, 0.5, 0.0],
                      [0.78, 0.25, 0.75, 0.5]])  # legs about to pass their duty factor: lift-offs within the steps
    try:
        rng = np.random.default_rng(5)
        state_in = np.stack([[robot_state(robot, 10 * k + e) for e in range(E)] for k in range(steps)])
        ref_in = np.stack([[reference(robot, s) for s in state_in[k]] for k in range(steps)])
        hips = state_in[:, :, 12:].reshape(steps, E, 4, 3) + rng.uniform(-0.03, 0.03, (steps, E, 4, 3))
        hips[..., 2] += 0.3
        stance = np.array(duty) / np.array(freq)
        height = np.full(E, 0.3)
        lift = state_in[0, :, 12:].reshape(E, 4, 3)
        keys = rng.integers(1, 2 ** 40, (steps, E, 2)).astype(np.int64)
        best0 = (rng.standard_normal((E, 144)) * 0.5).astype(f32)
        d_state = torch.from_numpy(state_in).cuda()
        d_keys = torch.from_numpy(keys).cuda()
        d_hips = torch.from_numpy(hips).cuda()

        def run_loop(ctrl, contacts_and_refs):
            best_t = torch.from_numpy(best0).cuda()
            d_prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")
            grfs, refs_seen = [], []
            for k in range(steps):
                seq, d_ref = contacts_and_refs(k, d_prev)
                current = seq[:, :, 0].contiguous()
                states, refs = ctrl.prepare_state_and_reference_device(d_state[k], d_ref, current, d_prev,
                                                                       best_control_parameters=best_t)
                out = ctrl.compute_control_device(states, refs, seq, best_t, d_keys[k])
                grfs.append(out[0].clone())
                refs_seen.append(d_ref.clone())
                d_prev = current
            torch.cuda.synchronize()
            return [g.cpu().numpy() for g in grfs], [r.cpu().numpy() for r in refs_seen]

        # the loop fed from the host: host gait generators and host srbd_frg calls, uploaded each step
        pggs = [PeriodicGaitGenerator(duty[e], freq[e], gaits[e], H) for e in range(E)]
        for e in range(E):
            pggs[e].set_phase_signal(start[e])
        host = HostGenerators(lib, stance, height, lift, mirror.gravity_constant)
        lifts = [0]

        def from_host(k, d_prev):
            seqs = []
            for e in range(E):
                pggs[e].run(dt, pggs[e].step_freq)
                seqs.append(pggs[e].compute_contact_sequence([dt], [H])[:, :H])
            seqs = np.stack(seqs).astype(f32)
            prev = d_prev.cpu().numpy()
            lifts[0] += int(((prev == 1) & (seqs[:, :, 0] == 0)).sum())
            s = state_in[k]
            x = dict(base_pos=np.ascontiguousarray(s[:, 0:3]), yaws=np.ascontiguousarray(s[:, 8]),
                     base_lin_vel=np.ascontiguousarray(s[:, 3:6]),
                     ref_lin_vel=np.ascontiguousarray(ref_in[k, :, 3:6]), hips=hips[k],
                     feet=np.ascontiguousarray(s[:, 12:].reshape(E, 4, 3)), prev=prev, cur=seqs[:, :, 0])
            seeds = host.step(x, full=np.array(gaits) == FULL_STANCE, chn=CHN)
            r = ref_in[k].copy()
            r[:, 12:] = seeds.reshape(E, 12)
            return torch.from_numpy(seqs).cuda(), torch.from_numpy(r).cuda()

        want_grf, want_ref = run_loop(on_host, from_host)
        assert lifts[0] >= 3, "the scenario must contain lift-offs"

        # the device loop: nothing comes from the host after the upload
        gen = BatchedPeriodicGaitGenerator(E, duty, freq, gaits, H)
        gen.set_phase_signal(start)
        frg = BatchedFootholdReferenceGenerator(E, stance, height, lift)
        d_ref_all = torch.from_numpy(ref_in.copy()).cuda()

        def from_device(k, d_prev):
            gen.run(dt)
            seq = gen.compute_contact_sequence([dt], [H])
            current = seq[:, :, 0].contiguous()
            s = d_state[k]
            frg.step(s[:, 0:3].contiguous(), s[:, 8].contiguous(), s[:, 3:6].contiguous(),
                     d_ref_all[k, :, 3:6].contiguous(), d_hips[k], s[:, 12:].reshape(E, 4, 3).contiguous(), d_prev,
                     current, gait=gen, ref=d_ref_all[k], com_height_nominal=CHN)
            return seq, d_ref_all[k]

        got_grf, got_ref = run_loop(on_dev, from_device)
        for k in range(steps):
            same_bits(got_ref[k], want_ref[k], f"step {k}: reference")
            assert not np.array_equal(want_ref[k][:, 12:], ref_in[k][:, 12:]), "the generator's feet must show"
            same_bits(got_grf[k], want_grf[k], f"step {k}: GRFs")
        same_state(frg, host, "six steps")
    finally:
        on_dev.close()
        on_host.close()
