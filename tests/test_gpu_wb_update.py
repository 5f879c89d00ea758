"""srbd_pgg_start_stop_device and srbd_wb_update_device (include/srbd_mpc.h; BatchedWBInterface) on the GPU.

The contract is bit equality, so no tolerance appears here: start-and-stop against the host function on the recorded
fixture's inputs; the fused update against the chain of the existing device calls it replaces, state arrays as bytes
and outputs with array_equal(equal_nan=True) after every one of 40 steps, for every stage set; and against the host
functions of srbd_host.h, which the CPU tests pin to the recorded reference, so the chain of equalities closes.
Shapes: E = 1, 3 (a ragged wave) and 65 (one quad in a second block); H = 12 in rows of 16; mixed gaits."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
from quadruped_pympc_amd.helpers.terrain_estimator import BatchedTerrainEstimator
from quadruped_pympc_amd.interfaces.wb_interface_batched import BatchedWBInterface

pytestmark = pytest.mark.gpu
H, STRIDE, LOOKAHEAD, STEPS = 12, 16, 3, 40
SIM_DT, REF_Z, CHN, GRAVITY, MAX_DISTANCE = 0.02, 0.31, 0.3, 9.81, 0.2
UNIFORM = ([0.02], [H])
NONUNIFORM = ([0.01, 0.04], [4, H])
VM, SS, TD = 1, 2, 4
HIPS_H = np.array([[0.19, 0.05], [0.19, -0.05], [-0.19, 0.05], [-0.19, -0.05]])
GAITS = [(0, 0.65, 1.4), (1, 0.7, 1.4), (5, 0.8, 0.5), (2, 0.65, 1.9), (3, 0.8, 0.7)]  # type, duty factor, frequency
INPUTS = ("com_pos", "base_pos", "base_lin_vel", "euler", "base_ang_vel", "feet", "hips", "ref_lin", "ref_ang")
OUTPUTS = ("ref", "contacts", "current", "previous", "seeds", "optimize", "lin", "ang", "terrain", "action")
REF = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "start_stop_ref.npz"))


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


def measurements(E, steps=STEPS, seed=5, nan_env=None):
    """Fixed-seed measurements per step.  Even environments stand still under the hips with no command for steps
    10..27 (they stop once all four feet are down, stand, and walk again); every fifth step a foot of environment
    e = step % E is far from its hip, which makes the modulator cut that environment's command."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(steps):
        yaw = rng.uniform(-3.1, 3.1, E)
        base = np.stack([0.02 * i + rng.uniform(-1, 1, E), rng.uniform(-1, 1, E), 0.3 + rng.uniform(-0.01, 0.01, E)], 1)
        c, s = np.cos(yaw), np.sin(yaw)
        rot = np.stack([np.stack([c, -s], 1), np.stack([s, c], 1)], 1)  # (E, 2, 2): horizontal -> world
        side = np.array([0.1, -0.1, 0.1, -0.1])
        hips, feet = np.zeros((E, 4, 3)), np.zeros((E, 4, 3))
        feet_h = HIPS_H + np.stack([rng.uniform(-0.02, 0.02, (E, 4)), side + rng.uniform(-0.02, 0.02, (E, 4))], 2)
        hips[:, :, :2] = np.einsum("eij,lj->eli", rot, HIPS_H) + base[:, None, :2]
        feet[:, :, :2] = np.einsum("eij,elj->eli", rot, feet_h) + base[:, None, :2]
        hips[:, :, 2], feet[:, :, 2] = base[:, None, 2], rng.uniform(0.0, 0.05, (E, 4))
        x = dict(com_pos=base + rng.uniform(-0.01, 0.01, (E, 3)), base_pos=base,
                 base_lin_vel=rng.uniform(-0.04, 0.04, (E, 3)), base_ang_vel=rng.uniform(-0.04, 0.04, (E, 3)),
                 euler=np.stack([rng.uniform(-0.03, 0.03, E), rng.uniform(-0.03, 0.03, E), yaw], 1), feet=feet,
                 hips=hips, ref_lin=rng.uniform(0.05, 0.4, (E, 3)), ref_ang=rng.uniform(-0.2, 0.2, (E, 3)))
        if 10 <= i < 28:
            x["ref_lin"][0::2] = 0.0
            x["ref_ang"][0::2] = 0.0
        if i % 5 == 4:
            x["feet"][i % E, i % 4, 0] += 0.5
        if nan_env is not None and i >= 3:
            x["base_lin_vel"][nan_env, i % 3] = np.nan
            if i % 2:
                x["feet"][nan_env, 1, 1] = np.nan
        out.append({k: np.ascontiguousarray(v) for k, v in x.items()})
    return out


class Loop:
    """One set of state tensors and the two ways to step it."""

    def __init__(self, lib, E, stages, seq=UNIFORM):
        self.lib, self.E, self.stages, self.seq = lib, E, stages, seq
        g = [GAITS[e % len(GAITS)] for e in range(E)]
        self.gait = BatchedPeriodicGaitGenerator(E, [v[1] for v in g], [v[2] for v in g], [v[0] for v in g], H)
        lift = np.zeros((E, 4, 3))
        lift[:, :, :2] = HIPS_H + np.array([0.0, 0.1]) * np.array([1, -1, 1, -1])[:, None]
        self.frg = BatchedFootholdReferenceGenerator(E, [0.4 + 0.01 * e for e in range(E)], 0.3, lift)
        self.terr = BatchedTerrainEstimator(E, REF_Z, roll_activated=[e % 2 == 1 for e in range(E)])
        self.com_off = torch.from_numpy(np.random.default_rng(2).uniform(-0.01, 0.01, (E, 3))).cuda()
        self.wb = BatchedWBInterface(E, self.gait, self.frg, self.terr, contact_sequence_dts=seq[0],
                                     contact_sequence_lenghts=seq[1], horizon=H, ref_z=REF_Z, com_height_nominal=CHN,
                                     gravity=GRAVITY, contact_stride=STRIDE, lookahead=LOOKAHEAD,
                                     max_distance=MAX_DISTANCE)
        self.wb.vm_activated, self.wb.start_and_stop_activated = bool(stages & VM), bool(stages & SS)
        self.wb.optimize_step_freq = bool(stages & TD)
        # the chain's own buffers (the interface's contact rows and trigger words are its state as well)
        self.contacts = torch.zeros((E, 4, STRIDE), dtype=torch.float32, device="cuda")
        self.ref = torch.zeros((E, 24), dtype=torch.float64, device="cuda")

    def states(self):
        return dict(pgg=self.gait.state, frg=self.frg.state, terrain=self.terr.state, contact=self.wb.current_contact,
                    rising_edge=self.wb.rising_edge)

    def fused(self, x):
        r = self.wb.update_state_and_reference_device(x["com_pos"], x["base_pos"], x["base_lin_vel"], x["euler"],
                                                      x["base_ang_vel"], x["feet"], x["hips"], SIM_DT, x["ref_lin"],
                                                      x["ref_ang"], com_pos_offset_w=self.com_off)
        return dict(zip(OUTPUTS, r + (self.wb.terrain, self.wb.action)))

    def chain(self, x):
        """The existing device calls in the order of srbd_wb_update_device's contract."""
        L, E, st = self.lib, self.E, self.stages
        contact, edge = self.wb.current_contact, self.wb.rising_edge
        yaws = x["euler"][:, 2].contiguous()
        lin, ang = x["ref_lin"], x["ref_ang"]
        if st & VM:
            lin, ang = L.vm_modulate_device(lin, ang, x["feet"], x["hips"], MAX_DISTANCE)
        action = torch.zeros(E, dtype=torch.int32, device="cuda")
        if st & SS:
            L.pgg_start_stop_device(self.gait.state, x["feet"], x["hips"], x["base_pos"], x["euler"], x["base_lin_vel"],
                                    x["base_ang_vel"], lin, ang, contact, frg=self.frg.state, out=action)
        L.pgg_run_device(self.gait.state, SIM_DT)
        L.pgg_contact_sequence_device(self.gait.state, H, self.seq[0], self.seq[1], out=self.contacts)
        previous = contact.clone()
        contact.copy_(self.contacts[:, :, 0])
        seeds = L.frg_step_device(self.frg.state, x["base_pos"], yaws, x["base_lin_vel"], lin, x["hips"], x["feet"],
                                  previous, contact, CHN, GRAVITY, pgg=self.gait.state, com_pos_offset_w=self.com_off,
                                  ref=self.ref)
        terrain = torch.zeros((E, 3), dtype=torch.float64, device="cuda")
        L.terrain_ref_step_device(self.terr.state, x["base_pos"], x["com_pos"], yaws, lin, ang, self.ref, REF_Z,
                                  frg=self.frg.state, com_pos_offset_w=self.com_off, out=terrain)
        optimize = torch.zeros(E, dtype=torch.int32, device="cuda")
        if st & TD:
            L.stc_touch_down_device(edge, contact, previous, self.contacts, LOOKAHEAD, horizon=H, out=optimize)
        return dict(ref=self.ref, contacts=self.contacts, current=contact, previous=previous, seeds=seeds,
                    optimize=optimize, lin=lin, ang=ang, terrain=terrain, action=action)


def run(loop, xs, how):
    """Step `loop` through xs; per step the state bytes and the outputs, as host arrays (one copy at the end)."""
    states, outs = [], []
    for x in xs:
        r = getattr(loop, how)({k: torch.from_numpy(v).cuda() for k, v in x.items()})
        states.append({k: v.clone() for k, v in loop.states().items()})
        outs.append({k: v.clone() for k, v in r.items()})
    torch.cuda.synchronize()
    return ([{k: v.cpu().numpy().tobytes() for k, v in s.items()} for s in states],
            [{k: v.cpu().numpy() for k, v in o.items()} for o in outs])


def assert_same(a, b, envs=None):
    (sa, oa), (sb, ob) = a, b
    assert len(sa) == len(sb)
    for i in range(len(sa)):
        for k in sa[i]:
            if envs is None:
                assert sa[i][k] == sb[i][k], (i, k)
            else:
                n = len(sa[i][k]) // len(oa[i]["optimize"])
                for e in envs:
                    assert sa[i][k][e * n:(e + 1) * n] == sb[i][k][e * n:(e + 1) * n], (i, k, e)
        for k in OUTPUTS:
            x, y = (oa[i][k], ob[i][k]) if envs is None else (oa[i][k][list(envs)], ob[i][k][list(envs)])
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (i, k)


@pytest.mark.parametrize("E", [1, 3, 65])
def test_start_stop_device_equals_the_host_function(lib, E):
    """The fixture's single calls, one per launch, broadcast over E environments that differ in gait and phase."""
    args = ("feet", "hips", "base_pos", "euler", "lin_vel", "ang_vel", "ref_lin", "ref_ang")
    hip = float(REF["hip_offset"])
    frg = BatchedFootholdReferenceGenerator(E, 0.4, 0.3, np.zeros((4, 3)))
    got_bytes, want_bytes, got_act, want_act = [], [], [], []
    for i in range(0, len(REF["case_names"]), 1 if E == 3 else 3):
        host = (lib.SrbdPgg * E)()
        for e in range(E):
            gait = int(REF["case_before_gait"][i]) if e == 0 else (7 if e % 3 == 0 else e % 7)
            assert lib.lib.srbd_pgg_init(C.byref(host[e]), gait, 0.65, 1.4, H) == 0
            host[e].previous_gait_type = int(REF["case_before_previous"][i]) if e == 0 else (e + 3) % 8
            for l in range(4):
                host[e].phase_signal[l] = float(REF["case_before_phase"][i][l]) + 0.01 * e
                host[e].init[l] = int(REF["case_before_init"][i][l]) * (1 + e % 2)
        pgg = torch.from_numpy(np.frombuffer(bytes(host), dtype=np.uint8).reshape(E, -1).copy()).cuda()
        x = {k: np.broadcast_to(REF[f"case_{k}"][i], (E,) + REF[f"case_{k}"][i].shape).copy()
             for k in args}
        contact = np.broadcast_to(REF["case_contact"][i], (E, 4)).copy()
        t = [torch.from_numpy(x[k]).cuda() for k in args] + [torch.from_numpy(contact.astype(np.float32)).cuda()]
        if i % 2:  # the hip offset from the foothold generator's structs, or the shared value
            act = lib.pgg_start_stop_device(pgg, *t, frg=frg.state)
        else:
            act = lib.pgg_start_stop_device(pgg, *t, hip_offset=hip)
        want = []
        for e in range(E):
            p = lib.dptr
            want.append(lib.lib.srbd_pgg_start_stop(C.byref(host[e]), p(x["feet"][e]), p(x["hips"][e]), hip,
                                                    p(x["base_pos"][e]), p(x["euler"][e]), p(x["lin_vel"][e]),
                                                    p(x["ang_vel"][e]), p(x["ref_lin"][e]), p(x["ref_ang"][e]),
                                                    p(contact[e])))
        assert want[0] == REF["case_action"][i]
        got_bytes.append(pgg), want_bytes.append(bytes(host)), got_act.append(act), want_act.append(want)
    torch.cuda.synchronize()
    for g, w, a, wa in zip(got_bytes, want_bytes, got_act, want_act):
        assert g.cpu().numpy().tobytes() == w
        assert np.array_equal(a.cpu().numpy(), np.array(wa, dtype=np.int32))
    assert {v for wa in want_act for v in wa} == {0, 1, 2}


STAGE_SETS = [VM | SS | TD, 0, VM, SS, TD]


@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("stages", STAGE_SETS)
def test_fused_update_equals_the_chain_of_device_calls(lib, E, stages):
    xs = measurements(E)
    seq = NONUNIFORM if (E == 3 and stages == (VM | SS | TD)) else UNIFORM
    fused, chain = run(Loop(lib, E, stages, seq), xs, "fused"), run(Loop(lib, E, stages, seq), xs, "chain")
    assert_same(fused, chain)
    acts = np.stack([o["action"] for o in chain[1]])
    if stages & SS and E > 1:  # the measurements do make environments stop, stand and walk again
        assert (acts == 1).sum() > 3 and (acts == 2).any() and (acts[-1] == 0).all()
    if stages & TD and (E > 1 or not stages & SS):  # (the one trotting environment stands through its only window)
        assert np.stack([o["optimize"] for o in chain[1]]).any()
    if stages & VM:
        assert any((o["lin"] == 0).all(axis=1).any() for o in chain[1])


def test_a_nan_in_one_environment_leaves_the_others_alone(lib):
    E, stages = 3, VM | SS | TD
    dirty, clean = measurements(E, nan_env=1), measurements(E)
    fused = run(Loop(lib, E, stages), dirty, "fused")
    assert_same(fused, run(Loop(lib, E, stages), dirty, "chain"))
    assert_same(fused, run(Loop(lib, E, stages), clean, "fused"), envs=(0, 2))
    assert any(np.isnan(o["ref"][1]).any() for o in fused[1])


def host_chain(lib, E, stages, xs, seq, com_off):
    """The same steps through the host functions of srbd_host.h on host structs: per step the state bytes and outputs."""
    fn, p = lib.lib, lib.dptr
    g = [GAITS[e % len(GAITS)] for e in range(E)]
    pgg, frg, terr = (lib.SrbdPgg * E)(), (lib.SrbdFrg * E)(), (lib.SrbdTerrainEst * E)()
    lift = np.zeros((4, 3))
    lift[:, :2] = HIPS_H + np.array([0.0, 0.1]) * np.array([1, -1, 1, -1])[:, None]
    for e in range(E):
        assert fn.srbd_pgg_init(C.byref(pgg[e]), g[e][0], g[e][1], g[e][2], H) == 0
        assert fn.srbd_frg_init(C.byref(frg[e]), 0.4 + 0.01 * e, 0.3, p(lift)) == 0
        assert fn.srbd_terrain_est_init(C.byref(terr[e])) == 0
        terr[e].roll_activated = int(e % 2 == 1)
    contact, edge = np.ones((E, 4)), (C.c_int32 * E)()
    dts, lens = np.array(seq[0], dtype=np.float64), np.array(seq[1], dtype=np.int32)
    states, outs = [], []
    for x in xs:
        o = dict(ref=np.zeros((E, 24)), contacts=np.zeros((E, 4, STRIDE), dtype=np.float32), seeds=np.zeros((E, 4, 3)),
                 previous=contact.astype(np.float32), optimize=np.zeros(E, dtype=np.int32), lin=x["ref_lin"].copy(),
                 ang=x["ref_ang"].copy(), terrain=np.zeros((E, 3)), action=np.zeros(E, dtype=np.int32))
        for e in range(E):
            if stages & VM:
                assert fn.srbd_vm_modulate(MAX_DISTANCE, p(x["ref_lin"][e]), p(x["ref_ang"][e]), p(x["feet"][e]),
                                           p(x["hips"][e]), p(o["lin"][e]), p(o["ang"][e])) == 0
            if stages & SS:
                o["action"][e] = fn.srbd_pgg_start_stop(C.byref(pgg[e]), p(x["feet"][e]), p(x["hips"][e]),
                                                        frg[e].hip_offset, p(x["base_pos"][e]), p(x["euler"][e]),
                                                        p(x["base_lin_vel"][e]), p(x["base_ang_vel"][e]), p(o["lin"][e]),
                                                        p(o["ang"][e]), p(contact[e]))
            flags, seq_out = np.zeros(4), np.zeros(8 * H)
            assert fn.srbd_pgg_run(C.byref(pgg[e]), SIM_DT, pgg[e].step_freq, p(flags)) == 0
            cols = fn.srbd_pgg_contact_sequence(C.byref(pgg[e]), p(dts), lib.iptr(lens), len(dts), p(seq_out), 8 * H)
            assert cols in (H, 2 * H)
            rows = np.ascontiguousarray(seq_out[:4 * cols].reshape(4, cols)[:, :H])
            o["contacts"][e, :, :H] = rows
            previous, contact[e] = contact[e].copy(), rows[:, 0]
            yaw, full = float(x["euler"][e, 2]), int(pgg[e].gait_type == 7)
            for update in (fn.srbd_frg_update_lift_off, fn.srbd_frg_update_touch_down):
                assert update(C.byref(frg[e]), p(previous), p(contact[e]), p(x["feet"][e]), full, p(x["base_pos"][e]),
                              yaw) == 0
            assert fn.srbd_frg_compute(C.byref(frg[e]), p(x["base_pos"][e]), yaw,
                                       p(np.ascontiguousarray(x["base_lin_vel"][e, :2])),
                                       p(np.ascontiguousarray(o["lin"][e, :2])), p(x["hips"][e]), CHN, GRAVITY,
                                       p(com_off[e]), p(o["seeds"][e])) == 0
            o["ref"][e, 12:] = o["seeds"][e].reshape(12)
            table = np.array(frg[e].lift_off, dtype=np.float64).reshape(4, 3)
            row = np.zeros(12)
            assert fn.srbd_terrain_estimate(C.byref(terr[e]), p(x["base_pos"][e]), yaw, p(table),
                                            p(o["terrain"][e])) == 0
            assert fn.srbd_reference_assemble(C.byref(terr[e]), REF_Z, float(x["base_pos"][e, 2]),
                                              float(x["com_pos"][e, 2]), float(com_off[e, 2]), p(o["lin"][e]),
                                              p(o["ang"][e]), p(row)) == 0
            o["ref"][e, :12] = row
            if stages & TD:
                word = C.c_int32(edge[e])
                o["optimize"][e] = fn.srbd_stc_touch_down(C.byref(word), p(contact[e]), p(previous), p(rows), H, H,
                                                          LOOKAHEAD)
                edge[e] = word.value
        o["current"] = contact.astype(np.float32)
        states.append(dict(pgg=bytes(pgg), frg=bytes(frg), terrain=bytes(terr),
                           contact=contact.astype(np.float32).tobytes(), rising_edge=bytes(edge)))
        outs.append(o)
    return states, outs


@pytest.mark.parametrize("stages,seq", [(VM | SS | TD, UNIFORM), (SS | TD, NONUNIFORM), (0, UNIFORM)])
def test_fused_update_equals_the_host_functions(lib, stages, seq):
    E = 3
    xs = measurements(E, steps=10, seed=9)
    for x in xs[2:]:  # environment 0 stands still from the third step on, so that it stops within the ten
        x["ref_lin"][0] = 0.0
        x["ref_ang"][0] = 0.0
    loop = Loop(lib, E, stages, seq)
    fused = run(loop, xs, "fused")
    host = host_chain(lib, E, stages, xs, seq, loop.com_off.cpu().numpy())
    assert_same(fused, host)
    if stages & SS:
        assert any(o["action"][0] == 1 for o in host[1])
