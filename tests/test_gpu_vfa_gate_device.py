"""The apex-gated foothold adaptation on the device (srbd_vfa_step_device; _lib.vfa_step_device;
BatchedVisualFootholdAdaptation.step_device / reset) against its equivalence contract: per environment srbd_vfa_mode on
the host, then -- for a searching environment -- what srbd_tamols_batch_device returns for the same inputs (which
tests/test_gpu_tamols_batch.py pins to the single-environment calls and the oracles), then srbd_vfa_commit on the host
(tests/test_vfa_gate_host.py pins both to the recorded reference).  Every comparison is bit for bit, NaNs by position;
no tolerance appears here.  Expected values never come from the gated path."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_tamols_batch import cuda, inputs

from quadruped_pympc_amd import config as mirror

pytestmark = pytest.mark.gpu
SENT = 7.25  # sentinel of the not-to-be-written entries
INTERVAL = 0.01
DT = 0.004


@pytest.fixture(scope="module")
def lib():
    from quadruped_pympc_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _lib


@pytest.fixture(scope="module")
def params():
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import tamols_params_struct

    p = dict(mirror.simulation_params["tamols_params"])
    p["h_des"] = 0.25
    return tamols_params_struct(p, "go2")


@pytest.fixture(scope="module")
def terrain(lib):
    from quadruped_pympc_amd.helpers.terrain import GpuTerrain, stepping_stones_scene

    t = GpuTerrain(**stepping_stones_scene())
    yield t
    t.close()


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)  # NaNs position for position
    if want.dtype.kind == "f":  # a NaN's sign and payload are not part of the contract
        nan = np.isnan(want)
        assert np.where(nan, 0, got).tobytes() == np.where(nan, 0, want).tobytes(), what


def plan_modes(E):
    """Interleaved: e % 4 = 0 searches (so 0 and 64 do), 1 holds, 2 passes without an apex, 3 passes by full stance."""
    return np.arange(E) % 4


def gate_state(lib, E, inp, seed, plan=None):
    """Per-environment srbd_stc / srbd_vfa structs and contacts that put environment e on the path plan[e]."""
    rng = np.random.default_rng(seed)
    plan = plan_modes(E) if plan is None else np.asarray(plan)
    stc, vfa = (lib.SrbdStc * E)(), (lib.SrbdVfa * E)()
    contact = inp["contact"].copy()
    for e in range(E):
        period = 0.25 + 0.01 * (e % 5)
        assert lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, period, 500.0, 10.0, lib.SWING_BEZIER_REF) == 0
        assert lib.lib.srbd_vfa_init(C.byref(vfa[e])) == 0
        leg = e % 4  # the leg that decides
        if plan[e] == 3:
            contact[e] = 1.0
        else:
            contact[e, leg] = 0.0
        for l in range(4):
            stc[e].swing_time[l] = rng.uniform(0.0, 0.02) if contact[e, l] == 0.0 else 0.0
        if plan[e] in (0, 1):
            stc[e].swing_time[leg] = period / 2.0 + rng.uniform(-0.005, 0.005)
        init = int(plan[e] in (1, 3))
        for l in range(4):
            vfa[e].initialized[l] = init
            vfa[e].valid[l] = int(rng.integers(0, 2))
        for k in range(12):
            vfa[e].footholds[k] = rng.uniform(-1.0, 1.0)
        for l in range(4):  # some legs hold a box, some none yet
            if (e + l) % 3:
                for k in range(6):
                    vfa[e].boxes[6 * l + k] = rng.uniform(-1.0, 1.0)
    return stc, vfa, contact


def struct_tensor(structs, nbytes):
    raw = np.frombuffer(bytes(structs), dtype=np.uint8).reshape(len(structs), nbytes).copy()
    return torch.from_numpy(raw).cuda()


def ungated(lib, terrain, p, d, rows, cols, hms=None):
    form = dict(heightmaps=hms) if hms is not None else dict(terrain=terrain, yaws=d["yaws"], rows=rows, cols=cols,
                                                              want_heightmaps=True)
    out = lib.tamols_batch_device(d["seeds"], d["hips"], p, forward_vel=d["vel"], base_pos=d["base"],
                                  contact=d["contact"], feet=d["feet"], want_seed_heights=True, want_scores=True, **form)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compose(lib, stc, vfa, contact, seeds, U):
    """The contract's right-hand side: the host structs stepped per environment (in place), the expected outputs."""
    E = len(stc)
    want = dict(footholds=np.zeros((E, 4, 3)), boxes=np.zeros((E, 4, 2, 3)), valid=np.zeros((E, 4), np.int32),
                mode=np.zeros(E, np.int32))
    p, ip = lib.dptr, lib.iptr
    for e in range(E):
        m = C.c_int32(-1)
        c = np.ascontiguousarray(contact[e], dtype=np.float64)
        assert lib.lib.srbd_vfa_mode(C.byref(vfa[e]), C.byref(stc[e]), p(c), INTERVAL, C.byref(m)) == 0
        search = m.value == lib.VFA_SEARCH
        sf = np.ascontiguousarray(U["footholds"][e]) if search else None
        sb = np.ascontiguousarray(U["boxes"][e]) if search else None
        sv = np.ascontiguousarray(U["valid"][e], dtype=np.int32) if search else None
        assert lib.lib.srbd_vfa_commit(C.byref(vfa[e]), m.value, p(np.ascontiguousarray(seeds[e])), p(sf), p(sb),
                                       ip(sv), p(want["footholds"][e]), p(want["boxes"][e]), ip(want["valid"][e])) == 0
        want["mode"][e] = m.value
    for k in ("seed_heights", "scores", "heightmaps"):
        if k in U:
            want[k] = np.where((want["mode"] == lib.VFA_SEARCH).reshape((E,) + (1,) * (U[k].ndim - 1)), U[k], SENT)
    want["ref"] = np.concatenate([np.full((E, 12), SENT), want["footholds"].reshape(E, 12)], axis=1)
    return want


def gated(lib, terrain, p, d, stc_t, vfa_t, rows, cols, hms=None, stream=None):
    E = d["seeds"].shape[0]
    nc = rows * cols
    out = dict(seed_heights=torch.full((E, 4), SENT, dtype=torch.float64, device="cuda"),
               scores=torch.full((E, 4, nc), SENT, dtype=torch.float64, device="cuda"))
    form = dict(heightmaps=hms)
    if hms is None:
        out["heightmaps"] = torch.full((E, 4, rows, cols, 3), SENT, dtype=torch.float64, device="cuda")
        form = dict(terrain=terrain, yaws=d["yaws"], rows=rows, cols=cols)
    ref = torch.full((E, 24), SENT, dtype=torch.float64, device="cuda")
    got = lib.vfa_step_device(vfa_t, stc_t, d["seeds"], d["hips"], p, d["contact"], apex_interval=INTERVAL,
                              forward_vel=d["vel"], base_pos=d["base"], feet=d["feet"], ref=ref, out=out, stream=stream,
                              **form)
    got["ref"] = ref
    return got


def check(lib, got, want, vfa_t, vfa_host, stc_t, stc_host, what):
    torch.cuda.synchronize()
    for k, w in want.items():
        same_bits(got[k], w, f"{what}: {k}")
    assert vfa_t.cpu().numpy().tobytes() == bytes(vfa_host), f"{what}: srbd_vfa bytes"
    assert stc_t.cpu().numpy().tobytes() == bytes(stc_host), f"{what}: d_stc is read only"


def run_case(lib, terrain, p, E, rows, cols, form, seed, plan=None, edit=None, edit_patches=None):
    """edit(inp, stc, vfa) changes the inputs before the upload; edit_patches(hms), patch form only, changes the
    caller's patches (E, 4, rows, cols, 3), which are raycast from the inputs as edit found them."""
    inp = inputs(E, seed)
    stc, vfa, inp["contact"] = gate_state(lib, E, inp, seed + 1, plan)
    d = {k: cuda(v) for k, v in inp.items()}
    hms = None
    if form == "patch":
        hms = ungated(lib, terrain, p, d, rows, cols)["heightmaps"]
        if edit_patches:
            edit_patches(hms)
        hms = cuda(hms)
    if edit:
        edit(inp, stc, vfa)
        d = {k: cuda(v) for k, v in inp.items()}
    U = ungated(lib, terrain, p, d, rows, cols, hms)
    stc_t, vfa_t = struct_tensor(stc, lib.STC_BYTES), struct_tensor(vfa, lib.VFA_BYTES)
    got = gated(lib, terrain, p, d, stc_t, vfa_t, rows, cols, hms)
    want = compose(lib, stc, vfa, inp["contact"], inp["seeds"], U)
    check(lib, got, want, vfa_t, vfa, stc_t, stc, f"E={E} {rows}x{cols} {form}")
    got["state"] = vfa_t
    return inp, U, got, want


@pytest.mark.parametrize("E,rows,cols,form", [(3, 13, 7, "terrain"), (3, 13, 7, "patch"), (65, 13, 7, "terrain"),
                                              (65, 13, 7, "patch"), (5, 3, 3, "terrain")])
def test_mixed_modes_in_one_launch(lib, terrain, params, E, rows, cols, form):
    inp, U, got, want = run_case(lib, terrain, params, E, rows, cols, form, 300 + E + rows)
    mode = want["mode"]
    assert mode[0] == lib.VFA_SEARCH and (E < 65 or mode[64] == lib.VFA_SEARCH)
    assert set(mode.tolist()) == {lib.VFA_PASS, lib.VFA_SEARCH, lib.VFA_HOLD}
    if E == 65 and rows == 13:  # the searches found something, and the searched rows are the ungated call's
        s = mode == lib.VFA_SEARCH
        assert U["valid"][s].any() and np.isfinite(U["scores"][s]).any()
    # a passing environment returns its seeds, a holding one not
    np.testing.assert_array_equal(want["footholds"][mode == lib.VFA_PASS], inp["seeds"][mode == lib.VFA_PASS])
    assert not np.array_equal(want["footholds"][mode == lib.VFA_HOLD], inp["seeds"][mode == lib.VFA_HOLD])


@pytest.mark.parametrize("path", [0, 1, 2, 3], ids=["search", "hold", "pass_no_apex", "pass_full_stance"])
def test_one_environment_per_mode(lib, terrain, params, path):
    _, _, _, want = run_case(lib, terrain, params, 1, 13, 7, "terrain", 40 + path, plan=[path])
    assert want["mode"][0] == (lib.VFA_SEARCH, lib.VFA_HOLD, lib.VFA_PASS, lib.VFA_PASS)[path]


def test_environments_are_independent(lib, terrain, params):
    """NaN seeds, NaN yaw and garbage hips in HOLD and PASS environments change no byte of any other environment, and
    neither does a NaN seed in one searching environment."""
    E = 12
    clean = run_case(lib, terrain, params, E, 13, 7, "terrain", 77)
    mode = clean[3]["mode"]
    quiet = np.flatnonzero(mode != lib.VFA_SEARCH)

    def poison(inp, stc, vfa):
        inp["seeds"][quiet[0::2]] = np.nan  # holding and passing ones (plan_modes: quiet = 1 2 3 5 6 7 9 10 11)
        inp["yaws"][quiet[1::4]] = np.nan
        inp["hips"][quiet[3::4]] = 1e300
        inp["yaws"][quiet[3::4]] = np.inf

    bad = run_case(lib, terrain, params, E, 13, 7, "terrain", 77, edit=poison)
    np.testing.assert_array_equal(bad[3]["mode"], mode)
    # only a PASS environment returns its own (NaN) seeds
    moved = np.array([e for e in quiet[0::2] if mode[e] == lib.VFA_PASS], dtype=int)
    assert len(moved) and (mode[quiet[0::2]] == lib.VFA_HOLD).any()
    others = np.setdiff1d(np.arange(E), moved)
    for k in ("footholds", "boxes", "valid", "ref", "seed_heights", "scores", "heightmaps"):
        same_bits(bad[2][k].cpu().numpy()[others], clean[2][k].cpu().numpy()[others], f"poisoned quiet, {k}")
    hold = np.flatnonzero(mode == lib.VFA_HOLD)
    assert np.isfinite(bad[2]["footholds"].cpu().numpy()[hold]).all()  # a holding environment returns what it holds

    victim = int(np.flatnonzero(mode == lib.VFA_SEARCH)[1])

    def poison_search(inp, stc, vfa):
        inp["seeds"][victim, 2] = np.nan

    bad = run_case(lib, terrain, params, E, 13, 7, "terrain", 77, edit=poison_search)
    others = np.setdiff1d(np.arange(E), [victim])
    for k in ("footholds", "boxes", "valid", "ref", "seed_heights", "scores", "heightmaps"):
        same_bits(bad[2][k].cpu().numpy()[others], clean[2][k].cpu().numpy()[others], f"poisoned search, {k}")


def test_environments_are_independent_patch_form(lib, terrain, params):
    """The caller's patches of HOLD and PASS environments made garbage (NaN, 1e300), and NaN seeds in some of them: no
    byte of any other environment's outputs or state changes, a holding environment returns what it holds, a passing
    one its seeds -- no non-searching block reads its patch."""
    E = 12
    clean = run_case(lib, terrain, params, E, 13, 7, "patch", 78)
    mode = clean[3]["mode"]
    quiet = np.flatnonzero(mode != lib.VFA_SEARCH)
    assert (mode[quiet] == lib.VFA_HOLD).any() and (mode[quiet] == lib.VFA_PASS).any()

    def garbage(hms):
        hms[quiet[0::2]] = np.nan
        hms[quiet[1::2]] = 1e300

    def nan_seeds(inp, stc, vfa):
        inp["seeds"][quiet[0::2]] = np.nan  # holding and passing ones

    bad = run_case(lib, terrain, params, E, 13, 7, "patch", 78, edit=nan_seeds, edit_patches=garbage)
    np.testing.assert_array_equal(bad[3]["mode"], mode)
    # only a PASS environment with NaN seeds returns other values than before: its own seeds
    moved = np.array([e for e in quiet[0::2] if mode[e] == lib.VFA_PASS], dtype=int)
    assert (mode[quiet[0::2]] == lib.VFA_HOLD).any()
    others = np.setdiff1d(np.arange(E), moved)
    for k in ("footholds", "boxes", "valid", "ref", "seed_heights", "scores", "state"):
        same_bits(bad[2][k].cpu().numpy()[others], clean[2][k].cpu().numpy()[others], f"garbage patches, {k}")
    got = bad[2]["footholds"].cpu().numpy()
    hold, passing = np.flatnonzero(mode == lib.VFA_HOLD), np.flatnonzero(mode == lib.VFA_PASS)
    assert np.isfinite(got[hold]).all()
    same_bits(got[passing], bad[0]["seeds"][passing], "a passing environment returns its seeds")
    assert len(moved) and np.isnan(got[moved]).all()
    # the searching environments did read their (clean) patches: scores were written
    assert np.isfinite(bad[2]["scores"].cpu().numpy()[mode == lib.VFA_SEARCH]).any()


def test_edge_of_the_apex_window(lib, terrain, params):
    """Clocks exactly at, one ulp inside and one ulp outside swing_period / 2 +- interval, for one and for several
    swing legs: the device's mode is srbd_vfa_mode's."""
    period = 0.25
    half = period / 2.0
    lo, hi = half - INTERVAL, half + INTERVAL
    clocks = [lo, np.nextafter(lo, 1.0), np.nextafter(lo, 0.0), hi, np.nextafter(hi, 0.0), np.nextafter(hi, 1.0), half]
    cases = []
    for t in clocks:
        cases.append(([0.0, 1.0, 1.0, 1.0], [t, 0.0, 0.0, 0.0]))               # one swing leg
        cases.append(([0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, t]))               # two, the last one decides
        cases.append(([0.0, 0.0, 0.0, 0.0], [hi, lo, t, np.nextafter(lo, 0)]))  # four, three of them outside
        cases.append(([1.0, 1.0, 1.0, 1.0], [t, t, t, t]))                     # the clock of a stance leg does not count
    E = len(cases)

    def edit(inp, stc, vfa):
        for e, (c, t) in enumerate(cases):
            inp["contact"][e] = c
            stc[e].swing_period = period
            for l in range(4):
                stc[e].swing_time[l] = t[l]
                vfa[e].initialized[l] = 0

    _, _, _, want = run_case(lib, terrain, params, E, 3, 3, "terrain", 91, plan=[2] * E, edit=edit)
    mode = want["mode"].reshape(len(clocks), 4)
    inside = [False, True, False, False, True, False, True]
    for i, ins in enumerate(inside):
        exp = lib.VFA_SEARCH if ins else lib.VFA_PASS
        assert mode[i].tolist() == [exp, exp, exp, lib.VFA_PASS], (i, clocks[i])


def test_stale_constraint_through_the_class(lib, terrain, params):
    """A search with an infeasible leg after an earlier feasible one returns the earlier box for that leg, valid 0."""
    from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation

    E = 4
    inp = inputs(E, 5)
    stc, _, inp["contact"] = gate_state(lib, E, inp, 6, plan=[0] * E)
    d = {k: cuda(v) for k, v in inp.items()}
    stc_t = struct_tensor(stc, lib.STC_BYTES)
    vfa = BatchedVisualFootholdAdaptation(E)
    vfa.tamols_params = dict(mirror.simulation_params["tamols_params"], h_des=0.25)
    args = (d["vel"], d["base"], d["contact"], d["feet"])
    f1, b1, v1, m1 = (t.clone() for t in vfa.step_device(d["seeds"], d["hips"], *args, stc=stc_t, terrain=terrain,
                                                         yaws=d["yaws"]))
    vfa.reset()  # in stream order; as a full stance would
    hips = d["hips"].clone()
    hips[:, 1, 2] += 1.7  # FR: nothing in reach
    f2, b2, v2, m2 = vfa.step_device(d["seeds"], hips, *args, stc=stc_t, terrain=terrain, yaws=d["yaws"])
    torch.cuda.synchronize()
    assert m1.tolist() == [lib.VFA_SEARCH] * E == m2.tolist()
    feasible = v1[:, 1].cpu().numpy() == 1
    assert feasible.any() and not v2[:, 1].any()
    same_bits(b2[:, 1][feasible], b1[:, 1].cpu().numpy()[feasible], "the earlier box")
    assert torch.isnan(b2[:, 1][~torch.from_numpy(feasible).cuda()]).all()
    np.testing.assert_array_equal(f2[:, 1, :2].cpu().numpy(), inp["seeds"][:, 1, :2])  # the seed at its height
    st = vfa.state_dict()
    assert all(list(st[e].initialized) == [1] * 4 and st[e].valid[1] == 0 for e in range(E))
    # hold: the same answer again, nothing searched
    f3, b3, v3, m3 = vfa.step_device(d["seeds"] + 1.0, hips, *args, stc=stc_t, terrain=terrain, yaws=d["yaws"])
    torch.cuda.synchronize()
    assert m3.tolist() == [lib.VFA_HOLD] * E
    same_bits(f3, f2.cpu().numpy(), "held footholds")


def test_ungated_call_unchanged(lib, terrain, params):
    E = 9
    inp = inputs(E, 123)
    stc, vfa, inp["contact"] = gate_state(lib, E, inp, 124)
    d = {k: cuda(v) for k, v in inp.items()}
    stc_t, vfa_t = struct_tensor(stc, lib.STC_BYTES), struct_tensor(vfa, lib.VFA_BYTES)
    before = ungated(lib, terrain, params, d, 13, 7)
    assert vfa_t.cpu().numpy().tobytes() == bytes(vfa)  # untouched by the ungated call
    gated(lib, terrain, params, d, stc_t, vfa_t, 13, 7)
    after_state = vfa_t.clone()
    after = ungated(lib, terrain, params, d, 13, 7)
    for k in before:
        same_bits(after[k], before[k], f"ungated {k}")
    assert torch.equal(vfa_t, after_state)


# ------------------------------------------------------------------ the loop
class Loop:
    """gait.run -> frg.step -> vfa.step_device -> stc.step for E = 3 environments (trot, pace, a trot at another step
    frequency and start phase) on synthetic dynamics, every step's outputs kept in preallocated device tensors."""

    def __init__(self, lib, terrain, steps):
        from quadruped_pympc_amd.helpers.foothold_reference_generator import BatchedFootholdReferenceGenerator
        from quadruped_pympc_amd.helpers.periodic_gait_generator import BatchedPeriodicGaitGenerator
        from quadruped_pympc_amd.helpers.swing_trajectory_controller import BatchedSwingTrajectoryController
        from quadruped_pympc_amd.helpers.visual_foothold_adaptation import BatchedVisualFootholdAdaptation
        from test_gpu_stc_device import args_of, draw_inputs, upload

        E = self.E = 3
        self.lib, self.terrain, self.K = lib, terrain, steps
        self.duty, self.freq = np.array([0.65, 0.7, 0.6]), np.array([1.4, 1.4, 2.0])
        self.period = (1.0 - self.duty) / self.freq
        self.gait = BatchedPeriodicGaitGenerator(E, self.duty, self.freq, [0, 1, 0], 12)
        st = self.gait.state_dict()
        # start phases with the start-up hold cleared, so that 200 steps of 0.004 s hold two swings of every leg pair
        for e, phases in enumerate(((0.0, 0.5, 0.5, 0.0), (0.8, 0.3, 0.8, 0.3), (0.3, 0.8, 0.8, 0.3))):
            for l, ph in enumerate(phases):
                st[e].phase_signal[l] = ph
                st[e].init[l] = 0
        self.gait.load_state_dict(st)
        inp = inputs(E, 9)
        self.inp = inp
        self.frg = BatchedFootholdReferenceGenerator(E, self.duty / self.freq, 0.3, inp["feet"])
        self.stc = BatchedSwingTrajectoryController(E, 0.06, self.period, 500.0, 10.0)
        self.vfa = BatchedVisualFootholdAdaptation(E)
        self.vfa.tamols_params = dict(mirror.simulation_params["tamols_params"], h_des=0.25)
        self.d = {k: cuda(v) for k, v in inp.items()}
        self.ref_vel = cuda(np.tile([0.4, 0.0, 0.0], (E, 1)))
        x = draw_inputs(np.random.default_rng(3), E, 0)
        self.dyn = upload(x)
        self.args_of = args_of
        z = lambda *s, dt=torch.float64: torch.full((steps,) + s, SENT, dtype=dt, device="cuda")  # noqa: E731
        self.contact, self.seeds = z(E, 4, dt=torch.float32), z(E, 4, 3)
        self.fh, self.bx, self.va, self.mo = z(E, 4, 3), z(E, 4, 2, 3), z(E, 4, dt=torch.int32), z(E, dt=torch.int32)
        self.ref = z(E, 24)
        self.state = torch.zeros((steps, E, lib.VFA_BYTES), dtype=torch.uint8, device="cuda")
        self.clocks = z(E, 4)
        self.U = {k: z(*s, dt=dt) for k, s, dt in (("footholds", (E, 4, 3), torch.float64),
                                                   ("boxes", (E, 4, 2, 3), torch.float64),
                                                   ("valid", (E, 4), torch.int32))}
        self.prev = torch.ones((E, 4), dtype=torch.float32, device="cuda")

    def step(self, k, sync=False):
        d, lib = self.d, self.lib
        wait = torch.cuda.synchronize if sync else (lambda: None)
        c = self.gait.run(DT)
        self.contact[k].copy_(c)
        wait()
        self.frg.step(d["base"], d["yaws"], d["vel"], self.ref_vel, d["hips"], d["feet"], self.prev, c, gait=self.gait,
                      out=self.seeds[k], com_height_nominal=0.3)
        wait()
        self.clocks[k].copy_(self.stc.swing_time)
        # the ungated call on the same inputs: what a searching environment must return
        lib.tamols_batch_device(self.seeds[k], d["hips"], self.vfa._params(), terrain=self.terrain, yaws=d["yaws"],
                                forward_vel=d["vel"], base_pos=d["base"], contact=c, feet=d["feet"],
                                out={n: t[k] for n, t in self.U.items()})
        f, b, v, m = self.vfa.step_device(self.seeds[k], d["hips"], d["vel"], d["base"], c, d["feet"], stc=self.stc,
                                          terrain=self.terrain, yaws=d["yaws"], ref=self.ref[k],
                                          out=dict(footholds=self.fh[k], boxes=self.bx[k], valid=self.va[k],
                                                   mode=self.mo[k]))
        wait()
        self.state[k].copy_(self.vfa.state)
        x = dict(self.dyn, contact=c, touch_down=f)  # the consumer: the swing controller lands on the footholds
        self.stc.step(DT, *self.args_of(x), frg=self.frg, apex_interval=INTERVAL)
        wait()
        self.prev = c

    def results(self):
        torch.cuda.synchronize()
        names = ("contact", "seeds", "fh", "bx", "va", "mo", "ref", "state", "clocks")
        out = {n: getattr(self, n).cpu().numpy() for n in names}
        out["U"] = {k: v.cpu().numpy() for k, v in self.U.items()}
        return out


def test_closed_loop_against_the_host_mirrors(lib, terrain):
    """200 steps of the device loop.  What is mirrored on the host, per environment and per step, is the gate and what
    it reads: srbd_vfa_mode / srbd_vfa_commit on host srbd_vfa structs and the swing clocks by
    srbd_stc_update_swing_time.  The contacts and seeds the mirrors are fed are the device run's (the gait generator and
    the foothold reference generator have their own device tests), and a searching environment's search result is the
    ungated call's on the same inputs."""
    K = 200
    loop = Loop(lib, terrain, K)
    for k in range(K):
        loop.step(k)
    r = loop.results()  # the single synchronisation
    E = loop.E
    stc, vfa = (lib.SrbdStc * E)(), (lib.SrbdVfa * E)()
    for e in range(E):
        assert lib.lib.srbd_stc_init(C.byref(stc[e]), 0.06, loop.period[e], 500.0, 10.0, lib.SWING_BEZIER_REF) == 0
        assert lib.lib.srbd_vfa_init(C.byref(vfa[e])) == 0
    seen = np.zeros((E, 3), dtype=int)
    for k in range(K):
        for e in range(E):
            assert list(stc[e].swing_time) == r["clocks"][k, e].tolist(), (k, e)
        U = {n: v[k] for n, v in r["U"].items()}
        want = compose(lib, stc, vfa, r["contact"][k], r["seeds"][k], U)
        for got, name in ((r["fh"], "footholds"), (r["bx"], "boxes"), (r["va"], "valid"), (r["mo"], "mode")):
            same_bits(got[k], want[name], f"step {k}: {name}")
        same_bits(r["ref"][k][:, 12:], want["ref"][:, 12:], f"step {k}: ref feet")
        assert r["state"][k].tobytes() == bytes(vfa), f"step {k}: srbd_vfa bytes"
        for e in range(E):
            seen[e, want["mode"][e]] += 1
            c = np.ascontiguousarray(r["contact"][k, e], dtype=np.float64)
            assert lib.lib.srbd_stc_update_swing_time(C.byref(stc[e]), lib.dptr(c), DT) == 0
    print("steps per mode (pass, search, hold) per environment:", seen.tolist())
    assert (seen > 0).all() and (seen[:, lib.VFA_SEARCH] >= 2).all(), seen  # not on pass-throughs alone


def test_stream_order(lib, terrain):
    """Seeds, contacts and d_stc produced by earlier launches on a non-default stream, the outputs consumed by a later
    launch on it, no synchronisation in between: the results equal the synchronised run."""
    K = 70  # past the first apex of every environment
    s = torch.cuda.Stream()
    a = Loop(lib, terrain, K)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for k in range(K):
            a.step(k)
    ra = a.results()
    b = Loop(lib, terrain, K)
    for k in range(K):
        b.step(k, sync=True)
    rb = b.results()
    assert (ra["mo"] == lib.VFA_SEARCH).any() and (ra["mo"] == lib.VFA_HOLD).any()
    for n in ("contact", "seeds", "fh", "bx", "va", "mo", "ref", "state", "clocks"):
        same_bits(ra[n], rb[n], f"stream order: {n}")
    assert bytes(a.stc.state_dict()) == bytes(b.stc.state_dict())
