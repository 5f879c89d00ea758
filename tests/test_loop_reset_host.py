"""The per-environment reset of the loop's state on the host (srbd_loop_reset, include/srbd_host.h; csrc/srbd_reset.h):
the oracle of the device form.  Level 1 against values recorded from the reference's own reset statements
(tests/golden/loop_reset_ref.npz, made by tests/golden/record_loop_reset_reference.py), level 2 against fresh
constructor calls, byte for byte.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

from quadruped_pympc_amd import _lib

lib = _lib.lib
HERE = os.path.dirname(os.path.abspath(__file__))
REF = np.load(os.path.join(HERE, "golden", "loop_reset_ref.npz"))
STRUCTS = (("pgg", _lib.SrbdPgg), ("frg", _lib.SrbdFrg), ("stc", _lib.SrbdStc), ("terrain_est", _lib.SrbdTerrainEst),
           ("vfa", _lib.SrbdVfa))
P = 36


def dp(a):
    return None if a is None else a.ctypes.data_as(_lib._DP)


def reset(level, feet=None, parts=None, snaps=None, edge=None, best=None, num_params=None):
    """srbd_loop_reset on the given structs (dicts name -> ctypes struct)."""
    parts, snaps = parts or {}, snaps or {}
    args = [C.byref(parts[n]) if n in parts else None for n, _ in STRUCTS]
    args += [C.byref(snaps[n]) if n in snaps else None for n, _ in STRUCTS]
    return lib.srbd_loop_reset(level, dp(feet), *args, None if edge is None else edge.ctypes.data_as(_lib._IP),
                               None if best is None else best.ctypes.data_as(_lib._FP),
                               (0 if best is None else best.size) if num_params is None else num_params)


def fresh(rng, feet=None):
    """One environment's structs as their constructor calls produce them, and the feet the foothold generator got."""
    feet = rng.uniform(-0.4, 0.4, (4, 3)) if feet is None else feet
    s = {n: t() for n, t in STRUCTS}
    assert lib.srbd_pgg_init(C.byref(s["pgg"]), int(rng.integers(0, 8)), 0.65, 1.4, 12) == _lib.OK
    assert lib.srbd_frg_init(C.byref(s["frg"]), 0.46, 0.28, dp(np.ascontiguousarray(feet))) == _lib.OK
    assert lib.srbd_stc_init(C.byref(s["stc"]), 0.06, 0.25, 100.0, 10.0, int(rng.integers(0, 2))) == _lib.OK
    assert lib.srbd_terrain_est_init(C.byref(s["terrain_est"])) == _lib.OK
    assert lib.srbd_vfa_init(C.byref(s["vfa"])) == _lib.OK
    return s, feet


def dirty(rng, like):
    """Structs of random bytes (the gait type kept: it is configuration the reference's reset reads)."""
    out = {}
    for n, t in STRUCTS:
        out[n] = t.from_buffer_copy(rng.integers(0, 256, C.sizeof(t), dtype=np.uint8).tobytes())
    out["pgg"].gait_type = like["pgg"].gait_type
    return out


def copy_of(parts):
    return {n: type(s).from_buffer_copy(bytes(s)) for n, s in parts.items()}


def pgg_from(prefix, i):
    g = _lib.SrbdPgg()
    g.duty_factor, g.step_freq = float(REF[prefix + "duty_factor"][i]), float(REF[prefix + "step_freq"][i])
    g.phase_signal[:] = REF[prefix + "phase_signal"][i].tolist()
    g.phase_offset[:] = REF[prefix + "phase_offset"][i].tolist()
    g.init[:] = REF[prefix + "init"][i].tolist()
    g.gait_type, g.previous_gait_type = int(REF[prefix + "gait_type"][i]), int(REF[prefix + "previous_gait_type"][i])
    g.horizon = 12
    return g


def check_pgg(g, prefix, i):
    assert np.array_equal(np.array(g.phase_signal[:]), REF[prefix + "phase_signal"][i])
    assert np.array_equal(np.array(g.phase_offset[:]), REF[prefix + "phase_offset"][i])
    assert np.array_equal(np.array(g.init[:]), REF[prefix + "init"][i])
    assert g.gait_type == REF[prefix + "gait_type"][i] and g.previous_gait_type == REF[prefix + "previous_gait_type"][i]
    assert g.step_freq == REF[prefix + "step_freq"][i] and g.duty_factor == REF[prefix + "duty_factor"][i]


def test_fixture_covers_what_the_issue_names():
    cases = set(zip(REF["pgg_case"].tolist(), REF["pgg_gait"].tolist()))
    for gait in range(8):
        for name in ("run0", "run1", "run37", "hold", "full_stance", "freq"):
            assert (name, gait) in cases
    hold = REF["pgg_case"] == "hold"
    assert REF["pgg_before_init"][hold].any(axis=1).sum() >= 7 and not REF["pgg_after_init"].any()
    assert (REF["pgg_before_gait_type"][REF["pgg_case"] == "full_stance"] == 7).all()
    assert os.path.getsize(os.path.join(HERE, "golden", "loop_reset_ref.npz")) < 64 * 1024


@pytest.mark.parametrize("i", range(len(REF["pgg_case"])), ids=lambda i: f"{REF['pgg_case'][i]}-g{REF['pgg_gait'][i]}")
def test_level_1_gait_generator_equals_the_reference(i):
    g = pgg_from("pgg_before_", i)
    assert reset(1, parts={"pgg": g}) == _lib.OK
    check_pgg(g, "pgg_after_", i)
    h = pgg_from("pgg_before_", i)  # srbd_pgg_reset is the same statement
    assert lib.srbd_pgg_reset(C.byref(h)) == _lib.OK and bytes(h) == bytes(g)


def frg_from(prefix, i):
    f = _lib.SrbdFrg()
    f.stance_time, f.hip_height = float(REF[prefix + "stance_time"][i]), float(REF[prefix + "hip_height"][i])
    f.hip_offset = float(REF[prefix + "hip_offset"][i])
    for name in ("lift_off", "lift_off_h", "touch_down", "touch_down_h", "last_reference_footholds"):
        src = np.ascontiguousarray(REF[prefix + name][i], dtype=np.float64)  # named: alive while memmove reads it
        assert src.nbytes == 96
        C.memmove(getattr(f, name), src.ctypes.data, src.nbytes)
    src = np.ascontiguousarray(REF[prefix + "vel_hist"][i], dtype=np.float64)
    assert src.nbytes == 320
    C.memmove(f.vel_hist, src.ctypes.data, src.nbytes)
    n = int(REF[prefix + "hist_len"][i])
    f.hist_len, f.hist_head = n, n % _lib.FRG_HIST
    return f


def table(f, name):
    return np.ctypeslib.as_array(getattr(f, name)).copy()


@pytest.mark.parametrize("i", range(len(REF["wbi_initial_feet"])))
def test_level_1_equals_wbinterface_reset(i):
    g, f, v = pgg_from("wbi_before_pgg_", i), frg_from("wbi_before_frg_", i), _lib.SrbdVfa()
    lib.srbd_vfa_init(C.byref(v))
    v.initialized[:] = [int(REF["wbi_before_vfa_initialized"][i])] * 4
    v.footholds[:] = REF["wbi_before_vfa_footholds"][i].reshape(-1).tolist()
    rng = np.random.default_rng(i)
    s, _ = fresh(rng)
    stc, terr = dirty(rng, s)["stc"], dirty(rng, s)["terrain_est"]
    parts = {"pgg": g, "frg": f, "stc": stc, "terrain_est": terr, "vfa": v}
    before = copy_of(parts)
    edge, best = np.array([1], dtype=np.int32), rng.standard_normal(P).astype(np.float32)
    best0 = best.copy()
    feet = np.ascontiguousarray(REF["wbi_initial_feet"][i])
    assert reset(1, feet, parts, edge=edge, best=best) == _lib.OK  # no snapshot is needed at level 1
    check_pgg(g, "wbi_after_pgg_", i)
    for name in ("lift_off", "lift_off_h", "touch_down", "touch_down_h", "last_reference_footholds", "vel_hist"):
        assert np.array_equal(table(f, name), REF["wbi_after_frg_" + name][i]), name
    assert np.array_equal(table(f, "lift_off"), feet)
    assert f.hist_len == REF["wbi_after_frg_hist_len"][i] and f.stance_time == REF["wbi_after_frg_stance_time"][i]
    assert list(v.initialized) == [int(REF["wbi_after_vfa_initialized"][i])] * 4 == [0] * 4
    assert np.array_equal(np.array(v.footholds[:]).reshape(4, 3), REF["wbi_after_vfa_footholds"][i])
    # what the reference leaves alone is bit-identical: stc, the terrain filter, the trigger, the warm start, and of
    # the three structs it does touch everything but the fields above
    assert bytes(stc) == bytes(before["stc"]) and bytes(terr) == bytes(before["terrain_est"])
    assert edge[0] == 1 and np.array_equal(best, best0)
    keep = before["frg"]
    C.memmove(keep.lift_off, feet.ctypes.data, 96)
    assert bytes(f) == bytes(keep)
    keep = before["vfa"]
    keep.initialized[:] = [0] * 4
    assert bytes(v) == bytes(keep)
    keep = before["pgg"]
    lib.srbd_pgg_reset(C.byref(keep))
    assert bytes(g) == bytes(keep) and g.step_freq == before["pgg"].step_freq
    assert (REF["wbi_after_current_contact"][i] == 1).all()  # the caller's rows: the device call's contact_rows


def test_vfa_reset_alone_equals_the_reference():
    v = _lib.SrbdVfa()
    lib.srbd_vfa_init(C.byref(v))
    v.initialized[:] = [int(REF["vfa_before_initialized"])] * 4
    v.footholds[:] = REF["vfa_before_footholds"].reshape(-1).tolist()
    w = _lib.SrbdVfa.from_buffer_copy(bytes(v))
    assert reset(1, parts={"vfa": v}) == _lib.OK and lib.srbd_vfa_reset(C.byref(w)) == _lib.OK
    assert bytes(v) == bytes(w) and list(v.initialized) == [int(REF["vfa_after_initialized"])] * 4
    assert np.array_equal(np.array(v.footholds[:]).reshape(4, 3), REF["vfa_after_footholds"])


@pytest.mark.parametrize("seed", range(4))
def test_level_2_equals_fresh_constructor_calls(seed):
    rng = np.random.default_rng(100 + seed)
    snaps, feet0 = fresh(rng)
    parts = dirty(rng, snaps)
    new_feet = np.ascontiguousarray(rng.uniform(-0.4, 0.4, (4, 3)))
    edge, best = np.array([1], dtype=np.int32), rng.standard_normal(P).astype(np.float32)
    assert reset(2, new_feet, parts, snaps, edge, best) == _lib.OK
    want = copy_of(snaps)
    assert lib.srbd_frg_init(C.byref(want["frg"]), 0.46, 0.28, dp(new_feet)) == _lib.OK
    for n, _ in STRUCTS:
        assert bytes(parts[n]) == bytes(want[n]), n
    f = parts["frg"]
    for name in ("lift_off", "lift_off_h", "touch_down", "touch_down_h"):
        assert np.array_equal(table(f, name), new_feet)
    assert f.hist_len == 0 and f.hist_head == 0 and not table(f, "vel_hist").any()
    assert not table(f, "last_reference_footholds").any() and f.hip_offset == 0.1
    assert edge[0] == 0 and not best.any() and np.array_equal(np.signbit(best), np.zeros(P, bool))
    # the snapshot's scalars win over what a step-frequency write-back left (srbd_gait_apply_freq)
    assert parts["pgg"].step_freq == 1.4 and parts["stc"].swing_period == 0.25 and f.stance_time == 0.46


def test_level_2_each_piece_alone_and_none():
    rng = np.random.default_rng(7)
    snaps, _ = fresh(rng)
    feet = np.ascontiguousarray(rng.uniform(-0.4, 0.4, (4, 3)))
    assert reset(1) == _lib.OK and reset(2) == _lib.OK  # nothing given: nothing to do
    for n, _ in STRUCTS:
        parts = dirty(rng, snaps)
        before = copy_of(parts)
        assert reset(2, feet, {n: parts[n]}, {n: snaps[n]}) == _lib.OK
        for m, _ in STRUCTS:
            if m != n:
                assert bytes(parts[m]) == bytes(before[m])
        assert bytes(parts[n]) != bytes(before[n])


def test_every_refusal_changes_nothing():
    rng = np.random.default_rng(11)
    snaps, _ = fresh(rng)
    parts = dirty(rng, snaps)
    before = copy_of(parts)
    feet = np.ascontiguousarray(rng.uniform(-0.4, 0.4, (4, 3)))
    edge, best = np.array([1], dtype=np.int32), np.ones(P, dtype=np.float32)

    def unchanged():
        return all(bytes(parts[n]) == bytes(before[n]) for n, _ in STRUCTS) and edge[0] == 1 and (best == 1).all()

    for level in (0, 3, -1, 7, 2 ** 31 - 1):
        assert reset(level, feet, parts, snaps, edge, best) == _lib.E_INVALID and unchanged(), level
    for level in (1, 2):
        assert reset(level, None, parts, snaps, edge, best) == _lib.E_INVALID and unchanged()  # frg without feet
        for bad in (0, -1):
            assert reset(level, feet, parts, snaps, edge, best, num_params=bad) == _lib.E_INVALID and unchanged()
    for n, _ in STRUCTS:  # level 2: a struct without its snapshot
        short = {m: s for m, s in snaps.items() if m != n}
        assert reset(2, feet, parts, short, edge, best) == _lib.E_INVALID and unchanged(), n
    # without the foothold generator the feet are not needed
    rest = {m: s for m, s in parts.items() if m != "frg"}
    assert reset(2, None, rest, snaps, edge, best) == _lib.OK


def test_constructors_and_resets_keep_their_bytes():
    """srbd_pgg_reset, srbd_frg_init and srbd_vfa_reset now run the shared statements of csrc/srbd_reset.h."""
    for gait, off in ((0, [0.5, 1.0, 1.0, 0.5]), (1, [0.8, 0.3, 0.8, 0.3]), (2, [0.5, 0.5, 0.0, 0.0]),
                      (3, [0.0, 0.25, 0.75, 0.5]), (4, [0.0, 0.25, 0.5, 0.75]), (5, [0.0, 0.5, 0.75, 0.25]),
                      (6, [0.5, 1.0, 0.75, 1.25]), (7, [0.0, 0.5, 0.5, 0.0]), (-3, [0.0, 0.5, 0.5, 0.0]),
                      (99, [0.0, 0.5, 0.5, 0.0])):
        g = _lib.SrbdPgg()
        assert lib.srbd_pgg_init(C.byref(g), gait, 0.65, 1.4, 12) == _lib.OK
        assert list(g.phase_offset) == off and list(g.phase_signal) == off and list(g.init) == [0] * 4
    f = _lib.SrbdFrg.from_buffer_copy(b"\xff" * C.sizeof(_lib.SrbdFrg))
    feet = np.arange(12, dtype=np.float64).reshape(4, 3) - 0.5
    assert lib.srbd_frg_init(C.byref(f), 0.4, 0.3, dp(feet)) == _lib.OK
    want = _lib.SrbdFrg()
    want.stance_time, want.hip_height, want.hip_offset = 0.4, 0.3, 0.1
    for name in ("lift_off", "lift_off_h", "touch_down", "touch_down_h"):
        C.memmove(getattr(want, name), feet.ctypes.data, 96)
    assert bytes(f) == bytes(want)
    assert lib.srbd_frg_init(C.byref(f), 0.5, 0.3, C.cast(f.touch_down, _lib._DP)) == _lib.OK  # a table of its own
    assert np.array_equal(table(f, "lift_off"), feet) and f.stance_time == 0.5
