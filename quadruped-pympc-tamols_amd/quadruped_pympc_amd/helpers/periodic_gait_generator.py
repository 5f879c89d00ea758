"""Periodic gait generator: the producer of the (4, H) ``contact_sequence`` the sampling MPC consumes.

Mirror of ``quadruped_pympc/helpers/periodic_gait_generator.py`` (reference): the same
constructor, attributes and methods (phase offsets per gait :22-46, ``run`` :48-76,
``set_phase_signal`` :78-87, ``compute_contact_sequence`` :93-118, full stance -> 2H ones).
The state lives in a ``srbd_pgg`` struct and every method runs in ``libsrbd_hip.so``'s C++
host producers (``include/srbd_host.h``), so the 100 Hz loop pays one
ctypes call per sequence instead of H NumPy passes.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib

TROT, PACE, BOUNDING, CIRCULARCRAWL, BFDIAGONALCRAWL, BACKDIAGONALCRAWL, FRONTDIAGONALCRAWL, FULL_STANCE = range(8)


def _check(rc, what):
    if rc < 0:
        raise ValueError(f"{what} failed ({rc})")
    return rc


def _check_lengths(lens, n_dts, horizon, gait_type):
    """Raise IndexError where the reference's loop (PGG:111-115) would read contact_sequence_lenghts past its end
    (the library reads lens[j] for j < n_dts only, so a shorter lengths array is walked here first)."""
    if len(lens) >= n_dts or gait_type == FULL_STANCE:
        return
    j = 0
    for i in range(1, horizon):
        if j >= len(lens):
            raise IndexError("compute_contact_sequence: contact_sequence_lenghts too short")
        if i >= lens[j]:
            j += 1
        if j >= n_dts:
            return  # dts[j] past the end: the library reports it


class PeriodicGaitGenerator:
    def __init__(self, duty_factor, step_freq, gait_type, horizon):
        self._g = _lib.SrbdPgg()
        self._gp = C.byref(self._g)
        _check(_lib.lib.srbd_pgg_init(self._gp, int(getattr(gait_type, "value", gait_type)), float(duty_factor),
                                      float(step_freq), int(horizon)), "srbd_pgg_init")
        self.start_and_stop_activated = False
        self.time_before_switch_freq = 0
        self._seq_key = None  # (dts, lens) bytes of the cached sequence-call arguments
        self._out = np.empty(8 * _lib.MAX_HORIZON)
        self._out_p = _lib.dptr(self._out)
        self._addr = C.addressof(self._g)

    # plain attributes of the reference, backed by the C struct
    duty_factor = property(lambda s: s._g.duty_factor, lambda s, v: setattr(s._g, "duty_factor", float(v)))
    step_freq = property(lambda s: s._g.step_freq, lambda s, v: setattr(s._g, "step_freq", float(v)))
    horizon = property(lambda s: s._g.horizon, lambda s, v: setattr(s._g, "horizon", int(v)))
    gait_type = property(lambda s: s._g.gait_type, lambda s, v: setattr(s._g, "gait_type", int(getattr(v, "value", v))))
    previous_gait_type = property(lambda s: s._g.previous_gait_type,
                                  lambda s, v: setattr(s._g, "previous_gait_type", int(getattr(v, "value", v))))
    n_contact = 4

    @property
    def phase_offset(self):
        return list(self._g.phase_offset)

    @property
    def _init(self):
        return np.array(self._g.init, dtype=bool)

    def reset(self):
        _lib.lib.srbd_pgg_reset(self._gp)
        self.time_before_switch_freq = 0

    def run(self, dt, new_step_freq):
        out = np.zeros(4)
        _lib.lib.srbd_pgg_run(self._gp, float(dt), float(new_step_freq), _lib.dptr(out))
        return out

    def set_phase_signal(self, phase_signal, init=None):
        assert len(phase_signal) == 4
        ph = np.ascontiguousarray(phase_signal, dtype=np.float64)
        ini = None if init is None else np.ascontiguousarray(init, dtype=np.int32)
        _lib.lib.srbd_pgg_set_phase_signal(self._gp, _lib.dptr(ph), _lib.iptr(ini))

    @property
    def phase_signal(self):
        return np.array(self._g.phase_signal)

    def compute_contact_sequence(self, contact_sequence_dts, contact_sequence_lenghts):
        if _lib.fast is not None:  # the same C call, its arguments and result array handled in C (_srbd_fast)
            return _lib.fast.pgg_contact_sequence(self._addr, contact_sequence_dts, contact_sequence_lenghts)
        key = (np.asarray(contact_sequence_dts, dtype=np.float64).tobytes(),
               np.asarray(contact_sequence_lenghts, dtype=np.int32).tobytes())
        _check_lengths(np.frombuffer(key[1], dtype=np.int32), len(key[0]) // 8, self._g.horizon, self._g.gait_type)
        if key != self._seq_key:  # the 100 Hz caller passes the same arrays every step
            self._dts = np.frombuffer(key[0], dtype=np.float64).copy()
            self._lens = np.frombuffer(key[1], dtype=np.int32).copy()
            self._dts_p, self._lens_p = _lib.dptr(self._dts), _lib.iptr(self._lens)
            self._seq_key = key
        H = self._g.horizon
        cols = _check(_lib.lib.srbd_pgg_contact_sequence(self._gp, self._dts_p, self._lens_p, len(self._dts),
                                                         self._out_p, min(self._out.size, 8 * H)),
                      "compute_contact_sequence")
        return self._out[:4 * cols].reshape(4, cols).copy()  # row-major 4 x cols

    def set_full_stance(self):
        self.gait_type = FULL_STANCE
        self.reset()

    def restore_previous_gait(self):
        self.gait_type = self.previous_gait_type
        self.reset()

    def update_start_and_stop(self, feet_pos, hip_pos, hip_offset, base_pos, base_ori_euler_xyz, base_lin_vel,
                              base_ang_vel, ref_base_lin_vel, ref_base_ang_vel, current_contact):
        """The reference's ``update_start_and_stop`` (PGG:128-196) in one ``srbd_pgg_start_stop`` call: full stance
        when the robot stands still with no command, the previous gait back when it does not.  feet_pos / hip_pos:
        a ``LegsAttr`` (FL FR RL RR) or a (4, 3) array.  Returns 0 / 1 / 2: untouched / stopped / restored (the
        reference returns None)."""
        def legs(p):
            if all(hasattr(p, n) for n in ("FL", "FR", "RL", "RR")):
                p = [p.FL, p.FR, p.RL, p.RR]
            return np.ascontiguousarray(p, dtype=np.float64).reshape(4, 3)

        def vec(v, n):
            return np.ascontiguousarray(v, dtype=np.float64).reshape(n)

        feet, hips = legs(feet_pos), legs(hip_pos)
        args = [vec(base_pos, 3), vec(base_ori_euler_xyz, 3), vec(base_lin_vel, 3), vec(base_ang_vel, 3),
                vec(ref_base_lin_vel, 3), vec(ref_base_ang_vel, 3), vec(current_contact, 4)]
        action = _check(_lib.lib.srbd_pgg_start_stop(self._gp, _lib.dptr(feet), _lib.dptr(hips), float(hip_offset),
                                                     *[_lib.dptr(a) for a in args]), "update_start_and_stop")
        if action:
            self.time_before_switch_freq = 0  # reset()'s
        return action


class BatchedPeriodicGaitGenerator:
    """``num_envs`` periodic gait generators whose state lives on the device (``srbd_pgg_run_device``,
    ``srbd_pgg_contact_sequence_device``, include/srbd_mpc.h): the producer of the (E, 4, H) contact sequences
    ``BatchContext.step_device`` consumes, with no host round trip.

    Environment ``e`` behaves as a ``PeriodicGaitGenerator(duty_factor[e], step_freq[e], gait_type[e], horizon)``
    that received the same calls: its state keeps the host struct's bytes and its contact flags are the host's,
    as float32.  ``duty_factor``, ``step_freq`` and ``gait_type`` are scalars or length-E sequences; the gait types
    are fixed at construction.  The state is one (E, sizeof(srbd_pgg)) uint8 tensor, ``state``, built from host
    ``srbd_pgg_init`` structs; ``phase_signal`` (E, 4) float64 and ``init`` (E, 4) int32 are views of it.  Every
    method enqueues on ``stream`` (None: torch's current stream) and does not wait for the device, except
    ``state_dict``.  A FULL_STANCE environment's sequence is H columns of ones (the step reads no more), not the
    host class's 2 H."""

    n_contact = 4

    def __init__(self, num_envs, duty_factor, step_freq, gait_type, horizon, device=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        if not 1 <= int(horizon) <= _lib.MAX_HORIZON:
            raise ValueError(f"horizon must be 1..{_lib.MAX_HORIZON}, got {horizon}")

        def per_env(name, v, dtype):
            a = np.asarray([getattr(x, "value", x) for x in v] if isinstance(v, (list, tuple)) else
                           getattr(v, "value", v), dtype=dtype)
            if a.ndim == 0:
                return np.full(E, a, dtype=dtype)
            if a.shape != (E,):
                raise ValueError(f"{name} must be a scalar or have {E} entries, got shape {a.shape}")
            return a

        duty = per_env("duty_factor", duty_factor, np.float64)
        freq = per_env("step_freq", step_freq, np.float64)
        gait = per_env("gait_type", gait_type, np.int32)
        self.num_envs, self.horizon = E, int(horizon)
        host = (_lib.SrbdPgg * E)()
        for e in range(E):
            _check(_lib.lib.srbd_pgg_init(C.byref(host[e]), int(gait[e]), float(duty[e]), float(freq[e]),
                                          self.horizon), "srbd_pgg_init")
        self._seq_key = None
        # everything above is host work; the upload is the first use of the device
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("BatchedPeriodicGaitGenerator: no HIP device visible (the generator state lives in "
                               "device memory; PeriodicGaitGenerator is the host form)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.empty((E, _lib.PGG_BYTES), dtype=torch.uint8, device=self.device)
        self.load_state_dict(host)

    def _views(self):
        import torch

        f = _lib.SrbdPgg
        d, i = self.state.view(torch.float64), self.state.view(torch.int32)
        return (d[:, f.phase_signal.offset // 8:f.phase_signal.offset // 8 + 4],
                d[:, f.phase_offset.offset // 8:f.phase_offset.offset // 8 + 4],
                i[:, f.init.offset // 4:f.init.offset // 4 + 4])

    @property
    def phase_signal(self):
        """(E, 4) float64 view of the state's phase signals."""
        return self._views()[0]

    @property
    def phase_offset(self):
        """(E, 4) float64 view of the state's phase offsets."""
        return self._views()[1]

    @property
    def init(self):
        """(E, 4) int32 view of the state's start-up holds."""
        return self._views()[2]

    def _on(self, stream):
        import torch

        return torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream)

    def state_dict(self):
        """The host structs, a ``(SrbdPgg * E)`` ctypes array (waits for the device): for checkpoints and tests.
        ``bytes()`` of it is a plain byte string; ``load_state_dict`` takes either."""
        raw = self.state.cpu().numpy().tobytes()
        return (_lib.SrbdPgg * self.num_envs).from_buffer_copy(raw)

    def load_state_dict(self, structs, stream=None):
        import torch

        raw = np.frombuffer(bytes(structs), dtype=np.uint8)
        if raw.size != self.num_envs * _lib.PGG_BYTES:
            raise ValueError(f"{self.num_envs} srbd_pgg structs expected ({self.num_envs * _lib.PGG_BYTES} bytes), got "
                             f"{raw.size} bytes")
        with self._on(stream):
            self.state.copy_(torch.from_numpy(raw.reshape(self.num_envs, _lib.PGG_BYTES).copy()))

    def reset(self, stream=None, *, mask=None):
        """``PeriodicGaitGenerator.reset`` of every environment: the phases back to the gaits' offsets, the holds
        cleared.  ``mask`` (E,) bool, int32 or int64 cuda tensor: only the environments whose entry is not zero, one
        launch (``srbd_loop_reset_device`` at the reference's level), the others untouched; no host wait."""
        if mask is not None:
            from .loop_reset import reference_words

            # the words are 0 or 1, so the snapshot the call asks for is never read: the state stands in for it
            _lib.loop_reset_device(reference_words(mask, self.num_envs, stream), pgg=self.state,
                                   snapshots={"pgg": self.state}, stream=stream)
            return
        ph, off, ini = self._views()
        with self._on(stream):
            ph.copy_(off)
            ini.zero_()

    def set_phase_signal(self, phase_signal, init=None, stream=None):
        """``set_phase_signal`` of every environment: phase_signal (E, 4) float64 values (array or tensor); init None
        (the holds are cleared) or (E, 4), stored as ``init != 0``."""
        import torch

        ph, _, ini = self._views()
        src = torch.as_tensor(phase_signal, dtype=torch.float64)
        if tuple(src.shape) != (self.num_envs, 4):
            raise ValueError(f"phase_signal must be ({self.num_envs}, 4), got {tuple(src.shape)}")
        flags = None if init is None else torch.as_tensor(init)
        if flags is not None and tuple(flags.shape) != (self.num_envs, 4):
            raise ValueError(f"init must be ({self.num_envs}, 4), got {tuple(flags.shape)}")
        with self._on(stream):
            ph.copy_(src)
            if flags is None:
                ini.zero_()
            else:
                ini.copy_((flags != 0).to(torch.int32))

    def run(self, dt, step_freqs=None, stream=None):
        """``run(dt, step_freqs[e])`` of every environment -> the contact flags, (E, 4) float32.  step_freqs None:
        each environment's own step frequency; else an (E,) float64 tensor."""
        return _lib.pgg_run_device(self.state, dt, step_freqs, stream=stream)

    def compute_contact_sequence(self, contact_sequence_dts, contact_sequence_lenghts, out=None, stream=None):
        """Every environment's look-ahead sequence -> (E, 4, H) float32, or ``out`` (E, 4, >=H) with its first H
        columns written: what ``step_device`` takes as ``contacts``.  The dts and lengths are host sequences shared
        by the environments; IndexError where the reference's loop would run past them."""
        key = (np.asarray(contact_sequence_dts, dtype=np.float64).tobytes(),
               np.asarray(contact_sequence_lenghts, dtype=np.int32).tobytes())
        if key != self._seq_key:  # the control loop passes the same arrays every step
            self._dts = np.frombuffer(key[0], dtype=np.float64).copy()
            self._lens = np.frombuffer(key[1], dtype=np.int32).copy()
            self._seq_key = key
        return _lib.pgg_contact_sequence_device(self.state, self.horizon, self._dts, self._lens, out=out,
                                                stream=stream)

    def update_start_and_stop(self, feet_pos, hip_pos, hip_offset, base_pos, base_ori_euler_xyz, base_lin_vel,
                              base_ang_vel, ref_base_lin_vel, ref_base_ang_vel, current_contact, out=None,
                              stream=None):
        """``update_start_and_stop`` of every environment (``srbd_pgg_start_stop_device``), one launch and no host
        wait.  feet_pos / hip_pos (E, 4, 3), the five vectors and the command (E, 3) float64 tensors,
        current_contact (E, 4) float32; hip_offset a float shared by the environments, or a
        ``BatchedFootholdReferenceGenerator`` (or its state tensor), whose per-environment hip offsets are read.
        Returns the actions (E,) int32: 0 untouched, 1 stopped (full stance), 2 restored."""
        frg = getattr(hip_offset, "state", hip_offset)
        shared = None
        if not hasattr(frg, "data_ptr"):
            frg, shared = None, float(hip_offset)
        return _lib.pgg_start_stop_device(self.state, feet_pos, hip_pos, base_pos, base_ori_euler_xyz, base_lin_vel,
                                          base_ang_vel, ref_base_lin_vel, ref_base_ang_vel, current_contact, frg=frg,
                                          hip_offset=shared, out=out, stream=stream)
