"""Terrain estimator: the filtered terrain roll, pitch and height the reference row is built from.

Mirror of ``quadruped_pympc/helpers/terrain_estimator.py`` (reference): the same attributes and the same
``compute_terrain_estimation`` signature with its dict of feet.  The state lives in a ``srbd_terrain_est`` struct and
the step runs in ``libsrbd_hip.so``'s C++ host producers (``include/srbd_host.h``).  ``assemble_reference`` is the part
of ``WBInterface.update_state_and_reference`` that follows it (quadruped_pympc/interfaces/wb_interface.py:258-291).
``BatchedTerrainEstimator`` keeps ``num_envs`` of these structs on the device and does both in one launch
(``srbd_terrain_ref_step_device``, ``include/srbd_mpc.h``).

The height filter equals the reference bit for bit; roll, pitch and the rotated command agree with it to rounding (the
header states why: the arctangent, cos and sin are the library's own, the rotations are written out).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, config as cfg
from .foothold_reference_generator import _check, _vec
from .legs_attr import LEG_NAMES


def _feet(feet_pos):
    """A (4, 3) float64 array from a dict or LegsAttr of feet (or a (4, 3) array)."""
    if isinstance(feet_pos, np.ndarray):
        out = np.ascontiguousarray(feet_pos, dtype=np.float64)
    else:
        out = np.array([np.asarray(feet_pos[k], dtype=np.float64) for k in LEG_NAMES])
    if out.shape != (4, 3):
        raise ValueError(f"four feet of three coordinates expected, got shape {out.shape}")
    return out


class TerrainEstimator:
    def __init__(self) -> None:
        self._g = _lib.SrbdTerrainEst()
        self._gp = C.byref(self._g)
        _check(_lib.lib.srbd_terrain_est_init(self._gp), "srbd_terrain_est_init")

    # plain attributes of the reference, backed by the C struct
    terrain_roll = property(lambda s: s._g.roll, lambda s, v: setattr(s._g, "roll", float(v)))
    terrain_pitch = property(lambda s: s._g.pitch, lambda s, v: setattr(s._g, "pitch", float(v)))
    terrain_height = property(lambda s: s._g.height, lambda s, v: setattr(s._g, "height", float(v)))
    roll_activated = property(lambda s: bool(s._g.roll_activated),
                              lambda s, v: setattr(s._g, "roll_activated", int(bool(v))))
    pitch_activated = property(lambda s: bool(s._g.pitch_activated),
                               lambda s, v: setattr(s._g, "pitch_activated", int(bool(v))))

    def compute_terrain_estimation(self, base_position, yaw, feet_pos, current_contact=None):
        """(terrain_roll, terrain_pitch, terrain_height) after one step.  ``current_contact`` is accepted and unused,
        as in the reference."""
        out = np.zeros(3)
        _check(_lib.lib.srbd_terrain_estimate(self._gp, _lib.dptr(_vec(base_position, 3, "base_position")), float(yaw),
                                              _lib.dptr(_feet(feet_pos)), _lib.dptr(out)),
               "compute_terrain_estimation")
        return float(out[0]), float(out[1]), float(out[2])

    def assemble_reference(self, ref_base_lin_vel, ref_base_ang_vel, base_position, com_position, com_pos_offset_w=None,
                           ref_z=None):
        """The reference's ``ref_position``, ``ref_linear_velocity``, ``ref_orientation`` and
        ``ref_angular_velocity`` from the state as it is (wb_interface.py:258-291): a dict of four (3,) arrays.
        ref_z: None for the configuration's ``ref_z``."""
        z = cfg.simulation_params["ref_z"] if ref_z is None else ref_z
        off = 0.0 if com_pos_offset_w is None else float(com_pos_offset_w[2])
        row = np.zeros(12)
        _check(_lib.lib.srbd_reference_assemble(
            self._gp, float(z), float(base_position[2]), float(com_position[2]), off,
            _lib.dptr(_vec(ref_base_lin_vel, 3, "ref_base_lin_vel")),
            _lib.dptr(_vec(ref_base_ang_vel, 3, "ref_base_ang_vel")), _lib.dptr(row)), "assemble_reference")
        return dict(ref_position=row[0:3].copy(), ref_linear_velocity=row[3:6].copy(),
                    ref_orientation=row[6:9].copy(), ref_angular_velocity=row[9:12].copy())


class BatchedTerrainEstimator:
    """``num_envs`` terrain estimators whose state lives on the device (``srbd_terrain_ref_step_device``,
    include/srbd_mpc.h): the producer of entries 0..11 of ``prepare_state_and_reference_device``'s ``ref`` rows, with
    no host round trip.

    Environment ``e`` behaves as a ``TerrainEstimator`` that received ``compute_terrain_estimation`` and then
    ``assemble_reference`` each step: its state keeps the host struct's bytes and its row is the host's.  ``ref_z`` is
    shared; ``roll_activated`` / ``pitch_activated`` are bools or length-E sequences.  The state is one
    (E, sizeof(srbd_terrain_est)) uint8 tensor, ``state``.  ``step`` enqueues on ``stream`` (None: torch's current
    stream) and does not wait for the device; ``state_dict`` does."""

    def __init__(self, num_envs, ref_z=None, roll_activated=False, pitch_activated=True, device=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        self.ref_z = float(cfg.simulation_params["ref_z"] if ref_z is None else ref_z)
        if not np.isfinite(self.ref_z):
            raise ValueError(f"ref_z must be finite, got {self.ref_z}")

        def per_env(name, v):
            a = np.asarray(v, dtype=bool)
            if a.ndim == 0:
                return np.full(E, a)
            if a.shape != (E,):
                raise ValueError(f"{name} must be a bool or have {E} entries, got shape {a.shape}")
            return a

        roll_on, pitch_on = per_env("roll_activated", roll_activated), per_env("pitch_activated", pitch_activated)
        self.num_envs = E
        host = (_lib.SrbdTerrainEst * E)()
        for e in range(E):
            _check(_lib.lib.srbd_terrain_est_init(C.byref(host[e])), "srbd_terrain_est_init")
            host[e].roll_activated, host[e].pitch_activated = int(roll_on[e]), int(pitch_on[e])
        # everything above is host work; the upload is the first use of the device
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("BatchedTerrainEstimator: no HIP device visible (the estimator state lives in device "
                               "memory; TerrainEstimator is the host form)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.empty((E, _lib.TERRAIN_EST_BYTES), dtype=torch.uint8, device=self.device)
        self.load_state_dict(host)

    def _doubles(self, field):
        import torch

        return self.state.view(torch.float64)[:, getattr(_lib.SrbdTerrainEst, field).offset // 8]

    terrain_roll = property(lambda s: s._doubles("roll"), doc="(E,) float64 view of the filtered rolls.")
    terrain_pitch = property(lambda s: s._doubles("pitch"), doc="(E,) float64 view of the filtered pitches.")
    terrain_height = property(lambda s: s._doubles("height"), doc="(E,) float64 view of the filtered heights.")

    def _on(self, stream):
        import torch

        return torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream)

    def state_dict(self):
        """The host structs, a ``(SrbdTerrainEst * E)`` ctypes array (waits for the device): for checkpoints and
        tests.  ``bytes()`` of it is a plain byte string; ``load_state_dict`` takes either."""
        raw = self.state.cpu().numpy().tobytes()
        return (_lib.SrbdTerrainEst * self.num_envs).from_buffer_copy(raw)

    def load_state_dict(self, structs, stream=None):
        import torch

        raw = np.frombuffer(bytes(structs), dtype=np.uint8)
        if raw.size != self.num_envs * _lib.TERRAIN_EST_BYTES:
            raise ValueError(f"{self.num_envs} srbd_terrain_est structs expected "
                             f"({self.num_envs * _lib.TERRAIN_EST_BYTES} bytes), got {raw.size} bytes")
        with self._on(stream):
            self.state.copy_(torch.from_numpy(raw.reshape(self.num_envs, _lib.TERRAIN_EST_BYTES).copy()))

    def step(self, base_pos, com_pos, yaws, ref_lin_vel, ref_ang_vel, ref, *, frg=None, lift_off=None,
             com_pos_offset_w=None, out=None, stream=None):
        """One control step of every environment: the terrain estimate from the lift-off positions, then entries
        0..11 of each row of ``ref`` (E, 24) float64, written in place (12..23, the feet, are left alone).  base_pos /
        com_pos / ref_lin_vel / ref_ang_vel (E, 3), yaws (E,) float64 tensors; the two velocities are the modulated
        command (``BatchedVelocityModulator.step``).  Exactly one of frg, a ``BatchedFootholdReferenceGenerator`` (or
        its state tensor) whose lift-off table is read, and lift_off (E, 4, 3).  com_pos_offset_w (E, 3); out (E, 3)
        receives roll, pitch and height.  Returns ``ref``."""
        _lib.terrain_ref_step_device(self.state, base_pos, com_pos, yaws, ref_lin_vel, ref_ang_vel, ref, self.ref_z,
                                     lift_off=lift_off, frg=getattr(frg, "state", frg),
                                     com_pos_offset_w=com_pos_offset_w, out=out, stream=stream)
        return ref
