"""Velocity modulator: the velocity command set to zero while a foot is far from its hip.

Mirror of ``quadruped_pympc/helpers/velocity_modulator.py`` (reference): ``activated`` from
``simulation_params['velocity_modulator']``, ``max_distance`` (0.2 for every robot) and ``modulate_velocities``, run
by ``WBInterface.update_state_and_reference`` before the foothold reference generator, which reads the modulated
command (quadruped_pympc/interfaces/wb_interface.py:168-172).  The arithmetic runs in ``libsrbd_hip.so``'s C++ host
producers (``include/srbd_host.h``) and equals the reference bit for bit, its quirks included: the "standing" test has
no ``abs``, so a negative command counts as standing, and the zeroing is a product with 0.0, so a negative entry becomes
-0.0 and a NaN stays.  ``BatchedVelocityModulator`` does ``num_envs`` of them in one launch
(``srbd_vm_modulate_device``, ``include/srbd_mpc.h``).
"""
from __future__ import annotations

import numpy as np

from .. import _lib, config as cfg
from .foothold_reference_generator import _check, _legs, _vec


class VelocityModulator:
    def __init__(self):
        self.activated = cfg.simulation_params['velocity_modulator']
        self.max_distance = 0.2  # the reference's value for every robot

    def modulate_velocities(self, ref_base_lin_vel, ref_base_ang_vel, feet_pos, hip_pos):
        lin_out, ang_out = np.zeros(3), np.zeros(3)
        _check(_lib.lib.srbd_vm_modulate(
            float(self.max_distance), _lib.dptr(_vec(ref_base_lin_vel, 3, "ref_base_lin_vel")),
            _lib.dptr(_vec(ref_base_ang_vel, 3, "ref_base_ang_vel")), _lib.dptr(_legs(feet_pos)),
            _lib.dptr(_legs(hip_pos)), _lib.dptr(lin_out), _lib.dptr(ang_out)), "modulate_velocities")
        return lin_out, ang_out


class BatchedVelocityModulator:
    """The velocity modulator of ``num_envs`` environments on the device (``srbd_vm_modulate_device``,
    include/srbd_mpc.h), stateless.  ``step`` enqueues one launch on ``stream`` (None: torch's current stream) and does
    not wait for the device; with ``activated`` false it returns the command as given, as the reference skips the
    call."""

    def __init__(self, num_envs, max_distance=0.2, activated=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        self.num_envs = E
        self.max_distance = float(max_distance)
        self.activated = cfg.simulation_params['velocity_modulator'] if activated is None else bool(activated)

    def step(self, ref_lin_vel, ref_ang_vel, feet, hips, out=None, stream=None):
        """(lin_out, ang_out), (E, 3) float64 each (``out`` when given: a pair of tensors), from ref_lin_vel /
        ref_ang_vel (E, 3) and feet / hips (E, 4, 3) float64 tensors.  lin_out is what
        ``BatchedFootholdReferenceGenerator.step`` takes as ref_lin_vel and ``BatchedTerrainEstimator.step`` rotates."""
        if tuple(getattr(ref_lin_vel, "shape", ())) != (self.num_envs, 3):
            raise ValueError(f"ref_lin_vel must be ({self.num_envs}, 3), got {tuple(getattr(ref_lin_vel, 'shape', ()))}")
        if not self.activated:
            return ref_lin_vel, ref_ang_vel
        return _lib.vm_modulate_device(ref_lin_vel, ref_ang_vel, feet, hips, self.max_distance, out=out, stream=stream)
