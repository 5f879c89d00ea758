"""Gait-adaptive ``Sampling_MPC`` over ``num_envs`` environments stepped by one call (``srbd_batch_set_gait`` +
``srbd_batch_step``, include/srbd_mpc.h).

The batch form of ``centroidal_nmpc_hip_gait_adaptive.Sampling_MPC``: per environment the leg phases (``timing``),
the nominal step frequency and ``optimize_swing`` on top of what ``Batched_Sampling_MPC`` takes.  Each environment's
candidate set is the one the single class forms (``_freq_set``: GA:687-692 random sampling, :834-838 MPPI); every
sample draws its step frequency on the device from its environment's set and rolls out with its own contact sequence.
Environment ``e`` of a ``compute_control`` call returns what the single gait-adaptive class returns with the same
key, bit for bit, ``best_step_frequency`` included.

``compute_control_device(..., gait=, optimize_swings=)`` is the same step with every per-environment value on the device (``srbd_batch_set_gait_device``
+ ``srbd_batch_step_device``): the leg phases come from a ``BatchedPeriodicGaitGenerator``'s state or a tensor, the
``optimize_swing`` flags from ``BatchedSwingTrajectoryController.check_touch_down_condition``, and
``apply_step_frequency`` writes the best frequencies back into the device states (wb_interface.py:354-358), so a
gait-adaptive loop never leaves the device or waits for it.

MPPI and random sampling; ``sampling_method == 'cem_mppi'`` raises ``NotImplementedError`` from the base class.
Gait-adaptive sampling together with the opt-in cost terms has no batch form (the library refuses it).
"""
from __future__ import annotations

import numpy as np

from ... import _lib
from .centroidal_nmpc_hip_batched import Batched_Sampling_MPC as _BatchedBase
from .centroidal_nmpc_hip_gait_adaptive import PGG_DUTY_FACTOR
from .centroidal_nmpc_hip_gait_adaptive import Sampling_MPC as _SingleGaitAdaptive

f32 = np.float32


class Batched_Sampling_MPC(_BatchedBase):
    """``num_envs`` gait-adaptive sampling controllers of one configuration behind one device context."""

    def __init__(self, num_envs: int, config_module=None):
        super().__init__(num_envs, config_module)
        # the single gait-adaptive class carries step_freq_available and forms the candidate sets; like the base
        # class's helper it never creates a device context
        self._one_ga = _SingleGaitAdaptive(config_module)
        self.step_freq_delta = self._one_ga.step_freq_delta
        self.dt = self._one_ga.dt

    # the device step returns the best rows' step frequencies in the frequency slot
    _device_step_frequencies_from_result = True

    def freq_sets(self, nominal_step_frequencies, optimize_swings) -> np.ndarray:
        """(E, n_freq): environment e's ``_freq_set(nominal_step_frequencies[e], optimize_swings[e])``."""
        E = self.num_envs
        nominal = np.broadcast_to(np.asarray(nominal_step_frequencies), (E,))
        swing = np.broadcast_to(np.asarray(optimize_swings), (E,))
        return np.stack([np.asarray(self._one_ga._freq_set(nominal[e], swing[e]), dtype=f32).reshape(-1)
                         for e in range(E)])

    def compute_control(self, states, references, contact_sequences, best_control_parameters, keys, timings,
                        nominal_step_frequencies, optimize_swings, *, noise=None, step_frequencies=None):
        """The batched return tuple with the best row's step frequency per environment (E,) in place of the
        constant.  timings (E, 4); nominal_step_frequencies and optimize_swings (E,) or scalars;
        step_frequencies None or (E, N) injected per-sample frequencies (with ``noise=``, the parity mode)."""
        fs = self.freq_sets(nominal_step_frequencies, optimize_swings)
        self.context.set_gait(np.asarray(timings, dtype=f32), self.dt, PGG_DUTY_FACTOR, fs, step_frequencies)
        grf, fh, pred, best, cost, _, costs = super().compute_control(states, references, contact_sequences,
                                                                      best_control_parameters, keys, noise=noise)
        freq = np.array([r.best_freq for r in self.last_results], dtype=f32)
        return grf, fh, pred, best, cost, freq, costs

    def _set_gait_device(self, *, gait=None, timings=None, nominal_step_frequencies=None, optimize_swings=None,
                         step_frequencies=None, stream=None):
        """The gait keywords of the inherited ``compute_control_device(states, refs, contacts, best, keys, *, gait=None,
        timings=None, nominal_step_frequencies=None, optimize_swings, step_frequencies=None, noise=None,
        stream=None)``: ``set_gait_device`` enqueued on ``stream`` ahead of the device step, so nothing crosses to the
        host and nothing waits for the device.  The leg phases come from exactly one of ``gait`` (a
        ``BatchedPeriodicGaitGenerator`` or its state tensor) and ``timings`` (E, 4) float32;
        nominal_step_frequencies (E,) float32, or None for ``gait``'s own step frequencies; optimize_swings (E,) int32
        as ``check_touch_down_condition`` returns them (required); step_frequencies None or (E, N) float32 injected
        per-sample frequencies (with ``noise=``, the parity mode).  The step then returns the (E,) float32 device
        tensor of the best rows' step frequencies in the frequency slot."""
        if optimize_swings is None:
            raise ValueError("optimize_swings is required with the gait arguments")
        self.context.set_gait_device(optimize_swings, self.step_freq_delta, self.dt, PGG_DUTY_FACTOR,
                                     pgg=getattr(gait, "state", gait), timings=timings,
                                     nominal_freqs=nominal_step_frequencies, freq_rows=step_frequencies, stream=stream)

    @staticmethod
    def apply_step_frequency(optimize_swings, best_step_frequencies, gait=None, frg=None, stc=None, stream=None):
        """wb_interface.py:354-358 for every environment on the device (``_lib.apply_step_frequency``): where
        optimize_swings[e] == 1, ``gait``'s step frequency, ``frg``'s stance time and ``stc``'s swing period are
        re-timed from best_step_frequencies[e], the frequency slot of ``compute_control_device``."""
        _lib.apply_step_frequency(optimize_swings, best_step_frequencies, gait=gait, frg=frg, stc=stc, stream=stream)
