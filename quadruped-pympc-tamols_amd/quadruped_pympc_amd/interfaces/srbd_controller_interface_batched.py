"""``SRBDControllerInterface`` over ``num_envs`` environments, device-resident (``srbd_batch_interface_step_device``,
include/srbd_mpc.h).

The sampling branch of the reference's ``SRBDControllerInterface.compute_control``
(quadruped_pympc/interfaces/srbd_controller_interface.py:113-180, :225-229) for every environment of a batched
controller in one library call on the caller's stream: prepare_state_and_reference (:118-126), then per sampling
iteration with_newkey (:128), CEM's with_newsigma(sigma_cem_mppi) at iteration 0 (:129-130) and the device step
(:131-168), then the footholds from the reference (:170-175), the GRFs times ``contact_sequence[:, 0]`` (:225-229) and
``previous_contact_mpc = current_contact``.  Nothing crosses to the host and nothing waits for the device; the keys --
on the Philox and on both ``jax.random`` streams -- advance on the device.

``Batched_SRBDControllerInterface(controller)`` works over ``Batched_Sampling_MPC``, its gait-adaptive subclass and
``Batched_CEM_Sampling_MPC``.  It owns the state the single interface and its controller carry between calls, as
tensors of the controller's device: ``previous_contact_mpc`` (E, 4), ``keys`` (E, 2), ``best_control_parameters``
(E, P) and, for CEM, ``sigma_cem_mppi`` (E, P).  Environment ``e`` of a call returns what a single
``SRBDControllerInterface`` with the same key returns, bit for bit.

The tensors are made when the interface is created, from the controller's ``master_keys``, ``_calls`` and
``best_control_parameters`` as they are then; from there on the interface's tensors are the state.  The controller's
own host attributes ``master_keys`` and ``best_control_parameters`` are not written back (that would bring the device
state to the host every step); only its call count ``_calls`` advances.  So do not mix the two on one controller:
after the first ``compute_control_device`` here, the controller's own ``compute_control`` / ``compute_control_device``
/ ``with_newkey`` would continue from the stale host key.  Set ``iface.keys`` or ``iface.best_control_parameters`` (in
place) to re-seed or re-start environments.

The reference does not solve on every simulation step (quadruped_pympc_wrapper.py:134): ``due = mpc_due(step_num,
simulation_dt, mpc_frequency)`` and ``compute_control_device(..., due=due)`` step only the environments whose own step
counter says so (``srbd_batch_interface_step_masked_device``); the others are neither written nor read, and the
returned tensors hold their last solve.

``shift_solution`` configurations raise ``NotImplementedError``, as ``prepare_state_and_reference_device`` does.  Graph
capture, gait-adaptive CEM and more than ``_lib.MAX_IFACE_ITERS`` sampling iterations are not provided; only the last
iteration's outputs are returned, as the reference keeps only the last.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..controllers.sampling.centroidal_nmpc_hip_batched import LazyBatchCosts


def mpc_due(step_num, simulation_dt: float, mpc_frequency: float):
    """The reference's MPC gate for every environment (QuadrupedPyMPC_Wrapper.compute_actions,
    quadruped_pympc_wrapper.py:134): ``step_num % round(1 / (mpc_frequency * simulation_dt)) == 0`` as an int32 tensor
    of ``step_num``'s device and shape, torch ops on the current stream and no host read.  step_num: the simulator's
    (E,) integer tensor of per-environment step counters, which restart with the episode.  The period is the
    reference's expression, Python's ``round`` included (2.5 -> 2).  The result is the ``due`` of
    ``compute_control_device`` and of ``BatchContext.interface_step_masked_device``."""
    import torch

    period = round(1 / (mpc_frequency * simulation_dt))
    return (step_num % period == 0).to(torch.int32)


class Batched_SRBDControllerInterface:
    """``num_envs`` controller interfaces of one configuration over one batched sampling controller."""

    def __init__(self, controller):
        mp = controller._one._cfg.mpc_params
        if mp["shift_solution"]:
            raise NotImplementedError("Batched_SRBDControllerInterface: shift_solution has no device form")
        self.controller = controller
        self.num_envs = controller.num_envs
        self.horizon = controller.horizon
        self.num_sampling_iterations = int(controller.num_sampling_iterations)
        if not 1 <= self.num_sampling_iterations <= _lib.MAX_IFACE_ITERS:
            raise NotImplementedError(f"num_sampling_iterations must be in 1..{_lib.MAX_IFACE_ITERS}, got "
                                      f"{self.num_sampling_iterations}")
        self._cem = controller.sampling_method == "cem_mppi"
        self._gait_adaptive = hasattr(controller, "step_freq_delta")
        self.sigma_reset_value = float(mp["sigma_cem_mppi"]) if self._cem else 0.0
        # the state, on the controller's device from the start (the controller's context is created here if it has
        # not stepped yet): previous_contact_mpc ones, keys and warm starts the controller's as they are now
        import torch

        dev = torch.device("cuda", controller.context.cfg.device_id)
        E, P = self.num_envs, controller.num_control_parameters
        self.previous_contact_mpc = torch.ones((E, 4), dtype=torch.float32, device=dev)
        self.keys = torch.from_numpy(self._initial_keys().view(np.int64)).to(dev)
        self.best_control_parameters = torch.from_numpy(
            np.array(controller.best_control_parameters, dtype=np.float32).reshape(E, P)).to(dev)
        self.sigma_cem_mppi = (torch.full((E, P), self.sigma_reset_value, dtype=torch.float32, device=dev)
                               if self._cem else None)
        self.last_device_result = None
        self._held_result = None  # the output dict the masked calls (due=) write their due rows into

    def _initial_keys(self) -> np.ndarray:
        """(E, 2) uint64: (seed, counter) on Philox; (packed JAX key, call count) on the JAX streams."""
        c = self.controller
        mk = np.asarray(c.master_keys)
        if c.rng == "philox":
            return np.array(mk, dtype=np.uint64).reshape(self.num_envs, 2)
        packed = [_lib.pack_key(mk[e]) for e in range(self.num_envs)]
        return np.array([[k, c._calls] for k in packed], dtype=np.uint64)

    def compute_control_device(self, state_in, ref_in, contact_sequences, *, gait=None, optimize_swings=None,
                               timings=None, nominal_step_frequencies=None, step_frequencies=None, due=None,
                               stream=None):
        """One control step of every environment on torch tensors of the controller's device, enqueued on ``stream``
        (None: torch's current stream) without a host synchronisation.

        state_in (E, 24) float64: per environment [position, linear_velocity, orientation, angular_velocity,
        foot_FL..RR]; ref_in (E, 24) float64: [ref_position .. ref_angular_velocity, ref_foot_FL..RR];
        contact_sequences (E, 4, >=H) float32, column 0 the current contact.  The gait keywords are those of the
        gait-adaptive ``compute_control_device`` (``gait`` or ``timings``, ``optimize_swings`` required with them):
        the gait setting is enqueued once, ahead of the sampling iterations.

        ``num_sampling_iterations`` and ``sigma_cem_mppi`` are read from the configuration.  The interface's
        ``previous_contact_mpc``, ``keys``, ``best_control_parameters`` and ``sigma_cem_mppi`` are updated in place.

        due None: every environment is stepped.  due an (E,) int32 or bool tensor of the controller's device
        (``mpc_due``): only the environments it names are stepped (``srbd_batch_interface_step_masked_device``).  An
        environment that is not due is neither written nor read -- its key does not advance, its warm start, sigma and
        ``previous_contact_mpc`` row stay those of its last solve -- and the interface keeps one output dict for these
        calls, so the returned tensors hold the last solve of the environments that are not due (zeros before an
        environment's first solve) and are overwritten in place by the next ``due=`` call.  The ``costs`` rows of
        environments that are not due are those of their last solve too.  The controller's ``_calls`` advances by
        ``num_sampling_iterations`` per call whatever the mask holds -- it numbers the calls for the lazy costs; the
        per-environment truth is ``keys``.

        Returns (GRFs (E, 12) float64, masked with the current contact; footholds (E, 12) float64; predicted states
        (E, 24) float32; best sample frequencies (E,); best costs (E,) float32; costs (E, N) lazy -- fetched to the
        host on first use)."""
        import torch

        c = self.controller
        ctx = c.context
        E = self.num_envs
        gait_given = any(v is not None for v in (gait, optimize_swings, timings, nominal_step_frequencies,
                                                 step_frequencies))
        gait_io = None
        if gait_given:
            if not self._gait_adaptive:
                raise ValueError("the gait keywords belong to the gait-adaptive Batched_Sampling_MPC")
            if optimize_swings is None:
                raise ValueError("optimize_swings is required with the gait arguments")
            from ..controllers.sampling.centroidal_nmpc_hip_gait_adaptive import PGG_DUTY_FACTOR

            gait_io = ctx.make_gait_io(optimize_swings, c.step_freq_delta, c.dt, PGG_DUTY_FACTOR,
                                       pgg=getattr(gait, "state", gait), timings=timings,
                                       nominal_freqs=nominal_step_frequencies, freq_rows=step_frequencies)
        kw = dict(iterations=self.num_sampling_iterations, sigma=self.sigma_cem_mppi,
                  sigma_reset=self.sigma_reset_value, gait_io=gait_io, stream=stream)
        if due is None:
            out = ctx.interface_step_device(state_in, ref_in, contact_sequences, self.keys, self.previous_contact_mpc,
                                            self.best_control_parameters, **kw)
        else:
            out = self._held_result = ctx.interface_step_masked_device(
                state_in, ref_in, contact_sequences, self.keys, self.previous_contact_mpc,
                self.best_control_parameters, due, out=self._held_result, **kw)
        c._calls += self.num_sampling_iterations
        dev = self.keys.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        with torch.cuda.stream(s):
            if self._gait_adaptive:
                freq = out["best_freq"]
            else:
                freq = torch.full((E,), 1.65 if self._cem else 1.4, dtype=torch.float64, device=dev)
        self.last_device_result = out
        self._plan_contacts = contact_sequences  # a reference, not a copy: compute_plan_device reads it
        return (out["grf"], out["footholds"], out["predicted_state"], freq, out["best_cost"],
                LazyBatchCosts(ctx, c._calls, c))

    def compute_plan_device(self, *, want=_lib.PLAN_OUTPUTS, stream=None):
        """The full-horizon plan of the last ``compute_control_device`` call (``BatchContext.plan_device``): the
        updated best parameters rolled out from that call's prepared state and reference rows, with its contact rows
        and, gait-adaptive, its ``best_freq``.  The interface holds references to those tensors and copies nothing,
        so call it before they are overwritten.  After a ``due=`` call the rows of an environment that was not due are
        those of its last solve, and its plan is that solve's -- provided the caller's contact tensor still holds the
        contact rows that solve saw.  Enqueued on ``stream`` (None: torch's current stream).  Returns the
        dict of ``plan_device``.  RuntimeError before the first step."""
        out = self.last_device_result
        if out is None:
            raise RuntimeError("compute_plan_device: no compute_control_device call yet")
        return self.controller.context.plan_device(out["states"], out["refs"], self._plan_contacts,
                                                   self.best_control_parameters,
                                                   out["best_freq"] if self._gait_adaptive else None, want=want,
                                                   stream=stream)

    def reset(self, mask=None):
        """``previous_contact_mpc`` back to ones (WBInterface.reset's ``current_contact = [1, 1, 1, 1]``) for every
        environment, or for those a device mask (E,) names (non-zero: reset), with one torch op on the current
        stream; the keys and the warm starts are left alone."""
        import torch

        p = self.previous_contact_mpc
        if mask is None:
            p.fill_(1.0)
        else:
            p.copy_(torch.where(mask.reshape(-1, 1) != 0, torch.ones_like(p), p))
