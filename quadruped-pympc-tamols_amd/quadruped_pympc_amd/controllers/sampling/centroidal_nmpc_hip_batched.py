"""``Sampling_MPC`` over ``num_envs`` environments stepped by one call (``srbd_batch_step``, include/srbd_mpc.h).

The reference runs many simulations as replica processes (simulation/batched_simulations.py:40-58), one controller
each.  ``Batched_Sampling_MPC`` is the one-process form: one configuration (the same config mirror ``Sampling_MPC``
reads), and per environment a state, reference, contact sequence, warm start and noise key.  Environment ``e`` of a
``compute_control`` call returns what a ``Sampling_MPC`` with the same key returns, bit for bit.

MPPI and random sampling; ``sampling_method == 'cem_mppi'`` raises ``NotImplementedError`` here: sigma is part of
every CEM step, so it has a class of its own, ``Batched_CEM_Sampling_MPC`` (centroidal_nmpc_hip_cem_batched).
"""
from __future__ import annotations

import numpy as np

from ... import _lib
from ...runtime import active_config
from .centroidal_nmpc_hip import Sampling_MPC

f32 = np.float32


class LazyBatchCosts:
    """Saturated per-sample costs (E, N) of one batch step, fetched from the device on first use."""

    def __init__(self, ctx: "_lib.BatchContext", step_id: int, owner: "Batched_Sampling_MPC"):
        self._ctx, self._step_id, self._owner, self._data = ctx, step_id, owner, None
        self.shape = (ctx.E, ctx.N)

    def __array__(self, dtype=None, copy=None):
        if self._data is None:
            if self._owner._calls != self._step_id:
                raise RuntimeError("costs of an older step: materialise them before the next compute call")
            self._data = self._ctx.copy_costs()
        return self._data if dtype is None else self._data.astype(dtype)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, i):
        return np.asarray(self)[i]


class Batched_Sampling_MPC:
    """``num_envs`` sampling controllers of one configuration behind one device context."""

    # False: 'cem_mppi' is refused (sigma is part of every CEM step: Batched_CEM_Sampling_MPC sets it)
    _accepts_cem = False
    _context_class = _lib.BatchContext

    def __init__(self, num_envs: int, config_module=None):
        cfg = active_config(config_module)
        if cfg.mpc_params["sampling_method"] == "cem_mppi" and not self._accepts_cem:
            raise NotImplementedError("Batched_Sampling_MPC: 'cem_mppi' carries sigma through every step; use "
                                      "Batched_CEM_Sampling_MPC (centroidal_nmpc_hip_cem_batched)")
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        # one single-environment controller carries the configuration and the per-environment host helpers
        # (with_newkey, prepare_state_and_reference); it never creates a device context
        self._one = Sampling_MPC(config_module)
        one = self._one
        self.rng = one.rng
        self.sampling_method = one.sampling_method
        self.control_parametrization = one.control_parametrization
        self.num_sampling_iterations = one.num_sampling_iterations
        self.num_parallel_computations = one.num_parallel_computations
        self.horizon = one.horizon
        self.num_control_parameters = one.num_control_parameters
        self.num_control_parameters_single_leg = one.num_control_parameters_single_leg
        self.best_control_parameters = np.zeros((self.num_envs, self.num_control_parameters), dtype=f32)
        # environment e starts from seed 42 + e: (seed, counter) for Philox, jax.random.PRNGKey(42 + e) otherwise
        if self.rng == "philox":
            self.master_keys = np.array([[42 + e, 0] for e in range(self.num_envs)], dtype=np.uint64)
        else:
            self.master_keys = np.stack([_lib.jax_prng_key(42 + e) for e in range(self.num_envs)])
        self._calls = 0
        self._ctx = None
        self.jitted_compute_control = self.compute_control

    @property
    def context(self) -> "_lib.BatchContext":
        if self._ctx is None:
            self._ctx = self._context_class(self._one._srbd_config(), self.num_envs)
            if self.rng != "philox":
                self._ctx.set_rng(self.rng)
        return self._ctx

    def set_cost_terms(self, r_force=(0.0, 0.0, 0.0), w_smooth: float = 0.0, w_cone: float = 0.0):
        """srbd_batch_set_cost_terms for every environment (all 0: the reference's cost)."""
        self.context.set_cost_terms(r_force, w_smooth, w_cone)

    def set_robot_parameters(self, *, mass=None, inertia=None, mu=None, grf_min=None, grf_max=None, q_diag=None,
                             mask=None):
        """Per-environment robot and cost parameters for every following step (srbd_batch_set_env_params): each
        keyword a scalar or a length-E array, as ``_lib.make_env_params`` takes them; fields not given keep the
        configuration's value.  mask None or (E,) booleans: False keeps an environment's current parameters.
        Environment e then returns what a ``Sampling_MPC`` of that robot returns, bit for bit.  The gait-adaptive and
        CEM classes inherit it."""
        ctx = self.context
        ctx.set_env_params(_lib.make_env_params(self.num_envs, ctx.cfg, mass=mass, inertia=inertia, mu=mu,
                                                grf_min=grf_min, grf_max=grf_max, q_diag=q_diag), mask)

    def clear_robot_parameters(self):
        """Every environment back to the configuration's robot (srbd_batch_clear_env_params)."""
        self.context.clear_env_params()

    def with_newkey(self):
        """Every environment's key advanced as Sampling_MPC.with_newkey advances its stream's."""
        one = self._one
        keys = np.array(self.master_keys)
        for e in range(self.num_envs):
            one.master_key = keys[e]
            keys[e] = one.with_newkey().master_key
        self.master_keys = keys
        return self

    def get_key(self):
        return self.master_keys

    def compute_control(self, states, references, contact_sequences, best_control_parameters, keys, *, noise=None):
        """The single class's return tuple, stacked on a leading environment axis:
        (GRFs (E, 12), footholds (E, 12), predicted states (E, 24), best parameters (E, P), best costs (E,),
        step frequencies (E,), costs (E, N) lazy)."""
        ctx = self.context
        E = self.num_envs
        self._calls += 1
        if self.rng == "philox":
            k = np.asarray(keys, dtype=np.uint64).reshape(E, -1)
            seeds, counters = k[:, 0], (k[:, 1] if k.shape[1] > 1 else np.zeros(E, np.uint64))
        else:  # the packed JAX keys; the counter only numbers the steps
            k = np.asarray(keys, dtype=np.uint32).reshape(E, 2)
            seeds = np.array([_lib.pack_key(k[e]) for e in range(E)], dtype=np.uint64)
            counters = np.full(E, self._calls, dtype=np.uint64)
        best, results, _ = ctx.step(states, references, contact_sequences, best_control_parameters, noise=noise,
                                    seeds=seeds, counters=counters)
        self.last_results = results
        grf = np.array([r.grf[:] for r in results], dtype=f32)
        pred = np.array([r.predicted_state[:] for r in results], dtype=f32)
        cost = np.array([r.best_cost for r in results], dtype=f32)
        return (grf, np.zeros((E, 12), dtype=np.int32), pred, best, cost, np.full(E, 1.4),
                LazyBatchCosts(ctx, self._calls, self))

    # the step frequencies compute_control_device returns: the constant of compute_control, or (the gait-adaptive
    # class) the best rows' frequencies
    _device_step_frequencies_from_result = False

    def _set_gait_device(self, **gait_arguments):
        """The gait keywords of ``compute_control_device``: the gait-adaptive class enqueues them."""
        raise ValueError("gait, timings, nominal_step_frequencies, optimize_swings and step_frequencies belong to the "
                         "gait-adaptive Batched_Sampling_MPC (centroidal_nmpc_hip_gait_adaptive_batched)")

    def compute_control_device(self, states, references, contact_sequences, best_control_parameters, keys, *,
                               noise=None, stream=None, gait=None, timings=None, nominal_step_frequencies=None,
                               optimize_swings=None, step_frequencies=None, due=None):
        """``compute_control`` on torch tensors of the context's device (``srbd_batch_step_device``): nothing crosses
        to the host and nothing waits for the device; the step is enqueued on ``stream`` (None: torch's current
        stream) and the returned tensors are ready in that stream's order.

        states, references (E, 24), contact_sequences (E, 4, >=H), best_control_parameters (E, P): contiguous float32
        tensors; best_control_parameters is updated in place and returned.  keys, int64 or uint64: for
        ``rng == 'philox'`` the (E, 2) (seed, counter) tensor; for the JAX streams the (E,) packed keys
        (``_lib.pack_key``), the step number being the counter as in ``compute_control``.  This call runs one
        sampling iteration with the keys as given; ``Batched_SRBDControllerInterface``
        (interfaces/srbd_controller_interface_batched) advances the keys of every stream on the device and runs the
        ``num_sampling_iterations`` iterations of a control step.

        Returns the single class's tuple: (GRFs (E, 12), footholds (E, 12), predicted states (E, 24), best parameters
        (E, P), best costs (E,), step frequencies (E,), costs (E, N) lazy -- fetched to the host on first use).

        The gait keywords (the gait-adaptive class only; see its ``_set_gait_device``): when any is given, the
        step's arguments are checked first and the gait setting is enqueued on ``stream`` ahead of the step
        (``srbd_batch_set_gait_device``); without them the step runs with the last gait setting made.

        due None: every environment is stepped.  due an (E,) int32 or bool tensor of the context's device
        (``mpc_due``, interfaces/srbd_controller_interface_batched): only the environments it names are stepped
        (``srbd_batch_step_masked_device``).  An environment that is not due is neither written nor read -- its row of
        best_control_parameters keeps its bytes -- and the controller keeps one output dict for these calls, so the
        returned tensors hold the last solve of the environments that are not due (zeros before the first) and are
        overwritten in place by the next ``due=`` call; so do the ``costs`` rows.  The keys are the caller's: advance
        only the due environments' keys.  The gait setter itself takes no mask (it is a setting, not a solve): with
        the gait keywords every environment's gait fields are rewritten from its inputs, and an environment reads
        them at its next due step; ``Batched_SRBDControllerInterface`` masks the gait setting with the rest."""
        import torch

        ctx = self.context
        E = self.num_envs
        gait_arguments = dict(gait=gait, timings=timings, nominal_step_frequencies=nominal_step_frequencies,
                              optimize_swings=optimize_swings, step_frequencies=step_frequencies)
        with_gait = any(v is not None for v in gait_arguments.values())
        if not isinstance(keys, torch.Tensor):
            raise ValueError("keys must be a torch tensor")
        dev = keys.device
        if self.rng == "philox":
            if keys.dim() != 2 or tuple(keys.shape) != (E, 2):
                raise ValueError(f"keys must be ({E}, 2) (seed, counter), got {tuple(keys.shape)}")
            s = torch.cuda.current_stream(dev) if stream is None else stream
            with torch.cuda.stream(s):
                seeds, counters = keys[:, 0].contiguous(), keys[:, 1].contiguous()
        else:
            if tuple(keys.shape) != (E,):
                raise ValueError(f"keys must be ({E},) packed JAX keys, got {tuple(keys.shape)}")
            s = torch.cuda.current_stream(dev) if stream is None else stream
            seeds = keys
            with torch.cuda.stream(s):
                counters = torch.full((E,), self._calls + 1, dtype=torch.int64, device=dev)
        if with_gait:  # every refusal before anything is enqueued
            ctx.check_step_device(states, references, contact_sequences, best_control_parameters, seeds, counters, noise)
            self._set_gait_device(stream=stream, **gait_arguments)
        if due is None:
            out = ctx.step_device(states, references, contact_sequences, best_control_parameters, seeds, counters,
                                  noise=noise, stream=stream)
        else:
            out = self._held_result = ctx.step_masked_device(states, references, contact_sequences,
                                                             best_control_parameters, seeds, counters, due,
                                                             noise=noise, out=getattr(self, "_held_result", None),
                                                             stream=stream)
        self._calls += 1
        with torch.cuda.stream(s):
            footholds = torch.zeros((E, 12), dtype=torch.int32, device=dev)
            freq = (out["best_freq"] if self._device_step_frequencies_from_result
                    else torch.full((E,), 1.4, dtype=torch.float64, device=dev))
        self.last_device_result = out
        self._device_best = best_control_parameters  # compute_plan_device's default row
        return (out["grf"], footholds, out["predicted_state"], best_control_parameters, out["best_cost"], freq,
                LazyBatchCosts(ctx, self._calls, self))

    def compute_plan_device(self, state, ref, contacts, best=None, freqs=None, *, want=_lib.PLAN_OUTPUTS,
                            stream=None):
        """The full-horizon plan of one parameter row per environment (``BatchContext.plan_device``): state, ref
        (E, 24) the prepared rows a step takes, contacts (E, 4, >=H), best (E, P) -- None: the controller's current
        best parameters, the tensor the last ``compute_control_device`` updated, else the host attribute uploaded --
        and freqs (E,) with gait-adaptive sampling (None: the last device step's ``best_freq``).  Returns the dict of
        ``plan_device``: plan_states, plan_grfs (E, H, 12), plan_contacts (E, 4, H), plan_run_cost (E, H), plan_cost
        (E,), ready in the stream's order."""
        import torch

        if best is None:
            best = getattr(self, "_device_best", None)
            if best is None:
                best = torch.from_numpy(np.ascontiguousarray(self.best_control_parameters, dtype=f32)).to(state.device)
        last = getattr(self, "last_device_result", None)
        if freqs is None and self._device_step_frequencies_from_result and last is not None:
            freqs = last["best_freq"]
        return self.context.plan_device(state, ref, contacts, best, freqs, want=want, stream=stream)

    def prepare_state_and_reference(self, states_current, reference_states, current_contacts, previous_contacts,
                                    mpc_frequency=100):
        """Sampling_MPC.prepare_state_and_reference (srbd_prepare_state) per environment: sequences of E state /
        reference dicts and contact vectors -> (states (E, 24), references (E, 24)); the warm starts' lift-off
        legs are zeroed in ``best_control_parameters``."""
        one = self._one
        states = np.zeros((self.num_envs, 24))
        refs = np.zeros((self.num_envs, 24))
        best = np.array(self.best_control_parameters, dtype=f32)
        for e in range(self.num_envs):
            one.best_control_parameters = best[e]
            states[e], refs[e] = one.prepare_state_and_reference(states_current[e], reference_states[e],
                                                                 current_contacts[e], previous_contacts[e],
                                                                 mpc_frequency)
            best[e] = one.best_control_parameters
        self.best_control_parameters = best
        return states, refs

    def prepare_state_and_reference_device(self, state_in, ref_in, current_contacts, previous_contacts, stream=None,
                                           *, best_control_parameters=None):
        """``prepare_state_and_reference`` on torch tensors of one cuda device (``srbd_prepare_state_device``),
        enqueued on ``stream`` (None: torch's current stream) without a host synchronisation.

        state_in (E, 24) float64: per environment [position, linear_velocity, orientation, angular_velocity,
        foot_FL, foot_FR, foot_RL, foot_RR]; ref_in (E, 24) float64: [ref_position, ref_linear_velocity,
        ref_orientation, ref_angular_velocity, ref_foot_FL..RR] (a float32 simulator state is widened exactly by
        ``.double()``).  current_contacts, previous_contacts (E, 4) float32: ``contact_sequences[:, :, 0]`` made
        contiguous, and the one of the previous step.  Returns (states, refs), (E, 24) float32: the host method's
        float64 outputs rounded as the step stages them, ready for ``compute_control_device``.

        The warm start: the device loop's warm start is the tensor the caller hands to ``compute_control_device``,
        which updates it in place, so the caller passes that same (E, P) float32 tensor here as
        ``best_control_parameters`` and the lift-off legs are zeroed in it in place.  The controller keeps no device
        copy of its own, and the host attribute ``self.best_control_parameters`` is not touched.  None: no zeroing.

        ``shift_solution`` configurations are refused: the device form restates the unshifted path only."""
        if self._one._cfg.mpc_params["shift_solution"]:
            raise NotImplementedError("prepare_state_and_reference_device: shift_solution has no device form")
        return _lib.prepare_state_device(state_in, ref_in, current_contacts, previous_contacts,
                                         self.num_control_parameters_single_leg, best_control_parameters,
                                         stream=stream)

    def reset(self):
        print("Resetting the controller")

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
