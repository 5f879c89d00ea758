"""CEM-MPPI ``Sampling_MPC`` over ``num_envs`` environments stepped by one call (``srbd_batch_step_cem``,
include/srbd_mpc.h).

``Batched_CEM_Sampling_MPC`` is ``Batched_Sampling_MPC`` for ``sampling_method == 'cem_mppi'``: besides a state,
reference, contact sequence, warm start and noise key, every environment carries its own sigma (P,), which each step
reads and replaces with the clipped standard deviation of its elite rows (centroidal_nmpc_jax.py:1075-1081).
Environment ``e`` of a ``compute_control`` call returns what a CEM ``Sampling_MPC`` returns for the same key and
sigma, bit for bit, the new sigma included.

The reference's iteration loop (srbd_controller_interface.py:113-180) on the device, for a controller ``c`` and
tensors of its device -- ``num_sampling_iterations`` calls per control step, sigma reset to the configured constant by
the first one, keys advanced between calls::

    sigma = torch.empty((E, P), dtype=torch.float32, device=dev)
    for it in range(c.num_sampling_iterations):
        c.with_newkey()
        keys = torch.as_tensor(c.get_key().astype(np.int64), device=dev)       # 'philox': (E, 2) (seed, counter)
        out = c.compute_control_device(states, refs, contacts, best, keys, sigma,
                                       sigma_reset=c.sigma_reset_value if it == 0 else None)
    grf = out[0]   # best and sigma were updated in place

``Batched_SRBDControllerInterface`` (interfaces/srbd_controller_interface_batched) is that loop as one device-resident
call, the keys of every stream advanced on the device.  Gait-adaptive CEM and graph capture are not provided.
"""
from __future__ import annotations

import numpy as np

from ... import _lib
from .centroidal_nmpc_hip_batched import Batched_Sampling_MPC, LazyBatchCosts

f32 = np.float32


class Batched_CEM_Sampling_MPC(Batched_Sampling_MPC):
    """``num_envs`` CEM-MPPI sampling controllers of one configuration behind one device context."""

    _accepts_cem = True
    _context_class = _lib.CemBatchContext

    def __init__(self, num_envs: int, config_module=None):
        super().__init__(num_envs, config_module)
        if self.sampling_method != "cem_mppi":
            raise ValueError(f"Batched_CEM_Sampling_MPC needs sampling_method 'cem_mppi', got "
                             f"{self.sampling_method!r}: use Batched_Sampling_MPC")
        # the configured constant every control step starts from (the single class's initial sigma_cem_mppi)
        self.sigma_reset_value = float(self._one._cfg.mpc_params["sigma_cem_mppi"])
        self.sigma_cem_mppi = np.full((self.num_envs, self.num_control_parameters), self.sigma_reset_value, dtype=f32)

    def with_newsigma(self, sigma):
        """A scalar, (P,) or (E, P) value for every environment's sigma (Sampling_MPC.with_newsigma)."""
        self.sigma_cem_mppi = np.array(np.broadcast_to(np.asarray(sigma, dtype=f32),
                                                       (self.num_envs, self.num_control_parameters)), dtype=f32)
        return self

    def get_sigma(self):
        return self.sigma_cem_mppi

    def compute_control(self, states, references, contact_sequences, best_control_parameters, keys, sigmas, *,
                        noise=None):
        """The single class's CEM return tuple, stacked on a leading environment axis:
        (GRFs (E, 12), footholds (E, 12), predicted states (E, 24), best parameters (E, P), best costs (E,),
        step frequencies (E,), costs (E, N) lazy, new sigmas (E, P)).  sigmas: scalar, (P,) or (E, P)."""
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
        best, sigma, results, _ = ctx.step_cem(states, references, contact_sequences, best_control_parameters, sigmas,
                                               noise=noise, seeds=seeds, counters=counters)
        self.last_results = results
        grf = np.array([r.grf[:] for r in results], dtype=f32)
        pred = np.array([r.predicted_state[:] for r in results], dtype=f32)
        cost = np.array([r.best_cost for r in results], dtype=f32)
        return (grf, np.zeros((E, 12), dtype=np.int32), pred, best, cost, np.full(E, 1.65),
                LazyBatchCosts(ctx, self._calls, self), sigma)

    def compute_control_device(self, states, references, contact_sequences, best_control_parameters, keys, sigma, *,
                               sigma_reset=None, noise=None, stream=None, due=None):
        """``compute_control`` on torch tensors of the context's device (``srbd_batch_step_cem_device``), enqueued on
        ``stream`` (None: torch's current stream) without a host synchronisation.  The tensors and ``keys`` are those
        of ``Batched_Sampling_MPC.compute_control_device``; sigma is an (E, P) float32 tensor updated in place.
        sigma_reset: None or 0 -- sigma is read; a positive constant -- every environment starts this call from it
        and sigma is only written (the first sampling iteration of a control step; see the module docstring).
        due: None, or the (E,) int32 or bool mask of ``Batched_Sampling_MPC.compute_control_device``
        (``srbd_batch_step_cem_masked_device``): an environment that is not due keeps its rows of best parameters and
        sigma -- sigma_reset is not applied to it -- and the returned tensors hold its last solve.
        Returns the 8-tuple of ``compute_control`` as tensors, best parameters and sigma being the arguments."""
        import torch

        ctx = self.context
        E = self.num_envs
        if not isinstance(keys, torch.Tensor):
            raise ValueError("keys must be a torch tensor")
        dev = keys.device
        s = torch.cuda.current_stream(dev) if stream is None else stream
        if self.rng == "philox":
            if keys.dim() != 2 or tuple(keys.shape) != (E, 2):
                raise ValueError(f"keys must be ({E}, 2) (seed, counter), got {tuple(keys.shape)}")
            with torch.cuda.stream(s):
                seeds, counters = keys[:, 0].contiguous(), keys[:, 1].contiguous()
        else:
            if tuple(keys.shape) != (E,):
                raise ValueError(f"keys must be ({E},) packed JAX keys, got {tuple(keys.shape)}")
            seeds = keys
            with torch.cuda.stream(s):
                counters = torch.full((E,), self._calls + 1, dtype=torch.int64, device=dev)
        reset = 0.0 if sigma_reset is None else float(sigma_reset)
        if due is None:
            out = ctx.step_cem_device(states, references, contact_sequences, best_control_parameters, sigma, seeds,
                                      counters, sigma_reset=reset, noise=noise, stream=stream)
        else:
            out = self._held_result = ctx.step_cem_masked_device(
                states, references, contact_sequences, best_control_parameters, sigma, seeds, counters, due,
                sigma_reset=reset, noise=noise, out=getattr(self, "_held_result", None), stream=stream)
        self._calls += 1
        with torch.cuda.stream(s):
            footholds = torch.zeros((E, 12), dtype=torch.int32, device=dev)
            freq = torch.full((E,), 1.65, dtype=torch.float64, device=dev)
        self.last_device_result = out
        return (out["grf"], footholds, out["predicted_state"], best_control_parameters, out["best_cost"], freq,
                LazyBatchCosts(ctx, self._calls, self), sigma)
