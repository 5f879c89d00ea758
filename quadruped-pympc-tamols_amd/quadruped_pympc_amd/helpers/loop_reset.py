"""Restarting single environments of the batched, device-resident loop (``srbd_loop_reset_device``,
include/srbd_mpc.h): what the reference's simulation loop does when an episode ends (simulation/simulation.py:773-781,
``WBInterface.reset``, wb_interface.py:469-484), for the environments a mask names, in one launch on the caller's
stream and without a host wait."""
from __future__ import annotations

from .. import _lib

RESET_REFERENCE, RESET_EPISODE = _lib.RESET_REFERENCE, _lib.RESET_EPISODE


def mask_words(mask, num_envs, stream=None):
    """The (E,) int32 mask words of ``srbd_loop_reset_device`` from a bool, int32 or int64 tensor, converted on
    ``stream`` without a host read.  Bool means level 1 (the reference's reset); an int32 tensor is passed as it is."""
    import torch

    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.int32, torch.int64):
        raise ValueError(f"mask must be a bool, int32 or int64 torch tensor, got "
                         f"{getattr(mask, 'dtype', type(mask).__name__)}")
    if tuple(mask.shape) != (num_envs,):
        raise ValueError(f"mask must be ({num_envs},), got {tuple(mask.shape)}")
    if mask.dtype == torch.int32 and mask.is_contiguous():
        return mask
    if mask.device.type != "cuda":
        raise ValueError(f"mask must be on a cuda device, got {mask.device}")
    with torch.cuda.stream(torch.cuda.current_stream(mask.device) if stream is None else stream):
        return mask.to(torch.int32).contiguous()


def reference_words(mask, num_envs, stream=None):
    """Mask words that select the reference's level wherever ``mask`` is not zero (what the classes' own
    ``reset(mask=...)`` pass): (E,) int32 of 0 and 1, formed on ``stream`` without a host read."""
    import torch

    words = mask_words(mask, num_envs, stream)
    if words.device.type != "cuda":
        raise ValueError(f"mask must be on a cuda device, got {words.device}")
    with torch.cuda.stream(torch.cuda.current_stream(words.device) if stream is None else stream):
        return (words != 0).to(torch.int32)


class BatchedLoopReset:
    """Per-environment reset of the batched loop's device state.

    ``gait`` a ``BatchedPeriodicGaitGenerator``, ``frg`` a ``BatchedFootholdReferenceGenerator``, ``stc`` a
    ``BatchedSwingTrajectoryController``, ``terrain_est`` a ``BatchedTerrainEstimator``, ``vfa`` a
    ``BatchedVisualFootholdAdaptation``, each optional.  The constructor clones each given class's state tensor: the
    clones are the snapshots an episode reset restores, so build this object right after the classes, before their
    first step.

    ``reset(mask, initial_feet)`` chooses per environment: 0 leaves it untouched (and unread: a NaN in its
    ``initial_feet`` changes nothing), 2 (``RESET_EPISODE``) puts every struct back to what its constructor produced
    -- the foothold generator rebuilt on ``initial_feet[e]`` with an empty velocity history, the swing clocks, the
    terrain filter, ``step_freq`` and ``swing_period`` at their constructor values, the touch-down trigger word and the
    warm-start row of ``best_control_parameters`` cleared -- and any other value (``RESET_REFERENCE``; a bool mask
    means this) is the reference's ``WBInterface.reset``: the gait generator's ``reset()``, the lift-off table =
    ``initial_feet[e]``, the adaptation's ``initialized`` cleared, nothing else.  At both levels the rows of every
    tensor in ``contact_rows`` are set to ones (``current_contact = [1, 1, 1, 1]``)."""

    def __init__(self, num_envs, gait=None, frg=None, stc=None, terrain_est=None, vfa=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        self.num_envs = E
        self._parts = dict(pgg=gait, frg=frg, stc=stc, terrain_est=terrain_est, vfa=vfa)
        for name, obj in self._parts.items():
            if obj is not None and int(getattr(obj, "num_envs", -1)) != E:
                raise ValueError(f"{name} holds {getattr(obj, 'num_envs', None)} environments, expected {E}")
        self.stc = stc
        # everything above is host work; the clones are the first use of the device
        self.snapshots = {name: obj.state.clone() for name, obj in self._parts.items() if obj is not None}

    def reset(self, mask, initial_feet=None, *, best_control_parameters=None, contact_rows=(), stream=None):
        """One launch on ``stream`` (None: torch's current stream), no host wait.  mask (E,) bool, int32 or int64;
        initial_feet (E, 4, 3) float64, required when a foothold generator was given; best_control_parameters (E, P)
        float32; contact_rows up to four (E, 4) float32 tensors.  The swing controller's touch-down trigger words
        (``rising_edge``) are reset with it when it has them."""
        words = mask_words(mask, self.num_envs, stream)
        states = {name: obj.state for name, obj in self._parts.items() if obj is not None}
        edge = getattr(self.stc, "rising_edge", None)
        _lib.loop_reset_device(words, initial_feet, snapshots=self.snapshots, rising_edge=edge,
                               best_params=best_control_parameters, contact_rows=contact_rows, stream=stream,
                               **states)
