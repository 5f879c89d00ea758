"""Early-stance detector: finds the swing foot that hit something before its touch-down, for the swing reflex.

Mirror of ``quadruped_pympc/helpers/early_stance_detector.py`` (reference): the same constructor, attributes
(``early_stance``, ``hitmoments``, ``hitpoints``, the three thresholds, the gait-cycle counter) and
``update_detection`` (:36-128), for ``reflex_trigger_mode`` ``'tracking'`` and ``False``.  The state lives in a
``srbd_reflex`` struct and the detection runs in ``libsrbd_hip.so``'s C++ host function ``srbd_reflex_detect``
(``include/srbd_host.h``, ``csrc/srbd_reflex.h``), the function the device launch ``srbd_reflex_step_device`` compiles
too.  ``'geom_contact'`` reads MuJoCo contact lists and is not available.

``ReflexSwingTrajectoryController`` (``swing_trajectory_controller.py``) holds one of these on the struct its spline
generator reads, as ``WBInterface`` holds ``esd`` beside ``stc``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .. import config as cfg
from .legs_attr import LEG_NAMES, LegsAttr


def trigger_code(mode):
    """``reflex_trigger_mode`` -> ``srbd_reflex.trigger_mode``."""
    if mode == "geom_contact":
        raise NotImplementedError("reflex_trigger_mode 'geom_contact' is not available (it reads MuJoCo contact "
                                  "lists): use 'tracking' or False")
    if mode is False or mode is None:
        return _lib.REFLEX_OFF
    if mode == "tracking":
        return _lib.REFLEX_TRACKING
    raise ValueError(f"reflex_trigger_mode must be 'tracking' or False, got {mode!r}")


def _legs(values, name, legs_order=LEG_NAMES):
    """(4, 3) float64 from a LegsAttr, a mapping by leg name or an array."""
    if isinstance(values, np.ndarray):
        rows = values
    else:
        rows = [np.asarray(values[leg], dtype=np.float64).reshape(-1) for leg in legs_order]
    a = np.ascontiguousarray(rows, dtype=np.float64)
    if a.size != 12:
        raise ValueError(f"{name} must hold 4 x 3 values, got shape {a.shape}")
    return a.reshape(4, 3)


class EarlyStanceDetector:
    def __init__(self, feet_geom_id=None, legs_order=("FL", "FR", "RL", "RR"), *, reflex=None):
        """``reflex``: a ``_lib.SrbdReflex`` to work on (``ReflexSwingTrajectoryController`` passes its own); None
        builds one from ``config.simulation_params`` as the reference's constructor reads them."""
        self.legs_order = legs_order
        self.feet_geom_id = feet_geom_id
        if reflex is None:
            sp = cfg.simulation_params
            reflex = _lib.SrbdReflex()
            rc = _lib.lib.srbd_reflex_init(C.byref(reflex), float(sp["reflex_max_step_height"]),
                                           int(sp["visual_foothold_adaptation"] == "blind"),
                                           trigger_code(sp["reflex_trigger_mode"]),
                                           int(bool(sp["reflex_next_steps_height_enhancement"])))
            if rc != _lib.OK:
                raise ValueError(f"srbd_reflex_init failed ({rc}): reflex_max_step_height must be finite")
        self._r = reflex

    # ---- the reference's attributes, read from the struct
    @property
    def trigger_mode(self):
        return "tracking" if self._r.trigger_mode == _lib.REFLEX_TRACKING else False

    @property
    def activated(self):
        return self._r.trigger_mode != _lib.REFLEX_OFF

    @property
    def early_stance(self):
        return LegsAttr(*[bool(v) for v in self._r.early_stance])

    @property
    def hitmoments(self):
        return LegsAttr(*[float(v) for v in self._r.hitmoments])

    @property
    def hitpoints(self):
        return LegsAttr(*[np.array(self._r.hitpoints[l][:]) if self._r.has_hitpoint[l] else None for l in range(4)])

    early_stance_time_threshold = property(lambda s: s._r.early_stance_time_threshold)
    relative_tracking_error_threshold = property(lambda s: s._r.relative_tracking_error_threshold)
    absolute_min_distance_error_threshold = property(lambda s: s._r.absolute_min_distance_error_threshold)
    gait_cycles_after_reflex_height_enanchement = property(lambda s: s._r.gait_cycles)
    use_reflex_next_steps_height_enhancement = property(lambda s: bool(s._r.use_height_enhancement))
    max_gait_cycles_height_enhancement = property(lambda s: s._r.max_gait_cycles)

    def update_detection(self, feet_pos, des_feet_pos, lift_off, touch_down, swing_time, swing_period,
                         current_contact, previous_contact, mujoco_contact=None, stc=None):
        """``update_detection`` (:36-128).  ``des_feet_pos`` are the desired foot positions the previous step wrote;
        they are stored in the struct's ``last_des_foot_pos``, which the detection reads.  ``stc``: the controller
        whose generator takes the height-enhancement flag; one that works on another struct than this detector's
        gets the flag copied."""
        des = _legs(des_feet_pos, "des_feet_pos", self.legs_order)
        for l in range(4):
            for k in range(3):
                self._r.last_des_foot_pos[l][k] = des[l, k]
        clocks = np.ascontiguousarray(swing_time, dtype=np.float64).reshape(4)
        rc = _lib.lib.srbd_reflex_detect(
            C.byref(self._r), _lib.dptr(_legs(feet_pos, "feet_pos", self.legs_order)),
            _lib.dptr(_legs(lift_off, "lift_off", self.legs_order)),
            _lib.dptr(_legs(touch_down, "touch_down", self.legs_order)), _lib.dptr(clocks), float(swing_period),
            _lib.dptr(np.ascontiguousarray(current_contact, dtype=np.float64).reshape(4)),
            _lib.dptr(np.ascontiguousarray(previous_contact, dtype=np.float64).reshape(4)))
        if rc != _lib.OK:
            raise ValueError(f"srbd_reflex_detect failed ({rc})")
        other = getattr(stc, "_r", None)
        if other is not None and other is not self._r:
            other.height_enhancement = self._r.height_enhancement
