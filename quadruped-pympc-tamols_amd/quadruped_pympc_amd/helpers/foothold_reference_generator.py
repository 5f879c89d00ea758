"""Foothold reference generator: the producer of the ``seeds`` the foothold adaptation refines, and on flat ground
(``visual_foothold_adaptation == 'blind'``) of the reference's feet directly.

Mirror of ``quadruped_pympc/helpers/foothold_reference_generator.py`` (reference): the same constructor, attributes
and methods (``compute_footholds_reference`` :53-157, ``update_lift_off_positions`` :159-178,
``update_touch_down_positions`` :180-199).  The state lives in a ``srbd_frg`` struct and every method runs in
``libsrbd_hip.so``'s C++ host producers (``include/srbd_host.h``).  ``BatchedFootholdReferenceGenerator`` keeps
``num_envs`` of these structs on the device and steps them in one launch (``srbd_frg_step_device``,
``include/srbd_mpc.h``).

Two differences from the reference, both stated in the header: cos and sin of the yaw are the correctly rounded
values (libm's differ in the last place for about 3 in 1000 yaws), and ``com_pos_offset_w`` is an attribute the
caller sets -- the reference forms it as ``Rotation.from_euler('xyz', rpy) @ com_pos_offset_b`` with a body offset
that is zero unless set by hand; that rotation is the caller's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib, config as cfg
from .legs_attr import LEG_NAMES, LegsAttr
from .periodic_gait_generator import FULL_STANCE


def _check(rc, what):
    if rc < 0:
        raise ValueError(f"{what} failed ({rc})")
    return rc


def _legs(a):
    """A (4, 3) float64 array from a LegsAttr (or anything indexable by leg name or leg number)."""
    if isinstance(a, np.ndarray):
        out = np.ascontiguousarray(a, dtype=np.float64)
    else:
        out = np.array([np.asarray(a[k], dtype=np.float64) for k in LEG_NAMES])
    if out.shape != (4, 3):
        raise ValueError(f"four legs of three coordinates expected, got shape {out.shape}")
    return out


def _legs_attr(table):
    return LegsAttr(*[np.array(table[l]) for l in range(4)])


def _vec(a, n, name):
    v = np.ascontiguousarray(a, dtype=np.float64)
    if v.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},), got {v.shape}")
    return v


class FootholdReferenceGenerator:
    def __init__(self, stance_time, lift_off_positions, vel_moving_average_length=20, hip_height=None):
        if int(vel_moving_average_length) != _lib.FRG_HIST:
            raise NotImplementedError(f"the velocity history holds {_lib.FRG_HIST} entries (SRBD_FRG_HIST); "
                                      f"vel_moving_average_length = {vel_moving_average_length} is not supported")
        self._g = _lib.SrbdFrg()
        self._gp = C.byref(self._g)
        self._no_hip_height = hip_height is None  # the reference constructs without one and fails where it is used
        _check(_lib.lib.srbd_frg_init(self._gp, float(stance_time), 0.0 if hip_height is None else float(hip_height),
                                      _lib.dptr(_legs(lift_off_positions))), "srbd_frg_init")
        self.com_pos_offset_b = np.zeros((3,))
        self.com_pos_offset_w = np.zeros((3,))
        self.gravity_constant = cfg.gravity_constant

    # plain attributes of the reference, backed by the C struct
    stance_time = property(lambda s: s._g.stance_time, lambda s, v: setattr(s._g, "stance_time", float(v)))
    hip_offset = property(lambda s: s._g.hip_offset, lambda s, v: setattr(s._g, "hip_offset", float(v)))

    @property
    def hip_height(self):
        return None if self._no_hip_height else self._g.hip_height

    @hip_height.setter
    def hip_height(self, v):
        self._no_hip_height = v is None
        self._g.hip_height = 0.0 if v is None else float(v)

    def _table(name):  # noqa: N805 -- a LegsAttr of copies; assign a LegsAttr to replace the table
        def get(self):
            return _legs_attr(getattr(self._g, name))

        def put(self, value):
            rows = _legs(value)
            field = getattr(self._g, name)
            for l in range(4):
                for k in range(3):
                    field[l][k] = rows[l, k]

        return property(get, put)

    lift_off_positions = _table("lift_off")
    lift_off_positions_h = _table("lift_off_h")
    touch_down_positions = _table("touch_down")
    touch_down_positions_h = _table("touch_down_h")
    last_reference_footholds = _table("last_reference_footholds")
    del _table

    @property
    def base_vel_hist(self):
        """The velocity history, oldest first: (n, 2), n <= 20."""
        g = self._g
        n, head = g.hist_len, g.hist_head
        first = head if n == _lib.FRG_HIST else 0
        return np.array([list(g.vel_hist[(first + i) % _lib.FRG_HIST]) for i in range(n)]).reshape(n, 2)

    def compute_footholds_reference(self, base_position, base_ori_euler_xyz, base_xy_lin_vel, ref_base_xy_lin_vel,
                                    hips_position, com_height_nominal):
        base_xy_lin_vel, ref_base_xy_lin_vel = np.asarray(base_xy_lin_vel), np.asarray(ref_base_xy_lin_vel)
        assert base_xy_lin_vel.shape == (2,) and ref_base_xy_lin_vel.shape == (2,), (
            f"Expected shape (2,):=[x_dot, y_dot], got {base_xy_lin_vel.shape} and {ref_base_xy_lin_vel.shape}."
        )
        if self._no_hip_height:
            raise TypeError("hip_height is None: compute_footholds_reference needs it (as in the reference)")
        out = np.zeros((4, 3))
        _check(_lib.lib.srbd_frg_compute(
            self._gp, _lib.dptr(_vec(base_position, 3, "base_position")), float(base_ori_euler_xyz[2]),
            _lib.dptr(_vec(base_xy_lin_vel, 2, "base_xy_lin_vel")),
            _lib.dptr(_vec(ref_base_xy_lin_vel, 2, "ref_base_xy_lin_vel")), _lib.dptr(_legs(hips_position)),
            float(com_height_nominal), float(self.gravity_constant),
            _lib.dptr(_vec(self.com_pos_offset_w, 3, "com_pos_offset_w")), _lib.dptr(out)),
            "compute_footholds_reference")
        return _legs_attr(out)

    def _update(self, fn, what, previous_contact, current_contact, feet_pos, legs_order, gait_type, base_position,
                base_ori_euler_xyz):
        order = [LEG_NAMES.index(k) for k in legs_order]
        if sorted(order) != [0, 1, 2, 3]:
            raise ValueError(f"legs_order must name FL, FR, RL and RR once each, got {legs_order}")
        prev, cur = np.zeros(4), np.zeros(4)
        for i, l in enumerate(order):  # contact i belongs to leg legs_order[i]
            prev[l], cur[l] = float(previous_contact[i]), float(current_contact[i])
        full = int(getattr(gait_type, "value", gait_type) == FULL_STANCE)
        _check(fn(self._gp, _lib.dptr(prev), _lib.dptr(cur), _lib.dptr(_legs(feet_pos)), full,
                  _lib.dptr(_vec(base_position, 3, "base_position")), float(base_ori_euler_xyz[2])), what)

    def update_lift_off_positions(self, previous_contact, current_contact, feet_pos, legs_order, gait_type,
                                  base_position, base_ori_euler_xyz):
        self._update(_lib.lib.srbd_frg_update_lift_off, "update_lift_off_positions", previous_contact,
                     current_contact, feet_pos, legs_order, gait_type, base_position, base_ori_euler_xyz)

    def update_touch_down_positions(self, previous_contact, current_contact, feet_pos, legs_order, gait_type,
                                    base_position, base_ori_euler_xyz):
        self._update(_lib.lib.srbd_frg_update_touch_down, "update_touch_down_positions", previous_contact,
                     current_contact, feet_pos, legs_order, gait_type, base_position, base_ori_euler_xyz)


class BatchedFootholdReferenceGenerator:
    """``num_envs`` foothold reference generators whose state lives on the device (``srbd_frg_step_device``,
    include/srbd_mpc.h): the producer of the (E, 4, 3) ``seeds`` ``BatchedVisualFootholdAdaptation`` consumes -- and,
    through ``ref``, of the reference's feet on flat ground -- with no host round trip.

    Environment ``e`` behaves as a ``FootholdReferenceGenerator(stance_time[e], lift_off_positions[e],
    hip_height=hip_height[e])`` that received ``update_lift_off_positions``, ``update_touch_down_positions`` and
    ``compute_footholds_reference`` in that order each step: its state keeps the host struct's bytes and its footholds
    are the host's.  ``stance_time`` and ``hip_height`` are scalars or length-E sequences; ``lift_off_positions`` is
    (4, 3) for all environments or (E, 4, 3).  The state is one (E, sizeof(srbd_frg)) uint8 tensor, ``state``, built
    from host ``srbd_frg_init`` structs.  ``step`` enqueues on ``stream`` (None: torch's current stream) and does not
    wait for the device; ``state_dict`` does."""

    def __init__(self, num_envs, stance_time, hip_height, lift_off_positions, device=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")

        def per_env(name, v):
            a = np.asarray(v, dtype=np.float64)
            if a.ndim == 0:
                return np.full(E, a)
            if a.shape != (E,):
                raise ValueError(f"{name} must be a scalar or have {E} entries, got shape {a.shape}")
            return a

        stance, height = per_env("stance_time", stance_time), per_env("hip_height", hip_height)
        lift = np.asarray(lift_off_positions if not isinstance(lift_off_positions, LegsAttr)
                          else _legs(lift_off_positions), dtype=np.float64)
        if lift.shape == (4, 3):
            lift = np.broadcast_to(lift, (E, 4, 3))
        if lift.shape != (E, 4, 3):
            raise ValueError(f"lift_off_positions must be (4, 3) or ({E}, 4, 3), got {lift.shape}")
        self.num_envs = E
        self.gravity_constant = cfg.gravity_constant
        host = (_lib.SrbdFrg * E)()
        for e in range(E):
            if _lib.lib.srbd_frg_init(C.byref(host[e]), float(stance[e]), float(height[e]),
                                      _lib.dptr(np.ascontiguousarray(lift[e]))) != _lib.OK:
                raise ValueError(f"environment {e}: stance_time and hip_height must be finite, got {stance[e]}, "
                                 f"{height[e]}")
        # everything above is host work; the upload is the first use of the device
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("BatchedFootholdReferenceGenerator: no HIP device visible (the generator state lives "
                               "in device memory; FootholdReferenceGenerator is the host form)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.empty((E, _lib.FRG_BYTES), dtype=torch.uint8, device=self.device)
        self.load_state_dict(host)

    def _doubles(self, field, n):
        import torch

        o = getattr(_lib.SrbdFrg, field).offset // 8
        return self.state.view(torch.float64)[:, o:o + n]

    @property
    def stance_time(self):
        """(E,) float64 view of the state's stance times."""
        return self._doubles("stance_time", 1)[:, 0]

    @property
    def lift_off_positions(self):
        """(E, 4, 3) float64 view of the state's world-frame lift-off positions."""
        return self._doubles("lift_off", 12).unflatten(1, (4, 3))

    @property
    def touch_down_positions(self):
        """(E, 4, 3) float64 view of the state's world-frame touch-down positions."""
        return self._doubles("touch_down", 12).unflatten(1, (4, 3))

    @property
    def last_reference_footholds(self):
        """(E, 4, 3) float64 view of the last step's footholds."""
        return self._doubles("last_reference_footholds", 12).unflatten(1, (4, 3))

    def _on(self, stream):
        import torch

        return torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream)

    def state_dict(self):
        """The host structs, a ``(SrbdFrg * E)`` ctypes array (waits for the device): for checkpoints and tests.
        ``bytes()`` of it is a plain byte string; ``load_state_dict`` takes either."""
        raw = self.state.cpu().numpy().tobytes()
        return (_lib.SrbdFrg * self.num_envs).from_buffer_copy(raw)

    def load_state_dict(self, structs, stream=None):
        import torch

        raw = np.frombuffer(bytes(structs), dtype=np.uint8)
        if raw.size != self.num_envs * _lib.FRG_BYTES:
            raise ValueError(f"{self.num_envs} srbd_frg structs expected ({self.num_envs * _lib.FRG_BYTES} bytes), got "
                             f"{raw.size} bytes")
        with self._on(stream):
            self.state.copy_(torch.from_numpy(raw.reshape(self.num_envs, _lib.FRG_BYTES).copy()))

    def set_stance_time(self, stance_time, stream=None):
        """Every environment's stance time (wb_interface.py:356 rewrites it when the step frequency changes):
        an (E,) float64 tensor or array, or a scalar."""
        import torch

        src = torch.as_tensor(stance_time, dtype=torch.float64)
        if src.dim() != 0 and tuple(src.shape) != (self.num_envs,):
            raise ValueError(f"stance_time must be a scalar or ({self.num_envs},), got {tuple(src.shape)}")
        with self._on(stream):
            self.stance_time.copy_(src.expand(self.num_envs))

    def step(self, base_pos, yaws, base_lin_vel, ref_lin_vel, hips, feet, previous_contact, current_contact,
             gait=None, com_pos_offset_w=None, ref=None, out=None, stream=None, com_height_nominal=None):
        """One control step of every environment: lift-off and touch-down bookkeeping, then the reference footholds
        -> the seeds, (E, 4, 3) float64 (``out`` when given).  base_pos / base_lin_vel / ref_lin_vel (E, 3), yaws
        (E,), hips / feet (E, 4, 3) float64 tensors; previous_contact / current_contact (E, 4) float32 as
        ``BatchedPeriodicGaitGenerator.run`` returns them.  gait: a ``BatchedPeriodicGaitGenerator`` (or its state
        tensor) whose FULL_STANCE environments take the reference's full-stance branch; com_pos_offset_w (E, 3);
        ref (E, 24) float64, ``prepare_state_and_reference_device``'s ref_in, whose entries 12..23 receive the
        footholds.  com_height_nominal: the shared nominal height, None for the configuration's ``ref_z``."""
        chn = cfg.simulation_params["ref_z"] if com_height_nominal is None else com_height_nominal
        pgg = getattr(gait, "state", gait)
        return _lib.frg_step_device(self.state, base_pos, yaws, base_lin_vel, ref_lin_vel, hips, feet,
                                    previous_contact, current_contact, chn, self.gravity_constant, pgg=pgg,
                                    com_pos_offset_w=com_pos_offset_w, ref=ref, out=out, stream=stream)
