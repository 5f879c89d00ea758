"""Stance and swing leg controller: the joint torques of a control step from the MPC's ground-reaction forces.

Mirror of ``quadruped_pympc/helpers/swing_trajectory_controller.py`` (reference): the same constructor, attributes
and methods (``compute_swing_control_cartesian_space`` :48-94, ``update_swing_time`` :120-127,
``check_apex_condition`` :129-138, ``check_full_stance_condition`` :140-146,
``regenerate_swing_trajectory_generator`` :35-46, ``check_touch_down_condition`` :148-165), with the 'bezier_ref' and
'explicit' swing generators.  The state
lives in a ``srbd_stc`` struct and every method runs in ``libsrbd_hip.so``'s C++ host functions
(``include/srbd_host.h``).  ``BatchedSwingTrajectoryController`` keeps ``num_envs`` of these structs on the device and
runs the whole of ``WBInterface.compute_stance_and_swing_torque``'s leg law (wb_interface.py:369-415, :435-465) for
all of them in one launch (``srbd_stc_step_device``, ``include/srbd_mpc.h``).

Differences from the reference, all stated in the header: the leg Jacobian is inverted by cofactors over the
determinant where the reference calls ``np.linalg.pinv`` (the zero matrix for a singular Jacobian), the gains are
scalars, and the early-stance arguments of these two classes are accepted and ignored (neither generator here reads
them).  The 'scipy' generator, which does read them, is ``ReflexSwingTrajectoryController`` and
``BatchedReflexSwingTrajectoryController`` below, with the early-stance detector ahead of it (``srbd_reflex_step``,
``srbd_reflex_step_device``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib


def _check(rc, what):
    if rc < 0:
        raise ValueError(f"{what} failed ({rc})")
    return rc


def _generator_code(generator):
    if generator == "scipy":
        raise NotImplementedError("the 'scipy' swing generator is not available in this class: use 'bezier_ref' or "
                                  "'explicit', or ReflexSwingTrajectoryController / "
                                  "BatchedReflexSwingTrajectoryController for the spline generator with its reflexes")
    # the reference's constructor takes any other name as 'explicit'
    return _lib.SWING_CODES.get(generator, _lib.SWING_EXPLICIT)


def _arr(a, shape, name):
    """A contiguous float64 array of `shape`; extra axes of length one are dropped, as the reference's reshapes do."""
    v = np.ascontiguousarray(a, dtype=np.float64)
    if v.size == int(np.prod(shape)):
        v = v.reshape(shape)
    if v.shape != shape:
        raise ValueError(f"{name} must have shape {shape}, got {v.shape}")
    return v


class SwingTrajectoryController:
    def __init__(self, step_height, swing_period, position_gain_fb, velocity_gain_fb, generator):
        self.generator = generator
        self._g = _lib.SrbdStc()
        self._gp = C.byref(self._g)
        _check(_lib.lib.srbd_stc_init(self._gp, float(step_height), float(swing_period), float(position_gain_fb),
                                      float(velocity_gain_fb), _generator_code(generator)), "srbd_stc_init")
        self._edge = C.c_int32(0)

    @property
    def rising_edge_detected(self):
        """The touch-down trigger's state, a bool as in the reference."""
        return bool(self._edge.value)

    @rising_edge_detected.setter
    def rising_edge_detected(self, value):
        self._edge.value = int(bool(value))

    # plain attributes of the reference, backed by the C struct
    step_height = property(lambda s: s._g.step_height)
    swing_period = property(lambda s: s._g.swing_period)
    position_gain_fb = property(lambda s: s._g.position_gain_fb,
                                lambda s, v: setattr(s._g, "position_gain_fb", float(v)))
    velocity_gain_fb = property(lambda s: s._g.velocity_gain_fb,
                                lambda s, v: setattr(s._g, "velocity_gain_fb", float(v)))
    use_feedback_linearization = property(lambda s: bool(s._g.use_feedback_linearization),
                                          lambda s, v: setattr(s._g, "use_feedback_linearization", int(bool(v))))
    use_friction_compensation = property(lambda s: bool(s._g.use_friction_compensation),
                                         lambda s, v: setattr(s._g, "use_friction_compensation", int(bool(v))))

    @property
    def swing_time(self):
        """The four swing clocks, a list as in the reference (a copy: assign a sequence of four to replace them)."""
        return list(self._g.swing_time)

    @swing_time.setter
    def swing_time(self, value):
        v = _arr(value, (4,), "swing_time")
        for l in range(4):
            self._g.swing_time[l] = v[l]

    def regenerate_swing_trajectory_generator(self, step_height, swing_period):
        _check(_lib.lib.srbd_stc_set_timing(self._gp, float(step_height), float(swing_period)),
               "regenerate_swing_trajectory_generator")

    def compute_trajectory_references(self, leg_id, lift_off, touch_down):
        """The generator alone at the leg's current clock: desired foot position, velocity and acceleration."""
        pos, vel, acc = np.zeros(3), np.zeros(3), np.zeros(3)
        _check(_lib.lib.srbd_stc_reference(self._gp, int(leg_id), _lib.dptr(_arr(lift_off, (3,), "lift_off")),
                                           _lib.dptr(_arr(touch_down, (3,), "touch_down")), _lib.dptr(pos),
                                           _lib.dptr(vel), _lib.dptr(acc)), "compute_trajectory_references")
        return pos, vel, acc

    def compute_swing_control_cartesian_space(self, leg_id, q_dot, J, J_dot, lift_off, touch_down, foot_pos, foot_vel,
                                              passive_force, h, mass_matrix, early_stance_hitmoments=None,
                                              early_stance_hitpoints=None):
        """The swing torque of one leg at its current clock, and the desired foot position and velocity.  As in the
        reference, ``passive_force`` is not used here (the caller subtracts it) and the clock is not advanced."""
        leg_id = int(leg_id)
        if not 0 <= leg_id <= 3:
            raise ValueError(f"leg_id must be 0..3, got {leg_id}")
        # a one-leg view of srbd_stc_step: the leg in swing, dt = 0 (the clock is left as it is: t + 0.0 below the
        # period), friction compensation off for the call
        g = _lib.SrbdStc.from_buffer_copy(bytes(self._g))
        g.use_friction_compensation = 0
        z3, z9 = np.zeros((4, 3)), np.zeros((4, 3, 3))

        def leg(a, shape, name):
            full = (z9 if shape == (3, 3) else z3).copy()
            full[leg_id] = _arr(a, shape, name)
            return full

        contact = np.ones(4)
        contact[leg_id] = 0.0
        tau, dpos, dvel = np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3))
        arrays = dict(jac=leg(J, (3, 3), "J"), jac_dot=leg(J_dot, (3, 3), "J_dot"),
                      mass_matrix=leg(mass_matrix, (3, 3), "mass_matrix"), q_dot=leg(q_dot, (3,), "q_dot"),
                      foot_pos=leg(foot_pos, (3,), "foot_pos"), foot_vel=leg(foot_vel, (3,), "foot_vel"),
                      qfrc_passive=z3.copy(), qfrc_bias=leg(h, (3,), "h"), grfs=z3.copy(),
                      lift_off=leg(lift_off, (3,), "lift_off"), touch_down=leg(touch_down, (3,), "touch_down"),
                      contact=contact, tau=tau, des_foot_pos=dpos, des_foot_vel=dvel)
        io = _lib.SrbdStcIo(apex_interval=0.0, **{k: _lib.dptr(v) for k, v in arrays.items()})
        _check(_lib.lib.srbd_stc_step(C.byref(g), C.byref(io), 0.0), "compute_swing_control_cartesian_space")
        return tau[leg_id].copy(), dpos[leg_id].copy(), dvel[leg_id].copy()

    def update_swing_time(self, current_contact, legs_order, dt):
        _check(_lib.lib.srbd_stc_update_swing_time(self._gp, _lib.dptr(_arr(current_contact, (4,), "current_contact")),
                                                   float(dt)), "update_swing_time")

    def check_apex_condition(self, current_contact, interval=0.02):
        return _check(_lib.lib.srbd_stc_apex(self._gp, _lib.dptr(_arr(current_contact, (4,), "current_contact")),
                                             float(interval)), "check_apex_condition")

    def check_full_stance_condition(self, current_contact):
        return _check(_lib.lib.srbd_stc_full_stance(_lib.dptr(_arr(current_contact, (4,), "current_contact"))),
                      "check_full_stance_condition")

    def check_touch_down_condition(self, current_contact, previous_contact, contact_sequence, lookahead=3):
        """1 when all feet have touched down since the last trigger (a rising edge of full stance), the first
        ``lookahead`` columns of the contact sequence are full stance and column ``lookahead`` is not; else 0
        (``srbd_stc_touch_down``).  IndexError where the reference's ``contact_sequence[:, lookahead]`` raises it."""
        seq = np.ascontiguousarray(contact_sequence, dtype=np.float64)
        if seq.ndim != 2 or seq.shape[0] != 4:
            raise ValueError(f"contact_sequence must be (4, horizon), got {seq.shape}")
        rc = _lib.lib.srbd_stc_touch_down(C.byref(self._edge), _lib.dptr(_arr(current_contact, (4,), "current_contact")),
                                          _lib.dptr(_arr(previous_contact, (4,), "previous_contact")), _lib.dptr(seq),
                                          seq.shape[1], seq.shape[1], int(lookahead))
        if rc < 0:
            raise IndexError(f"lookahead must be 1..{seq.shape[1] - 1} for a sequence of {seq.shape[1]} columns, got "
                             f"{lookahead}")
        return rc

    def step(self, dt, jac, jac_dot, q_dot, foot_pos, foot_vel, qfrc_passive, qfrc_bias, mass_matrix, grfs, lift_off,
             touch_down, contact, apex_interval=0.01):
        """One whole control step (``srbd_stc_step``): the clock update, the four legs, friction compensation and the
        two flags.  Arrays are (4, 3, 3) / (4, 3) / (4,) float64.  Returns ``(tau, des_foot_pos, des_foot_vel,
        des_joint_vel, apex, full_stance)``, the first four (4, 3), the flags ints."""
        out = {k: np.zeros((4, 3)) for k in ("tau", "des_foot_pos", "des_foot_vel", "des_joint_vel")}
        apex, full = C.c_int32(0), C.c_int32(0)
        m, v = (4, 3, 3), (4, 3)
        arrays = dict(jac=_arr(jac, m, "jac"), jac_dot=_arr(jac_dot, m, "jac_dot"),
                      mass_matrix=_arr(mass_matrix, m, "mass_matrix"), q_dot=_arr(q_dot, v, "q_dot"),
                      foot_pos=_arr(foot_pos, v, "foot_pos"), foot_vel=_arr(foot_vel, v, "foot_vel"),
                      qfrc_passive=_arr(qfrc_passive, v, "qfrc_passive"), qfrc_bias=_arr(qfrc_bias, v, "qfrc_bias"),
                      grfs=_arr(grfs, v, "grfs"), lift_off=_arr(lift_off, v, "lift_off"),
                      touch_down=_arr(touch_down, v, "touch_down"), contact=_arr(contact, (4,), "contact"), **out)
        io = _lib.SrbdStcIo(apex_interval=float(apex_interval), apex=C.pointer(apex), full_stance=C.pointer(full),
                            **{k: _lib.dptr(a) for k, a in arrays.items()})
        _check(_lib.lib.srbd_stc_step(self._gp, C.byref(io), float(dt)), "srbd_stc_step")
        return (out["tau"], out["des_foot_pos"], out["des_foot_vel"], out["des_joint_vel"], int(apex.value),
                int(full.value))


class BatchedSwingTrajectoryController:
    """``num_envs`` leg controllers whose state lives on the device (``srbd_stc_step_device``, include/srbd_mpc.h): the
    consumer of the (E, 12) ground-reaction forces ``Batched_Sampling_MPC.compute_control_device`` returns and the
    producer of the joint torques a batched simulator applies, with no host round trip.

    Environment ``e`` behaves as a host ``SwingTrajectoryController(step_height[e], swing_period[e],
    position_gain_fb[e], velocity_gain_fb[e], generator[e])`` whose ``step`` is called each control step: its state
    keeps the host struct's bytes and its outputs are the host's, bit for bit.  The four numbers are scalars or
    length-E sequences, ``generator`` a name or a sequence of E names.  The state is one (E, sizeof(srbd_stc)) uint8
    tensor, ``state``, built from host ``srbd_stc_init`` structs; the touch-down trigger's state is ``rising_edge``,
    an (E,) int32 tensor.  ``step`` and ``check_touch_down_condition`` enqueue on the current stream and do not wait
    for the device; ``state_dict`` does.  The Jacobians, mass matrices, bias and passive forces are the
    simulator's to provide."""

    def __init__(self, num_envs, step_height, swing_period, position_gain_fb, velocity_gain_fb,
                 generator="bezier_ref", device=None):
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

        height, period = per_env("step_height", step_height), per_env("swing_period", swing_period)
        kp, kd = per_env("position_gain_fb", position_gain_fb), per_env("velocity_gain_fb", velocity_gain_fb)
        names = [generator] * E if isinstance(generator, str) else list(generator)
        if len(names) != E:
            raise ValueError(f"generator must be a name or {E} names, got {len(names)}")
        codes = [_generator_code(n) for n in names]
        self.num_envs = E
        host = (_lib.SrbdStc * E)()
        for e in range(E):
            if _lib.lib.srbd_stc_init(C.byref(host[e]), height[e], period[e], kp[e], kd[e], codes[e]) != _lib.OK:
                raise ValueError(f"environment {e}: swing_period must be positive and finite, got {period[e]}")
        # everything above is host work; the upload is the first use of the device
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("BatchedSwingTrajectoryController: no HIP device visible (the controller state lives "
                               "in device memory; SwingTrajectoryController is the host form)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.state = torch.empty((E, _lib.STC_BYTES), dtype=torch.uint8, device=self.device)
        self.rising_edge = torch.zeros(E, dtype=torch.int32, device=self.device)
        self._out = None
        self.load_state_dict(host)

    def _doubles(self, field, n):
        import torch

        o = getattr(_lib.SrbdStc, field).offset // 8
        return self.state.view(torch.float64)[:, o:o + n]

    @property
    def swing_time(self):
        """(E, 4) float64 view of the state's swing clocks."""
        return self._doubles("swing_time", 4)

    @property
    def swing_period(self):
        """(E,) float64 view of the state's swing periods."""
        return self._doubles("swing_period", 1)[:, 0]

    @property
    def step_height(self):
        """(E,) float64 view of the state's step heights."""
        return self._doubles("step_height", 1)[:, 0]

    def state_dict(self):
        """The host structs, a ``(SrbdStc * E)`` ctypes array (waits for the device): for checkpoints and tests.
        ``bytes()`` of it is a plain byte string; ``load_state_dict`` takes either.  The trigger's state rides along
        as the array's ``rising_edge`` attribute, an (E,) int32 NumPy array."""
        raw = self.state.cpu().numpy().tobytes()
        structs = (_lib.SrbdStc * self.num_envs).from_buffer_copy(raw)
        structs.rising_edge = self.rising_edge.cpu().numpy().copy()
        return structs

    def load_state_dict(self, structs):
        import torch

        raw = np.frombuffer(bytes(structs), dtype=np.uint8)
        if raw.size != self.num_envs * _lib.STC_BYTES:
            raise ValueError(f"{self.num_envs} srbd_stc structs expected ({self.num_envs * _lib.STC_BYTES} bytes), got "
                             f"{raw.size} bytes")
        # the trigger's state: what state_dict attached, or no edge pending (a plain byte string carries none)
        edge = np.asarray(getattr(structs, "rising_edge", np.zeros(self.num_envs)), dtype=np.int32)
        if edge.shape != (self.num_envs,):
            raise ValueError(f"rising_edge must have {self.num_envs} entries, got shape {edge.shape}")
        with torch.cuda.stream(torch.cuda.current_stream(self.device)):
            self.state.copy_(torch.from_numpy(raw.reshape(self.num_envs, _lib.STC_BYTES).copy()))
            self.rising_edge.copy_(torch.from_numpy(edge.copy()))

    def check_touch_down_condition(self, current, previous, contacts, lookahead=3, stream=None):
        """``check_touch_down_condition`` of every environment (``srbd_stc_touch_down_device``): current / previous
        (E, 4) float32 as ``BatchedPeriodicGaitGenerator.run`` returns them, contacts (E, 4, H) float32 as its
        ``compute_contact_sequence`` returns them.  Returns the (E,) int32 cuda tensor of flags, ``optimize_swing`` per
        environment; ``rising_edge`` is updated in place.  One launch, no host synchronisation."""
        return _lib.stc_touch_down_device(self.rising_edge, current, previous, contacts, lookahead, stream=stream)

    def regenerate_swing_trajectory_generator(self, step_height, swing_period):
        """Every environment's step height and swing period (wb_interface.py:358); the clocks are left alone.
        (E,) float64 tensors or arrays, or scalars; a swing period must be positive and finite."""
        import torch

        h = torch.as_tensor(step_height, dtype=torch.float64)
        p = torch.as_tensor(swing_period, dtype=torch.float64)
        for name, t in (("step_height", h), ("swing_period", p)):
            if t.dim() != 0 and tuple(t.shape) != (self.num_envs,):
                raise ValueError(f"{name} must be a scalar or ({self.num_envs},), got {tuple(t.shape)}")
        if p.device.type == "cpu" and not bool((torch.isfinite(p) & (p > 0)).all()):
            raise ValueError("swing_period must be positive and finite")
        with torch.cuda.stream(torch.cuda.current_stream(self.device)):
            self.step_height.copy_(h.expand(self.num_envs))
            self.swing_period.copy_(p.expand(self.num_envs))

    def step(self, dt, jac, jac_dot, q_dot, foot_pos, foot_vel, qfrc_passive, qfrc_bias, mass_matrix, grfs, touch_down,
             contact, lift_off=None, frg=None, apex_interval=0.01):
        """One control step of every environment on torch's current stream: the swing clocks, then per leg the stance
        torque ``-J.T @ grf`` or the swing generator with the Cartesian PD law and feedback linearisation, friction
        compensation, and the desired joint velocity.  jac / jac_dot / mass_matrix (E, 4, 3, 3), the leg's own three
        joint columns; q_dot / foot_pos / foot_vel / qfrc_passive / qfrc_bias / grfs / touch_down (E, 4, 3) float64
        cuda tensors (grfs may be the (E, 12) float64 GRFs viewed as (E, 4, 3)); contact (E, 4) float32 as
        ``BatchedPeriodicGaitGenerator.run`` returns it.  The lift-off positions come from ``lift_off`` (E, 4, 3) or
        from ``frg``, a ``BatchedFootholdReferenceGenerator`` (or its state tensor); exactly one of the two.
        Returns ``(tau, des_foot_pos, des_foot_vel, des_joint_vel, apex, full_stance)``: four (E, 4, 3) float64 and
        two (E,) int32 tensors, allocated once and rewritten by every call."""
        out = _lib.stc_step_device(self.state, dt, jac, jac_dot, q_dot, foot_pos, foot_vel, qfrc_passive, qfrc_bias,
                                   mass_matrix, grfs, touch_down, contact, lift_off=lift_off,
                                   frg=getattr(frg, "state", frg), apex_interval=apex_interval, out=self._out)
        self._out = out
        return (out["tau"], out["des_foot_pos"], out["des_foot_vel"], out["des_joint_vel"], out["apex"],
                out["full_stance"])


def _reflex_struct(reflex_max_step_height, blind, reflex_trigger_mode, next_steps_height_enhancement):
    from .early_stance_detector import trigger_code

    r = _lib.SrbdReflex()
    height = float(reflex_max_step_height)
    if _lib.lib.srbd_reflex_init(C.byref(r), height, int(bool(blind)), trigger_code(reflex_trigger_mode),
                                 int(bool(next_steps_height_enhancement))) != _lib.OK:
        raise ValueError(f"reflex_max_step_height must be finite, got {height}")
    return r


class ReflexSwingTrajectoryController(SwingTrajectoryController):
    """The reference's ``SwingTrajectoryController(generator="scipy")`` together with the ``EarlyStanceDetector`` that
    feeds it, as ``WBInterface.compute_stance_and_swing_torque`` composes them (wb_interface.py:362-415): ``esd`` is the
    detector, on the same ``srbd_reflex`` struct the spline generator reads, and ``step`` is one whole tick
    (``srbd_reflex_step``): the detector on what the previous tick left, the clock update, the leg law with the spline,
    the desired foot positions kept for the next tick's detector.  ``reflex_max_step_height`` and ``blind`` are what the
    reference's generator reads from its config (``reflex_max_step_height``, ``visual_foothold_adaptation == 'blind'``),
    ``reflex_trigger_mode`` and ``next_steps_height_enhancement`` what its detector reads."""

    def __init__(self, step_height, swing_period, position_gain_fb, velocity_gain_fb, generator="scipy", *,
                 reflex_max_step_height, blind=False, reflex_trigger_mode="tracking",
                 next_steps_height_enhancement=False):
        if generator != "scipy":
            raise ValueError(f"ReflexSwingTrajectoryController runs the 'scipy' generator, got {generator!r}")
        from .early_stance_detector import EarlyStanceDetector

        super().__init__(step_height, swing_period, position_gain_fb, velocity_gain_fb, "bezier_ref")
        self.generator = "scipy"  # the struct's generator code is not read by srbd_reflex_*
        self._r = _reflex_struct(reflex_max_step_height, blind, reflex_trigger_mode, next_steps_height_enhancement)
        self.esd = EarlyStanceDetector(reflex=self._r)

    reflex_max_step_height = property(lambda s: s._r.reflex_max_step_height)
    blind_locomotion = property(lambda s: bool(s._r.blind))
    reflex_next_steps_height_enhancement = property(lambda s: bool(s._r.height_enhancement),
                                                    lambda s, v: setattr(s._r, "height_enhancement", int(bool(v))))

    def compute_trajectory_references(self, leg_id, lift_off, touch_down):
        """The spline generator alone at the leg's current clock, with the leg's hit as the detector holds it."""
        pos, vel, acc = np.zeros(3), np.zeros(3), np.zeros(3)
        _check(_lib.lib.srbd_reflex_reference(self._gp, C.byref(self._r), int(leg_id),
                                              _lib.dptr(_arr(lift_off, (3,), "lift_off")),
                                              _lib.dptr(_arr(touch_down, (3,), "touch_down")), _lib.dptr(pos),
                                              _lib.dptr(vel), _lib.dptr(acc)), "compute_trajectory_references")
        return pos, vel, acc

    def compute_swing_control_cartesian_space(self, *args, **kwargs):
        raise NotImplementedError("ReflexSwingTrajectoryController has no one-leg form: step() runs the whole tick, "
                                  "the detector included")

    def step(self, dt, jac, jac_dot, q_dot, foot_pos, foot_vel, qfrc_passive, qfrc_bias, mass_matrix, grfs, lift_off,
             touch_down, contact, previous_contact, apex_interval=0.01):
        """One whole control step (``srbd_reflex_step``).  The parent's arguments plus ``previous_contact`` (4), the
        previous step's contact flags.  Returns the parent's tuple."""
        out = {k: np.zeros((4, 3)) for k in ("tau", "des_foot_pos", "des_foot_vel", "des_joint_vel")}
        apex, full = C.c_int32(0), C.c_int32(0)
        m, v = (4, 3, 3), (4, 3)
        arrays = dict(jac=_arr(jac, m, "jac"), jac_dot=_arr(jac_dot, m, "jac_dot"),
                      mass_matrix=_arr(mass_matrix, m, "mass_matrix"), q_dot=_arr(q_dot, v, "q_dot"),
                      foot_pos=_arr(foot_pos, v, "foot_pos"), foot_vel=_arr(foot_vel, v, "foot_vel"),
                      qfrc_passive=_arr(qfrc_passive, v, "qfrc_passive"), qfrc_bias=_arr(qfrc_bias, v, "qfrc_bias"),
                      grfs=_arr(grfs, v, "grfs"), lift_off=_arr(lift_off, v, "lift_off"),
                      touch_down=_arr(touch_down, v, "touch_down"), contact=_arr(contact, (4,), "contact"), **out)
        io = _lib.SrbdStcIo(apex_interval=float(apex_interval), apex=C.pointer(apex), full_stance=C.pointer(full),
                            **{k: _lib.dptr(a) for k, a in arrays.items()})
        _check(_lib.lib.srbd_reflex_step(self._gp, C.byref(self._r), C.byref(io),
                                         _lib.dptr(_arr(previous_contact, (4,), "previous_contact")), float(dt)),
               "srbd_reflex_step")
        return (out["tau"], out["des_foot_pos"], out["des_foot_vel"], out["des_joint_vel"], int(apex.value),
                int(full.value))


class BatchedReflexSwingTrajectoryController(BatchedSwingTrajectoryController):
    """``num_envs`` reflex leg controllers whose state lives on the device (``srbd_reflex_step_device``,
    include/srbd_mpc.h): ``BatchedSwingTrajectoryController`` with the early-stance detector ahead of the torques and
    the 'scipy' spline generator in the Bezier generators' place.  Environment ``e`` behaves as a host
    ``ReflexSwingTrajectoryController`` whose ``step`` is called each control step: both structs keep the host structs'
    bytes and the outputs are the host's, bit for bit.

    ``state`` stays the (E, sizeof(srbd_stc)) tensor of the parent, so ``apply_step_frequency``, ``BatchedLoopReset``,
    ``vfa.step_device(stc=)`` and ``rising_edge`` work on it unchanged; ``reflex_state`` is the
    (E, sizeof(srbd_reflex)) uint8 tensor beside it.  ``reflex_max_step_height`` and ``blind`` are scalars or length-E
    sequences; the trigger mode and the enhancement switch are shared.  ``BatchedLoopReset`` does not know
    ``reflex_state``: a caller that restarts environments calls ``reset(mask)`` here as well, on the same stream."""

    def __init__(self, num_envs, step_height, swing_period, position_gain_fb, velocity_gain_fb, *,
                 reflex_max_step_height, blind=False, reflex_trigger_mode="tracking",
                 next_steps_height_enhancement=False, device=None):
        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        heights = np.asarray(reflex_max_step_height, dtype=np.float64)
        blinds = np.asarray(blind)
        for name, a in (("reflex_max_step_height", heights), ("blind", blinds)):
            if a.ndim != 0 and a.shape != (E,):
                raise ValueError(f"{name} must be a scalar or have {E} entries, got shape {a.shape}")
        heights, blinds = np.broadcast_to(heights, (E,)), np.broadcast_to(blinds, (E,))
        host = (_lib.SrbdReflex * E)()
        for e in range(E):
            host[e] = _reflex_struct(heights[e], blinds[e], reflex_trigger_mode, next_steps_height_enhancement)
        super().__init__(E, step_height, swing_period, position_gain_fb, velocity_gain_fb, "bezier_ref", device=device)
        import torch

        raw = np.frombuffer(bytes(host), dtype=np.uint8).reshape(E, _lib.REFLEX_BYTES).copy()
        with torch.cuda.stream(torch.cuda.current_stream(self.device)):
            self._reflex_initial = torch.from_numpy(raw).to(self.device)
            self.reflex_state = self._reflex_initial.clone()

    def state_dict(self):
        """``{"stc": (SrbdStc * E) array, "reflex": (SrbdReflex * E) array}`` (waits for the device): the parent's
        structs, with ``rising_edge`` riding along as there, and the reflex structs, for checkpoints and tests."""
        reflex = (_lib.SrbdReflex * self.num_envs).from_buffer_copy(self.reflex_state.cpu().numpy().tobytes())
        return {"stc": super().state_dict(), "reflex": reflex}

    def load_state_dict(self, state):
        """What ``state_dict`` returns: both entries are required (each a ctypes array or its bytes), so a checkpoint
        cannot resume with one half of the controller stale.  The parent's form alone -- a ``(SrbdStc * E)`` array or a
        byte string -- is refused with a ValueError naming the missing half."""
        import torch

        if not hasattr(self, "reflex_state"):  # the parent's constructor uploading its own structs
            return super().load_state_dict(state)
        if not isinstance(state, dict) or set(state) != {"stc", "reflex"}:
            raise ValueError("load_state_dict takes the dict state_dict returns, {'stc': ..., 'reflex': ...}: the "
                             "srbd_stc structs alone would leave the hits, counters and last_des_foot_pos stale")
        raw = np.frombuffer(bytes(state["reflex"]), dtype=np.uint8)
        if raw.size != self.num_envs * _lib.REFLEX_BYTES:
            raise ValueError(f"{self.num_envs} srbd_reflex structs expected "
                             f"({self.num_envs * _lib.REFLEX_BYTES} bytes), got {raw.size} bytes")
        super().load_state_dict(state["stc"])
        with torch.cuda.stream(torch.cuda.current_stream(self.device)):
            self.reflex_state.copy_(torch.from_numpy(raw.reshape(self.num_envs, _lib.REFLEX_BYTES).copy()))

    def reset(self, mask, stream=None):
        """The masked environments' reflex structs back to their constructor bytes: no hit, counter -1, flag off,
        ``last_des_foot_pos`` zero.  mask (E,) bool, int32 or int64 cuda tensor; a torch copy on ``stream`` (None: the
        current stream), no host wait.  The ``srbd_stc`` structs are ``BatchedLoopReset``'s to restore."""
        import torch

        from .loop_reset import mask_words

        words = mask_words(mask, self.num_envs, stream)
        with torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream):
            self.reflex_state.copy_(torch.where(words.to(self.device)[:, None] != 0, self._reflex_initial,
                                                self.reflex_state))

    def step(self, dt, jac, jac_dot, q_dot, foot_pos, foot_vel, qfrc_passive, qfrc_bias, mass_matrix, grfs, touch_down,
             contact, previous_contact, lift_off=None, frg=None, apex_interval=0.01):
        """One control step of every environment on torch's current stream (``srbd_reflex_step_device``): the
        parent's arguments plus ``previous_contact`` (E, 4) float32, the previous control step's contact flags (the
        row ``BatchedWBInterface`` owns).  Returns the parent's tuple."""
        out = _lib.reflex_step_device(self.state, self.reflex_state, dt, jac, jac_dot, q_dot, foot_pos, foot_vel,
                                      qfrc_passive, qfrc_bias, mass_matrix, grfs, touch_down, contact, previous_contact,
                                      lift_off=lift_off, frg=getattr(frg, "state", frg), apex_interval=apex_interval,
                                      out=self._out)
        self._out = out
        return (out["tau"], out["des_foot_pos"], out["des_foot_vel"], out["des_joint_vel"], out["apex"],
                out["full_stance"])
