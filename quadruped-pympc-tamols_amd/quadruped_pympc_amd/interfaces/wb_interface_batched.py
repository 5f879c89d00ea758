"""``WBInterface.update_state_and_reference`` for a batch of environments, device-resident, in one launch
(``srbd_wb_update_device``, include/srbd_mpc.h): velocity modulator, start-and-stop, gait generator run, contact
sequence, contact bookkeeping, foothold reference generator, terrain estimate with the reference row and the touch-down
trigger (quadruped_pympc/interfaces/wb_interface.py:168-298).  The visual foothold adaptation (:230-246) is not part of
it: ``BatchedVisualFootholdAdaptation.step`` stays the separate launch behind this call and rewrites ``ref[:, 12:24]``.

A batched control step is then::

    ref, contacts, cur, prev, seeds, optimize, lin, ang = wb.update_state_and_reference_device(
        com_pos, base_pos, base_lin_vel, base_ori_euler_xyz, base_ang_vel, feet_pos, hip_pos, simulation_dt,
        ref_base_lin_vel, ref_base_ang_vel)
    # (vfa.step(...) on uneven ground)
    out = controller.compute_control_device(state, ref, contacts, ...)          # the interface step
    apply_step_frequency(optimize, out["best_freq"], gait, frg, stc)            # when optimize_step_freq
    tau = stc.step(simulation_dt, ..., contact=cur, frg=frg)                    # leg torques
    reset.reset(done, initial_feet, contact_rows=wb.contact_rows)               # episodes that ended

The current contact is column 0 of the contact sequence, also in an environment that start-and-stop put into full
stance -- there the sequence is all ones, whatever ``gait.run`` would have returned -- so ``cur`` (not the flags of a
separate ``gait.run``) is what the leg controller and the next step's bookkeeping take.

Episode reset.  ``BatchedLoopReset.reset(mask, initial_feet, contact_rows=wb.contact_rows)`` sets this interface's two
contact rows to ones for every reset environment, as ``WBInterface.reset`` sets ``current_contact``.  The trigger words
are reset with the swing controller's when the interface was built on them (``rising_edge=stc.rising_edge``); an
interface that owns its words clears them itself, ``wb.rising_edge.masked_fill_(mask, 0)``.  An environment that was
in full stance keeps ``gait_type == FULL_STANCE`` through the reference's level (``pgg.reset()`` keeps the gait type,
as in the reference) and walks again at the next step with a command; the episode level puts the generator back to
its constructor bytes, gait type included.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _lib
from .. import config as cfg


class BatchedWBInterface:
    """The front half of the batched control step on the device objects the caller already has.

    ``gait`` a ``BatchedPeriodicGaitGenerator``, ``frg`` a ``BatchedFootholdReferenceGenerator``, ``terrain_est`` a
    ``BatchedTerrainEstimator``: their state tensors are advanced in place, nothing is constructed twice.  The
    interface owns ``current_contact`` and ``previous_contact`` (E, 4) float32, ones at start, and ``rising_edge`` (E,)
    int32 (or shares the one given), and the output tensors it returns, which the next call overwrites.

    Attributes as in the reference, read at every call: ``vm_activated`` and ``start_and_stop_activated`` (both False
    by default), ``optimize_step_freq`` (the configuration's), ``lookahead`` (3), ``max_distance`` (0.2)."""

    def __init__(self, num_envs, gait, frg, terrain_est, *, mpc_dt=None, contact_sequence_dts=None,
                 contact_sequence_lenghts=None, horizon=None, ref_z=None, com_height_nominal=None, gravity=None,
                 contact_stride=None, lookahead=3, max_distance=0.2, optimize_step_freq=None, rising_edge=None):
        import torch

        E = int(num_envs)
        if not 1 <= E <= _lib.MAX_ENVS:
            raise ValueError(f"num_envs must be 1..{_lib.MAX_ENVS}, got {num_envs}")
        for name, obj, size in (("gait", gait, _lib.PGG_BYTES), ("frg", frg, _lib.FRG_BYTES),
                                ("terrain_est", terrain_est, _lib.TERRAIN_EST_BYTES)):
            st = getattr(obj, "state", None)
            if not isinstance(st, torch.Tensor) or tuple(st.shape) != (E, size) or st.dtype != torch.uint8:
                raise ValueError(f"{name} must be the batched class of {E} environments (state ({E}, {size}) uint8)")
        H = int(gait.horizon if horizon is None else horizon)
        if not 2 <= H <= _lib.MAX_HORIZON:
            raise ValueError(f"horizon must be 2..{_lib.MAX_HORIZON}, got {H}")
        if contact_sequence_dts is None:
            if mpc_dt is None:
                raise ValueError("give mpc_dt or contact_sequence_dts / contact_sequence_lenghts")
            contact_sequence_dts, contact_sequence_lenghts = [mpc_dt], [H]
        self._dts = np.ascontiguousarray(contact_sequence_dts, dtype=np.float64).reshape(-1)
        self._lens = np.ascontiguousarray(contact_sequence_lenghts, dtype=np.int32).reshape(-1)
        n = min(self._dts.size, self._lens.size)
        if not 1 <= n <= _lib.MAX_DTS:
            raise ValueError(f"contact_sequence_dts / lenghts must have 1..{_lib.MAX_DTS} entries")
        stride = H if contact_stride is None else int(contact_stride)
        if stride < H:
            raise ValueError(f"contact_stride must be at least the horizon {H}, got {stride}")
        if not 1 <= int(lookahead) <= H - 1:
            raise IndexError(f"lookahead must be 1..{H - 1} (horizon - 1), got {lookahead}")
        z = float(terrain_est.ref_z if ref_z is None else ref_z)
        chn = float(cfg.simulation_params["ref_z"] if com_height_nominal is None else com_height_nominal)
        grav = float(frg.gravity_constant if gravity is None else gravity)
        if not (math.isfinite(z) and math.isfinite(chn) and math.isfinite(grav) and grav > 0.0):
            raise ValueError(f"ref_z and com_height_nominal must be finite and gravity finite and positive, got {z}, "
                             f"{chn}, {grav}")
        self.num_envs, self.horizon, self.lookahead = E, H, int(lookahead)
        self.gait, self.frg, self.terrain_est = gait, frg, terrain_est
        self.vm_activated = False
        self.start_and_stop_activated = False
        self.optimize_step_freq = bool(cfg.mpc_params["optimize_step_freq"] if optimize_step_freq is None
                                       else optimize_step_freq)
        self.max_distance = float(max_distance)
        self.device = dev = gait.state.device
        for name, obj in (("frg", frg), ("terrain_est", terrain_est)):
            if obj.state.device != dev:
                raise ValueError(f"{name} must be on {dev}, got {obj.state.device}")
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        self.current_contact = torch.ones((E, 4), dtype=f32, device=dev)   # the contact state the call advances
        self.previous_contact = torch.ones((E, 4), dtype=f32, device=dev)
        if rising_edge is None:
            rising_edge = torch.zeros(E, dtype=i32, device=dev)
        elif (not isinstance(rising_edge, torch.Tensor) or tuple(rising_edge.shape) != (E,) or
              rising_edge.dtype != i32 or rising_edge.device != dev or not rising_edge.is_contiguous()):
            raise ValueError(f"rising_edge must be a contiguous ({E},) int32 tensor on {dev}")
        self.rising_edge = rising_edge
        self.contacts = torch.zeros((E, 4, stride), dtype=f32, device=dev)
        self.seeds = torch.empty((E, 4, 3), dtype=f64, device=dev)
        self.ref = torch.empty((E, 24), dtype=f64, device=dev)
        self.lin, self.ang = torch.empty((E, 3), dtype=f64, device=dev), torch.empty((E, 3), dtype=f64, device=dev)
        self.terrain = torch.empty((E, 3), dtype=f64, device=dev)
        self.optimize = torch.empty(E, dtype=i32, device=dev)
        self.action = torch.empty(E, dtype=i32, device=dev)
        # the io struct is built once; a call rewrites the ten input pointers, ref, dt and the stage word
        self._io = _lib.SrbdWbUpdateIo(
            dts=_lib.dptr(self._dts), lens=_lib.iptr(self._lens), n_dts=n, horizon=H, contact_stride=stride,
            lookahead=self.lookahead, max_distance=self.max_distance, com_height_nominal=chn, gravity=grav, ref_z=z,
            lin_out=self.lin.data_ptr(), ang_out=self.ang.data_ptr(), contacts=self.contacts.data_ptr(),
            current_contact=None, previous_contact=self.previous_contact.data_ptr(), seeds=self.seeds.data_ptr(),
            ref=self.ref.data_ptr(), terrain=self.terrain.data_ptr(), optimize=self.optimize.data_ptr(),
            action=self.action.data_ptr())
        self._io_ref = C.byref(self._io)
        self._state_ptrs = (gait.state.data_ptr(), frg.state.data_ptr(), terrain_est.state.data_ptr(),
                            self.current_contact.data_ptr(), self.rising_edge.data_ptr())
        self._inputs = (("com_pos", (E, 3)), ("base_pos", (E, 3)), ("base_lin_vel", (E, 3)), ("euler", (E, 3)),
                        ("base_ang_vel", (E, 3)), ("feet", (E, 4, 3)), ("hips", (E, 4, 3)), ("ref_lin", (E, 3)),
                        ("ref_ang", (E, 3)))
        self._f64 = f64
        self._current_stream = torch.cuda.current_stream
        self._current_device = torch.cuda.current_device
        self._device_guard = torch.cuda.device

    @property
    def contact_rows(self):
        """The two rows ``BatchedLoopReset.reset(..., contact_rows=)`` sets to ones for a reset environment."""
        return (self.current_contact, self.previous_contact)

    def stages(self):
        return ((_lib.WB_VM if self.vm_activated else 0) | (_lib.WB_START_STOP if self.start_and_stop_activated else 0) |
                (_lib.WB_TOUCH_DOWN if self.optimize_step_freq else 0))

    def update_state_and_reference_device(self, com_pos, base_pos, base_lin_vel, base_ori_euler_xyz, base_ang_vel,
                                          feet_pos, hip_pos, simulation_dt, ref_base_lin_vel, ref_base_ang_vel, *,
                                          ref=None, com_pos_offset_w=None, stream=None):
        """One launch on ``stream`` (None: torch's current stream), no host copy and no wait.  The five state vectors
        and the command (E, 3), feet_pos / hip_pos (E, 4, 3): contiguous float64 tensors on the interface's device.
        ``ref`` (E, 24) float64: the reference rows to write (None: the interface's own).  Returns ``(ref, contacts,
        current_contact, previous_contact, seeds, optimize, lin, ang)``: the reference rows, the (E, 4, stride)
        contact sequences, the two contact rows, the foothold seeds (E, 4, 3), the trigger flags (E,) int32 (zeros
        when ``optimize_step_freq`` is off) and the modulated command; all device tensors the interface owns."""
        io, dev, f64 = self._io, self.device, self._f64
        given = (com_pos, base_pos, base_lin_vel, base_ori_euler_xyz, base_ang_vel, feet_pos, hip_pos,
                 ref_base_lin_vel, ref_base_ang_vel)
        for (name, shape), t in zip(self._inputs, given):  # the one pass over dtype, shape, contiguity and device
            try:
                ok = t.dtype == f64 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev
            except AttributeError:
                ok = False
            if not ok:
                raise ValueError(f"{name} must be a contiguous {shape} float64 tensor on {dev}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))} on "
                                 f"{getattr(t, 'device', None)}")
            setattr(io, name, t.data_ptr())
        for name, t, shape in (("ref", ref, (self.num_envs, 24)),
                               ("com_pos_offset_w", com_pos_offset_w, (self.num_envs, 3))):
            if t is not None and not (isinstance(t, type(self.ref)) and t.dtype == f64 and tuple(t.shape) == shape and
                                      t.is_contiguous() and t.device == dev):
                raise ValueError(f"{name} must be a contiguous {shape} float64 tensor on {dev}")
        dt = float(simulation_dt)
        if not math.isfinite(dt):
            raise ValueError(f"simulation_dt must be finite, got {dt}")
        out_ref = self.ref if ref is None else ref
        io.ref = out_ref.data_ptr()
        io.com_pos_offset_w = None if com_pos_offset_w is None else com_pos_offset_w.data_ptr()
        io.dt = dt
        io.stages = self.stages()
        io.max_distance = self.max_distance
        handle = (self._current_stream(dev) if stream is None else stream).cuda_stream
        if self._current_device() != dev.index:
            with self._device_guard(dev):
                rc = _lib.lib.srbd_wb_update_device(*self._state_ptrs, self.num_envs, self._io_ref, handle)
        else:
            rc = _lib.lib.srbd_wb_update_device(*self._state_ptrs, self.num_envs, self._io_ref, handle)
        if rc != _lib.OK:
            raise RuntimeError(f"srbd_wb_update_device failed ({rc})")
        return (out_ref, self.contacts, self.current_contact, self.previous_contact, self.seeds, self.optimize,
                self.lin, self.ang)

    def state_dict(self):
        """The interface's own state (waits for the device): the two contact rows and the trigger words.  The gait
        generator, the foothold generator and the terrain estimator keep theirs."""
        return dict(current_contact=self.current_contact.cpu().numpy().copy(),
                    previous_contact=self.previous_contact.cpu().numpy().copy(),
                    rising_edge=self.rising_edge.cpu().numpy().copy())

    def load_state_dict(self, state):
        import torch

        E = self.num_envs
        for name, shape, dtype in (("current_contact", (E, 4), np.float32), ("previous_contact", (E, 4), np.float32),
                                   ("rising_edge", (E,), np.int32)):
            a = np.ascontiguousarray(state[name], dtype=dtype)
            if a.shape != shape:
                raise ValueError(f"{name} must be {shape}, got {a.shape}")
            getattr(self, name).copy_(torch.from_numpy(a))
