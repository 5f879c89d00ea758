/*
 * srbd_host.h -- C-ABI of the host-side producers and transports around the sampling MPC step
 * (libsrbd_hip.so).  Plain C++ on the host: no device work.
 *
 *   srbd_pgg_init / srbd_pgg_reset   <- PeriodicGaitGenerator.__init__ / reset
 *                                       quadruped_pympc/helpers/periodic_gait_generator.py:8-46
 *   srbd_pgg_run                     <- PeriodicGaitGenerator.run               :48-76
 *   srbd_pgg_set_phase_signal        <- PeriodicGaitGenerator.set_phase_signal  :78-87
 *   srbd_pgg_contact_sequence        <- PeriodicGaitGenerator.compute_contact_sequence :93-118
 *   srbd_pgg_start_stop              <- PeriodicGaitGenerator.update_start_and_stop    :128-196
 *   srbd_prepare_state               <- Sampling_MPC.prepare_state_and_reference
 *                                       quadruped_pympc/controllers/sampling/centroidal_nmpc_jax.py:563-627
 *   srbd_frg_init / _compute / _update_lift_off / _update_touch_down / _mean
 *                                    <- FootholdReferenceGenerator
 *                                       quadruped_pympc/helpers/foothold_reference_generator.py:15-199
 *   srbd_stc_init / _set_timing / _update_swing_time / _reference / _step / _apex / _full_stance
 *                                    <- SwingTrajectoryController and the leg law of
 *                                       WBInterface.compute_stance_and_swing_torque
 *                                       quadruped_pympc/helpers/swing_trajectory_controller.py:5-146
 *                                       quadruped_pympc/interfaces/wb_interface.py:369-415, :435-465
 *   srbd_reflex_init / _detect / _reference / _step
 *                                    <- EarlyStanceDetector and the 'scipy' SwingTrajectoryGenerator, the swing reflex
 *                                       quadruped_pympc/helpers/early_stance_detector.py:7-128
 *                                       quadruped_pympc/helpers/swing_generators/scipy_swing_trajectory_generator.py:8-122
 *                                       quadruped_pympc/interfaces/wb_interface.py:362-365
 *   srbd_stc_touch_down / srbd_gait_apply_freq
 *                                    <- SwingTrajectoryController.check_touch_down_condition and the step-frequency
 *                                       write-back of WBInterface.compute_stance_and_swing_torque
 *                                       quadruped_pympc/helpers/swing_trajectory_controller.py:148-165
 *                                       quadruped_pympc/interfaces/wb_interface.py:354-358
 *   srbd_vfa_init / _mode / _commit / _reset / _height_search
 *                                    <- the apex gate of WBInterface.update_state_and_reference around the foothold
 *                                       search and VisualFootholdAdaptation's state
 *                                       quadruped_pympc/interfaces/wb_interface.py:230-246
 *                                       quadruped_pympc/helpers/visual_foothold_adaptation.py:59-72
 *   srbd_vm_modulate / srbd_terrain_est_init / srbd_terrain_estimate / srbd_reference_assemble
 *                                    <- VelocityModulator, TerrainEstimator and the reference row of
 *                                       WBInterface.update_state_and_reference
 *                                       quadruped_pympc/helpers/velocity_modulator.py:19-46
 *                                       quadruped_pympc/helpers/terrain_estimator.py:5-106
 *                                       quadruped_pympc/interfaces/wb_interface.py:168-172, :250-291
 *   srbd_loop_reset                  <- the episode's end, simulation/simulation.py:773-781, and WBInterface.reset
 *                                       quadruped_pympc/interfaces/wb_interface.py:469-484
 *   srbd_shm_publish / srbd_shm_read <- the MPC -> WBC shared-memory seqlock of ros2/run_controller.py
 *                                       (payload layout :50-83, writer :343-358, reader :565-580)
 *
 * Same conventions as srbd_mpc.h: caller-owned arrays, 0 / negative SRBD_E* codes, no retained
 * pointers.  Arithmetic is float64 in the reference's order (built with -ffp-contract=off).
 */
#ifndef SRBD_HOST_H
#define SRBD_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* quadruped_pympc/helpers/quadruped_utils.py GaitType values */
enum {
    SRBD_GAIT_TROT = 0,
    SRBD_GAIT_PACE = 1,
    SRBD_GAIT_BOUNDING = 2,
    SRBD_GAIT_CIRCULARCRAWL = 3,
    SRBD_GAIT_BFDIAGONALCRAWL = 4,
    SRBD_GAIT_BACKDIAGONALCRAWL = 5,
    SRBD_GAIT_FRONTDIAGONALCRAWL = 6,
    SRBD_GAIT_FULL_STANCE = 7
};

/* Gait generator state (plain data: the caller may copy, inspect or persist it). */
typedef struct srbd_pgg {
    double duty_factor, step_freq;
    double phase_signal[4];
    double phase_offset[4];
    int32_t init[4];
    int32_t gait_type, previous_gait_type, horizon;
} srbd_pgg;

int srbd_pgg_init(srbd_pgg* g, int32_t gait_type, double duty_factor, double step_freq, int32_t horizon);
/* offsets and phase from gait_type, init cleared (periodic_gait_generator.py:22-46) */
int srbd_pgg_reset(srbd_pgg* g);
/* advance every leg by dt * step_freq and return its contact flag (1.0 / 0.0) */
int srbd_pgg_run(srbd_pgg* g, double dt, double step_freq, double contact_out[4]);
/* init == NULL clears the start-up hold */
int srbd_pgg_set_phase_signal(srbd_pgg* g, const double phase[4], const int32_t* init);
/*
 * Look-ahead contact sequence, row-major 4 x cols into out (capacity out_cap doubles); returns cols
 * (horizon, or 2 * horizon of ones for FULL_STANCE, which also resets the generator) or a negative
 * code.  dts[j] holds for steps i < lens[j] (nonuniform sampling); the state is restored afterwards.
 */
int srbd_pgg_contact_sequence(srbd_pgg* g, const double* dts, const int32_t* lens, int32_t n_dts, double* out,
                              int32_t out_cap);
/*
 * update_start_and_stop (periodic_gait_generator.py:128-196; WBInterface.update_state_and_reference calls it at
 * wb_interface.py:175-189 when pgg.start_and_stop_activated), statement for statement (csrc/srbd_start_stop.h, which
 * the device forms srbd_pgg_start_stop_device and srbd_wb_update_device of srbd_mpc.h compile too).
 * Stop condition, all of: norm(ref_lin) == 0.0; norm(ref_ang) == 0.0; norm(base_lin_vel) < 0.1; norm(base_ang_vel) <
 * 0.1; |euler[0]| < 0.05; |euler[1]| < 0.05; the four current contacts sum to 4; and for every leg the horizontal-frame
 * distance of foot and hip < 0.06, where a point's horizontal-frame xy is R_W2H @ (p_xy - base_xy) with cos / sin of
 * euler[2] from csrc/yaw_sincos.h (each row two products summed left to right), the foot's y then shifted by
 * hip_offset (- for FL and RL, + for FR and RR), and the distance sqrt(dx dx + dy dy).  A norm is sqrt((x x + y y) +
 * z z): a command whose squares underflow counts as zero, as in NumPy.  A NaN anywhere makes the condition false.
 *   condition holds          gait_type = SRBD_GAIT_FULL_STANCE, then srbd_pgg_reset's assignments; on every such call,
 *                            as the reference; previous_gait_type is left alone.  Returns 1.
 *   else, in FULL_STANCE     gait_type = previous_gait_type, then srbd_pgg_reset's assignments.  Returns 2.
 *   otherwise                nothing is written.  Returns 0.
 * feet and hips are 4 x 3 (z unused); ref_lin / ref_ang are the (modulated) command.  The reference's mean of the
 * four distances is never read and is not formed.  The comparisons agree with the reference's wherever the compared
 * quantity is further from its threshold than the rounding of cos / sin and of the sums.
 * SRBD_E_INVALID (nothing written): a NULL pointer.
 */
int srbd_pgg_start_stop(srbd_pgg* g, const double* feet /* 4 x 3 */, const double* hips /* 4 x 3 */, double hip_offset,
                        const double base_pos[3], const double euler[3], const double base_lin_vel[3],
                        const double base_ang_vel[3], const double ref_lin[3], const double ref_ang[3],
                        const double current_contact[4]);

/*
 * prepare_state_and_reference: state_in = [position, linear_velocity, orientation, angular_velocity,
 * foot_FL, foot_FR, foot_RL, foot_RR] (24), ref_in = [ref_position, ref_linear_velocity,
 * ref_orientation, ref_angular_velocity, ref_foot_FL..RR] (24).  Swing feet (current_contact == 0)
 * take the reference foot; a leg lifting off (previous 1 -> current 0) zeroes its params_per_leg
 * entries of best_params (in/out, 4 * params_per_leg floats; may be NULL).
 */
int srbd_prepare_state(const double state_in[24], const double ref_in[24], const double current_contact[4],
                       const double previous_contact[4], int32_t params_per_leg, float* best_params,
                       double state_out[24], double ref_out[24]);

/* ---- Foothold reference generator: the seeds of the foothold adaptation, and on flat ground the reference's feet
 * directly (quadruped_pympc/helpers/foothold_reference_generator.py, run by WBInterface.update_state_and_reference
 * every step between the gait generator and the foothold adaptation, wb_interface.py:202-227).
 *   srbd_frg_init              <- FootholdReferenceGenerator.__init__                     :15-51
 *   srbd_frg_compute           <- FootholdReferenceGenerator.compute_footholds_reference  :53-157
 *   srbd_frg_update_lift_off   <- FootholdReferenceGenerator.update_lift_off_positions    :159-178
 *   srbd_frg_update_touch_down <- FootholdReferenceGenerator.update_touch_down_positions  :180-199
 * State (plain data: the caller may copy, inspect or persist it; sizeof is a multiple of 8, so an array of them in
 * device memory keeps every double aligned).  Legs FL FR RL RR, positions xyz.  vel_hist is the reference's
 * deque(maxlen = 20) of horizontal-frame base velocities as a ring: hist_len entries are held; hist_head is the slot
 * the next entry goes to -- equal to hist_len while the ring fills (the oldest entry is slot 0), the oldest entry
 * once it is full. */
#define SRBD_FRG_HIST 20
typedef struct srbd_frg {
    double stance_time, hip_height;
    double hip_offset;                       /* 0.1 (:44); y offset of the nominal foothold from the hip */
    double lift_off[4][3], lift_off_h[4][3]; /* world frame, and the horizontal frame of the lift-off instant */
    double touch_down[4][3], touch_down_h[4][3];
    double last_reference_footholds[4][3];   /* the last srbd_frg_compute result */
    double vel_hist[SRBD_FRG_HIST][2];
    int32_t hist_len, hist_head;             /* two words: no further padding is needed */
} srbd_frg;

/* All four position tables start as copies of lift_off (4 x 3), the _h tables too (the reference's "TODO wrong" is
 * reproduced); the history starts empty and last_reference_footholds at zero.  SRBD_E_INVALID: a NULL pointer, a
 * stance_time or hip_height that is not finite. */
int srbd_frg_init(srbd_frg* g, double stance_time, double hip_height, const double* lift_off /* 4 x 3 */);
/* The lift-off and touch-down bookkeeping.  Contacts are doubles compared with == 1 and == 0 as the reference compares
 * them; full_stance != 0 is the reference's gait_type == FULL_STANCE branch (every leg takes its foot, the _h tables
 * are left alone).  Otherwise a leg lifting off (1 -> 0) takes its foot and stores it in the horizontal frame,
 * R_W2H @ (foot - base_pos); a leg in swing (0 -> 0) is carried with the base, R_W2H.T @ lift_off_h + base_pos.  Touch
 * down is the same with 0 -> 1 and 1 -> 1.  R_W2H is the 3 x 3 yaw rotation, written out element by element:
 * (c x + s y, -s x + c y, z), transposed (c x + (-s) y, s x + c y, z).  feet is 4 x 3. */
int srbd_frg_update_lift_off(srbd_frg* g, const double previous_contact[4], const double current_contact[4],
                             const double* feet, int32_t full_stance, const double base_pos[3], double yaw);
int srbd_frg_update_touch_down(srbd_frg* g, const double previous_contact[4], const double current_contact[4],
                               const double* feet, int32_t full_stance, const double base_pos[3], double yaw);
/* The Raibert-style reference footholds, in the reference's order: both velocities rotated into the horizontal
 * frame; the base velocity pushed into the ring and the mean of what the ring holds taken (the sum starts from the
 * oldest entry, adds oldest to newest and is divided by the count, as np.mean of the deque's rows: an all -0.0
 * history has a -0.0 mean); delta = clip((stance_time / 2) * ref_vel_H, -1.5 hip_height, 1.5 hip_height); err =
 * sqrt(com_height_nominal / gravity) * (mean - ref_vel_H) limited to +-0.05 (a NaN passes); per leg R_W2H @ (hip_xy -
 * base_xy), y +- hip_offset (+ FL RL, - FR RR), + (delta + err), R_W2H.T @ ... + base_xy, + com_pos_offset_w[0:2],
 * z = lift_off[leg][2].  out (4 x 3) receives the footholds, and so does last_reference_footholds.
 *   com_pos_offset_w: 3 doubles, or NULL for the reference's zero offset (the additions of +0.0 still happen).  The
 *   reference forms it as Rotation.from_euler('xyz', rpy) @ com_pos_offset_b, and the body offset is zero unless set
 *   by hand from the ROS console: that rotation is the caller's, this call takes only the world offset.
 * cos and sin of the yaw are the correctly rounded values in all three functions (csrc/yaw_sincos.h;
 * srbd_selftest_yaw_sincos shows them): the same bits as the device form, srbd_frg_step_device (srbd_mpc.h); libm's
 * differ from them in the last place for about 3 in 1000 yaws.
 * SRBD_E_INVALID: a NULL pointer (com_pos_offset_w excepted).  Nothing else is refused: NaN inputs flow through as in
 * NumPy. */
int srbd_frg_compute(srbd_frg* g, const double base_pos[3], double yaw, const double base_xy_vel[2],
                     const double ref_xy_vel[2], const double* hips /* 4 x 3 */, double com_height_nominal,
                     double gravity, const double* com_pos_offset_w /* 3, or NULL */, double* out /* 4 x 3 */);
/* The moving average srbd_frg_compute uses: the mean of what the ring holds, summed oldest to newest from the oldest
 * entry (not from zero) and divided by the count; NaN for an empty ring.  For inspection and tests. */
int srbd_frg_mean(const srbd_frg* g, double mean_out[2]);

/* ---- Stance and swing leg controller: the joint torques of one control step from the MPC's ground-reaction forces,
 * the last stage of the reference's step (WBInterface.compute_stance_and_swing_torque, quadruped_pympc/interfaces/
 * wb_interface.py:304-467, with SwingTrajectoryController, quadruped_pympc/helpers/swing_trajectory_controller.py).
 *   srbd_stc_init              <- SwingTrajectoryController.__init__                              :5-33
 *   srbd_stc_set_timing        <- SwingTrajectoryController.regenerate_swing_trajectory_generator :35-46
 *   srbd_stc_update_swing_time <- SwingTrajectoryController.update_swing_time                     :120-127
 *   srbd_stc_reference         <- SwingTrajectoryGenerator.compute_trajectory_references of
 *                                 swing_generators/bezier_ref_swing_trajectory_generator.py:222-265 ('bezier_ref', the
 *                                 reference's default) and explicit_swing_trajectory_generator.py:57-113 ('explicit')
 *   srbd_stc_step              <- wb_interface.py:369-415 and :435-465 with compute_swing_control_cartesian_space :48-94
 *   srbd_stc_apex              <- SwingTrajectoryController.check_apex_condition                  :129-138
 *   srbd_stc_full_stance       <- SwingTrajectoryController.check_full_stance_condition           :140-146
 * State (plain data, sizeof 80: the caller may copy, inspect or persist it, and an array of them in device memory
 * keeps every double aligned).  Legs FL FR RL RR.  The arithmetic is float64 in the fixed order csrc/srbd_stc.h writes
 * out, which the device form (srbd_stc_step_device, srbd_mpc.h) compiles too; integer powers are repeated
 * multiplication where the reference's `**` calls pow, so values agree with the reference to rounding, not to the bit.
 * Deviation: the reference inverts the leg Jacobian with np.linalg.pinv (an SVD); here Jinv is the 3 x 3 inverse by
 * cofactors over the determinant.  For a well-conditioned Jacobian the two agree to rounding.  For a singular one they
 * do not: when the determinant is zero or not finite Jinv is the zero matrix, so every output stays finite and the
 * feedback-linearisation term reduces to the bias force.
 * Not in these calls: the early-stance detector and the 'scipy' generator, the one generator that reads the detector's
 * hit moment and hit point, have entry points of their own, below (srbd_reflex_*).  Out of scope: inverse kinematics and
 * des_joints_pos, and the kinodynamic branch.  The re-timing from optimize_swing /
 * best_sample_freq (wb_interface.py:354-358) is not part of srbd_stc_step: srbd_stc_touch_down and srbd_gait_apply_freq
 * below are its trigger and its write-back (srbd_stc_set_timing is the call it would make for the swing period). */
enum { SRBD_SWING_BEZIER_REF = 0, SRBD_SWING_EXPLICIT = 1 };
typedef struct srbd_stc {
    double step_height, swing_period, position_gain_fb, velocity_gain_fb;
    int32_t generator;                  /* SRBD_SWING_BEZIER_REF, SRBD_SWING_EXPLICIT */
    int32_t use_feedback_linearization; /* 1 after init */
    int32_t use_friction_compensation;  /* 1 after init */
    int32_t reserved;                   /* 0: the fourth word, so that no padding is left to chance */
    double swing_time[4];               /* the per-leg swing clocks */
} srbd_stc;

/* One environment's step.  Matrices are 4 x 3 x 3 row-major, already sliced to the leg's own three joint columns;
 * vectors are 4 x 3. */
typedef struct srbd_stc_io {
    /* inputs */
    const double *jac, *jac_dot, *mass_matrix;                 /* 4 x 3 x 3 */
    const double *q_dot, *foot_pos, *foot_vel;                 /* 4 x 3 */
    const double *qfrc_passive, *qfrc_bias, *grfs;             /* 4 x 3 */
    const double *lift_off, *touch_down;                       /* 4 x 3 */
    const double* contact;                                     /* 4: a leg is in swing iff its flag == 0 */
    double apex_interval;
    /* outputs */
    double *tau, *des_foot_pos, *des_foot_vel;                 /* 4 x 3 */
    double* des_joint_vel;                                     /* 4 x 3, or NULL */
    int32_t *apex, *full_stance;                               /* one word each, or NULL */
} srbd_stc_io;

/* Clocks at zero, both switches on.  SRBD_E_INVALID (nothing written): a NULL g, a swing_period that is not positive
 * or not finite, an unknown generator. */
int srbd_stc_init(srbd_stc* g, double step_height, double swing_period, double position_gain_fb,
                  double velocity_gain_fb, int32_t generator);
/* regenerate_swing_trajectory_generator: the new step height and swing period; the clocks are left alone.
 * SRBD_E_INVALID as srbd_stc_init. */
int srbd_stc_set_timing(srbd_stc* g, double step_height, double swing_period);
/* A swing leg (contact == 0) whose clock is below swing_period advances by dt (so a clock passes swing_period by
 * less than dt and then holds); a stance leg's clock is zero.  SRBD_E_INVALID: NULL, a dt that is not finite. */
int srbd_stc_update_swing_time(srbd_stc* g, const double contact[4], double dt);
/* The generator alone at leg's current clock: desired foot position, velocity and acceleration (3 each).
 *   bezier_ref: s = clip(swing_time / swing_period, 0, 1); the degree-6 Bezier with control points P0 = P1 = P2 =
 *   lift_off, P4 = P5 = P6 = touch_down, P3 = (mid_x, mid_y, (64 z_mid - 22 z0 - 22 zf) / 20), z_mid = max(z0, zf) +
 *   step_height; velocity / swing_period, acceleration / swing_period^2.
 *   explicit, with the reference's quirks: two cubic Beziers split at half = swing_period / 2 by swing_time <= half,
 *   local time fmod(swing_time, half) / half -- so swing_time == half evaluates the first curve at its start, and a
 *   clock past swing_period wraps to the start of the second curve; the apex control points sit at the absolute
 *   height step_height; velocity and acceleration are not rescaled to time.
 * SRBD_E_INVALID: NULL, leg outside 0..3, a struct srbd_stc_init would refuse. */
int srbd_stc_reference(const srbd_stc* g, int32_t leg, const double lift_off[3], const double touch_down[3],
                       double pos[3], double vel[3], double acc[3]);
/* The whole step of one environment, in this order: the clock update (srbd_stc_update_swing_time); then per leg
 *   stance (contact != 0): tau = -(J.T @ grf), des_foot_pos = touch_down, des_foot_vel = 0;
 *   swing (contact == 0): e_p = des_pos - foot_pos, e_v = des_vel - foot_vel, fb = kp e_p + kd e_v, tau = J.T @ fb,
 *     and with use_feedback_linearization tau += ((M @ Jinv) @ ((des_acc + fb) - J_dot @ q_dot)) + h;
 *   des_joint_vel = q_dot + clip(Jinv @ des_foot_vel - q_dot, -10, 10) (wb_interface.py:435-465);
 * then, with use_friction_compensation, tau -= qfrc_passive for every leg, stance or swing; then apex and full_stance
 * from the clocks as this call leaves them -- what the next step's update_state_and_reference would see.
 * SRBD_E_INVALID (nothing written): a NULL g, io or required pointer; a struct srbd_stc_init would refuse; a dt or
 * apex_interval that is not finite.  NaN inputs flow through as in NumPy. */
int srbd_stc_step(srbd_stc* g, const srbd_stc_io* io, double dt);
/* 1 if a swing leg's clock lies strictly inside swing_period / 2 +- interval (the reference's two comparisons),
 * else 0; negative: NULL, or an interval that is not finite. */
int srbd_stc_apex(const srbd_stc* g, const double contact[4], double interval);
/* 1 if no contact equals 0, else 0; negative: NULL. */
int srbd_stc_full_stance(const double contact[4]);

/* ---- Swing reflexes: the early-stance detector and the 'scipy' swing generator, the reflex path of the leg controller
 * (csrc/srbd_reflex.h, which the device form srbd_reflex_step_device of srbd_mpc.h compiles too).
 *   srbd_reflex_init      <- EarlyStanceDetector.__init__          quadruped_pympc/helpers/early_stance_detector.py:7-33
 *                            and the reflex fields of the scipy SwingTrajectoryGenerator.__init__
 *                            quadruped_pympc/helpers/swing_generators/scipy_swing_trajectory_generator.py:8-23
 *   srbd_reflex_detect    <- EarlyStanceDetector.update_detection  early_stance_detector.py:36-128
 *   srbd_reflex_reference <- SwingTrajectoryGenerator.createCurve / compute_trajectory_references
 *                            scipy_swing_trajectory_generator.py:25-122
 *   srbd_reflex_step      <- wb_interface.py:362-415 and :435-465 with SwingTrajectoryController(generator="scipy")
 * State: one srbd_reflex per environment (plain data, sizeof 320, doubles first, no byte of padding), next to that
 * environment's srbd_stc, which is reused unchanged for the gains, step height, swing period, switches and clocks; its
 * `generator` field is not read by these calls.  Legs FL FR RL RR.
 * The detector, statement for statement (trigger_mode SRBD_REFLEX_TRACKING, the reference's configuration; with
 * SRBD_REFLEX_OFF every leg is cleared each tick).  Leg by leg: a stance leg (contact == 1) only clears early_stance --
 * its hit moment and hit point stay until its next swing tick; a leg that has not triggered and whose clock is inside
 * the last early_stance_time_threshold (0.07 s) of the swing is skipped; a leg that has triggered keeps its hit for the
 * rest of the swing; otherwise local = last_des_foot_pos - foot, disp = touch_down - lift_off and the leg triggers when
 * norm(local) / norm(disp) > 0.3 and norm(local) > 0.1 (IEEE: a zero disp gives inf or NaN, compared as NumPy compares
 * them; norm = sqrt((x x + y y) + z z)): hitpoint = foot, hitmoment = the clock, early_stance = 1, the gait-cycle
 * counter = 0, and the tick ends there -- the legs after the first that triggers are not touched at all.  A leg that
 * does not trigger is cleared (hitmoment -1, no hitpoint).  Then, only with the enhancement switched on: at most one
 * touch-down edge (contact == 1 and previous_contact == 0) increments the counter, and only while it is >= 0; the flag
 * height_enhancement is 0 <= gait_cycles < max_gait_cycles (6), otherwise the counter returns to -1.
 * The generator: five knots per axis and scipy's CubicSpline(bc_type=["clamped", "clamped"]) through them, solved as
 * the 3 x 3 tridiagonal system of the interior knot derivatives by elimination in the fixed order csrc/srbd_reflex.h
 * writes out.  The contract is agreement with scipy to rounding, not to the bit; as an observation, on the recorded
 * fixture (scipy 1.15.3) the spline's values did come out equal bit for bit, because LAPACK's tridiagonal solve makes
 * no row exchange on these systems and then performs the same elimination.  Without a hit the knots are lift_off, the three
 * step_height / 1.5 way-points and touch_down over t = 0, T/4, T/2, 3T/4, T (reflex_max_step_height in step_height's
 * place while height_enhancement is set); with a hit the curve starts at the hit point, is pushed back by 0.01 (xf - x0),
 * rises to reflex_max_step_height, ends x and y at its fourth knot and z at touch_down's (plus
 * reflex_max_step_height / 2 when blind), over the hit moment to T in quarters.  Intervals are half-open, the last one
 * closed, and the end intervals extrapolate.
 * Deviation: with a hit recorded and swing_period - hitmoment not positive (only after a re-timing shortened the
 * swing) the knots are not increasing and scipy raises; here that leg takes the no-hit curve from lift_off for that
 * tick and its detector state is left alone.  The Jacobian inverse is srbd_stc_step's.
 * Out of scope: the 'geom_contact' trigger (SRBD_REFLEX_GEOM_CONTACT is refused: it reads MuJoCo contact lists),
 * inverse kinematics and des_joints_pos, the kinodynamic branch. */
enum { SRBD_REFLEX_OFF = 0, SRBD_REFLEX_TRACKING = 1, SRBD_REFLEX_GEOM_CONTACT = 2 /* refused */ };
typedef struct srbd_reflex {
    double reflex_max_step_height;
    double early_stance_time_threshold;           /* 0.07 after init */
    double relative_tracking_error_threshold;     /* 0.3 */
    double absolute_min_distance_error_threshold; /* 0.1 */
    double hitmoments[4];                         /* the clock at the hit, or -1 */
    double hitpoints[4][3];                       /* the foot at the hit; zeros while has_hitpoint is 0 */
    double last_des_foot_pos[4][3];               /* the desired foot positions the previous step wrote; zeros at init */
    int32_t has_hitpoint[4];                      /* 0: the reference's None */
    int32_t early_stance[4];
    int32_t trigger_mode;                         /* SRBD_REFLEX_OFF, SRBD_REFLEX_TRACKING */
    int32_t blind;                                /* visual_foothold_adaptation == 'blind' */
    int32_t use_height_enhancement;               /* reflex_next_steps_height_enhancement, the switch */
    int32_t height_enhancement;                   /* the generator's flag as the last detection left it */
    int32_t gait_cycles;                          /* gait cycles since the last reflex, -1 at init */
    int32_t max_gait_cycles;                      /* 6 after init */
    int32_t reserved[2];                          /* 0: so that no padding is left to chance */
} srbd_reflex;

/* The reference's values: the thresholds 0.07, 0.3 and 0.1, six cycles, no hit, counter -1, flag 0, last_des_foot_pos
 * zero.  SRBD_E_INVALID (nothing written): a NULL r, a reflex_max_step_height that is not finite, a trigger_mode other
 * than SRBD_REFLEX_OFF and SRBD_REFLEX_TRACKING. */
int srbd_reflex_init(srbd_reflex* r, double reflex_max_step_height, int32_t blind, int32_t trigger_mode,
                     int32_t use_height_enhancement);
/* update_detection alone.  swing_time are the clocks the previous step left (4), feet the feet now, lift_off and
 * touch_down 4 x 3, contact and previous_contact 4; the desired foot positions are r->last_des_foot_pos.
 * SRBD_E_INVALID (nothing written): a NULL pointer, a struct srbd_reflex_init would refuse. */
int srbd_reflex_detect(srbd_reflex* r, const double* feet, const double* lift_off, const double* touch_down,
                       const double swing_time[4], double swing_period, const double contact[4],
                       const double previous_contact[4]);
/* The generator alone for one leg at that leg's clock g->swing_time[leg], with the leg's hit and the flag as r holds
 * them.  SRBD_E_INVALID: NULL, leg outside 0..3, structs srbd_reflex_step would refuse. */
int srbd_reflex_reference(const srbd_stc* g, const srbd_reflex* r, int32_t leg, const double lift_off[3],
                          const double touch_down[3], double pos[3], double vel[3], double acc[3]);
/* One environment's whole step, in this order: the detector (on the clocks and r->last_des_foot_pos the previous step
 * left, io->foot_pos, io->lift_off, io->touch_down, io->contact and previous_contact); the clock update; srbd_stc_step's
 * leg law with the spline generator in the place of the Bezier ones; io->des_foot_pos into r->last_des_foot_pos; apex
 * and full stance.  SRBD_E_INVALID (nothing written): what srbd_stc_step refuses (the generator code of g excepted: it
 * is not read), a NULL r or previous_contact, an unknown or refused trigger mode, a reflex_max_step_height that is not
 * finite. */
int srbd_reflex_step(srbd_stc* g, srbd_reflex* r, const srbd_stc_io* io, const double previous_contact[4], double dt);

/* ---- Gait adaptation (mpc_params['optimize_step_freq']): when to optimise the step frequency, and what the sampler's
 * best frequency re-times (csrc/srbd_gait_adapt.h, which the device forms srbd_stc_touch_down_device and
 * srbd_gait_apply_freq_device of srbd_mpc.h compile too).
 *   srbd_stc_touch_down   <- SwingTrajectoryController.check_touch_down_condition
 *                            quadruped_pympc/helpers/swing_trajectory_controller.py:148-165 (called wb_interface.py:298)
 *   srbd_gait_apply_freq  <- WBInterface.compute_stance_and_swing_torque, quadruped_pympc/interfaces/wb_interface.py:354-358
 * srbd_stc_touch_down, statement for statement: *rising_edge (the reference's rising_edge_detected, caller-owned, 0
 * at start) is set when all four current_contact == 1 and not all four previous_contact == 1; stable = every entry of
 * columns 0..lookahead-1 of the 4 x horizon contact sequence (row l at contact_sequence + l * contact_stride) == 1;
 * next_lift = not every entry of column `lookahead` == 1; when the edge is set, stable and next_lift all hold the edge
 * is cleared and 1 returned, else 0.  The comparisons are `== 1` as in the reference (a contact of 2.0 or NaN is not
 * stance).  SRBD_E_INVALID (nothing written): a NULL pointer, contact_stride < horizon, lookahead outside
 * 1..horizon-1 (where the reference raises IndexError; its default is 3).
 * srbd_gait_apply_freq: with optimize != 1 nothing is written and 0 is returned.  Otherwise pgg->step_freq =
 * best_freq, frg->stance_time = (1 / f) * duty and stc->swing_period = (1 - duty) * (1 / f) with duty =
 * pgg->duty_factor, stc->step_height unchanged, and 1 is returned.  best_freq is the float32 scalar the sampler
 * returns, and the two products are float32 products as the reference forms them under NumPy 2 (NEP 50: Python scalars
 * do not widen a float32): inv = 1.0f / f, stance = inv * (float)duty, swing = (float)(1.0 - duty) * inv, each widened
 * exactly to the struct's double -- the recorded reference values bit for bit.  frg and stc may each be NULL.  A
 * best_freq that is zero, negative or not finite, or a duty factor that leaves a swing period srbd_stc_set_timing
 * refuses, leaves all three structs untouched and returns 0 (the reference would divide and store the result).
 * SRBD_E_INVALID: a NULL pgg.  Deviation: see csrc/srbd_gait_adapt.h on the reference's float32 phase increment after
 * its first write-back; srbd_pgg_run is unchanged. */
int srbd_stc_touch_down(int32_t* rising_edge, const double current_contact[4], const double previous_contact[4],
                        const double* contact_sequence /* 4 x contact_stride */, int32_t contact_stride,
                        int32_t horizon, int32_t lookahead);
int srbd_gait_apply_freq(srbd_pgg* pgg, srbd_frg* frg /* or NULL */, srbd_stc* stc /* or NULL */, int32_t optimize,
                         float best_freq);

/* ---- Apex-gated foothold adaptation: the state machine WBInterface.update_state_and_reference keeps around the
 * foothold search (csrc/srbd_vfa.h, which the device form srbd_vfa_step_device of srbd_mpc.h compiles too).
 *   srbd_vfa_init / srbd_vfa_reset <- VisualFootholdAdaptation.__init__ / reset
 *                                     quadruped_pympc/helpers/visual_foothold_adaptation.py:38-46, :63-64
 *   srbd_vfa_mode                  <- the two conditions of quadruped_pympc/interfaces/wb_interface.py:232 and :243
 *   srbd_vfa_commit                <- update_footholds_adaptation :59-61, reset :63-64, get_footholds_adapted :66-72,
 *                                     and what compute_adaptation :193-228 stores per leg
 * The reference, per control step (wb_interface.py:230-246):
 *   if stc.check_apex_condition(contact, 0.01) and not vfa.initialized:  search; footholds_adaptation = result;
 *                                                                        initialized = True
 *   if stc.check_full_stance_condition(contact):                         initialized = False
 *   not initialized: footholds_adaptation = seeds, return the seeds;  initialized: return footholds_adaptation
 * so it searches once per swing, at the apex, holds that result until the next full stance, and passes the seeds
 * through from there until the next apex.  Three modes name the three paths:
 *   SRBD_VFA_SEARCH  apex and not initialized
 *   SRBD_VFA_HOLD    initialized and not full stance
 *   SRBD_VFA_PASS    everything else (not initialized without an apex; or full stance, which resets)
 * An apex needs a leg in swing and full stance needs none, so a search and the reset never fall on one step.  Both
 * conditions are srbd_stc_apex's and srbd_stc_full_stance's, on the swing clocks as the last leg-controller step left
 * them: the reference checks the apex before this step's update_swing_time.
 * State (plain data, sizeof 320, no padding: four words, 36 doubles, four words; the caller may copy, inspect or
 * persist it, and an array of them in device memory keeps every double aligned).  Legs FL FR RL RR.
 *   initialized  the reference's `initialized`, one word per leg, always all four equal: replicated so that the
 *                device kernel's block (leg, environment) reads and writes only its own word
 *   footholds    the reference's footholds_adaptation
 *   boxes        the reference's footholds_constraints, two vertices per leg; NaN where the reference holds None
 *   valid        whether the leg's last search found a candidate
 * Stale constraint: a search that finds no candidate for a leg leaves that leg's box as it was (the reference assigns
 * footholds_constraints only for a feasible leg, :209-228), so the box returned with valid 0 is the last feasible
 * search's, or NaN if there was none.  Neither the reset nor a pass-through touches boxes or valid.
 * Out of scope: the 'vfa' strategy, the early-stance detector and inverse kinematics (start-and-stop
 * is the gait generator's, srbd_pgg_start_stop above, and does not touch this state;
 * the per-environment masked reset of this and the loop's other state is srbd_loop_reset, below). */
enum { SRBD_VFA_PASS = 0, SRBD_VFA_SEARCH = 1, SRBD_VFA_HOLD = 2 };
typedef struct srbd_vfa {
    int32_t initialized[4]; /* 0 / 1, all four equal (16 bytes: the doubles behind them stay aligned) */
    double footholds[12];   /* 4 x 3 */
    double boxes[24];       /* 4 x 2 x 3 */
    int32_t valid[4];       /* the struct ends on a multiple of 8 */
} srbd_vfa;

/* Not initialized, zero footholds, NaN boxes, valid 0.  SRBD_E_INVALID: NULL. */
int srbd_vfa_init(srbd_vfa* g);
/* The reference's reset(): initialized = 0, nothing else.  SRBD_E_INVALID: NULL. */
int srbd_vfa_reset(srbd_vfa* g);
/* *mode = the step's mode from g->initialized, the clocks of stc and the contact flags (a leg is in swing iff its
 * flag == 0).  Nothing is written to g.  SRBD_E_INVALID (nothing written): a NULL pointer, an apex_interval that is
 * not finite, a g whose four initialized words differ. */
int srbd_vfa_mode(const srbd_vfa* g, const srbd_stc* stc, const double contact[4], double apex_interval,
                  int32_t* mode);
/* The step's state update and what get_footholds_adapted returns, per leg:
 *   SEARCH  footholds = searched_footholds; boxes = searched_boxes only where searched_valid (see above); valid =
 *           searched_valid; initialized = 1
 *   HOLD    nothing is stored
 *   PASS    footholds = seeds; initialized = 0; boxes and valid are left alone
 * and in all three out_footholds / out_boxes / out_valid are the state's after that.  The three searched_ pointers may
 * be NULL unless mode is SEARCH.  SRBD_E_INVALID (nothing written): a NULL required pointer, an unknown mode, a g
 * whose four initialized words differ. */
int srbd_vfa_commit(srbd_vfa* g, int32_t mode, const double seeds[12], const double searched_footholds[12],
                    const double searched_boxes[24], const int32_t searched_valid[4], double out_footholds[12],
                    double out_boxes[24], int32_t out_valid[4]);
/* The 'height' strategy's search of one leg (visual_foothold_adaptation.py:145-151 with HeightMap.get_height): patch
 * is the leg's rows x cols x 3 points (x, y, z), seed its reference foothold.  idx = the point with the smallest
 * (x - seed[0]) * (x - seed[0]) + (y - seed[1]) * (y - seed[1]) (float64, unfused) under numpy.argmin's rule: the
 * first minimum wins, and a NaN distance wins at its first occurrence.  foothold = (seed[0], seed[1], z[idx] + 0.02);
 * *valid = 0 when that z is NaN (a ray that missed on a scene whose miss_z is NaN), else 1.  The strategy has no
 * foothold constraints: the searched boxes handed to srbd_vfa_commit with this result are NaN.  csrc/srbd_vfa.h
 * states the search once for this function and for the kernel of srbd_vfa_height_step_device (srbd_mpc.h).
 * SRBD_E_INVALID (nothing written): a NULL pointer, rows or cols below 1, rows * cols above 320. */
int srbd_vfa_height_search(const double* patch, int32_t rows, int32_t cols, const double seed[3], double foothold[3],
                           int32_t* valid);

/* ---- Velocity modulator, terrain estimator and the reference row's first twelve entries: what
 * WBInterface.update_state_and_reference builds every control step from the velocity command, before and after the
 * foothold reference generator (quadruped_pympc/interfaces/wb_interface.py:168-172 and :250-291).
 *   srbd_vm_modulate        <- VelocityModulator.modulate_velocities   quadruped_pympc/helpers/velocity_modulator.py:19-46
 *   srbd_terrain_est_init   <- TerrainEstimator.__init__               quadruped_pympc/helpers/terrain_estimator.py:5-11
 *   srbd_terrain_estimate   <- TerrainEstimator.compute_terrain_estimation                                  :13-106
 *   srbd_reference_assemble <- wb_interface.py:258-291: ref_position, the command rotated into the terrain frame with
 *                              its two pitch quirks, ref_orientation, ref_angular_velocity
 * The struct is named srbd_terrain_est because srbd_terrain is the ray-cast terrain handle of srbd_mpc.h.
 * State (plain data, sizeof 32: the caller may copy, inspect or persist it, and an array of them in device memory keeps
 * every double aligned).  The arithmetic is float64 in the fixed order csrc/srbd_terrain.h writes out, which the device
 * forms (srbd_vm_modulate_device, srbd_terrain_ref_step_device, srbd_mpc.h) compile too.  The modulator and the height
 * filter are IEEE operations only and equal the reference bit for bit.  Roll, pitch and the rotated command agree with
 * the reference to rounding: cos / sin are the correctly rounded values of csrc/yaw_sincos.h, the arctangent is the
 * header's own (within 1 ulp of the true value; srbd_selftest_atan shows it), the yaw rotation is written out where the
 * reference calls a BLAS product, and the terrain rotation is Ry(pitch) Rx(roll) written out where the reference goes
 * through scipy's quaternion.
 * Out of scope: the early-stance detector, inverse kinematics and the kinodynamic branch.  update_start_and_stop,
 * which the reference runs between the modulator and the gait generator, is srbd_pgg_start_stop above. */
typedef struct srbd_terrain_est {
    double roll, pitch, height;               /* the three filtered values, 0 after init */
    int32_t roll_activated, pitch_activated;  /* 0 and 1 after init; a switched-off angle is set to 0.0 every step */
} srbd_terrain_est;

/* If lin[0] < 0.01 and lin[1] < 0.01 (no abs: a negative command counts as standing, a NaN as moving) the command is
 * returned as it is.  Otherwise, if sqrt(square(dx) + square(dy)) of foot minus hip is strictly above max_distance
 * for any leg, lin_out = lin * 0.0 and ang_out = ang * 0.0 -- products, so a negative entry becomes -0.0 and a NaN
 * stays; a NaN distance fails the comparison.  The reference's max_distance is 0.2 for every robot.  feet and hips
 * are 4 x 3 (z unused).  SRBD_E_INVALID: a NULL pointer.  Nothing else is refused. */
int srbd_vm_modulate(double max_distance, const double lin[3], const double ang[3], const double* feet /* 4 x 3 */,
                     const double* hips /* 4 x 3 */, double lin_out[3], double ang_out[3]);
/* roll = pitch = height = 0, roll_activated = 0, pitch_activated = 1.  SRBD_E_INVALID: NULL. */
int srbd_terrain_est_init(srbd_terrain_est* g);
/* One step of the estimator.  feet (4 x 3, FL FR RL RR) are the positions the reference passes: the foothold
 * generator's lift-off table.  The four R_W2H @ (foot - base_pos) are formed first (each row's products summed left to
 * right, the zero products included, so a NaN coordinate spreads as in NumPy), then front = FL - FR, back = RL - RR,
 * left = FL - RL, right = FR - RR; pitch = (arctan(|left z| / |left x + 0.001|) + arctan(|right z| / |right x +
 * 0.001|)) * 0.5, roll the same from front and back over y; roll is negated if front z * 0.5 + back z * 0.5 < 0, pitch
 * if left z * 0.5 + right z * 0.5 > 0; the filters are value * 0.99 + new * 0.01 for an activated angle (0.0 for one
 * switched off) and height * 0.2 + ((z0 + z1 + z2 + z3) / 4) * 0.8.  A zero denominator gives inf and the angle pi / 2;
 * 0 / 0 gives NaN, which stays in the filter.  The reference's current_contact argument is unused there and absent
 * here.  out (3, or NULL) receives roll, pitch, height.  SRBD_E_INVALID: a NULL g, base_pos or feet. */
int srbd_terrain_estimate(srbd_terrain_est* g, const double base_pos[3], double yaw, const double* feet /* 4 x 3 */,
                          double out[3]);
/* Entries 0..11 of the 24-entry reference row srbd_prepare_state reads, from the estimator's state and the (modulated)
 * command: ref_position = (0, 0, (ref_z + height) - (base_z - (com_z + com_off_z))); ref_linear_velocity = R @ lin with
 * R = [[cp, sp sr, sp cr], [0, cr, -sr], [-sp, cp sr, cp cr]], each row summed left to right, then z negated if pitch >
 * 0, then x / 2 and z * 2 if |pitch| > 0.2; ref_orientation = (roll, pitch, 0.0); ref_angular_velocity = ang.
 * SRBD_E_INVALID: a NULL pointer.  NaN inputs flow through. */
int srbd_reference_assemble(const srbd_terrain_est* g, double ref_z, double base_z, double com_z, double com_off_z,
                            const double lin[3], const double ang[3], double ref_out[12]);
/* Self-test: out[i] = the arctangent both sides use, of x[i] >= 0 (+inf and NaN included), evaluated on the host by
 * the function the device kernel compiles (plain float64 add, multiply and divide: the same bits on both sides). */
int srbd_selftest_atan(const double* x, int32_t n, double* out);

/* ---- Restarting one environment of the loop: what the reference does when an episode ends, and what a batch needs
 * besides (csrc/srbd_reset.h, which the device form srbd_loop_reset_device of srbd_mpc.h compiles too).
 *   srbd_loop_reset <- the episode's end of simulation/simulation.py:773-781 (env.reset, quadrupedpympc_wrapper.reset),
 *                      which reaches WBInterface.reset, quadruped_pympc/interfaces/wb_interface.py:469-484
 * Two levels:
 *   SRBD_RESET_REFERENCE (1)  WBInterface.reset statement for statement: srbd_pgg_reset on pgg (step_freq is left
 *       alone, as the reference leaves it); frg->lift_off = initial_feet, that table only -- the _h tables, touch_down,
 *       the velocity history, stc and the terrain filter are untouched (wb_interface.py:477-479 has those resets
 *       commented out); vfa->initialized[0..3] = 0 (srbd_vfa_reset), nothing else of it.  rising_edge and best_params
 *       are not touched.
 *   SRBD_RESET_EPISODE (2)    every struct handed in becomes, byte for byte, what its constructor call produced: pgg,
 *       stc, terrain_est and vfa the bytes of their snapshot (a copy of the struct taken when the loop was built: so
 *       step_freq and swing_period go back to their constructor values even after srbd_gait_apply_freq changed them);
 *       frg what srbd_frg_init(snapshot stance_time, snapshot hip_height, initial_feet) builds, with hip_offset the
 *       snapshot's: all four position tables copies of the new feet, the history empty and zeroed,
 *       last_reference_footholds zero; *rising_edge = 0; best_params[0..num_params) = 0.0f.  The reference has no such
 *       call, one process being one robot; a batch needs it so that a restarted episode does not inherit the previous
 *       one's 20-entry velocity history and swing clocks.
 * At both levels the reference also sets current_contact = [1, 1, 1, 1] (wb_interface.py:483): the contact flags are
 * the caller's own arrays here (the device call takes them as contact_rows).
 * Every struct pointer, rising_edge and best_params may be NULL: that piece is not part of the caller's loop.
 * SRBD_E_INVALID, nothing changed: a level outside {1, 2}; frg without initial_feet; at level 2 a struct without its
 * snapshot; best_params with num_params < 1. */
enum { SRBD_RESET_REFERENCE = 1, SRBD_RESET_EPISODE = 2 };
int srbd_loop_reset(int32_t level, const double initial_feet[12], srbd_pgg* pgg, srbd_frg* frg, srbd_stc* stc,
                    srbd_terrain_est* terrain_est, srbd_vfa* vfa, const srbd_pgg* pgg_snapshot,
                    const srbd_frg* frg_snapshot, const srbd_stc* stc_snapshot,
                    const srbd_terrain_est* terrain_est_snapshot, const srbd_vfa* vfa_snapshot, int32_t* rising_edge,
                    float* best_params, int32_t num_params);

/* ---- MPC -> WBC shared-memory seqlock (single writer, any number of readers) ---- */
#define SRBD_SHM_DOUBLES 75
enum {
    SRBD_SHM_GRF = 0,         /* 12: GRFs (contact-masked), legs FL FR RL RR */
    SRBD_SHM_FOOTHOLDS = 12,  /* 12 */
    SRBD_SHM_JOINTS_POS = 24, /* 12 */
    SRBD_SHM_JOINTS_VEL = 36, /* 12 */
    SRBD_SHM_JOINTS_ACC = 48, /* 12 */
    SRBD_SHM_PRED = 60,       /* 12: predicted state [p, v, rpy, omega] */
    SRBD_SHM_BEST_FREQ = 72,
    SRBD_SHM_LOOP_TIME = 73,
    SRBD_SHM_STAMP = 74
};

/* One MPC result as the writer packs it (joints may be NULL -> zeros, as the sampling controller). */
typedef struct srbd_shm_msg {
    double grf[12], footholds[12], joints_pos[12], joints_vel[12], joints_acc[12], pred[12];
    double best_freq, loop_time, stamp;
} srbd_shm_msg;

/* Pack and publish: seq odd while writing, even when stable (run_controller.py:343-358).
 * seq and payload (SRBD_SHM_DOUBLES) live in memory shared with the readers. */
int srbd_shm_publish(uint64_t* seq, double* payload, const srbd_shm_msg* msg);
/* Consistent snapshot: returns 1 and fills msg (and *seq_out) when no write overlapped the copy,
 * 0 when the writer was active (caller keeps its previous values), negative on bad arguments. */
int srbd_shm_read(const uint64_t* seq, const double* payload, srbd_shm_msg* msg, uint64_t* seq_out);

/* jax.random keys of the reference's noise stream (srbd_set_rng SRBD_RNG_JAX / SRBD_RNG_JAX_LEGACY; the
 * draws themselves are made on the device).  partitionable: jax_threefry_partitionable (1 = JAX's default
 * since 0.5.0, 0 = earlier JAX).  A key is uint32[2]; srbd_step's `seed` packs it as key[0] << 32 | key[1].
 *   srbd_jax_prng_key <- jax.random.PRNGKey(seed)   quadruped_pympc/controllers/sampling/centroidal_nmpc_jax.py:167
 *   srbd_jax_split    <- jax.random.split(key, num) (with_newkey = split(key)[0], centroidal_nmpc_jax.py:498-501) */
int srbd_jax_prng_key(uint64_t seed, uint32_t key_out[2]);
int srbd_jax_split(const uint32_t key[2], int32_t num, int32_t partitionable, uint32_t* keys_out /* num x 2 */);

#ifdef __cplusplus
}
#endif
#endif /* SRBD_HOST_H */
