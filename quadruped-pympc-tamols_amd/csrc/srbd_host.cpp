// srbd_host.cpp -- host producers and transports around the MPC step (include/srbd_host.h).
// Reference paths are relative to the reference repository root:
//   PGG  = quadruped_pympc/helpers/periodic_gait_generator.py
//   NMPC = quadruped_pympc/controllers/sampling/centroidal_nmpc_jax.py
//   ROS  = ros2/run_controller.py
//   FRG  = quadruped_pympc/helpers/foothold_reference_generator.py
//   STC  = quadruped_pympc/helpers/swing_trajectory_controller.py
//   WBI  = quadruped_pympc/interfaces/wb_interface.py
//   VM   = quadruped_pympc/helpers/velocity_modulator.py
//   TE   = quadruped_pympc/helpers/terrain_estimator.py
//   ESD  = quadruped_pympc/helpers/early_stance_detector.py
//   SCI  = quadruped_pympc/helpers/swing_generators/scipy_swing_trajectory_generator.py
// Built with -ffp-contract=off: every float64 operation rounds as NumPy's does.
#include <math.h>
#include <string.h>

#include "../../include/srbd_host.h"
#include "../../include/srbd_mpc.h"
#include "srbd_frg.h"
#include "srbd_gait_adapt.h"
#include "srbd_iface.h"
#include "srbd_jaxrng.h"
#include "srbd_reflex.h"
#include "srbd_reset.h"
#include "srbd_start_stop.h"
#include "srbd_stc.h"
#include "srbd_terrain.h"
#include "srbd_vfa.h"

namespace {

// Python's float `x % 1.0` (result takes the divisor's sign; fmod is exact).
double pymod1(double x) {
    double r = fmod(x, 1.0);
    if (r != 0.0) {
        if (r < 0.0) r += 1.0;
    } else {
        r = copysign(0.0, 1.0);
    }
    return r;
}

}  // namespace

extern "C" int srbd_pgg_reset(srbd_pgg* g) {
    if (!g) return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l) srbd::pgg_reset_leg(g, l);  // PGG:22-46 (srbd_reset.h, shared with the device reset)
    return SRBD_OK;
}

extern "C" int srbd_pgg_init(srbd_pgg* g, int32_t gait_type, double duty_factor, double step_freq, int32_t horizon) {
    if (!g || horizon < 1) return SRBD_E_INVALID;
    memset(g, 0, sizeof(*g));
    g->duty_factor = duty_factor;
    g->step_freq = step_freq;
    g->horizon = horizon;
    g->gait_type = gait_type;
    g->previous_gait_type = gait_type;
    return srbd_pgg_reset(g);
}

// PGG:48-76, one leg at a time in the reference's order of operations.
extern "C" int srbd_pgg_run(srbd_pgg* g, double dt, double step_freq, double contact_out[4]) {
    if (!g || !contact_out) return SRBD_E_INVALID;
    const double inc = dt * step_freq;
    for (int l = 0; l < 4; ++l) {
        double ph = g->phase_signal[l] + inc;
        ph = pymod1(ph);
        double c;
        if (g->init[l]) {
            if (ph <= g->phase_offset[l]) {
                c = 1.0;
            } else {
                g->init[l] = 0;
                c = 1.0;
                ph = 0.0;
            }
        } else {
            c = ph < g->duty_factor ? 1.0 : 0.0;
        }
        g->phase_signal[l] = ph;
        contact_out[l] = c;
    }
    return SRBD_OK;
}

extern "C" int srbd_pgg_set_phase_signal(srbd_pgg* g, const double phase[4], const int32_t* init) {
    if (!g || !phase) return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l) {
        g->phase_signal[l] = phase[l];
        g->init[l] = init ? (init[l] != 0) : 0;
    }
    return SRBD_OK;
}

// PGG:93-118.  The generator state is restored afterwards (set_phase_signal(t_init, init_init)).
extern "C" int srbd_pgg_contact_sequence(srbd_pgg* g, const double* dts, const int32_t* lens, int32_t n_dts,
                                         double* out, int32_t out_cap) {
    if (!g || !out || g->horizon < 1) return SRBD_E_INVALID;
    const int H = g->horizon;
    if (g->gait_type == SRBD_GAIT_FULL_STANCE) {
        if (out_cap < 8 * H) return SRBD_E_INVALID;
        for (int i = 0; i < 8 * H; ++i) out[i] = 1.0;
        srbd_pgg_reset(g);
        return 2 * H;
    }
    if (out_cap < 4 * H || (H > 1 && (!dts || !lens || n_dts < 1))) return SRBD_E_INVALID;
    double t_init[4];
    int32_t init_init[4];
    memcpy(t_init, g->phase_signal, sizeof(t_init));
    memcpy(init_init, g->init, sizeof(init_init));
    double c[4];
    srbd_pgg_run(g, 0.0, g->step_freq, c);
    for (int l = 0; l < 4; ++l) out[l * H] = c[l];
    int j = 0;
    for (int i = 1; i < H; ++i) {
        if (i >= lens[j]) ++j;
        if (j >= n_dts) {  // the reference would raise IndexError here
            srbd_pgg_set_phase_signal(g, t_init, init_init);
            return SRBD_E_INVALID;
        }
        srbd_pgg_run(g, dts[j], g->step_freq, c);
        for (int l = 0; l < 4; ++l) out[l * H + i] = c[l];
    }
    srbd_pgg_set_phase_signal(g, t_init, init_init);
    return H;
}

// PGG:128-196 through the pieces the device kernels spread over a quad (srbd_start_stop.h): four leg verdicts, the
// conjuncts that belong to no leg, the action, then each leg's share of the rewrite.
extern "C" int srbd_pgg_start_stop(srbd_pgg* g, const double* feet, const double* hips, double hip_offset,
                                   const double base_pos[3], const double euler[3], const double base_lin_vel[3],
                                   const double base_ang_vel[3], const double ref_lin[3], const double ref_ang[3],
                                   const double current_contact[4]) {
    if (!g || !feet || !hips || !base_pos || !euler || !base_lin_vel || !base_ang_vel || !ref_lin || !ref_ang ||
        !current_contact)
        return SRBD_E_INVALID;
    double c, s;
    srbd::yaw_sincos(euler[2], c, s);
    bool stop = srbd::ss_quiet(ref_lin, ref_ang, base_lin_vel, base_ang_vel, euler, current_contact);
    for (int l = 0; l < 4; ++l)
        stop = srbd::ss_leg_close(l, feet + 3 * l, hips + 3 * l, base_pos, c, s, hip_offset) && stop;
    const int32_t action = srbd::ss_action(stop, g->gait_type);
    const int32_t gait = srbd::ss_next_gait(action, g->gait_type, g->previous_gait_type);
    for (int l = 0; l < 4; ++l)
        srbd::ss_apply_leg(l, action, gait, g->phase_offset[l], g->phase_signal[l], g->init[l]);
    if (action != srbd::SS_UNTOUCHED) g->gait_type = gait;
    return action;
}

// NMPC:563-627 (shift_solution off, config.py:188).
extern "C" int srbd_prepare_state(const double state_in[24], const double ref_in[24], const double current_contact[4],
                                  const double previous_contact[4], int32_t params_per_leg, float* best_params,
                                  double state_out[24], double ref_out[24]) {
    if (!state_in || !ref_in || !current_contact || !previous_contact || !state_out || !ref_out)
        return SRBD_E_INVALID;
    if (best_params && params_per_leg < 1) return SRBD_E_INVALID;
    double st[24];
    memcpy(st, state_in, sizeof(st));
    for (int l = 0; l < 4; ++l)
        if (current_contact[l] == 0.0) memcpy(st + 12 + 3 * l, ref_in + 12 + 3 * l, sizeof(double) * 3);
    memcpy(ref_out, ref_in, sizeof(double) * 24);
    memcpy(state_out, st, sizeof(st));
    if (best_params)
        for (int l = 0; l < 4; ++l)
            if (previous_contact[l] == 1.0 && current_contact[l] == 0.0)
                for (int j = 0; j < params_per_leg; ++j) best_params[l * params_per_leg + j] = 0.0f;
    return SRBD_OK;
}

// ------------------------------------------------------------------ foothold reference generator (srbd_frg.h)
extern "C" int srbd_frg_init(srbd_frg* g, double stance_time, double hip_height, const double* lift_off) {  // FRG:15-51
    if (!g || !lift_off || !std::isfinite(stance_time) || !std::isfinite(hip_height)) return SRBD_E_INVALID;
    double feet[12];  // lift_off may be a table of g itself
    memcpy(feet, lift_off, sizeof(feet));
    // srbd_reset.h, shared with the device reset: the four tables are copies of lift_off (the _h tables too: the
    // reference's "TODO wrong", reproduced), everything behind them zero
    srbd::frg_init_words(g, stance_time, hip_height, 0.1, feet, 0, 1);
    return SRBD_OK;
}

extern "C" int srbd_frg_update_lift_off(srbd_frg* g, const double previous_contact[4], const double current_contact[4],
                                        const double* feet, int32_t full_stance, const double base_pos[3],
                                        double yaw) {  // FRG:159-178
    if (!g || !previous_contact || !current_contact || !feet || !base_pos) return SRBD_E_INVALID;
    double c, s;
    srbd::yaw_sincos(yaw, c, s);
    for (int l = 0; l < 4; ++l)
        srbd::frg_leg_lift_off(g, l, previous_contact[l], current_contact[l], feet + 3 * l, full_stance != 0, base_pos,
                               c, s);
    return SRBD_OK;
}

extern "C" int srbd_frg_update_touch_down(srbd_frg* g, const double previous_contact[4],
                                          const double current_contact[4], const double* feet, int32_t full_stance,
                                          const double base_pos[3], double yaw) {  // FRG:180-199
    if (!g || !previous_contact || !current_contact || !feet || !base_pos) return SRBD_E_INVALID;
    double c, s;
    srbd::yaw_sincos(yaw, c, s);
    for (int l = 0; l < 4; ++l)
        srbd::frg_leg_touch_down(g, l, previous_contact[l], current_contact[l], feet + 3 * l, full_stance != 0,
                                 base_pos, c, s);
    return SRBD_OK;
}

extern "C" int srbd_frg_compute(srbd_frg* g, const double base_pos[3], double yaw, const double base_xy_vel[2],
                                const double ref_xy_vel[2], const double* hips, double com_height_nominal,
                                double gravity, const double* com_pos_offset_w, double* out) {  // FRG:53-157
    if (!g || !base_pos || !base_xy_vel || !ref_xy_vel || !hips || !out) return SRBD_E_INVALID;
    double c, s;
    srbd::yaw_sincos(yaw, c, s);
    const double vx = c * base_xy_vel[0] + s * base_xy_vel[1], vy = -s * base_xy_vel[0] + c * base_xy_vel[1];
    const double rx = c * ref_xy_vel[0] + s * ref_xy_vel[1], ry = -s * ref_xy_vel[0] + c * ref_xy_vel[1];
    double mx, my;
    srbd::frg_mean_with(g, g->hist_len, g->hist_head, vx, vy, mx, my);
    int len, head;
    const int slot = srbd::frg_ring_next(g->hist_len, g->hist_head, len, head);
    g->vel_hist[slot][0] = vx;
    g->vel_hist[slot][1] = vy;
    g->hist_len = len;
    g->hist_head = head;
    double ox, oy;
    srbd::frg_compensation(g, rx, ry, mx, my, sqrt(com_height_nominal / gravity), ox, oy);
    for (int l = 0; l < 4; ++l)
        srbd::frg_leg_foothold(g, l, hips + 3 * l, base_pos, c, s, ox, oy, com_pos_offset_w, out + 3 * l);
    return SRBD_OK;
}

// The mean srbd_frg_compute formed at its last push: the ring as it was before that push, plus the newest entry.
extern "C" int srbd_frg_mean(const srbd_frg* g, double mean_out[2]) {
    if (!g || !mean_out) return SRBD_E_INVALID;
    int len = g->hist_len, head = g->hist_head;
    srbd::frg_ring_sane(len, head);
    if (len == 0) {
        mean_out[0] = mean_out[1] = NAN;
        return SRBD_OK;
    }
    const int newest = head == 0 ? SRBD_FRG_HIST - 1 : head - 1;
    const bool full = len == SRBD_FRG_HIST;  // the ring before the push: full with its head at `newest`, or one shorter
    srbd::frg_mean_with(g, full ? len : len - 1, newest, g->vel_hist[newest][0], g->vel_hist[newest][1], mean_out[0],
                        mean_out[1]);
    return SRBD_OK;
}

// ------------------------------------------------------------------ stance and swing leg controller (srbd_stc.h)
extern "C" int srbd_stc_init(srbd_stc* g, double step_height, double swing_period, double position_gain_fb,
                             double velocity_gain_fb, int32_t generator) {  // STC:5-33
    if (!g || !(swing_period > 0.0) || !std::isfinite(swing_period)) return SRBD_E_INVALID;
    if (generator != SRBD_SWING_BEZIER_REF && generator != SRBD_SWING_EXPLICIT) return SRBD_E_INVALID;
    memset(g, 0, sizeof(*g));
    g->step_height = step_height;
    g->swing_period = swing_period;
    g->position_gain_fb = position_gain_fb;
    g->velocity_gain_fb = velocity_gain_fb;
    g->generator = generator;
    g->use_feedback_linearization = 1;
    g->use_friction_compensation = 1;
    return SRBD_OK;
}

extern "C" int srbd_stc_set_timing(srbd_stc* g, double step_height, double swing_period) {  // STC:35-46
    if (!g || !(swing_period > 0.0) || !std::isfinite(swing_period)) return SRBD_E_INVALID;
    g->step_height = step_height;
    g->swing_period = swing_period;
    return SRBD_OK;
}

extern "C" int srbd_stc_update_swing_time(srbd_stc* g, const double contact[4], double dt) {  // STC:120-127
    if (!g || !contact || !std::isfinite(dt)) return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l) g->swing_time[l] = srbd::stc_clock(g->swing_time[l], g->swing_period, contact[l], dt);
    return SRBD_OK;
}

extern "C" int srbd_stc_reference(const srbd_stc* g, int32_t leg, const double lift_off[3], const double touch_down[3],
                                  double pos[3], double vel[3], double acc[3]) {
    if (!g || !lift_off || !touch_down || !pos || !vel || !acc || leg < 0 || leg > 3 || !srbd::stc_struct_ok(g))
        return SRBD_E_INVALID;
    srbd::stc_reference(g, g->swing_time[leg], lift_off, touch_down, pos, vel, acc);
    return SRBD_OK;
}

// WBI:369-415, :435-465: the clock update, the four legs (friction compensation inside each: the same subtraction
// the reference makes after its loop), then the two flags from the updated clocks.
extern "C" int srbd_stc_step(srbd_stc* g, const srbd_stc_io* io, double dt) {
    if (!g || !io || !std::isfinite(dt) || !std::isfinite(io->apex_interval) || !srbd::stc_struct_ok(g))
        return SRBD_E_INVALID;
    if (!io->jac || !io->jac_dot || !io->mass_matrix || !io->q_dot || !io->foot_pos || !io->foot_vel ||
        !io->qfrc_passive || !io->qfrc_bias || !io->grfs || !io->lift_off || !io->touch_down || !io->contact ||
        !io->tau || !io->des_foot_pos || !io->des_foot_vel)
        return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l)
        g->swing_time[l] = srbd::stc_clock(g->swing_time[l], g->swing_period, io->contact[l], dt);
    for (int l = 0; l < 4; ++l) {
        const srbd::StcLeg x = {io->jac + 9 * l,         io->jac_dot + 9 * l,      io->mass_matrix + 9 * l,
                                io->q_dot + 3 * l,       io->foot_pos + 3 * l,     io->foot_vel + 3 * l,
                                io->qfrc_passive + 3 * l, io->qfrc_bias + 3 * l,   io->grfs + 3 * l,
                                io->lift_off + 3 * l,    io->touch_down + 3 * l,   io->tau + 3 * l,
                                io->des_foot_pos + 3 * l, io->des_foot_vel + 3 * l,
                                io->des_joint_vel ? io->des_joint_vel + 3 * l : nullptr};
        srbd::stc_leg(g, g->swing_time[l], io->contact[l], x);
    }
    if (io->apex) *io->apex = srbd::stc_apex(g->swing_time, g->swing_period, io->contact, io->apex_interval);
    if (io->full_stance) *io->full_stance = srbd::stc_full_stance(io->contact);
    return SRBD_OK;
}

extern "C" int srbd_stc_apex(const srbd_stc* g, const double contact[4], double interval) {  // STC:129-138
    if (!g || !contact || !std::isfinite(interval)) return SRBD_E_INVALID;
    return srbd::stc_apex(g->swing_time, g->swing_period, contact, interval);
}

extern "C" int srbd_stc_full_stance(const double contact[4]) {  // STC:140-146
    if (!contact) return SRBD_E_INVALID;
    return srbd::stc_full_stance(contact);
}

// ------------------------------------------- swing reflexes: early-stance detector and spline generator (srbd_reflex.h)
extern "C" int srbd_reflex_init(srbd_reflex* r, double reflex_max_step_height, int32_t blind, int32_t trigger_mode,
                                int32_t use_height_enhancement) {  // ESD:7-33, SCI:8-23
    if (!r || !std::isfinite(reflex_max_step_height)) return SRBD_E_INVALID;
    if (trigger_mode != SRBD_REFLEX_OFF && trigger_mode != SRBD_REFLEX_TRACKING) return SRBD_E_INVALID;
    memset(r, 0, sizeof(*r));
    r->reflex_max_step_height = reflex_max_step_height;
    r->early_stance_time_threshold = 0.07;
    r->relative_tracking_error_threshold = 0.3;
    r->absolute_min_distance_error_threshold = 0.1;
    for (int l = 0; l < 4; ++l) r->hitmoments[l] = -1.0;
    r->trigger_mode = trigger_mode;
    r->blind = blind != 0;
    r->use_height_enhancement = use_height_enhancement != 0;
    r->gait_cycles = -1;
    r->max_gait_cycles = 6;
    return SRBD_OK;
}

namespace {

bool reflex_struct_ok(const srbd_reflex* r) {
    return (r->trigger_mode == SRBD_REFLEX_OFF || r->trigger_mode == SRBD_REFLEX_TRACKING) &&
           std::isfinite(r->reflex_max_step_height);
}

// ESD:36-128: the legs in order, ending at the first that triggers; then the cycle counter and the flag.
void reflex_detect(srbd_reflex* r, const double* feet, const double* lift_off, const double* touch_down,
                   const double* swing_time, double swing_period, const double* contact, const double* previous) {
    bool triggered = false;
    for (int l = 0; l < 4 && !triggered; ++l) {
        srbd::ReflexLeg s;
        srbd::reflex_leg_load(r, l, s);
        triggered = srbd::reflex_leg_detect(r, s, swing_time[l], swing_period, contact[l], feet + 3 * l,
                                            r->last_des_foot_pos[l], lift_off + 3 * l, touch_down + 3 * l);
        srbd::reflex_leg_store(r, l, s);
    }
    srbd::reflex_cycles(r, triggered, contact, previous, r->gait_cycles, r->height_enhancement);
}

}  // namespace

extern "C" int srbd_reflex_detect(srbd_reflex* r, const double* feet, const double* lift_off, const double* touch_down,
                                  const double swing_time[4], double swing_period, const double contact[4],
                                  const double previous_contact[4]) {
    if (!r || !feet || !lift_off || !touch_down || !swing_time || !contact || !previous_contact || !reflex_struct_ok(r))
        return SRBD_E_INVALID;
    reflex_detect(r, feet, lift_off, touch_down, swing_time, swing_period, contact, previous_contact);
    return SRBD_OK;
}

extern "C" int srbd_reflex_reference(const srbd_stc* g, const srbd_reflex* r, int32_t leg, const double lift_off[3],
                                     const double touch_down[3], double pos[3], double vel[3], double acc[3]) {
    if (!g || !r || !lift_off || !touch_down || !pos || !vel || !acc || leg < 0 || leg > 3 ||
        !srbd::reflex_structs_ok(g, r))
        return SRBD_E_INVALID;
    srbd::ReflexLeg s;
    srbd::reflex_leg_load(r, leg, s);
    srbd::reflex_reference(g, r, s, r->height_enhancement, g->swing_time[leg], lift_off, touch_down, pos, vel, acc);
    return SRBD_OK;
}

// WBI:362-415, :435-465: the detector on what the previous step left, then srbd_stc_step's stages with the spline
// generator, and the desired foot positions kept for the next step's detector (WBI:408).
extern "C" int srbd_reflex_step(srbd_stc* g, srbd_reflex* r, const srbd_stc_io* io, const double previous_contact[4],
                                double dt) {
    if (!g || !r || !io || !previous_contact || !std::isfinite(dt) || !std::isfinite(io->apex_interval) ||
        !srbd::reflex_structs_ok(g, r))
        return SRBD_E_INVALID;
    if (!io->jac || !io->jac_dot || !io->mass_matrix || !io->q_dot || !io->foot_pos || !io->foot_vel ||
        !io->qfrc_passive || !io->qfrc_bias || !io->grfs || !io->lift_off || !io->touch_down || !io->contact ||
        !io->tau || !io->des_foot_pos || !io->des_foot_vel)
        return SRBD_E_INVALID;
    reflex_detect(r, io->foot_pos, io->lift_off, io->touch_down, g->swing_time, g->swing_period, io->contact,
                  previous_contact);
    for (int l = 0; l < 4; ++l)
        g->swing_time[l] = srbd::stc_clock(g->swing_time[l], g->swing_period, io->contact[l], dt);
    for (int l = 0; l < 4; ++l) {
        const srbd::StcLeg x = {io->jac + 9 * l,         io->jac_dot + 9 * l,      io->mass_matrix + 9 * l,
                                io->q_dot + 3 * l,       io->foot_pos + 3 * l,     io->foot_vel + 3 * l,
                                io->qfrc_passive + 3 * l, io->qfrc_bias + 3 * l,   io->grfs + 3 * l,
                                io->lift_off + 3 * l,    io->touch_down + 3 * l,   io->tau + 3 * l,
                                io->des_foot_pos + 3 * l, io->des_foot_vel + 3 * l,
                                io->des_joint_vel ? io->des_joint_vel + 3 * l : nullptr};
        srbd::ReflexSplineGen gen = {g, r, {}, r->height_enhancement, g->swing_time[l], x.lift_off, x.touch_down};
        srbd::reflex_leg_load(r, l, gen.s);
        srbd::stc_leg_with(g, io->contact[l], x, gen);
    }
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 3; ++k) r->last_des_foot_pos[l][k] = io->des_foot_pos[3 * l + k];
    if (io->apex) *io->apex = srbd::stc_apex(g->swing_time, g->swing_period, io->contact, io->apex_interval);
    if (io->full_stance) *io->full_stance = srbd::stc_full_stance(io->contact);
    return SRBD_OK;
}

// ------------------------------------------- gait adaptation: trigger and frequency write-back (srbd_gait_adapt.h)
extern "C" int srbd_stc_touch_down(int32_t* rising_edge, const double current_contact[4],
                                   const double previous_contact[4], const double* contact_sequence,
                                   int32_t contact_stride, int32_t horizon, int32_t lookahead) {  // STC:148-165
    if (!rising_edge || !current_contact || !previous_contact || !contact_sequence) return SRBD_E_INVALID;
    if (horizon < 2 || contact_stride < horizon || lookahead < 1 || lookahead > horizon - 1) return SRBD_E_INVALID;
    return srbd::ga_touch_down(rising_edge, current_contact, previous_contact, contact_sequence, contact_stride,
                               lookahead);
}

extern "C" int srbd_gait_apply_freq(srbd_pgg* pgg, srbd_frg* frg, srbd_stc* stc, int32_t optimize,
                                    float best_freq) {  // WBI:354-358
    if (!pgg) return SRBD_E_INVALID;
    return srbd::ga_apply_freq(pgg, frg, stc, optimize, best_freq);
}

// ------------------------------------------- apex-gated foothold adaptation: the state machine (srbd_vfa.h)
extern "C" int srbd_vfa_init(srbd_vfa* g) {  // VFA:38-46
    if (!g) return SRBD_E_INVALID;
    memset(g, 0, sizeof(*g));
    for (int k = 0; k < 24; ++k) g->boxes[k] = NAN;
    return SRBD_OK;
}

extern "C" int srbd_vfa_reset(srbd_vfa* g) {  // VFA:63-64
    if (!g) return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l) srbd::vfa_reset_leg(g, l);
    return SRBD_OK;
}

extern "C" int srbd_vfa_mode(const srbd_vfa* g, const srbd_stc* stc, const double contact[4], double apex_interval,
                             int32_t* mode) {  // WBI:232, :243
    if (!g || !stc || !contact || !mode || !std::isfinite(apex_interval) || !srbd::vfa_struct_ok(g))
        return SRBD_E_INVALID;
    *mode = srbd::vfa_mode(g->initialized[0], stc, contact, apex_interval);
    return SRBD_OK;
}

extern "C" int srbd_vfa_commit(srbd_vfa* g, int32_t mode, const double seeds[12], const double searched_footholds[12],
                               const double searched_boxes[24], const int32_t searched_valid[4],
                               double out_footholds[12], double out_boxes[24], int32_t out_valid[4]) {
    if (!g || !seeds || !out_footholds || !out_boxes || !out_valid || !srbd::vfa_mode_ok(mode) ||
        !srbd::vfa_struct_ok(g))
        return SRBD_E_INVALID;
    const bool search = mode == SRBD_VFA_SEARCH;
    if (search && (!searched_footholds || !searched_boxes || !searched_valid)) return SRBD_E_INVALID;
    for (int l = 0; l < 4; ++l)
        srbd::vfa_commit_leg(g, l, mode, seeds + 3 * l, search ? searched_footholds + 3 * l : nullptr,
                             search ? searched_boxes + 6 * l : nullptr, search ? searched_valid[l] : 0,
                             out_footholds + 3 * l, out_boxes + 6 * l, out_valid + l);
    return SRBD_OK;
}

extern "C" int srbd_vfa_height_search(const double* patch, int32_t rows, int32_t cols, const double seed[3],
                                      double foothold[3], int32_t* valid) {  // VFA:145-151, PatchHeightMap.get_height
    if (!patch || !seed || !foothold || !valid || rows < 1 || cols < 1 || (int64_t)rows * cols > 320)
        return SRBD_E_INVALID;
    const int i = srbd::vfa_height_nearest(patch, rows * cols, seed[0], seed[1]);
    srbd::vfa_height_result(seed[0], seed[1], patch[3 * i + 2], foothold, valid);
    return SRBD_OK;
}

// ------------------------------------------- per-environment reset of the loop's state (srbd_reset.h)
extern "C" int srbd_loop_reset(int32_t level, const double initial_feet[12], srbd_pgg* pgg, srbd_frg* frg,
                               srbd_stc* stc, srbd_terrain_est* terrain_est, srbd_vfa* vfa,
                               const srbd_pgg* pgg_snapshot, const srbd_frg* frg_snapshot,
                               const srbd_stc* stc_snapshot, const srbd_terrain_est* terrain_est_snapshot,
                               const srbd_vfa* vfa_snapshot, int32_t* rising_edge, float* best_params,
                               int32_t num_params) {  // WBI:469-484, SIM:773-781
    const srbd::LoopResetEnv x = {initial_feet,  pgg,          frg,          stc,
                                  terrain_est,   vfa,          pgg_snapshot, frg_snapshot,
                                  stc_snapshot,  terrain_est_snapshot, vfa_snapshot, rising_edge,
                                  best_params,   num_params};
    if (level != SRBD_RESET_REFERENCE && level != SRBD_RESET_EPISODE) return SRBD_E_INVALID;
    if (srbd::loop_reset_refusal(x, level)) return SRBD_E_INVALID;
    srbd::loop_reset_env(x, level, 0, 1);
    return SRBD_OK;
}

// ------------------------------------------- velocity modulator, terrain estimator, reference row (srbd_terrain.h)
extern "C" int srbd_vm_modulate(double max_distance, const double lin[3], const double ang[3], const double* feet,
                                const double* hips, double lin_out[3], double ang_out[3]) {  // VM:19-46
    if (!lin || !ang || !feet || !hips || !lin_out || !ang_out) return SRBD_E_INVALID;
    bool beyond = false;
    for (int l = 0; l < 4; ++l) beyond = beyond || srbd::vm_distance(feet + 3 * l, hips + 3 * l) > max_distance;
    const bool standing = srbd::vm_standing(lin);
    for (int k = 0; k < 3; ++k) {
        lin_out[k] = srbd::vm_entry(lin[k], standing, beyond);
        ang_out[k] = srbd::vm_entry(ang[k], standing, beyond);
    }
    return SRBD_OK;
}

extern "C" int srbd_terrain_est_init(srbd_terrain_est* g) {  // TE:5-11
    if (!g) return SRBD_E_INVALID;
    memset(g, 0, sizeof(*g));
    g->pitch_activated = 1;
    return SRBD_OK;
}

// TE:13-106 through the pieces the device kernel spreads over a quad: four rotations, four slopes, one filter.
extern "C" int srbd_terrain_estimate(srbd_terrain_est* g, const double base_pos[3], double yaw, const double* feet,
                                     double out[3]) {
    if (!g || !base_pos || !feet) return SRBD_E_INVALID;
    double c, s, r[4][3], angle[4], dz[4], foot_z[4];
    srbd::yaw_sincos(yaw, c, s);
    for (int l = 0; l < 4; ++l) {
        srbd::terr_rotate(feet + 3 * l, base_pos, c, s, r[l]);
        foot_z[l] = feet[3 * l + 2];
    }
    for (int k = 0; k < 4; ++k) {
        int a, b;
        srbd::terr_pair(k, a, b);
        angle[k] = srbd::terr_slope(k, r[a], r[b], dz[k]);
    }
    srbd::terr_filter(g, angle, dz, foot_z);
    if (out) out[0] = g->roll, out[1] = g->pitch, out[2] = g->height;
    return SRBD_OK;
}

extern "C" int srbd_reference_assemble(const srbd_terrain_est* g, double ref_z, double base_z, double com_z,
                                       double com_off_z, const double lin[3], const double ang[3],
                                       double ref_out[12]) {  // WBI:258-291
    if (!g || !lin || !ang || !ref_out) return SRBD_E_INVALID;
    double cr, sr, cp, sp;
    srbd::yaw_sincos(g->roll, cr, sr);
    srbd::yaw_sincos(g->pitch, cp, sp);
    srbd::terr_assemble(g->roll, g->pitch, g->height, cr, sr, cp, sp, ref_z, base_z, com_z, com_off_z, lin, ang,
                        ref_out);
    return SRBD_OK;
}

extern "C" int srbd_selftest_atan(const double* x, int32_t n, double* out) {
    if (!x || !out || n < 0) return SRBD_E_INVALID;
    for (int32_t i = 0; i < n; ++i) out[i] = srbd::terr_atan(x[i]);
    return SRBD_OK;
}

// srbd_api.hip: the chained form (TAMOLS writes the step's device input; one host wait), 1 when not taken.
extern "C" int srbd_foothold_chain(srbd_tamols_ctx* t, srbd_terrain* ter, const srbd_tamols_params* p, srbd_ctx* c,
                                   srbd_foothold_io* io, const float* contact, int32_t stride, float* best,
                                   int32_t ppl, uint64_t seed, uint64_t counter, srbd_result* out);

// helpers/foothold_pipeline.py TamolsMpcStep.step in one host call (include/srbd_mpc.h).  The base position and
// the current feet TAMOLS reads are the state's own (state_in[0:3], state_in[12:24]); its contact flags are the
// current contact truncated to int32 (VFA's astype).  Chained on the device where the context allows it, else the
// calls in sequence below; the same results either way.
extern "C" int srbd_foothold_mpc_step(srbd_tamols_ctx* tamols, srbd_terrain* terrain, const srbd_tamols_params* params,
                                      srbd_ctx* ctx, srbd_foothold_io* io, const float* contact,
                                      int32_t contact_stride, float* best_params, int32_t params_per_leg,
                                      uint64_t seed, uint64_t counter, srbd_result* out) {
    if (!tamols || !terrain || !params || !ctx || !io || !contact || !best_params || !out || params_per_leg < 1)
        return SRBD_E_INVALID;
    io->stage = 0;
    const int chained = srbd_foothold_chain(tamols, terrain, params, ctx, io, contact, contact_stride, best_params,
                                            params_per_leg, seed, counter, out);
    if (chained != 1) return chained;
    int32_t cint[4];
    for (int l = 0; l < 4; ++l) cint[l] = (int32_t)io->current_contact[l];
    int rc = srbd_tamols_run_terrain(tamols, terrain, io->yaw, io->rows, io->cols, io->dist_x, io->dist_y, io->ray_z,
                                     io->seeds, io->hips, io->forward_vel, io->state_in, cint, io->state_in + 12,
                                     params, io->footholds, io->boxes, io->valid, io->scores, io->seed_heights,
                                     io->heightmaps);
    if (rc != SRBD_OK) return rc;
    io->stage = 1;
    double ref_in[24];
    memcpy(ref_in, io->ref_base, sizeof(double) * 12);
    memcpy(ref_in + 12, io->footholds, sizeof(double) * 12);  // wb_interface.py:268-285
    rc = srbd_prepare_state(io->state_in, ref_in, io->current_contact, io->previous_contact, params_per_leg,
                            best_params, io->state_out, io->ref_out);
    if (rc != SRBD_OK) return rc;
    io->stage = 2;
    float st[24], rf[24];
    for (int i = 0; i < 24; ++i) {
        st[i] = (float)io->state_out[i];
        rf[i] = (float)io->ref_out[i];
    }
    rc = srbd_step(ctx, st, rf, contact, contact_stride, best_params, nullptr, nullptr, seed, counter, out, nullptr);
    if (rc == SRBD_OK) io->stage = 3;
    return rc;
}

// ROS:343-358.  The payload words are written with relaxed atomic stores between the odd and even
// sequence stores, so a reader that sees the same even sequence before and after its copy holds one
// message (release on the closing store; acquire/fence on the reader side).
extern "C" int srbd_shm_publish(uint64_t* seq, double* payload, const srbd_shm_msg* m) {
    if (!seq || !payload || !m) return SRBD_E_INVALID;
    double buf[SRBD_SHM_DOUBLES];
    memcpy(buf + SRBD_SHM_GRF, m->grf, sizeof(double) * 12);
    memcpy(buf + SRBD_SHM_FOOTHOLDS, m->footholds, sizeof(double) * 12);
    memcpy(buf + SRBD_SHM_JOINTS_POS, m->joints_pos, sizeof(double) * 12);
    memcpy(buf + SRBD_SHM_JOINTS_VEL, m->joints_vel, sizeof(double) * 12);
    memcpy(buf + SRBD_SHM_JOINTS_ACC, m->joints_acc, sizeof(double) * 12);
    memcpy(buf + SRBD_SHM_PRED, m->pred, sizeof(double) * 12);
    buf[SRBD_SHM_BEST_FREQ] = m->best_freq;
    buf[SRBD_SHM_LOOP_TIME] = m->loop_time;
    buf[SRBD_SHM_STAMP] = m->stamp;
    const uint64_t s = __atomic_load_n(seq, __ATOMIC_RELAXED);
    if ((s & 1u) == 0) __atomic_store_n(seq, s + 1, __ATOMIC_RELAXED);  // odd: writing
    __atomic_thread_fence(__ATOMIC_RELEASE);
    uint64_t* w = reinterpret_cast<uint64_t*>(payload);
    const uint64_t* b = reinterpret_cast<const uint64_t*>(buf);
    for (int i = 0; i < SRBD_SHM_DOUBLES; ++i) __atomic_store_n(w + i, b[i], __ATOMIC_RELAXED);
    __atomic_store_n(seq, (s | 1u) + 1, __ATOMIC_RELEASE);  // even: stable
    return SRBD_OK;
}

// ROS:565-580.
extern "C" int srbd_shm_read(const uint64_t* seq, const double* payload, srbd_shm_msg* m, uint64_t* seq_out) {
    if (!seq || !payload || !m) return SRBD_E_INVALID;
    const uint64_t s1 = __atomic_load_n(seq, __ATOMIC_ACQUIRE);
    if (s1 & 1u) return 0;
    uint64_t buf[SRBD_SHM_DOUBLES];
    const uint64_t* r = reinterpret_cast<const uint64_t*>(payload);
    for (int i = 0; i < SRBD_SHM_DOUBLES; ++i) buf[i] = __atomic_load_n(r + i, __ATOMIC_RELAXED);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const uint64_t s2 = __atomic_load_n(seq, __ATOMIC_RELAXED);
    if (s1 != s2) return 0;
    const double* d = reinterpret_cast<const double*>(buf);
    memcpy(m->grf, d + SRBD_SHM_GRF, sizeof(double) * 12);
    memcpy(m->footholds, d + SRBD_SHM_FOOTHOLDS, sizeof(double) * 12);
    memcpy(m->joints_pos, d + SRBD_SHM_JOINTS_POS, sizeof(double) * 12);
    memcpy(m->joints_vel, d + SRBD_SHM_JOINTS_VEL, sizeof(double) * 12);
    memcpy(m->joints_acc, d + SRBD_SHM_JOINTS_ACC, sizeof(double) * 12);
    memcpy(m->pred, d + SRBD_SHM_PRED, sizeof(double) * 12);
    m->best_freq = d[SRBD_SHM_BEST_FREQ];
    m->loop_time = d[SRBD_SHM_LOOP_TIME];
    m->stamp = d[SRBD_SHM_STAMP];
    if (seq_out) *seq_out = s2;
    return 1;
}

// ------------------------------------------------------------------ jax.random keys (srbd_jaxrng.h)
extern "C" int srbd_jax_prng_key(uint64_t seed, uint32_t key_out[2]) {  // threefry_seed
    if (!key_out) return SRBD_E_INVALID;
    key_out[0] = (uint32_t)(seed >> 32);
    key_out[1] = (uint32_t)seed;
    return SRBD_OK;
}

extern "C" int srbd_jax_split(const uint32_t key[2], int32_t num, int32_t partitionable, uint32_t* out) {
    if (!key || !out || num < 1) return SRBD_E_INVALID;
    // partitionable: key i = threefry(key, (0, i)); legacy: the 2 num bits of iota(2 num), reshaped (num, 2)
    for (int32_t i = 0; i < num; ++i) {
        if (partitionable) {
            uint32_t x0 = 0, x1 = (uint32_t)i;
            srbd::threefry2x32_20(key[0], key[1], x0, x1);
            out[2 * i] = x0;
            out[2 * i + 1] = x1;
        } else {
            const uint64_t M = 2 * (uint64_t)num;
            out[2 * i] = srbd::jax_bits(key[0], key[1], 2 * (uint64_t)i, M, false);
            out[2 * i + 1] = srbd::jax_bits(key[0], key[1], 2 * (uint64_t)i + 1, M, false);
        }
    }
    return SRBD_OK;
}

// ------------------------------------------------------------------ one plugin-API MPC step in one call
// SRBDControllerInterface.compute_control's sampling branch (srbd_controller_interface.py:113-180) over the plain
// Sampling_MPC (include/srbd_mpc.h srbd_interface_step): prepare_state_and_reference (NMPC:563-627, no solution
// shift), then per sampling iteration with_newkey (NMPC:498-501), CEM's with_newsigma(sigma_cem_mppi) at iteration 0,
// jitted_compute_control (srbd_step on device draws, NMPC:629-1094), and the GRFs times current_contact (SCI:175-178).
// The same calls in the same order as the Python chain, so the same bits.
extern "C" int srbd_interface_step(srbd_ctx* ctx, srbd_interface_io* io, const float* contact,
                                   const double* contact64, int32_t contact_stride, float* best_params,
                                   int32_t params_per_leg, float* sigma, srbd_result* out) {
    if (!ctx || !io || (!contact == !contact64) || !best_params || !out || params_per_leg < 1 ||
        io->iterations < 1 || contact_stride < io->horizon || io->horizon < 1 || io->horizon > SRBD_MAX_HORIZON)
        return SRBD_E_INVALID;
    if (io->cem && !sigma) return SRBD_E_INVALID;
    io->stage = 0;
    int rc = srbd_prepare_state(io->state_in, io->ref_in, io->current_contact, io->previous_contact, params_per_leg,
                                best_params, io->state_out, io->ref_out);
    if (rc != SRBD_OK) return rc;
    io->stage = 1;
    float st[24], rf[24];
    for (int i = 0; i < 24; ++i) {  // the step's float32 staging (Context._stage: numpy's round-to-nearest cast)
        st[i] = (float)io->state_out[i];
        rf[i] = (float)io->ref_out[i];
    }
    float cf[4 * SRBD_MAX_HORIZON];
    const float* cs = contact;
    int32_t stride = contact_stride;
    if (contact64) {
        const int H = io->horizon;
        for (int l = 0; l < 4; ++l)
            for (int k = 0; k < H; ++k) cf[l * H + k] = (float)contact64[(size_t)l * contact_stride + k];
        cs = cf;
        stride = H;
    }
    const int P = 4 * params_per_leg;
    for (int it = 0; it < io->iterations; ++it) {
        uint64_t seed, counter;
        if (io->rng == SRBD_RNG_PHILOX) {  // master_key = (seed, counter + 1)
            io->key[1] += 1;
            seed = io->key[0];
            counter = io->key[1];
        } else {  // master_key = split(master_key)[0]; the call count numbers the device step
            const uint32_t k[2] = {(uint32_t)(io->key[0] >> 32), (uint32_t)io->key[0]};
            uint32_t o[4];
            if ((rc = srbd_jax_split(k, 2, io->rng == SRBD_RNG_JAX ? 1 : 0, o)) != SRBD_OK) return rc;
            io->key[0] = ((uint64_t)o[0] << 32) | o[1];
            io->key[1] += 1;
            seed = io->key[0];
            counter = io->key[1];
        }
        if (io->cem && it == 0)
            for (int j = 0; j < P; ++j) sigma[j] = (float)io->sigma_reset;
        rc = srbd_step(ctx, st, rf, cs, stride, best_params, io->cem ? sigma : nullptr, nullptr, seed, counter, out,
                       nullptr);
        if (rc != SRBD_OK) return rc;
        io->stage = 2 + it;
    }
    for (int l = 0; l < 4; ++l)
        for (int c = 0; c < 3; ++c) io->grf[3 * l + c] = (double)out->grf[3 * l + c] * io->current_contact[l];
    return SRBD_OK;
}

// The key schedule of srbd_batch_interface_step_device's prologue kernel on the host (srbd_iface.h: the same function
// the kernel runs; it is also the schedule of srbd_interface_step above), for the CPU tests.
extern "C" int srbd_selftest_interface_keys(uint64_t* keys_io, int32_t n, int32_t rng, int32_t iterations,
                                            uint64_t* step_keys) {
    if (!keys_io || !step_keys || n < 1 || iterations < 1 || iterations > srbd::IFACE_MAX_ITERS) return SRBD_E_INVALID;
    if (rng != SRBD_RNG_PHILOX && rng != SRBD_RNG_JAX && rng != SRBD_RNG_JAX_LEGACY) return SRBD_E_INVALID;
    for (int32_t e = 0; e < n; ++e) {
        uint64_t k0 = keys_io[2 * (size_t)e], k1 = keys_io[2 * (size_t)e + 1];
        for (int32_t i = 0; i < iterations; ++i) {
            srbd::iface_next_key(rng, k0, k1);
            uint64_t* o = step_keys + 2 * ((size_t)i * n + e);
            o[0] = k0;
            o[1] = k1;
        }
        keys_io[2 * (size_t)e] = k0;
        keys_io[2 * (size_t)e + 1] = k1;
    }
    return SRBD_OK;
}
