// srbd_start_stop.h -- the gait generator's start-and-stop decision: whether a robot that stands still with no command
// drops into full stance, and whether one in full stance takes its gait up again.  Plain functions compiled by the
// host C++ (srbd_host.cpp srbd_pgg_start_stop) and by the HIP kernels (srbd_producers.hip start_stop_kernel,
// wb_update_kernel), float64 and unfused, with cos / sin of the yaw from yaw_sincos.h and no libm call besides the
// correctly rounded sqrt, so both sides leave the same bits.
//   PGG = quadruped_pympc/helpers/periodic_gait_generator.py (update_start_and_stop :128-196, set_full_stance
//         :120-122, restore_previous_gait :124-126)
//   WBI = quadruped_pympc/interfaces/wb_interface.py (the call :175-189)
// The work is cut the way a quad of lanes owns it: one leg's foot-to-hip distance in the horizontal frame
// (ss_leg_close), the conjuncts that belong to no leg (ss_quiet), the verdict (ss_action, ss_next_gait) and one leg's
// share of the struct's rewrite (ss_apply_leg).  The host runs the same pieces in a loop over the legs.
// The reference's mean of the four distances (PGG:176-178) is never read and is not formed here.
// Agreement with the reference: its R_W2H holds np.cos / np.sin of the yaw and its norms are np.linalg.norm; here the
// rotation is yaw_sincos.h's and a norm is sqrt((x x + y y) + z z).  The two agree to rounding, so a quantity that lies
// within rounding of 0.1, 0.05 or 0.06 may fall on the other side of its threshold; the recorded fixture
// (tests/golden/start_stop_ref.npz) keeps every such quantity at least 1e-9 relative away from it.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "srbd_reset.h"
#include "yaw_sincos.h"

namespace srbd {

enum { SS_UNTOUCHED = 0, SS_STOPPED = 1, SS_RESTORED = 2 };

// PGG:182-185: sqrt((x x + y y) + z z).  A component whose square underflows adds zero, as in NumPy.
YAW_HD inline double ss_norm(const double* v) {
#pragma clang fp contract(off)
    return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// PGG:148-175, :189-192 for leg l (FL FR RL RR): foot and hip rotated into the horizontal frame, R_W2H @ (p_xy -
// base_xy) with each row's two products summed left to right; the foot's y shifted by the hip offset (- for FL and RL,
// + for FR and RR); the distance sqrt(dx dx + dy dy) and its comparison with 0.06.  A NaN fails the comparison.
YAW_HD inline bool ss_leg_close(int l, const double* foot, const double* hip, const double* base, double c, double s,
                                double hip_offset) {
#pragma clang fp contract(off)
    const double fx = foot[0] - base[0], fy = foot[1] - base[1];
    const double fhx = c * fx + s * fy;
    double fhy = -s * fx + c * fy;
    fhy = (l == 0 || l == 2) ? fhy - hip_offset : fhy + hip_offset;
    const double px = hip[0] - base[0], py = hip[1] - base[1];
    const double hhx = c * px + s * py;
    const double hhy = -s * px + c * py;
    const double dx = fhx - hhx, dy = fhy - hhy;
    return sqrt(dx * dx + dy * dy) < 0.06;
}

// PGG:182-188: the seven conjuncts that belong to no leg.  contact: the four current contact flags widened to
// double, summed first to last as np.sum sums four entries.  A NaN anywhere fails its comparison.
YAW_HD inline bool ss_quiet(const double* ref_lin, const double* ref_ang, const double* lin_vel, const double* ang_vel,
                            const double* euler, const double* contact) {
#pragma clang fp contract(off)
    return ss_norm(ref_lin) == 0.0 && ss_norm(ref_ang) == 0.0 && ss_norm(lin_vel) < 0.1 && ss_norm(ang_vel) < 0.1 &&
           fabs(euler[0]) < 0.05 && fabs(euler[1]) < 0.05 &&
           ((contact[0] + contact[1]) + contact[2]) + contact[3] == 4.0;
}

// PGG:193-196: stop on every call in which the condition holds; otherwise a generator in full stance is restored.
YAW_HD inline int32_t ss_action(bool stop, int32_t gait_type) {
    return stop ? SS_STOPPED : gait_type == SRBD_GAIT_FULL_STANCE ? SS_RESTORED : SS_UNTOUCHED;
}

// The gait type after the action: set_full_stance's, restore_previous_gait's, or the one found.
YAW_HD inline int32_t ss_next_gait(int32_t action, int32_t gait_type, int32_t previous_gait_type) {
    return action == SS_STOPPED ? (int32_t)SRBD_GAIT_FULL_STANCE : action == SS_RESTORED ? previous_gait_type : gait_type;
}

// Leg l's share of set_full_stance / restore_previous_gait: srbd_pgg_reset's three assignments (srbd_reset.h
// pgg_reset_leg's) for the new gait type `gait`, on the leg's three words wherever the caller keeps them -- the struct
// on the host, registers in a kernel that goes on to advance them.  The caller stores `gait` itself; previous_gait_type
// is left alone.  Nothing is written for SS_UNTOUCHED.
YAW_HD inline void ss_apply_leg(int l, int32_t action, int32_t gait, double& phase_offset, double& phase_signal,
                                int32_t& init) {
    if (action == SS_UNTOUCHED) return;
    const double off = pgg_gait_offset(gait, l);
    phase_offset = off;
    phase_signal = off;
    init = 0;
}

}  // namespace srbd
