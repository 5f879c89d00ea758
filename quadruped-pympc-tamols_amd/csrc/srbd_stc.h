// srbd_stc.h -- the stance and swing leg controller's arithmetic, one leg at a time, for the host functions
// (srbd_host.cpp srbd_stc_*) and the device kernel (srbd_producers.hip stc_step_kernel).  Both sides compile these
// same float64 operations unfused, in the order written here, and the only libm calls are fmod and fabs (exact on
// both sides), so they leave the same bits.
//   STC = quadruped_pympc/helpers/swing_trajectory_controller.py
//   BEZ = quadruped_pympc/helpers/swing_generators/bezier_ref_swing_trajectory_generator.py
//   EXP = quadruped_pympc/helpers/swing_generators/explicit_swing_trajectory_generator.py
//   WBI = quadruped_pympc/interfaces/wb_interface.py (compute_stance_and_swing_torque :304-467)
// 3 x 3 matrices are row-major.  Products are written out and summed left to right:
//   (A @ v)[i]   = (A[i][0] v[0] + A[i][1] v[1]) + A[i][2] v[2]
//   (A.T @ v)[j] = (A[0][j] v[0] + A[1][j] v[1]) + A[2][j] v[2]
//   (A @ B)[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]
// Integer powers are repeated multiplication, x^k = x^(k-1) * x; the reference's `**` goes through libm's pow, which
// differs from that in the last places.
// Deviation, Jinv: the reference takes np.linalg.pinv(J) (an SVD).  Here Jinv is the 3 x 3 inverse by cofactors over
// the determinant.  For a well-conditioned J the two agree to rounding; for a singular J they do not: the
// pseudo-inverse is the least-squares inverse, this one is the zero matrix whenever det is zero or not finite, so
// outputs stay finite and the feedback-linearisation term reduces to the bias force h.
// Not in this file: the early-stance detector and the scipy generator, which reads its hit moment and hit point, have
// a file of their own (srbd_reflex.h, srbd_reflex_step); it runs stc_leg_with below with its spline in the generator's
// place.  Out of scope: inverse kinematics and des_joints_pos; the kinodynamic branch.  The re-timing from
// optimize_swing / best_sample_freq (WBI:354-358) lives in srbd_gait_adapt.h.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "yaw_sincos.h"

namespace srbd {

// What srbd_stc_step refuses in the struct: an unknown generator, a swing_period that is not positive and finite.
YAW_HD inline bool stc_struct_ok(const srbd_stc* g) {
    const bool gen = g->generator == SRBD_SWING_BEZIER_REF || g->generator == SRBD_SWING_EXPLICIT;
    return gen && g->swing_period > 0.0 && fabs(g->swing_period) <= 1.7976931348623157e308;
}

// STC:120-127, one leg: the clock after update_swing_time.  A NaN contact is not == 0: the clock is reset.
YAW_HD inline double stc_clock(double swing_time, double swing_period, double contact, double dt) {
#pragma clang fp contract(off)
    if (contact == 0.0) return swing_time < swing_period ? swing_time + dt : swing_time;
    return 0.0;
}

// np.clip(x, lo, hi): a NaN x passes.
YAW_HD inline double stc_clip(double x, double lo, double hi) {
    const double t = x != x ? x : (x > lo ? x : lo);
    return t != t ? t : (t < hi ? t : hi);
}

// Python's float `x % y` (the result takes the divisor's sign; fmod is exact).
YAW_HD inline double stc_pymod(double x, double y) {
#pragma clang fp contract(off)
    double r = fmod(x, y);
    if (r != 0.0) {
        if ((y < 0.0) != (r < 0.0)) r = r + y;
    } else {
        r = y < 0.0 ? -0.0 : 0.0;
    }
    return r;
}

// BEZ:62-265: the degree-6 Bezier from lift_off to touch_down at clock t.  Control points P0 = P1 = P2 = lift_off,
// P4 = P5 = P6 = touch_down, P3 = (mid_x, mid_y, (64 z_mid - 22 z0 - 22 zf) / 20), z_mid = max(z0, zf) + step_height
// (Python's max: zf if zf > z0, else z0).  Each Bernstein term is comb * s^i * (1 - s)^(6 - i) left to right, the
// derivative terms as BEZ:151-187 writes them, and the three sums start from 0.0 and add i = 0..6 in order.
YAW_HD inline void stc_bezier_ref(double step_height, double swing_period, double t, const double* lo,
                                  const double* td, double* pos, double* vel, double* acc) {
#pragma clang fp contract(off)
    const double s = stc_clip(t / swing_period, 0.0, 1.0);
    const double u = 1.0 - s;
    double sp[7], up[7];  // s^k, (1 - s)^k
    sp[0] = 1.0, up[0] = 1.0;
    for (int k = 1; k < 7; ++k) {
        sp[k] = sp[k - 1] * s;
        up[k] = up[k - 1] * u;
    }
    const double z0 = lo[2], zf = td[2];
    const double z_mid = (zf > z0 ? zf : z0) + step_height;
    const double p3[3] = {0.5 * (lo[0] + td[0]), 0.5 * (lo[1] + td[1]), ((64.0 * z_mid - 22.0 * z0) - 22.0 * zf) / 20.0};
    const double comb[7] = {1.0, 6.0, 15.0, 20.0, 15.0, 6.0, 1.0};
    double p[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 7; ++i) {
        const int n = 6;
        const double c = comb[i];
        const double b = (c * sp[i]) * up[n - i];
        double db = 0.0;
        if (i > 0) db = db + (((double)i * c) * sp[i - 1]) * up[n - i];
        if (i < n) db = db - (((double)(n - i) * c) * sp[i]) * up[n - i - 1];
        double d2b = 0.0;
        if (i >= 2) d2b = d2b + (((double)(i * (i - 1)) * c) * sp[i - 2]) * up[n - i];
        if (i >= 1 && i < n) d2b = d2b - (((double)(2 * i * (n - i)) * c) * sp[i - 1]) * up[n - i - 1];
        if (i < n - 1) d2b = d2b + (((double)((n - i) * (n - i - 1)) * c) * sp[i]) * up[n - i - 2];
        const double* cp = i < 3 ? lo : i == 3 ? p3 : td;
        for (int k = 0; k < 3; ++k) {
            p[k] = p[k] + b * cp[k];
            v[k] = v[k] + db * cp[k];
            a[k] = a[k] + d2b * cp[k];
        }
    }
    const double t2 = swing_period * swing_period;
    for (int k = 0; k < 3; ++k) {
        pos[k] = p[k];
        vel[k] = v[k] / swing_period;
        acc[k] = a[k] / t2;
    }
}

// EXP:57-113, with its quirks: two cubic Beziers split at half = swing_period / 2 by t <= half, local time
// (t % half) * (1 / half), so t == half evaluates the first curve at 0 and a clock past swing_period (by less than
// dt, STC:124) wraps to the start of the second curve; the apex control points sit at the absolute height
// step_height; velocity and acceleration are derivatives in the local parameter, not rescaled to time.
YAW_HD inline void stc_explicit(double step_height, double swing_period, double t, const double* lo, const double* td,
                                double* pos, double* vel, double* acc) {
#pragma clang fp contract(off)
    const double half = swing_period / 2.0;
    const double factor = 1.0 / half;
    const double mid[3] = {0.5 * (lo[0] + td[0]), 0.5 * (lo[1] + td[1]), step_height};
    double c1[3], c2[3], c3[3], c4[3];
    if (t <= half) {
        for (int k = 0; k < 3; ++k) c1[k] = lo[k], c2[k] = lo[k], c3[k] = lo[k], c4[k] = mid[k];
        c3[2] = step_height;
    } else {
        for (int k = 0; k < 3; ++k) c1[k] = mid[k], c2[k] = td[k], c3[k] = td[k], c4[k] = td[k];
        c2[2] = step_height;
    }
    const double x = factor * stc_pymod(t, half);
    const double u = 1.0 - x;
    const double u2 = u * u, x2 = x * x;
    const double b1 = u2 * u, b2 = (3.0 * x) * u2, b3 = (3.0 * x2) * u, b4 = x2 * x;
    const double d1 = 3.0 * u2, d2 = (6.0 * u) * x, d3 = 3.0 * x2;
    const double a1 = 6.0 * u, a2 = 6.0 * x;
    for (int k = 0; k < 3; ++k) {
        pos[k] = ((b1 * c1[k] + b2 * c2[k]) + b3 * c3[k]) + b4 * c4[k];
        vel[k] = (d1 * (c2[k] - c1[k]) + d2 * (c3[k] - c2[k])) + d3 * (c4[k] - c3[k]);
        acc[k] = a1 * ((c3[k] - 2.0 * c2[k]) + c1[k]) + a2 * ((c4[k] - 2.0 * c3[k]) + c2[k]);
    }
}

// The generator g selects, at clock t.
YAW_HD inline void stc_reference(const srbd_stc* g, double t, const double* lo, const double* td, double* pos,
                                 double* vel, double* acc) {
    if (g->generator == SRBD_SWING_EXPLICIT)
        stc_explicit(g->step_height, g->swing_period, t, lo, td, pos, vel, acc);
    else
        stc_bezier_ref(g->step_height, g->swing_period, t, lo, td, pos, vel, acc);
}

YAW_HD inline void stc_matvec(const double* A, const double* v, double* out) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i) out[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}

YAW_HD inline void stc_matTvec(const double* A, const double* v, double* out) {
#pragma clang fp contract(off)
    for (int j = 0; j < 3; ++j) out[j] = (A[j] * v[0] + A[3 + j] * v[1]) + A[6 + j] * v[2];
}

// The inverse by cofactors over det = a (e i - f h) - b (d i - f g) + c (d h - e g); the zero matrix when det is
// zero or not finite (see the header).
YAW_HD inline void stc_inverse(const double* J, double* inv) {
#pragma clang fp contract(off)
    const double a = J[0], b = J[1], c = J[2], d = J[3], e = J[4], f = J[5], g = J[6], h = J[7], i = J[8];
    const double A = e * i - f * h, B = d * i - f * g, C = d * h - e * g;
    const double det = (a * A - b * B) + c * C;
    if (det == 0.0 || !(fabs(det) <= 1.7976931348623157e308)) {
        for (int k = 0; k < 9; ++k) inv[k] = 0.0;
        return;
    }
    inv[0] = A / det;
    inv[1] = (c * h - b * i) / det;
    inv[2] = (b * f - c * e) / det;
    inv[3] = -B / det;
    inv[4] = (a * i - c * g) / det;
    inv[5] = (c * d - a * f) / det;
    inv[6] = C / det;
    inv[7] = (b * g - a * h) / det;
    inv[8] = (a * e - b * d) / det;
}

// One leg's inputs (3 x 3 row-major matrices, 3-vectors) and outputs; des_joint_vel may be NULL.
struct StcLeg {
    const double *jac, *jac_dot, *mass_matrix, *q_dot, *foot_pos, *foot_vel, *passive, *bias, *grf, *lift_off,
        *touch_down;
    double *tau, *des_foot_pos, *des_foot_vel, *des_joint_vel;
};

// WBI:369-415, :435-465 and STC:73-94 for one leg whose clock (after this step's update) is t.
//   stance (contact != 0): tau = -(J.T @ grf), des_foot_pos = touch_down, des_foot_vel = 0
//   swing  (contact == 0): fb = kp (des_pos - foot_pos) + kd (des_vel - foot_vel), tau = J.T @ fb, and with feedback
//     linearisation tau += ((M @ Jinv) @ ((des_acc + fb) - J_dot @ q_dot)) + h
//   friction compensation, either kind of leg: tau -= passive
//   des_joint_vel = q_dot + clip(Jinv @ des_foot_vel - q_dot, -10, 10)
// gen(pos, vel, acc) is the swing generator at the leg's clock, called for a swing leg only.
template <class Gen>
YAW_HD inline void stc_leg_with(const srbd_stc* g, double contact, const StcLeg& x, const Gen& gen) {
#pragma clang fp contract(off)
    double tau[3], dpos[3], dvel[3], jinv[9];
    stc_inverse(x.jac, jinv);
    if (contact == 0.0) {
        double dacc[3], fb[3], w[3], jq[3], mj[9], lin[3];
        gen(dpos, dvel, dacc);
        for (int k = 0; k < 3; ++k) {
            const double ep = dpos[k] - x.foot_pos[k], ev = dvel[k] - x.foot_vel[k];
            fb[k] = g->position_gain_fb * ep + g->velocity_gain_fb * ev;
        }
        stc_matTvec(x.jac, fb, tau);
        if (g->use_feedback_linearization) {
            stc_matvec(x.jac_dot, x.q_dot, jq);
            for (int k = 0; k < 3; ++k) w[k] = (dacc[k] + fb[k]) - jq[k];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    mj[3 * i + j] = (x.mass_matrix[3 * i] * jinv[j] + x.mass_matrix[3 * i + 1] * jinv[3 + j]) +
                                    x.mass_matrix[3 * i + 2] * jinv[6 + j];
            stc_matvec(mj, w, lin);
            for (int k = 0; k < 3; ++k) tau[k] = tau[k] + (lin[k] + x.bias[k]);
        }
    } else {
        stc_matTvec(x.jac, x.grf, tau);
        for (int k = 0; k < 3; ++k) {
            tau[k] = -tau[k];
            dpos[k] = x.touch_down[k];
            dvel[k] = 0.0;
        }
    }
    if (g->use_friction_compensation)
        for (int k = 0; k < 3; ++k) tau[k] = tau[k] - x.passive[k];
    double jv[3] = {0.0, 0.0, 0.0};
    if (x.des_joint_vel) stc_matvec(jinv, dvel, jv);
    for (int k = 0; k < 3; ++k) {
        x.tau[k] = tau[k];
        x.des_foot_pos[k] = dpos[k];
        x.des_foot_vel[k] = dvel[k];
        if (x.des_joint_vel) x.des_joint_vel[k] = x.q_dot[k] + stc_clip(jv[k] - x.q_dot[k], -10.0, 10.0);
    }
}

// The generator g selects at clock t, as stc_leg_with's hook.
struct StcBezierGen {
    const srbd_stc* g;
    double t;
    const double *lift_off, *touch_down;
    YAW_HD void operator()(double* pos, double* vel, double* acc) const {
        stc_reference(g, t, lift_off, touch_down, pos, vel, acc);
    }
};

YAW_HD inline void stc_leg(const srbd_stc* g, double t, double contact, const StcLeg& x) {
    stc_leg_with(g, contact, x, StcBezierGen{g, t, x.lift_off, x.touch_down});
}

// STC:129-138 from the four clocks: 1 if a swing leg's clock lies strictly inside swing_period / 2 +- interval.
YAW_HD inline int32_t stc_apex(const double* clocks, double swing_period, const double* contact, double interval) {
#pragma clang fp contract(off)
    int32_t apex = 0;
    const double half = swing_period / 2.0;
    for (int l = 0; l < 4; ++l)
        if (contact[l] == 0.0 && clocks[l] > half - interval && clocks[l] < half + interval) apex = 1;
    return apex;
}

// STC:140-146.
YAW_HD inline int32_t stc_full_stance(const double* contact) {
    int32_t stance = 1;
    for (int l = 0; l < 4; ++l)
        if (contact[l] == 0.0) stance = 0;
    return stance;
}

}  // namespace srbd
