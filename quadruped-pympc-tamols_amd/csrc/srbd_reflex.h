// srbd_reflex.h -- the swing reflex of the leg controller, one leg at a time, for the host functions (srbd_host.cpp
// srbd_reflex_*) and the device kernel (reflex_kernel.hip reflex_step_kernel): the early-stance detector and the
// 'scipy' swing generator, the one generator that reads what the detector finds.  Both sides compile these same
// float64 operations unfused, in the order written here; the only libm calls are sqrt and fabs (correctly rounded on
// both sides), so they leave the same bits.
//   ESD = quadruped_pympc/helpers/early_stance_detector.py (update_detection :36-128)
//   SCI = quadruped_pympc/helpers/swing_generators/scipy_swing_trajectory_generator.py (createCurve :25-94,
//         compute_trajectory_references :96-122)
//   WBI = quadruped_pympc/interfaces/wb_interface.py (compute_stance_and_swing_torque :362-408)
// The spline.  SCI builds three scipy CubicSpline(t, y, bc_type=["clamped", "clamped"]) over five knots.  With end
// derivatives s0 = s4 = 0 scipy's banded system reduces to the 3 x 3 tridiagonal one for the interior knot derivatives
//   dx[i] s[i-1] + 2 (dx[i-1] + dx[i]) s[i] + dx[i-1] s[i+1] = 3 (dx[i] m[i-1] + dx[i-1] m[i]),  i = 1..3,
// dx[i] = t[i+1] - t[i], m[i] = (y[i+1] - y[i]) / dx[i].  Here it is solved without pivoting in this order:
//   d1 = 2 (dx0 + dx1), d2 = 2 (dx1 + dx2), d3 = 2 (dx2 + dx3)
//   w2 = dx2 / d1, e2 = d2 - w2 dx0, w3 = dx3 / e2, e3 = d3 - w3 dx1            (once, shared by the three axes)
//   b[i] = 3 (dx[i] m[i-1] + dx[i-1] m[i]);  c2 = b2 - w2 b1;  c3 = b3 - w3 c2
//   s3 = c3 / e3;  s2 = (c2 - dx1 s3) / e2;  s1 = (b1 - dx0 s2) / d1
// (the matrix is strictly diagonally dominant for increasing knots, so no pivot is needed; LAPACK's pivoted solve
// agrees to rounding).  The cubic of interval i is scipy's: q = ((s[i] + s[i+1]) - 2 m[i]) / dx[i], c0 = q / dx[i],
// c1 = (m[i] - s[i]) / dx[i] - q, c2 = s[i], c3 = y[i], and with u = x - t[i] the three values are summed from the
// constant term up, the power of u accumulated by repeated multiplication, as PPoly evaluates them:
//   pos = ((c3 + c2 u) + c1 u^2) + c0 u^3;  vel = (c2 + (2 c1) u) + (3 c0) u^2;  acc = (2 c1) + (2 (3 c0)) u
// Intervals are half-open and the last one closed; outside the knots the first or the last interval extrapolates, so a
// clock that has passed swing_period by less than dt uses the last interval.  A NaN clock gives NaN.
// Deviation: with a hit recorded and swing_period - hitmoment not positive (possible only after a re-timing shortened
// the swing; or not a number) the knots are not increasing and scipy raises.  Here that leg takes the no-hit curve from
// lift_off for that tick; its detector state is left alone.  NaN values flow through where scipy raises on them.
// Out of scope: the 'geom_contact' trigger (it reads MuJoCo contact lists): refused.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "srbd_stc.h"
#include "yaw_sincos.h"

namespace srbd {

YAW_HD inline bool reflex_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// What srbd_reflex_step refuses in the two structs: a swing_period that is not positive and finite (the generator code
// of the srbd_stc is not read here), an unknown or unsupported trigger mode, a reflex_max_step_height that is not
// finite.
YAW_HD inline bool reflex_structs_ok(const srbd_stc* g, const srbd_reflex* r) {
    const bool period = g->swing_period > 0.0 && reflex_finite(g->swing_period);
    const bool mode = r->trigger_mode == SRBD_REFLEX_OFF || r->trigger_mode == SRBD_REFLEX_TRACKING;
    return period && mode && reflex_finite(r->reflex_max_step_height);
}

// np.linalg.norm of three components.
YAW_HD inline double reflex_norm3(const double* v) {
#pragma clang fp contract(off)
    return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// One leg's words of the detector, held in registers between the load and the store.
struct ReflexLeg {
    double hitmoment, hitpoint[3];
    int32_t has_hitpoint, early_stance;
};

YAW_HD inline void reflex_leg_load(const srbd_reflex* r, int l, ReflexLeg& s) {
    s.hitmoment = r->hitmoments[l];
    for (int k = 0; k < 3; ++k) s.hitpoint[k] = r->hitpoints[l][k];
    s.has_hitpoint = r->has_hitpoint[l];
    s.early_stance = r->early_stance[l];
}

YAW_HD inline void reflex_leg_store(srbd_reflex* r, int l, const ReflexLeg& s) {
    r->hitmoments[l] = s.hitmoment;
    for (int k = 0; k < 3; ++k) r->hitpoints[l][k] = s.hitpoint[k];
    r->has_hitpoint[l] = s.has_hitpoint;
    r->early_stance[l] = s.early_stance;
}

// hitmoments = -1.0, hitpoints = None (the three doubles are zeroed so that the struct's bytes do not depend on the
// hit that was cleared).
YAW_HD inline void reflex_leg_clear_hit(ReflexLeg& s) {
    s.hitmoment = -1.0;
    s.has_hitpoint = 0;
    for (int k = 0; k < 3; ++k) s.hitpoint[k] = 0.0;
}

// ESD:53-88, one leg's pass through the loop body, on the leg's words `s`.  Returns true if the leg triggers (ESD:76-80:
// the `break`, which ends the tick for the legs after it; the caller leaves those untouched and sets the cycle counter
// to 0).  swing_time is the leg's clock before this tick's update, des the desired foot position the previous tick
// wrote.  The `continue`s of ESD:65 and :68 skip the clean-up of :86-88: a stance leg keeps its hit moment and point.
YAW_HD inline bool reflex_leg_detect(const srbd_reflex* r, ReflexLeg& s, double swing_time, double swing_period,
                                     double contact, const double* foot, const double* des, const double* lift_off,
                                     const double* touch_down) {
#pragma clang fp contract(off)
    if (r->trigger_mode != SRBD_REFLEX_TRACKING) {  // ESD:53-57, not activated
        s.early_stance = 0;
        reflex_leg_clear_hit(s);
        return false;
    }
    if (contact == 1.0) {  // :63-65
        s.early_stance = 0;
        return false;
    }
    if (s.early_stance == 0 && swing_time > swing_period - r->early_stance_time_threshold) {  // :66-68
        s.early_stance = 0;
        return false;
    }
    if (s.early_stance == 0) {  // :70-84
        double disp[3], local[3];
        for (int k = 0; k < 3; ++k) {
            disp[k] = touch_down[k] - lift_off[k];
            local[k] = des[k] - foot[k];
        }
        const double nl = reflex_norm3(local), nd = reflex_norm3(disp);
        if (nl / nd > r->relative_tracking_error_threshold && nl > r->absolute_min_distance_error_threshold) {
            for (int k = 0; k < 3; ++k) s.hitpoint[k] = foot[k];
            s.has_hitpoint = 1;
            s.hitmoment = swing_time;
            s.early_stance = 1;
            return true;
        }
        s.early_stance = 0;
        reflex_leg_clear_hit(s);
    }
    if (s.early_stance == 0) reflex_leg_clear_hit(s);  // :86-88
    return false;
}

// ESD:118-128 on the cycle counter (after a trigger has set it to 0): at most one touch-down edge of the tick counts,
// and only while the counter is >= 0; the flag is 0 <= cycles < max, else the counter returns to -1.  Only with the
// enhancement switched on; otherwise the flag is left as it is.  cycles and flag come in as the previous tick left
// them (the device lanes load them before lane 0 stores) and go out as this tick leaves them.
YAW_HD inline void reflex_cycles(const srbd_reflex* r, bool triggered, const double* contact, const double* previous,
                                 int32_t& cycles, int32_t& flag) {
    if (triggered) cycles = 0;  // ESD:79
    if (!r->use_height_enhancement) return;
    for (int l = 0; l < 4; ++l)
        if (contact[l] == 1.0 && previous[l] == 0.0 && cycles >= 0) {
            cycles = cycles + 1;
            break;
        }
    if (cycles >= 0 && cycles < r->max_gait_cycles) {
        flag = 1;
    } else {
        flag = 0;
        cycles = -1;
    }
}

// a[i] of four / five values by comparisons, so that the arrays stay in registers.
YAW_HD inline double reflex_pick4(int i, double a0, double a1, double a2, double a3) {
    return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : a3;
}

// One axis of the clamped five-knot spline at interval i, local coordinate u (see the header).
struct ReflexSplineLhs {
    double dx[4], d1, w2, e2, w3, e3;
};

YAW_HD inline void reflex_spline_lhs(const double* t, ReflexSplineLhs& a) {
#pragma clang fp contract(off)
    for (int i = 0; i < 4; ++i) a.dx[i] = t[i + 1] - t[i];
    a.d1 = 2.0 * (a.dx[0] + a.dx[1]);
    const double d2 = 2.0 * (a.dx[1] + a.dx[2]), d3 = 2.0 * (a.dx[2] + a.dx[3]);
    a.w2 = a.dx[2] / a.d1;
    a.e2 = d2 - a.w2 * a.dx[0];
    a.w3 = a.dx[3] / a.e2;
    a.e3 = d3 - a.w3 * a.dx[1];
}

YAW_HD inline void reflex_spline_axis(const ReflexSplineLhs& a, const double* y, int i, double u, double& pos,
                                      double& vel, double& acc) {
#pragma clang fp contract(off)
    const double m0 = (y[1] - y[0]) / a.dx[0], m1 = (y[2] - y[1]) / a.dx[1], m2 = (y[3] - y[2]) / a.dx[2],
                 m3 = (y[4] - y[3]) / a.dx[3];
    const double b1 = 3.0 * (a.dx[1] * m0 + a.dx[0] * m1), b2 = 3.0 * (a.dx[2] * m1 + a.dx[1] * m2),
                 b3 = 3.0 * (a.dx[3] * m2 + a.dx[2] * m3);
    const double c2 = b2 - a.w2 * b1;
    const double c3 = b3 - a.w3 * c2;
    const double s3 = c3 / a.e3;
    const double s2 = (c2 - a.dx[1] * s3) / a.e2;
    const double s1 = (b1 - a.dx[0] * s2) / a.d1;
    const double sl = reflex_pick4(i, 0.0, s1, s2, s3), sr = reflex_pick4(i, s1, s2, s3, 0.0);
    const double m = reflex_pick4(i, m0, m1, m2, m3), h = reflex_pick4(i, a.dx[0], a.dx[1], a.dx[2], a.dx[3]);
    const double q = ((sl + sr) - 2.0 * m) / h;
    const double k0 = q / h, k1 = (m - sl) / h - q, k2 = sl, k3 = reflex_pick4(i, y[0], y[1], y[2], y[3]);
    const double v0 = 3.0 * k0, v1 = 2.0 * k1;  // derivative(): c[:-1] * (3, 2, 1)
    const double a0 = 2.0 * v0;                 // and again: * (2, 1)
    const double u2 = u * u, u3 = u2 * u;
    pos = ((k3 + k2 * u) + k1 * u2) + k0 * u3;
    vel = (k2 + v1 * u) + v0 * u2;
    acc = v1 + a0 * u;
}

// SCI:25-122 for one leg at clock x: the knots of createCurve, then the three splines.  `flag` is the generator's
// reflex_next_steps_height_enhancement as this tick's detector left it.
YAW_HD inline void reflex_reference(const srbd_stc* g, const srbd_reflex* r, const ReflexLeg& s, int32_t flag, double x,
                                    const double* lift_off, const double* touch_down, double* pos, double* vel,
                                    double* acc) {
#pragma clang fp contract(off)
    const double T = g->swing_period;
    const double updated = T - s.hitmoment;  // SCI:45
    // SCI:98-102, :29; and the header's deviation
    const bool from_hit = s.has_hitpoint != 0;
    bool reflex = from_hit && s.hitmoment != -1.0;
    const bool degenerate = reflex && !(updated > 0.0);
    if (degenerate) reflex = false;
    double x0[3];
    for (int k = 0; k < 3; ++k) x0[k] = (from_hit && !degenerate) ? s.hitpoint[k] : lift_off[k];
    const double* xf = touch_down;
    double t[5], y[3][5];
    if (reflex) {  // SCI:30-46
        const double hmax = r->reflex_max_step_height;
        const double low = g->step_height / 1.5, high = hmax / 1.5;
        for (int k = 0; k < 2; ++k) {
            y[k][0] = x0[k];
            y[k][1] = (x0[k] - 0.01 * (xf[k] - x0[k])) + 0.0;
            y[k][2] = 0.5 * (x0[k] + xf[k]) + 0.0;
            y[k][3] = (0.2 * x0[k] + 0.8 * xf[k]) + 0.0;
            y[k][4] = y[k][3];
        }
        y[2][0] = x0[2];
        y[2][1] = x0[2] + low;
        y[2][2] = 0.5 * (x0[2] + xf[2]) + hmax;
        y[2][3] = (0.2 * x0[2] + 0.8 * xf[2]) + high;
        y[2][4] = r->blind ? xf[2] + hmax / 2.0 : xf[2];
        t[0] = s.hitmoment;
        t[1] = s.hitmoment + updated / 4.0;
        t[2] = s.hitmoment + updated / 2.0;
        t[3] = s.hitmoment + (updated * 3.0) / 4.0;
        t[4] = T;
    } else {  // SCI:49-61
        const double height = flag ? r->reflex_max_step_height : g->step_height;
        const double low = height / 1.5;
        for (int k = 0; k < 2; ++k) {
            y[k][0] = x0[k];
            y[k][1] = x0[k] + 0.0;
            y[k][2] = 0.5 * (x0[k] + xf[k]) + 0.0;
            y[k][3] = xf[k] + 0.0;
            y[k][4] = xf[k];
        }
        y[2][0] = x0[2];
        y[2][1] = x0[2] + low;
        y[2][2] = 0.5 * (x0[2] + xf[2]) + height;
        y[2][3] = xf[2] + low;
        y[2][4] = xf[2];
        const double half = T / 2.0;
        t[0] = 0.0;
        t[1] = half / 2.0;
        t[2] = half;
        t[3] = (half * 3.0) / 2.0;
        t[4] = half * 2.0;
    }
    // the interval that holds x: half-open, the last one closed, the ends extrapolate; a NaN x takes interval 0 and
    // gives NaN
    const int i = x >= t[3] ? 3 : x >= t[2] ? 2 : x >= t[1] ? 1 : 0;
    const double u = x - reflex_pick4(i, t[0], t[1], t[2], t[3]);
    ReflexSplineLhs a;
    reflex_spline_lhs(t, a);
    for (int k = 0; k < 3; ++k) reflex_spline_axis(a, y[k], i, u, pos[k], vel[k], acc[k]);
}

// stc_leg_with's hook: the spline generator at the leg's clock.
struct ReflexSplineGen {
    const srbd_stc* g;
    const srbd_reflex* r;
    ReflexLeg s;
    int32_t flag;
    double t;
    const double *lift_off, *touch_down;
    YAW_HD void operator()(double* pos, double* vel, double* acc) const {
        reflex_reference(g, r, s, flag, t, lift_off, touch_down, pos, vel, acc);
    }
};

}  // namespace srbd
