// srbd_terrain.h -- the velocity modulator, the terrain estimator and the assembly of the reference row's first twelve
// entries, for the host functions (srbd_host.cpp srbd_vm_modulate, srbd_terrain_estimate, srbd_reference_assemble)
// and the device kernels (srbd_producers.hip vm_modulate_kernel, terrain_ref_step_kernel).  Both sides compile these
// same float64 operations unfused; cos / sin of the yaw, roll and pitch come from yaw_sincos.h and the arctangent from
// terr_atan below, which calls neither libm nor the device library, so both sides leave the same bits.
//   VM  = quadruped_pympc/helpers/velocity_modulator.py
//   TE  = quadruped_pympc/helpers/terrain_estimator.py
//   WBI = quadruped_pympc/interfaces/wb_interface.py
// The work of one environment is cut into pieces one lane of a quad can own: one foot rotation (terr_rotate), one
// slope with its arctangent (terr_slope), one sin or cos series, and the filter (terr_filter) on the lane that owns
// the state.  The host runs the same pieces in a loop.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "yaw_sincos.h"

namespace srbd {

// arctan(x) for x >= 0, +inf and NaN included (a negative x is not supported: the estimator passes a quotient of
// absolute values).  Plain IEEE add, multiply and divide in the order written, no fma, no library call.
// The reduction is the classical one to |t| <= 7 / 16 around the points 0.5, 1, 1.5 and infinity,
//   arctan(x) = arctan(c) + arctan((x - c) / (1 + c x)),   arctan(x) = pi / 2 - arctan(1 / x),
// with arctan(c) held as a float64 pair, and arctan(t) = t - t z Q(z), z = t^2, where Q interpolates
// (t - arctan t) / t^3 on [0, (7 / 16)^2] at 14 Chebyshev points (its rounded coefficients leave |Q error| < 2^-55,
// below 2^-58 of the result).  The break points are 7/16, 11/16, 19/16 and 39/16; below 2^-27 arctan(x) rounds to x,
// from 2^66 on to pi / 2.  The result is within 1 ulp of the true value (measured: tests/test_terrain_host.py), so
// it differs from a correctly rounded arctan by at most one place.
YAW_HD inline double terr_atan(double x) {
#pragma clang fp contract(off)
    constexpr double Q[14] = {0x1.5555555555555p-2,  -0x1.9999999999999p-3, 0x1.24924924923eep-3,  -0x1.c71c71c711a38p-4,
                              0x1.745d1742da9b5p-4,  -0x1.3b13b0be12b6cp-4, 0x1.111103af625edp-4,  -0x1.e1dfedfd40214p-5,
                              0x1.af0eda9128d5ep-5,  -0x1.852a773c8cf17p-5, 0x1.5e04a6f09af0ep-5,  -0x1.2af76bc83e5f3p-5,
                              0x1.a6b94e339b7f2p-6,  -0x1.5d55d08f9de57p-7};
    constexpr double PIO2_HI = 0x1.921fb54442d18p+0, PIO2_LO = 0x1.1a62633145c07p-54;
    if (x != x) return x + x;
    if (x >= 0x1p66) return PIO2_HI + PIO2_LO;
    double t, hi, lo;
    bool reduced = true;
    if (x < 0.4375) {
        if (x < 0x1p-27) return x;
        t = x, hi = 0.0, lo = 0.0;
        reduced = false;
    } else if (x < 0.6875) {
        t = (2.0 * x - 1.0) / (2.0 + x);
        hi = 0x1.dac670561bb4fp-2, lo = 0x1.a2b7f222f65e2p-56;
    } else if (x < 1.1875) {
        t = (x - 1.0) / (x + 1.0);
        hi = 0x1.921fb54442d18p-1, lo = 0x1.1a62633145c07p-55;
    } else if (x < 2.4375) {
        t = (x - 1.5) / (1.0 + 1.5 * x);
        hi = 0x1.f730bd281f69bp-1, lo = 0x1.007887af0cbbdp-56;
    } else {
        t = -1.0 / x;
        hi = PIO2_HI, lo = PIO2_LO;
    }
    // Q(z) as its even and its odd half in w = z^2: two Horner walks of seven side by side
    const double z = t * t, w = z * z;
    double even = Q[12], odd = Q[13];
#pragma unroll
    for (int n = 10; n >= 0; n -= 2) {
        even = even * w + Q[n];
        odd = odd * w + Q[n + 1];
    }
    const double p = z * (even + z * odd);
    if (!reduced) return t - t * p;
    return hi - ((t * p - lo) - t);
}

// VM:20-31, one leg: sqrt(square(dx) + square(dy)) of foot minus hip.
YAW_HD inline double vm_distance(const double* foot, const double* hip) {
#pragma clang fp contract(off)
    const double dx = foot[0] - hip[0], dy = foot[1] - hip[1];
    return sqrt(dx * dx + dy * dy);
}

// VM:33-35: the reference's "not moving" test, without abs: a negative command counts as standing, a NaN as moving.
YAW_HD inline bool vm_standing(const double* lin) { return lin[0] < 0.01 && lin[1] < 0.01; }

// VM:37-46 from the four strict comparisons' disjunction: products with 0.0 on a hit (a negative entry becomes -0.0,
// a NaN stays), the command itself otherwise.
YAW_HD inline double vm_entry(double v, bool standing, bool beyond) {
#pragma clang fp contract(off)
    return (!standing && beyond) ? v * 0.0 : v;
}

// TE:40-52: R_W2H @ (foot - base) for one foot, each row's three products summed left to right, the products with
// the matrix's zeros and its one included: a NaN or an infinity in one coordinate reaches the others as in NumPy.
YAW_HD inline void terr_rotate(const double* foot, const double* base, double c, double s, double* out) {
#pragma clang fp contract(off)
    const double x = foot[0] - base[0], y = foot[1] - base[1], z = foot[2] - base[2];
    out[0] = (c * x + s * y) + 0.0 * z;
    out[1] = (-s * x + c * y) + 0.0 * z;
    out[2] = (0.0 * x + 0.0 * y) + 1.0 * z;
}

// TE:49-64: the four differences of rotated feet (legs FL FR RL RR) are a - b with
//   k = 0 left  = FL - RL over x    k = 1 right = FR - RR over x      (the pitch pair)
//   k = 2 front = FL - FR over y    k = 3 back  = RL - RR over y      (the roll pair)
YAW_HD inline void terr_pair(int k, int& a, int& b) {
    a = (k == 1) ? 1 : (k == 3) ? 2 : 0;
    b = (k == 0) ? 2 : (k == 2) ? 1 : 3;
}

// Difference k of the rotated feet ra, rb (terr_pair's legs) and its slope angle: dz receives the difference's z; the
// angle is arctan(|dz| / |d + 0.001|), d the difference's x (k < 2) or y: x / 0 is inf and its arctangent pi / 2,
// 0 / 0 is NaN.
YAW_HD inline double terr_slope(int k, const double* ra, const double* rb, double& dz) {
#pragma clang fp contract(off)
    const double d = k < 2 ? ra[0] - rb[0] : ra[1] - rb[1];
    dz = ra[2] - rb[2];
    return terr_atan(fabs(dz) / fabs(d + 0.001));
}

// TE:56-103 from the four angles and z differences (terr_slope's order) and the four feet's world z: the two means,
// the two sign tests and the three filters, into the state.
YAW_HD inline void terr_filter(srbd_terrain_est* g, const double* angle, const double* dz, const double* foot_z) {
#pragma clang fp contract(off)
    double pitch = (angle[0] + angle[1]) * 0.5;
    double roll = (angle[2] + angle[3]) * 0.5;
    if (dz[2] * 0.5 + dz[3] * 0.5 < 0.0) roll = -roll;
    if (dz[0] * 0.5 + dz[1] * 0.5 > 0.0) pitch = -pitch;
    g->roll = g->roll_activated ? g->roll * 0.99 + roll * 0.01 : 0.0;
    g->pitch = g->pitch_activated ? g->pitch * 0.99 + pitch * 0.01 : 0.0;
    const double mean = (((foot_z[0] + foot_z[1]) + foot_z[2]) + foot_z[3]) / 4.0;
    g->height = g->height * 0.2 + mean * 0.8;
}

// WBI:258-291 from the filtered roll, pitch and height and their cos / sin (cr, sr, cp, sp): ref_position,
// ref_linear_velocity, ref_orientation and ref_angular_velocity, entries 0..11 of the reference row.  The rotation
// is Ry(pitch) Rx(roll) = [[cp, sp sr, sp cr], [0, cr, -sr], [-sp, cp sr, cp cr]] (scipy's from_euler("xyz", [roll,
// pitch, 0]) to rounding), each row times the command summed left to right; then the sign flip for pitch > 0 and
// the halving of x and doubling of z for |pitch| > 0.2, in that order.
YAW_HD inline void terr_assemble(double roll, double pitch, double height, double cr, double sr, double cp, double sp,
                                 double ref_z, double base_z, double com_z, double com_off_z, const double* lin,
                                 const double* ang, double* out) {
#pragma clang fp contract(off)
    double pz = ref_z + height;
    double v0 = (cp * lin[0] + (sp * sr) * lin[1]) + (sp * cr) * lin[2];
    const double v1 = (0.0 * lin[0] + cr * lin[1]) + -sr * lin[2];
    double v2 = (-sp * lin[0] + (cp * sr) * lin[1]) + (cp * cr) * lin[2];
    if (pitch > 0.0) v2 = -v2;
    if (fabs(pitch) > 0.2) {
        v0 = v0 / 2.0;
        v2 = v2 * 2.0;
    }
    pz = pz - (base_z - (com_z + com_off_z));
    out[0] = 0.0, out[1] = 0.0, out[2] = pz;
    out[3] = v0, out[4] = v1, out[5] = v2;
    out[6] = roll, out[7] = pitch, out[8] = 0.0;
    out[9] = ang[0], out[10] = ang[1], out[11] = ang[2];
}

}  // namespace srbd
