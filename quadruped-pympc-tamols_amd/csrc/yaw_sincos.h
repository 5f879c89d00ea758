// yaw_sincos.h -- cos / sin of a yaw on the device, correctly rounded (float64).
// The single-environment calls form a patch's yaw cos / sin on the host (srbd_api.hip tamols_terrain_job,
// terrain_kernel.hip terrain_enqueue: libm's cos / sin); the batched foothold search reads its yaws from device
// memory, and the device library's cos / sin may differ from libm's in the last place.  This one evaluates both in
// double-double (about 100 bits) and rounds once, so it returns the correctly rounded values -- what libm returns
// wherever libm itself rounds correctly.  glibc's cos / sin are within an ulp but not always correctly rounded: over
// 2 x 10^7 yaws in [-700, 700] glibc 2.35 differed from these in 0.3 % (in each case checked against a 300-bit
// evaluation the value here was the nearer one), so for such a yaw the batched patch coordinates differ from the
// single-environment call's in the last place.  srbd_selftest_yaw_sincos is the host twin
// (tests/test_tamols_batch_capi.py compares it with libm).  Plain IEEE float64 operations and fma only, no table: the
// host and the device compute the same bits.
// Range: |yaw| < 2^20 quarter turns (the reduction's products are exact up to there); beyond it the result is
// unspecified.  A non-finite yaw gives NaN, as libm.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define YAW_HD __host__ __device__
#else
#define YAW_HD
#endif

namespace srbd {

struct DD {
    double hi, lo;
};

YAW_HD inline DD dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
YAW_HD inline DD dd_quick(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
YAW_HD inline DD dd_two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
YAW_HD inline DD dd_add(DD a, DD b) {
    DD s = dd_two_sum(a.hi, b.hi);
    const DD t = dd_two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = dd_quick(s.hi, s.lo);
    s.lo += t.lo;
    return dd_quick(s.hi, s.lo);
}
YAW_HD inline DD dd_mul(DD a, DD b) {
    DD p = dd_two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return dd_quick(p.hi, p.lo);
}

// The series of sin(r) / r (cosine == false) or cos(r) (cosine == true) in r2 = r * r, |r| <= pi / 4 (+ a rounding):
// the coefficients (-1)^n / (2n + 1)! or (-1)^n / (2n)!, n < 8 as double-double and the tail n = 8..15 (below 2^-47
// of the sum, so its plain-float64 rounding stays below 2^-100) by a plain Horner walk.  The terms past n = 15 are
// below 2^-110.  One lane evaluates one series, so the sine and the cosine run side by side on two lanes.
YAW_HD inline DD yaw_series(DD r2, bool cosine) {
#pragma clang fp contract(off)
    constexpr DD SH[8] = {{0x1.0000000000000p+0, 0x0.0p+0},
                          {-0x1.5555555555555p-3, -0x1.5555555555555p-57},
                          {0x1.1111111111111p-7, 0x1.1111111111111p-63},
                          {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73},
                          {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},
                          {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80},
                          {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
                          {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97}};
    constexpr DD CH[8] = {{0x1.0000000000000p+0, 0x0.0p+0},
                          {-0x1.0000000000000p-1, 0x0.0p+0},
                          {0x1.5555555555555p-5, 0x1.5555555555555p-59},
                          {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65},
                          {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},
                          {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76},
                          {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
                          {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92}};
    constexpr double ST[8] = {0x1.952c77030ad4ap-49,  -0x1.2f49b46814157p-57, 0x1.71b8ef6dcf572p-66,
                              -0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84,  -0x1.d1ab1c2dccea3p-94,
                              0x1.259f98b4358adp-103, -0x1.434d2e783f5bcp-113};
    constexpr double CT[8] = {0x1.ae7f3e733b81fp-45,  -0x1.6827863b97d97p-53, 0x1.e542ba4020225p-62,
                              -0x1.0ce396db7f853p-70, 0x1.f2cf01972f578p-80,  -0x1.88e85fc6a4e5ap-89,
                              0x1.0a18a2635085dp-98,  -0x1.3932c5047d60ep-108};
    double t = cosine ? CT[7] : ST[7];
#pragma unroll
    for (int n = 6; n >= 0; --n) t = t * r2.hi + (cosine ? CT[n] : ST[n]);
    DD acc = {t, 0.0};
#pragma unroll
    for (int n = 7; n >= 0; --n) acc = dd_add(dd_mul(acc, r2), cosine ? CH[n] : SH[n]);
    return acc;
}

// The reduction: x = k pi / 2 + r, |r| <= pi / 4 (+ a rounding of k), r as a double-double; returns the quadrant k & 3.
// pi / 2 = P1 + P2 + P3 + P4: P1, P2 of 33 bits (k P1, k P2 exact for k < 2^20), P3, P4 of 53.
YAW_HD inline int yaw_reduce(double x, DD& r) {
#pragma clang fp contract(off)
    const double P1 = 0x1.921fb54400000p+0, P2 = 0x1.0b4611a600000p-34, P3 = 0x1.3198a2e037073p-69,
                 P4 = 0x1.129024e088a68p-123;
    double k = rint(x * 0x1.45f306dc9c883p-1);
    k = fabs(k) < 1048576.0 ? k : 0.0;  // past the range: no reduction (the result is unspecified)
    r = dd_two_sum(x, -(k * P1));
    r = dd_add(r, DD{-(k * P2), 0.0});
    DD t = dd_two_prod(k, P3);
    r = dd_add(r, DD{-t.hi, -t.lo});
    t = dd_two_prod(k, P4);
    r = dd_add(r, DD{-t.hi, -t.lo});
    return (int)k & 3;  // two's complement: the quadrant of a negative k too
}

// One of the two values on the calling lane: sin(r) (cosine == false) or cos(r), rounded once.
YAW_HD inline double yaw_series_value(DD r, bool cosine) {
#pragma clang fp contract(off)
    DD v = yaw_series(dd_mul(r, r), cosine);
    if (!cosine) v = dd_mul(v, r);
    return v.hi + v.lo;
}

// From sin(r), cos(r) and the quadrant: c = cos(x), s = sin(x).  A zero keeps libm's values (sin keeps the zero's
// sign), a non-finite x gives NaN.
YAW_HD inline void yaw_finish(double x, int q, double sv, double cv, double& c, double& s) {
    if (!(fabs(x) <= 1.79769313486231570815e308)) {
        c = s = x - x;
    } else if (x == 0.0) {
        c = 1.0;
        s = x;
    } else {
        s = q == 0 ? sv : q == 1 ? cv : q == 2 ? -sv : -cv;
        c = q == 0 ? cv : q == 1 ? -sv : q == 2 ? -cv : sv;
    }
}

// c = cos(x), s = sin(x) on one lane (the host twin: srbd_selftest_yaw_sincos).
YAW_HD inline void yaw_sincos(double x, double& c, double& s) {
    DD r;
    const int q = yaw_reduce(x, r);
    yaw_finish(x, q, yaw_series_value(r, false), yaw_series_value(r, true), c, s);
}

}  // namespace srbd
