// srbd_quad.h -- the four-lane sample layout shared by the rollout and merge translation units
// (srbd_kernels.hip, srbd_batch.hip): lane constants, DPP quad permutations, the rigid-body step.
#pragma once

#include "srbd_device.h"

namespace srbd {

// ---- four lanes per sample: lane c in {0,1,2} owns component c (x, y, z) of every 3-vector of
// the model (forces per leg, torques, p, v, rpy, omega); lane 3 mirrors lane 2.  Cross-lane data
// moves are DPP quad permutations.  Every float operation is the one the thread-per-sample kernel
// performs, in the same order, so both kernels give bitwise identical costs; the 4x wave count
// and ~1.6x shorter per-lane instruction stream cut the latency when N is too small to fill
// the GPU one sample per lane.
constexpr int QP_B0 = 0x00, QP_B1 = 0x55, QP_B2 = 0xAA;  // quad_perm broadcast of lane 0/1/2
constexpr int QP_NEXT = 0x09;   // lanes (0,1,2,3) <- (1,2,0,0): component c+1 (mod 3)
constexpr int QP_NEXT2 = 0x52;  // lanes (0,1,2,3) <- (2,0,1,1): component c+2 (mod 3)
constexpr int QP_XOR1 = 0xB1;   // lanes (0,1,2,3) <- (1,0,3,2)
constexpr int QP_XOR2 = 0x4E;   // lanes (0,1,2,3) <- (2,3,0,1)

#ifndef SRBD_XS
#define SRBD_XS 0  // experiment knob: quad permutations through ds_swizzle (the LDS crossbar) instead of DPP
#endif
#ifndef SRBD_PRIO
#define SRBD_PRIO 0  // experiment knob: s_setprio of the rollout blocks' waves (the draw blocks stay at 0)
#endif
#ifndef SRBD_PRIO_MIN
#define SRBD_PRIO_MIN 0  // ... for launches of at least this many rollout blocks
#endif
template <int CTRL>
__device__ __forceinline__ float qp(float v) {
#if SRBD_XS
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x8000 | CTRL));
#else
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
#endif
}
__device__ __forceinline__ float sel3(int c, float a0, float a1, float a2) { return c == 0 ? a0 : (c == 1 ? a1 : a2); }

// Lane constants of the four-lane layout: lane c in {0,1,2} owns component c, lane 3 mirrors lane 2.
struct QuadLane {
    int c;
    float g, Ir0, Ir1, Ir2, Ii0, Ii1, Ii2;
};
// kc: the model constants' view (srbd_core.h KView: the shared ModelConst or one environment's EnvModel)
template <class KC>
__device__ __forceinline__ QuadLane quad_lane(const KC& kc, int c) {
    const float* inertia = kc.inertia();
    const float* Iinv = kc.Iinv();
    QuadLane L;
    L.c = c;
    L.g = c == 2 ? -9.81f : 0.0f;
    L.Ir0 = sel3(c, inertia[0], inertia[3], inertia[6]);
    L.Ir1 = sel3(c, inertia[1], inertia[4], inertia[7]);
    L.Ir2 = sel3(c, inertia[2], inertia[5], inertia[8]);
    L.Ii0 = sel3(c, Iinv[0], Iinv[3], Iinv[6]);
    L.Ii1 = sel3(c, Iinv[1], Iinv[4], Iinv[7]);
    L.Ii2 = sel3(c, Iinv[2], Iinv[5], Iinv[8]);
    return L;
}

// One explicit-Euler step of the single rigid body (Centroidal_Model_JAX.fd + integrate_jax,
// CMJ:93-174) in the four-lane layout, from this lane's component of the contact-weighted force sum
// `temp` = sum_i f_i c_i and torque sum `temp2` = sum_i (p_i - p_com) x f_i c_i.  The float ops and
// their order are those of integrate() in srbd_core.h (rollout_kernel), so both layouts agree bit
// for bit.  All four lanes of each quad must be active (DPP quad permutations).
// Split in two so the merge tail can form the state-only part (rotation, Euler rates, gyroscopic
// term) while the weighted sums are still being reduced: quad_rb_prep needs only r and w,
// quad_rb_apply adds the forces.  quad_rigid_body = apply(prep); the float ops are unchanged.
struct QuadRB {
    float er, R0, R1, R2, a1;
};
__device__ __forceinline__ QuadRB quad_rb_prep(const QuadLane& L, float r, float w) {
    const int c = L.c;
    float sn, cs;
    sincos_(r, &sn, &cs);
    const float sr = qp<QP_B0>(sn), cr = qp<QP_B0>(cs);
    const float sp = qp<QP_B1>(sn), cp = qp<QP_B1>(cs);
    const float sy = qp<QP_B2>(sn), cy = qp<QP_B2>(cs);
    const float w0 = qp<QP_B0>(w), w1 = qp<QP_B1>(w), w2 = qp<QP_B2>(w);
    float k1, k2;
    euler_rate_coefs(c, sr, cr, sp, cp, k1, k2);
    // euler_rate_row, with both operands of every lane select computed first (straight-line code:
    // selects, not divergent branches)
    const float kw1 = k1 * w1;
    const float er0 = w0 + kw1;
    const float er = (c == 0 ? er0 : kw1) + k2 * w2;
    // row c of b_R_w (CMJ:136-150)
    const float A = c == 1 ? sr : cr;
    const float B0 = c == 1 ? -cr : sr, B1 = c == 1 ? cr : -sr;
    const float Asp = A * sp;
    const float r0a = cp * cy, r0b = Asp * cy + B0 * sy;
    const float r1a = cp * sy, r1b = Asp * sy + B1 * cy;
    const float r2b = A * cp;
    const float R0 = c == 0 ? r0a : r0b;
    const float R1 = c == 0 ? r1a : r1b;
    const float R2 = c == 0 ? -sp : r2b;
    const float Iw = L.Ir0 * w0 + L.Ir1 * w1 + L.Ir2 * w2;
    const float wx = (-qp<QP_NEXT2>(w)) * qp<QP_NEXT>(Iw) + qp<QP_NEXT>(w) * qp<QP_NEXT2>(Iw);
    const float a1 = L.Ii0 * qp<QP_B0>(wx) + L.Ii1 * qp<QP_B1>(wx) + L.Ii2 * qp<QP_B2>(wx);
    return QuadRB{er, R0, R1, R2, a1};
}
template <class KC>
__device__ __forceinline__ void quad_rb_apply(const KC& kc, const QuadLane& L, const QuadRB& q, float temp,
                                              float temp2, float dt, float& p, float& v, float& r, float& w) {
    const float lin = kc.inv_m() * temp + L.g;
    const float Rt = q.R0 * qp<QP_B0>(temp2) + q.R1 * qp<QP_B1>(temp2) + q.R2 * qp<QP_B2>(temp2);
    const float a2 = L.Ii0 * qp<QP_B0>(Rt) + L.Ii1 * qp<QP_B1>(Rt) + L.Ii2 * qp<QP_B2>(Rt);
    const float aa = -q.a1 + a2;
    const float pn = p + v * dt, vn = v + lin * dt, rn = r + q.er * dt, wn = w + aa * dt;
    p = pn;
    v = vn;
    r = rn;
    w = wn;
}
// quad_rb_apply with the torque sum's three components already on every lane (the leg-parallel force phase):
// the same float operations, no broadcasts.
template <class KC>
__device__ __forceinline__ void quad_rb_apply3(const KC& kc, const QuadLane& L, const QuadRB& q, float temp,
                                               float t2x, float t2y, float t2z, float dt, float& p, float& v, float& r,
                                               float& w) {
    const float lin = kc.inv_m() * temp + L.g;
    const float Rt = q.R0 * t2x + q.R1 * t2y + q.R2 * t2z;
    const float a2 = L.Ii0 * qp<QP_B0>(Rt) + L.Ii1 * qp<QP_B1>(Rt) + L.Ii2 * qp<QP_B2>(Rt);
    const float aa = -q.a1 + a2;
    const float pn = p + v * dt, vn = v + lin * dt, rn = r + q.er * dt, wn = w + aa * dt;
    p = pn;
    v = vn;
    r = rn;
    w = wn;
}
template <class KC>
__device__ __forceinline__ void quad_rigid_body(const KC& kc, const QuadLane& L, float temp, float temp2,
                                                float dt, float& p, float& v, float& r, float& w) {
    quad_rb_apply(kc, L, quad_rb_prep(L, r, w), temp, temp2, dt, p, v, r, w);
}

// This lane's component of (p_i - p_com) x f_i (jnp.dot(skew(v), f), CMJ:100-101, zero terms dropped).
__device__ __forceinline__ float quad_cross(float vl, float fl) {
    const float vn1 = qp<QP_NEXT>(vl), vn2 = qp<QP_NEXT2>(vl);
    const float fn1 = qp<QP_NEXT>(fl), fn2 = qp<QP_NEXT2>(fl);
    return (-vn2) * fn1 + vn1 * fn2;
}

}  // namespace srbd
