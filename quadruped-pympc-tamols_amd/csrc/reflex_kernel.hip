// reflex_kernel.hip -- the swing reflex path of the leg controller on the device: the early-stance detector, the swing
// clocks and the stance and swing torques with the 'scipy' spline generator, for E environments in one launch
// (srbd_reflex_step_device; include/srbd_mpc.h).  The kernel restates srbd_reflex_step of srbd_host.cpp per
// environment through the per-leg functions both sides compile (srbd_reflex.h, srbd_stc.h) -- float64, the same
// operations in the same order, unfused -- so both structs keep the bytes the host function would leave and every
// output row holds the host's values.
//   ESD = quadruped_pympc/helpers/early_stance_detector.py:36-128
//   SCI = quadruped_pympc/helpers/swing_generators/scipy_swing_trajectory_generator.py:25-122
//   WBI = quadruped_pympc/interfaces/wb_interface.py:362-415, :435-465
// One lane per (environment, leg), as in stc_step_kernel: lane t of the grid is leg t & 3 of environment t >> 2, 64
// environments per 256-thread block, the lanes past 4 E idle.  No LDS.  The one cross-leg dependence is the detector's
// `break`: the first leg that triggers ends the tick for the legs after it.  Whether a leg would trigger depends on
// that leg's own words and inputs alone, so every lane forms its own answer and the quad exchanges the four bits by
// width-4 shuffles; a lane stands down (keeps the words it loaded) if a lower leg triggered.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/srbd_host.h"
#include "../../include/srbd_mpc.h"
#include "srbd_enqueue.h"
#include "srbd_reflex.h"
#include "srbd_stc.h"

namespace srbd {

// The arrays of one srbd_reflex_step_device call (srbd_reflex_batch_io).
struct ReflexJob {
    const double *jac, *jac_dot, *mass_matrix, *q_dot, *foot_pos, *foot_vel, *passive, *bias, *grfs, *lift_off,
        *touch_down;
    const srbd_frg* frg;
    const float *contact, *previous_contact;
    double dt, apex_interval;
    double *tau, *des_foot_pos, *des_foot_vel, *des_joint_vel;
    int32_t *apex, *full_stance;
};

// Lane (e, l) owns leg l's words of rfx[e] (hit moment, hit point, has_hitpoint, early_stance, last_des_foot_pos row),
// clock l of stc[e] and row (e, l) of the outputs, and writes nothing else; lane (e, 0) owns the cycle counter, the
// flag word and the two output flags besides.  Every lane needs the new flag before it evaluates its curve: it
// recomputes it from the quad's bits, the contacts and the old counter (reflex_cycles, the operation lane 0 performs)
// and never reads it back.  Everything another lane of the quad stores -- the four clocks, the counter, the flag --
// is loaded before any lane stores: a quad lies inside one wave, which runs the loads and then the stores in program
// order, and the fence keeps the compiler from moving a store above them.  The two exits ahead of the shuffles are per
// environment, so a quad takes them together.  An environment srbd_reflex_step would refuse is left as found, its
// output rows unwritten.
__global__ void __launch_bounds__(PROD_BLOCK) reflex_step_kernel(srbd_stc* __restrict__ stc,
                                                                 srbd_reflex* __restrict__ rfx, int E,
                                                                 const ReflexJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    srbd_stc* g = stc + e;
    srbd_reflex* r = rfx + e;
    if (!reflex_structs_ok(g, r)) return;
    double clocks[4], contact[4], previous[4], des[3];
    for (int k = 0; k < 4; ++k) {
        clocks[k] = g->swing_time[k];
        contact[k] = (double)j.contact[4 * (size_t)e + k];
        previous[k] = (double)j.previous_contact[4 * (size_t)e + k];
    }
    ReflexLeg found;
    reflex_leg_load(r, l, found);
    for (int k = 0; k < 3; ++k) des[k] = r->last_des_foot_pos[l][k];
    int32_t cycles = r->gait_cycles, flag = r->height_enhancement;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const double period = g->swing_period;
    const size_t v = 3 * (size_t)t, m = 9 * (size_t)t;
    const double* lift_off = j.frg ? j.frg[e].lift_off[l] : j.lift_off + v;
    const double* touch_down = j.touch_down + v;

    // the detector: this leg's own pass, then the quad's four answers
    ReflexLeg mine = found;
    const int trig = reflex_leg_detect(r, mine, clocks[l], period, contact[l], j.foot_pos + v, des, lift_off,
                                       touch_down)
                         ? 1
                         : 0;
    const int b0 = __shfl(trig, 0, 4), b1 = __shfl(trig, 1, 4), b2 = __shfl(trig, 2, 4), b3 = __shfl(trig, 3, 4);
    const bool lower = (l > 0 && b0) || (l > 1 && b1) || (l > 2 && b2);
    if (lower)
        mine = found;  // the tick ended before this leg: not touched at all
    else
        reflex_leg_store(r, l, mine);
    reflex_cycles(r, (b0 | b1 | b2 | b3) != 0, contact, previous, cycles, flag);
    if (l == 0) {
        r->gait_cycles = cycles;
        r->height_enhancement = flag;
    }

    // the clock and the leg law, the spline in the generator's place
    const double now = stc_clock(clocks[l], period, contact[l], j.dt);
    const StcLeg x = {j.jac + m,
                      j.jac_dot + m,
                      j.mass_matrix + m,
                      j.q_dot + v,
                      j.foot_pos + v,
                      j.foot_vel + v,
                      j.passive + v,
                      j.bias + v,
                      j.grfs + v,
                      lift_off,
                      touch_down,
                      j.tau + v,
                      j.des_foot_pos + v,
                      j.des_foot_vel + v,
                      j.des_joint_vel ? j.des_joint_vel + v : nullptr};
    stc_leg_with(g, contact[l], x, ReflexSplineGen{g, r, mine, flag, now, lift_off, touch_down});
    g->swing_time[l] = now;
    for (int k = 0; k < 3; ++k) r->last_des_foot_pos[l][k] = x.des_foot_pos[k];
    if (l == 0) {
        clocks[0] = now;
        for (int k = 1; k < 4; ++k) clocks[k] = stc_clock(clocks[k], period, contact[k], j.dt);
        if (j.apex) j.apex[e] = stc_apex(clocks, period, contact, j.apex_interval);
        if (j.full_stance) j.full_stance[e] = stc_full_stance(contact);
    }
}

}  // namespace srbd

using namespace srbd;

extern "C" int srbd_reflex_step_device(srbd_stc* d_stc, srbd_reflex* d_reflex, int32_t num_envs, double dt,
                                       const srbd_reflex_batch_io* io, void* hip_stream) {
    if (!d_stc || !d_reflex || !io || !envs_ok(num_envs) || !std::isfinite(dt) || !std::isfinite(io->stc.apex_interval))
        return SRBD_E_INVALID;
    const srbd_stc_batch_io& s = io->stc;
    if (!s.jac || !s.jac_dot || !s.mass_matrix || !s.q_dot || !s.foot_pos || !s.foot_vel || !s.qfrc_passive ||
        !s.qfrc_bias || !s.grfs || !s.touch_down || !s.contact || !s.tau || !s.des_foot_pos || !s.des_foot_vel ||
        !io->previous_contact)
        return SRBD_E_INVALID;
    if ((s.lift_off != nullptr) == (s.frg != nullptr)) return SRBD_E_INVALID;  // exactly one of the two
    ReflexJob j = {};
    j.jac = s.jac;
    j.jac_dot = s.jac_dot;
    j.mass_matrix = s.mass_matrix;
    j.q_dot = s.q_dot;
    j.foot_pos = s.foot_pos;
    j.foot_vel = s.foot_vel;
    j.passive = s.qfrc_passive;
    j.bias = s.qfrc_bias;
    j.grfs = s.grfs;
    j.lift_off = s.lift_off;
    j.touch_down = s.touch_down;
    j.frg = s.frg;
    j.contact = s.contact;
    j.previous_contact = io->previous_contact;
    j.dt = dt;
    j.apex_interval = s.apex_interval;
    j.tau = s.tau;
    j.des_foot_pos = s.des_foot_pos;
    j.des_foot_vel = s.des_foot_vel;
    j.des_joint_vel = s.des_joint_vel;
    j.apex = s.apex;
    j.full_stance = s.full_stance;
    hipLaunchKernelGGL(reflex_step_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_stc,
                       d_reflex, num_envs, j);
    return launch_status();
}
