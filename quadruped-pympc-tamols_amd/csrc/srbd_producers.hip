// srbd_producers.hip -- the producers of the batched device-resident step on the device: the periodic gait generator
// and prepare_state_and_reference for E environments per launch (srbd_pgg_run_device,
// srbd_pgg_contact_sequence_device, srbd_prepare_state_device; include/srbd_mpc.h).  Each kernel restates one host
// producer of srbd_host.cpp per environment -- float64, the same operations in the same order, unfused -- so the
// generator state keeps the bytes the host functions would leave and the outputs are the host's values cast to
// float32.  Reference paths as in srbd_host.cpp:
//   PGG  = quadruped_pympc/helpers/periodic_gait_generator.py
//   NMPC = quadruped_pympc/controllers/sampling/centroidal_nmpc_jax.py
//   pgg_run_kernel               srbd_pgg_run               PGG:48-76
//   pgg_contact_sequence_kernel  srbd_pgg_contact_sequence  PGG:93-118
//   prepare_state_kernel         srbd_prepare_state         NMPC:563-627 (no solution shift)
// Legs are independent in all three, so one lane owns one (environment, leg): lane t of the grid is leg t & 3 of
// environment t >> 2, 64 environments per 256-thread block, the lanes past 4 E idle.  No LDS, no cross-lane traffic.
// frg_step_kernel (srbd_frg_step_device) is the foothold reference generator of the same loop, one lane per
// (environment, leg) too: srbd_frg_update_lift_off, _update_touch_down and _compute of srbd_host.cpp in that order,
// through the per-leg functions both sides share (srbd_frg.h; FRG = quadruped_pympc/helpers/
// foothold_reference_generator.py:53-199).  Its one piece of cross-lane traffic is a quad broadcast of the velocity
// ring's length and head (see the kernel).
// stc_step_kernel (srbd_stc_step_device) is the loop's last stage, the stance and swing leg torques, one lane per
// (environment, leg) as well: srbd_stc_step of srbd_host.cpp through the per-leg functions of srbd_stc.h (STC =
// quadruped_pympc/helpers/swing_trajectory_controller.py, quadruped_pympc/interfaces/wb_interface.py:369-465).  No
// cross-lane traffic.
// vm_modulate_kernel (srbd_vm_modulate_device) and terrain_ref_step_kernel (srbd_terrain_ref_step_device) build what
// the reference derives from the velocity command before and after the foothold generator: the modulated command, the
// terrain estimate and entries 0..11 of the reference row (srbd_terrain.h; quadruped_pympc/helpers/
// velocity_modulator.py, terrain_estimator.py, wb_interface.py:168-172, :250-291).  Both spread an environment over
// its quad and exchange values by shuffles (see the kernels).
// touch_down_kernel (srbd_stc_touch_down_device) and gait_apply_freq_kernel (srbd_gait_apply_freq_device) close the gait
// adaptation loop around the step: the trigger that decides whether to optimise the step frequency and the write-back
// of the sampler's best frequency (srbd_gait_adapt.h; STC:148-165, wb_interface.py:354-358).  One lane per
// environment, no cross-lane traffic.
// srbd_tamols_batch_device, the loop's foothold search, is validated and enqueued here too; its kernel lives with the
// single-environment one (tamols_kernel.hip tamols_batch_kernel), whose device functions it runs.  So is
// srbd_vfa_step_device, the same search behind the reference's apex gate (srbd_vfa.h; wb_interface.py:230-246): the
// same job with the gate's four fields, the same grid, the kernel's gated instantiation.  And their forms with one
// terrain scene per environment (srbd_tamols_batch_scenes_device, srbd_vfa_step_scenes_device): the same job again,
// behind it the table of a srbd_terrain_set (terrain_kernel.hip) and the caller's scene indices.
// loop_reset_kernel (srbd_loop_reset_device) restarts the environments a mask names (srbd_reset.h; simulation/
// simulation.py:773-781, wb_interface.py:469-484): one wave per environment, see the kernel.
// iface_prologue_kernel and iface_epilogue_kernel are the two launches srbd_batch_interface_step_device
// (srbd_api_batch.hip) puts around its sampling iterations (SCI =
// quadruped_pympc/interfaces/srbd_controller_interface.py:113-180,
// :225-229): prepare_state through the device function prepare_state_kernel runs and the key schedule of
// srbd_iface.h ahead of them; the GRFs times the current contact, the footholds and previous_contact_mpc behind them.
// One lane per (environment, leg), no cross-lane traffic.
// start_stop_kernel (srbd_pgg_start_stop_device) is the gait generator's start-and-stop decision (srbd_start_stop.h;
// PGG:128-196), one quad per environment with its verdict combined by shuffles.  wb_update_kernel
// (srbd_wb_update_device) runs the whole of WBInterface.update_state_and_reference (wb_interface.py:168-298, the
// foothold search excepted) in one launch: the stages of vm_modulate_kernel, start_stop_kernel, pgg_run_kernel,
// pgg_contact_sequence_kernel, frg_step_kernel, terrain_ref_step_kernel and touch_down_kernel through the device
// functions those kernels run, what one stage hands the next kept in registers (see the kernel).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <initializer_list>

#include "../../include/srbd_host.h"
#include "../../include/srbd_mpc.h"
#include "srbd_enqueue.h"
#include "srbd_frg.h"
#include "srbd_gait_adapt.h"
#include "srbd_iface.h"
#include "srbd_launch.h"
#include "srbd_reset.h"
#include "srbd_start_stop.h"
#include "srbd_stc.h"
#include "srbd_terrain.h"
#include "yaw_sincos.h"

namespace srbd {

constexpr int PROD_MAX_DTS = 32;

// Python's float `x % 1.0` (srbd_host.cpp pymod1; the float64 fmod is exact on both sides).
__device__ inline double pymod1_dev(double x) {
    double r = fmod(x, 1.0);
    if (r != 0.0) {
        if (r < 0.0) r += 1.0;
    } else {
        r = copysign(0.0, 1.0);
    }
    return r;
}

// One leg's srbd_pgg_run: the phase and the start-up hold are advanced in place, the contact flag returned.
__device__ inline float pgg_leg_run(double& ph, int32_t& ini, double offset, double duty, double inc) {
#pragma clang fp contract(off)
    ph = pymod1_dev(ph + inc);
    if (ini) {
        if (!(ph <= offset)) {
            ini = 0;
            ph = 0.0;
        }
        return 1.0f;
    }
    return ph < duty ? 1.0f : 0.0f;
}

__global__ void __launch_bounds__(PROD_BLOCK) pgg_run_kernel(srbd_pgg* __restrict__ pgg, int E, double dt,
                                                             const double* __restrict__ step_freqs,
                                                             float* __restrict__ contact_out) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    srbd_pgg* g = pgg + e;
    const double inc = dt * (step_freqs ? step_freqs[e] : g->step_freq);
    double ph = g->phase_signal[l];
    int32_t ini = g->init[l];
    const float c = pgg_leg_run(ph, ini, g->phase_offset[l], g->duty_factor, inc);
    g->phase_signal[l] = ph;
    g->init[l] = ini;
    contact_out[t] = c;
}

// dts[j] holds for the steps i < lens[j]; validated on the host (the walk below never reaches n_dts).
struct PggSeqConst {
    double dts[PROD_MAX_DTS];
    int32_t lens[PROD_MAX_DTS];
    int32_t n_dts, H, stride;
};

// One leg's words of a srbd_pgg, held in registers by the kernels that carry them from one stage to the next.
struct PggLeg {
    double ph, offset;
    int32_t ini;
};

// One leg's srbd_pgg_contact_sequence on the leg's words `s`: row[0 .. H) written, column 0 returned.  A full-stance
// leg gets ones and srbd_pgg_reset's words; any other is left as found, its hold stored as init != 0 (the host
// restores the state through srbd_pgg_set_phase_signal, which stores it so).
__device__ __forceinline__ float pgg_leg_sequence(PggLeg& s, int32_t gait, int l, double duty, double freq,
                                                  const PggSeqConst& sc, float* __restrict__ row) {
#pragma clang fp contract(off)
    if (gait == SRBD_GAIT_FULL_STANCE) {  // ones, and srbd_pgg_reset (gait_offsets' row of this gait)
        for (int i = 0; i < sc.H; ++i) row[i] = 1.0f;
        const double off = (l == 1 || l == 2) ? 0.5 : 0.0;
        s.offset = off;
        s.ph = off;
        s.ini = 0;
        return 1.0f;
    }
    double ph = s.ph;
    int32_t ini = s.ini;
    const float first = pgg_leg_run(ph, ini, s.offset, duty, 0.0 * freq);
    row[0] = first;
    int j = 0;
    for (int i = 1; i < sc.H; ++i) {
        if (i >= sc.lens[j]) ++j;
        if (j >= sc.n_dts) break;  // refused on the host; never an index past the arrays
        row[i] = pgg_leg_run(ph, ini, s.offset, duty, sc.dts[j] * freq);
    }
    if (s.ini != (s.ini != 0)) s.ini = 1;
    return first;
}

__global__ void __launch_bounds__(PROD_BLOCK) pgg_contact_sequence_kernel(srbd_pgg* __restrict__ pgg, int E,
                                                                          const PggSeqConst sc,
                                                                          float* __restrict__ contacts) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    srbd_pgg* g = pgg + e;
    const int32_t gait = g->gait_type;
    PggLeg s = {g->phase_signal[l], g->phase_offset[l], g->init[l]};
    const int32_t ini0 = s.ini;
    pgg_leg_sequence(s, gait, l, g->duty_factor, g->step_freq, sc, contacts + (size_t)t * sc.stride);
    if (gait == SRBD_GAIT_FULL_STANCE) {
        g->phase_offset[l] = s.offset;
        g->phase_signal[l] = s.ph;
        g->init[l] = s.ini;
    } else if (s.ini != ini0) {
        g->init[l] = s.ini;
    }
}

// One leg's srbd_prepare_state: lane (e, l) copies the base entries 3 l .. 3 l + 2 and foot l of state and reference,
// and zeroes leg l's warm start when it lifts off.  cur, prev: the leg's current and previous contact flags (the
// previous one is read only for a swing leg with a warm start).
__device__ __forceinline__ void prepare_state_leg(int e, int l, const float* __restrict__ cur,
                                                  const float* __restrict__ prev,
                                                  const double* __restrict__ state_in,
                                                  const double* __restrict__ ref_in, int params_per_leg,
                                                  int num_params, float* __restrict__ best_params,
                                                  float* __restrict__ states, float* __restrict__ refs) {
    const double* __restrict__ si = state_in + 24 * (size_t)e;
    const double* __restrict__ ri = ref_in + 24 * (size_t)e;
    float* __restrict__ so = states + 24 * (size_t)e;
    float* __restrict__ ro = refs + 24 * (size_t)e;
    const bool swing = (double)*cur == 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int b = 3 * l + k, f = 12 + 3 * l + k;
        so[b] = (float)si[b];
        ro[b] = (float)ri[b];
        const double rf = ri[f];
        so[f] = (float)(swing ? rf : si[f]);
        ro[f] = (float)rf;
    }
    if (best_params && swing && (double)*prev == 1.0) {
        float* __restrict__ bp = best_params + (size_t)e * num_params + (size_t)l * params_per_leg;
        for (int j = 0; j < params_per_leg; ++j) bp[j] = 0.0f;
    }
}

__global__ void __launch_bounds__(PROD_BLOCK) prepare_state_kernel(int E, const double* __restrict__ state_in,
                                                                   const double* __restrict__ ref_in,
                                                                   const float* __restrict__ current_contact,
                                                                   const float* __restrict__ previous_contact,
                                                                   int params_per_leg, int num_params,
                                                                   float* __restrict__ best_params,
                                                                   float* __restrict__ states,
                                                                   float* __restrict__ refs) {
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    prepare_state_leg(t >> 2, t & 3, current_contact + t, previous_contact + t, state_in, ref_in, params_per_leg,
                      num_params, best_params, states, refs);
}

// srbd_batch_interface_step_device's prologue (include/srbd_mpc.h; SCI:118-128): lane (e, l) runs prepare_state_leg
// with the current contact read from column 0 of the contact sequence, and lane (e, 0) runs environment e's key
// schedule (srbd_iface.h): keys[e] advanced `iterations` times, iteration i's (seed, counter) stored at step_keys
// [i][0][e] and [i][1][e] -- the unit-stride seeds / counters rows iteration i's step reads -- and the advanced key
// written back.  One lane is one environment's key, so every access here is a vector load or store.  No lane reads a
// word another lane of the launch writes: previous_contact and contacts are only read, best_params is written per
// leg, the key words per environment.
struct IfaceJob {
    const double *state_in, *ref_in;
    const float *contacts, *previous_contact;
    float *best_params, *states, *refs;
    uint64_t *keys, *step_keys;
    int32_t contact_stride, iterations, params_per_leg, num_params, rng;
};
// due (srbd_batch_interface_step_masked_device; NULL otherwise): the four lanes of an environment that is not due
// return behind that one load -- nothing of it is prepared, its key stays where its last solve left it.
__global__ void __launch_bounds__(PROD_BLOCK) iface_prologue_kernel(int E, const IfaceJob j,
                                                                    const int32_t* __restrict__ due) {
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    if (due && due[e] == 0) return;
    prepare_state_leg(e, l, j.contacts + (size_t)t * j.contact_stride, j.previous_contact + t, j.state_in, j.ref_in,
                      j.params_per_leg, j.num_params, j.best_params, j.states, j.refs);
    if (l == 0) {
        uint64_t k0 = j.keys[2 * (size_t)e], k1 = j.keys[2 * (size_t)e + 1];
        for (int i = 0; i < j.iterations; ++i) {
            iface_next_key(j.rng, k0, k1);
            uint64_t* __restrict__ row = j.step_keys + 2 * (size_t)i * E;
            row[e] = k0;
            row[(size_t)E + e] = k1;
        }
        j.keys[2 * (size_t)e] = k0;
        j.keys[2 * (size_t)e + 1] = k1;
    }
}

// Its epilogue (SCI:170-175, :225-229, and previous_contact_mpc = current_contact): lane (e, l) masks leg l's GRFs of
// the last iteration with the leg's current contact -- the float64 product of srbd_host.cpp's mask line, one rounding
// and no fused operation -- copies the leg's reference foothold and stores the contact as the next call's previous
// one.  The contact is read from the caller's sequence again: nothing between the prologue and here writes it.
__global__ void __launch_bounds__(PROD_BLOCK) iface_epilogue_kernel(int E, const float* __restrict__ grf_raw,
                                                                    const float* __restrict__ contacts,
                                                                    int contact_stride,
                                                                    const double* __restrict__ ref_in,
                                                                    double* __restrict__ grf,
                                                                    double* __restrict__ footholds,
                                                                    float* __restrict__ previous_contact,
                                                                    const int32_t* __restrict__ due) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    if (due && due[e] == 0) return;  // not due: previous_contact keeps the contact of its last solve
    const float cur = contacts[(size_t)t * contact_stride];
    const double cd = (double)cur;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        grf[3 * (size_t)t + c] = (double)grf_raw[3 * (size_t)t + c] * cd;
        footholds[3 * (size_t)t + c] = ref_in[24 * (size_t)e + 12 + 3 * l + c];
    }
    previous_contact[t] = cur;
}

// The arrays of one srbd_frg_step_device call (srbd_frg_batch_io) and the values formed on the host.
struct FrgJob {
    const double *base_pos, *yaws, *base_vel, *ref_vel, *hips, *feet, *com_off;
    const float *prev, *cur;
    const srbd_pgg* pgg;
    double root;  // sqrt(com_height_nominal / gravity)
    double *seeds, *ref;
};

// Lane (e, l) owns row l of the five position tables of environment e and writes nothing else, lane (e, 0) the
// velocity ring besides.  All four lanes need the ring's mean: each forms it from the ring as it was and the new entry
// it holds in registers (frg_mean_with), and lane 0 alone stores that entry -- into a slot that is unused (ring not
// full) or holds the evicted oldest entry (ring full), which the new mean excludes.  The ring's length and head are
// rewritten by lane 0 as well, so lane 0 alone loads them and hands them to its three neighbours with a quad
// broadcast (4 E lanes are live and a quad is one environment, so its lane 0 is live whenever the others are).  No
// lane reads a word another lane of the launch writes.
// That step for lane l of environment g's quad, the values it reads already in hand: prev / cur the leg's contacts,
// (c, s) cos / sin of the yaw, (bx, by) / (qx, qy) the base and the reference velocity, off com_pos_offset_w or NULL.
// out[3] receives the leg's foothold.
__device__ __forceinline__ void frg_leg_step(srbd_frg* g, int l, const double* base, const double* foot,
                                             const double* hip, double prev, double cur, bool full_stance, double c,
                                             double s, double bx, double by, double qx, double qy, double root,
                                             const double* off, double* out) {
#pragma clang fp contract(off)
    int len = 0, head = 0;
    if (l == 0) {
        len = g->hist_len;
        head = g->hist_head;
    }
    len = __shfl(len, 0, 4);
    head = __shfl(head, 0, 4);
    frg_leg_lift_off(g, l, prev, cur, foot, full_stance, base, c, s);
    frg_leg_touch_down(g, l, prev, cur, foot, full_stance, base, c, s);
    const double vx = c * bx + s * by, vy = -s * bx + c * by;
    const double rx = c * qx + s * qy, ry = -s * qx + c * qy;
    double mx, my, ox, oy;
    frg_mean_with(g, len, head, vx, vy, mx, my);
    frg_compensation(g, rx, ry, mx, my, root, ox, oy);
    frg_leg_foothold(g, l, hip, base, c, s, ox, oy, off, out);
    if (l == 0) {
        int len1, head1;
        const int slot = frg_ring_next(len, head, len1, head1);
        g->vel_hist[slot][0] = vx;
        g->vel_hist[slot][1] = vy;
        g->hist_len = len1;
        g->hist_head = head1;
    }
}

__global__ void __launch_bounds__(PROD_BLOCK) frg_step_kernel(srbd_frg* __restrict__ frg, int E, const FrgJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    const double base[3] = {j.base_pos[3 * (size_t)e], j.base_pos[3 * (size_t)e + 1], j.base_pos[3 * (size_t)e + 2]};
    const bool full_stance = j.pgg && j.pgg[e].gait_type == SRBD_GAIT_FULL_STANCE;
    double c, s;
    yaw_sincos(j.yaws[e], c, s);
    double out[3];
    frg_leg_step(frg + e, l, base, j.feet + 3 * (size_t)t, j.hips + 3 * (size_t)t, (double)j.prev[t], (double)j.cur[t],
                 full_stance, c, s, j.base_vel[3 * (size_t)e], j.base_vel[3 * (size_t)e + 1], j.ref_vel[3 * (size_t)e],
                 j.ref_vel[3 * (size_t)e + 1], j.root, j.com_off ? j.com_off + 3 * (size_t)e : nullptr, out);
    double* __restrict__ seed = j.seeds + 3 * (size_t)t;
    seed[0] = out[0], seed[1] = out[1], seed[2] = out[2];
    if (j.ref) {
        double* __restrict__ r = j.ref + 24 * (size_t)e + 12 + 3 * l;
        r[0] = out[0], r[1] = out[1], r[2] = out[2];
    }
}

// The arrays of one srbd_stc_step_device call (srbd_stc_batch_io).
struct StcJob {
    const double *jac, *jac_dot, *mass_matrix, *q_dot, *foot_pos, *foot_vel, *passive, *bias, *grfs, *lift_off,
        *touch_down;
    const srbd_frg* frg;
    const float* contact;
    double dt, apex_interval;
    double *tau, *des_foot_pos, *des_foot_vel, *des_joint_vel;
    int32_t *apex, *full_stance;
};

// srbd_stc_step of srbd_host.cpp per environment, through the per-leg functions both sides share (srbd_stc.h).  Lane
// (e, l) owns clock l of environment e and row (e, l) of the outputs and writes nothing else, lane (e, 0) the two
// flag words besides.  The apex flag needs all four updated clocks: every lane loads the four old clocks and the four
// contacts first, and lane 0 recomputes its neighbours' clocks from them (stc_clock, the operation they perform), so
// there is no cross-lane exchange.  The old clocks are loaded before any lane of the quad stores its new one: a quad
// lies inside one wave, which runs the loads and then the stores in program order, and the fence keeps the compiler
// from moving a store above them.  An environment whose struct srbd_stc_step would refuse is left as found, its
// output rows unwritten, as on the host.
__global__ void __launch_bounds__(PROD_BLOCK) stc_step_kernel(srbd_stc* __restrict__ stc, int E, const StcJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    srbd_stc* g = stc + e;
    if (!stc_struct_ok(g)) return;
    double clocks[4], contact[4];
    for (int k = 0; k < 4; ++k) {
        clocks[k] = g->swing_time[k];
        contact[k] = (double)j.contact[4 * (size_t)e + k];
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const double period = g->swing_period;
    const double now = stc_clock(clocks[l], period, contact[l], j.dt);
    const size_t v = 3 * (size_t)t, m = 9 * (size_t)t;
    const StcLeg x = {j.jac + m,
                      j.jac_dot + m,
                      j.mass_matrix + m,
                      j.q_dot + v,
                      j.foot_pos + v,
                      j.foot_vel + v,
                      j.passive + v,
                      j.bias + v,
                      j.grfs + v,
                      j.frg ? j.frg[e].lift_off[l] : j.lift_off + v,
                      j.touch_down + v,
                      j.tau + v,
                      j.des_foot_pos + v,
                      j.des_foot_vel + v,
                      j.des_joint_vel ? j.des_joint_vel + v : nullptr};
    stc_leg(g, now, contact[l], x);
    g->swing_time[l] = now;
    if (l == 0) {
        clocks[0] = now;
        for (int k = 1; k < 4; ++k) clocks[k] = stc_clock(clocks[k], period, contact[k], j.dt);
        if (j.apex) j.apex[e] = stc_apex(clocks, period, contact, j.apex_interval);
        if (j.full_stance) j.full_stance[e] = stc_full_stance(contact);
    }
}

// The arrays of one srbd_vm_modulate_device call (srbd_vm_batch_io).
struct VmJob {
    const double *lin, *ang, *feet, *hips;
    double max_distance;
    double *lin_out, *ang_out;
};

// srbd_vm_modulate of srbd_host.cpp per environment (srbd_terrain.h).  Lane (e, l) forms leg l's distance and its
// comparison; the four comparisons are or-ed across the quad (all four lanes of a live quad are live), and lanes 0..2
// write entry l of the two outputs.  No state.
// The modulator's disjunction for a quad: the lane's own leg's comparison or-ed with its three neighbours'.
__device__ __forceinline__ bool vm_quad_beyond(const double* foot, const double* hip, double max_distance) {
    int beyond = vm_distance(foot, hip) > max_distance ? 1 : 0;
    beyond |= __shfl_xor(beyond, 1, 4);
    beyond |= __shfl_xor(beyond, 2, 4);
    return beyond != 0;
}

__global__ void __launch_bounds__(PROD_BLOCK) vm_modulate_kernel(int E, const VmJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    const bool beyond = vm_quad_beyond(j.feet + 3 * (size_t)t, j.hips + 3 * (size_t)t, j.max_distance);
    if (l == 3) return;
    const double* lin = j.lin + 3 * (size_t)e;
    const bool standing = vm_standing(lin);
    j.lin_out[3 * (size_t)e + l] = vm_entry(lin[l], standing, beyond);
    j.ang_out[3 * (size_t)e + l] = vm_entry(j.ang[3 * (size_t)e + l], standing, beyond);
}

// The arrays of one srbd_terrain_ref_step_device call (srbd_terrain_ref_batch_io).
struct TerrJob {
    const double *base_pos, *com_pos, *com_off, *yaws, *lin, *ang, *feet;
    const srbd_frg* frg;
    double ref_z;
    double *ref, *terrain;
};

// cos and sin of x on the lanes of a pair: the reduction on both, the sine series on the even lane and the cosine
// series on the odd one side by side, exchanged by one shuffle; yaw_sincos's functions, so its bits.
__device__ inline void pair_sincos(double x, int l, double& c, double& s) {
    DD r;
    const int q = yaw_reduce(x, r);
    const bool cosine = (l & 1) != 0;
    const double mine = yaw_series_value(r, cosine);
    const double other = __shfl_xor(mine, 1, 4);
    yaw_finish(x, q, cosine ? other : mine, cosine ? mine : other, c, s);
}

// srbd_terrain_estimate and srbd_reference_assemble of srbd_host.cpp per environment, through the pieces both sides
// share (srbd_terrain.h), an environment spread over its quad: lane l rotates foot l, forms difference l with its
// arctangent (l = 0, 1 the pitch pair, 2, 3 the roll pair), and evaluates one of the four series of cos / sin of roll
// and pitch; the values move inside the quad by shuffles (4 E lanes are live and a quad is one environment, so every
// source lane is live).  Lane 0 alone loads the state, runs the filter and stores the three filtered words, and hands
// them to its neighbours with a quad broadcast: no lane reads a word another lane of the launch writes.  Lane l
// stores entries 3 l .. 3 l + 2 of the reference row.
// That step for lane l of an environment's quad: tg its estimator struct, foot the leg's three coordinates, (c, s)
// cos / sin of the yaw, lin / ang the (modulated) command, terrain_row the environment's roll / pitch / height output
// or NULL, row entries 3 l .. 3 l + 2 of its reference row.
__device__ __forceinline__ void terr_quad(srbd_terrain_est* tg, int l, const double* base, const double* foot,
                                          double c, double s, double ref_z, double com_z, double com_off_z,
                                          const double* lin, const double* ang, double* __restrict__ terrain_row,
                                          double* __restrict__ row) {
#pragma clang fp contract(off)
    double rot[3];
    terr_rotate(foot, base, c, s, rot);
    int a, b;
    terr_pair(l, a, b);
    double ra[3], rb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ra[k] = __shfl(rot[k], a, 4);
        rb[k] = __shfl(rot[k], b, 4);
    }
    double dz_l;
    const double angle_l = terr_slope(l, ra, rb, dz_l);
    double angle[4], dz[4], foot_z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        angle[k] = __shfl(angle_l, k, 4);
        dz[k] = __shfl(dz_l, k, 4);
        foot_z[k] = __shfl(foot[2], k, 4);
    }
    srbd_terrain_est g = {};
    if (l == 0) {
        g = *tg;
        terr_filter(&g, angle, dz, foot_z);
        tg->roll = g.roll;
        tg->pitch = g.pitch;
        tg->height = g.height;
        if (terrain_row) terrain_row[0] = g.roll, terrain_row[1] = g.pitch, terrain_row[2] = g.height;
    }
    const double roll = __shfl(g.roll, 0, 4), pitch = __shfl(g.pitch, 0, 4), height = __shfl(g.height, 0, 4);
    double cc, ss;  // lanes 0, 1: of the roll; lanes 2, 3: of the pitch
    pair_sincos(l < 2 ? roll : pitch, l, cc, ss);
    const double cr = __shfl(cc, 0, 4), sr = __shfl(ss, 0, 4), cp = __shfl(cc, 2, 4), sp = __shfl(ss, 2, 4);
    double out[12];
    terr_assemble(roll, pitch, height, cr, sr, cp, sp, ref_z, base[2], com_z, com_off_z, lin, ang, out);
#pragma unroll
    for (int k = 0; k < 3; ++k) row[k] = l == 0 ? out[k] : l == 1 ? out[3 + k] : l == 2 ? out[6 + k] : out[9 + k];
}

__global__ void __launch_bounds__(PROD_BLOCK) terrain_ref_step_kernel(srbd_terrain_est* __restrict__ terr, int E,
                                                                      const TerrJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    const double base[3] = {j.base_pos[3 * (size_t)e], j.base_pos[3 * (size_t)e + 1], j.base_pos[3 * (size_t)e + 2]};
    const double* fp = j.frg ? j.frg[e].lift_off[l] : j.feet + 3 * (size_t)t;
    const double foot[3] = {fp[0], fp[1], fp[2]};
    double c, s;
    pair_sincos(j.yaws[e], l, c, s);
    terr_quad(terr + e, l, base, foot, c, s, j.ref_z, j.com_pos[3 * (size_t)e + 2],
              j.com_off ? j.com_off[3 * (size_t)e + 2] : 0.0, j.lin + 3 * (size_t)e, j.ang + 3 * (size_t)e,
              j.terrain ? j.terrain + 3 * (size_t)e : nullptr, j.ref + 24 * (size_t)e + 3 * l);
}

// The arrays of one srbd_pgg_start_stop_device call (srbd_start_stop_batch_io).
struct StartStopJob {
    const double *feet, *hips, *base_pos, *euler, *lin_vel, *ang_vel, *ref_lin, *ref_ang;
    const float* contact;
    const srbd_frg* frg;
    double hip_offset;
    int32_t* action;
};

// srbd_pgg_start_stop's verdict for lane l of an environment's quad (srbd_start_stop.h): the lane forms its own leg's
// distance and comparison, the four are and-ed across the quad, the four contact flags are gathered from the four
// lanes, and every lane evaluates the conjuncts that belong to no leg (the same values on all four).  Returns the
// action for the gait type found.  All four lanes of a live quad are live.
__device__ __forceinline__ int32_t start_stop_quad(int l, const double* foot, const double* hip, const double* base,
                                                   const double* euler, const double* lin_vel, const double* ang_vel,
                                                   const double* ref_lin, const double* ref_ang, float contact_l,
                                                   double c, double s, double hip_offset, int32_t gait_type) {
#pragma clang fp contract(off)
    double contact[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) contact[k] = (double)__shfl(contact_l, k, 4);
    int close = ss_leg_close(l, foot, hip, base, c, s, hip_offset) ? 1 : 0;
    close &= __shfl_xor(close, 1, 4);
    close &= __shfl_xor(close, 2, 4);
    const bool stop = ss_quiet(ref_lin, ref_ang, lin_vel, ang_vel, euler, contact) && close != 0;
    return ss_action(stop, gait_type);
}

// The two gait type words of an environment, loaded by its lane 0 alone (which rewrites one of them) and handed to
// the quad by a broadcast.
__device__ __forceinline__ void pgg_quad_gait(const srbd_pgg* g, int l, int32_t& gait, int32_t& previous) {
    gait = 0, previous = 0;
    if (l == 0) {
        gait = g->gait_type;
        previous = g->previous_gait_type;
    }
    gait = __shfl(gait, 0, 4);
    previous = __shfl(previous, 0, 4);
}

// srbd_pgg_start_stop of srbd_host.cpp per environment.  Lane (e, l) owns leg l's three words of pgg[e] and writes
// nothing else, lane (e, 0) the gait type and action[e] besides.  No lane reads a word another lane of the launch
// writes.
__global__ void __launch_bounds__(PROD_BLOCK) start_stop_kernel(srbd_pgg* __restrict__ pgg, int E,
                                                                const StartStopJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    const size_t e3 = 3 * (size_t)e;
    srbd_pgg* g = pgg + e;
    int32_t gait, previous;
    pgg_quad_gait(g, l, gait, previous);
    double c, s;
    pair_sincos(j.euler[e3 + 2], l, c, s);
    const int32_t action = start_stop_quad(l, j.feet + 3 * (size_t)t, j.hips + 3 * (size_t)t, j.base_pos + e3,
                                           j.euler + e3, j.lin_vel + e3, j.ang_vel + e3, j.ref_lin + e3, j.ref_ang + e3,
                                           j.contact[t], c, s, j.frg ? j.frg[e].hip_offset : j.hip_offset, gait);
    if (l == 0 && j.action) j.action[e] = action;
    if (action == SS_UNTOUCHED) return;
    gait = ss_next_gait(action, gait, previous);
    ss_apply_leg(l, action, gait, g->phase_offset[l], g->phase_signal[l], g->init[l]);
    if (l == 0) g->gait_type = gait;
}

// The arrays and shared values of one srbd_wb_update_device call (srbd_wb_update_io) with the state arrays.
struct WbJob {
    const double *com_pos, *base_pos, *base_vel, *euler, *ang_vel, *feet, *hips, *ref_lin, *ref_ang, *com_off;
    double dt, max_distance, root, ref_z;  // root = sqrt(com_height_nominal / gravity)
    double *lin_out, *ang_out;
    float *contacts, *cur_out, *prev_out;
    double *seeds, *ref, *terrain;
    int32_t *optimize, *action;
    srbd_pgg* pgg;
    srbd_frg* frg;
    srbd_terrain_est* terr;
    float* contact;
    int32_t* rising_edge;
    int32_t lookahead, stages;
    PggSeqConst sc;
};

// WBInterface.update_state_and_reference (WBI:168-298, the visual foothold adaptation excepted) per environment: the
// stages of vm_modulate_kernel, start_stop_kernel, pgg_run_kernel, pgg_contact_sequence_kernel, frg_step_kernel,
// terrain_ref_step_kernel and touch_down_kernel in that order, through the device functions those kernels run, so
// every stage has one body and leaves the bits its own launch leaves.  Lane (e, l) is leg l of environment e, as in
// all of them.  What a stage hands to a later one stays in registers:
//   the modulated command       lin_m / ang_m, formed by every lane of the quad (the same values on all four)
//   the gait type               `gait`: loaded by lane 0, broadcast, replaced by start-and-stop's verdict in every
//                               lane's register; the sequence and the foothold generator read that register, and lane
//                               0 stores it at the end -- no lane reads gait_type from memory after it is written
//   the leg's phase, offset     `leg`: loaded once, rewritten by start-and-stop, run and the sequence in registers,
//   and hold                    stored once behind the sequence
//   the previous contact and    prev_f (the contact state as found) and cur_f (the sequence's column 0 as the lane
//   column 0 of the sequence    itself formed it); start-and-stop gathers the quad's four prev_f by shuffles
//   the lift-off row            lane l rereads lift_off[l] of frg[e], which no lane but itself writes (frg_leg_lift_off
//                               just before, in program order): its own store, so no fence is needed; the terrain stage
//                               then exchanges the rotated feet by shuffles
// The touch-down trigger reads the lane's own row of the sequence back (the stores a few statements above it, the same
// thread) and combines the four legs' conjunctions by shuffles; lane 0 owns rising_edge[e] and optimize[e].  The stage
// word is a kernel argument, so every branch on it is uniform.  No LDS, no atomics; environments share nothing.
__global__ void __launch_bounds__(PROD_BLOCK) wb_update_kernel(int E, const WbJob j) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (t >= 4 * E) return;
    const int e = t >> 2, l = t & 3;
    const size_t e3 = 3 * (size_t)e, t3 = 3 * (size_t)t;
    const double base[3] = {j.base_pos[e3], j.base_pos[e3 + 1], j.base_pos[e3 + 2]};
    const double* foot = j.feet + t3;
    const double* hip = j.hips + t3;
    double c, s;
    pair_sincos(j.euler[e3 + 2], l, c, s);

    // 1. the velocity modulator (WBI:168-172); switched off, `beyond` is false and vm_entry returns the command
    const double* lin = j.ref_lin + e3;
    const double* ang = j.ref_ang + e3;
    const bool beyond = (j.stages & SRBD_WB_VM) ? vm_quad_beyond(foot, hip, j.max_distance) : false;
    const bool standing = vm_standing(lin);
    double lin_m[3], ang_m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lin_m[k] = vm_entry(lin[k], standing, beyond);
        ang_m[k] = vm_entry(ang[k], standing, beyond);
    }
    if (l < 3) {
        if (j.lin_out) j.lin_out[e3 + l] = l == 0 ? lin_m[0] : l == 1 ? lin_m[1] : lin_m[2];
        if (j.ang_out) j.ang_out[e3 + l] = l == 0 ? ang_m[0] : l == 1 ? ang_m[1] : ang_m[2];
    }

    srbd_pgg* g = j.pgg + e;
    srbd_frg* fg = j.frg + e;
    PggLeg leg = {g->phase_signal[l], g->phase_offset[l], g->init[l]};
    const double duty = g->duty_factor, freq = g->step_freq;
    int32_t gait, previous_gait;
    pgg_quad_gait(g, l, gait, previous_gait);
    const float prev_f = j.contact[t];

    // 2. start-and-stop (WBI:175-189) on the modulated command and the contact state as found
    int32_t action = SS_UNTOUCHED;
    if (j.stages & SRBD_WB_START_STOP) {
        action = start_stop_quad(l, foot, hip, base, j.euler + e3, j.base_vel + e3, j.ang_vel + e3, lin_m, ang_m,
                                 prev_f, c, s, fg->hip_offset, gait);
        gait = ss_next_gait(action, gait, previous_gait);
        ss_apply_leg(l, action, gait, leg.offset, leg.ph, leg.ini);
    }
    if (l == 0 && j.action) j.action[e] = action;

    // 3., 4. run(dt) with its flags discarded and the contact sequence (WBI:191-194)
    (void)pgg_leg_run(leg.ph, leg.ini, leg.offset, duty, j.dt * freq);
    float* row = j.contacts + (size_t)t * j.sc.stride;
    const float cur_f = pgg_leg_sequence(leg, gait, l, duty, freq, j.sc, row);
    g->phase_signal[l] = leg.ph;
    g->phase_offset[l] = leg.offset;
    g->init[l] = leg.ini;
    if (l == 0 && action != SS_UNTOUCHED) g->gait_type = gait;

    // 5. previous_contact = current_contact, current_contact = column 0 (WBI:196-199)
    if (j.prev_out) j.prev_out[t] = prev_f;
    j.contact[t] = cur_f;
    if (j.cur_out) j.cur_out[t] = cur_f;

    // 6. the foothold reference generator (WBI:202-227)
    double out[3];
    frg_leg_step(fg, l, base, foot, hip, (double)prev_f, (double)cur_f, gait == SRBD_GAIT_FULL_STANCE, c, s,
                 j.base_vel[e3], j.base_vel[e3 + 1], lin_m[0], lin_m[1], j.root, j.com_off ? j.com_off + e3 : nullptr,
                 out);
    double* __restrict__ seed = j.seeds + t3;
    seed[0] = out[0], seed[1] = out[1], seed[2] = out[2];
    double* __restrict__ rf = j.ref + 24 * (size_t)e + 12 + 3 * l;
    rf[0] = out[0], rf[1] = out[1], rf[2] = out[2];

    // 7. the terrain estimate on the lift-off table and the reference row (WBI:250-291)
    const double lift[3] = {fg->lift_off[l][0], fg->lift_off[l][1], fg->lift_off[l][2]};
    terr_quad(j.terr + e, l, base, lift, c, s, j.ref_z, j.com_pos[e3 + 2], j.com_off ? j.com_off[e3 + 2] : 0.0, lin_m,
              ang_m, j.terrain ? j.terrain + e3 : nullptr, j.ref + 24 * (size_t)e + 3 * l);

    // 8. the touch-down trigger (WBI:295-300)
    if (j.stages & SRBD_WB_TOUCH_DOWN) {
        bool stable = true, next_all = true;
        ga_leg_window(row, j.lookahead, stable, next_all);
        int bits = (cur_f == 1.0f ? 1 : 0) | (prev_f == 1.0f ? 2 : 0) | (stable ? 4 : 0) | (next_all ? 8 : 0);
        bits &= __shfl_xor(bits, 1, 4);
        bits &= __shfl_xor(bits, 2, 4);
        if (l == 0) {
            int32_t edge = j.rising_edge[e];
            j.optimize[e] = ga_trigger(&edge, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0);
            j.rising_edge[e] = edge;
        }
    } else if (l == 0) {
        j.optimize[e] = 0;
    }
}

// srbd_stc_touch_down of srbd_host.cpp per environment (srbd_gait_adapt.h ga_touch_down): lane e owns rising_edge[e]
// and optimize[e] and reads its own 4 + 4 + 4 x (lookahead + 1) contact flags.
__global__ void __launch_bounds__(PROD_BLOCK) touch_down_kernel(int32_t* __restrict__ rising_edge, int E,
                                                                const float* __restrict__ current,
                                                                const float* __restrict__ previous,
                                                                const float* __restrict__ contacts, int stride,
                                                                int lookahead, int32_t* __restrict__ optimize) {
    const int e = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (e >= E) return;
    int32_t edge = rising_edge[e];
    optimize[e] = ga_touch_down(&edge, current + 4 * (size_t)e, previous + 4 * (size_t)e,
                                contacts + (size_t)e * 4 * stride, stride, lookahead);
    rising_edge[e] = edge;
}

// srbd_gait_apply_freq of srbd_host.cpp per environment (ga_apply_freq): lane e owns the three words it rewrites in
// pgg[e], frg[e] and stc[e].
__global__ void __launch_bounds__(PROD_BLOCK) gait_apply_freq_kernel(srbd_pgg* __restrict__ pgg,
                                                                     srbd_frg* __restrict__ frg,
                                                                     srbd_stc* __restrict__ stc, int E,
                                                                     const int32_t* __restrict__ optimize,
                                                                     const float* __restrict__ best_freq) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * PROD_BLOCK + threadIdx.x;
    if (e >= E) return;
    ga_apply_freq(pgg + e, frg ? frg + e : nullptr, stc ? stc + e : nullptr, optimize[e], best_freq[e]);
}

// srbd_loop_reset of srbd_host.cpp per environment (srbd_reset.h loop_reset_env, the statements both sides run).  One
// wave owns one environment: the wave index and with it e are wave-uniform, the mask word is loaded once and made
// uniform too, and a wave whose word is 0 leaves after that one load -- it reads nothing else of its environment and
// writes nothing.  A reset wave spreads each struct's 8-byte words over its lanes (lane l takes the words l, l + 64,
// ..: consecutive lanes, consecutive addresses) and lanes 0..15 the up to four contact rows.  Every pointer of the job
// is a kernel argument, so the branches on them are uniform as well.  Waves share nothing: no LDS, no atomics.
__global__ void __launch_bounds__(64 * LOOP_RESET_WAVES) loop_reset_kernel(int E, const LoopResetJob j) {
    const int e = blockIdx.x * LOOP_RESET_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (e >= E) return;
    const int32_t level = loop_reset_level(__builtin_amdgcn_readfirstlane(j.mask[e]));
    if (level == 0) return;
    const int lane = threadIdx.x & 63;
    const size_t n = (size_t)e;
    const LoopResetEnv x = {j.feet ? j.feet + 12 * n : nullptr,
                            j.pgg ? j.pgg + n : nullptr,
                            j.frg ? j.frg + n : nullptr,
                            j.stc ? j.stc + n : nullptr,
                            j.terr ? j.terr + n : nullptr,
                            j.vfa ? j.vfa + n : nullptr,
                            j.pgg0 ? j.pgg0 + n : nullptr,
                            j.frg0 ? j.frg0 + n : nullptr,
                            j.stc0 ? j.stc0 + n : nullptr,
                            j.terr0 ? j.terr0 + n : nullptr,
                            j.vfa0 ? j.vfa0 + n : nullptr,
                            j.rising_edge ? j.rising_edge + n : nullptr,
                            j.best ? j.best + n * (size_t)j.num_params : nullptr,
                            j.num_params};
    loop_reset_env(x, level, lane, 64);
    const int r = lane >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i == r && i < j.n_rows) loop_reset_contact(j.rows[i] + 4 * n, lane & 3, 4);
}

}  // namespace srbd

using namespace srbd;

namespace {

// The sequence call's own checks (srbd_pgg_contact_sequence_device), and its constants.
bool pgg_seq_const(int32_t horizon, int32_t min_horizon, const double* dts, const int32_t* lens, int32_t n_dts,
                          int32_t contact_stride, PggSeqConst& sc) {
    if (!dts || !lens) return false;
    if (horizon < min_horizon || horizon > SRBD_MAX_HORIZON || contact_stride < horizon) return false;
    if (n_dts < 1 || n_dts > PROD_MAX_DTS) return false;
    for (int i = 1, j = 0; i < horizon; ++i) {  // srbd_pgg_contact_sequence's walk: the reference's IndexError
        if (i >= lens[j]) ++j;
        if (j >= n_dts) return false;
    }
    sc = {};
    for (int j = 0; j < n_dts; ++j) {
        sc.dts[j] = dts[j];
        sc.lens[j] = lens[j];
    }
    sc.n_dts = n_dts;
    sc.H = horizon;
    sc.stride = contact_stride;
    return true;
}

}  // namespace

extern "C" int srbd_pgg_run_device(srbd_pgg* d_pgg, int32_t num_envs, double dt, const double* d_step_freqs,
                                   float* d_contact_out, void* hip_stream) {
    if (!d_pgg || !d_contact_out || !envs_ok(num_envs)) return SRBD_E_INVALID;
    hipLaunchKernelGGL(pgg_run_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_pgg,
                       num_envs, dt, d_step_freqs, d_contact_out);
    return launch_status();
}

extern "C" int srbd_pgg_contact_sequence_device(srbd_pgg* d_pgg, int32_t num_envs, int32_t horizon, const double* dts,
                                                const int32_t* lens, int32_t n_dts, float* d_contacts,
                                                int32_t contact_stride, void* hip_stream) {
    if (!d_pgg || !d_contacts || !envs_ok(num_envs)) return SRBD_E_INVALID;
    PggSeqConst sc;
    if (!pgg_seq_const(horizon, 1, dts, lens, n_dts, contact_stride, sc)) return SRBD_E_INVALID;
    hipLaunchKernelGGL(pgg_contact_sequence_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0,
                       stream_of(hip_stream), d_pgg, num_envs, sc, d_contacts);
    return launch_status();
}

extern "C" int srbd_prepare_state_device(int32_t num_envs, const double* d_state_in, const double* d_ref_in,
                                         const float* d_current_contact, const float* d_previous_contact,
                                         int32_t params_per_leg, int32_t num_params, float* d_best_params,
                                         float* d_states, float* d_refs, void* hip_stream) {
    if (!d_state_in || !d_ref_in || !d_current_contact || !d_previous_contact || !d_states || !d_refs ||
        !envs_ok(num_envs))
        return SRBD_E_INVALID;
    if (d_best_params && (params_per_leg < 1 || (int64_t)4 * params_per_leg > num_params)) return SRBD_E_INVALID;
    hipLaunchKernelGGL(prepare_state_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream),
                       num_envs, d_state_in, d_ref_in, d_current_contact, d_previous_contact, params_per_leg,
                       num_params, d_best_params, d_states, d_refs);
    return launch_status();
}

// srbd_batch_interface_step_device (srbd_api_batch.hip, which owns the batch) enqueues its two launches through these.
void srbd::launch_iface_prologue(const srbd_batch_interface_io& io, int rng, int num_params, uint64_t* step_keys, int E,
                                 hipStream_t s, const int32_t* due) {
    IfaceJob j = {};
    j.state_in = io.state_in, j.ref_in = io.ref_in;
    j.contacts = io.contacts, j.previous_contact = io.previous_contact;
    j.best_params = io.best_params, j.states = io.states, j.refs = io.refs;
    j.keys = io.keys, j.step_keys = step_keys;
    j.contact_stride = io.contact_stride, j.iterations = io.iterations;
    j.params_per_leg = io.params_per_leg, j.num_params = num_params, j.rng = rng;
    hipLaunchKernelGGL(iface_prologue_kernel, dim3(blocks_of(E)), dim3(PROD_BLOCK), 0, s, E, j, due);
}
void srbd::launch_iface_epilogue(const srbd_batch_interface_io& io, int E, hipStream_t s, const int32_t* due) {
    hipLaunchKernelGGL(iface_epilogue_kernel, dim3(blocks_of(E)), dim3(PROD_BLOCK), 0, s, E, io.grf_raw, io.contacts,
                       io.contact_stride, io.ref_in, io.grf, io.footholds, io.previous_contact, due);
}

extern "C" int srbd_frg_step_device(srbd_frg* d_frg, int32_t num_envs, const srbd_frg_batch_io* io, void* hip_stream) {
    if (!d_frg || !io || !envs_ok(num_envs)) return SRBD_E_INVALID;
    if (!io->base_pos || !io->yaws || !io->base_lin_vel || !io->ref_lin_vel || !io->hips || !io->feet ||
        !io->previous_contact || !io->current_contact || !io->seeds)
        return SRBD_E_INVALID;
    if (!std::isfinite(io->com_height_nominal) || !std::isfinite(io->gravity) || !(io->gravity > 0.0))
        return SRBD_E_INVALID;
    FrgJob j = {};
    j.base_pos = io->base_pos;
    j.yaws = io->yaws;
    j.base_vel = io->base_lin_vel;
    j.ref_vel = io->ref_lin_vel;
    j.hips = io->hips;
    j.feet = io->feet;
    j.com_off = io->com_pos_offset_w;
    j.prev = io->previous_contact;
    j.cur = io->current_contact;
    j.pgg = io->pgg;
    j.root = sqrt(io->com_height_nominal / io->gravity);  // once, here: srbd_frg_compute's value
    j.seeds = io->seeds;
    j.ref = io->ref;
    hipLaunchKernelGGL(frg_step_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_frg,
                       num_envs, j);
    return launch_status();
}

extern "C" int srbd_stc_step_device(srbd_stc* d_stc, int32_t num_envs, double dt, const srbd_stc_batch_io* io,
                                    void* hip_stream) {
    if (!d_stc || !io || !envs_ok(num_envs) || !std::isfinite(dt) || !std::isfinite(io->apex_interval))
        return SRBD_E_INVALID;
    if (!io->jac || !io->jac_dot || !io->mass_matrix || !io->q_dot || !io->foot_pos || !io->foot_vel ||
        !io->qfrc_passive || !io->qfrc_bias || !io->grfs || !io->touch_down || !io->contact || !io->tau ||
        !io->des_foot_pos || !io->des_foot_vel)
        return SRBD_E_INVALID;
    if ((io->lift_off != nullptr) == (io->frg != nullptr)) return SRBD_E_INVALID;  // exactly one of the two
    StcJob j = {};
    j.jac = io->jac;
    j.jac_dot = io->jac_dot;
    j.mass_matrix = io->mass_matrix;
    j.q_dot = io->q_dot;
    j.foot_pos = io->foot_pos;
    j.foot_vel = io->foot_vel;
    j.passive = io->qfrc_passive;
    j.bias = io->qfrc_bias;
    j.grfs = io->grfs;
    j.lift_off = io->lift_off;
    j.touch_down = io->touch_down;
    j.frg = io->frg;
    j.contact = io->contact;
    j.dt = dt;
    j.apex_interval = io->apex_interval;
    j.tau = io->tau;
    j.des_foot_pos = io->des_foot_pos;
    j.des_foot_vel = io->des_foot_vel;
    j.des_joint_vel = io->des_joint_vel;
    j.apex = io->apex;
    j.full_stance = io->full_stance;
    hipLaunchKernelGGL(stc_step_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_stc,
                       num_envs, j);
    return launch_status();
}

extern "C" int srbd_stc_touch_down_device(int32_t* d_rising_edge, int32_t num_envs, const float* d_current,
                                          const float* d_previous, const float* d_contacts, int32_t contact_stride,
                                          int32_t horizon, int32_t lookahead, int32_t* d_optimize, void* hip_stream) {
    if (!d_rising_edge || !d_current || !d_previous || !d_contacts || !d_optimize || !envs_ok(num_envs))
        return SRBD_E_INVALID;
    if (horizon < 2 || horizon > SRBD_MAX_HORIZON || contact_stride < horizon) return SRBD_E_INVALID;
    if (lookahead < 1 || lookahead > horizon - 1) return SRBD_E_INVALID;  // the reference's IndexError
    hipLaunchKernelGGL(touch_down_kernel, dim3((unsigned)((num_envs + PROD_BLOCK - 1) / PROD_BLOCK)), dim3(PROD_BLOCK),
                       0, stream_of(hip_stream), d_rising_edge, num_envs, d_current, d_previous, d_contacts,
                       contact_stride, lookahead, d_optimize);
    return launch_status();
}

extern "C" int srbd_gait_apply_freq_device(srbd_pgg* d_pgg, srbd_frg* d_frg, srbd_stc* d_stc, int32_t num_envs,
                                           const int32_t* d_optimize, const float* d_best_freq, void* hip_stream) {
    if (!d_pgg || !d_optimize || !d_best_freq || !envs_ok(num_envs)) return SRBD_E_INVALID;
    hipLaunchKernelGGL(gait_apply_freq_kernel, dim3((unsigned)((num_envs + PROD_BLOCK - 1) / PROD_BLOCK)),
                       dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_pgg, d_frg, d_stc, num_envs, d_optimize,
                       d_best_freq);
    return launch_status();
}

extern "C" int srbd_vm_modulate_device(int32_t num_envs, const srbd_vm_batch_io* io, void* hip_stream) {
    if (!io || !envs_ok(num_envs)) return SRBD_E_INVALID;
    if (!io->lin || !io->ang || !io->feet || !io->hips || !io->lin_out || !io->ang_out) return SRBD_E_INVALID;
    if (io->max_distance != io->max_distance) return SRBD_E_INVALID;
    VmJob j = {};
    j.lin = io->lin;
    j.ang = io->ang;
    j.feet = io->feet;
    j.hips = io->hips;
    j.max_distance = io->max_distance;
    j.lin_out = io->lin_out;
    j.ang_out = io->ang_out;
    hipLaunchKernelGGL(vm_modulate_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream),
                       num_envs, j);
    return launch_status();
}

extern "C" int srbd_terrain_ref_step_device(srbd_terrain_est* d_terrain, int32_t num_envs,
                                            const srbd_terrain_ref_batch_io* io, void* hip_stream) {
    if (!d_terrain || !io || !envs_ok(num_envs) || !std::isfinite(io->ref_z)) return SRBD_E_INVALID;
    if (!io->base_pos || !io->com_pos || !io->yaws || !io->lin || !io->ang || !io->ref) return SRBD_E_INVALID;
    if ((io->feet != nullptr) == (io->frg != nullptr)) return SRBD_E_INVALID;  // exactly one of the two
    TerrJob j = {};
    j.base_pos = io->base_pos;
    j.com_pos = io->com_pos;
    j.com_off = io->com_pos_offset_w;
    j.yaws = io->yaws;
    j.lin = io->lin;
    j.ang = io->ang;
    j.feet = io->feet;
    j.frg = io->frg;
    j.ref_z = io->ref_z;
    j.ref = io->ref;
    j.terrain = io->terrain;
    hipLaunchKernelGGL(terrain_ref_step_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream),
                       d_terrain, num_envs, j);
    return launch_status();
}

extern "C" int srbd_pgg_start_stop_device(srbd_pgg* d_pgg, int32_t num_envs, const srbd_start_stop_batch_io* io,
                                          void* hip_stream) {
    if (!d_pgg || !io || !envs_ok(num_envs)) return SRBD_E_INVALID;
    if (!io->feet || !io->hips || !io->base_pos || !io->euler || !io->base_lin_vel || !io->base_ang_vel ||
        !io->ref_lin || !io->ref_ang || !io->current_contact)
        return SRBD_E_INVALID;
    if ((io->frg != nullptr) == (io->hip_offset != nullptr)) return SRBD_E_INVALID;  // exactly one of the two
    StartStopJob j = {};
    j.feet = io->feet;
    j.hips = io->hips;
    j.base_pos = io->base_pos;
    j.euler = io->euler;
    j.lin_vel = io->base_lin_vel;
    j.ang_vel = io->base_ang_vel;
    j.ref_lin = io->ref_lin;
    j.ref_ang = io->ref_ang;
    j.contact = io->current_contact;
    j.frg = io->frg;
    j.hip_offset = io->hip_offset ? *io->hip_offset : 0.0;  // a host value: it travels in the kernel arguments
    j.action = io->action;
    hipLaunchKernelGGL(start_stop_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream), d_pgg,
                       num_envs, j);
    return launch_status();
}

extern "C" int srbd_wb_update_device(srbd_pgg* d_pgg, srbd_frg* d_frg, srbd_terrain_est* d_terrain, float* d_contact,
                                     int32_t* d_rising_edge, int32_t num_envs, const srbd_wb_update_io* io,
                                     void* hip_stream) {
    if (!d_pgg || !d_frg || !d_terrain || !d_contact || !io || !envs_ok(num_envs)) return SRBD_E_INVALID;
    if (io->stages & ~(SRBD_WB_VM | SRBD_WB_START_STOP | SRBD_WB_TOUCH_DOWN)) return SRBD_E_INVALID;
    if (!io->com_pos || !io->base_pos || !io->base_lin_vel || !io->euler || !io->base_ang_vel || !io->feet ||
        !io->hips || !io->ref_lin || !io->ref_ang || !io->contacts || !io->seeds || !io->ref || !io->optimize)
        return SRBD_E_INVALID;
    WbJob j = {};
    if (!pgg_seq_const(io->horizon, 2, io->dts, io->lens, io->n_dts, io->contact_stride, j.sc)) return SRBD_E_INVALID;
    if (io->stages & SRBD_WB_TOUCH_DOWN) {
        if (!d_rising_edge) return SRBD_E_INVALID;
        if (io->lookahead < 1 || io->lookahead > io->horizon - 1) return SRBD_E_INVALID;  // the reference's IndexError
    }
    if (!std::isfinite(io->dt) || !std::isfinite(io->ref_z) || !std::isfinite(io->com_height_nominal) ||
        !std::isfinite(io->gravity) || !(io->gravity > 0.0))
        return SRBD_E_INVALID;
    if ((io->stages & SRBD_WB_VM) && io->max_distance != io->max_distance) return SRBD_E_INVALID;
    j.com_pos = io->com_pos;
    j.base_pos = io->base_pos;
    j.base_vel = io->base_lin_vel;
    j.euler = io->euler;
    j.ang_vel = io->base_ang_vel;
    j.feet = io->feet;
    j.hips = io->hips;
    j.ref_lin = io->ref_lin;
    j.ref_ang = io->ref_ang;
    j.com_off = io->com_pos_offset_w;
    j.dt = io->dt;
    j.max_distance = io->max_distance;
    j.root = sqrt(io->com_height_nominal / io->gravity);  // once, here: srbd_frg_step_device's value
    j.ref_z = io->ref_z;
    j.lin_out = io->lin_out;
    j.ang_out = io->ang_out;
    j.contacts = io->contacts;
    j.cur_out = io->current_contact;
    j.prev_out = io->previous_contact;
    j.seeds = io->seeds;
    j.ref = io->ref;
    j.terrain = io->terrain;
    j.optimize = io->optimize;
    j.action = io->action;
    j.pgg = d_pgg;
    j.frg = d_frg;
    j.terr = d_terrain;
    j.contact = d_contact;
    j.rising_edge = d_rising_edge;
    j.lookahead = io->lookahead;
    j.stages = io->stages;
    hipLaunchKernelGGL(wb_update_kernel, dim3(blocks_of(num_envs)), dim3(PROD_BLOCK), 0, stream_of(hip_stream),
                       num_envs, j);
    return launch_status();
}

namespace {

// What srbd_tamols_batch_device refuses, and the launch's job from its arguments (srbd_vfa_step_device adds the gate).
// terrain: the terrain form (its scene `dev`, or NULL for a launch that takes its scenes elsewhere) on device `*device`;
// neither pointer is followed before the arguments have passed.
int tamols_batch_job(bool terrain, const int* device, const TerrainDev* dev, const srbd_tamols_params* params,
                     int32_t num_envs, const srbd_tamols_batch_io* io, TamolsBatchJob& j) {
    if (!params || !io || !io->seeds || !io->hips || !io->footholds || !io->boxes || !io->valid || !envs_ok(num_envs))
        return SRBD_E_INVALID;
    if (io->rows < 1 || io->cols < 1 || (int64_t)io->rows * io->cols > TAMOLS_MAXCAND) return SRBD_E_INVALID;
    if (terrain) {
        if (!io->yaws || !(io->dist_x > 0.0) || !(io->dist_y > 0.0)) return SRBD_E_INVALID;
    } else if (!io->heightmaps || io->heightmaps_out) {
        return SRBD_E_INVALID;
    }
    j = {};
    j.seeds = io->seeds;
    j.hips = io->hips;
    j.vel = io->forward_vel;
    j.base = io->base_pos;
    j.feet = io->feet;
    j.contact = io->contact;
    j.footholds = io->footholds;
    j.boxes = io->boxes;
    j.valid = io->valid;
    j.seed_heights = io->seed_heights;
    j.scores = io->scores;
    j.ref = io->ref;
    j.p = *params;
    j.E = num_envs;
    j.rows = io->rows;
    j.cols = io->cols;
    if (terrain) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != *device) return SRBD_E_INVALID;
        j.use_terrain = 1;
        if (dev) j.t = *dev;
        j.yaws = io->yaws;
        j.hm_out = io->heightmaps_out;
        j.dist_x = io->dist_x;
        j.dist_y = io->dist_y;
        j.inv_dx = 1.0 / io->dist_x;  // as tamols_terrain_job (srbd_api.hip) forms them
        j.inv_dy = 1.0 / io->dist_y;
        j.ray_z = io->ray_z;
        j.lattice = std::isfinite(io->dist_x) && std::isfinite(io->dist_y);
    } else {
        j.hm = io->heightmaps;
    }
    return SRBD_OK;
}

}  // namespace

extern "C" int srbd_tamols_batch_device(srbd_terrain* terrain, const srbd_tamols_params* params, int32_t num_envs,
                                        const srbd_tamols_batch_io* io, void* hip_stream) {
    TamolsBatchJob j;
    const int rc = tamols_batch_job(terrain != nullptr, terrain ? &terrain->device : nullptr,
                                    terrain ? &terrain->dev : nullptr, params, num_envs, io, j);
    if (rc != SRBD_OK) return rc;
    launch_tamols_batch(j, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_vfa_step_device(srbd_vfa* d_vfa, const srbd_stc* d_stc, srbd_terrain* terrain,
                                    const srbd_tamols_params* params, int32_t num_envs, const srbd_tamols_batch_io* io,
                                    double apex_interval, int32_t* d_mode, void* hip_stream) {
    if (!d_vfa || !d_stc || !io || !io->contact || !std::isfinite(apex_interval)) return SRBD_E_INVALID;
    TamolsBatchJob j;
    const int rc = tamols_batch_job(terrain != nullptr, terrain ? &terrain->device : nullptr,
                                    terrain ? &terrain->dev : nullptr, params, num_envs, io, j);
    if (rc != SRBD_OK) return rc;
    j.vfa = d_vfa;
    j.stc = d_stc;
    j.mode = d_mode;
    j.apex_interval = apex_interval;
    launch_tamols_batch_gated(j, stream_of(hip_stream));
    return launch_status();
}

namespace {

// What the two scenes calls refuse, with a message, and the launch's job: the shared-scene job of the terrain form,
// the set's table and the caller's indices behind it.
int tamols_scenes_job(const char* what, srbd_terrain_set* set, const int32_t* d_scene, const srbd_tamols_params* params,
                      int32_t num_envs, const srbd_tamols_batch_io* io, TamolsBatchScenesJob& j) {
    const std::string w = std::string(what) + ": ";
    if (!set) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "null set");
    if (!d_scene) return terrain_set_fail(set, SRBD_E_INVALID, w + "null d_scene");
    if (reinterpret_cast<uintptr_t>(d_scene) % alignof(int32_t))
        return terrain_set_fail(set, SRBD_E_INVALID, w + "d_scene is not 4-byte aligned");
    if (io && io->heightmaps)
        return terrain_set_fail(set, SRBD_E_INVALID,
                                w + "io->heightmaps given: the patch form has no scenes, it is srbd_tamols_batch_device's");
    const int rc = tamols_batch_job(true, &set->device, nullptr, params, num_envs, io, j);
    if (rc != SRBD_OK)
        return terrain_set_fail(set, rc,
                                w + "an argument the terrain form of srbd_tamols_batch_device refuses (a NULL required "
                                    "pointer, num_envs, rows, cols, dist_x, dist_y), or the set is not on the current "
                                    "device");
    j.table = set->d_table;
    j.scene = d_scene;
    j.num_scenes = set->num_scenes;
    return SRBD_OK;
}

}  // namespace

extern "C" int srbd_tamols_batch_scenes_device(srbd_terrain_set* set, const int32_t* d_scene,
                                               const srbd_tamols_params* params, int32_t num_envs,
                                               const srbd_tamols_batch_io* io, void* hip_stream) {
    TamolsBatchScenesJob j;
    const int rc = tamols_scenes_job("srbd_tamols_batch_scenes_device", set, d_scene, params, num_envs, io, j);
    if (rc != SRBD_OK) return rc;
    launch_tamols_batch_scenes(j, false, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_vfa_step_scenes_device(srbd_vfa* d_vfa, const srbd_stc* d_stc, srbd_terrain_set* set,
                                           const int32_t* d_scene, const srbd_tamols_params* params, int32_t num_envs,
                                           const srbd_tamols_batch_io* io, double apex_interval, int32_t* d_mode,
                                           void* hip_stream) {
    const char* what = "srbd_vfa_step_scenes_device";
    if (!set) return terrain_set_fail(nullptr, SRBD_E_INVALID, std::string(what) + ": null set");
    if (!d_vfa || !d_stc || !io || !io->contact || !std::isfinite(apex_interval))
        return terrain_set_fail(set, SRBD_E_INVALID,
                                std::string(what) + ": a NULL d_vfa, d_stc, io or io->contact, or an apex_interval that "
                                                    "is not finite");
    TamolsBatchScenesJob j;
    const int rc = tamols_scenes_job(what, set, d_scene, params, num_envs, io, j);
    if (rc != SRBD_OK) return rc;
    j.vfa = d_vfa;
    j.stc = d_stc;
    j.mode = d_mode;
    j.apex_interval = apex_interval;
    launch_tamols_batch_scenes(j, true, stream_of(hip_stream));
    return launch_status();
}

// ------------------------------------------------------------------ device-resident height scans, 'height' footholds
namespace {

// The lattice both calls share (rows, cols, dist_x, dist_y); NULL: accepted.  finite_dist: the scans ask for finite
// spacings, the gated step for what srbd_vfa_step_device asks.
const char* lattice_refused(int32_t rows, int32_t cols, double dist_x, double dist_y, bool finite_dist) {
    if (rows < 1) return "rows must be at least 1";
    if (cols < 1) return "cols must be at least 1";
    if ((int64_t)rows * cols > PATCH_BATCH_MAX_RAYS) return "rows * cols must be at most 320";
    if (!(dist_x > 0.0) || (finite_dist && !std::isfinite(dist_x)))
        return finite_dist ? "dist_x must be positive and finite" : "dist_x must be positive";
    if (!(dist_y > 0.0) || (finite_dist && !std::isfinite(dist_y)))
        return finite_dist ? "dist_y must be positive and finite" : "dist_y must be positive";
    return nullptr;
}

const char* patch_io_refused(int32_t num_envs, const srbd_patch_batch_io* io) {
    if (!io) return "null io";
    if (!io->centers) return "null io->centers";
    if (!io->yaws) return "null io->yaws";
    if (!io->points && !io->heights) return "io->points and io->heights are both null";
    if (!envs_ok(num_envs)) return "num_envs must be 1..4096";
    if (io->patches_per_env < 1 || io->patches_per_env > PATCH_BATCH_MAX_K) return "io->patches_per_env must be 1..16";
    if (const char* why = lattice_refused(io->rows, io->cols, io->dist_x, io->dist_y, true)) return why;
    if (!std::isfinite(io->ray_z)) return "ray_z must be finite";
    return nullptr;
}

PatchBatchJob patch_job(int32_t num_envs, const srbd_patch_batch_io* io) {
    PatchBatchJob j = {};
    j.centers = io->centers;
    j.yaws = io->yaws;
    j.points = io->points;
    j.heights = io->heights;
    j.E = num_envs;
    j.K = io->patches_per_env;
    j.rows = io->rows;
    j.cols = io->cols;
    j.dist_x = io->dist_x;
    j.dist_y = io->dist_y;
    j.ray_z = io->ray_z;
    return j;
}

bool on_current_device(int device) {
    int cur = -1;
    return hipGetDevice(&cur) != hipSuccess || cur == device;  // no device: the launch reports it
}

// What the two 'height' steps refuse of the arguments they share (NULL: nothing).
const char* height_step_refused(const srbd_vfa* d_vfa, const srbd_stc* d_stc, int32_t num_envs,
                                const srbd_tamols_batch_io* io, double apex_interval) {
    if (!d_vfa) return "null d_vfa";
    if (!d_stc) return "null d_stc";
    if (!io) return "null io";
    if (!io->contact) return "null io->contact";
    if (!std::isfinite(apex_interval)) return "apex_interval must be finite";
    if (!io->seeds) return "null io->seeds";
    if (!io->footholds) return "null io->footholds";
    if (!io->boxes) return "null io->boxes";
    if (!io->valid) return "null io->valid";
    if (!envs_ok(num_envs)) return "num_envs must be 1..4096";
    if (io->heightmaps) return "io->heightmaps given: the 'height' step has no patch form";
    if (!io->yaws) return "null io->yaws";
    return lattice_refused(io->rows, io->cols, io->dist_x, io->dist_y, false);
}

VfaHeightJob height_job(srbd_vfa* d_vfa, const srbd_stc* d_stc, int32_t num_envs, const srbd_tamols_batch_io* io,
                        double apex_interval, int32_t* d_mode) {
    VfaHeightJob j = {};
    j.seeds = io->seeds;
    j.yaws = io->yaws;
    j.contact = io->contact;
    j.footholds = io->footholds;
    j.boxes = io->boxes;
    j.valid = io->valid;
    j.seed_heights = io->seed_heights;
    j.hm_out = io->heightmaps_out;
    j.ref = io->ref;
    j.E = num_envs;
    j.rows = io->rows;
    j.cols = io->cols;
    j.dist_x = io->dist_x;
    j.dist_y = io->dist_y;
    j.ray_z = io->ray_z;
    j.vfa = d_vfa;
    j.stc = d_stc;
    j.mode = d_mode;
    j.apex_interval = apex_interval;
    return j;
}

}  // namespace

// An argument refusal leaves its message where srbd_terrain_last_error(NULL) / srbd_terrain_set_last_error(NULL) read it:
// the handle is not followed before the arguments have passed.
extern "C" int srbd_terrain_patches_device(srbd_terrain* terrain, int32_t num_envs, const srbd_patch_batch_io* io,
                                           void* hip_stream) {
    const std::string w = "srbd_terrain_patches_device: ";
    if (!terrain) return terrain_fail(nullptr, SRBD_E_INVALID, w + "null terrain");
    if (const char* why = patch_io_refused(num_envs, io)) return terrain_fail(nullptr, SRBD_E_INVALID, w + why);
    if (!on_current_device(terrain->device))
        return terrain_fail(terrain, SRBD_E_INVALID, w + "the terrain is not on the current device");
    PatchBatchJob j = patch_job(num_envs, io);
    j.t = terrain->dev;
    launch_patch_batch(j, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_terrain_set_patches_device(srbd_terrain_set* set, const int32_t* d_scene, int32_t num_envs,
                                               const srbd_patch_batch_io* io, void* hip_stream) {
    const std::string w = "srbd_terrain_set_patches_device: ";
    if (!set) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "null set");
    if (!d_scene) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "null d_scene");
    if (reinterpret_cast<uintptr_t>(d_scene) % alignof(int32_t))
        return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "d_scene is not 4-byte aligned");
    if (const char* why = patch_io_refused(num_envs, io)) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + why);
    if (!on_current_device(set->device))
        return terrain_set_fail(set, SRBD_E_INVALID, w + "the set is not on the current device");
    PatchBatchJob j = patch_job(num_envs, io);
    j.table = set->d_table;
    j.scene = d_scene;
    j.num_scenes = set->num_scenes;
    launch_patch_batch(j, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_vfa_height_step_device(srbd_vfa* d_vfa, const srbd_stc* d_stc, srbd_terrain* terrain,
                                           int32_t num_envs, const srbd_tamols_batch_io* io, double apex_interval,
                                           int32_t* d_mode, void* hip_stream) {
    const std::string w = "srbd_vfa_height_step_device: ";
    if (!terrain) return terrain_fail(nullptr, SRBD_E_INVALID, w + "null terrain");
    if (const char* why = height_step_refused(d_vfa, d_stc, num_envs, io, apex_interval))
        return terrain_fail(nullptr, SRBD_E_INVALID, w + why);
    if (!on_current_device(terrain->device))
        return terrain_fail(terrain, SRBD_E_INVALID, w + "the terrain is not on the current device");
    VfaHeightJob j = height_job(d_vfa, d_stc, num_envs, io, apex_interval, d_mode);
    j.t = terrain->dev;
    launch_vfa_height(j, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_vfa_height_step_scenes_device(srbd_vfa* d_vfa, const srbd_stc* d_stc, srbd_terrain_set* set,
                                                  const int32_t* d_scene, int32_t num_envs,
                                                  const srbd_tamols_batch_io* io, double apex_interval,
                                                  int32_t* d_mode, void* hip_stream) {
    const std::string w = "srbd_vfa_height_step_scenes_device: ";
    if (!set) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "null set");
    if (!d_scene) return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "null d_scene");
    if (reinterpret_cast<uintptr_t>(d_scene) % alignof(int32_t))
        return terrain_set_fail(nullptr, SRBD_E_INVALID, w + "d_scene is not 4-byte aligned");
    if (const char* why = height_step_refused(d_vfa, d_stc, num_envs, io, apex_interval))
        return terrain_set_fail(nullptr, SRBD_E_INVALID, w + why);
    if (!on_current_device(set->device))
        return terrain_set_fail(set, SRBD_E_INVALID, w + "the set is not on the current device");
    VfaHeightJob j = height_job(d_vfa, d_stc, num_envs, io, apex_interval, d_mode);
    j.table = set->d_table;
    j.scene = d_scene;
    j.num_scenes = set->num_scenes;
    launch_vfa_height(j, stream_of(hip_stream));
    return launch_status();
}

extern "C" int srbd_loop_reset_device(int32_t num_envs, const srbd_loop_reset_io* io, void* hip_stream) {
    if (!envs_ok(num_envs)) return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: num_envs must be 1..4096");
    if (!io) return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: null io");
    if (!io->mask) return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: null mask");
    if (io->n_contact_rows < 0 || io->n_contact_rows > 4)
        return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: n_contact_rows must be 0..4");
    LoopResetJob j = {};
    for (int i = 0; i < io->n_contact_rows; ++i) {
        if (!io->contact_rows[i]) return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: null contact row");
        j.rows[i] = io->contact_rows[i];
    }
    j.n_rows = io->n_contact_rows;
    j.mask = io->mask;
    j.feet = io->initial_feet;
    j.pgg = io->pgg;
    j.frg = io->frg;
    j.stc = io->stc;
    j.terr = io->terrain_est;
    j.vfa = io->vfa;
    j.pgg0 = io->pgg_snapshot;
    j.frg0 = io->frg_snapshot;
    j.stc0 = io->stc_snapshot;
    j.terr0 = io->terrain_est_snapshot;
    j.vfa0 = io->vfa_snapshot;
    j.rising_edge = io->rising_edge;
    j.best = io->best_params;
    j.num_params = io->num_params;
    // the host call's refusals; the levels are in device memory, so a struct needs its snapshot whatever they are
    const LoopResetEnv x = {j.feet, j.pgg, j.frg, j.stc, j.terr, j.vfa, j.pgg0, j.frg0, j.stc0, j.terr0, j.vfa0,
                            j.rising_edge, j.best, j.num_params};
    if (const char* why = loop_reset_refusal(x, -1)) {
        static thread_local char text[96];
        snprintf(text, sizeof(text), "srbd_loop_reset_device: %s", why);
        return fail_global(SRBD_E_INVALID, text);
    }
    for (const void* p : {(const void*)j.feet, (const void*)j.pgg, (const void*)j.frg, (const void*)j.stc,
                          (const void*)j.terr, (const void*)j.vfa, (const void*)j.pgg0, (const void*)j.frg0,
                          (const void*)j.stc0, (const void*)j.terr0, (const void*)j.vfa0})
        if ((uintptr_t)p % 8 != 0)
            return fail_global(SRBD_E_INVALID, "srbd_loop_reset_device: a struct array is not 8-byte aligned");
    const unsigned blocks = (unsigned)((num_envs + LOOP_RESET_WAVES - 1) / LOOP_RESET_WAVES);
    hipLaunchKernelGGL(loop_reset_kernel, dim3(blocks), dim3(64 * LOOP_RESET_WAVES), 0, stream_of(hip_stream),
                       num_envs, j);
    return launch_status();
}

extern "C" int srbd_selftest_yaw_sincos(const double* yaws, int32_t n, double* out_cs) {
    if (!yaws || !out_cs || n < 0) return SRBD_E_INVALID;
    for (int32_t i = 0; i < n; ++i) yaw_sincos(yaws[i], out_cs[2 * i], out_cs[2 * i + 1]);
    return SRBD_OK;
}
