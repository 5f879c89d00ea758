// srbd_batch.hip -- batched environments: E independent MPC problems of one configuration stepped by one set of
// launches (srbd_batch_step, include/srbd_mpc.h).  Environment e lies on blockIdx.y of every launch and owns in[e], the
// noise matrix at e P ldn, its costs row and its nleaf leaf records; within an environment every float operation is
// the single context's, in its order (the shared device code of srbd_core.h, srbd_device.h, srbd_quad.h and
// srbd_merge.h), and the reduction tree is keyed by the environment's own rows, so environment e's outputs are
// srbd_step's bit for bit.
//   batch_copy_kernel       the E step inputs, host-mapped staging -> device
//   batch_rng_kernel        rng_items per environment, keyed by in[e]'s seed and counter
//   batch_transpose_kernel  injected noise (row-major) -> SoA per environment (transpose_tile)
//   batch_rollout_kernel    rollout_quad_kernel's horizon (MPPI / random sampling, CEM, the opt-in cost terms), with
//                           that kernel's template parameter order: one 64-sample leaf per 256-thread block, leaf
//                           records only (no in-launch fold, merge or draws: with E x nleaf blocks in flight the tail
//                           those forms shorten is amortised)
//   batch_rollout_ga_kernel rollout_ga_quad_kernel (gait-adaptive sampling), the same block and record layout
//   batch_merge_kernel      one block per environment: merge_body over its leaf records -> out[e]; the last block to
//                           finish publishes the step's sequence word
// The device-resident step (srbd_batch_step_device) replaces the input copy and the host's read of out[e]:
//   batch_pack_kernel       in[e] from the caller's device arrays, as fill_input (srbd_api.hip) builds it on the host
//   batch_unpack_kernel     out[e] (device memory on this path) and the costs row -> the caller's device arrays
// A CEM batch (srbd_batch_step_cem, srbd_batch_step_cem_device) moves sigma with them: batch_copy2_kernel,
// batch_pack_cem_kernel and batch_unpack_cem_kernel; batch_merge_kernel runs merge_body's unsplit CEM form as it is.
// The device form of srbd_batch_set_gait (srbd_batch_set_gait_device):
//   batch_set_gait_kernel   the gait fields of in[e] from the caller's device arrays, as fill_gait (srbd_api.hip)
//                           writes them on the host, and the injected frequency rows into the batch's array
// The due mask (srbd_batch_step_masked_device and its CEM and interface forms): every kernel of the device step takes
// a trailing `due`, E words of the caller's device memory or NULL.  The environment is block-uniform in all of them,
// so a block of an environment with due[e] == 0 reads that one word and returns before any other global access
// (not_due); batch_merge_kernel's block skips merge_body and still counts itself.  NULL -- every launch of the
// unmasked entry points and of the host step -- is a uniform branch on a kernel argument: the same instantiations.
#include <algorithm>

#include "srbd_device.h"
#include "srbd_gait_adapt.h"
#include "srbd_merge.h"
#include "srbd_quad.h"

namespace srbd {

// The due mask: this block's environment is skipped.  One scalar load of due[env], none when the launch has no mask.
__device__ __forceinline__ bool not_due(const int32_t* __restrict__ due, int env) { return due && due[env] == 0; }

__global__ void __launch_bounds__(256) batch_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                         int nwords, int stride_words) {
    const size_t o = (size_t)blockIdx.x * stride_words;
    for (int i = threadIdx.x; i < nwords; i += 256) dst[o + i] = src[o + i];
}
// A CEM batch's copy: a second range of each input (sigma[P]) besides the first, as copy16_kernel has
__global__ void __launch_bounds__(256) batch_copy2_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          int nwords, int stride_words, int off2_words,
                                                          int nwords2) {
    const size_t o = (size_t)blockIdx.x * stride_words;
    for (int i = threadIdx.x; i < nwords; i += 256) dst[o + i] = src[o + i];
    for (int i = threadIdx.x; i < nwords2; i += 256) dst[o + off2_words + i] = src[o + off2_words + i];
}

// fill_input (srbd_api.hip) on the device, one wave per environment: state | ref, the contact columns (the first H
// from the caller's stride, the rest of MAXH zero), fzref, cost_feet, the key halves, noise_scaled and best.  Every
// float operation is the host's, in its order and unfused (the pragma: the host compiles this sum without FMA, and the
// division is the compiler's correctly rounded one), so in[e] is the host path's bit for bit.  The gait fields and
// sigma of in[e] are not written.  vec: states, refs and best_params are 16-byte aligned.
// CEM (batch_pack_cem_kernel, srbd_batch_step_cem_device): sigma of in[e] too -- the caller's row, or the constant
// sigma_reset when it is positive (the caller's array is then not read).  svec: cem.sigma is 16-byte aligned.
struct BatchPackConst {
    float q_feet[12];  // srbd_config::q_diag[12..23]
    float mg;
    int H, P;
};
// m: where mg and q_feet come from -- the batch's BatchPackConst, or with ENVT (srbd_batch_set_env_params)
// environment e's record envs[e], as fill_input forms fzref and cost_feet from that record on the host.
template <bool CEM, bool ENVT>
__device__ __forceinline__ void batch_pack_body(const srbd_batch_device_io& io, int H, int P,
                                                const std::conditional_t<ENVT, EnvModel, BatchPackConst>& m, int vec,
                                                StepInput* in_arr, const srbd_batch_cem_io& cem, int svec) {
#pragma clang fp contract(off)
    const int e = blockIdx.x, tid = threadIdx.x;
    StepInput* __restrict__ in = in_arr + e;
    if constexpr (CEM) {
        if (cem.sigma_reset > 0.0f) {
            for (int i = tid; i < P; i += 64) in->sigma[i] = cem.sigma_reset;
        } else {
            const float* __restrict__ sp = cem.sigma + (size_t)e * P;
            if (svec)
                for (int i = tid; i < P / 4; i += 64)
                    reinterpret_cast<float4*>(in->sigma)[i] = reinterpret_cast<const float4*>(sp)[i];
            else
                for (int i = tid; i < P; i += 64) in->sigma[i] = sp[i];
        }
    }
    const float* __restrict__ st = io.states + 24 * (size_t)e;
    const float* __restrict__ rf = io.refs + 24 * (size_t)e;
    const float* __restrict__ bp = io.best_params + (size_t)e * P;
    static_assert(offsetof(StepInput, state) == 0 && offsetof(StepInput, ref) == 96, "state | ref head the input");
    if (vec) {
        if (tid < 12)
            reinterpret_cast<float4*>(in)[tid] =
                tid < 6 ? reinterpret_cast<const float4*>(st)[tid] : reinterpret_cast<const float4*>(rf)[tid - 6];
        for (int i = tid; i < P / 4; i += 64)
            reinterpret_cast<float4*>(in->best)[i] = reinterpret_cast<const float4*>(bp)[i];
    } else {
        if (tid < 48) reinterpret_cast<float*>(in)[tid] = tid < 24 ? st[tid] : rf[tid - 24];
        for (int i = tid; i < P; i += 64) in->best[i] = bp[i];
    }
    if (tid < MAXH) {  // column n of the four legs
        const int n = tid;
        const float* __restrict__ ct = io.contacts + (size_t)e * 4 * io.contact_stride + n;
        float c[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            c[l] = n < H ? ct[(size_t)l * io.contact_stride] : 0.0f;
            in->contact[l][n] = c[l];
        }
        if (n < H) in->fzref[n] = m.mg / (((c[0] + c[1]) + c[2]) + c[3]);  // inf when no leg is in stance
    } else if (tid == MAXH) {
        float cf = 0.0f;
#pragma unroll
        for (int i = 12; i < 24; ++i) {
            const float d = st[i] - rf[i];
            cf = cf + (d * m.q_feet[i - 12]) * d;
        }
        in->cost_feet = cf;
        const uint64_t seed = io.seeds[e], counter = io.counters[e];
        in->seed_lo = (uint32_t)seed;
        in->seed_hi = (uint32_t)(seed >> 32);
        in->ctr_lo = (uint32_t)counter;
        in->ctr_hi = (uint32_t)(counter >> 32);
        in->noise_scaled = io.noise ? 1 : 0;
    }
}
__global__ void __launch_bounds__(64) batch_pack_kernel(const srbd_batch_device_io io, const BatchPackConst pc, int vec,
                                                        StepInput* __restrict__ in_arr,
                                                        const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.x)) return;
    batch_pack_body<false, false>(io, pc.H, pc.P, pc, vec, in_arr, srbd_batch_cem_io{nullptr, 0.0f, 0}, 0);
}
__global__ void __launch_bounds__(64) batch_pack_cem_kernel(const srbd_batch_device_io io, const BatchPackConst pc,
                                                            int vec, StepInput* __restrict__ in_arr,
                                                            const srbd_batch_cem_io cem, int svec,
                                                            const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.x)) return;
    batch_pack_body<true, false>(io, pc.H, pc.P, pc, vec, in_arr, cem, svec);
}
template <bool CEM>
__global__ void __launch_bounds__(64) batch_pack_env_kernel(const srbd_batch_device_io io, int H, int P, int vec,
                                                            StepInput* __restrict__ in_arr,
                                                            const EnvModel* __restrict__ envs,
                                                            const srbd_batch_cem_io cem, int svec,
                                                            const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.x)) return;
    batch_pack_body<CEM, true>(io, H, P, envs[(int)blockIdx.x], vec, in_arr, cem, svec);
}

// srbd_batch_set_env_params_device: one thread per environment.  A selected environment's record (39 floats of the
// caller's array) is checked as srbd_create checks a configuration; when it passes, the raw fields go to raw[e]
// (srbd_batch_get_env_params) and the derived record to envs[e] through env_model_fill, the function the host setter
// and srbd_create's model call; when it fails, both are left alone and rejected[e] = 1.  A masked-out environment's
// record is neither read nor written; its rejected word is 0.
__global__ void __launch_bounds__(64) batch_set_env_params_kernel(const srbd_env_params* __restrict__ params,
                                                                  const int32_t* __restrict__ mask,
                                                                  int32_t* __restrict__ rejected, int E,
                                                                  srbd_env_params* __restrict__ raw,
                                                                  EnvModel* __restrict__ envs) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    int rej = 0;
    if (!mask || mask[e] != 0) {
        const srbd_env_params p = params[e];
        if (env_params_ok(p)) {
            EnvModel m;
            env_model_fill(p, &m);
            raw[e] = p;
            envs[e] = m;
        } else {
            rej = 1;
        }
    }
    if (rejected) rejected[e] = rej;
}

// out[e] (the merge blocks' records, device memory) and environment e's costs row into the caller's arrays: copies
// only.  vec: best_params, grf and predicted_state are 16-byte aligned.
// CEM (batch_unpack_cem_kernel): out[e].sigma into the caller's sigma row too (threads 192 .. 255; svec: 16-byte
// aligned).
template <bool CEM>
__device__ __forceinline__ void batch_unpack_body(const srbd_batch_device_io& io,
                                                  const StepOutput* __restrict__ out_arr,
                                                  const float* __restrict__ costs_arr, int P, int N, int ldn, int vec,
                                                  float* __restrict__ sigma, int svec) {
    const int e = blockIdx.x, tid = threadIdx.x;
    const StepOutput* __restrict__ o = out_arr + e;
    if constexpr (CEM) {
        static_assert(offsetof(StepOutput, sigma) % 16 == 0, "float4 reads");
        if (tid >= 192) {
            if (svec)
                for (int i = tid - 192; i < P / 4; i += 64)
                    reinterpret_cast<float4*>(sigma + (size_t)e * P)[i] = reinterpret_cast<const float4*>(o->sigma)[i];
            else
                for (int i = tid - 192; i < P; i += 64) sigma[(size_t)e * P + i] = o->sigma[i];
        }
    }
    static_assert(offsetof(StepOutput, grf) % 16 == 0 && offsetof(StepOutput, pred) % 16 == 0, "float4 reads");
    if (vec) {
        for (int i = tid; i < P / 4; i += 256)
            reinterpret_cast<float4*>(io.best_params + (size_t)e * P)[i] = reinterpret_cast<const float4*>(o->best)[i];
        if (tid >= 64 && tid < 67)
            reinterpret_cast<float4*>(io.grf + 12 * (size_t)e)[tid - 64] = reinterpret_cast<const float4*>(o->grf)[tid - 64];
        if (tid >= 67 && tid < 73)
            reinterpret_cast<float4*>(io.predicted_state + 24 * (size_t)e)[tid - 67] =
                reinterpret_cast<const float4*>(o->pred)[tid - 67];
    } else {
        for (int i = tid; i < P; i += 256) io.best_params[(size_t)e * P + i] = o->best[i];
        if (tid >= 64 && tid < 76) io.grf[12 * (size_t)e + tid - 64] = o->grf[tid - 64];
        if (tid >= 76 && tid < 100) io.predicted_state[24 * (size_t)e + tid - 76] = o->pred[tid - 76];
    }
    if (tid == 128) {
        io.best_cost[e] = o->best_cost;
        io.best_index[e] = o->best_index;
        io.best_freq[e] = o->best_freq;
        io.status[e] = o->status;
    }
    if (io.costs)
        for (int i = tid; i < N; i += 256) io.costs[(size_t)e * N + i] = costs_arr[(size_t)e * ldn + i];
}
__global__ void __launch_bounds__(256) batch_unpack_kernel(const srbd_batch_device_io io,
                                                           const StepOutput* __restrict__ out_arr,
                                                           const float* __restrict__ costs_arr, int P, int N, int ldn,
                                                           int vec, const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.x)) return;
    batch_unpack_body<false>(io, out_arr, costs_arr, P, N, ldn, vec, nullptr, 0);
}
__global__ void __launch_bounds__(256) batch_unpack_cem_kernel(const srbd_batch_device_io io,
                                                               const StepOutput* __restrict__ out_arr,
                                                               const float* __restrict__ costs_arr, int P, int N,
                                                               int ldn, int vec, float* __restrict__ sigma,
                                                               int svec, const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.x)) return;
    batch_unpack_body<true>(io, out_arr, costs_arr, P, N, ldn, vec, sigma, svec);
}

// fill_gait (srbd_api.hip) on the device, one block per environment: thread 0 forms environment e's candidate set
// (ga_freq_set) and writes the gait fields of in[e] through the function the host compiles (ga_write_fields), so they
// are the host path's bytes; nothing else of in[e] is written.  With injected frequencies every thread copies rows
// k = tid, tid + blockDim.x, ... < N of freq_rows[e] to ga_freq[e ldn + k]; the padding rows N .. ldn stay zero.
__global__ void __launch_bounds__(256) batch_set_gait_kernel(const BatchGaitJob j, StepInput* __restrict__ in_arr,
                                                             float* __restrict__ ga_freq,
                                                             const int32_t* __restrict__ due) {
    const int e = blockIdx.x, tid = threadIdx.x;
    if (not_due(due, e)) return;
    if (tid == 0) {
        float timing[4], set[SRBD_MAX_FREQS];
#pragma unroll
        for (int l = 0; l < 4; ++l)
            timing[l] = j.io.pgg ? (float)j.io.pgg[e].phase_signal[l] : j.io.timings[4 * (size_t)e + l];
        const float nominal = j.io.nominal_freqs ? j.io.nominal_freqs[e] : (float)j.io.pgg[e].step_freq;
        ga_freq_set(j.random_sampling, j.io.optimize[e], nominal, j.io.available, j.io.n_freq, set);
        ga_write_fields(in_arr + e, timing, j.io.pgg_dt, j.io.duty_factor, set, j.io.n_freq, j.cb, GA_MAXCB,
                        j.io.freq_rows != nullptr);
    }
    if (j.io.freq_rows)
        for (int k = tid; k < j.N; k += blockDim.x)
            ga_freq[(size_t)e * j.ldn + k] = j.io.freq_rows[(size_t)e * j.N + k];
}

__global__ void __launch_bounds__(256) batch_rng_kernel(const ModelConst mc, const StepInput* __restrict__ in,
                                                        float* __restrict__ noise,
                                                        const int32_t* __restrict__ due) {
    const int e = blockIdx.y;
    if (not_due(due, e)) return;
    const RngJob job{noise + (size_t)e * mc.P * mc.ldn, 0, 0, 1, 0, nullptr};  // keyed by in[e] (dev_ctr)
    rng_items(mc, in + e, job, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// transpose_kernel with one matrix per environment on blockIdx.z
__global__ void __launch_bounds__(256) batch_transpose_kernel(const float* __restrict__ src, int n, int P, int ldn,
                                                              float* __restrict__ dst,
                                                              const int32_t* __restrict__ due) {
    if (not_due(due, blockIdx.z)) return;
    transpose_tile(src + (size_t)blockIdx.z * n * P, n, P, ldn, dst + (size_t)blockIdx.z * P * ldn, blockIdx.x * 32,
                   blockIdx.y * 32);
}

// rollout_quad_kernel<KIND, HT, ST, CEMT, EXT> (srbd_kernels.hip) with the environment on blockIdx.y and that
// kernel's horizon restated, so the costs and records are its bits; CEMT (srbd_batch_create_cem) and EXT
// (srbd_batch_set_cost_terms) are that kernel's forms, and the measured reasons for the pin, the slot windows and
// CLEAD are written there.  Added here: the environment's offsets, the model view and KRE (below).  Left out: the
// step input by value and the in-launch draws, folds and merges.  (One shared body for both kernels was tried and
// dropped: inlined from a common function the horizon allocates more registers or spills in several instantiations
// of either file -- DESIGN section 4.)
// ENVT (srbd_batch_set_env_params): the robot's and the cost's constants -- inv_m, the inertia and its inverse, the
// force bounds, mu, Q -- come from envs[env], this block's environment record, instead of mc.  The address is
// block-uniform and the array is read-only through a restrict pointer, so the values are scalar loads made once ahead
// of the horizon (they take the SGPRs the kernel argument's fields took).  The other instantiations take a model view
// of mc (model_view); they are passed envs == NULL and never read it.
template <bool ENVT>
__device__ __forceinline__ auto model_view(const ModelConst& mc, const EnvModel* __restrict__ envs, int env) {
    if constexpr (ENVT)
        return EnvRegs(envs[env]);
    else
        return McConst{mc};
}
template <int KIND, int HT, int ST, bool CEMT, bool EXT, bool ENVT>  // rollout_quad_kernel's order; ENVT trails
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) batch_rollout_kernel(
    const ModelConst mc, const StepInput* __restrict__ in_arr, const float* __restrict__ noise_arr,
    float* __restrict__ costs_arr, float* __restrict__ recs_arr, int rec_stride,
    const EnvModel* __restrict__ envs, const int32_t* __restrict__ due) {
    const int env = blockIdx.y;
    if (not_due(due, env)) return;  // no draws read, no costs, no leaf record
    const auto kc = model_view<ENVT>(mc, envs, env);
    const StepInput* __restrict__ in = in_arr + env;
    const float* __restrict__ noise = noise_arr + (size_t)env * mc.P * mc.ldn;
    float* __restrict__ costs = costs_arr + (size_t)env * mc.ldn;
    float* __restrict__ recs = recs_arr + (size_t)env * mc.nleaf * rec_stride;
    const int nroll = gridDim.x;

    constexpr bool CT = HT > 0 && (KIND == SRBD_ZERO_ORDER || ST > 0);
    const int SPB = 64;  // one leaf per block
    const int H = CT ? HT : mc.H;
    const int S = CT ? ST : mc.S;
    const int PL = CT ? (KIND == SRBD_ZERO_ORDER ? 3 * HT : (KIND == SRBD_LINEAR_SPLINE ? 3 * (ST + 1) : 12 * ST))
                      : mc.PL;
    // ZST (zero-order, compile-time horizon H <= 12): the noise a lane reads stays raw in its registers and goes to
    // LDS after the horizon, where the leaf sums read it (38.5 KB per block: four blocks per CU)
    constexpr bool ZST = CT && KIND == SRBD_ZERO_ORDER && !EXT && HT <= 12;
    constexpr int PCT = ZST ? 12 * HT : 1;
    constexpr int ZSTR = PCT + 1;
    __shared__ __attribute__((aligned(16))) float zst[ZST ? 64 * ZSTR : 1];
    __shared__ float bls[ZST ? PCT : 1];
    __shared__ float sls[ZST && CEMT ? PCT : 1];  // CEMT: sigma beside best (39.6 KB per block: still four per CU)
    const int tid = threadIdx.x;
    const int q4 = tid & 3;
    const int c = q4 < 3 ? q4 : 2;
    const int sib = tid >> 2;
    const int k = blockIdx.x * SPB + sib;
    const bool valid = k < mc.n_local;
    const size_t ldn = (size_t)mc.ldn;
    const float* __restrict__ nz = noise + k;
    const float* __restrict__ best = in->best;
    const bool zs = CEMT && zs_scaled(mc, in);  // CEMT: CEM kernels only carry the scaling code

    // lane constants
    const QuadLane L = quad_lane(kc, c);
    const float Qp = sel3(c, kc.Q(0), kc.Q(1), kc.Q(2)), Qv = sel3(c, kc.Q(3), kc.Q(4), kc.Q(5));
    const float Qr = sel3(c, kc.Q(6), kc.Q(7), kc.Q(8)), Qw = sel3(c, kc.Q(9), kc.Q(10), kc.Q(11));
    const float* st = in->state;
    const float* rf = in->ref;
    const float rp = sel3(c, rf[0], rf[1], rf[2]), rv = sel3(c, rf[3], rf[4], rf[5]);
    const float rr = sel3(c, rf[6], rf[7], rf[8]), rw = sel3(c, rf[9], rf[10], rf[11]);
    float feet[4];  // EXT: this lane's component of every foot
#pragma unroll
    for (int l = 0; l < 4; ++l) feet[l] = sel3(c, st[12 + 3 * l], st[13 + 3 * l], st[14 + 3 * l]);
    float p = sel3(c, st[0], st[1], st[2]), v = sel3(c, st[3], st[4], st[5]);
    float r = sel3(c, st[6], st[7], st[8]), w = sel3(c, st[9], st[10], st[11]);
    float cost = 0.0f;
    // EXT: this lane's component of extra_cost_step
    const float rwc = sel3(c, mc.cost_r[0], mc.cost_r[1], mc.cost_r[2]);
    float fprev[4];
    constexpr bool LEGP = !EXT;  // the force phase leg-parallel; EXT keeps the component-parallel form
    const int lq = q4;  // this lane's leg in the force phase
    uint32_t lmask[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) lmask[l] = lq == l ? ~0u : 0u;
    float footL[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) footL[q] = st[12 + 3 * lq + q];
    constexpr int NCL = ZST ? HT : 1;
    float clreg[NCL];
    if constexpr (ZST) {
#pragma unroll
        for (int n = 0; n < HT; ++n) clreg[n] = in->contact[lq][n];
    }

    // specialised shapes: every parameter this lane reads over the horizon is loaded before the first step
    constexpr int NPRE = !CT ? 1 : (KIND == SRBD_ZERO_ORDER ? HT : (KIND == SRBD_LINEAR_SPLINE ? ST + 1 : 4 * ST));
    // LEGP: pre[q][i] = component q's slot i of this lane's leg; else pre[l][i] = this lane's component's slot i
    // of leg l
    float pre[LEGP ? 3 : 4][NPRE];
    // noise through a buffer descriptor over this environment's matrix alone (P ldn 4 < 2^31, checked at create):
    // a lane's offset can never reach another environment's rows
    const int cblk = LEGP ? lq * PL
                          : (KIND == SRBD_ZERO_ORDER ? c * HT : (KIND == SRBD_LINEAR_SPLINE ? c * (ST + 1) : 4 * c));
    const auto nrs = __builtin_amdgcn_make_buffer_rsrc((void*)noise, (short)0, mc.P * mc.ldn * 4, 0x00020000);
    const int voff = (cblk * mc.ldn + k) * 4;
    const float* __restrict__ bl = best + cblk;
    const float* __restrict__ sl = in->sigma + cblk;
    if constexpr (ZST) {  // best (and sigma) -> LDS
        for (int j = tid; j < PCT; j += 256) {
            bls[j] = best[j];
            if constexpr (CEMT) sls[j] = in->sigma[j];
        }
    }
    auto load_slot = [&](const int i) __attribute__((always_inline)) {
#pragma unroll
        for (int l = 0; l < (LEGP ? 3 : 4); ++l) {
            const int jr = LEGP ? (KIND == SRBD_ZERO_ORDER ? l * HT + i
                                   : (KIND == SRBD_LINEAR_SPLINE ? l * (ST + 1) + i : 10 * (i >> 2) + 4 * l + (i & 3)))
                                : l * PL + (KIND == SRBD_CUBIC_SPLINE ? 10 * (i >> 2) + (i & 3) : i);
            const float nzv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(nrs, voff, jr * mc.ldn * 4, 0));
            if constexpr (ZST) {
                pre[l][i] = nzv;  // raw: best is added at use, the value staged for the epilogue
            } else if constexpr (CEMT) {  // unscaled CEM device draws: Z * sigma_j (z * 1 == z; the load unconditional)
                const float sj = sl[jr];
                pre[l][i] = bl[jr] + nzv * (zs ? sj : 1.0f);
            } else {
                pre[l][i] = bl[jr] + nzv;
            }
        }
    };
    // EXT zero-order: slot n + PW loads at step n
    constexpr int PW = (EXT && KIND == SRBD_ZERO_ORDER) ? (NPRE < 4 ? NPRE : 4) : NPRE;
    // CEM cubic splines with S > 1: chunk q's four slots are loaded CLEAD steps before its first step instead of up
    // front, as rollout_quad_kernel does (without the window its C3 kernel spills 80 B per lane instead of 16)
    constexpr int CLEAD = 2;
    constexpr bool CWIN = CT && CEMT && KIND == SRBD_CUBIC_SPLINE && ST > 1;
    if constexpr (CWIN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_slot(i);
    } else if constexpr (CT) {
#pragma unroll
        for (int i = 0; i < PW; ++i) load_slot(i);
    }
    if constexpr (ZST) {  // the LDS copy of best is complete (the noise loads stay in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    float dep = p;  // step_ptr dependency: set part-way through each step
    auto step = [&](const int n) __attribute__((always_inline)) {
        if constexpr (CT && PW < NPRE)
            if (n + PW < NPRE) load_slot(n + PW);  // n is a compile-time constant here (unrolled horizon)
        if constexpr (CWIN) {
#pragma unroll
            for (int q = 1; q < (CWIN ? ST : 1); ++q) {
                const int at = q * HT / ST - CLEAD;
                if (n == (at > 0 ? at : 0))
#pragma unroll
                    for (int i = 4 * q; i < 4 * q + 4; ++i) load_slot(i);
            }
        }
        const auto is = step_ptr(in, dep);
        float cl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (!ZST)
#pragma unroll
            for (int l = 0; l < 4; ++l) cl[l] = is->contact[l][n];
        const float fref = is->fzref[n];
        const float dt = mc.dts[n];
        const float sq = mc.sq[n], somq = mc.somq[n], sa = mc.sa[n], sb = mc.sb[n], scc = mc.sc[n], sd = mc.sd[n];
        const int idx = CT && KIND != SRBD_ZERO_ORDER ? chunk_index(n, HT, ST) : mc.sidx[n];
        float ex = 0.0f;
        if constexpr (LEGP) {
            const float clq = ZST ? clreg[ZST ? n : 0]
                                  : __uint_as_float((__float_as_uint(cl[0]) & lmask[0]) | (__float_as_uint(cl[1]) & lmask[1]) |
                                                    (__float_as_uint(cl[2]) & lmask[2]) | (__float_as_uint(cl[3]) & lmask[3]));
            const int lbase = lq * PL;
            // component q of this leg's decoded force (slot i, parameter j of the leg when not prefetched)
            auto PQ = [&](int q, int i, int j) {
                if constexpr (ZST) {
                    if constexpr (CEMT) return bls[lbase + j] + pre[q][i] * (zs ? sls[lbase + j] : 1.0f);
                    return bls[lbase + j] + pre[q][i];
                } else if constexpr (CT) {
                    return pre[q][i];
                } else {
                    const float z = nz[(size_t)(lbase + j) * ldn];
                    if constexpr (CEMT) return best[lbase + j] + (zs ? z * in->sigma[lbase + j] : z);
                    return best[lbase + j] + z;
                }
            };
            float rq[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (KIND == SRBD_ZERO_ORDER) {
                    rq[q] = PQ(q, n, n + q * H);
                } else if (KIND == SRBD_LINEAR_SPLINE) {
                    const int o = idx + q * (S + 1);
                    rq[q] = somq * PQ(q, idx, o) + sq * PQ(q, idx + 1, o + 1);
                } else {
                    const int o = 10 * idx + 4 * q;
                    const float p0 = PQ(q, 4 * idx, o), p1 = PQ(q, 4 * idx + 1, o + 1), p2 = PQ(q, 4 * idx + 2, o + 2),
                                p3 = PQ(q, 4 * idx + 3, o + 3);
                    const float phi = 0.5f * ((p2 - p1) + (p1 - p0));
                    const float phin = 0.5f * ((p3 - p2) + (p2 - p1));
                    rq[q] = sa * p1 + sb * phi + scc * p2 + sd * phin;
                }
            }
            // shape_leg / clip_leg (srbd_core.h), this lane's leg
            const float fz = clamp_cs((fref + rq[2]) * clq, kc.grf_min(), kc.grf_max());
            const float lo = kc.neg_mu() * fz, hi = kc.mu() * fz;
            const float fx = clamp_cs(third(rq[0] * clq), lo, hi), fy = clamp_cs(third(rq[1] * clq), lo, hi);
            // integrate(): skew_dot(p_foot - p, f) * c (the position's components from their lanes)
            const float vx = footL[0] - qp<QP_B0>(p), vy = footL[1] - qp<QP_B1>(p), vz = footL[2] - qp<QP_B2>(p);
            float sm[6] = {fx * clq, fy * clq, fz * clq, ((-vz) * fy + vy * fz) * clq, (vz * fx + (-vx) * fz) * clq,
                           ((-vy) * fx + vx * fy) * clq};
#pragma unroll
            for (int i = 0; i < 6; ++i) {  // quad butterfly: (l0 + l1) + (l2 + l3) on every lane (adds commute)
                sm[i] = sm[i] + qp<QP_XOR1>(sm[i]);
                sm[i] = sm[i] + qp<QP_XOR2>(sm[i]);
            }
            const float temp = sel3(c, sm[0], sm[1], sm[2]);
            dep = sm[5];  // the next step's scalar loads issue from here on (step_ptr)
            quad_rb_apply3(kc, L, quad_rb_prep(L, r, w), temp, sm[3], sm[4], sm[5], dt, p, v, r, w);
        } else {
            float tf[4], tt[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const int base = l * PL;
                // parameter j of this leg (i: its slot in the prefetched block when the shape is specialised)
                auto P = [&](int i, int j) {
                    if constexpr (CT) {
                        return pre[l][i];
                    } else {
                        const float z = nz[(size_t)(base + j) * ldn];
                        if constexpr (CEMT) return best[base + j] + (zs ? z * in->sigma[base + j] : z);
                        return best[base + j] + z;
                    }
                };
                float raw;
                if (KIND == SRBD_ZERO_ORDER) {
                    raw = P(n, n + c * H);
                } else if (KIND == SRBD_LINEAR_SPLINE) {
                    const int o = idx + c * (S + 1);
                    raw = somq * P(idx, o) + sq * P(idx + 1, o + 1);
                } else {
                    const int o = 10 * idx + 4 * c;
                    const float p0 = P(4 * idx, o), p1 = P(4 * idx + 1, o + 1), p2 = P(4 * idx + 2, o + 2),
                                p3 = P(4 * idx + 3, o + 3);
                    const float phi = 0.5f * ((p2 - p1) + (p1 - p0));
                    const float phin = 0.5f * ((p3 - p2) + (p2 - p1));
                    raw = sa * p1 + sb * phi + scc * p2 + sd * phin;
                }
                // shape_leg / clip_leg, component-wise
                float zp = clamp_cs((fref + raw) * cl[l], kc.grf_min(), kc.grf_max());
                const float xy = third(raw * cl[l]);
                const float fz = qp<QP_B2>(c == 2 ? zp : xy);
                const float f = c == 2 ? fz : clamp_cs(xy, kc.neg_mu() * fz, kc.mu() * fz);
                tf[l] = f * cl[l];
                tt[l] = quad_cross(feet[l] - p, f) * cl[l];
                // extra_cost_step (srbd_core.h), this lane's component, leg by leg
                const float u = c == 2 ? f - (cl[l] != 0.0f ? fref : 0.0f) : f;
                float term = (u * rwc) * u;
                if (n > 0) {
                    const float d = f - fprev[l];
                    term = term + (d * mc.cost_smooth) * d;
                }
                {  // x / y lanes only, as a select
                    float vv = fabsf(xy) - kc.mu() * fz;
                    vv = vv > 0.0f ? vv : 0.0f;
                    const float cone = (vv * mc.cost_cone) * vv;
                    term = c < 2 ? term + cone : term;
                }
                ex = ex + term;
                fprev[l] = f;
            }
            const float temp = (tf[0] + tf[1]) + (tf[2] + tf[3]);
            const float temp2 = (tt[0] + tt[1]) + (tt[2] + tt[3]);
            dep = temp2;  // the next step's scalar loads issue from here on (step_ptr)
            quad_rigid_body(kc, L, temp, temp2, dt, p, v, r, w);
        }
        // tracking cost (NMPC:451), accumulated per component lane
        const float ep = p - rp, ev = v - rv, er_ = r - rr, ew = w - rw;
        const float tp = (ep * Qp) * ep, tv = (ev * Qv) * ev, tr = (er_ * Qr) * er_, tw = (ew * Qw) * ew;
        cost = cost + (((tp + tv) + tr) + tw);
        if constexpr (EXT) {
            cost = cost + ex;
            asm volatile("" : "+v"(cost));  // each step's terms stay in their step
        }
    };
    if constexpr (CT) {
        unroll_seq([&](auto nc) { step(decltype(nc)::value); }, std::make_integer_sequence<int, (CT ? HT : 1)>{});
    } else {
        for (int n = 0; n < H; ++n) step(n);
    }
    cost = (qp<QP_B0>(cost) + qp<QP_B1>(cost)) + qp<QP_B2>(cost);
    cost = cost + in->cost_feet;  // 0, or NaN when a foot term is non-finite (Q_feet = 0)
    if (isnan(cost) || isinf(cost)) cost = 1000000.0f;
    // KRE (the zero-order and linear CEM forms at H 16): the sample's index is formed again behind the horizon, tied to
    // the cost so it is not hoisted.  Kept live across the unrolled horizon it is the value those two forms spill (12 B
    // of scratch per lane, where rollout_quad_kernel's CEM forms of the shapes have none).  Not elsewhere: no other form
    // spills it, and the C3 form (cubic H 16) measured 4-6 % slower per step with it.
    constexpr bool KRE = CEMT && CT && !EXT && HT == 16 && KIND != SRBD_CUBIC_SPLINE;
    int k_t = k;
    if constexpr (KRE) {
        int sib_t = tid >> 2;
        asm volatile("" : "+v"(sib_t) : "v"(cost));
        k_t = blockIdx.x * SPB + sib_t;
    }
    if (valid && q4 == 0) costs[k_t] = cost;
    if constexpr (ZST) {  // the block's noise, sample-major (leg lq's block of columns lq PL .. lq PL + PL - 1)
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int i = 0; i < NPRE; ++i) zst[sib * ZSTR + lq * PL + q * HT + i] = pre[q][i];
    }
    const GroupArgs grp{nullptr, nullptr, 1, nullptr};  // gsize 1: leaf records only
    block_epilogue<CEMT, ZST>(mc, in, SPB, q4 == 0 ? sib : -1, valid, cost, noise, recs, rec_stride, 0.0f, grp, nroll,
                              ZST ? zst : nullptr, ZSTR);
}

// rollout_ga_quad_kernel<KIND, HT> (srbd_kernels.hip) with the environment on blockIdx.y (srbd_batch_set_gait): the
// sample's step frequency, contact masks, stance counters and per-leg spline coefficients on each of its four lanes,
// the decode of this lane's component, the rigid-body step, the tracking cost and the frequency term, statement for
// statement; the leaf record carries the frequency as its tag (-> StepOutput::best_freq).  Everything the sample's
// gait depends on is environment e's: in[e]'s leg phases, frequency set, seed and counter (the JAX streams:
// jax_choice_index on in[e]'s key).  Injected frequencies: row k of environment e at ga_freq_arr[e ldn + k] (k < ldn;
// mc.ga_freq, one context's pointer, is not read).  Left out: the in-launch draws.
// ENVT: as in batch_rollout_kernel; fz_ns, the gravity share per stance count, is the environment's too.
template <int KIND, int HT, bool ENVT = false>
__global__ void __launch_bounds__(512) batch_rollout_ga_kernel(const ModelConst mc, const StepInput* __restrict__ in_arr,
                                                               const float* __restrict__ noise_arr,
                                                               float* __restrict__ costs_arr,
                                                               float* __restrict__ recs_arr, int rec_stride,
                                                               const float* __restrict__ ga_freq_arr,
                                                               const EnvModel* __restrict__ envs,
                                                               const int32_t* __restrict__ due) {
    const int env = blockIdx.y;
    if (not_due(due, env)) return;
    const auto kc = model_view<ENVT>(mc, envs, env);
    const StepInput* __restrict__ in = in_arr + env;
    const float* __restrict__ noise = noise_arr + (size_t)env * mc.P * mc.ldn;
    float* __restrict__ costs = costs_arr + (size_t)env * mc.ldn;
    float* __restrict__ recs = recs_arr + (size_t)env * mc.nleaf * rec_stride;
    const int nroll = gridDim.x;

    const int H = HT > 0 ? HT : mc.H, S = mc.S, PL = mc.PL;  // HT: horizon fixed at compile time
    const int tid = threadIdx.x;
    const int q4 = tid & 3;
    const int c = q4 < 3 ? q4 : 2;
    const int sib = tid >> 2;
    const int SPB = 64;  // one leaf per block
    const int k = blockIdx.x * SPB + sib;  // < nleaf 64 <= ldn
    const bool valid = k < mc.n_local;
    const size_t ldn = (size_t)mc.ldn;
    const float* __restrict__ nz = noise + k;
    const float* __restrict__ best = in->best;

    // ga_sample_freq with the injected row read from this environment's slice
    const float f = in->ga_explicit ? ga_freq_arr[(size_t)env * ldn + k] : ga_sample_freq(mc, in, k);
    uint32_t mask[4];
    ga_contact_masks(in, H, f, mask);
    float seg[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) seg[l] = ((float)__popc(mask[l]) + 1.0f) / (float)S;
    int cnt[4] = {-1, -1, -1, -1};

    const QuadLane L = quad_lane(kc, c);
    const float Qp = sel3(c, kc.Q(0), kc.Q(1), kc.Q(2)), Qv = sel3(c, kc.Q(3), kc.Q(4), kc.Q(5));
    const float Qr = sel3(c, kc.Q(6), kc.Q(7), kc.Q(8)), Qw = sel3(c, kc.Q(9), kc.Q(10), kc.Q(11));
    const float* st_ = in->state;
    const float* rf = in->ref;
    const float rp = sel3(c, rf[0], rf[1], rf[2]), rv = sel3(c, rf[3], rf[4], rf[5]);
    const float rr = sel3(c, rf[6], rf[7], rf[8]), rw = sel3(c, rf[9], rf[10], rf[11]);
    float feet[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) feet[l] = sel3(c, st_[12 + 3 * l], st_[13 + 3 * l], st_[14 + 3 * l]);
    float p = sel3(c, st_[0], st_[1], st_[2]), v = sel3(c, st_[3], st_[4], st_[5]);
    float r = sel3(c, st_[6], st_[7], st_[8]), w = sel3(c, st_[9], st_[10], st_[11]);
    float cost = 0.0f;
    // unrolled when HT > 0: every step's parameter loads depend only on the contact masks, so they issue ahead of the
    // physics chain
    constexpr int UNR = HT > 0 ? HT : 1;
#pragma unroll UNR
    for (int n = 0; n < H; ++n) {
        float cl[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const uint32_t b = (mask[l] >> n) & 1u;
            cl[l] = b ? 1.0f : 0.0f;
            cnt[l] += (int)b;
        }
        const float ns = ((cl[0] + cl[1]) + cl[2]) + cl[3];
        const float fref = kc.fz_ns((int)ns);
        float tf[4], tt[4];  // per-leg force / torque contributions, summed pairwise (integrate()'s order)
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int base = l * PL;
            auto acc = [&](int j) {
                j = j < 0 ? j + PL : j;
                return best[base + j] + nz[(size_t)(base + j) * ldn];
            };
            const int stc = cnt[l];
            float raw;
            if (KIND == SRBD_ZERO_ORDER) {
                raw = acc(stc + c * H);
            } else {
                int idx = 0;
                for (int i = 0; i <= S; ++i)
                    if (stc >= in->ga_cb[i]) idx = i;
                float tau = (float)stc / seg[l];
                tau = tau - (float)idx;
                const float q = tau / 1.0f;
                if (KIND == SRBD_LINEAR_SPLINE) {
                    const float omq = 1.0f - q;
                    const int o = idx + c * (S + 1);
                    raw = omq * acc(o) + q * acc(o + 1);
                } else {
                    const float a = 2.0f * q * q * q - 3.0f * q * q + 1.0f;
                    const float bb = (q * q * q - 2.0f * q * q + q) * 1.0f;
                    const float cc = -2.0f * q * q * q + 3.0f * q * q;
                    const float d = (q * q * q - q * q) * 1.0f;
                    const int o = 10 * idx + 4 * c;
                    const float p0 = acc(o), p1 = acc(o + 1), p2 = acc(o + 2), p3 = acc(o + 3);
                    const float phi = 0.5f * ((p2 - p1) + (p1 - p0));
                    const float phin = 0.5f * ((p3 - p2) + (p2 - p1));
                    raw = a * p1 + bb * phi + cc * p2 + d * phin;
                }
            }
            const float zp = clamp_cs((fref + raw) * cl[l], kc.grf_min(), kc.grf_max());
            const float xy = third(raw * cl[l]);
            const float fz = qp<QP_B2>(c == 2 ? zp : xy);
            const float fo = c == 2 ? fz : clamp_cs(xy, kc.neg_mu() * fz, kc.mu() * fz);
            tf[l] = fo * cl[l];
            tt[l] = quad_cross(feet[l] - p, fo) * cl[l];
        }
        const float temp = (tf[0] + tf[1]) + (tf[2] + tf[3]), temp2 = (tt[0] + tt[1]) + (tt[2] + tt[3]);
        quad_rigid_body(kc, L, temp, temp2, mc.dts[n], p, v, r, w);
        const float ep = p - rp, ev = v - rv, er_ = r - rr, ew = w - rw;
        const float tp = (ep * Qp) * ep, tv = (ev * Qv) * ev, tr = (er_ * Qr) * er_, tw = (ew * Qw) * ew;
        cost = cost + (((tp + tv) + tr) + tw);
    }
    cost = (qp<QP_B0>(cost) + qp<QP_B1>(cost)) + qp<QP_B2>(cost);
    cost = cost + in->cost_feet;
    const float df = f - 1.3f;
    cost = cost + (df * 100.0f) * df;  // GA:500
    if (isnan(cost) || isinf(cost)) cost = 1000000.0f;
    if (valid && q4 == 0) costs[k] = cost;
    const GroupArgs grp{nullptr, nullptr, 1, nullptr};  // gsize 1: leaf records only
    block_epilogue<false>(mc, in, SPB, q4 == 0 ? sib : -1, valid, cost, noise, recs, rec_stride, f, grp, nroll);
}

// One block per environment (blockIdx.y; blockIdx.x == 0, as merge_body's unsplit form expects): the environment's
// leaf records folded to the root and out[e] written, exactly as merge_kernel does for one problem.  merge_body ends
// with every wave's output stores complete, a system release by thread 0 (fence_sys) and its own publish word
// (eflag[e], device memory, unread).  Then thread 0 counts its block; the last arriver resets the counter for the
// next launch and stores `seq` into the host's word -- after every block's outputs, so one word publishes them all.
// ENVT (srbd_batch_set_env_params): the tail lanes' final GRFs and predicted state use envs[e] (merge_body's ENVT).
// The due mask: a block whose environment is not due skips merge_body -- in[e], its records, out[e] and eflag[e] are
// neither written nor read -- and still takes part in the arrival count, so the count reaches gridDim.y, the counter
// is zero again and `seq` is published whatever the mask holds, an all-zero one included.
template <int NT, bool STAGE, bool ENVT = false>
__global__ void __launch_bounds__(NT) batch_merge_kernel(const ModelConst mc, StepInput* __restrict__ in,
                                                         const float* __restrict__ recs, int rec_stride,
                                                         const float* __restrict__ noise,
                                                         StepOutput* __restrict__ out, uint32_t* __restrict__ eflag,
                                                         uint32_t* __restrict__ count, uint32_t* __restrict__ flag,
                                                         uint32_t seq, const EnvModel* __restrict__ envs,
                                                         const int32_t* __restrict__ due) {
    const int e = blockIdx.y;
    __shared__ MergeShared<NT> sh;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    if (!not_due(due, e))
        merge_body<NT, STAGE, false, ENVT>(mc, in + e, recs + (size_t)e * mc.nleaf * rec_stride, mc.nleaf, rec_stride,
                                           0, noise + (size_t)e * mc.P * mc.ldn, nullptr, out + e, 0, 0, nullptr,
                                           eflag + e, seq, 0, 1, sh, dsm, false, 0, nullptr,
                                           ENVT ? envs + e : nullptr);
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == gridDim.y - 1) {
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ------------------------------------------------------------------ launchers
void batch_prepare() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&batch_merge_kernel<MERGE_STAGE_THREADS, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)MERGE_LDS_DYN_MAX);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&batch_merge_kernel<MERGE_STAGE_THREADS, true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)MERGE_LDS_DYN_MAX);
}

void launch_batch_copy(const StepInput* in_host, StepInput* in, int E, size_t bytes, hipStream_t s, size_t off2,
                       size_t bytes2) {
    if (bytes2)
        hipLaunchKernelGGL(batch_copy2_kernel, dim3(E), dim3(256), 0, s, (const uint4*)in_host, (uint4*)in,
                           (int)(bytes / 16), (int)(sizeof(StepInput) / 16), (int)(off2 / 16), (int)(bytes2 / 16));
    else
        hipLaunchKernelGGL(batch_copy_kernel, dim3(E), dim3(256), 0, s, (const uint4*)in_host, (uint4*)in,
                           (int)(bytes / 16), (int)(sizeof(StepInput) / 16));
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void launch_batch_pack(const ModelConst& mc, const float* q_feet, const srbd_batch_device_io& io, StepInput* in, int E,
                       hipStream_t s, const srbd_batch_cem_io* cem, const EnvModel* envs, const int32_t* due) {
    if (envs) {
        const int v = aligned16(io.states) && aligned16(io.refs) && aligned16(io.best_params);
        if (cem)
            hipLaunchKernelGGL(batch_pack_env_kernel<true>, dim3(E), dim3(64), 0, s, io, mc.H, mc.P, v, in, envs, *cem,
                               (int)aligned16(cem->sigma), due);
        else
            hipLaunchKernelGGL(batch_pack_env_kernel<false>, dim3(E), dim3(64), 0, s, io, mc.H, mc.P, v, in, envs,
                               srbd_batch_cem_io{nullptr, 0.0f, 0}, 0, due);
        return;
    }
    BatchPackConst pc;
    for (int i = 0; i < 12; ++i) pc.q_feet[i] = q_feet[i];
    pc.mg = mc.mg;
    pc.H = mc.H;
    pc.P = mc.P;
    const int vec = aligned16(io.states) && aligned16(io.refs) && aligned16(io.best_params);
    if (cem)
        hipLaunchKernelGGL(batch_pack_cem_kernel, dim3(E), dim3(64), 0, s, io, pc, vec, in, *cem,
                           (int)aligned16(cem->sigma), due);
    else
        hipLaunchKernelGGL(batch_pack_kernel, dim3(E), dim3(64), 0, s, io, pc, vec, in, due);
}

void launch_batch_unpack(const ModelConst& mc, const srbd_batch_device_io& io, const StepOutput* out,
                         const float* costs, int E, hipStream_t s, float* sigma, const int32_t* due) {
    const int vec = aligned16(io.best_params) && aligned16(io.grf) && aligned16(io.predicted_state);
    if (sigma)
        hipLaunchKernelGGL(batch_unpack_cem_kernel, dim3(E), dim3(256), 0, s, io, out, costs, mc.P, mc.n_local, mc.ldn,
                           vec, sigma, (int)aligned16(sigma), due);
    else
        hipLaunchKernelGGL(batch_unpack_kernel, dim3(E), dim3(256), 0, s, io, out, costs, mc.P, mc.n_local, mc.ldn,
                           vec, due);
}

void launch_batch_set_env_params(const srbd_env_params* params, const int32_t* mask, int32_t* rejected, int E,
                                 srbd_env_params* raw, EnvModel* envs, hipStream_t s) {
    hipLaunchKernelGGL(batch_set_env_params_kernel, dim3((E + 63) / 64), dim3(64), 0, s, params, mask, rejected, E, raw,
                       envs);
}

void launch_batch_set_gait(const BatchGaitJob& j, StepInput* in, float* ga_freq, int E, hipStream_t s,
                           const int32_t* due) {
    // one wave per environment for the fields alone; four when N rows are copied besides
    hipLaunchKernelGGL(batch_set_gait_kernel, dim3(E), dim3(j.io.freq_rows ? 256 : 64), 0, s, j, in, ga_freq, due);
}

void launch_batch_rng(const ModelConst& mc, const StepInput* in, float* noise, int E, hipStream_t s,
                      const int32_t* due) {
    // the draws do not depend on the grid (rng_items strides over the items): about 32 768 blocks in all
    const int gx = std::max(1, std::min(rng_grid(mc), 32768 / E));
    hipLaunchKernelGGL(batch_rng_kernel, dim3(gx, E), dim3(256), 0, s, mc, in, noise, due);
}

void launch_batch_transpose(const ModelConst& mc, const float* src, float* noise, int E, hipStream_t s,
                            const int32_t* due) {
    const dim3 grid((mc.n_local + 31) / 32, (mc.P + 31) / 32, E);
    hipLaunchKernelGGL(batch_transpose_kernel, grid, dim3(256), 0, s, src, mc.n_local, mc.P, mc.ldn, noise, due);
}

void launch_batch_rollout(const ModelConst& mc, const StepInput* in, const float* noise, float* costs, float* recs,
                          int rec_stride, int E, hipStream_t s, const EnvModel* envs, const int32_t* due) {
    const dim3 grid(mc.nleaf, E);
    const int H = mc.H, S = mc.S;
    // mc.cost_on (srbd_batch_set_cost_terms): the EXT instantiations, on the same compile-time shapes; CEM
    // (srbd_batch_create_cem): the CEMT ones, with or without EXT, as launch_rollout_t picks them
    const bool cem = mc.method == SRBD_CEM_MPPI;
    const EnvModel* const none = nullptr;
#define SRBD_BR_(K, HH, SS, ENVT, EV)                                                                             \
    {                                                                                                             \
        if (cem && mc.cost_on)                                                                                    \
            hipLaunchKernelGGL((batch_rollout_kernel<K, HH, SS, true, true, ENVT>), grid, dim3(256), 0, s, mc,    \
                               in, noise, costs, recs, rec_stride, EV, due);                                      \
        else if (cem)                                                                                             \
            hipLaunchKernelGGL((batch_rollout_kernel<K, HH, SS, true, false, ENVT>), grid, dim3(256), 0, s, mc,   \
                               in, noise, costs, recs, rec_stride, EV, due);                                      \
        else if (mc.cost_on)                                                                                      \
            hipLaunchKernelGGL((batch_rollout_kernel<K, HH, SS, false, true, ENVT>), grid, dim3(256), 0, s, mc,   \
                               in, noise, costs, recs, rec_stride, EV, due);                                      \
        else                                                                                                      \
            hipLaunchKernelGGL((batch_rollout_kernel<K, HH, SS, false, false, ENVT>), grid, dim3(256), 0, s, mc,  \
                               in, noise, costs, recs, rec_stride, EV, due);                                      \
        return;                                                                                                   \
    }
#define SRBD_BR(K, HH, SS) SRBD_BR_(K, HH, SS, false, none)
#define SRBD_BRE(K, HH, SS) SRBD_BR_(K, HH, SS, true, envs)
    if (envs) {
        // per-environment parameters: the flagship's compile-time shape (zero-order, H 12) and the generic kernel of
        // each parametrization -- every shape returns srbd_step's bits, so the choice only costs time
        switch (mc.kind) {
            case SRBD_ZERO_ORDER:
                if (H == 12) SRBD_BRE(SRBD_ZERO_ORDER, 12, 0);
                SRBD_BRE(SRBD_ZERO_ORDER, 0, 0);
            case SRBD_LINEAR_SPLINE:
                SRBD_BRE(SRBD_LINEAR_SPLINE, 0, 0);
            default:
                SRBD_BRE(SRBD_CUBIC_SPLINE, 0, 0);
        }
    }
    switch (mc.kind) {  // launch_rollout's compile-time shapes
        case SRBD_ZERO_ORDER:
            if (H == 10) SRBD_BR(SRBD_ZERO_ORDER, 10, 0);
            if (H == 12) SRBD_BR(SRBD_ZERO_ORDER, 12, 0);
            if (H == 16) SRBD_BR(SRBD_ZERO_ORDER, 16, 0);
            SRBD_BR(SRBD_ZERO_ORDER, 0, 0);
        case SRBD_LINEAR_SPLINE:
            if (S == 2 && H == 12) SRBD_BR(SRBD_LINEAR_SPLINE, 12, 2);
            if (S == 2 && H == 16) SRBD_BR(SRBD_LINEAR_SPLINE, 16, 2);
            SRBD_BR(SRBD_LINEAR_SPLINE, 0, 0);
        default:
            if (S == 2 && H == 12) SRBD_BR(SRBD_CUBIC_SPLINE, 12, 2);
            if (S == 2 && H == 16) SRBD_BR(SRBD_CUBIC_SPLINE, 16, 2);
            SRBD_BR(SRBD_CUBIC_SPLINE, 0, 0);
    }
#undef SRBD_BR
#undef SRBD_BRE
#undef SRBD_BR_
}

void launch_batch_rollout_ga(const ModelConst& mc, const StepInput* in, const float* noise, float* costs, float* recs,
                             int rec_stride, const float* ga_freq, int E, hipStream_t s, const EnvModel* envs,
                             const int32_t* due) {
    const dim3 grid(mc.nleaf, E);
    const int H = mc.H;
    const EnvModel* const none = nullptr;
#define SRBD_BG_(K, HH, ENVT, EV)                                                                                 \
    {                                                                                                             \
        hipLaunchKernelGGL((batch_rollout_ga_kernel<K, HH, ENVT>), grid, dim3(256), 0, s, mc, in, noise, costs,   \
                           recs, rec_stride, ga_freq, EV, due);                                                   \
        return;                                                                                                   \
    }
#define SRBD_BG(K, HH) SRBD_BG_(K, HH, false, none)
#define SRBD_BGE(K, HH) SRBD_BG_(K, HH, true, envs)
    if (envs) {  // as launch_batch_rollout picks them
        switch (mc.kind) {
            case SRBD_ZERO_ORDER:
                if (H == 12) SRBD_BGE(SRBD_ZERO_ORDER, 12);
                SRBD_BGE(SRBD_ZERO_ORDER, 0);
            case SRBD_LINEAR_SPLINE:
                SRBD_BGE(SRBD_LINEAR_SPLINE, 0);
            default:
                SRBD_BGE(SRBD_CUBIC_SPLINE, 0);
        }
    }
    switch (mc.kind) {  // launch_rollout_ga's compile-time shapes
        case SRBD_ZERO_ORDER:
            if (H == 10) SRBD_BG(SRBD_ZERO_ORDER, 10);
            if (H == 12) SRBD_BG(SRBD_ZERO_ORDER, 12);
            if (H == 16) SRBD_BG(SRBD_ZERO_ORDER, 16);
            SRBD_BG(SRBD_ZERO_ORDER, 0);
        case SRBD_LINEAR_SPLINE:
            if (H == 12) SRBD_BG(SRBD_LINEAR_SPLINE, 12);
            if (H == 16) SRBD_BG(SRBD_LINEAR_SPLINE, 16);
            SRBD_BG(SRBD_LINEAR_SPLINE, 0);
        default:
            if (H == 12) SRBD_BG(SRBD_CUBIC_SPLINE, 12);
            if (H == 16) SRBD_BG(SRBD_CUBIC_SPLINE, 16);
            SRBD_BG(SRBD_CUBIC_SPLINE, 0);
    }
#undef SRBD_BG
#undef SRBD_BGE
#undef SRBD_BG_
}

void launch_batch_merge(const ModelConst& mc, StepInput* in, const float* recs, int rec_stride, const float* noise,
                        StepOutput* out, uint32_t* eflag, uint32_t* count, uint32_t* flag, uint32_t seq, int E,
                        hipStream_t s, const EnvModel* envs, const int32_t* due) {
    size_t smem = 0;
    const dim3 grid(1, E);
    const EnvModel* const none = nullptr;
    const bool stage = merge_stage_fits(mc.nleaf, rec_stride, mc.P, mc.K, &smem);
    if (stage && envs)
        hipLaunchKernelGGL((batch_merge_kernel<MERGE_STAGE_THREADS, true, true>), grid, dim3(MERGE_STAGE_THREADS), smem,
                           s, mc, in, recs, rec_stride, noise, out, eflag, count, flag, seq, envs, due);
    else if (stage)
        hipLaunchKernelGGL((batch_merge_kernel<MERGE_STAGE_THREADS, true>), grid, dim3(MERGE_STAGE_THREADS), smem, s, mc,
                           in, recs, rec_stride, noise, out, eflag, count, flag, seq, none, due);
    else if (envs)
        hipLaunchKernelGGL((batch_merge_kernel<MERGE_THREADS, false, true>), grid, dim3(MERGE_THREADS), smem, s, mc, in,
                           recs, rec_stride, noise, out, eflag, count, flag, seq, envs, due);
    else
        hipLaunchKernelGGL((batch_merge_kernel<MERGE_THREADS, false>), grid, dim3(MERGE_THREADS), smem, s, mc, in, recs,
                           rec_stride, noise, out, eflag, count, flag, seq, none, due);
}

}  // namespace srbd
