// srbd_plan.hip -- the full-horizon plan of one parameter row per environment (srbd_batch_plan_device, srbd_plan;
// include/srbd_mpc.h): plan_kernel rolls params[e] out from states[e], refs[e] and the contact sequence once and keeps
// what the step's rollout computes and drops -- the state after every step, the shaped forces, the contact flags, the
// running cost -- besides the row's final cost.
// One thread per environment, the thread-per-sample body of srbd_rollout_thread.hip (rollout_kernel's horizon and
// epilogue for caller-given contacts, rollout_ga_kernel's for gait-adaptive sampling) on the shared functions of
// srbd_core.h and srbd_device.h, statement for statement and unfused, so every float is the one the step's rollout
// formed for a row with these parameters (the four-lane kernels of the batch agree with the thread form bit for bit).
// Built without SLP vectorisation as that file is, for the same reason.
// What the step reads from in[e] and the launch has no in[e] for is formed here as batch_pack_kernel / fill_input form
// it: fzref[n] = mg / (((c0 + c1) + c2) + c3) and cost_feet.  Gait-adaptive sampling reads the gait fields of the
// environment's StepInput (leg phases, PGG dt, duty factor, chunk boundaries), which the gait setters wrote.
// Stores: a lane's outputs are H x 29 floats of its own environment, so stored directly a wave would write 64 rows
// 4 bytes at a time.  The block stages them in LDS in the arrays' own order and writes every array with contiguous
// 16-byte stores (flush_rows).  A chunk of at most PLAN_CHUNK_MAX steps is staged at a time; longer horizons flush
// once per chunk.
#include "srbd_device.h"

namespace srbd {

// LDS floats of one block staging hc steps: states and forces in rows of 12 hc + 4 (an odd number of 16-byte slots, so
// the lanes' 16-byte writes spread over the banks), contacts [4][hc] and the running cost [hc] unpadded.
__host__ __device__ constexpr int plan_row(int hc) { return 12 * hc + 4; }
__host__ __device__ constexpr size_t plan_lds_bytes(int hc) {
    return sizeof(float) * PLAN_ENVS * (size_t)(2 * plan_row(hc) + 5 * hc);
}
static_assert(plan_lds_bytes(PLAN_CHUNK_MAX) <= PLAN_LDS_MAX, "a chunk fits the dynamic LDS limit");

// nrows rows of `run` floats, LDS row r at l + r lstr -> g + r gstr, by the block's one wave; rows that are contiguous
// on both sides are one run.  16-byte loads and stores when both sides are aligned.
__device__ __forceinline__ void flush_rows(const float* l, int lstr, float* __restrict__ g, size_t gstr, int run,
                                           int nrows, int tid) {
    if (lstr == run && gstr == (size_t)run) {
        run *= nrows;
        nrows = 1;
    }
    const bool vec = (((unsigned)lstr | (unsigned)run | (unsigned)gstr) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(g) & 15) == 0 && (reinterpret_cast<uintptr_t>(l) & 15) == 0;
    for (int r = 0; r < nrows; ++r) {
        const float* lr = l + (size_t)r * lstr;
        float* __restrict__ gr = g + (size_t)r * gstr;
        if (vec)
            for (int k = tid; k < run / 4; k += PLAN_ENVS)
                reinterpret_cast<float4*>(gr)[k] = reinterpret_cast<const float4*>(lr)[k];
        else
            for (int k = tid; k < run; k += PLAN_ENVS) gr[k] = lr[k];
    }
}

// GA: the contact flags come from the environment's gait fields and freqs[e] (rollout_ga_kernel), else from
// contacts[e] (rollout_kernel).  ENVT (srbd_batch_set_env_params): the robot's and the cost's constants from envs[e].
template <int KIND, bool GA, bool ENVT>
__global__ void __launch_bounds__(PLAN_ENVS) plan_kernel(const ModelConst mc, const PlanJob j) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = mc.H, S = mc.S, PL = mc.PL, HC = j.hc;
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * PLAN_ENVS;
    const int nlive = j.E - e0 < PLAN_ENVS ? j.E - e0 : PLAN_ENVS;
    const bool valid = tid < nlive;
    const int e = e0 + (valid ? tid : 0);  // a lane past E rolls the block's first environment out and stores nothing
    const int SROW = plan_row(HC);
    float* const lS = lds;
    float* const lG = lS + PLAN_ENVS * SROW;
    float* const lC = lG + PLAN_ENVS * SROW;
    float* const lR = lC + PLAN_ENVS * 4 * HC;

    const EnvModel* const em = ENVT ? j.envs + e : nullptr;
    const auto kc = [&] {
        if constexpr (ENVT)
            return EnvConst{*em};
        else
            return McConst{mc};
    }();
    const float* __restrict__ st = j.states + 24 * (size_t)e;
    const float* __restrict__ rf = j.refs + 24 * (size_t)e;
    const float* __restrict__ pr = j.params + (size_t)e * mc.P;
    const float* __restrict__ ct = GA ? nullptr : j.contacts + (size_t)e * 4 * j.contact_stride;
    const StepInput* __restrict__ in = GA ? j.in_arr + (j.in_single ? 0 : e) : nullptr;

    float x[12], feet[12], ref[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        x[i] = st[i];
        feet[i] = st[12 + i];
        ref[i] = rf[i];
    }
    // cost_feet as fill_input / batch_pack_kernel form it
    float cost_feet = 0.0f;
#pragma unroll
    for (int i = 12; i < 24; ++i) {
        const float d = st[i] - rf[i];
        cost_feet = cost_feet + (d * (ENVT ? em->q_feet[i - 12] : j.q_feet[i - 12])) * d;
    }
    const float mg = ENVT ? em->mg : j.mg;

    float f = 0.0f;
    uint32_t mask[4] = {0u, 0u, 0u, 0u};
    float seg[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    int cnt[4] = {-1, -1, -1, -1};
    if constexpr (GA) {
        f = j.freqs[e];
        ga_contact_masks(in, H, f, mask);
#pragma unroll
        for (int l = 0; l < 4; ++l) seg[l] = ((float)__popc(mask[l]) + 1.0f) / (float)S;
    }

    float cost3[3] = {0.0f, 0.0f, 0.0f};
    const bool extra = mc.cost_on != 0;  // opt-in cost terms (srbd_set_cost_terms)
    // extra_cost_step reads the weights and mu from a ModelConst: the shared one, with the environment's mu under ENVT
    // (the four values are all it reads, so the copy is four registers)
    const auto extra_step = [&](auto&&... a) {
        if constexpr (ENVT) {
            ModelConst mcx = mc;
            mcx.mu = em->mu;
            extra_cost_step(mcx, a...);
        } else {
            extra_cost_step(mc, a...);
        }
    };
    float Fprev[12];
    for (int n0 = 0; n0 < H; n0 += HC) {
        const int hc = H - n0 < HC ? H - n0 : HC;
        for (int jn = 0; jn < hc; ++jn) {
            const int n = n0 + jn;
            float c[4], fref;
            if constexpr (GA) {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const uint32_t b = (mask[l] >> n) & 1u;
                    c[l] = b ? 1.0f : 0.0f;
                    cnt[l] += (int)b;
                }
                const float ns = ((c[0] + c[1]) + c[2]) + c[3];
                fref = kc.fz_ns((int)ns);
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l) c[l] = ct[(size_t)l * j.contact_stride + n];
                fref = mg / (((c[0] + c[1]) + c[2]) + c[3]);  // inf when no leg is in stance
            }
            float F[12], RX[4], RY[4];
#pragma unroll
            for (int leg = 0; leg < 4; ++leg) {
                const int base = leg * PL;
                auto acc = [&](int i) {
                    if constexpr (GA) i = i < 0 ? i + PL : i;  // jnp's negative index before the first touchdown
                    return pr[base + i];
                };
                float fx, fy, fz;
                if constexpr (GA) {
                    const int stc = cnt[leg];
                    int idx = 0;
                    float q = 0.0f, omq = 0.0f, a = 0.0f, bb = 0.0f, cc = 0.0f, d = 0.0f;
                    if (KIND != SRBD_ZERO_ORDER) {  // rollout_ga_kernel's per-leg spline coefficients
                        for (int i = 0; i <= S; ++i)
                            if (stc >= in->ga_cb[i]) idx = i;
                        float tau = (float)stc / seg[leg];
                        tau = tau - (float)idx;
                        q = tau / 1.0f;
                        omq = 1.0f - q;
                        a = 2.0f * q * q * q - 3.0f * q * q + 1.0f;
                        bb = (q * q * q - 2.0f * q * q + q) * 1.0f;
                        cc = -2.0f * q * q * q + 3.0f * q * q;
                        d = (q * q * q - q * q) * 1.0f;
                    }
                    decode_leg(KIND, H, S, idx, q, omq, a, bb, cc, d, stc, acc, fx, fy, fz);
                } else {
                    decode_leg(KIND, H, S, mc.sidx[n], mc.sq[n], mc.somq[n], mc.sa[n], mc.sb[n], mc.sc[n], mc.sd[n], n,
                               acc, fx, fy, fz);
                }
                RX[leg] = fx;
                RY[leg] = fy;
                shape_leg_k(kc, fref, c[leg], fx, fy, fz);
                F[3 * leg] = fx;
                F[3 * leg + 1] = fy;
                F[3 * leg + 2] = fz;
            }
            integrate_k(kc, x, feet, F, c, mc.dts[n]);
            // tracking cost (NMPC:451) per component
            float t[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const float er = x[i] - ref[i];
                t[i] = (er * kc.Q(i)) * er;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) cost3[q] = cost3[q] + (((t[q] + t[3 + q]) + t[6 + q]) + t[9 + q]);
            if (extra) extra_step(n, F, RX, RY, c, fref, Fprev, cost3);
            // this step's outputs into the block's stage
            if (j.plan_states) {
                float4* o = reinterpret_cast<float4*>(lS + tid * SROW + 12 * jn);
#pragma unroll
                for (int i = 0; i < 3; ++i) o[i] = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
            }
            if (j.plan_grfs) {
                float4* o = reinterpret_cast<float4*>(lG + tid * SROW + 12 * jn);
#pragma unroll
                for (int i = 0; i < 3; ++i) o[i] = make_float4(F[4 * i], F[4 * i + 1], F[4 * i + 2], F[4 * i + 3]);
            }
            if (j.plan_contacts) {
#pragma unroll
                for (int l = 0; l < 4; ++l) lC[tid * 4 * HC + l * HC + jn] = c[l];
            }
            if (j.plan_run_cost) lR[tid * HC + jn] = (cost3[0] + cost3[1]) + cost3[2];
        }
        __syncthreads();
        if (j.plan_states)
            flush_rows(lS, SROW, j.plan_states + ((size_t)e0 * H + n0) * 12, (size_t)H * 12, 12 * hc, nlive, tid);
        if (j.plan_grfs)
            flush_rows(lG, SROW, j.plan_grfs + ((size_t)e0 * H + n0) * 12, (size_t)H * 12, 12 * hc, nlive, tid);
        if (j.plan_contacts) {
            if (HC == H) {
                flush_rows(lC, 4 * H, j.plan_contacts + (size_t)e0 * 4 * H, (size_t)4 * H, 4 * H, nlive, tid);
            } else {
                for (int l = 0; l < 4; ++l)
                    flush_rows(lC + l * HC, 4 * HC, j.plan_contacts + (size_t)e0 * 4 * H + (size_t)l * H + n0,
                               (size_t)4 * H, hc, nlive, tid);
            }
        }
        if (j.plan_run_cost) flush_rows(lR, HC, j.plan_run_cost + (size_t)e0 * H + n0, (size_t)H, hc, nlive, tid);
        __syncthreads();
    }
    if (j.plan_cost) {
        float cost = (cost3[0] + cost3[1]) + cost3[2];
        cost = cost + cost_feet;  // 0, or NaN when a foot term is non-finite (Q_feet = 0)
        if constexpr (GA) {
            const float df = f - 1.3f;
            cost = cost + (df * 100.0f) * df;  // GA:500
        }
        if (isnan(cost) || isinf(cost)) cost = 1000000.0f;  // NMPC:686-687
        if (valid) j.plan_cost[e] = cost;
    }
}

// ------------------------------------------------------------------ launcher (srbd_launch.h)
int plan_chunk(int H) {
    const int nchunks = (H + PLAN_CHUNK_MAX - 1) / PLAN_CHUNK_MAX;
    return (H + nchunks - 1) / nchunks;
}

template <int KIND, bool GA, bool ENVT>
static hipError_t launch_plan_t(const ModelConst& mc, const PlanJob& j, hipStream_t s) {
    const void* fn = reinterpret_cast<const void*>(&plan_kernel<KIND, GA, ENVT>);
    const size_t smem = plan_lds_bytes(j.hc);
    if (smem > 64 * 1024) {  // the limit a launch gets without the attribute
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLAN_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((plan_kernel<KIND, GA, ENVT>), dim3((j.E + PLAN_ENVS - 1) / PLAN_ENVS), dim3(PLAN_ENVS), smem, s,
                       mc, j);
    return hipSuccess;
}

hipError_t launch_plan(const ModelConst& mc, const PlanJob& j, hipStream_t s) {
#define SRBD_PL(K)                                                            \
    {                                                                         \
        if (mc.ga) {                                                          \
            if (j.envs) return launch_plan_t<K, true, true>(mc, j, s);       \
            return launch_plan_t<K, true, false>(mc, j, s);                  \
        }                                                                     \
        if (j.envs) return launch_plan_t<K, false, true>(mc, j, s);          \
        return launch_plan_t<K, false, false>(mc, j, s);                     \
    }
    switch (mc.kind) {
        case SRBD_ZERO_ORDER:
            SRBD_PL(SRBD_ZERO_ORDER)
        case SRBD_LINEAR_SPLINE:
            SRBD_PL(SRBD_LINEAR_SPLINE)
        default:
            SRBD_PL(SRBD_CUBIC_SPLINE)
    }
#undef SRBD_PL
}

}  // namespace srbd
