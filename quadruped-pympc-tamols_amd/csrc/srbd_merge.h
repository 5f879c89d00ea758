// srbd_merge.h -- the merge of one problem's reduction-tree records (merge_body), shared by the merge kernels of
// srbd_kernels.hip and the batched merge of srbd_batch.hip.
#pragma once

#include "srbd_quad.h"

namespace srbd {

// ------------------------------------------------------------------ merge
__device__ __forceinline__ uint64_t rec_key(const float* R, int P, int q) {
    return ((uint64_t)f2u(R[REC_HDR + P + 2 * q + 1]) << 32) | (uint64_t)f2u(R[REC_HDR + P + 2 * q]);
}

constexpr int MERGE_THREADS = 1024;
constexpr int MERGE_RPT = 8;    // record headers per thread (nrec <= MERGE_RPT * MERGE_THREADS)
// The LDS-staged merge runs two waves per SIMD: its phases are short dependent chains that every
// wave repeats (index math, the beta reduction), so 16 waves pay ~2x the issue of 8, while fewer
// waves stage the records more slowly (C2 merge 9.0 / 8.4 / 9.8 us at 1024 / 512 / 256 threads).
constexpr int MERGE_STAGE_THREADS = 512;
// Block-wide K smallest record keys (ascending) into `elite`, by selection and ranks.  Every record's
// key list is the sorted K smallest keys of its samples, so its first key is its minimum, and the K
// smallest keys overall lie in the K records with the smallest minima (any other record's minimum already
// exceeds K keys of those records).  Keys are unique (cost bits, row); only the ~0 padding repeats.
//  1. the K smallest record minima, with their records: per chunk of NT records, every record's rank in
//     its wave's 64 minima (64 independent LDS-broadcast compares) sends the wave's K smallest to a
//     candidate list, then the candidates' ranks among themselves and the K carried from the chunks
//     before (<= NW K + K compares) keep the K smallest;
//  2. those records' K-key lists (K x K keys), ranked among themselves, give the K smallest keys.
// Compares are independent, so the phase is issue-bound (~4 us at C3's 1024 records) where K dependent
// rounds of DPP wave minima per level were latency-bound (10 us).  Caller syncs afterwards.
template <int NT>
struct TopkLds {
    static constexpr int NCT = (NT / 64) * MAXK + MAXK > MAXK * MAXK ? (NT / 64) * MAXK + MAXK : MAXK * MAXK;
    uint64_t keys[NT > MAXK * MAXK ? NT : MAXK * MAXK];  // a chunk's record minima, then step 2's K x K keys
    uint64_t cand[NCT];  // candidates (block_topk_nodes: a K x K table)
    int cand_r[NCT];
    int cnt[MAXK * MAXK];                   // block_topk_nodes' rank counts
    uint64_t top[MAXK], ntop[MAXK];         // carried K smallest minima (and the next chunk's)
    int top_r[MAXK], ntop_r[MAXK];
    int sel[MAXK];                          // block_topk_nodes: the selected level-0 nodes
};
template <int NT>
__device__ __forceinline__ void block_topk_rank(const float* __restrict__ recs, int nrec, int rec_stride, int P, int K,
                                                uint64_t* elite, TopkLds<NT>& t) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, T = NT, wv = tid >> 6;
    const int NC = NW * K + K;  // candidates per chunk: the waves' K smallest + the carried K
    if (tid < K) {
        t.top[tid] = KEY_NONE;
        t.top_r[tid] = 0;
    }
    for (int base = 0; base < nrec; base += T) {
        const int r = base + tid;
        const uint64_t x = r < nrec ? rec_key(recs + (size_t)r * rec_stride, P, 0) : KEY_NONE;
        t.keys[tid] = x;
        for (int i = tid; i < NW * K; i += T) t.cand[i] = KEY_NONE;
        __syncthreads();
        const uint64_t* wk = t.keys + (wv << 6);
        int cnt = 0;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) cnt += wk[j] < x ? 1 : 0;
        if (cnt < K && x != KEY_NONE) {
            t.cand[wv * K + cnt] = x;
            t.cand_r[wv * K + cnt] = r;
        }
        if (tid < K) {
            t.cand[NW * K + tid] = t.top[tid];
            t.cand_r[NW * K + tid] = t.top_r[tid];
            t.ntop[tid] = KEY_NONE;
        }
        __syncthreads();
        if (tid < NC) {
            const uint64_t y = t.cand[tid];
            int c2 = 0;
            for (int j = 0; j < NC; ++j) c2 += t.cand[j] < y ? 1 : 0;
            if (c2 < K && y != KEY_NONE) {
                t.ntop[c2] = y;
                t.ntop_r[c2] = t.cand_r[tid];
            }
        }
        __syncthreads();
        if (tid < K) {
            t.top[tid] = t.ntop[tid];
            t.top_r[tid] = t.ntop_r[tid];
        }
        __syncthreads();
    }
    const int KK = K * K;
    for (int i = tid; i < KK; i += T) {
        const int e = i / K, q = i - e * K;
        t.keys[i] = t.top[e] != KEY_NONE ? rec_key(recs + (size_t)t.top_r[e] * rec_stride, P, q) : KEY_NONE;
    }
    if (tid < K) elite[tid] = KEY_NONE;
    __syncthreads();
    for (int i = tid; i < KK; i += T) {
        const uint64_t y = t.keys[i];
        int c3 = 0;
        for (int j = 0; j < KK; ++j) c3 += t.keys[j] < y ? 1 : 0;
        if (c3 < K && y != KEY_NONE) elite[c3] = y;
    }
}

// The same K smallest keys as block_topk_rank, from the keys the merge's header pass already holds: every
// record's key (its minimum) in t.keys[r] (KEY_NONE up to NT; nrec <= NT) and the tree's level-0 node keys
// nk[g] (the minimum of records [32 g, 32 g + 32)).  Far fewer compares (C3: ~2 k against ~95 k):
//  A. the K smallest node keys.  The K smallest record minima lie in those nodes: any other node has K nodes
//     below its minimum, so K records below each of its records;
//  B. in each selected node, every record's rank among the node's 32: its K smallest, in order, form row s of
//     a K x K candidate table;
//  C. a candidate's overall rank = the entries below it summed over the table's rows (one thread per
//     (candidate, row), counts added in LDS): the K smallest record minima and their records;
//  D. those records' key lists (each ascending) ranked the same way: the K smallest keys.
// Entry state, with a barrier since: t.sel[0, MAXK) = -1, t.top[0, MAXK) = KEY_NONE, t.cand[0, K K) = KEY_NONE,
// t.cnt[0, K K) = 0.  Caller syncs afterwards.
template <int NT>
__device__ __forceinline__ void block_topk_nodes(const float* __restrict__ recs, int nrec, int rec_stride, int P,
                                                 int K, const uint64_t* nk, uint64_t* elite, TopkLds<NT>& t,
                                                 uint64_t* dbg = nullptr) {
    const int tid = threadIdx.x, KK = K * K;
#define TOPK_MARK(i) \
    if (dbg && tid == 0 && blockIdx.x < 2) dbg[32 * blockIdx.x + 25 + (i)] = __builtin_amdgcn_s_memrealtime()
    const int n1 = (nrec + TREE_FAN - 1) / TREE_FAN;
    if (tid < n1) {  // A
        const uint64_t y = nk[tid];
        int c = 0;
#pragma unroll 8
        for (int g = 0; g < n1; ++g) c += nk[g] < y ? 1 : 0;
        if (c < K && y != KEY_NONE) t.sel[c] = tid;
    }
    __syncthreads();
    TOPK_MARK(0);
    for (int i = tid; i < K * TREE_FAN; i += NT) {  // B
        const int sl = i / TREE_FAN, g = t.sel[sl];
        if (g < 0) continue;
        const uint64_t* nodek = t.keys + g * TREE_FAN;
        const uint64_t y = nodek[i % TREE_FAN];  // KEY_NONE past nrec
        if (y == KEY_NONE) continue;
        int c = 0;
#pragma unroll
        for (int j = 0; j < TREE_FAN; ++j) c += nodek[j] < y ? 1 : 0;
        if (c < K) {
            t.cand[sl * K + c] = y;
            t.cand_r[sl * K + c] = g * TREE_FAN + i % TREE_FAN;
        }
    }
    __syncthreads();
    // cnt[i] = entries of the K x K table below entry i.  Every row is ascending (B: a node's K smallest record
    // minima by rank, KEY_NONE after them; D: a record's key list, ascending, KEY_NONE-padded) and the keys are
    // unique, so a row's count below y is its lower bound: found by binary lifting (five dependent LDS reads for
    // K <= 16) -- the same count as comparing every entry, a third of the LDS traffic (C3: 1.3 us per call so)
    static_assert(MAXK <= 31, "binary lifting from a step of 16");
    auto table_ranks = [&](const uint64_t* tab) {
        for (int i = tid; i < KK * K; i += NT) {
            const int c = i / K, b = i - c * K;
            const uint64_t y = tab[c];
            if (y == KEY_NONE) continue;
            const uint64_t* row = tab + b * K;
            int n = 0;
#pragma unroll
            for (int s = 16; s >= 1; s >>= 1)
                if (n + s <= K && row[n + s - 1] < y) n += s;
            if (n) atomicAdd(&t.cnt[c], n);
        }
    };
    TOPK_MARK(1);
    table_ranks(t.cand);  // C
    __syncthreads();
    TOPK_MARK(2);
    for (int c = tid; c < KK; c += NT) {
        const uint64_t y = t.cand[c];
        const int n = t.cnt[c];
        if (y != KEY_NONE && n < K) {
            t.top[n] = y;
            t.top_r[n] = t.cand_r[c];
        }
    }
    __syncthreads();
    for (int i = tid; i < KK; i += NT) {  // D
        const int e = i / K, q = i - e * K;
        t.keys[i] = t.top[e] != KEY_NONE ? rec_key(recs + (size_t)t.top_r[e] * rec_stride, P, q) : KEY_NONE;
        t.cnt[i] = 0;
    }
    if (tid < K) elite[tid] = KEY_NONE;
    __syncthreads();
    TOPK_MARK(3);
    table_ranks(t.keys);
    __syncthreads();
    TOPK_MARK(4);
#undef TOPK_MARK
    for (int i = tid; i < KK; i += NT) {
        const uint64_t y = t.keys[i];
        const int n = t.cnt[i];
        if (y != KEY_NONE && n < K) elite[n] = y;
    }
}

// One block merges `nrec` records (per-block records of one rank, or gathered rank records).
//  L. one memory round trip: record headers (min cost, best row) and the first MERGE_PREF weighted-
//     sum values of every (column j, record group g) thread;
//  1. global (min cost, first row) key beta;  2. per-record rescale exp(-(m_r - beta)) -> LDS;
//  3. sum_r scale_r * v_r[j] and sum_r scale_r * s_r in fixed order (groups, then columns);
//  4. top-K keys: per-thread sorted lists -> per-wave K-round DPP minima -> one wave over the 16
//     wave lists; 5. elite rows -> LDS;  6. outputs: rank record and/or final step outputs; with
//     `chain` the new parameters, sigma and RNG counter are written back into `in` (warm start).
// Column-split launch (split_cs > 0, final step outputs only): every block reads all record headers (beta
// and the normaliser are recomputed per block, in the same order, so they agree bit for bit); block b >= 1
// (a slice) folds the columns [(b-1)cs, b cs) and writes the non-tail ones and sigma; block 0 (the tail
// block) writes the mc.tailc columns final_grf_pred decodes, the GRFs, the predicted state and the step
// scalars.  They meet through SplitXchg (srbd_core.h) inside the launch: the slices publish their root sums
// and the tail block reads its columns' back (it folds none itself); for CEM the tail block computes the
// top-K once and the slices read it back.  Each block publishes flag[blockIdx.x] = seq.  This spreads the
// record reads over CUs and drops the single block's serial column loop (C2: 8.8 -> see DESIGN).
// STAGE: the block first copies its records into LDS with 16-byte loads (one memory round trip,
// a quarter of the load instructions of dword column reads; the whole per-block record array at C2 is
// 157 x 152 floats = 95 KB) and every later phase reads them from LDS.
// Host-published outputs (flag != NULL) are stored system-scope (write-through to the mapped host
// buffer); after every wave's vmcnt(0) and a barrier the flag store follows them, so the system-wide
// L2 write-back of __threadfence_system is not needed for them (fence_sys = 1 keeps it).
// The merge's fixed-size LDS, passed in so a caller can place it (the merge kernels declare it; the zero-order
// rollout's final merge carves it from its noise stage, rollout_quad_kernel).
// alignas(16): the dynamic LDS that follows it (staged records, read as float4) starts 16-byte aligned
// (an 8-byte aligned start cost the C2 merge 1 us)
template <int NT>
struct alignas(16) MergeShared {
    uint64_t red[NT / 64];
    uint64_t elite[MAXK];
    int elite_src[MAXK];
    TopkLds<NT> tk;  // block_topk_rank
    float Vs[MAXP + 1];
    float nb[MAXP];
    float tag_sh;  // header tag (gait-adaptive step frequency) of the record holding beta's row
    // tail lanes: StepInput fields (13), the force-independent step (5), the ModelConst values the tail
    // uses (16) -- read back in one batch (kernarg fields re-read lazily are serial scalar loads)
    float tail_sh[4][40];
    float osh[sizeof(StepOutput) / sizeof(float)];  // the step outputs assembled for the burst
};
// The merge's tail lanes (0..3, component qc of the four-lane layout): the step inputs they use (tail_pre: fzref[0],
// the legs' contact at step 0, p / v / rpy / omega and the feet, component qc), the force-independent part of the
// predicted state (NMPC:752-784 via CMJ:93-174) and the ModelConst values of the final GRFs, into the lane's row of
// tail_sh -- read back in one batch by the outputs phase.
template <class IN>
__device__ __forceinline__ void merge_tail_load(const IN* in, int qc, float* tail_pre) {
    tail_pre[0] = in->fzref[0];
#pragma unroll
    for (int l = 0; l < 4; ++l) tail_pre[1 + l] = in->contact[l][0];
#pragma unroll
    for (int q = 0; q < 4; ++q) tail_pre[5 + q] = in->state[3 * q + qc];  // p, v, rpy, omega
#pragma unroll
    for (int l = 0; l < 4; ++l) tail_pre[9 + l] = in->state[12 + 3 * l + qc];  // feet
}
// kc: the robot's constants (KView: the shared ModelConst, or the environment's record in a batch with per-environment
// parameters); the decode coefficients and dts[0] are always the shared ones.
template <class KC>
__device__ __forceinline__ void merge_tail_lane(const ModelConst& mc, const KC& kc, int qc, const float* tail_pre,
                                                float* row) {
    const QuadLane L = quad_lane(kc, qc);
    const QuadRB rb = quad_rb_prep(L, tail_pre[7], tail_pre[8]);
    row[36] = L.Ii0;
    row[37] = L.Ii1;
    row[38] = L.Ii2;
    row[39] = L.g;
#pragma unroll
    for (int i = 0; i < 13; ++i) row[i] = tail_pre[i];
    row[13] = rb.er;
    row[14] = rb.R0;
    row[15] = rb.R1;
    row[16] = rb.R2;
    row[17] = rb.a1;
    const int iv[5] = {mc.kind, mc.H, mc.PL, mc.S, mc.fidx};
#pragma unroll
    for (int i = 0; i < 5; ++i) row[18 + i] = __int_as_float(iv[i]);
    const float fv[13] = {mc.fq,        mc.fomq, mc.fa,       mc.fb,      mc.fc,     mc.fd, kc.grf_min(),
                          kc.grf_max(), kc.mu(), kc.neg_mu(), kc.inv_m(), mc.dts[0], 0.0f};
#pragma unroll
    for (int i = 0; i < 13; ++i) row[23 + i] = fv[i];
}
// Final GRFs (NMPC:695-750) and the predicted state (NMPC:752-784) on tail lane c (four-lane layout, all four lanes
// of the quad active): lane c decodes component c of every leg from the new parameters `nb` (decode_leg at step 0.0,
// horizon_leg 1), shapes and clips it as shape_leg does (the rollout's component form), then one Euler step from
// the prepared rigid-body terms.  ts: the lane's merge_tail_lane row.  One straight-line read of the legs' parameters
// per kind, so the reads issue together.  merge_body and fast_tail share it, so both give the same bits.
__device__ __forceinline__ void merge_tail_grf(int c, const float* ts, const float* nb, float f[4], float& p, float& v,
                                               float& r, float& w) {
    const float* tail_pre = ts;
    const QuadRB rb{ts[13], ts[14], ts[15], ts[16], ts[17]};
    const int kind = __float_as_int(ts[18]), H = __float_as_int(ts[19]), PL = __float_as_int(ts[20]),
              S = __float_as_int(ts[21]), fidx = __float_as_int(ts[22]);
    const float fq = ts[23], fomq = ts[24], fa = ts[25], fb = ts[26], fc = ts[27], fd = ts[28];
    const float gmin = ts[29], gmax = ts[30], mu = ts[31], neg_mu = ts[32];
    float raw[4];
    if (kind == SRBD_ZERO_ORDER) {
#pragma unroll
        for (int l = 0; l < 4; ++l) raw[l] = nb[l * PL + c * H];
    } else if (kind == SRBD_LINEAR_SPLINE) {
        float x0[4], x1[4];
        const int o = fidx + c * (S + 1);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            x0[l] = nb[l * PL + o];
            x1[l] = nb[l * PL + o + 1];
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) raw[l] = fomq * x0[l] + fq * x1[l];
    } else {
        float x[4][4];
        const int o = 10 * fidx + 4 * c;
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int k = 0; k < 4; ++k) x[l][k] = nb[l * PL + o + k];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float p0 = x[l][0], p1 = x[l][1], p2 = x[l][2], p3 = x[l][3];
            const float phi = 0.5f * ((p2 - p1) + (p1 - p0));
            const float phin = 0.5f * ((p3 - p2) + (p2 - p1));
            raw[l] = fa * p1 + fb * phi + fc * p2 + fd * phin;
        }
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const float cl = tail_pre[1 + l];
        const float zp = clamp_cs((tail_pre[0] + raw[l]) * cl, gmin, gmax);
        const float xy = third(raw[l] * cl);
        const float fz = qp<QP_B2>(c == 2 ? zp : xy);
        f[l] = c == 2 ? fz : clamp_cs(xy, neg_mu * fz, mu * fz);
    }
    p = tail_pre[5], v = tail_pre[6], r = tail_pre[7], w = tail_pre[8];
    const float c0 = tail_pre[1], c1 = tail_pre[2], c2 = tail_pre[3], c3 = tail_pre[4];
    const float temp = (f[0] * c0 + f[1] * c1) + (f[2] * c2 + f[3] * c3);  // integrate()'s order
    const float temp2 = (quad_cross(tail_pre[9] - p, f[0]) * c0 + quad_cross(tail_pre[10] - p, f[1]) * c1) +
                        (quad_cross(tail_pre[11] - p, f[2]) * c2 + quad_cross(tail_pre[12] - p, f[3]) * c3);
    {  // quad_rb_apply with the copies of inv_m / dt and this lane's constants
        const float lin = ts[33] * temp + ts[39];
        const float Rt = rb.R0 * qp<QP_B0>(temp2) + rb.R1 * qp<QP_B1>(temp2) + rb.R2 * qp<QP_B2>(temp2);
        const float a2 = ts[36] * qp<QP_B0>(Rt) + ts[37] * qp<QP_B1>(Rt) + ts[38] * qp<QP_B2>(Rt);
        const float aa = -rb.a1 + a2;
        const float dt = ts[34];
        const float pn = p + v * dt, vn = v + lin * dt, rn = r + rb.er * dt, wn = w + aa * dt;
        p = pn;
        v = vn;
        r = rn;
        w = wn;
    }
}

// smem: [STAGE: records] | scale[nrec_pad] | tree levels | node keys | erow[K*ncol] (merge_smem_bytes).  prestaged
// (STAGE): the records are already in smem.  The staged body's sums use G = MERGE_STAGE_THREADS / (ncol + 1)
// record groups whatever NT is, so a 256-thread block merges bit for bit as the 512-thread kernel does.
// ENVT (batch_merge_kernel with per-environment parameters): the tail lanes take the robot's constants from `em`, this
// block's environment record, instead of mc; nothing else of the merge reads them.
template <int NT, bool STAGE, bool SPLITX = false, bool ENVT = false>
__device__ __forceinline__ void merge_body(const ModelConst& mc, StepInput* __restrict__ in,
                                           const float* __restrict__ recs, int nrec, int rec_stride, int rows_in_rec,
                                           const float* __restrict__ noise, float* __restrict__ rank_out,
                                           StepOutput* __restrict__ out, int chain, int ctr_inc,
                                           uint64_t* __restrict__ dbg, uint32_t* __restrict__ flag, uint32_t seq,
                                           int split_cs, int fence_sys, MergeShared<NT>& sh, float* smem,
                                           bool prestaged = false, int levels_up = 0, SplitXchg* xg = nullptr,
                                           const EnvModel* __restrict__ em = nullptr) {
    constexpr int NW = NT / 64;
    uint64_t* red = sh.red;
    uint64_t* elite = sh.elite;
    int* elite_src = sh.elite_src;
    TopkLds<NT>& tk = sh.tk;
    float* Vs = sh.Vs;
    float* nb = sh.nb;
    float& tag_sh = sh.tag_sh;
    auto& tail_sh = sh.tail_sh;
    const int sblk = split_cs > 0 ? (int)blockIdx.x : 0;  // stamps: a split launch's blocks 0 and 1, else this block
#define MERGE_STAMP(i) \
    if (dbg && threadIdx.x == 0 && sblk < 2) dbg[32 * sblk + (i)] = __builtin_amdgcn_s_memrealtime()
    // finer marks (diagnostic build of the phases call only: dbg[16 + i])
#define MERGE_MARK(i) MERGE_STAMP(16 + (i))
    MERGE_STAMP(0);
    if (dbg && threadIdx.x == 0 && sblk < 2) dbg[32 * sblk + 8] = __builtin_amdgcn_s_memtime();  // clock

    // T: the launch's block size, a template constant (blockDim.x is a dependent load)
    const int tid = threadIdx.x, T = NT, lane = tid & 63, wv = tid >> 6;
    const int P = mc.P, K = mc.K;
    const bool rs = mc.method == SRBD_RANDOM_SAMPLING, cem = mc.method == SRBD_CEM_MPPI;
    const bool split = split_cs > 0;
    const bool tailblk = split && blockIdx.x == 0;
    const bool sysout = flag != nullptr;  // outputs read by the host after the flag
    // Unsplit: the step outputs are assembled in LDS and written out in one burst at the end, so no
    // wave waits for a host store's completion mid-merge (a wave overwriting a register of a pending
    // store waits vmcnt(0), ~1 us for a PCIe write) and the publish waits for one round of them.
    // A column split's tail block assembles its outputs (its tail columns of best, the GRFs, the prediction and the
    // scalars) the same way and bursts only those (C3: its direct host stores cost ~1 us of register-reuse waits).
    float* osh = sh.osh;
    const bool shadow = !split || tailblk;
    auto ostore = [&](void* dst, float v) {
        if (shadow)
            osh[reinterpret_cast<float*>(dst) - reinterpret_cast<float*>(out)] = v;
        else if (sysout)
            __hip_atomic_store(reinterpret_cast<uint32_t*>(dst), __float_as_uint(v), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        else
            *reinterpret_cast<float*>(dst) = v;
    };
    // this block's columns: local index i -> parameter column jc(i)
    const int j0 = split && !tailblk ? ((int)blockIdx.x - 1) * split_cs : 0;
    const int ncol = !split ? P : (tailblk ? mc.ntail : min(split_cs, P - j0));
    auto jc = [&](int i) { return tailblk ? (int)mc.tailc[i] : j0 + i; };
    // parameters this block writes: all (unsplit), the tail columns (tail block), the others (slices)
    auto owns = [&](int jj) { return !split || tailblk || !is_tail_col(mc, jj); };
    const bool do_tail = out && (!split || tailblk);
    const int cols = ncol + 1;
    const int nrec_pad = (nrec + 3) & ~3;
    // the tree levels above the input records (merge_smem_bytes): even levels in lvA / nkA (n1 nodes at most), odd
    // levels in lvB / nkB (n1b), this block's cols columns each
    const int n1 = (nrec + TREE_FAN - 1) / TREE_FAN, n1b = (n1 + TREE_FAN - 1) / TREE_FAN;
    const int lvfA = (n1 * cols + 3) & ~3, lvfB = (n1b * cols + 3) & ~3;
    float* stage = smem;
    float* scale = STAGE ? smem + (size_t)nrec * rec_stride : smem;
    float* lvA = scale + nrec_pad;
    float* lvB = lvA + lvfA;
    uint64_t* nkA = reinterpret_cast<uint64_t*>(lvB + lvfB);  // 8-byte aligned: lvf* and nrec_pad are multiples of 4
    uint64_t* nkB = nkA + n1;
    float* erow = reinterpret_cast<float*>(nkB + n1b);

    // ---- L: loads.  The StepInput fields the output phases need are fetched first, so their latency
    // hides under the record loads instead of stalling the tail.
    const float best_pre = (out && tid < ncol && owns(jc(tid))) ? in->best[jc(tid)] : 0.0f;
    const int qc = tid < 3 ? tid : 2;  // tail lanes 0..3: component of the four-lane layout
    const bool tail_lane = do_tail && tid < 4;
    float tail_pre[13];  // kept in tail_sh across the merge (register pressure: 1024-thread block)
    if (tail_lane) merge_tail_load(in, qc, tail_pre);
    const float state_hi = (do_tail && tid >= 12 && tid < 24) ? in->state[tid] : 0.0f;
    // the predicted state's force-independent part (NMPC:752-784 via CMJ:93-174), formed while the
    // record loads are in flight
    auto tail_prep = [&]() {
        if (tail_lane) {
            if constexpr (ENVT)
                merge_tail_lane(mc, EnvConst{*em}, qc, tail_pre, tail_sh[tid]);
            else
                merge_tail_lane(mc, McConst{mc}, qc, tail_pre, tail_sh[tid]);
        }
    };
    if constexpr (STAGE) {
        constexpr int U = 8;
        const int n4 = (nrec * rec_stride) >> 2;
        const float4* __restrict__ src = reinterpret_cast<const float4*>(recs);
        float4* dst = reinterpret_cast<float4*>(stage);
        auto chunk = [&](int base, bool first) __attribute__((always_inline)) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = base + u * T + tid;
                v[u] = i < n4 ? src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            if (first) {
                tail_prep();
                MERGE_STAMP(7);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = base + u * T + tid;
                if (i < n4) dst[i] = v[u];
            }
        };
        if (prestaged) {
            tail_prep();
        } else {
            chunk(0, true);
            for (int base = U * T; base < n4; base += U * T) chunk(base, false);
        }
        __syncthreads();
        MERGE_STAMP(6);
        recs = stage;
    }
    // ---- 1. beta.  Staged: only the waves holding a record scan and reduce (nrec <= RPT * T, but a
    // step's few hundred records sit in the first waves), and the block minimum is over those waves.
    uint64_t mine = KEY_NONE, kk0 = KEY_NONE;
    float mtag = 0.0f;
    // the top-K's record minima are these headers' keys: kept for it when one chunk holds them all
    // Column split (SplitXchg after the StepInput): the slices fold every column's sums and publish them; the tail
    // block folds none and reads its columns' sums back.  CEM: the tail block computes the top-K once and publishes
    // it; the slices read it back (each slice recomputed both before: C3 merge 15.5 -> 12.8 us).
    const bool hand = SPLITX && split && !rs;  // SPLITX: merge_kernel, the only split launch, passes xg
    const uint32_t ep = hand ? __hip_atomic_load(&xg->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u : 0u;
    // a hand-off word (SplitXchg): polled until it carries this launch's tag, bounded (the tail block reports a
    // timed-out wait as status 1)
    int hand_late = 0;
    auto poll = [&](const uint64_t* w) -> uint32_t {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        uint64_t v;
        while ((uint32_t)((v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != ep) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > XCHG_TIMEOUT_TICKS) {
                hand_late = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        return (uint32_t)v;
    };
    auto tagged = [&](uint32_t x) { return ((uint64_t)ep << 32) | x; };
    const bool topk_here = K > 1 && !rank_out && (!split || tailblk);
    const bool pre_topk = topk_here && nrec <= T;
    const int nhw = STAGE ? (nrec + 63) >> 6 : NW;  // waves that hold a record (staged: <= RPT * NW)
    // the tree's first level rides along (srbd_core.h: 32 consecutive records per node, so a node is a 32-lane half
    // of a wave here): its node keys (nkA) and each record's scale exp(-(m_r - m_node)), formed in this pass
    if (!STAGE || wv < nhw) {
#pragma unroll
        for (int i = 0; i < MERGE_RPT; ++i) {
            if (i * T >= nrec) break;
            const int r = tid + i * T;
            uint64_t kk = KEY_NONE;
            float m_r = 0.0f;
            if (r < nrec) {
                const float* R = recs + (size_t)r * rec_stride;
                m_r = R[0];
                kk = ((uint64_t)f2u(m_r) << 32) | (uint64_t)f2u(R[2]);
                const float tg = R[3];
                mtag = kk < mine ? tg : mtag;
                mine = umin64(mine, kk);
            }
            if (i == 0) kk0 = kk;
            if (!rs) {
                uint64_t nlo, nhi;
                half_wave_min_u64(kk, &nlo, &nhi);
                const uint64_t nk = lane < 32 ? nlo : nhi;
                if (r < nrec) {
                    if ((r & (TREE_FAN - 1)) == 0) nkA[r / TREE_FAN] = nk;
                    scale[r] = expf(-1.0f * (m_r - u2f((uint32_t)(nk >> 32))));
                }
            }
        }
        const uint64_t wmin = wave_min_u64(mine);
        if (lane == 0 && wv < NW) red[wv] = wmin;
    }
    if (pre_topk) {  // block_topk_nodes' entry state
        tk.keys[tid] = kk0;
        if (tid < MAXK) {
            tk.sel[tid] = -1;
            tk.top[tid] = KEY_NONE;
        }
        for (int i = tid; i < K * K; i += T) {
            tk.cand[i] = KEY_NONE;
            tk.cnt[i] = 0;
        }
    }
    MERGE_MARK(0);
    if constexpr (!STAGE)
        if (!(SPLITX && hand && tailblk)) tail_prep();  // a hand-off tail block: after its top-K (off its critical path)
    MERGE_MARK(1);
    __syncthreads();
    MERGE_MARK(2);
    uint64_t bkey = red[0];
    for (int i = 1; i < (STAGE ? (nhw < NW ? nhw : NW) : NW); ++i) bkey = umin64(bkey, red[i]);
    const float beta = u2f((uint32_t)(bkey >> 32));
    if (mine == bkey && mine != KEY_NONE) tag_sh = mtag;  // keys are unique: one writer
    MERGE_STAMP(1);

    // ---- 2./3. the reduction tree's sums (srbd_core.h): the input records folded level by level, TREE_FAN
    // consecutive children per node in order (the fold of fold_node_lds, srbd_device.h), to the root -- or, for a
    // rank record (rank_out), `levels_up` levels, up to this rank's nodes of the exchange level.  Every block of a
    // column split folds its own columns; all recompute the node keys the same way.
    auto off_of = [&](int jj) { return jj < ncol ? REC_HDR + jc(jj) : 1; };
    int nlev = nrec;            // nodes of the current level
    bool lev_recs = true;       // the current level is the input records
    const float* lvp = nullptr;  // values of the current level (lev_recs: the records)
    const uint64_t* nkp = nullptr;
    if (!rs && !(hand && tailblk)) {
        float* lv_out = lvA;
        uint64_t* nk_out = nkA;
        for (int L = 0; rank_out ? L < levels_up : nlev > 1; ++L) {
            const int n2 = (nlev + TREE_FAN - 1) / TREE_FAN;
            // level 0's keys and scales came with the beta pass; above it, one wave per node, lane = child
            for (int g2 = wv; L > 0 && g2 < n2; g2 += NW) {
                const int c = TREE_FAN * g2 + lane;
                const bool have = lane < TREE_FAN && c < nlev;
                const uint64_t kc = !have ? KEY_NONE
                                          : lev_recs ? ((uint64_t)f2u(recs[(size_t)c * rec_stride]) << 32) |
                                                           (uint64_t)f2u(recs[(size_t)c * rec_stride + 2])
                                                     : nkp[c];
                const uint64_t k = wave_min_u64(kc);
                if (lane == 0) nk_out[g2] = k;
                if (have) scale[c] = expf(-1.0f * (u2f((uint32_t)(kc >> 32)) - u2f((uint32_t)(k >> 32))));
            }
            if (L > 0) __syncthreads();
            if (L == 1) MERGE_MARK(6);
            for (int q = tid; q < n2 * cols; q += T) {  // (node, column) sums, child by child
                const int g2 = (int)((uint32_t)q / (uint32_t)cols), jq = (int)((uint32_t)q % (uint32_t)cols);
                const int c0 = TREE_FAN * g2, nc = min(TREE_FAN, nlev - c0);
                const float* src = lev_recs ? recs + (size_t)c0 * rec_stride + off_of(jq) : lvp + (size_t)c0 * cols + jq;
                const int sstride = lev_recs ? rec_stride : cols;
                float a = 0.0f;
                int cb = 0;
                for (; cb + 8 <= nc; cb += 8) {  // 8 children's loads in flight, then their adds in order
                    float x[8], sc[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        x[u] = src[(size_t)(cb + u) * sstride];
                        sc[u] = scale[c0 + cb + u];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) a = a + sc[u] * x[u];
                }
                for (; cb < nc; ++cb) a = a + scale[c0 + cb] * src[(size_t)cb * sstride];
                lv_out[(size_t)g2 * cols + jq] = a;
            }
            __syncthreads();
            if (L == 0) MERGE_MARK(4);
            if (L == 1) MERGE_MARK(7);
            lvp = lv_out;
            nkp = nk_out;
            lev_recs = false;
            nlev = n2;
            lv_out = lv_out == lvA ? lvB : lvA;
            nk_out = nk_out == nkA ? nkB : nkA;
        }
        MERGE_MARK(5);
        if (!rank_out)  // the root
            for (int jj = tid; jj < cols; jj += T) Vs[jj] = lev_recs ? recs[off_of(jj)] : lvp[jj];
    }
    if (SPLITX && hand && !tailblk) {  // a slice publishes its columns' sums (block 1 also the weights' sum)
        __syncthreads();
        // srbd_debug_split_drop (tests): block 1 withholds the weights' sum, so the tail block's wait times out
        const bool drop = blockIdx.x == 1 && __hip_atomic_load(&xg->drop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int i = tid; i <= ncol; i += T)
            if (i < ncol || (blockIdx.x == 1 && !drop))
                __hip_atomic_store(&xg->sums[i < ncol ? jc(i) : P], tagged(f2u(Vs[i])), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
    MERGE_STAMP(2);

    if (rank_out) {  // ---- a rank record: this rank's nodes of the exchange level (unsplit: column i == i)
        const int rstride = rec_floats_rank(P, K);
        int span = 1;
        for (int L = 0; L < levels_up; ++L) span *= TREE_FAN;
        const bool zs = zs_scaled(mc, in);
        const int nout = (nrec + span - 1) / span;  // == nlev after the folds (random sampling folds no sums)
        for (int g = 0; g < nout; ++g) {
            const int r0 = g * span, r1 = min(r0 + span, nrec);
            float* R = rank_out + (size_t)g * rstride;
            // the node's key (its records' minimum) and the tag of the record holding it
            uint64_t km = KEY_NONE;
            for (int r = r0 + tid; r < r1; r += T)
                km = umin64(km, ((uint64_t)f2u(recs[(size_t)r * rec_stride]) << 32) | f2u(recs[(size_t)r * rec_stride + 2]));
            km = wave_min_u64(km);
            __syncthreads();
            if (lane == 0) red[wv] = km;
            __syncthreads();
            uint64_t nk = red[0];
            for (int i = 1; i < NW; ++i) nk = umin64(nk, red[i]);
            for (int r = r0 + tid; r < r1; r += T)
                if ((((uint64_t)f2u(recs[(size_t)r * rec_stride]) << 32) | f2u(recs[(size_t)r * rec_stride + 2])) == nk)
                    tag_sh = recs[(size_t)r * rec_stride + 3];
            if (K == 1) {
                if (tid == 0) elite[0] = nk;
            } else {
                block_topk_rank<NT>(recs + (size_t)r0 * rec_stride, r1 - r0, rec_stride, P, K, elite, tk);
            }
            __syncthreads();
            for (int jj = tid; jj < P; jj += T)
                R[REC_HDR + jj] = rs ? 0.0f : (lev_recs ? recs[(size_t)g * rec_stride + REC_HDR + jj] : lvp[(size_t)g * cols + jj]);
            for (int e = tid; e < K; e += T) {
                R[REC_HDR + P + 2 * e] = u2f((uint32_t)elite[e]);
                R[REC_HDR + P + 2 * e + 1] = u2f((uint32_t)(elite[e] >> 32));
            }
            const bool rows = rs || cem;  // the rows the root needs: random sampling's best, CEM's elite
            for (int t = tid; t < K * P; t += T) {
                const int e = t / P, jj = t % P;
                float v = 0.0f;
                if (rows && elite[e] != KEY_NONE) {
                    v = noise[(size_t)jj * mc.ldn + ((int)(uint32_t)elite[e] - mc.row0)];
                    if (zs) v = v * in->sigma[jj];
                }
                R[REC_HDR + P + 2 * K + t] = v;
            }
            if (tid == 0) {
                R[0] = u2f((uint32_t)(nk >> 32));
                R[1] = rs ? 1.0f : (lev_recs ? recs[(size_t)g * rec_stride + 1] : lvp[(size_t)g * cols + P]);
                R[2] = u2f((uint32_t)nk);
                R[3] = tag_sh;
            }
            __syncthreads();
        }
        return;
    }

    // ---- 4. top-K keys (ascending; keys are unique).  The tail block of a CEM split never reads
    // elite rows (sigma belongs to the slices), so it skips them.
    const bool want_elite = !tailblk || rs;
    if (K == 1) {
        if (tid == 0) elite[0] = bkey;
    } else if (SPLITX && !topk_here) {  // a CEM slice: the tail block's keys (halves: little-endian words)
        if (tid < 2 * K) reinterpret_cast<uint32_t*>(elite)[tid] = poll(&xg->elite[tid]);
    } else {
        if (pre_topk)
            block_topk_nodes<NT>(recs, nrec, rec_stride, P, K, nkA, elite, tk, dbg);
        else
            block_topk_rank<NT>(recs, nrec, rec_stride, P, K, elite, tk);
        if (SPLITX && split) {  // the tail block publishes them
            __syncthreads();
            if (tid < 2 * K)
                __hip_atomic_store(&xg->elite[tid], tagged(reinterpret_cast<const uint32_t*>(elite)[tid]),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (SPLITX && hand && tailblk) {  // the tail block's sums: the slices'
        if constexpr (!STAGE) tail_prep();
        for (int i = tid; i <= ncol; i += T) Vs[i] = u2f(poll(&xg->sums[i < ncol ? jc(i) : P]));
        // any thread's timed-out word fails the step (status bit 1; the host then resets SplitXchg)
        hand_late = __syncthreads_or(hand_late);
        // every slice has stored its sums, so every slice has read the epoch: advance it for the next launch.  Not
        // after a timeout: a slice may not have read it yet (it would tag its late sums with the next launch's epoch)
        if (tid == 0 && !hand_late) __hip_atomic_store(&xg->epoch, ep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (SPLITX && hand && !tailblk && !topk_here && K > 1) hand_late = __syncthreads_or(hand_late);  // elite keys
    __syncthreads();
    // record slot of every elite key (needed when rows travel inside the records)
    const bool need_rows = want_elite && (rs || cem);  // MPPI's update is the weighted sum alone
    if (rows_in_rec && need_rows) {
        for (int t = tid; t < nrec * K; t += T) {
            const int r = t / K, q = t % K;
            const uint64_t x = rec_key(recs + (size_t)r * rec_stride, P, q);
            for (int e = 0; e < K; ++e)
                if (x == elite[e] && x != KEY_NONE) elite_src[e] = t;
        }
        __syncthreads();
    }
    MERGE_STAMP(3);

    // ---- 5. elite rows (this block's columns) -> LDS
    int Kv = 0;
    for (int e = 0; e < K; ++e) Kv += elite[e] != KEY_NONE;
    const bool zs = zs_scaled(mc, in);
    for (int t = tid; need_rows && t < K * ncol; t += T) {
        const int e = t / ncol, i = t % ncol, jj = jc(i);
        float v = 0.0f;
        if (elite[e] != KEY_NONE) {
            if (rows_in_rec) {
                const int st = elite_src[e];
                v = recs[(size_t)(st / K) * rec_stride + REC_HDR + P + 2 * K + (size_t)(st % K) * P + jj];
            } else {
                v = noise[(size_t)jj * mc.ldn + ((int)(uint32_t)elite[e] - mc.row0)];
                if (zs) v = v * in->sigma[jj];
            }
        }
        erow[t] = v;
    }
    __syncthreads();

    // ---- 6. outputs
    if (out) {
        for (int i = tid; i < ncol; i += T) {
            const int jj = jc(i);
            if (owns(jj)) {
                const float b0 = i == tid ? best_pre : in->best[jj];
                const float v = rs ? b0 + erow[i] : b0 + Vs[i] / Vs[ncol];
                nb[jj] = v;
                ostore(&out->best[jj], v);
            }
            if (cem && !tailblk) {  // NMPC:1075-1081
                float s = 0.0f;
                for (int e = 0; e < Kv; ++e) s = s + erow[e * ncol + i];
                const float mean = s / (float)Kv;
                float var = 0.0f;
                for (int e = 0; e < Kv; ++e) {
                    const float d = erow[e * ncol + i] - mean;
                    var = var + d * d;
                }
                var = var / (float)(Kv - 1);
                float sg = sqrtf(var + 1e-8f);
                sg = sg > 5.0f ? 5.0f : sg;
                sg = sg < 0.2f ? 0.2f : sg;
                ostore(&out->sigma[jj], sg);
                if (chain) in->sigma[jj] = sg;
            }
        }
        __syncthreads();
        MERGE_STAMP(4);
        if (tail_lane) {
            float ts[40];  // one batch of LDS reads
#pragma unroll
            for (int i = 0; i < 40; ++i) ts[i] = tail_sh[tid][i];
            const int c = qc;
            float f[4], p, v, r, w;
            merge_tail_grf(c, ts, nb, f, p, v, r, w);
            if (tid < 3) {
#pragma unroll
                for (int l = 0; l < 4; ++l) ostore(&out->grf[3 * l + c], f[l]);
                ostore(&out->pred[c], p);
                ostore(&out->pred[3 + c], v);
                ostore(&out->pred[6 + c], r);
                ostore(&out->pred[9 + c], w);
            }
        }
        if (do_tail && tid >= 12 && tid < 24) ostore(&out->pred[tid], state_hi);
        if (do_tail && tid == 0) {
            ostore(&out->best_cost, beta);
            ostore(&out->best_index, __uint_as_float((uint32_t)bkey));
            ostore(&out->best_freq, tag_sh);
            // a column split: the host zeroes status before the launch, and a late block ORs its bit in (below)
            if (!split) ostore(&out->status, __int_as_float(0));
            // chain: the next draws come from the device RNG.  (Split: slices read noise_scaled too, but a
            // chain's steps all run with it 0 already -- reset_noise_scaled -- so this store never changes it.)
            if (chain) in->noise_scaled = 0;
            if (chain && ctr_inc) advance_key(mc, in, ctr_inc);
        }
        if (chain)
            for (int i = tid; i < ncol; i += T) {
                const int jj = jc(i);
                if (owns(jj)) in->best[jj] = nb[jj];
            }
    }
    if (out && shadow) {  // the burst: best[P] | sigma[P] (CEM) | grf, pred, scalars
        __syncthreads();
        constexpr int TAILF = (int)((sizeof(StepOutput) - offsetof(StepOutput, grf)) / sizeof(float));
        constexpr int TAIL0 = (int)(offsetof(StepOutput, grf) / sizeof(float));
        constexpr int SIG0 = (int)(offsetof(StepOutput, sigma) / sizeof(float));
        constexpr int STAT = (int)(offsetof(StepOutput, status) / sizeof(float));
        // unsplit: the whole StepOutput; a split's tail block: its columns of best, then grf .. the scalars except
        // status (the host zeroed it; a late block ORs its bit in)
        const int nb0 = split ? ncol : P;
        const int nsig = cem && !split ? P : 0;
        float* o = reinterpret_cast<float*>(out);
        for (int t = tid; t < nb0 + nsig + TAILF; t += T) {
            const int k = t < nb0 ? (split ? jc(t) : t) : (t < nb0 + nsig ? SIG0 + (t - nb0) : TAIL0 + (t - nb0 - nsig));
            if (split && k == STAT) continue;
            if (sysout)
                __hip_atomic_store(reinterpret_cast<uint32_t*>(o + k), __float_as_uint(osh[k]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            else
                o[k] = osh[k];
        }
    }
    MERGE_STAMP(5);
    MERGE_MARK(8);
    if (dbg && threadIdx.x == 0 && sblk < 2) dbg[32 * sblk + 9] = __builtin_amdgcn_s_memtime();
#undef MERGE_STAMP
#undef MERGE_MARK
    // a hand-off word of the column split never arrived (bounded poll): tail block bit 1, a slice bit 2
    if (SPLITX && hand && hand_late && tid == 0 && out)
        __hip_atomic_fetch_or(reinterpret_cast<uint32_t*>(&out->status), tailblk ? 1u : 2u, __ATOMIC_RELAXED,
                              sysout ? __HIP_MEMORY_SCOPE_SYSTEM : __HIP_MEMORY_SCOPE_AGENT);
    if (flag) {  // every thread's output writes have completed before thread 0 publishes `seq`
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            if (fence_sys) {
                __threadfence_system();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __hip_atomic_store(flag + (split ? blockIdx.x : 0), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// LDS staging of the records (merge_body<true>): when the block's records fit beside the merge's own
// dynamic LDS.  The publish flag follows the system-scope output stores without a system fence (the
// stores are write-through to the host; every wave waits vmcnt(0) first, merge_body).
constexpr size_t MERGE_LDS_DYN_MAX = 140 * 1024;  // + the staged merge's static LDS (block_topk_rank) <= 160 KB
// the exchange kernel's static LDS holds both passes' merge_body arrays: its dynamic limit is this much lower
constexpr size_t XCHG_LDS_STATIC = 24 * 1024;
static bool merge_stage_fits(int nrec_block, int rec_stride, int P, int K, size_t* smem) {
    const size_t base = merge_smem_bytes(nrec_block, P, K);
    const size_t st = sizeof(float) * (size_t)nrec_block * rec_stride;
    if ((rec_stride & 3) == 0 && base + st <= MERGE_LDS_DYN_MAX &&
        nrec_block <= MERGE_RPT * MERGE_STAGE_THREADS) {
        *smem = base + st;
        return true;
    }
    *smem = base;
    return false;
}

}  // namespace srbd
