// srbd_api_internal.h -- what the two C-ABI files share: srbd_api.hip (the single context, which defines everything
// declared here) and srbd_api_batch.hip (the batched environments; an srbd_batch holds an srbd_ctx).  Only what the
// batch file calls is declared; the rest of the context's helpers stay static in srbd_api.hip.
#pragma once
#include <chrono>
#include <rccl/rccl.h>  // types only: RCCL is dlopen'ed (the caller's copy, e.g. torch's)

#include "srbd_launch.h"

struct srbd_ctx {
    srbd_config cfg;
    srbd::ModelConst mc;
    // rollout blocks, leaf records per block (the reduction tree's leaves, srbd_core.h) and this rank's leaves;
    // wrec_stride: floats per leaf / level-1 record; rrec_stride: floats of one rank buffer (its exchange-level
    // node records, t_xmax of them)
    int mode = 0, threads = 64, nblocks = 0, lpb = 1, nleaf = 0, wrec_stride = 0, rrec_stride = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    srbd::StepInput* d_in = nullptr;
    srbd::StepInput* h_in = nullptr;
    srbd::StepInput* d_in_host = nullptr;  // device alias of the mapped pinned h_in (upload_input)
    srbd::StepOutput* d_out = nullptr;
    // Host-driven steps: the merge writes StepOutput straight into mapped pinned host memory (h_out,
    // device alias d_out_host) and then publishes a sequence number in h_flag; the host spins on it.
    // (Measured on MI355X: launch + spin on a mapped flag 5.8 us vs launch + hipStreamSynchronize 11.3;
    // a 2-kernel graph + sync 19.4: hipGraphs cost more than they save at this size.)
    srbd::StepOutput* h_out = nullptr;
    srbd::StepOutput* d_out_host = nullptr;
    uint32_t* h_flag = nullptr;
    uint32_t* d_flag = nullptr;
    uint32_t seq = 0;
    // Sharded transport owned by the library: an RCCL communicator (srbd_comm_init) and the rank
    // record / gathered records it exchanges with ncclAllGather on the context stream.
    ncclComm_t comm = nullptr;
    int comm_world = 0;
    float* d_myrec = nullptr;
    float* d_gath = nullptr;
    // xGMI exchange (merge_xchg_kernel): this rank's mailbox (uncached device memory, IPC-exported),
    // the peer table handed to the kernel, a device word pair {error, epoch counter}, the cached stage
    // the second merge pass reads, and the two-step / one-step graphs of the device-resident chain.
    float* xg_base = nullptr;
    std::vector<void*> xg_opened;
    srbd::XchgArgs xa{};
    srbd::XchgArgs* d_xa = nullptr;  // device copy (the rollout launch's in-launch exchange, GroupArgs::xa)
    int xg_world = 0;
    int* xg_err = nullptr;
    float* xg_stage = nullptr;
    hipGraphExec_t g_xg2 = nullptr, g_xg1 = nullptr;
    // Noise matrices, double buffered: the rollout launch of a step reading d_noise[cur] also draws the
    // predicted next step's noise (counter + 1) into the other buffer (MPPI / random sampling; CEM's
    // draws depend on the sigma the step produces).
    float* d_noise[2] = {nullptr, nullptr};
    int cur = 0;
    bool pref_valid = false;
    int pref_buf = 0;
    uint64_t pref_seed = 0, pref_ctr = 0;
    bool chain_started = false;  // sharded device-resident chain
    float* d_noise_rm = nullptr;
    size_t noise_rm_cap = 0;
    float* d_costs = nullptr;
    float* d_wrec = nullptr;
    // in-launch level-1 fold of the leaf records (GroupArgs): gsize = TREE_FAN leaves per node, ngroups
    // level-1 records the merge reads; gsize 1: the merge reads the nleaf leaf records
    int gsize = 1, ngroups = 0;
    float* d_grec = nullptr;
    uint32_t* d_gcnt = nullptr;
    // in-launch final merge (final_merge_ok): the rollout's last group writes the host step's outputs
    bool final_merge = false;
    uint32_t* d_gdone = nullptr;
    // fast_tail (fast_tail_ok, SRBD_FAST_TAIL=0 turns it off): the node records the folders hand over, tagged words
    bool fast_tail = false;
    bool gen_env = true;  // SRBD_GEN != "0" at create (gen_now)
    // quads the epilogue regenerates (SRBD_GEN_RG at create), the rest stored and read
    int gen_rg = srbd::GEN_REGEN_QUADS;
    int gen_quad_min = 0;  // four-lane form: rows from which the launch makes its draws (gen_now); 0 off
    uint64_t* d_gtag = nullptr;
    // its host-step outputs as tagged words (GroupArgs::outt, tagged_outputs), host-mapped
    uint64_t* h_outt = nullptr;
    uint64_t* d_outt = nullptr;
    // host steps pass the step input to the rollout as a kernel argument (ks_ok): no upload kernel
    bool ks = false;
    hipGraphExec_t g_dev2 = nullptr, g_dev1 = nullptr;
    float* d_ga_freq = nullptr;  // injected per-row step frequencies (gait-adaptive parity mode), ldn floats
    float* d_plan = nullptr;     // srbd_plan: its device copies of the caller's arrays, allocated at the first call
    bool input_ready = false;
    // Armed host steps (srbd_set_armed): during a step the next one's copy, rollout and merge are queued
    // behind it, the copy kernel spinning on the host-mapped word h_go; the next srbd_step writes its
    // input and stores the go word instead of launching.  The armed run writes its costs into
    // d_costs_arm (swapped in when it fires), so a cancelled run (which recomputes the previous input)
    // leaves every buffer a later call reads unchanged.
    int arm_mode = 0;
    uint64_t arm_deadline_us = 50000;
    uint32_t* h_go = nullptr;
    uint32_t* d_go = nullptr;
    uint32_t* d_fired = nullptr;  // arm_copy_kernel's verdict for the chain behind it (Publish::gate)
    int64_t arm_refired = 0;      // claimed chains whose copy had already given up: re-run unarmed
    uint32_t arm_test_delay_us = 0;  // srbd_debug_arm_delay: host sleep between claim and go (tests only)
    float* d_costs_arm = nullptr;
    bool armed = false;
    uint32_t arm_seq = 0;
    int arm_buf = 0, arm_nflags = 1;
    bool arm_fused = true;  // the chain's draws were made ahead (fused); else its RNG kernel draws them
    uint64_t arm_seed = 0, arm_ctr = 0;
    std::chrono::steady_clock::time_point arm_t0;
    int64_t arm_served = 0, arm_cancelled = 0;
    int64_t foothold_chained = 0;  // srbd_foothold_mpc_step calls run chained (srbd_foothold_chain)
    std::string err;
};

#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                        \
            return SRBD_E_HIP;                                                                      \
        }                                                                                           \
    } while (0)

// Hidden: not exported, and srbd_step's calls of fill_input and wait_published bind directly, as to static functions
namespace srbd __attribute__((visibility("hidden"))) {
int fail(srbd_ctx* c, int code, const std::string& m);  // m: c's error text, or the calling thread's (c NULL)
const char* last_error_global();                        // that text: srbd_last_error(NULL), srbd_batch_last_error(NULL)
srbd_env_params env_params_of(const srbd_config* cfg);
int build_model(const srbd_config* cfg, ModelConst* mc, std::string* why);
int fill_input(const srbd_config* cfg, const ModelConst& mc, StepInput* in, const float* state, const float* ref,
               const float* contact, int stride, const float* best, const float* sigma, uint64_t seed,
               uint64_t counter, const EnvModel* em = nullptr);
void ga_chunk_bounds(const ModelConst& mc, int32_t* cb /* GA_MAXCB */);
void fill_gait(const ModelConst& mc, StepInput* in, const float* timing, float pgg_dt, float duty_factor,
               const float* freq_set, int n_freq, bool explicit_rows);
int wait_published(srbd_ctx* c, uint32_t seq, int nflags = 1, int* cancelled = nullptr);
}  // namespace srbd
