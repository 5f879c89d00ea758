// srbd_api_batch.hip -- C-ABI of libsrbd_hip.so, the batched environments (srbd_batch_*, include/srbd_mpc.h): struct
// srbd_batch, its host and device-resident steps, its gait, cost-term and per-environment parameter setters and the
// controller-interface step.  The kernels are srbd_batch.hip's and srbd_producers.hip's (srbd_launch.h).  From the
// single context (srbd_api.hip) it takes the context structure, fail, HIP_TRY and six helpers, declared in
// srbd_api_internal.h; nothing here is called from there.
// E independent problems of one configuration behind one host call: per step one input copy, one draw (or
// transpose) launch, one rollout launch and one merge launch over all environments (srbd_batch.hip), and one host
// wait on one published word.  The single context's fields the batch shares -- configuration, ModelConst, stream,
// publish word, sequence number, error text -- live in `c`, so fill_input and wait_published serve both.
#include <math.h>
#include <string.h>

#include "srbd_api_internal.h"

using namespace srbd;

struct srbd_batch {
    srbd_ctx c;
    int E = 0;
    StepInput* h_in = nullptr;       // E, mapped pinned staging
    StepInput* d_in_host = nullptr;  // its device alias
    StepInput* d_in = nullptr;       // E
    StepOutput* h_out = nullptr;     // E, mapped pinned: the merge blocks write them
    StepOutput* d_out_host = nullptr;
    float* d_noise = nullptr;        // E x P x ldn
    float* d_costs = nullptr;        // E x ldn
    float* d_rec = nullptr;          // E x nleaf leaf records
    uint32_t* d_eflag = nullptr;     // E (merge_body's own publish word per block)
    uint32_t* d_count = nullptr;     // the merge blocks' arrival count, zero between steps
    float* d_noise_rm = nullptr;     // injected noise as given (row-major), E x N x P
    float* d_ga_freq = nullptr;      // injected per-row step frequencies (srbd_batch_set_gait), E x ldn, padding zero
    bool stepped = false;
    // the device-resident step (srbd_batch_step_device): the merge blocks' records in device memory, the event recorded
    // behind each device step's last launch, and the stream of the last one while no entry point has joined it
    StepOutput* d_out = nullptr;     // E
    hipEvent_t dev_done = nullptr;
    hipStream_t dev_stream = nullptr;
    bool dev_pending = false;
    // srbd_batch_set_gait_device wrote d_in's gait fields past the staging: the host step, which copies the staging
    // over them, is refused until srbd_batch_set_gait or srbd_batch_clear_gait
    bool ga_staging_stale = false;
    // per-environment robot and cost parameters (srbd_batch_set_env_params): the fields as set and the records derived
    // from them, on the device (what the ENVT kernels and the getter read) and mirrored on the host (what the host
    // step's fill_input and the host setter read).  Both hold the configuration's values until a setter changes them.
    // env_on: the steps run the ENVT kernels; env_host_stale: the device setter wrote past the mirrors, the next host
    // call that needs them downloads them.
    srbd_env_params* d_env_raw = nullptr;  // E
    EnvModel* d_env = nullptr;             // E
    std::vector<srbd_env_params> h_env_raw;
    std::vector<EnvModel> h_env;
    bool env_on = false;
    bool env_host_stale = false;
    // srbd_batch_interface_step_device: the step keys its prologue writes and its iterations' steps read,
    // SRBD_MAX_IFACE_ITERS rows of 2 E words (row i: E seeds, then E counters)
    uint64_t* d_iface_keys = nullptr;
    // srbd_batch_plan (the host form): its device copies of the caller's arrays, allocated at the first call
    float* d_plan = nullptr;
};

// The internal buffers (d_in, d_noise, d_rec, d_costs, d_count, d_ga_freq) are shared by the host path and the device
// steps, which run on the caller's stream.  The host: wait for the last device step.
static hipError_t batch_join_host(srbd_batch* b) {
    if (!b->dev_pending) return hipSuccess;
    const hipError_t e = hipEventSynchronize(b->dev_done);
    if (e == hipSuccess) b->dev_pending = false;
    return e;
}

// A host setter before it touches the shared buffers: no device call and no step in flight reads them
static int batch_quiesce(srbd_batch* b) {
    srbd_ctx* c = &b->c;
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    HIP_TRY(c, batch_join_host(b));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRBD_OK;
}

// The stream and event protocol: every device entry point brackets what it enqueues with this pair.  Begin: NULL is
// the batch's own stream, so the null stream goes by its explicit handle (handed on as the null stream); the previous
// device call on another stream still owns the internal buffers, so this one's stream waits on its event.
static int batch_dev_begin(srbd_batch* b, void* hip_stream, hipStream_t* stream) {
    srbd_ctx* c = &b->c;
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    hipStream_t s = (hipStream_t)hip_stream;
    if (!s) s = c->stream;
    else if (s == hipStreamLegacy) s = nullptr;
    if (b->dev_pending && b->dev_stream != s) HIP_TRY(c, hipStreamWaitEvent(s, b->dev_done, 0));
    *stream = s;
    return SRBD_OK;
}
// End, behind the call's last launch: the event is recorded whatever the launches returned (what was enqueued still
// orders the other entry points), then the launch error is reported before the record's.
static int batch_dev_end(srbd_batch* b, hipStream_t s) {
    const hipError_t le = hipGetLastError();
    const hipError_t re = hipEventRecord(b->dev_done, s);
    b->dev_stream = s;
    b->dev_pending = re == hipSuccess;
    HIP_TRY(&b->c, le);
    HIP_TRY(&b->c, re);
    return SRBD_OK;
}

// The pointers an io structure requires, by name: the first NULL one's name, or NULL
struct batch_req {
    const void* p;
    const char* name;
};
template <size_t N>
static const char* batch_first_null(const batch_req (&req)[N]) {
    for (const batch_req& r : req)
        if (!r.p) return r.name;
    return nullptr;
}

// Every environment's parameters back to the configuration's, mirrors and device arrays (the stream is idle)
static hipError_t batch_env_reset(srbd_batch* b) {
    const srbd_env_params p = env_params_of(&b->c.cfg);
    EnvModel m;
    env_model_fill(p, &m);
    b->h_env_raw.assign((size_t)b->E, p);
    b->h_env.assign((size_t)b->E, m);
    b->env_on = false;
    b->env_host_stale = false;
    hipError_t e = hipMemcpy(b->d_env_raw, b->h_env_raw.data(), sizeof(srbd_env_params) * (size_t)b->E,
                             hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(b->d_env, b->h_env.data(), sizeof(EnvModel) * (size_t)b->E, hipMemcpyHostToDevice);
    return e;
}
// The mirrors after srbd_batch_set_env_params_device (no device work of the batch is in flight)
static hipError_t batch_env_download(srbd_batch* b) {
    if (!b->env_host_stale) return hipSuccess;
    hipError_t e = hipMemcpy(b->h_env_raw.data(), b->d_env_raw, sizeof(srbd_env_params) * (size_t)b->E,
                             hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(b->h_env.data(), b->d_env, sizeof(EnvModel) * (size_t)b->E, hipMemcpyDeviceToHost);
    if (e == hipSuccess) b->env_host_stale = false;
    return e;
}

extern "C" void srbd_batch_destroy(srbd_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->c.cfg.device_id);
    (void)batch_join_host(b);
    if (b->c.stream) (void)hipStreamSynchronize(b->c.stream);
    if (b->dev_done) (void)hipEventDestroy(b->dev_done);
    (void)hipFree(b->d_out);
    (void)hipFree(b->d_in);
    (void)hipFree(b->d_noise);
    (void)hipFree(b->d_costs);
    (void)hipFree(b->d_rec);
    (void)hipFree(b->d_eflag);
    (void)hipFree(b->d_count);
    (void)hipFree(b->d_noise_rm);
    (void)hipFree(b->d_ga_freq);
    (void)hipFree(b->d_env_raw);
    (void)hipFree(b->d_env);
    (void)hipFree(b->d_iface_keys);
    (void)hipFree(b->d_plan);
    if (b->h_in) (void)hipHostFree(b->h_in);
    if (b->h_out) (void)hipHostFree(b->h_out);
    if (b->c.h_flag) (void)hipHostFree(b->c.h_flag);
    if (b->c.stream) (void)hipStreamDestroy(b->c.stream);
    delete b;
}

extern "C" const char* srbd_batch_last_error(const srbd_batch* b) {
    return b ? b->c.err.c_str() : last_error_global();
}

extern "C" int srbd_batch_num_envs(const srbd_batch* b) { return b ? b->E : SRBD_E_INVALID; }

// cem: srbd_batch_create_cem (CEM-MPPI and nothing else); else srbd_batch_create (everything but CEM-MPPI)
static int batch_create(const srbd_config* cfg, int32_t num_envs, srbd_batch** out, bool cem) {
    if (!cfg || !out) return fail(nullptr, SRBD_E_INVALID, "null argument");
    *out = nullptr;
    if (num_envs < 1 || num_envs > BATCH_MAX_ENVS)
        return fail(nullptr, SRBD_E_INVALID, "num_envs must be in [1, " + std::to_string(BATCH_MAX_ENVS) + "]");
    if (cfg->num_samples > BATCH_MAX_SAMPLES)
        return fail(nullptr, SRBD_E_INVALID,
                    "num_samples per environment must be <= " + std::to_string(BATCH_MAX_SAMPLES) +
                        " (256 leaves, what one merge block folds): beyond that one environment fills the GPU, use "
                        "separate contexts");
    if (!cem && cfg->method == SRBD_CEM_MPPI)
        return fail(nullptr, SRBD_E_INVALID,
                    "srbd_batch_create does not take CEM-MPPI (sigma is part of every step): create the batch with "
                    "srbd_batch_create_cem and step it with srbd_batch_step_cem / srbd_batch_step_cem_device");
    if (cem && cfg->method != SRBD_CEM_MPPI)
        return fail(nullptr, SRBD_E_INVALID,
                    "srbd_batch_create_cem takes method SRBD_CEM_MPPI only: MPPI and random sampling go through "
                    "srbd_batch_create");
    if ((cfg->world_size > 1) || cfg->rank != 0)
        return fail(nullptr, SRBD_E_INVALID, "a batch is unsharded: rank / world_size must be 0 / 1");
    ModelConst mc;
    std::string why;
    int rc = build_model(cfg, &mc, &why);
    if (rc) return fail(nullptr, rc, why);
    if ((long long)mc.P * mc.ldn * 4 >= (1LL << 31))  // the rollout's per-environment buffer descriptor
        return fail(nullptr, SRBD_E_INVALID, "noise matrix of one environment exceeds 2^31 bytes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, SRBD_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, SRBD_E_NODEVICE, "bad device_id");
    srbd_batch* b = new srbd_batch();
    b->c.cfg = *cfg;
    b->c.cfg.world_size = 1;
    b->c.mc = mc;
    b->c.nleaf = mc.nleaf;
    b->c.wrec_stride = rec_floats_wave(mc.P, mc.K);
    b->E = num_envs;
    const size_t E = (size_t)num_envs;
    auto cleanup_fail = [&](const char* what, hipError_t e) {
        std::string m = std::string(what) + ": " + hipGetErrorString(e);
        srbd_batch_destroy(b);
        return fail(nullptr, e == hipErrorOutOfMemory ? SRBD_E_NOMEM : SRBD_E_HIP, m);
    };
    hipError_t e;
    if ((e = hipSetDevice(cfg->device_id)) != hipSuccess) return cleanup_fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&b->c.stream, hipStreamNonBlocking)) != hipSuccess)
        return cleanup_fail("hipStreamCreate", e);
    batch_prepare();
    if ((e = hipHostMalloc((void**)&b->h_in, sizeof(StepInput) * E, hipHostMallocMapped)) != hipSuccess)
        return cleanup_fail("hipHostMalloc", e);
    if ((e = hipHostGetDevicePointer((void**)&b->d_in_host, b->h_in, 0)) != hipSuccess)
        return cleanup_fail("hipHostGetDevicePointer", e);
    if ((e = hipHostMalloc((void**)&b->h_out, sizeof(StepOutput) * E, hipHostMallocMapped | hipHostMallocCoherent)) !=
        hipSuccess)
        return cleanup_fail("hipHostMalloc", e);
    if ((e = hipHostGetDevicePointer((void**)&b->d_out_host, b->h_out, 0)) != hipSuccess)
        return cleanup_fail("hipHostGetDevicePointer", e);
    if ((e = hipHostMalloc((void**)&b->c.h_flag, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent)) !=
        hipSuccess)
        return cleanup_fail("hipHostMalloc", e);
    if ((e = hipHostGetDevicePointer((void**)&b->c.d_flag, b->c.h_flag, 0)) != hipSuccess)
        return cleanup_fail("hipHostGetDevicePointer", e);
    __atomic_store_n(b->c.h_flag, 0u, __ATOMIC_RELEASE);
    memset(b->h_in, 0, sizeof(StepInput) * E);
    memset(b->h_out, 0, sizeof(StepOutput) * E);
    // sizes in 64 bits: E x P x ldn floats passes 2^32 bytes long before the limits
    const size_t noise_bytes = sizeof(float) * E * (size_t)mc.P * (size_t)mc.ldn;
    const size_t rec_bytes = sizeof(float) * E * (size_t)mc.nleaf * (size_t)b->c.wrec_stride;
    if ((e = hipMalloc((void**)&b->d_in, sizeof(StepInput) * E)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_noise, noise_bytes)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_costs, sizeof(float) * E * (size_t)mc.ldn)) != hipSuccess)
        return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_rec, rec_bytes)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_eflag, sizeof(uint32_t) * E)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_count, sizeof(uint32_t))) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_out, sizeof(StepOutput) * E)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = hipEventCreateWithFlags(&b->dev_done, hipEventDisableTiming)) != hipSuccess)
        return cleanup_fail("hipEventCreate", e);
    if ((e = hipMalloc((void**)&b->d_env_raw, sizeof(srbd_env_params) * E)) != hipSuccess)
        return cleanup_fail("hipMalloc", e);
    if ((e = hipMalloc((void**)&b->d_env, sizeof(EnvModel) * E)) != hipSuccess) return cleanup_fail("hipMalloc", e);
    if ((e = batch_env_reset(b)) != hipSuccess) return cleanup_fail("hipMemcpy", e);
    if ((e = hipMalloc((void**)&b->d_iface_keys, sizeof(uint64_t) * 2 * E * SRBD_MAX_IFACE_ITERS)) != hipSuccess)
        return cleanup_fail("hipMalloc", e);
    // the noise padding rows (n_local .. ldn) stay zero, as in a single context
    if ((e = hipMemsetAsync(b->d_noise, 0, noise_bytes, b->c.stream)) != hipSuccess ||
        (e = hipMemsetAsync(b->d_in, 0, sizeof(StepInput) * E, b->c.stream)) != hipSuccess ||
        (e = hipMemsetAsync(b->d_costs, 0, sizeof(float) * E * (size_t)mc.ldn, b->c.stream)) != hipSuccess ||
        (e = hipMemsetAsync(b->d_eflag, 0, sizeof(uint32_t) * E, b->c.stream)) != hipSuccess ||
        (e = hipMemsetAsync(b->d_count, 0, sizeof(uint32_t), b->c.stream)) != hipSuccess ||
        (e = hipMemsetAsync(b->d_out, 0, sizeof(StepOutput) * E, b->c.stream)) != hipSuccess)
        return cleanup_fail("hipMemset", e);
    if ((e = hipStreamSynchronize(b->c.stream)) != hipSuccess) return cleanup_fail("hipStreamSynchronize", e);
    *out = b;
    return SRBD_OK;
}

extern "C" int srbd_batch_create(const srbd_config* cfg, int32_t num_envs, srbd_batch** out) {
    return batch_create(cfg, num_envs, out, false);
}

// A CEM-MPPI batch: build_model checks num_elite (2 .. SRBD_MAX_ELITE) as it does for srbd_create; the leaf records
// carry each leaf's K smallest keys, the merge block folds every column unsplit and writes out[e].sigma.
extern "C" int srbd_batch_create_cem(const srbd_config* cfg, int32_t num_envs, srbd_batch** out) {
    return batch_create(cfg, num_envs, out, true);
}

extern "C" int srbd_batch_set_rng(srbd_batch* b, int32_t kind) {
    if (!b) return SRBD_E_INVALID;
    if (kind != SRBD_RNG_PHILOX && kind != SRBD_RNG_JAX && kind != SRBD_RNG_JAX_LEGACY)
        return fail(&b->c, SRBD_E_INVALID, "unknown RNG kind");
    b->c.mc.rng = kind;  // (N - 1) P < 2^32 holds for every batch shape; no draws are made ahead
    return SRBD_OK;
}

// What srbd_batch_set_gait and srbd_batch_set_gait_device both refuse.  The host setter looks at the method before
// n_freq, the device setter after n_freq and its NULL batch (the host setter's never gets here): method_first.
static int batch_gait_refuse(srbd_batch* b, int n_freq, bool method_first) {
    srbd_ctx* c = b ? &b->c : nullptr;
    const bool cem = b && c->mc.method == SRBD_CEM_MPPI;
    const char* const no_cem =
        "gait-adaptive CEM is not provided (the reference's branch is broken as wired, SURVEY App. B #2)";
    if (method_first && cem) return fail(c, SRBD_E_INVALID, no_cem);
    if (n_freq < 1 || n_freq > SRBD_MAX_FREQS)
        return fail(c, SRBD_E_INVALID, "n_freq must be in [1, " + std::to_string(SRBD_MAX_FREQS) + "]");
    if (!b) return fail(nullptr, SRBD_E_INVALID, "srbd_batch_set_gait_device: null batch");
    if (cem) return fail(c, SRBD_E_INVALID, no_cem);
    if (c->mc.kind != SRBD_ZERO_ORDER && c->mc.S + 1 > GA_MAXCB) return fail(c, SRBD_E_INVALID, "num_splines > 32");
    if (c->mc.cost_on)
        return fail(c, SRBD_E_INVALID,
                    "gait-adaptive sampling with the opt-in cost terms has no batch form (one context runs it on its "
                    "thread-per-sample kernel): clear the cost weights first, or use separate contexts");
    return SRBD_OK;
}

// d_ga_freq (E x ldn, zero) on its first use.  async NULL: the host setter, hipMemset; else the device setter,
// hipMemsetAsync on its stream *async, so the allocation is the one call of it that may block.
static int batch_reserve_ga_freq(srbd_batch* b, const hipStream_t* async) {
    if (b->d_ga_freq) return SRBD_OK;
    const size_t bytes = sizeof(float) * (size_t)b->E * (size_t)b->c.mc.ldn;
    float* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, bytes);
    if (e == hipSuccess && (e = async ? hipMemsetAsync(d, 0, bytes, *async) : hipMemset(d, 0, bytes)) != hipSuccess)
        (void)hipFree(d);
    if (e != hipSuccess)
        return fail(&b->c, e == hipErrorOutOfMemory ? SRBD_E_NOMEM : SRBD_E_HIP,
                    std::string("hipMalloc: ") + hipGetErrorString(e));
    b->d_ga_freq = d;
    return SRBD_OK;
}

// Gait-adaptive sampling and the opt-in cost terms of a batch: srbd_set_gait / srbd_clear_gait / srbd_set_cost_terms
// with the per-step values (leg phases, frequency set, injected frequencies) per environment.  The gait fields live
// in the staging h_in[e], which srbd_batch_step's fill_input leaves alone and batch_copy_kernel carries with the rest
// of the input; ModelConst (ga, the cost weights) goes to every launch by value, so a setting holds from the next step.
extern "C" int srbd_batch_set_gait(srbd_batch* b, const float* timings, float pgg_dt, float duty_factor,
                                   const float* freq_sets, int32_t n_freq, const float* freq_rows) {
    if (!b) return SRBD_E_INVALID;
    srbd_ctx* c = &b->c;
    ModelConst& mc = c->mc;
    if (!timings || !freq_sets) return fail(c, SRBD_E_INVALID, "null argument");
    int rc;
    if ((rc = batch_gait_refuse(b, n_freq, true)) != SRBD_OK) return rc;
    if ((rc = batch_quiesce(b)) != SRBD_OK) return rc;  // the staging, d_in and d_ga_freq
    const size_t E = (size_t)b->E, ldn = (size_t)mc.ldn, N = (size_t)mc.n_local;
    if (freq_rows) {  // before the staging is touched: a failure leaves the setting as it was
        if ((rc = batch_reserve_ga_freq(b, nullptr)) != SRBD_OK) return rc;
        // environment e's N rows to e * ldn; the padding rows stay zero
        HIP_TRY(c, hipMemcpy2D(b->d_ga_freq, sizeof(float) * ldn, freq_rows, sizeof(float) * N, sizeof(float) * N, E,
                               hipMemcpyHostToDevice));
    }
    for (size_t e = 0; e < E; ++e)
        fill_gait(mc, b->h_in + e, timings + 4 * e, pgg_dt, duty_factor, freq_sets + (size_t)n_freq * e, n_freq,
                  freq_rows != nullptr);
    // a device step (srbd_batch_step_device) never reads the staging: the gait fields go to d_in here (the host step's
    // batch_copy_kernel writes the same bytes over them)
    constexpr size_t G0 = offsetof(StepInput, ga_nfreq), G1 = offsetof(StepInput, best);
    HIP_TRY(c, hipMemcpy2D((char*)b->d_in + G0, sizeof(StepInput), (const char*)b->h_in + G0, sizeof(StepInput),
                           G1 - G0, E, hipMemcpyHostToDevice));
    mc.ga = 1;
    b->ga_staging_stale = false;
    return SRBD_OK;
}

// srbd_batch_set_gait with every per-environment value in the caller's device memory, enqueued on the caller's stream:
// batch_set_gait_kernel writes d_in[e]'s gait fields as fill_gait writes the staging's (the same stores,
// srbd_gait_adapt.h) and copies the injected rows.  No synchronising call: the launch joins the device steps' event
// protocol, so it follows the last device step's reads of d_in and d_ga_freq and the next device step follows it.
// Its refusals, which srbd_batch_interface_step_device makes too before it enqueues anything
static int batch_gait_dev_check(srbd_batch* b, const srbd_batch_gait_io* io) {
    srbd_ctx* c = b ? &b->c : nullptr;
    if (!io) return fail(c, SRBD_E_INVALID, "srbd_batch_set_gait_device: null io");
    if (!io->optimize) return fail(c, SRBD_E_INVALID, "srbd_batch_set_gait_device: null required pointer: optimize");
    if ((io->pgg != nullptr) == (io->timings != nullptr))
        return fail(c, SRBD_E_INVALID, "srbd_batch_set_gait_device: exactly one of pgg and timings must be given");
    if (!io->pgg && !io->nominal_freqs)
        return fail(c, SRBD_E_INVALID, "srbd_batch_set_gait_device: timings need nominal_freqs");
    return batch_gait_refuse(b, io->n_freq, false);
}

// due: NULL, or the due mask of srbd_batch_interface_step_masked_device -- the gait fields of d_in[e] and d_ga_freq's
// slice of an environment that is not due keep what its last solve set
static int batch_set_gait_dev(srbd_batch* b, const srbd_batch_gait_io* io, const int32_t* due, void* hip_stream) {
    int rc = batch_gait_dev_check(b, io);
    if (rc != SRBD_OK) return rc;
    ModelConst& mc = b->c.mc;
    hipStream_t s;
    if ((rc = batch_dev_begin(b, hip_stream, &s)) != SRBD_OK) return rc;  // d_in and d_ga_freq
    if (io->freq_rows && (rc = batch_reserve_ga_freq(b, &s)) != SRBD_OK) return rc;
    BatchGaitJob j = {};
    j.io = *io;
    ga_chunk_bounds(mc, j.cb);
    j.random_sampling = mc.method == SRBD_RANDOM_SAMPLING;
    j.N = mc.n_local;
    j.ldn = mc.ldn;
    launch_batch_set_gait(j, b->d_in, b->d_ga_freq, b->E, s, due);
    if ((rc = batch_dev_end(b, s)) != SRBD_OK) return rc;
    mc.ga = 1;
    b->ga_staging_stale = true;
    return SRBD_OK;
}

extern "C" int srbd_batch_set_gait_device(srbd_batch* b, const srbd_batch_gait_io* io, void* hip_stream) {
    return batch_set_gait_dev(b, io, nullptr, hip_stream);
}

extern "C" int srbd_batch_clear_gait(srbd_batch* b) {
    if (!b) return SRBD_E_INVALID;
    if (b->c.mc.ga) {
        const int rc = batch_quiesce(b);
        if (rc != SRBD_OK) return rc;
        b->c.mc.ga = 0;
    }
    b->ga_staging_stale = false;  // the gait fields are not read again until a set call rewrites them
    return SRBD_OK;
}

extern "C" int srbd_batch_set_cost_terms(srbd_batch* b, const float* r_force, float w_smooth, float w_cone) {
    if (!b) return SRBD_E_INVALID;
    srbd_ctx* c = &b->c;
    ModelConst& mc = c->mc;
    if (!r_force) return fail(c, SRBD_E_INVALID, "null argument");
    const float w[5] = {r_force[0], r_force[1], r_force[2], w_smooth, w_cone};
    int on = 0;
    for (float x : w) {
        if (!(x >= 0.0f && x < INFINITY)) return fail(c, SRBD_E_INVALID, "cost weights must be finite and >= 0");
        on |= x != 0.0f;
    }
    if (on && mc.ga)
        return fail(c, SRBD_E_INVALID,
                    "the opt-in cost terms with gait-adaptive sampling have no batch form (one context runs them on "
                    "its thread-per-sample kernel): srbd_batch_clear_gait first, or use separate contexts");
    const int rc = batch_quiesce(b);
    if (rc != SRBD_OK) return rc;
    mc.cost_on = on;
    memcpy(mc.cost_r, r_force, sizeof(mc.cost_r));
    mc.cost_smooth = w_smooth;
    mc.cost_cone = w_cone;
    return SRBD_OK;
}

// Per-environment robot and cost parameters.  The records live in device memory (d_env, read by the ENVT kernels of
// srbd_batch.hip through launch_batch_*'s envs argument) and in host mirrors; the launches take envs only while
// env_on, so a batch that never set parameters, or cleared them, launches the kernels it always did.
extern "C" int srbd_batch_set_env_params(srbd_batch* b, const srbd_env_params* params, const uint8_t* mask) {
    if (!b) return fail(nullptr, SRBD_E_INVALID, "srbd_batch_set_env_params: null batch");
    srbd_ctx* c = &b->c;
    if (!params) return fail(c, SRBD_E_INVALID, "srbd_batch_set_env_params: null params");
    const int E = b->E;
    for (int e = 0; e < E; ++e)  // before anything changes
        if ((!mask || mask[e]) && !env_params_ok(params[e]))
            return fail(c, SRBD_E_INVALID,
                        "srbd_batch_set_env_params: environment " + std::to_string(e) +
                            ": need 0 <= grf_min <= grf_max and mu >= 0 (nothing was changed)");
    const int rc = batch_quiesce(b);  // the records
    if (rc != SRBD_OK) return rc;
    HIP_TRY(c, batch_env_download(b));
    for (int e = 0; e < E; ++e)
        if (!mask || mask[e]) {
            b->h_env_raw[e] = params[e];
            env_model_fill(params[e], &b->h_env[e]);
        }
    HIP_TRY(c, hipMemcpy(b->d_env_raw, b->h_env_raw.data(), sizeof(srbd_env_params) * (size_t)E,
                         hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(b->d_env, b->h_env.data(), sizeof(EnvModel) * (size_t)E, hipMemcpyHostToDevice));
    b->env_on = true;
    return SRBD_OK;
}

// The same from the caller's device memory, enqueued on the caller's stream: one launch (batch_set_env_params_kernel)
// that joins the device steps' event protocol as srbd_batch_set_gait_device does.  No synchronising call and no host
// access to device memory: the host mirrors go stale and are downloaded by the next host call that needs them.
extern "C" int srbd_batch_set_env_params_device(srbd_batch* b, const srbd_env_params* d_params, const int32_t* d_mask,
                                                int32_t* d_rejected, void* hip_stream) {
    if (!b) return fail(nullptr, SRBD_E_INVALID, "srbd_batch_set_env_params_device: null batch");
    srbd_ctx* c = &b->c;
    if (!d_params) return fail(c, SRBD_E_INVALID, "srbd_batch_set_env_params_device: null d_params");
    if ((reinterpret_cast<uintptr_t>(d_params) | reinterpret_cast<uintptr_t>(d_mask) |
         reinterpret_cast<uintptr_t>(d_rejected)) & 3)
        return fail(c, SRBD_E_INVALID,
                    "srbd_batch_set_env_params_device: d_params, d_mask and d_rejected must be 4-byte aligned");
    int rc;
    hipStream_t s;
    if ((rc = batch_dev_begin(b, hip_stream, &s)) != SRBD_OK) return rc;  // the records
    launch_batch_set_env_params(d_params, d_mask, d_rejected, b->E, b->d_env_raw, b->d_env, s);
    if ((rc = batch_dev_end(b, s)) != SRBD_OK) return rc;
    b->env_on = true;
    b->env_host_stale = true;
    return SRBD_OK;
}

extern "C" int srbd_batch_get_env_params(srbd_batch* b, srbd_env_params* out) {
    if (!b) return fail(nullptr, SRBD_E_INVALID, "srbd_batch_get_env_params: null batch");
    srbd_ctx* c = &b->c;
    if (!out) return fail(c, SRBD_E_INVALID, "srbd_batch_get_env_params: null out");
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    HIP_TRY(c, batch_join_host(b));
    HIP_TRY(c, batch_env_download(b));
    memcpy(out, b->h_env_raw.data(), sizeof(srbd_env_params) * (size_t)b->E);
    return SRBD_OK;
}

extern "C" int srbd_batch_clear_env_params(srbd_batch* b) {
    if (!b) return fail(nullptr, SRBD_E_INVALID, "srbd_batch_clear_env_params: null batch");
    srbd_ctx* c = &b->c;
    if (!b->env_on) return SRBD_OK;
    const int rc = batch_quiesce(b);
    if (rc != SRBD_OK) return rc;
    HIP_TRY(c, batch_env_reset(b));
    return SRBD_OK;
}

extern "C" int srbd_batch_copy_costs(srbd_batch* b, float* out_costs) {
    if (!b || !out_costs) return SRBD_E_INVALID;
    if (!b->stepped) return fail(&b->c, SRBD_E_STATE, "no step yet");
    srbd_ctx* c = &b->c;
    const ModelConst& mc = c->mc;
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    HIP_TRY(c, batch_join_host(b));
    HIP_TRY(c, hipMemcpy2DAsync(out_costs, sizeof(float) * mc.n_local, b->d_costs, sizeof(float) * mc.ldn,
                                sizeof(float) * mc.n_local, b->E, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SRBD_OK;
}

// srbd_batch_step (sigma NULL, cem false) and srbd_batch_step_cem
static int batch_step_host(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                           int32_t contact_stride, float* best_params, float* sigma, bool cem, const float* noise,
                           const uint64_t* seeds, const uint64_t* counters, srbd_result* out, float* out_costs) {
    if (!b) return SRBD_E_INVALID;
    srbd_ctx* c = &b->c;
    const ModelConst& mc = c->mc;
    if (!cem && mc.method == SRBD_CEM_MPPI)
        return fail(c, SRBD_E_INVALID, "CEM: sigma is part of the step (srbd_batch_step_cem)");
    if (cem && mc.method != SRBD_CEM_MPPI)
        return fail(c, SRBD_E_INVALID, "srbd_batch_step_cem: not a CEM batch (srbd_batch_create_cem)");
    if (cem && !sigma) return fail(c, SRBD_E_INVALID, "CEM: sigma is part of the step");
    if (!states || !refs || !contacts || !best_params || !seeds || !counters || !out || contact_stride < mc.H)
        return fail(c, SRBD_E_INVALID, "invalid step arguments");
    if (b->ga_staging_stale)
        return fail(c, SRBD_E_INVALID,
                    "srbd_batch_step: the gait fields were last set on the device (srbd_batch_set_gait_device) and the "
                    "host staging is stale: call srbd_batch_set_gait or srbd_batch_clear_gait first, or step with "
                    "srbd_batch_step_device");
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    if (b->dev_pending) {  // a device step in flight on another stream: this step's launches follow it
        HIP_TRY(c, hipStreamWaitEvent(c->stream, b->dev_done, 0));
        b->dev_pending = false;
    }
    const int E = b->E, P = mc.P;
    if (b->env_host_stale) {  // the parameters were last set on the device: the event above orders the download
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, batch_env_download(b));
    }
    const EnvModel* envs = b->env_on ? b->d_env : nullptr;
    for (int e = 0; e < E; ++e) {
        StepInput* in = b->h_in + e;
        const int rc = fill_input(&c->cfg, mc, in, states + 24 * (size_t)e, refs + 24 * (size_t)e,
                                  contacts + (size_t)e * 4 * contact_stride, contact_stride,
                                  best_params + (size_t)e * P, cem ? sigma + (size_t)e * P : nullptr, seeds[e],
                                  counters[e], b->env_on ? &b->h_env[e] : nullptr);
        if (rc) return fail(c, rc, "invalid step arguments");
        in->noise_scaled = noise ? 1 : 0;  // CEM: injected noise is used as given, device draws are unscaled
    }
    launch_batch_copy(b->d_in_host, b->d_in, E, offsetof(StepInput, best) + sizeof(float) * (size_t)P, c->stream,
                      offsetof(StepInput, sigma), cem ? sizeof(float) * (size_t)P : 0);
    if (noise) {
        const size_t bytes = sizeof(float) * (size_t)E * mc.n_local * P;
        if (!b->d_noise_rm) {
            const hipError_t e = hipMalloc((void**)&b->d_noise_rm, bytes);
            if (e != hipSuccess) {
                b->d_noise_rm = nullptr;
                (void)hipStreamSynchronize(c->stream);
                return fail(c, e == hipErrorOutOfMemory ? SRBD_E_NOMEM : SRBD_E_HIP,
                            std::string("hipMalloc: ") + hipGetErrorString(e));
            }
        }
        HIP_TRY(c, hipMemcpyAsync(b->d_noise_rm, noise, bytes, hipMemcpyHostToDevice, c->stream));
        launch_batch_transpose(mc, b->d_noise_rm, b->d_noise, E, c->stream);
    } else {
        launch_batch_rng(mc, b->d_in, b->d_noise, E, c->stream);
    }
    if (mc.ga)
        launch_batch_rollout_ga(mc, b->d_in, b->d_noise, b->d_costs, b->d_rec, c->wrec_stride, b->d_ga_freq, E,
                                c->stream, envs);
    else
        launch_batch_rollout(mc, b->d_in, b->d_noise, b->d_costs, b->d_rec, c->wrec_stride, E, c->stream, envs);
    const uint32_t seq = ++c->seq;
    launch_batch_merge(mc, b->d_in, b->d_rec, c->wrec_stride, b->d_noise, b->d_out_host, b->d_eflag, b->d_count,
                       c->d_flag, seq, E, c->stream, envs);
    HIP_TRY(c, hipGetLastError());
    int rc = wait_published(c, seq);
    if (rc) {  // the stream has drained (or failed): a launch that stopped part-way may have left arrivals counted
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemset(b->d_count, 0, sizeof(uint32_t));
        return rc;
    }
    b->stepped = true;
    if (out_costs && (rc = srbd_batch_copy_costs(b, out_costs))) return rc;
    for (int e = 0; e < E; ++e) {
        const StepOutput& o = b->h_out[e];
        memcpy(best_params + (size_t)e * P, o.best, sizeof(float) * P);
        if (cem) memcpy(sigma + (size_t)e * P, o.sigma, sizeof(float) * P);
        memcpy(out[e].grf, o.grf, sizeof(out[e].grf));
        memcpy(out[e].predicted_state, o.pred, sizeof(out[e].predicted_state));
        out[e].best_cost = o.best_cost;
        out[e].best_index = o.best_index;
        out[e].best_freq = o.best_freq;
        out[e].status = o.status;
    }
    return SRBD_OK;
}

extern "C" int srbd_batch_step(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                               int32_t contact_stride, float* best_params, const float* noise, const uint64_t* seeds,
                               const uint64_t* counters, srbd_result* out, float* out_costs) {
    return batch_step_host(b, states, refs, contacts, contact_stride, best_params, nullptr, false, noise, seeds,
                           counters, out, out_costs);
}

extern "C" int srbd_batch_step_cem(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                                   int32_t contact_stride, float* best_params, float* sigma, const float* noise,
                                   const uint64_t* seeds, const uint64_t* counters, srbd_result* out,
                                   float* out_costs) {
    return batch_step_host(b, states, refs, contacts, contact_stride, best_params, sigma, true, noise, seeds, counters,
                           out, out_costs);
}

// srbd_batch_step with every array in the caller's device memory, enqueued on the caller's stream: batch_pack_kernel
// builds d_in[e] as fill_input does, the draws / transpose (reading io->noise in place), rollouts and merges are the
// host step's launches, the merge blocks write their records to d_out (device memory) and batch_unpack_kernel scatters
// them and the costs rows to the caller's arrays.  The sequence word is advanced and stored as in the host step, and
// not waited on.  No synchronising call: the event behind the last launch orders the other entry points after it.
// srbd_batch_step_device (cem NULL, is_cem false) and srbd_batch_step_cem_device: batch_pack_cem_kernel also writes
// d_in[e].sigma (the caller's rows or the reset constant) and batch_unpack_cem_kernel also scatters d_out[e].sigma.
// Its refusals, which srbd_batch_interface_step_device makes too before it enqueues anything
// The entry point's name in the messages: the masked forms (srbd_batch_step_masked_device, _step_cem_masked_device) or
// the unmasked ones
static const char* batch_step_dev_name(bool is_cem, bool masked) {
    if (masked) return is_cem ? "srbd_batch_step_cem_masked_device" : "srbd_batch_step_masked_device";
    return is_cem ? "srbd_batch_step_cem_device" : "srbd_batch_step_device";
}
static int batch_step_dev_check(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem,
                                bool is_cem, bool masked = false) {
    // the arguments first, so a bad io is named as such whatever b is (b == NULL: the calling thread's error text)
    srbd_ctx* c = b ? &b->c : nullptr;
    const std::string fn = batch_step_dev_name(is_cem, masked);
    if (!io) return fail(c, SRBD_E_INVALID, fn + ": null io");
    if (is_cem) {
        if (!cem) return fail(c, SRBD_E_INVALID, fn + ": null cem");
        if (!cem->sigma) return fail(c, SRBD_E_INVALID, fn + ": null required pointer: sigma");
        if (!(cem->sigma_reset >= 0.0f && cem->sigma_reset < INFINITY))
            return fail(c, SRBD_E_INVALID, fn + ": sigma_reset must be finite and >= 0");
    }
    const batch_req req[] = {{io->states, "states"},       {io->refs, "refs"},
                             {io->contacts, "contacts"},   {io->seeds, "seeds"},
                             {io->counters, "counters"},   {io->best_params, "best_params"},
                             {io->grf, "grf"},             {io->predicted_state, "predicted_state"},
                             {io->best_cost, "best_cost"}, {io->best_index, "best_index"},
                             {io->best_freq, "best_freq"}, {io->status, "status"}};
    if (const char* name = batch_first_null(req))
        return fail(c, SRBD_E_INVALID, fn + ": null required pointer: " + name);
    if (!b) return fail(nullptr, SRBD_E_INVALID, fn + ": null batch");
    const ModelConst& mc = c->mc;
    if (!is_cem && mc.method == SRBD_CEM_MPPI)
        return fail(c, SRBD_E_INVALID,
                    std::string("CEM: sigma is part of the step (") + batch_step_dev_name(true, masked) + ")");
    if (is_cem && mc.method != SRBD_CEM_MPPI)
        return fail(c, SRBD_E_INVALID, fn + ": not a CEM batch (srbd_batch_create_cem)");
    if (io->contact_stride < mc.H)
        return fail(c, SRBD_E_INVALID, fn + ": contact_stride is smaller than the horizon");
    return SRBD_OK;
}

// due: NULL (the unmasked entry points: the launches they always made, the kernels' mask argument NULL), or the due
// mask of the masked ones, handed to every launch -- the same grids, and the blocks of an environment that is not due
// return at once.  The merge blocks count themselves whatever the mask holds, so d_count is zero and `seq` stored
// behind every call: the next step, host or device, masked or not, finds the counter and the word as it expects them.
static int batch_step_dev(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem, bool is_cem,
                          void* hip_stream, const int32_t* due = nullptr, bool masked = false) {
    int rc = batch_step_dev_check(b, io, cem, is_cem, masked);
    if (rc != SRBD_OK) return rc;
    srbd_ctx* c = &b->c;
    const ModelConst& mc = c->mc;
    hipStream_t s;
    if ((rc = batch_dev_begin(b, hip_stream, &s)) != SRBD_OK) return rc;
    const int E = b->E;
    const EnvModel* envs = b->env_on ? b->d_env : nullptr;
    launch_batch_pack(mc, c->cfg.q_diag + 12, *io, b->d_in, E, s, is_cem ? cem : nullptr, envs, due);
    if (io->noise)
        launch_batch_transpose(mc, io->noise, b->d_noise, E, s, due);
    else
        launch_batch_rng(mc, b->d_in, b->d_noise, E, s, due);
    if (mc.ga)
        launch_batch_rollout_ga(mc, b->d_in, b->d_noise, b->d_costs, b->d_rec, c->wrec_stride, b->d_ga_freq, E, s,
                                envs, due);
    else
        launch_batch_rollout(mc, b->d_in, b->d_noise, b->d_costs, b->d_rec, c->wrec_stride, E, s, envs, due);
    const uint32_t seq = ++c->seq;
    launch_batch_merge(mc, b->d_in, b->d_rec, c->wrec_stride, b->d_noise, b->d_out, b->d_eflag, b->d_count, c->d_flag,
                       seq, E, s, envs, due);
    launch_batch_unpack(mc, *io, b->d_out, b->d_costs, E, s, is_cem ? cem->sigma : nullptr, due);
    if ((rc = batch_dev_end(b, s)) != SRBD_OK) return rc;
    b->stepped = true;
    return SRBD_OK;
}

extern "C" int srbd_batch_step_device(srbd_batch* b, const srbd_batch_device_io* io, void* hip_stream) {
    return batch_step_dev(b, io, nullptr, false, hip_stream);
}

extern "C" int srbd_batch_step_cem_device(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem,
                                          void* hip_stream) {
    return batch_step_dev(b, io, cem, true, hip_stream);
}

// The masked steps (SCI:134 of the reference's wrapper: the solve runs only on the steps that are due).  io and due
// are looked at first, so either is named whatever b is; the rest is the unmasked step's.
static int batch_step_masked(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem, bool is_cem,
                             const int32_t* due, void* hip_stream) {
    srbd_ctx* c = b ? &b->c : nullptr;
    const std::string fn = batch_step_dev_name(is_cem, true);
    if (!io) return fail(c, SRBD_E_INVALID, fn + ": null io");
    if (!due)
        return fail(c, SRBD_E_INVALID,
                    fn + ": null due (to step every environment call " + batch_step_dev_name(is_cem, false) + ")");
    return batch_step_dev(b, io, cem, is_cem, hip_stream, due, true);
}

extern "C" int srbd_batch_step_masked_device(srbd_batch* b, const srbd_batch_device_io* io, const int32_t* due,
                                             void* hip_stream) {
    return batch_step_masked(b, io, nullptr, false, due, hip_stream);
}

extern "C" int srbd_batch_step_cem_masked_device(srbd_batch* b, const srbd_batch_device_io* io,
                                                 const srbd_batch_cem_io* cem, const int32_t* due, void* hip_stream) {
    return batch_step_masked(b, io, cem, true, due, hip_stream);
}

// SRBDControllerInterface.compute_control's sampling branch (srbd_controller_interface.py:113-180, :225-229) for every
// environment of a batch, enqueued on the caller's stream: srbd_interface_step (srbd_host.cpp) statement for statement.
// The prologue launch is its prepare_state and its with_newkey of every iteration (the step keys go to d_iface_keys,
// one row per iteration); the iterations are srbd_batch_step_device / _step_cem_device as they are, reading their row
// (the CEM form with sigma_reset at iteration 0: with_newsigma); the epilogue launch is the mask, the footholds and
// previous_contact_mpc.  Every refusal -- this call's, the gait setter's and the step's -- is made before the first
// launch, so a refused call has changed nothing.  The step keys are read by the steps' pack launches only, which the
// event protocol of the steps already orders against a call on another stream; the prologue joins it here, and the
// event is recorded once more behind the epilogue, so a call on another stream also follows the epilogue's store of
// previous_contact, the one caller-owned array that is state between calls.
// due: NULL (srbd_batch_interface_step_device), or the due mask of srbd_batch_interface_step_masked_device, handed to
// the prologue, the gait setter, every iteration's step and the epilogue.
static int batch_iface_step(srbd_batch* b, const srbd_batch_interface_io* io, const int32_t* due, void* hip_stream) {
    srbd_ctx* c = b ? &b->c : nullptr;
    const bool masked = due != nullptr;
    const std::string fn = masked ? "srbd_batch_interface_step_masked_device" : "srbd_batch_interface_step_device";
    if (!b) return fail(nullptr, SRBD_E_INVALID, fn + ": null batch");
    if (!io) return fail(c, SRBD_E_INVALID, fn + ": null io");
    const ModelConst& mc = c->mc;
    const bool is_cem = mc.method == SRBD_CEM_MPPI;
    const batch_req req[] = {{io->state_in, "state_in"},   {io->ref_in, "ref_in"},
                             {io->contacts, "contacts"},   {io->keys, "keys"},
                             {io->previous_contact, "previous_contact"},
                             {io->best_params, "best_params"},
                             {io->states, "states"},       {io->refs, "refs"},
                             {io->grf, "grf"},             {io->footholds, "footholds"},
                             {io->grf_raw, "grf_raw"},     {io->predicted_state, "predicted_state"},
                             {io->best_cost, "best_cost"}, {io->best_index, "best_index"},
                             {io->best_freq, "best_freq"}, {io->status, "status"}};
    if (const char* name = batch_first_null(req))
        return fail(c, SRBD_E_INVALID, fn + ": null required pointer: " + name);
    if (is_cem && !io->sigma) return fail(c, SRBD_E_INVALID, fn + ": null required pointer: sigma (a CEM batch)");
    if (io->iterations < 1 || io->iterations > SRBD_MAX_IFACE_ITERS)
        return fail(c, SRBD_E_INVALID, fn + ": iterations must be in [1, " + std::to_string(SRBD_MAX_IFACE_ITERS) + "]");
    if (io->contact_stride < mc.H) return fail(c, SRBD_E_INVALID, fn + ": contact_stride is smaller than the horizon");
    if (io->params_per_leg < 1 || (int64_t)4 * io->params_per_leg != mc.P)
        return fail(c, SRBD_E_INVALID,
                    fn + ": params_per_leg must be >= 1 and 4 * params_per_leg the batch's " + std::to_string(mc.P) +
                        " parameters");
    if (is_cem && !(io->sigma_reset > 0.0f && io->sigma_reset < INFINITY))
        return fail(c, SRBD_E_INVALID, fn + ": sigma_reset must be positive and finite on a CEM batch");
    if (is_cem && io->gait)
        return fail(c, SRBD_E_INVALID, fn + ": gait on a CEM batch (gait-adaptive CEM is not provided)");
    if (io->gait && mc.cost_on)
        return fail(c, SRBD_E_INVALID,
                    fn + ": gait together with active cost terms (gait-adaptive sampling with the opt-in cost terms "
                         "has no batch form)");
    int rc;
    if (io->gait && (rc = batch_gait_dev_check(b, io->gait)) != SRBD_OK) return rc;
    srbd_batch_device_io sio = {};
    sio.states = io->states, sio.refs = io->refs, sio.contacts = io->contacts;
    sio.seeds = b->d_iface_keys, sio.counters = b->d_iface_keys + b->E;
    sio.contact_stride = io->contact_stride;
    sio.best_params = io->best_params;
    sio.grf = io->grf_raw, sio.predicted_state = io->predicted_state, sio.best_cost = io->best_cost;
    sio.best_index = io->best_index, sio.best_freq = io->best_freq, sio.status = io->status, sio.costs = io->costs;
    srbd_batch_cem_io cem = {io->sigma, io->sigma_reset, 0};
    if ((rc = batch_step_dev_check(b, &sio, is_cem ? &cem : nullptr, is_cem, masked)) != SRBD_OK) return rc;
    hipStream_t s;
    if ((rc = batch_dev_begin(b, hip_stream, &s)) != SRBD_OK) return rc;  // d_iface_keys
    launch_iface_prologue(*io, mc.rng, mc.P, b->d_iface_keys, b->E, s, due);
    HIP_TRY(c, hipGetLastError());  // the steps below record the event behind their launches
    // the explicit handle again for the calls below: NULL would mean the batch's own stream to them
    void* const hs = s ? (void*)s : (void*)hipStreamLegacy;
    if (io->gait && (rc = batch_set_gait_dev(b, io->gait, due, hs)) != SRBD_OK) return rc;
    for (int it = 0; it < io->iterations; ++it) {
        sio.seeds = b->d_iface_keys + 2 * (size_t)it * b->E;
        sio.counters = sio.seeds + b->E;
        cem.sigma_reset = it == 0 ? io->sigma_reset : 0.0f;
        if ((rc = batch_step_dev(b, &sio, is_cem ? &cem : nullptr, is_cem, hs, due, masked)) != SRBD_OK) return rc;
    }
    launch_iface_epilogue(*io, b->E, s, due);
    // the event again, behind the epilogue: previous_contact lives between calls, so a following call on another
    // stream, which waits on the event, must see the epilogue's store of it and not only the last step
    return batch_dev_end(b, s);
}

extern "C" int srbd_batch_interface_step_device(srbd_batch* b, const srbd_batch_interface_io* io, void* hip_stream) {
    return batch_iface_step(b, io, nullptr, hip_stream);
}

// io and due are looked at first, so either is named whatever b is
extern "C" int srbd_batch_interface_step_masked_device(srbd_batch* b, const srbd_batch_interface_io* io,
                                                       const int32_t* due, void* hip_stream) {
    srbd_ctx* c = b ? &b->c : nullptr;
    const std::string fn = "srbd_batch_interface_step_masked_device";
    if (!io) return fail(c, SRBD_E_INVALID, fn + ": null io");
    if (!due)
        return fail(c, SRBD_E_INVALID,
                    fn + ": null due (to step every environment call srbd_batch_interface_step_device)");
    return batch_iface_step(b, io, due, hip_stream);
}

// The full-horizon plan (srbd_plan.hip): one launch over the caller's device arrays on the caller's stream, inside the
// device steps' event protocol -- the launch reads d_in[e]'s gait fields and the environment records, which the device
// setters write on their streams, and a plan behind a step on another stream has to follow that step's outputs.
// Its refusals, before anything is enqueued
static int batch_plan_check(srbd_batch* b, const srbd_batch_plan_io* io) {
    srbd_ctx* c = b ? &b->c : nullptr;
    const std::string fn = "srbd_batch_plan_device";
    if (!io) return fail(c, SRBD_E_INVALID, fn + ": null io");
    const batch_req req[] = {{io->states, "states"}, {io->refs, "refs"}, {io->params, "params"}};
    if (const char* name = batch_first_null(req))
        return fail(c, SRBD_E_INVALID, fn + ": null required pointer: " + name);
    if (!io->plan_states && !io->plan_grfs && !io->plan_contacts && !io->plan_run_cost && !io->plan_cost)
        return fail(c, SRBD_E_INVALID, fn + ": every output is NULL");
    if (!b) return fail(nullptr, SRBD_E_INVALID, fn + ": null batch");
    const ModelConst& mc = c->mc;
    if (mc.ga) {
        if (!io->freqs)
            return fail(c, SRBD_E_INVALID,
                        fn + ": null required pointer: freqs (gait-adaptive sampling is set: the contact sequence "
                             "comes from each environment's step frequency)");
    } else {
        if (!io->contacts) return fail(c, SRBD_E_INVALID, fn + ": null required pointer: contacts");
        if (io->contact_stride < mc.H)
            return fail(c, SRBD_E_INVALID, fn + ": contact_stride is smaller than the horizon");
    }
    return SRBD_OK;
}

extern "C" int srbd_batch_plan_device(srbd_batch* b, const srbd_batch_plan_io* io, void* hip_stream) {
    int rc = batch_plan_check(b, io);
    if (rc != SRBD_OK) return rc;
    srbd_ctx* c = &b->c;
    const ModelConst& mc = c->mc;
    hipStream_t s;
    if ((rc = batch_dev_begin(b, hip_stream, &s)) != SRBD_OK) return rc;
    PlanJob j = {};
    j.states = io->states, j.refs = io->refs, j.contacts = io->contacts, j.params = io->params, j.freqs = io->freqs;
    j.plan_states = io->plan_states, j.plan_grfs = io->plan_grfs, j.plan_contacts = io->plan_contacts;
    j.plan_run_cost = io->plan_run_cost, j.plan_cost = io->plan_cost;
    j.in_arr = b->d_in;
    j.envs = b->env_on ? b->d_env : nullptr;
    memcpy(j.q_feet, c->cfg.q_diag + 12, sizeof(j.q_feet));
    j.mg = mc.mg;
    j.contact_stride = io->contact_stride, j.E = b->E, j.hc = plan_chunk(mc.H), j.in_single = 0;
    const hipError_t le = launch_plan(mc, j, s);
    if ((rc = batch_dev_end(b, s)) != SRBD_OK) return rc;
    HIP_TRY(c, le);
    return SRBD_OK;
}

// The same arrays in host memory: one device buffer holds the inputs (contacts packed to stride H) and the outputs;
// upload, the launch on the batch's stream, download, one wait.
extern "C" int srbd_batch_plan(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                               int32_t contact_stride, const float* params, const float* freqs, float* plan_states,
                               float* plan_grfs, float* plan_contacts, float* plan_run_cost, float* plan_cost) {
    srbd_batch_plan_io io = {states, refs,        contacts,  params,        freqs,         contact_stride, 0,
                             plan_states, plan_grfs, plan_contacts, plan_run_cost, plan_cost};
    int rc = batch_plan_check(b, &io);
    if (rc != SRBD_OK) return rc;
    srbd_ctx* c = &b->c;
    const ModelConst& mc = c->mc;
    const size_t E = (size_t)b->E, H = (size_t)mc.H, P = (size_t)mc.P;
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    // floats: states | refs | contacts (stride H) | params | freqs | the five outputs
    // (every array on a 16-byte boundary, so the launch takes its 16-byte stores)
    auto al = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t o_st = 0, o_rf = o_st + 24 * E, o_ct = o_rf + 24 * E, o_pr = o_ct + 4 * H * E, o_fq = o_pr + P * E,
                 o_ps = al(o_fq + E), o_pg = o_ps + 12 * H * E, o_pc = o_pg + 12 * H * E, o_rc = o_pc + 4 * H * E,
                 o_co = al(o_rc + H * E), total = o_co + E;
    if (!b->d_plan) {
        const hipError_t e = hipMalloc((void**)&b->d_plan, sizeof(float) * total);
        if (e != hipSuccess) {
            b->d_plan = nullptr;
            return fail(c, e == hipErrorOutOfMemory ? SRBD_E_NOMEM : SRBD_E_HIP,
                        std::string("hipMalloc: ") + hipGetErrorString(e));
        }
    }
    float* d = b->d_plan;
    hipStream_t s = c->stream;
    if (b->dev_pending && b->dev_stream != s) HIP_TRY(c, hipStreamWaitEvent(s, b->dev_done, 0));  // d_plan's last reader
    HIP_TRY(c, hipMemcpyAsync(d + o_st, states, sizeof(float) * 24 * E, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_rf, refs, sizeof(float) * 24 * E, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_pr, params, sizeof(float) * P * E, hipMemcpyHostToDevice, s));
    if (mc.ga)
        HIP_TRY(c, hipMemcpyAsync(d + o_fq, freqs, sizeof(float) * E, hipMemcpyHostToDevice, s));
    else
        HIP_TRY(c, hipMemcpy2DAsync(d + o_ct, sizeof(float) * H, contacts, sizeof(float) * (size_t)contact_stride,
                                    sizeof(float) * H, 4 * E, hipMemcpyHostToDevice, s));
    srbd_batch_plan_io dio = {d + o_st, d + o_rf, d + o_ct, d + o_pr, d + o_fq, (int32_t)H, 0,
                              plan_states ? d + o_ps : nullptr, plan_grfs ? d + o_pg : nullptr,
                              plan_contacts ? d + o_pc : nullptr, plan_run_cost ? d + o_rc : nullptr,
                              plan_cost ? d + o_co : nullptr};
    if ((rc = srbd_batch_plan_device(b, &dio, nullptr)) != SRBD_OK) return rc;
    if (plan_states) HIP_TRY(c, hipMemcpyAsync(plan_states, d + o_ps, sizeof(float) * 12 * H * E, hipMemcpyDeviceToHost, s));
    if (plan_grfs) HIP_TRY(c, hipMemcpyAsync(plan_grfs, d + o_pg, sizeof(float) * 12 * H * E, hipMemcpyDeviceToHost, s));
    if (plan_contacts)
        HIP_TRY(c, hipMemcpyAsync(plan_contacts, d + o_pc, sizeof(float) * 4 * H * E, hipMemcpyDeviceToHost, s));
    if (plan_run_cost) HIP_TRY(c, hipMemcpyAsync(plan_run_cost, d + o_rc, sizeof(float) * H * E, hipMemcpyDeviceToHost, s));
    if (plan_cost) HIP_TRY(c, hipMemcpyAsync(plan_cost, d + o_co, sizeof(float) * E, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return SRBD_OK;
}
