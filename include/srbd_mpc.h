/*
 * srbd_mpc.h -- C-ABI of the MI355X-native sampling SRBD MPC (libsrbd_hip.so).
 *
 * This is the drop-in boundary for the reference's sampling controller hot path.
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference repository root Magicyw/Quadruped-PyMPC-TAMOLS):
 *
 *   srbd_create            <- Sampling_MPC.__init__            centroidal_nmpc_jax.py:23-178
 *   srbd_step              <- Sampling_MPC.jitted_compute_control, i.e.
 *                             compute_control_random_sampling   centroidal_nmpc_jax.py:629-787
 *                             compute_control_mppi              centroidal_nmpc_jax.py:789-932
 *                             compute_control_cem_mppi          centroidal_nmpc_jax.py:934-1094
 *                             (called from srbd_controller_interface.py:140,159)
 *   srbd_step_local /
 *   srbd_step_finish       <- the same call, split around the one cross-GPU exchange
 *                             (row-sharded rollouts)
 *   srbd_tamols_run        <- VisualFootholdAdaptation.compute_adaptation, strategy 'tamols'
 *                             visual_foothold_adaptation.py:153-231 (+ helpers :261-714)
 *   srbd_terrain_patches   <- gym_quadruped HeightMap.update_height_map (wb_interface.py:233-234)
 *
 * Conventions: plain pointers and sizes, caller owns every host array, nothing is
 * retained past a call, 0 = success and negative SRBD_E* codes on failure (message
 * via srbd_last_error), nothing throws across the ABI.  One context per thread or
 * process; a context creates its HIP state lazily in srbd_create (never at load).
 * Results are bitwise reproducible for identical inputs (fixed reduction order).
 */
#ifndef SRBD_MPC_H
#define SRBD_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRBD_ABI_VERSION 1
#define SRBD_MAX_HORIZON 32
#define SRBD_MAX_PARAMS 384
#define SRBD_MAX_ELITE 16
#define SRBD_MAX_FREQS 8 /* candidate step frequencies of the gait-adaptive sampler */

enum {
    SRBD_OK = 0,
    SRBD_E_INVALID = -1,  /* bad argument / unsupported configuration */
    SRBD_E_HIP = -2,      /* HIP runtime error */
    SRBD_E_NODEVICE = -3, /* no HIP device visible: there is no CPU fallback */
    SRBD_E_STATE = -4,    /* call out of order */
    SRBD_E_NOMEM = -5
};

/* mpc_params['sampling_method'] (config.py:181) */
enum { SRBD_RANDOM_SAMPLING = 0, SRBD_MPPI = 1, SRBD_CEM_MPPI = 2 };
/* mpc_params['control_parametrization'] (config.py:182) */
enum { SRBD_ZERO_ORDER = 0, SRBD_LINEAR_SPLINE = 1, SRBD_CUBIC_SPLINE = 2 };

typedef struct srbd_config {
    int32_t num_samples;     /* N = num_parallel_computations (global, all ranks) */
    int32_t horizon;         /* H (<= SRBD_MAX_HORIZON) */
    int32_t method;          /* SRBD_RANDOM_SAMPLING | SRBD_MPPI | SRBD_CEM_MPPI */
    int32_t parametrization; /* SRBD_ZERO_ORDER | SRBD_LINEAR_SPLINE | SRBD_CUBIC_SPLINE */
    int32_t num_splines;     /* S (linear / cubic) */
    int32_t num_elite;       /* CEM elite count; reference: 10 (centroidal_nmpc_jax.py:1075) */
    int32_t device_id;       /* HIP ordinal */
    int32_t rank;            /* shard index: rows srbd_shard_rows(num_samples, rank, world_size) */
    int32_t world_size;      /* 1 for single GPU */
    int32_t use_graph;       /* 1: replay srbd_step as one hipGraph */
    float mass;              /* config.mass */
    float mg;                /* float32(mass * 9.81), rounded once from double as the reference does */
    float grf_min, grf_max, mu;
    float inertia[9];        /* config.inertia, row-major, float32 */
    float dts[SRBD_MAX_HORIZON]; /* Centroidal_Model_JAX.dts (centroidal_model_jax.py:42-53) */
    float q_diag[24];        /* diag(Q), centroidal_nmpc_jax.py:118-130 */
    float sigma_mppi;        /* mpc_params['sigma_mppi'] */
    float sigma_random_sampling[3]; /* mpc_params['sigma_random_sampling'] */
} srbd_config;

typedef struct srbd_result {
    float grf[12];             /* nmpc_GRFs (FL, FR, RL, RR) x (x, y, z) */
    float predicted_state[24]; /* nmpc_predicted_state */
    float best_cost;           /* saturated cost of the best sample */
    int32_t best_index;        /* global row of the best sample (nanargmin, first on ties) */
    int32_t status;
    float best_freq;           /* gait-adaptive: step frequency of the best sample (best_step_frequency,
                                  centroidal_nmpc_jax_gait_adaptive.py:705,861); 0 otherwise */
} srbd_result;

typedef struct srbd_ctx srbd_ctx;

/* Parameter count P for a configuration (centroidal_nmpc_jax.py:52-93), or < 0. */
int srbd_num_params(const srbd_config* cfg);
int srbd_device_count(int32_t* count);
int srbd_abi_version(void);

int srbd_create(const srbd_config* cfg, srbd_ctx** out);
void srbd_destroy(srbd_ctx* ctx);
/* Last error of ctx, or of the calling thread's last failed srbd_create when ctx == NULL. */
const char* srbd_last_error(const srbd_ctx* ctx);
/* Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); disables graphs. */
int srbd_set_stream(srbd_ctx* ctx, void* hip_stream);

/*
 * One sampling iteration (one jitted_compute_control call).
 *   state, ref        : 24 floats each (prepare_state_and_reference output, cast to f32)
 *   contact           : 4 rows x contact_stride floats, row-major; the first H columns are used
 *   best_params       : P floats, in: previous best, out: updated best (reassigned by the interface)
 *   sigma             : P floats (CEM only, in/out; NULL otherwise)
 *   noise             : NULL -> device RNG: Philox4x32-10 keyed by (seed, counter), or the reference's
 *                       jax.random stream keyed by seed (srbd_set_rng);
 *                       else N x P row-major additional_random_parameters (row 0 must be zero)
 *   out_costs         : N floats (saturated) or NULL
 */
int srbd_step(srbd_ctx* ctx, const float* state, const float* ref, const float* contact, int32_t contact_stride,
              float* best_params, float* sigma, const float* noise, uint64_t seed, uint64_t counter,
              srbd_result* out, float* out_costs);

/* Armed host steps: the same srbd_step calls with the launch latency taken off the call.  Each
 * srbd_step with device draws (noise == NULL) queues its successor -- copy, rollout and merge for
 * (seed, counter + 1) -- behind itself; that chain's copy kernel waits (bounded by deadline_us, 0: 50 ms)
 * on a host-mapped word, and the next srbd_step stores its inputs and that word instead of launching.  A
 * call the chain cannot serve (injected noise, another counter or seed, past half the deadline) and every
 * other entry point cancel it: the cancelled chain computes nothing (its copy kernel writes its verdict
 * to a device word every kernel of the chain checks first) and nothing a caller reads changes.  A claimed
 * chain whose copy kernel had already given up (deadline passed before the go word) publishes a cancel
 * token instead of outputs, and the call re-runs unarmed.  Outputs are bit-identical to unarmed steps.  One context per process
 * is armed at a time.  While armed, the copy kernel occupies its hardware queue (other streams of the
 * process that share that queue wait behind it, up to the deadline), hence opt-in: for a process whose
 * controller owns the GPU queue (the reference's 100 Hz MPC loop).  No reference counterpart (launch
 * latency has none in JAX's dispatch model); replaces nothing in SCI:140-159's call.  enable = 0 cancels. */
int srbd_set_armed(srbd_ctx* ctx, int32_t enable, uint64_t deadline_us);
/* Armed steps served (fired) and cancelled since the context was created. */
int srbd_armed_stats(const srbd_ctx* ctx, int64_t* served, int64_t* cancelled);
/* Claimed chains that had already given up and were re-run unarmed (counted as cancelled above). */
int srbd_armed_refired(const srbd_ctx* ctx, int64_t* refired);
/* Test hook: the host sleeps delay_us between claiming an armed chain and storing its go word. */
int srbd_debug_arm_delay(srbd_ctx* ctx, uint32_t delay_us);
/* Test hook: the next column-split merge (CEM, or > 256 records) has one slice withhold its hand-off word, so
 * the tail block's bounded wait (2 s) times out and the step fails with SRBD_E_HIP; the call resets the
 * hand-off state, and the following step is exact again. */
int srbd_debug_split_drop(srbd_ctx* ctx);
/* srbd_foothold_mpc_step calls on this context that ran chained on the device (TAMOLS writing the step's input;
 * one host wait), since the context was created. */
int srbd_foothold_chained(const srbd_ctx* ctx, int64_t* n);

/*
 * Gait-adaptive sampling (centroidal_nmpc_jax_gait_adaptive.py; replaces
 * compute_rollout :326-501 and the step-frequency draws :687-692 (random sampling), :834-838
 * (MPPI)).  After this call every step of the context (srbd_step, the sharded and device-resident
 * forms) samples one step frequency per sample and rolls out with that sample's own contact
 * sequence: PeriodicGaitGeneratorJax (periodic_gait_generator_jax.py:68-151) advanced from
 * `timing` with pgg_dt * f per step and contact = t < duty_factor; the per-leg decode index counts
 * the leg's stance steps (GA:353-379) and the cost gains (f - 1.3) * 100 * (f - 1.3) (GA:500).
 * The caller's contact sequence of srbd_step is still the one the final GRFs use (GA:720-796).
 *   timing      : 4 floats, the periodic gait generator phase of each leg (pgg_phase_signal)
 *   pgg_dt      : mpc_params['dt'] (GA:179);  duty_factor: 0.65 in the reference (GA:179)
 *   freq_set    : n_freq (1..SRBD_MAX_FREQS) candidate frequencies, drawn uniformly per sample
 *                 (jax.random.choice); the caller forms the set per method and call:
 *                 RS: optimize_swing ? step_freq_available : n x nominal; MPPI: step_freq_available
 *   freq_local  : NULL -> device draw (Philox, keyed by seed/counter and global row); else the
 *                 frequency of each of this shard's rows (parity / injection mode, like `noise`)
 * Call again before each step to change any of these; srbd_clear_gait returns to the plain path.
 * CEM is not supported (the reference's gait-adaptive CEM is broken as wired):
 * SRBD_E_INVALID.
 */
int srbd_set_gait(srbd_ctx* ctx, const float* timing, float pgg_dt, float duty_factor, const float* freq_set,
                  int32_t n_freq, const float* freq_local);
int srbd_clear_gait(srbd_ctx* ctx);

/*
 * Opt-in per-sample cost terms (the north star's "friction-cone + GRF-smoothing terms").  The
 * reference's sampling cost has none of them (its R input cost is commented out, NMPC:132-157 and
 * :453-484; the cone is enforced by projection), so all weights default to 0 and
 * then the cost is exactly the reference's.  Per horizon step and leg, with f the clipped, masked
 * force and fref the step's gravity share:
 *   r_force[q] * u_q^2         u = (fx, fy, fz - fref if the leg is in stance else fz)
 *                              (the reference's R; its values were 0.1, 0.1, 0.001)
 *   w_smooth * |f_n - f_{n-1}|^2            steps n >= 1 (GRF smoothing)
 *   w_cone * (max(0, |fx'| - mu fz)^2 + max(0, |fy'| - mu fz)^2)   fx', fy' before the cone clip
 * Weights must be finite and >= 0.  Applies to every following step of the context (all methods,
 * parametrizations and rollout forms, gait-adaptive included).
 */
int srbd_set_cost_terms(srbd_ctx* ctx, const float r_force[3], float w_smooth, float w_cone);

/*
 * Device noise stream of every following step of the context (default SRBD_RNG_PHILOX):
 *   SRBD_RNG_PHILOX     : Philox4x32-10 + Box-Muller keyed by (seed, counter) (this library's own stream)
 *   SRBD_RNG_JAX        : the reference's jax.random stream (centroidal_nmpc_jax.py:654-676, 811, 957;
 *                         gait-adaptive choice :692, 836), jax_threefry_partitionable = True (JAX >= 0.5)
 *   SRBD_RNG_JAX_LEGACY : the same with jax_threefry_partitionable = False (earlier JAX)
 * In the JAX modes the `seed` of srbd_step is the step's key (uint32[2] packed key[0] << 32 | key[1], the
 * key the reference's interface passes: master_key after with_newkey, srbd_controller_interface.py:126-164);
 * `counter` only numbers the steps.  The draws made ahead (fused next-step draws, device-resident chains,
 * armed steps) assume the next key is with_newkey's split(key)[0] (srbd_jax_split, include/srbd_host.h).
 */
enum { SRBD_RNG_PHILOX = 0, SRBD_RNG_JAX = 1, SRBD_RNG_JAX_LEGACY = 2 };
int srbd_set_rng(srbd_ctx* ctx, int32_t kind);
int srbd_get_rng(const srbd_ctx* ctx);

/* Sharded form.  The rows of a rank are whole nodes of one level of the fixed reduction tree every merge
 * folds (64-row leaves, 32 children per node; the exchange level is the highest one that gives every rank a
 * node), so the merged result is the same bits for every world_size.  A rank's record ("rank buffer") holds
 * its nodes of that level, ceil(nodes / world_size) record slots; gathered in rank order the buffers are the
 * level's node list.  Size in floats (identical on every rank). */
int srbd_record_floats(const srbd_ctx* ctx);
/* Host-only: srbd_record_floats of a context of this configuration (rank / world_size as given). */
int srbd_record_floats_host(const srbd_config* cfg);
/* Host-only: the first global row and row count of `rank` of `world` ranks over num_samples rows
 * (SRBD_E_INVALID when some rank would get no node). */
int srbd_shard_rows(int64_t num_samples, int32_t rank, int32_t world, int64_t* row0, int64_t* rows);
/* Rows of this rank only; writes this rank's partial record to d_record (device pointer).
 * noise_local: NULL or (rows of this shard) x P row-major.  Asynchronous on the context stream. */
int srbd_step_local(srbd_ctx* ctx, const float* state, const float* ref, const float* contact, int32_t contact_stride,
                    const float* best_params, const float* sigma, const float* noise_local, uint64_t seed,
                    uint64_t counter, void* d_record);
/* Merge the gathered rank buffers (device pointer, rank order; num_records == world_size) and finish the step. */
int srbd_step_finish(srbd_ctx* ctx, const void* d_records, int32_t num_records, float* best_params, float* sigma,
                     srbd_result* out, float* out_costs_local);
/* Host-only merge of rank records (same math; no device needed). */
int srbd_finish_host(const srbd_config* cfg, const float* records, int32_t num_records, const float* state,
                     const float* contact, int32_t contact_stride, float* best_params, float* sigma,
                     srbd_result* out);
/* Host-only: build one rank record from a shard's saturated costs and noise rows (shard x P row-major). */
int srbd_make_record_host(const srbd_config* cfg, int32_t rank, int32_t world_size, const float* costs,
                          const float* noise_rows, float* record);

/*
 * Checkpoint / restore (exact golden replays of device-resident chains).  The state is what the next
 * device-resident step starts from: the warm start best_params (P floats), sigma (P floats, CEM
 * only; may be NULL otherwise) and the device RNG key (seed, counter).  After a host srbd_step it is
 * that step's inputs; every device-resident step (srbd_bench_device_steps, srbd_sharded_device_steps,
 * srbd_device_step_local/finish) advances it on the device.  Host steps are stateless here: their
 * state is their arguments (Sampling_MPC.get_state in the Python mirror).  Both calls block until the
 * context stream is idle and need one srbd_step first (it sets the state / reference inputs).
 */
int srbd_get_state(srbd_ctx* ctx, float* best_params, float* sigma, uint64_t* seed, uint64_t* counter);
int srbd_set_state(srbd_ctx* ctx, const float* best_params, const float* sigma, uint64_t seed, uint64_t counter);

/* Measurement: replay `steps` device-resident steps (RNG -> rollout -> reduction -> warm start
 * written back on device) back to back; returns elapsed ms (hipEvents on the context stream). */
int srbd_bench_device_steps(srbd_ctx* ctx, int32_t steps, float* elapsed_ms);
/* Measurement: `steps` srbd_step calls from C (srbd_step_sharded on a sharded context with a connected
 * xGMI / RCCL exchange), cycling through n_in input sets (state / ref: n_in x 24 floats, contact:
 * n_in x 4 x contact_stride), best (and sigma, CEM) fed back, counters counter0, counter0 + 1, ...;
 * lat_us[i] = wall time of call i (host-to-host at the C-ABI boundary, us). */
int srbd_bench_host_steps(srbd_ctx* ctx, const float* state, const float* ref, const float* contact,
                          int32_t contact_stride, int32_t n_in, float* best_params, float* sigma, uint64_t seed,
                          uint64_t counter0, int32_t steps, float* lat_us);
/* Average per-launch duration (us) of each kernel of one step: one hipEvent pair on the context
 * stream around `iters` back-to-back launches of that kernel (agrees with rocprofv3's kernel-trace
 * average).  fused_rollout_us: the rollout launch that also draws the next step's noise (the form
 * the step runs when fusion applies; 0 otherwise).  event_floor_us: the same measurement of an
 * empty kernel (launch-to-launch spacing).  Any out pointer may be NULL. */
int srbd_time_kernels(srbd_ctx* ctx, int32_t iters, float* rollout_us, float* rng_us, float* reduce_us,
                      float* fused_rollout_us, float* event_floor_us);

/* Measurement: average duration (us) of one kind of launch, `iters` back to back (one hipEvent pair), alone, so
 * a rocprofv3 pass over the call sees only it.  SRBD_TL_STEP_ROLLOUT is the rollout launch exactly as srbd_step
 * issues it (*form: 1 fused next-step draws | 2 step input by value | 4 in-launch final merge | 8 thread-per-sample
 * rollout kernel, else four lanes per sample | 16 fast_tail | 32 the launch makes the step's
 * draws itself: srbd_step then issues no RNG launch); SRBD_TL_STEP_MERGE
 * the merge launch srbd_step issues after it (0 when the rollout launch merges).  form may be NULL. */
enum { SRBD_TL_RNG = 0, SRBD_TL_ROLLOUT = 1, SRBD_TL_ROLLOUT_FUSED = 2, SRBD_TL_STEP_ROLLOUT = 3,
       SRBD_TL_STEP_MERGE = 4, SRBD_TL_EMPTY = 5 };
int srbd_time_launch(srbd_ctx* ctx, int32_t which, int32_t iters, float* us, int32_t* form);

/* Device-resident sharded chain (benchmark / pipelined callers): reuses the inputs of the last
 * srbd_step_local on the device.  srbd_device_step_local: RNG -> rollout -> rank record into d_record;
 * srbd_device_step_finish: merge -> outputs -> warm start (best/sigma/counter) written back on
 * device.  Both are asynchronous on the context stream. */
int srbd_device_step_local(srbd_ctx* ctx, void* d_record);
int srbd_device_step_finish(srbd_ctx* ctx, const void* d_records, int32_t num_records);
/* Block until the context stream is idle and copy the last step's outputs. */
int srbd_sync_result(srbd_ctx* ctx, float* best_params, float* sigma, srbd_result* out);
/* Test / diagnostic: the device draws a step keyed by (seed, counter) uses (the context's stream,
 * srbd_set_rng): this shard's rows of additional_random_parameters, n_local x P row-major (row 0 of the
 * problem is zero; CEM: the unscaled standard normals the step multiplies by sigma).  Blocks. */
int srbd_draw_noise(srbd_ctx* ctx, uint64_t seed, uint64_t counter, float* out_rows);
/* Saturated costs of this rank's rows from the last step (lazy materialisation). */
int srbd_copy_costs(srbd_ctx* ctx, float* out_costs);

/*
 * Sharded transport owned by the library (one process per GPU).  RCCL is loaded at run time from
 * `rccl_path` (the copy the process already uses, e.g. torch/lib/librccl.so) or /opt/rocm/lib.
 *   srbd_comm_get_unique_id : rank 0 makes the id (128 bytes); the caller broadcasts it
 *   srbd_comm_init          : every rank joins (rank / world_size from the context's config)
 *   srbd_step_sharded       : srbd_step_local + ncclAllGather of the rank records + srbd_step_finish
 *   srbd_sharded_device_steps: `steps` device-resident sharded steps, elapsed ms (hipEvents)
 */
int srbd_comm_get_unique_id(const char* rccl_path, uint8_t* id_out);
int srbd_comm_init(srbd_ctx* ctx, const char* rccl_path, const uint8_t* id_in);
int srbd_step_sharded(srbd_ctx* ctx, const float* state, const float* ref, const float* contact,
                      int32_t contact_stride, float* best_params, float* sigma, const float* noise_local,
                      uint64_t seed, uint64_t counter, srbd_result* out, float* out_costs_local);
int srbd_sharded_device_steps(srbd_ctx* ctx, int32_t steps, float* elapsed_ms);

/*
 * xGMI exchange (no collective launch): the merge kernel stores its rank record straight into
 * every rank's mailbox (uncached device memory, IPC-mapped over xGMI), sets per-rank epoch flags,
 * waits (bounded, 2 s) for the W records in its own mailbox and merges them in the same launch.
 * Once connected, srbd_step_sharded / srbd_sharded_device_steps use it instead of RCCL.
 *   srbd_xgmi_export        : allocate this rank's mailbox, 64-byte IPC handle out
 *   srbd_xgmi_connect       : world x 64 handle bytes in rank order (the caller all-gathers them)
 *   srbd_xgmi_connect_local : every rank's context in this process (index r = rank r)
 *   srbd_xgmi_probe         : one bounded round trip through the mailboxes (*ok = 1 on success)
 *   srbd_xgmi_disconnect    : back to RCCL (srbd_comm_init) for later steps
 */
int srbd_xgmi_export(srbd_ctx* ctx, uint8_t* handle_out);
int srbd_xgmi_connect(srbd_ctx* ctx, const uint8_t* handles);
int srbd_xgmi_connect_local(srbd_ctx* const* ctxs, int32_t world);
int srbd_xgmi_probe(srbd_ctx* ctx, int32_t* ok);
int srbd_xgmi_disconnect(srbd_ctx* ctx);

/* Diagnostic: mean duration (us) of the merge kernel's 5 phases (s_memrealtime stamps), then (staged merge)
 * the times from its start at which the records were in LDS and the tail prep was done, then the
 * shader clock in MHz over the kernel, then 16 finer marks (us from the start; 0 = unset): 24 floats for
 * block 0, then the same 24 for block 1 of a column-split merge (a slice block; zeros when unsplit): 48. */
int srbd_debug_merge_phases(srbd_ctx* ctx, int32_t iters, float* out_us);

/* Self-test of the correctly rounded division used in the rollout (a/b; b == 3 uses the constant
 * path).  Host results always; device results when out_dev != NULL (needs a GPU). */
int srbd_selftest_div(const float* a, const float* b, int32_t n, float* out_host, float* out_dev);
/* Self-test of the reference noise stream's log1p (jax.random.normal's erf_inv argument, NMPC:654/811/957): the
 * float of log1p(t) evaluated as float64 (t in (-1, 0]), on the host (out_host, with *nfallback = the arguments the
 * float64 log1p itself decided) and / or the device (out_dev).  Either output may be NULL. */
int srbd_selftest_log1p(const float* t, int32_t n, float* out_host, float* out_dev, int64_t* nfallback);

/* ------------------------------------------------------------------ TAMOLS */
typedef struct srbd_tamols_params {
    double gradient_delta;    /* 0.04 */
    double slope_threshold;   /* 0.7 */
    double w_edge, w_rough, w_dev, w_nominal, w_tracking, w_stability;
    double stability_margin;  /* 0.06 */
    double swing_time;        /* estimated_swing_time 0.25 */
    double h_des;             /* hip height */
    double l_min, l_max;      /* per-robot reach */
    double box_dx, box_dy;    /* constraint box */
    double stance_duration;   /* 0.3 (visual_foothold_adaptation.py:387) */
    double alphas[5];         /* np.linspace(0.2, 0.8, 5) (visual_foothold_adaptation.py:402) */
} srbd_tamols_params;

typedef struct srbd_tamols_ctx srbd_tamols_ctx;

int srbd_tamols_create(int32_t device_id, srbd_tamols_ctx** out);
void srbd_tamols_destroy(srbd_tamols_ctx* ctx);
const char* srbd_tamols_last_error(const srbd_tamols_ctx* ctx);
/*
 * heightmaps : 4 legs x rows x cols x 3 (x, y, z) doubles (HeightMap.data[:, :, 0, :])
 * seeds, hips: 4 x 3;  forward_vel: 3 or NULL;  base_pos: 3 or NULL;
 * contact    : 4 (1 stance, 0 swing) or NULL (-> all swing);  feet: 4 x 3 or NULL
 * outputs    : footholds 4x3, boxes 4x2x3, valid 4, scores 4 x rows*cols (or NULL),
 *              seed_heights 4 (nearest height + 0.02 at the seed, or NULL)
 */
int srbd_tamols_run(srbd_tamols_ctx* ctx, const double* heightmaps, int32_t rows, int32_t cols, const double* seeds,
                    const double* hips, const double* forward_vel, const double* base_pos, const int32_t* contact,
                    const double* feet, const srbd_tamols_params* params, double* out_footholds, double* out_boxes,
                    int32_t* out_valid, double* out_scores, double* out_seed_heights);

/* ------------------------------------------------------------------ terrain heightmap patches
 * GPU producer of the per-leg heightmap patches TAMOLS consumes: replaces
 * gym_quadruped's HeightMap.update_height_map (a MuJoCo mj_ray per patch point on the CPU; called at
 * quadruped_pympc/interfaces/wb_interface.py:233-234 with HeightMap(13, 7, 0.04, 0.04), simulation.py
 * :490-511).  The scene is uploaded once; every patch point casts a vertical ray down from ray_z and
 * takes the highest surface at or below ray_z: the ground plane, the top face of a box (yawed about
 * z) or of an upright cylinder, or a height field (cells split along the (i, j)-(i+1, j+1) diagonal).
 * A ray that hits nothing reports miss_z.  Patch point (i, j) of a patch centred at c with yaw psi:
 *   dx = (i - (rows - 1) / 2) * dist_x,  dy = (j - (cols - 1) / 2) * dist_y,
 *   x = c.x + cos(psi) dx - sin(psi) dy,  y = c.y + sin(psi) dx + cos(psi) dy   (float64).
 * gym_quadruped is absent here, so this layout is the one our PatchHeightMap uses (parity unpinned
 * against the real sensor; pinned against oracle/terrain_oracle.py bit for bit). */
enum { SRBD_PRIM_BOX = 0, SRBD_PRIM_CYLINDER = 1 };
typedef struct srbd_terrain_prim {
    int32_t type, pad;
    double cx, cy, cz; /* centre */
    double a, b, c;    /* box: half sizes x, y, z;  cylinder: radius, unused, half height */
    double yaw;        /* box rotation about z (radians) */
} srbd_terrain_prim;

typedef struct srbd_terrain srbd_terrain;

/* hfield: hf_nx x hf_ny heights, row-major [ix][iy], point (ix, iy) at (hf_x0 + ix hf_dx, hf_y0 + iy hf_dy);
 * NULL for none.  has_ground: a plane at ground_z. */
int srbd_terrain_create(int32_t device_id, const srbd_terrain_prim* prims, int32_t nprims, int32_t has_ground,
                        double ground_z, const double* hfield, int32_t hf_nx, int32_t hf_ny, double hf_x0,
                        double hf_y0, double hf_dx, double hf_dy, double miss_z, srbd_terrain** out);
void srbd_terrain_destroy(srbd_terrain* terrain);
const char* srbd_terrain_last_error(const srbd_terrain* terrain);
/* npatch patches (centres npatch x 3, yaws npatch) -> out npatch x rows x cols x 3 (x, y, z). */
int srbd_terrain_patches(srbd_terrain* terrain, const double* centers, const double* yaws, int32_t npatch,
                         int32_t rows, int32_t cols, double dist_x, double dist_y, double ray_z, double* out);
/* srbd_tamols_run with the four patches raycast on the device from `terrain` (centres = the seeds,
 * one yaw) in the same launch (the heightmap sensor fused into the search): no host round trip of the
 * patch.  out_heightmaps (4 x rows x cols x 3) and out_scores may be NULL (then only the footholds,
 * boxes, validity and seed heights cross PCIe). */
int srbd_tamols_run_terrain(srbd_tamols_ctx* ctx, srbd_terrain* terrain, double yaw, int32_t rows, int32_t cols,
                            double dist_x, double dist_y, double ray_z, const double* seeds, const double* hips,
                            const double* forward_vel, const double* base_pos, const int32_t* contact,
                            const double* feet, const srbd_tamols_params* params, double* out_footholds,
                            double* out_boxes, int32_t* out_valid, double* out_scores, double* out_seed_heights,
                            double* out_heightmaps);
/* ------------------------------------------------------------------ one C4 MPC step in one call
 * The per-MPC-step chain of helpers/foothold_pipeline.py TamolsMpcStep.step (wb_interface.py:230-291 +
 * srbd_controller_interface.py:113-180, MPPI / random sampling, one sampling iteration) behind one host call:
 * srbd_tamols_run_terrain on the patches around the seeds -> the adapted footholds (an infeasible leg: the seed at
 * its terrain height, VFA:223-228) as ref_foot_* after ref_base -> srbd_prepare_state -> srbd_step (device draws).
 * The same calls in the same order as the Python chain, so the same results bit for bit; the host work between
 * them is C instead of ~60 us of Python. */
typedef struct srbd_foothold_io {
    /* inputs */
    double state_in[24];        /* position, linear_velocity, orientation, angular_velocity, foot_FL..RR */
    double ref_base[12];        /* ref_position, ref_linear_velocity, ref_orientation, ref_angular_velocity */
    double seeds[12], hips[12]; /* reference footholds and hips, legs FL FR RL RR */
    double forward_vel[3];      /* TAMOLS forward velocity (the base linear velocity) */
    double current_contact[4], previous_contact[4];
    double yaw, dist_x, dist_y, ray_z;
    int32_t rows, cols;
    /* outputs */
    double footholds[12];       /* adapted ref_foot_* */
    double boxes[24];           /* constraint boxes (valid legs) */
    double seed_heights[4];
    int32_t valid[4];
    double state_out[24], ref_out[24]; /* prepare_state_and_reference's outputs */
    double* scores;             /* 4 x rows*cols, or NULL */
    double* heightmaps;         /* 4 x rows x cols x 3, or NULL */
    int32_t stage;              /* out: the calls that completed (0 none, 1 TAMOLS, 2 + prepare_state, 3 + step),
                                   so a caller can leave its objects as the chain would on an error */
    int32_t pad;
} srbd_foothold_io;

/* best_params (in/out, 4 x params_per_leg floats): the warm start; lift-off legs are zeroed before the step and the
 * step's result replaces it.  contact: 4 x contact_stride floats (the first `horizon` columns are used). */
int srbd_foothold_mpc_step(srbd_tamols_ctx* tamols, srbd_terrain* terrain, const srbd_tamols_params* params,
                           srbd_ctx* ctx, srbd_foothold_io* io, const float* contact, int32_t contact_stride,
                           float* best_params, int32_t params_per_leg, uint64_t seed, uint64_t counter,
                           srbd_result* out);

/* ------------------------------------------------------------------ one plugin-API MPC step in one call
 * SRBDControllerInterface.compute_control's sampling branch (srbd_controller_interface.py:113-180) over the plain
 * Sampling_MPC, behind one host call: prepare_state_and_reference (centroidal_nmpc_jax.py:563-627, no solution
 * shift: the caller keeps that case) -> per sampling iteration: with_newkey (:498-501) -> CEM's
 * with_newsigma(sigma_cem_mppi) at iteration 0 -> jitted_compute_control (srbd_step on device draws) -> the GRFs
 * times current_contact (SCI:175-178).  The same calls in the same order as the Python chain, so the same bits.
 * Key (in/out, advanced once per iteration as with_newkey + the step's key arguments do):
 *   SRBD_RNG_PHILOX   : key = (seed, counter); with_newkey: counter + 1; the step runs (seed, counter)
 *   SRBD_RNG_JAX[_LEGACY]: key[0] = the packed JAX key (key[0] << 32 | key[1]), key[1] = the controller's call
 *                       count; with_newkey: key = split(key)[0]; the step runs (packed key, call count + 1). */
typedef struct srbd_interface_io {
    /* inputs */
    double state_in[24];        /* position, linear_velocity, orientation, angular_velocity, foot_FL..RR */
    double ref_in[24];          /* ref_position .. ref_angular_velocity, ref_foot_FL..RR */
    double current_contact[4];  /* contact_sequence[:, 0] */
    double previous_contact[4]; /* the interface's previous_contact_mpc */
    double sigma_reset;         /* CEM: mpc_params['sigma_cem_mppi'] */
    uint64_t key[2];            /* in/out, see above */
    int32_t horizon, iterations, rng, cem; /* H, num_sampling_iterations, SRBD_RNG_*, method == CEM */
    /* outputs */
    double state_out[24], ref_out[24]; /* prepare_state_and_reference's outputs */
    double grf[12];             /* the last iteration's GRFs times current_contact (float64) */
    int32_t stage;              /* the calls that completed: 0 none, 1 prepare_state, 2 + i: iteration i's step */
    int32_t pad;
} srbd_interface_io;

/* contact / contact64: 4 x contact_stride float32 or float64 values (exactly one non-NULL; the first `horizon`
 * columns are used, float64 rounded to float32 as the step stages them).  best_params (in/out, 4 x params_per_leg):
 * the warm start (lift-off legs zeroed, then each iteration's result); sigma (in/out, CEM only, P floats).  `out`:
 * the last iteration's srbd_result. */
int srbd_interface_step(srbd_ctx* ctx, srbd_interface_io* io, const float* contact, const double* contact64,
                        int32_t contact_stride, float* best_params, int32_t params_per_leg, float* sigma,
                        srbd_result* out);

/* ------------------------------------------------------------------ batched environments
 * One context holding E environments of one configuration, and one host call that steps all of them: the
 * reference's replica mode (simulation/batched_simulations.py:40-58, SURVEY 3.4 and 8(e) "Replica mode") inside one
 * process, for evaluation sweeps, dataset generation (simulation/generate_dataset.py) and training loops.  A step
 * costs four launches whatever E is (input copy, draws or the transpose of injected noise, rollouts, merges) and
 * one host wait on one published word.  The device-resident step (srbd_batch_step_device below) takes and returns
 * device arrays on the caller's stream: five launches (pack, draws or transpose, rollouts, merges, unpack) and no
 * host wait.
 *   Shared: the srbd_config -- N (num_samples is per environment), H, method, parametrization, S, dts, sigmas, elite
 *   count.  Per environment: everything per step -- state, reference, contact sequence, warm start, noise key; and,
 *   opt-in (srbd_batch_set_env_params below), the robot, Q and the bounds: mass, mg, inertia, grf_min, grf_max, mu and
 *   q_diag.  Until they are set, every environment has the srbd_config's.
 *   Equivalence: environment e returns exactly what srbd_step returns on a context srbd_create(cfg) (world_size 1)
 *   for the same inputs, (seeds[e], counters[e]) and noise stream -- every output bit for bit (one fixed reduction
 *   tree, keyed by the environment's own rows 0..N-1).  Device draws of environment e are srbd_draw_noise(seeds[e],
 *   counters[e])'s; row 0 is zero.  Environments are independent: a NaN state or an all-swing contact sequence in
 *   one changes nothing in another.
 *   Range: 1 <= num_envs <= 4096, 1 <= N <= 16 384 (256 leaves of the reduction tree: what one merge block folds;
 *   beyond that one environment fills the GPU and separate contexts lose nothing).
 *   Supported: MPPI and random sampling; the three parametrizations at any H and S srbd_create takes; the Philox
 *   and both JAX streams; injected noise.
 *   SRBD_E_INVALID (with a message saying which and why): a larger N or num_envs, CEM-MPPI (sigma is part of every
 *   CEM step: srbd_batch_create_cem and the _cem step calls below), rank / world_size other than 0 / 1.  use_graph
 *   is ignored.  Gait-adaptive sampling and the opt-in cost terms have batch forms
 *   (srbd_batch_set_gait, srbd_batch_set_cost_terms below), but not both at once.  There are no batch forms of
 *   armed steps or the single context's device-resident chains (srbd_device_step_local and its kin); the batch's
 *   device-resident form is srbd_batch_step_device.  A failed allocation: SRBD_E_NOMEM; no device: SRBD_E_NODEVICE.
 *   A call that returns an error has changed nothing in best_params.  A step whose launches end without publishing
 *   returns SRBD_E_HIP, leaves the arrival count zero and the next step exact. */
typedef struct srbd_batch srbd_batch;
int srbd_batch_create(const srbd_config* cfg, int32_t num_envs, srbd_batch** out);
void srbd_batch_destroy(srbd_batch* b);
/* Last error of b, or of the calling thread's last failed srbd_batch_create when b == NULL. */
const char* srbd_batch_last_error(const srbd_batch* b);
int srbd_batch_num_envs(const srbd_batch* b);
/* SRBD_RNG_* (srbd_set_rng); default SRBD_RNG_PHILOX. */
int srbd_batch_set_rng(srbd_batch* b, int32_t kind);
/*   states, refs  : E x 24
 *   contacts      : E x 4 x contact_stride; the first H columns are used
 *   best_params   : E x P, in: warm starts, out: updated
 *   noise         : NULL -> device draws; else E x N x P row-major, row 0 of each environment zero
 *   seeds, counters : E each
 *   out           : E results
 *   out_costs     : E x N saturated costs, or NULL */
int srbd_batch_step(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                    int32_t contact_stride, float* best_params, const float* noise, const uint64_t* seeds,
                    const uint64_t* counters, srbd_result* out, float* out_costs);
/* E x N saturated costs of the last step. */
int srbd_batch_copy_costs(srbd_batch* b, float* out_costs);
/* Gait-adaptive sampling and the opt-in cost terms in a batch: srbd_set_gait, srbd_clear_gait and srbd_set_cost_terms
 * with every per-step value per environment and every configuration value shared.  A setting applies to every
 * following srbd_batch_step until changed.
 *   timings       : E x 4 leg phases
 *   freq_sets     : E x n_freq candidate step frequencies (random sampling's set depends on each environment's
 *                   optimize_swing); n_freq, pgg_dt and duty_factor are shared
 *   freq_rows     : NULL -> every sample draws its frequency on the device from its environment's set, keyed by
 *                   (seeds[e], counters[e]) as srbd_step keys it; else E x N injected frequencies
 *   r_force, w_smooth, w_cone : shared; all zero turns the terms off (the plain kernel again)
 *   Equivalence: environment e returns exactly what srbd_step returns on a context that received
 *   srbd_set_gait(timing_e, pgg_dt, duty_factor, freq_set_e, n_freq, freq_rows_e), or srbd_set_cost_terms(r_force,
 *   w_smooth, w_cone), for the same inputs -- every output bit for bit, srbd_result::best_freq included (the best
 *   row's frequency; 0 after srbd_batch_clear_gait).
 *   SRBD_E_INVALID (with a message): null arguments, n_freq outside 1..SRBD_MAX_FREQS, num_splines + 1 > 33 for
 *   the spline parametrizations, weights negative or not finite, and gait-adaptive sampling together with non-zero
 *   weights (one context runs that combination on its thread-per-sample kernel; it has no batch form): whichever
 *   call would make both active fails and changes nothing.  A failed allocation of the frequency array:
 *   SRBD_E_NOMEM. */
int srbd_batch_set_gait(srbd_batch* b, const float* timings, float pgg_dt, float duty_factor, const float* freq_sets,
                        int32_t n_freq, const float* freq_rows);
int srbd_batch_clear_gait(srbd_batch* b);
int srbd_batch_set_cost_terms(srbd_batch* b, const float r_force[3], float w_smooth, float w_cone);
/* The device-resident step: srbd_batch_step with every array in device memory, enqueued on the caller's stream.
 *   Every pointer is device memory of the batch's device; the layouts are srbd_batch_step's.  costs may be NULL,
 *   noise NULL selects device draws; every other pointer is required.  Arrays must not overlap.
 *   Enqueue contract: hip_stream == NULL selects the batch's own stream; the null (legacy default) stream is
 *   selected by its explicit handle hipStreamLegacy, (hipStream_t)1.  The call enqueues five launches (pack:
 *   the step inputs built on the device as srbd_batch_step builds them on the host; draws, or the transpose reading
 *   io->noise in place; rollouts; merges; unpack: the outputs scattered to the caller's arrays) and returns.  It
 *   makes no synchronising HIP call, does not wait on the published word and touches no device memory from the
 *   host.  The outputs are ready when the work enqueued on the stream so far has completed: synchronise the stream,
 *   or enqueue the consumers on it.  The input arrays are read, and best_params rewritten, in stream order, so
 *   they may be produced by earlier work on that stream and reused by later work on it.
 *   Equivalence: for the same inputs, keys, noise stream and settings (srbd_batch_set_rng, _set_gait, _clear_gait,
 *   _set_cost_terms) every output array holds exactly the bytes srbd_batch_step returns in best_params, srbd_result
 *   and out_costs -- status and best_freq included.
 *   Ordering: the batch's internal buffers are shared with the host path.  Every device step records an event
 *   behind its last launch; srbd_batch_step makes its stream wait on it, srbd_batch_copy_costs, _set_gait,
 *   _clear_gait, _set_cost_terms and _destroy synchronise on it, and a device step on a different stream than the
 *   previous one makes that stream wait on it.  So the entry points may be mixed freely from one host thread;
 *   srbd_batch_copy_costs after a device step returns that step's costs.  The arrays of a step still in flight
 *   must stay allocated until it has completed.
 *   SRBD_E_INVALID (with a message, before anything is enqueued): b or io NULL, a required pointer NULL,
 *   contact_stride < H.  Capturing the call into a HIP graph is not supported. */
typedef struct srbd_batch_device_io {
    /* inputs, float32 unless noted */
    const float* states;       /* E x 24 */
    const float* refs;         /* E x 24 */
    const float* contacts;     /* E x 4 x contact_stride; the first H columns are used */
    const float* noise;        /* NULL -> device draws; else E x N x P row-major, row 0 of each environment zero */
    const uint64_t* seeds;     /* E */
    const uint64_t* counters;  /* E */
    int32_t contact_stride, pad;
    /* in / out */
    float* best_params;        /* E x P: warm starts in, updated out */
    /* outputs */
    float* grf;                /* E x 12 */
    float* predicted_state;    /* E x 24 */
    float* best_cost;          /* E */
    int32_t* best_index;       /* E */
    float* best_freq;          /* E */
    int32_t* status;           /* E */
    float* costs;              /* E x N saturated costs, or NULL */
} srbd_batch_device_io;
int srbd_batch_step_device(srbd_batch* b, const srbd_batch_device_io* io, void* hip_stream);

/* Batched CEM-MPPI.  CEM's sigma is part of every step (in: the spread the draws are scaled by; out: the elite rows'
 * clipped standard deviation, centroidal_nmpc_jax.py:1075-1081), so a CEM batch has a creator and step calls of its
 * own; srbd_batch_create keeps refusing SRBD_CEM_MPPI.
 *   srbd_batch_create_cem: srbd_batch_create's ranges (1 <= num_envs <= 4096, N <= 16 384, rank / world_size 0 / 1)
 *   with method == SRBD_CEM_MPPI and 2 <= num_elite <= SRBD_MAX_ELITE as srbd_create requires (0 selects 10).  Any
 *   other method, and every violation, returns SRBD_E_INVALID with a message, before any HIP call.
 *   srbd_batch_step_cem: srbd_batch_step with sigma, E x P, in / out.  Injected noise is used as given (it is not
 *   multiplied by sigma, as srbd_step treats it); device draws are the unscaled srbd_draw_noise rows, multiplied by
 *   sigma[e] where they are read.
 *   srbd_batch_step_cem_device: srbd_batch_step_device with cem->sigma, E x P device memory of the batch's device
 *   (it must not overlap the other arrays).  sigma_reset > 0: every environment starts this step from that constant
 *   and sigma is only written -- the reference's with_newsigma(sigma_cem_mppi) at the first sampling iteration of a
 *   control step (srbd_controller_interface.py:128-129), at no extra launch.  sigma_reset == 0: sigma is read and
 *   rewritten.  The enqueue contract, the stream handle, the ordering rule and the five launches are
 *   srbd_batch_step_device's; the call makes no synchronising HIP call.  Capturing it into a HIP graph is not
 *   supported.
 *   Equivalence: environment e returns exactly what srbd_step returns on a context srbd_create(cfg) for the same
 *   inputs, sigma[e], (seeds[e], counters[e]) and noise stream -- every output bit for bit, the new sigma included
 *   (the merge block folds the one fixed reduction tree with every column in one block, where one context splits
 *   the columns over blocks: the same sums in the same order).  The device form returns the host form's bytes.
 *   Settings: srbd_batch_set_rng as for any batch.  srbd_batch_set_cost_terms works on a CEM batch (one context runs
 *   CEM with the opt-in cost terms on its four-lane kernel, and the batch restates that form); environment e then
 *   equals a context that received srbd_set_cost_terms.  srbd_batch_set_gait and srbd_batch_set_gait_device return
 *   SRBD_E_INVALID on a CEM batch, as srbd_set_gait does on a CEM context.
 *   Mixing: srbd_batch_step / srbd_batch_step_device on a CEM batch, and the _cem steps on a batch made by
 *   srbd_batch_create, return SRBD_E_INVALID and change nothing.  srbd_batch_copy_costs serves both kinds.
 *   SRBD_E_INVALID besides (before anything is enqueued): b, io or cem NULL, a required pointer NULL (sigma among
 *   them, also with sigma_reset > 0: it is written), contact_stride < H, sigma_reset negative or not finite. */
typedef struct srbd_batch_cem_io {
    float* sigma;        /* E x P, in / out (sigma_reset > 0: out only) */
    float sigma_reset;   /* > 0: the step starts from this constant; 0: from sigma */
    int32_t pad;
} srbd_batch_cem_io;
int srbd_batch_create_cem(const srbd_config* cfg, int32_t num_envs, srbd_batch** out);
int srbd_batch_step_cem(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                        int32_t contact_stride, float* best_params, float* sigma, const float* noise,
                        const uint64_t* seeds, const uint64_t* counters, srbd_result* out, float* out_costs);
int srbd_batch_step_cem_device(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem,
                               void* hip_stream);

/* Per-environment robot and cost parameters: the seven srbd_config fields of the same names, one record per
 * environment (payload, friction, inertia, force-limit and cost-weight sweeps inside one batch).
 *   A setting holds for every following step until changed or cleared, and applies to every step entry point:
 *   srbd_batch_step, _step_device, _step_cem, _step_cem_device, and those steps after srbd_batch_set_gait[_device] or
 *   srbd_batch_set_cost_terms.  Everything else in the srbd_config stays shared (N, H, method, parametrization, S,
 *   dts, sigmas, elite count).  Before the first set, and after srbd_batch_clear_env_params, the batch behaves and
 *   launches exactly as a batch without parameters: the same kernels with the same arguments.
 *   Equivalence: environment e returns exactly what srbd_step returns on srbd_create(cfg_e), cfg_e being the batch's
 *   srbd_config with mass, mg, grf_min, grf_max, mu, inertia and q_diag replaced by params[e], for the same inputs,
 *   keys, noise stream and srbd_set_gait / srbd_set_cost_terms / sigma -- every output bit for bit: costs,
 *   best_params, the new sigma, GRFs, predicted state, best_cost, best_index, best_freq, status.  The values derived
 *   from a record (1 / mass, -mu, the inverse inertia, mg / n_stance) are formed by the one function srbd_create's
 *   model uses, on the host and on the device.
 *   srbd_batch_set_env_params: params, E records in host memory; mask NULL, or E bytes: environments with mask[e] == 0
 *   keep their parameters and their records are not read.  Every selected record is checked as srbd_create checks its
 *   configuration (0 <= grf_min <= grf_max, mu >= 0): at the first that fails the call returns SRBD_E_INVALID, names
 *   that environment in srbd_batch_last_error and changes nothing.  Synchronises as srbd_batch_set_cost_terms does.
 *   srbd_batch_set_env_params_device: the same from device memory of the batch's device, one launch on the caller's
 *   stream (hip_stream as srbd_batch_step_device reads it), no host wait and no host access to device memory; it
 *   joins the device steps' event protocol as srbd_batch_set_gait_device does.  d_mask NULL, or E int32 words (the
 *   mask of srbd_loop_reset_device: an episode reset re-draws its robots with it); a masked-out record is neither
 *   read nor written.  The call cannot return a per-environment error: a selected environment whose record fails the
 *   checks keeps its previous parameters and gets d_rejected[e] = 1; every other environment gets 0, masked-out ones
 *   included (d_rejected NULL: not reported).  After this call every step runs the per-environment kernels until
 *   srbd_batch_clear_env_params.
 *   srbd_batch_get_env_params: synchronises on the batch's event and returns every environment's seven fields as set,
 *   or the srbd_config's where never set.
 *   srbd_batch_clear_env_params: every environment back to the srbd_config's values; synchronises.
 *   SRBD_E_INVALID (with a message, before anything is enqueued): b, params, d_params or out NULL; d_params, d_mask
 *   or d_rejected not 4-byte aligned.  A failed allocation of the record array: SRBD_E_NOMEM.
 *   Refusal rule: a step never runs an environment that was given parameters on the shared values; a form without
 *   per-environment kernels would return SRBD_E_INVALID with a message instead (there is none: every batch step form
 *   has them). */
typedef struct srbd_env_params { /* 39 floats, no padding; the srbd_config fields of the same names */
    float mass, mg, grf_min, grf_max, mu;
    float inertia[9];
    float q_diag[24];
    float reserved; /* the 39th float: not read by the setters' checks or the model; returned as given (0 by default) */
} srbd_env_params;
int srbd_batch_set_env_params(srbd_batch* b, const srbd_env_params* params, const uint8_t* mask);
int srbd_batch_set_env_params_device(srbd_batch* b, const srbd_env_params* d_params, const int32_t* d_mask,
                                     int32_t* d_rejected, void* hip_stream);
int srbd_batch_get_env_params(srbd_batch* b, srbd_env_params* out);
int srbd_batch_clear_env_params(srbd_batch* b);

/* The full-horizon plan of one parameter row per environment: the trajectory a step's rollout computes for a row and
 * drops -- every step form returns the first knot alone (grf, predicted_state), as the reference's compute_control
 * does.  Reference lines restated: compute_rollout, centroidal_nmpc_jax.py:316-496 (caller-given contacts) and
 * centroidal_nmpc_jax_gait_adaptive.py:326-501 (gait-adaptive sampling: the sample's own contact sequence from its
 * step frequency, the per-leg stance counter, horizon_leg = stance steps + 1 and the negative-index wrap), with the
 * saturation of :686-687.
 *   One launch for all E environments on the caller's stream (plan_kernel, one thread per environment): params[e] is
 *   decoded, shaped and integrated over the H steps from states[e] and refs[e], with the batch's current settings --
 *   srbd_batch_set_gait[_device] (the contact flags then come from environment e's leg phases and freqs[e], the step's
 *   best_freq output or any frequency of the set; contacts is not read), srbd_batch_set_cost_terms (the terms are
 *   part of the costs) and srbd_batch_set_env_params (environment e's robot).  A CEM batch is served the same way:
 *   only params matter.
 *   states, refs : the rows the step rolled out from (prepared rows, as the step takes them).
 *   Outputs, float32, any of them NULL when not wanted (at least one is not):
 *     plan_states   E x H x 12  the 12 evolving states after step n (the feet are constant: states[e][12..23])
 *     plan_grfs     E x H x 12  the forces of step n after the contact mask and the clip
 *     plan_contacts E x 4 x H   the contact flags used (with gait-adaptive sampling the only place they are visible)
 *     plan_run_cost E x H       (cost_x + cost_y) + cost_z accumulated up to and including step n
 *     plan_cost     E           the row's cost: the last running cost + the feet term (+ (f - 1.3) 100 (f - 1.3) with
 *                               gait-adaptive sampling), saturated to 1 000 000 when not finite
 *   Equivalence: with params[e] = the step's warm start + its noise row r (for CEM as the step scales it) and, with
 *   gait-adaptive sampling, freqs[e] = row r's frequency, plan_cost[e] is the step's costs[e][r] bit for bit: the
 *   launch runs the functions the rollouts run, in their order, unfused.  With params = the step's new best_params,
 *   plan_states[e][0] and plan_grfs[e][0] are predicted_state[e][0..11] and grf[e] -- bit for bit for the zero-order
 *   parametrization; the splines' final decode evaluates step 0.0 with horizon_leg 1 (NMPC:706-710), the plan step 0
 *   of H, the same value up to rounding; with gait-adaptive sampling only where the caller's contact column 0 equals
 *   the sample's (the final GRFs use the caller's sequence, GA:720-796).  Environment e of the batch form equals
 *   srbd_plan on a context created with e's configuration and settings, and srbd_batch_plan returns the device form's
 *   bytes.
 *   srbd_batch_plan_device: every pointer device memory of the batch's device, arrays must not overlap.  hip_stream as
 *   srbd_batch_step_device reads it; the call makes no synchronising HIP call and no host copy, and follows that
 *   call's ordering rule (it waits on, then records, the batch's event), so enqueued behind a step on any stream it
 *   reads that step's outputs, and a later step is not disturbed.  Capturing the call into a HIP graph is not
 *   supported.
 *   srbd_batch_plan: the same arrays in host memory: upload, the launch, one wait, download.
 *   srbd_plan: the single-context form, the same kernel at E = 1 with the context's settings (srbd_set_gait: freq is
 *   read and contact is not; srbd_set_cost_terms, also together with srbd_set_gait); it synchronises the context's
 *   stream.  A sharded context (world_size > 1) is refused.
 *   SRBD_E_INVALID (with a message, before anything is enqueued): b, c or io NULL, a required pointer NULL (states,
 *   refs, params; contacts without gait-adaptive sampling; freqs with it), every output NULL, contact_stride < H.
 *   Out of scope: the plan from inside the step's launch, plans of rows the caller does not pass, the sharded step,
 *   graph capture, and a batch with gait-adaptive sampling and cost terms at once (the batch refuses that combination
 *   itself; srbd_plan on one context runs it). */
typedef struct srbd_batch_plan_io {
    const float* states;      /* E x 24: the rows the step rolled out from (prepared) */
    const float* refs;        /* E x 24 */
    const float* contacts;    /* E x 4 x contact_stride; ignored with gait-adaptive sampling */
    const float* params;      /* E x P: any parameter rows, e.g. the step's new best_params */
    const float* freqs;       /* E: required when gait fields are set, else ignored */
    int32_t contact_stride, pad;
    float* plan_states;       /* E x H x 12, or NULL */
    float* plan_grfs;         /* E x H x 12, or NULL */
    float* plan_contacts;     /* E x 4 x H, or NULL */
    float* plan_run_cost;     /* E x H, or NULL */
    float* plan_cost;         /* E, or NULL */
} srbd_batch_plan_io;
int srbd_batch_plan_device(srbd_batch* b, const srbd_batch_plan_io* io, void* hip_stream);
int srbd_batch_plan(srbd_batch* b, const float* states, const float* refs, const float* contacts,
                    int32_t contact_stride, const float* params, const float* freqs, float* plan_states,
                    float* plan_grfs, float* plan_contacts, float* plan_run_cost, float* plan_cost);
int srbd_plan(srbd_ctx* c, const float* state, const float* ref, const float* contact, int32_t contact_stride,
              const float* params, float freq, float* plan_states, float* plan_grfs, float* plan_contacts,
              float* plan_run_cost, float* plan_cost);

/* The producers of the device-resident step on the device: the periodic gait generator and
 * prepare_state_and_reference (srbd_host.h: srbd_pgg_run, srbd_pgg_contact_sequence, srbd_prepare_state) for
 * num_envs environments per call, so that generator.run -> contact sequence -> prepare -> srbd_batch_step_device
 * never leaves the GPU.  Reference lines restated per environment (paths as in srbd_host.h):
 *   srbd_pgg_run_device              <- PeriodicGaitGenerator.run                       periodic_gait_generator.py:48-76
 *   srbd_pgg_contact_sequence_device <- PeriodicGaitGenerator.compute_contact_sequence  :93-118
 *   srbd_prepare_state_device        <- Sampling_MPC.prepare_state_and_reference        centroidal_nmpc_jax.py:563-627
 *   Generator state: d_pgg is an array of num_envs srbd_pgg structs (srbd_host.h, unchanged plain data) in device
 *   memory.  The caller initialises them on the host with srbd_pgg_init, uploads them, and may download and inspect
 *   them at any time.
 *   srbd_pgg_run_device: every environment's phases advanced by dt * d_step_freqs[e] (d_step_freqs NULL: by dt * its
 *   own step_freq field), the start-up hold (init) honoured against phase_offset and cleared on release, the state
 *   written back, and the contact flags written as float32 1.0 / 0.0 to d_contact_out (num_envs x 4).
 *   srbd_pgg_contact_sequence_device: the run(0) column, then horizon - 1 run(dts[j]) steps with j advanced by lens
 *   (dts[j] holds for the steps i < lens[j]), written to d_contacts[e][leg][0 .. horizon) of a num_envs x 4 x
 *   contact_stride array -- the layout srbd_batch_step_device reads; the columns at and beyond horizon are not
 *   written.  The `horizon` argument is used; the structs' horizon field is not read.  The state is left as found,
 *   except in a SRBD_GAIT_FULL_STANCE environment, which gets ones in its horizon columns and its generator reset, as
 *   the host does (the step reads only `horizon` columns, so the host's 2 x horizon is not reproduced).  dts and lens
 *   are host arrays of n_dts entries shared by all environments; they are checked on the host and travel in the
 *   kernel arguments.
 *   srbd_prepare_state_device: d_state_in, d_ref_in num_envs x 24 float64 (srbd_prepare_state's layouts),
 *   d_current_contact, d_previous_contact num_envs x 4 float32; d_states, d_refs num_envs x 24 float32.  Swing feet
 *   (current 0) take the reference foot; a leg lifting off (previous 1, current 0) zeroes its params_per_leg entries
 *   of d_best_params[e] (num_envs x num_params float32, in place; may be NULL).
 *   Equivalence: for environment e the device state after any sequence of these calls holds the bytes of a host
 *   srbd_pgg that received the same calls, and the outputs are the host functions' float64 values cast to float32:
 *   exact for the contact flags, and for states and refs the cast the host step makes when it stages them.  The
 *   arithmetic is float64 in the order of the host functions, unfused.
 *   Enqueue contract: each call enqueues exactly one launch on hip_stream and returns; it makes no synchronising HIP
 *   call and touches no device memory from the host.  The stream handle is read as srbd_batch_step_device reads it,
 *   except that NULL also selects the legacy null stream (there is no batch here to own a stream).  The pointers
 *   are memory of the current device.  None of a batch's internal buffers are used, so the calls need no event and
 *   do not enter the ordering rule above: order them against a step as any work on a stream.
 *   SRBD_E_INVALID (before any HIP call): a NULL required pointer; num_envs outside 1..4096; horizon outside
 *   1..SRBD_MAX_HORIZON; contact_stride < horizon; n_dts outside 1..32; lens that would run past n_dts before step
 *   horizon - 1 (where the reference raises IndexError); params_per_leg < 1 or 4 * params_per_leg > num_params when
 *   d_best_params is given.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
struct srbd_pgg;
int srbd_pgg_run_device(struct srbd_pgg* d_pgg, int32_t num_envs, double dt,
                        const double* d_step_freqs /* E, or NULL: each entry's own step_freq */,
                        float* d_contact_out /* E x 4 */, void* hip_stream);
int srbd_pgg_contact_sequence_device(struct srbd_pgg* d_pgg, int32_t num_envs, int32_t horizon, const double* dts,
                                     const int32_t* lens, int32_t n_dts /* host arrays */, float* d_contacts,
                                     int32_t contact_stride, void* hip_stream);
int srbd_prepare_state_device(int32_t num_envs, const double* d_state_in, const double* d_ref_in,
                              const float* d_current_contact, const float* d_previous_contact, int32_t params_per_leg,
                              int32_t num_params, float* d_best_params /* or NULL */, float* d_states, float* d_refs,
                              void* hip_stream);

/* The foothold search of the device-resident loop: TAMOLS (srbd_tamols_run / srbd_tamols_run_terrain above, i.e.
 * VisualFootholdAdaptation.compute_adaptation, strategy 'tamols', visual_foothold_adaptation.py:153-231 with its
 * helpers :261-714, and the heightmap raycast of wb_interface.py:233-234) for num_envs environments in one launch,
 * device in and device out, so that generator.run -> footholds -> prepare -> srbd_batch_step_device never leaves
 * the GPU.  Stateless: no context, no allocation.
 *   Forms: terrain != NULL raycasts every leg's rows x cols patch from the one scene all environments share (one
 *   scene per environment: srbd_tamols_batch_scenes_device, below), centred at the leg's seed and yawed by yaws[e] (what srbd_tamols_run_terrain does per call); terrain == NULL reads the
 *   caller's patches from `heightmaps` (what srbd_tamols_run does).  params, rows, cols, the spacings and ray_z are
 *   shared by the environments; NULL forward_vel / base_pos / contact / feet mean what they mean in srbd_tamols_run,
 *   for every environment.  contact is float32 as srbd_pgg_run_device writes it (stance iff 1.0f).
 *   Outputs per environment as srbd_tamols_run's; an infeasible leg (valid 0, NaN box) returns the seed at its
 *   terrain height (VFA:223-228).  ref, when given, is srbd_prepare_state_device's d_ref_in: entries 12..23 of row e
 *   (ref_foot_FL..RR) receive environment e's footholds, entries 0..11 are not written.
 *   Equivalence: for environment e every output holds the bytes the single-environment call returns for that
 *   environment's inputs (NaNs position for position); the kernel runs the single kernel's device functions, float64
 *   in the same order.  Environments are independent.  One caveat, terrain form: the single call forms cos / sin of
 *   its yaw with the host's libm, this call on the device, correctly rounded (csrc/yaw_sincos.h;
 *   srbd_selftest_yaw_sincos is its host twin).  For a yaw where libm's value is not the correctly rounded one
 *   (glibc 2.35: about 3 in 1000 yaws, by one ulp) the patch coordinates, and with them the footholds, differ in
 *   the last place.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it; every pointer is
 *   memory of the current device, which must be the terrain's; no event and no ordering rule.  The terrain must
 *   outlive the launch.
 *   SRBD_E_INVALID (before any HIP call): a NULL params, io or required pointer (seeds, hips, footholds, boxes,
 *   valid); num_envs outside 1..4096; rows or cols below 1 or rows * cols above 320; terrain form without yaws or with
 *   a dist_x or dist_y that is not positive (the lattice patch, the only one the plugin API produces); patch form
 *   without heightmaps; heightmaps_out in patch form.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device
 *   exists. */
typedef struct srbd_tamols_batch_io {
    /* inputs: device memory, float64 unless noted; E = num_envs */
    const double* seeds;        /* E x 4 x 3 */
    const double* hips;         /* E x 4 x 3 */
    const double* forward_vel;  /* E x 3, or NULL */
    const double* base_pos;     /* E x 3, or NULL */
    const float* contact;       /* E x 4 float32: stance iff == 1.0f; NULL -> all swing */
    const double* feet;         /* E x 4 x 3, or NULL */
    const double* yaws;         /* E: terrain form only */
    const double* heightmaps;   /* E x 4 x rows x cols x 3: patch form only (terrain == NULL) */
    int32_t rows, cols;
    double dist_x, dist_y, ray_z; /* terrain form */
    /* outputs: device memory */
    double* footholds;          /* E x 4 x 3 */
    double* boxes;              /* E x 4 x 2 x 3; NaN for an infeasible leg */
    int32_t* valid;             /* E x 4 */
    double* seed_heights;       /* E x 4, or NULL */
    double* scores;             /* E x 4 x rows*cols, or NULL */
    double* heightmaps_out;     /* E x 4 x rows x cols x 3, terrain form, or NULL */
    double* ref;                /* E x 24 or NULL: entries 12..23 of row e receive environment e's footholds */
} srbd_tamols_batch_io;
int srbd_tamols_batch_device(srbd_terrain* terrain /* NULL: patch form */, const srbd_tamols_params* params,
                             int32_t num_envs, const srbd_tamols_batch_io* io, void* hip_stream);
/* The same search behind the reference's apex gate (wb_interface.py:230-246 with VisualFootholdAdaptation's state,
 * visual_foothold_adaptation.py:59-72): an environment searches once per swing, at the apex, holds that foothold until
 * the next full stance and passes its seeds through from there to the next apex -- where srbd_tamols_batch_device
 * searches every leg of every environment on every call.  srbd_host.h (srbd_vfa, srbd_vfa_mode, srbd_vfa_commit) and
 * csrc/srbd_vfa.h state the machine; this is its device form.
 *   State: d_vfa is an array of num_envs srbd_vfa structs in device memory (initialise on the host with srbd_vfa_init
 *   and upload; the caller may download and inspect them); d_stc the num_envs srbd_stc structs srbd_stc_step_device
 *   advances, read only here.  The gate reads the swing clocks as the last srbd_stc_step_device left them, so within
 *   a control step this call comes before that one (the reference checks the apex before update_swing_time).
 *   io is srbd_tamols_batch_device's, every field with its meaning there, except: io->contact is required (float32 as
 *   srbd_pgg_run_device writes it; the gate's swing legs are those == 0.0f, the search's stance legs those == 1.0f);
 *   footholds, boxes, valid and ref's entries 12..23 receive what get_footholds_adapted returns (the search's result,
 *   the held footholds, or the seeds; the box of a leg whose last search was infeasible is its older one, see
 *   srbd_host.h); seed_heights, scores and heightmaps_out are written for searching environments only, other
 *   environments' rows are left untouched.  d_mode, when given, receives SRBD_VFA_SEARCH / _HOLD / _PASS per environment.
 *   Launch shape: srbd_tamols_batch_device's grid (4 legs x num_envs) and block.  Block (leg, e) forms the mode itself
 *   from d_stc[e], io->contact[e] and its own word d_vfa[e].initialized[leg] -- the word is replicated per leg for
 *   this, nothing crosses blocks; one wave reads it, once, before any lane of the block writes it -- and branches
 *   before the patch stage: a HOLD or PASS block copies its leg's ten
 *   values and leaves; a SEARCH block runs the ungated kernel's stages through the same device functions.
 *   Equivalence: for environment e the call does, on a host srbd_vfa with d_vfa[e]'s bytes, srbd_vfa_mode (contacts
 *   widened to double); then, when the mode is SEARCH, what srbd_tamols_batch_device returns for that environment's
 *   inputs; then srbd_vfa_commit.  Afterwards d_vfa[e] holds the host struct's bytes, every output row the host's
 *   values bit for bit (NaNs position for position), d_mode[e] the mode.  Environments are independent: a NaN seed or
 *   yaw in one changes nothing in another, and a non-searching environment reads neither its yaw, hips, patch nor the
 *   terrain.  A d_vfa[e] whose four initialized words differ (which no call here produces) is not refused on the
 *   device: each leg follows its own word.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it; no event and no
 *   ordering rule; d_stc is read only.
 *   SRBD_E_INVALID (before any HIP call): everything srbd_tamols_batch_device refuses; a NULL d_vfa, d_stc or
 *   io->contact; an apex_interval that is not finite.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device
 *   exists.
 *   The 'height' strategy behind the same gate is srbd_vfa_height_step_device, below.
 *   Out of scope: the 'vfa' strategy; the early-stance detector and inverse kinematics (start-and-stop
 *   is the gait generator's: srbd_pgg_start_stop_device and srbd_wb_update_device, below);
 *   compacting the searching environments into a smaller grid (their count would have to reach the host).  The
 *   per-environment masked reset of d_vfa and the loop's other device state is srbd_loop_reset_device, below. */
struct srbd_vfa;
struct srbd_stc;
int srbd_vfa_step_device(struct srbd_vfa* d_vfa, const struct srbd_stc* d_stc, srbd_terrain* terrain /* NULL: patch form */,
                         const srbd_tamols_params* params, int32_t num_envs, const srbd_tamols_batch_io* io,
                         double apex_interval, int32_t* d_mode /* E, or NULL */, void* hip_stream);
/* One terrain scene per environment: a device-resident set of scenes and the two calls above reading, per environment,
 * an index into it -- so one batch can sweep the ground as srbd_batch_set_env_params lets it sweep the robot, and an
 * environment can move to another scene at reset, in one launch and with nothing on the host knowing which
 * environment stands on which scene.
 *   srbd_terrain_scene holds srbd_terrain_create's arguments of one scene (80 bytes, no padding).
 *   srbd_terrain_set_create takes 1..4096 scenes and checks each as srbd_terrain_create checks its arguments; the
 *   first scene that fails returns SRBD_E_INVALID with its index in the message, before any HIP call, and so do
 *   scenes whose primitives or height-field points together number more than 2^31 - 1, a NULL scenes or out and a
 *   num_scenes outside 1..4096.  On the device the set holds the scenes' primitives concatenated, their box-yaw
 *   cos / sin pairs concatenated (formed by the function srbd_terrain_create forms them with: a scene in a set and the
 *   same scene alone hold the same bits), the height fields concatenated, and a table of one record per scene
 *   pointing into those arrays.  The host arrays are not kept.  The set is immutable after creation.  No device:
 *   SRBD_E_NODEVICE; a failed allocation: SRBD_E_NOMEM; another failed HIP call: SRBD_E_HIP.
 *   srbd_terrain_set_last_error: the set's last message; NULL: the calling thread's last failed create, or its last
 *   call below refused for a NULL set.  Two conventions meet on this handle: the two searches here store an argument
 *   refusal on the set, so they follow the handle to refuse; srbd_terrain_set_patches_device and
 *   srbd_vfa_height_step_scenes_device (further below) refuse their arguments before they follow any handle and
 *   store the message on the thread's slot, read with NULL -- after SRBD_E_INVALID from one of those two, the set's
 *   own message is an older one (the shared-scene forms of those two do the same with srbd_terrain_last_error(NULL)).
 *   srbd_terrain_set_num_scenes(NULL) is SRBD_E_INVALID,
 *   srbd_terrain_set_destroy(NULL) a no-op.
 *   srbd_tamols_batch_scenes_device is the terrain form of srbd_tamols_batch_device with environment e's rays cast
 *   against scene d_scene[e].  d_scene (num_envs int32) is the caller's device memory, read in stream order: a reset
 *   writes new indices with an ordinary operation earlier on the same stream, no entry point is needed for that and
 *   nothing reaches the host.
 *   Equivalence: every output of environment e (footholds, boxes, valid, seed_heights, scores, heightmaps_out, ref's
 *   entries 12..23; ref's entries 0..11 are not written) holds the bytes srbd_tamols_batch_device writes for that
 *   environment's inputs on a srbd_terrain created from scene d_scene[e].  Both form the yaw's cos / sin on the
 *   device, so the libm caveat of the single call does not arise.  Environments are independent.
 *   An index outside 0..num_scenes-1 cannot be reported from a launch: that environment runs on the empty scene (no
 *   ground, no primitives, no height field, miss_z NaN) and its outputs are those on such a srbd_terrain; nothing is
 *   read out of bounds.
 *   Launch shape: srbd_tamols_batch_device's grid, block and LDS.  Block (leg, e) reads d_scene[e] once (one wave),
 *   bounds-checks it and copies the scene's 88-byte record (or forms the empty one) next to the environment's other
 *   arguments; from there the stages are the shared-scene kernel's.
 *   Enqueue contract: srbd_tamols_batch_device's -- exactly one launch on hip_stream, no synchronising HIP call, no
 *   device memory touched from the host, the stream handle read the same way; the set must outlive the launch and
 *   live on the current device.
 *   SRBD_E_INVALID (before any HIP call, with a message): everything the terrain form of srbd_tamols_batch_device
 *   refuses; a NULL set or d_scene; a d_scene that is not 4-byte aligned; io->heightmaps given (the patch form has no
 *   scenes: that is srbd_tamols_batch_device).
 *   srbd_vfa_step_scenes_device is srbd_vfa_step_device with the same substitution: its equivalence, its launch
 *   shape, its read-once rule for initialized[leg] and its HOLD / PASS early exit.  A block that does not search reads
 *   neither its scene index nor the set, as it reads neither its yaw nor the terrain: an out-of-range index on a
 *   holding or passing environment has no effect.
 *   Out of scope: adding or replacing a scene after creation; per-environment scene origins, rows, cols or spacings;
 *   the patch form and the single-environment calls; a per-environment error flag for bad indices. */
typedef struct srbd_terrain_scene {
    const srbd_terrain_prim* prims; /* nprims primitives, or NULL when nprims == 0 */
    int32_t nprims, has_ground;
    double ground_z;
    const double* hfield;           /* hf_nx x hf_ny heights as in srbd_terrain_create, or NULL */
    int32_t hf_nx, hf_ny;
    double hf_x0, hf_y0, hf_dx, hf_dy;
    double miss_z;
} srbd_terrain_scene;
typedef struct srbd_terrain_set srbd_terrain_set;
int srbd_terrain_set_create(int32_t device_id, const srbd_terrain_scene* scenes, int32_t num_scenes,
                            srbd_terrain_set** out);
void srbd_terrain_set_destroy(srbd_terrain_set* set);
const char* srbd_terrain_set_last_error(const srbd_terrain_set* set);
int srbd_terrain_set_num_scenes(const srbd_terrain_set* set);
int srbd_tamols_batch_scenes_device(srbd_terrain_set* set, const int32_t* d_scene /* E */,
                                    const srbd_tamols_params* params, int32_t num_envs,
                                    const srbd_tamols_batch_io* io, void* hip_stream);
int srbd_vfa_step_scenes_device(struct srbd_vfa* d_vfa, const struct srbd_stc* d_stc, srbd_terrain_set* set,
                                const int32_t* d_scene /* E */, const srbd_tamols_params* params, int32_t num_envs,
                                const srbd_tamols_batch_io* io, double apex_interval, int32_t* d_mode /* E, or NULL */,
                                void* hip_stream);
/* Device-resident height scans: the heightmap sensor of the batched loop.  K rows x cols patches per environment,
 * raycast against the one scene all environments share (srbd_terrain_patches_device) or against scene d_scene[e] of a
 * set (srbd_terrain_set_patches_device), device in and device out on the caller's stream -- what a policy trained or
 * evaluated on the batched loop reads around the base or the feet, and what srbd_terrain_patches returns to the host.
 *   Inputs: centers num_envs x K x 3 (z is not read), yaws num_envs (one per environment, as the sensor has), the
 *   lattice (rows, cols, dist_x, dist_y) and ray_z shared by all patches.  Outputs, at least one of them: points
 *   num_envs x K x rows x cols x 3 (x, y, z) and heights num_envs x K x rows x cols, which is points[..., 2].
 *   Arithmetic: patch point (i, j), its coordinates and its ray are srbd_terrain_patches's (csrc/terrain_ray.h,
 *   float64, unfused); the yaw's cos / sin are formed on the device, correctly rounded (csrc/yaw_sincos.h), as
 *   srbd_tamols_batch_device forms them.
 *   Equivalence: every output of environment e holds the bytes heightmaps_out of srbd_tamols_batch_scenes_device
 *   (srbd_tamols_batch_device for the shared scene) holds for the same centres as seeds, the same yaw and lattice; for
 *   a yaw whose libm cos / sin equal srbd_selftest_yaw_sincos's it also holds the bytes srbd_terrain_patches returns on
 *   a srbd_terrain created from that scene.  "The bytes" as in the calls above: NaNs position for position (a NaN's
 *   sign and payload are not part of the contract).  Environments are independent: a NaN centre or yaw in one changes
 *   nothing in another.
 *   d_scene is read in stream order; an index outside 0..num_scenes-1 runs on the empty scene (no ground,
 *   no primitives, no height field, miss_z NaN) and nothing is read out of bounds.
 *   Launch shape: grid (K, num_envs), one block per (patch, environment) of rows * cols threads rounded up to whole
 *   waves (at most 320), one thread per ray; block (k, e) reads d_scene[e] once, bounds-checks it and copies the
 *   scene's record into LDS; heights are written as consecutive 8-byte stores.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it; every pointer is
 *   memory of the current device, which must be the terrain's or the set's; they must outlive the launch.
 *   SRBD_E_INVALID (before any HIP call, with a message naming the argument -- read it with
 *   srbd_terrain_last_error(NULL) / srbd_terrain_set_last_error(NULL): the handle is not followed before the arguments
 *   have passed): a NULL terrain, set, d_scene, io, centers or yaws; both outputs NULL; num_envs outside 1..4096;
 *   patches_per_env outside 1..16; rows or cols below 1 or rows * cols above 320; a dist_x or dist_y that is not
 *   positive and finite; a ray_z that is not finite; a d_scene that is not 4-byte aligned.  A failed launch:
 *   SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists.
 *   Out of scope: per-environment lattices, float32 outputs, graph capture. */
typedef struct srbd_patch_batch_io {
    const double* centers;   /* E x K x 3, device */
    const double* yaws;      /* E, device: one yaw per environment, as the sensor has */
    int32_t patches_per_env; /* K, 1..16 */
    int32_t rows, cols;      /* rows * cols 1..320, as srbd_tamols_batch_device */
    double dist_x, dist_y, ray_z;
    double* points;          /* E x K x rows x cols x 3 (x, y, z), or NULL */
    double* heights;         /* E x K x rows x cols (z only), or NULL; at least one of the two */
} srbd_patch_batch_io;
int srbd_terrain_patches_device(srbd_terrain* terrain, int32_t num_envs, const srbd_patch_batch_io* io,
                                void* hip_stream);
int srbd_terrain_set_patches_device(srbd_terrain_set* set, const int32_t* d_scene /* E */, int32_t num_envs,
                                    const srbd_patch_batch_io* io, void* hip_stream);
/* The 'height' strategy behind the apex gate (VisualFootholdAdaptation.compute_adaptation, strategy 'height',
 * visual_foothold_adaptation.py:145-151, inside wb_interface.py:230-246): srbd_vfa_step_device with another search --
 * a searching leg's foothold is its seed with z = the height of the nearest point of the leg's raycast patch + 0.02
 * (srbd_vfa_height_search of srbd_host.h is the host twin; csrc/srbd_vfa.h states it once for both).  The state is the
 * same srbd_vfa, the gate the same, so srbd_loop_reset_device resets it as before and an environment may be stepped by
 * either strategy.
 *   io is srbd_tamols_batch_device's struct.  Read: seeds, contact (required), yaws, rows, cols, dist_x, dist_y, ray_z.
 *   Written: footholds, boxes, valid, ref's entries 12..23 (what get_footholds_adapted returns), and for searching
 *   environments only seed_heights (the foothold's z) and heightmaps_out (the leg's patch: the bytes
 *   srbd_terrain_patches_device writes for the seed as centre).  hips, forward_vel, base_pos, feet and scores are
 *   ignored and may be NULL.  There is no patch form: io->heightmaps is refused.
 *   Boxes: the strategy has no foothold constraints, so the searched box is NaN, and the call inherits
 *   srbd_vfa_commit's rule for it -- a leg whose ray hit (valid 1) stores the NaN box, a leg whose nearest point is a
 *   miss on a scene with miss_z NaN (foothold z NaN, valid 0) keeps the box its state held (NaN after srbd_vfa_init;
 *   an older TAMOLS box if the state came from that strategy).
 *   Launch shape: grid (4 legs, num_envs), rows * cols threads rounded up to whole waves.  The gate, the read-once rule
 *   for initialized[leg] and the HOLD / PASS early exit are srbd_vfa_step_device's; a SEARCH block casts one ray per
 *   thread and reduces the argmin with wave shuffles and then LDS, the lowest index winning ties (numpy.argmin's rule:
 *   the first minimum, a NaN distance at its first occurrence), without atomics.
 *   Equivalence: environment e does what srbd_vfa_mode, then -- in SEARCH -- srbd_vfa_height_search on the four patches
 *   srbd_terrain_patches_device returns for its seeds, then srbd_vfa_commit with NaN boxes do on a host srbd_vfa with
 *   d_vfa[e]'s bytes: d_vfa[e], every output row and d_mode[e] hold the host's bytes (NaNs position for position).
 *   Environments are independent,
 *   and a non-searching environment reads neither its yaw, its scene index nor the scene.
 *   Enqueue contract: srbd_vfa_step_device's.
 *   SRBD_E_INVALID (before any HIP call, with a message as above): a NULL terrain, set, d_scene, d_vfa, d_stc, io,
 *   io->contact, io->seeds, io->footholds, io->boxes, io->valid or io->yaws; an apex_interval that is not finite;
 *   num_envs outside 1..4096; rows or cols below 1 or rows * cols above 320; a dist_x or dist_y that is not positive;
 *   io->heightmaps given; a d_scene that is not 4-byte aligned.
 *   Out of scope: a patch form; the 'vfa' strategy; compacting the searching environments into a smaller grid. */
int srbd_vfa_height_step_device(struct srbd_vfa* d_vfa, const struct srbd_stc* d_stc, srbd_terrain* terrain,
                                int32_t num_envs, const srbd_tamols_batch_io* io, double apex_interval,
                                int32_t* d_mode /* E, or NULL */, void* hip_stream);
int srbd_vfa_height_step_scenes_device(struct srbd_vfa* d_vfa, const struct srbd_stc* d_stc, srbd_terrain_set* set,
                                       const int32_t* d_scene /* E */, int32_t num_envs,
                                       const srbd_tamols_batch_io* io, double apex_interval,
                                       int32_t* d_mode /* E, or NULL */, void* hip_stream);
/* Self-test: out_cs[2 i], out_cs[2 i + 1] = the cos and sin srbd_tamols_batch_device's kernel forms of yaws[i],
 * evaluated on the host by the same function (plain float64 operations and fma: the same bits on both sides). */
int srbd_selftest_yaw_sincos(const double* yaws, int32_t n, double* out_cs);

/* The foothold reference generator of the device-resident loop: the `seeds` srbd_tamols_batch_device reads, and on
 * flat ground the reference's feet directly (FootholdReferenceGenerator, foothold_reference_generator.py:53-199, run
 * by WBInterface.update_state_and_reference every step between the gait generator and the foothold adaptation,
 * wb_interface.py:202-227), for num_envs environments in one launch, so that generator.run -> seeds -> footholds ->
 * prepare -> srbd_batch_step_device never leaves the GPU.
 *   Generator state: d_frg is an array of num_envs srbd_frg structs (srbd_host.h, plain data) in device memory.  The
 *   caller initialises them on the host with srbd_frg_init, uploads them, and may download and inspect them at any
 *   time.  Stance time, hip height and hip offset are per environment, read from the struct; com_height_nominal and
 *   gravity are shared.
 *   Equivalence: for environment e the call does what these three host calls do in order on a host srbd_frg with the
 *   same bytes: srbd_frg_update_lift_off, srbd_frg_update_touch_down, srbd_frg_compute (srbd_host.h), with the
 *   contacts widened to double, full_stance = (pgg != NULL and pgg[e].gait_type == SRBD_GAIT_FULL_STANCE), base_pos[e],
 *   yaws[e], the x and y of base_lin_vel[e] and ref_lin_vel[e], and com_pos_offset_w[e] or NULL.  Afterwards d_frg[e]
 *   holds exactly the host struct's bytes and seeds[e] the host's `out`, bit for bit, NaNs position for position.  The
 *   arithmetic is float64 in the order of the host functions, unfused -- both sides compile the same per-leg
 *   functions -- with cos / sin of the yaw correctly rounded on both (csrc/yaw_sincos.h) and sqrt(com_height_nominal
 *   / gravity) evaluated once on the host.  Environments are independent: a NaN in one changes nothing in another.
 *   ref, when given, is srbd_prepare_state_device's d_ref_in: entries 12..23 of row e (ref_foot_FL..RR) receive
 *   environment e's footholds, entries 0..11 are not written -- the flat-ground loop ('blind') needs no other
 *   foothold call.  previous_contact / current_contact are float32 as srbd_pgg_run_device writes them.  Only
 *   gait_type is read from pgg.
 *   Enqueue contract (the producers' above, srbd_prepare_state_device's): exactly one launch on hip_stream, no
 *   synchronising HIP call, no device memory touched from the host; the stream handle is read as
 *   srbd_prepare_state_device reads it (NULL and hipStreamLegacy both select the legacy null stream); every pointer is
 *   memory of the current device; no event and no ordering rule.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL d_frg, io or required pointer (every pointer except pgg,
 *   com_pos_offset_w and ref); a com_height_nominal or gravity that is not finite; gravity <= 0; num_envs outside
 *   1..4096.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
struct srbd_frg;
typedef struct srbd_frg_batch_io {
    /* inputs: device memory, float64 unless noted; E = num_envs */
    const double* base_pos;           /* E x 3 */
    const double* yaws;               /* E */
    const double* base_lin_vel;       /* E x 3, x and y used */
    const double* ref_lin_vel;        /* E x 3, x and y used */
    const double* hips;               /* E x 4 x 3 */
    const double* feet;               /* E x 4 x 3 */
    const float* previous_contact;    /* E x 4 float32, as srbd_pgg_run_device writes it */
    const float* current_contact;     /* E x 4 float32 */
    const struct srbd_pgg* pgg;       /* E, or NULL; only gait_type is read: FULL_STANCE -> the full-stance branch */
    const double* com_pos_offset_w;   /* E x 3, or NULL */
    double com_height_nominal, gravity; /* shared */
    /* outputs */
    double* seeds;                    /* E x 4 x 3: the layout srbd_tamols_batch_device reads */
    double* ref;                      /* E x 24 or NULL: entries 12..23 of row e receive the footholds */
} srbd_frg_batch_io;
int srbd_frg_step_device(struct srbd_frg* d_frg, int32_t num_envs, const srbd_frg_batch_io* io, void* hip_stream);

/* The stance and swing leg controller of the device-resident loop: the joint torques a simulator applies, from the
 * ground-reaction forces srbd_batch_step_device returns (WBInterface.compute_stance_and_swing_torque,
 * wb_interface.py:369-415 and :435-465, with SwingTrajectoryController, swing_trajectory_controller.py:48-146, and the
 * 'bezier_ref' and 'explicit' swing generators), for num_envs environments in one launch, so that generator.run ->
 * footholds -> prepare -> srbd_batch_step_device -> torques never leaves the GPU.
 *   Controller state: d_stc is an array of num_envs srbd_stc structs (srbd_host.h, plain data) in device memory.  The
 *   caller initialises them on the host with srbd_stc_init, uploads them, and may download and inspect them at any
 *   time.  Step height, swing period, gains, generator and the two switches are per environment, read from the
 *   struct; dt and apex_interval are shared.
 *   Inputs are the simulator's: jac, jac_dot and mass_matrix are each leg's 3 x 3 block (row-major, already sliced to
 *   the leg's own three joint columns), q_dot, qfrc_passive and qfrc_bias the leg's three joints.  lift_off is given
 *   either as an array or through frg, the device state of srbd_frg_step_device, whose lift_off table is read; exactly
 *   one of the two.  contact is float32 as srbd_pgg_run_device writes it: a leg is in swing iff its flag == 0.0f.
 *   Equivalence: for environment e the call does what the host call srbd_stc_step (srbd_host.h) does on a host srbd_stc
 *   with the same bytes and the same inputs, the contacts widened to double.  Afterwards d_stc[e] holds exactly the
 *   host struct's bytes and every output row the host's values, bit for bit, NaNs position for position; apex[e] and
 *   full_stance[e] are the host's two words.  The arithmetic is float64 in the order of the host function, unfused --
 *   both sides compile the same per-leg functions (csrc/srbd_stc.h).  Environments are independent: a NaN in one
 *   changes nothing in another.  An environment whose struct the host call refuses (unknown generator, swing_period not
 *   positive and finite) is left as found and its output rows are not written.  The deviations from the reference are
 *   the host function's: Jinv is the 3 x 3 inverse by cofactors over the determinant where the reference calls
 *   np.linalg.pinv, and the zero matrix for a singular Jacobian (determinant zero or not finite).
 *   Enqueue contract (the producers' above, srbd_prepare_state_device's): exactly one launch on hip_stream, no
 *   synchronising HIP call, no device memory touched from the host; the stream handle is read as
 *   srbd_prepare_state_device reads it (NULL and hipStreamLegacy both select the legacy null stream); every pointer is
 *   memory of the current device; no event and no ordering rule.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL d_stc, io or required pointer (every pointer except lift_off, frg,
 *   des_joint_vel, apex and full_stance); both or neither of lift_off and frg; num_envs outside 1..4096; a dt or
 *   apex_interval that is not finite.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
struct srbd_stc;
typedef struct srbd_stc_batch_io {
    /* inputs: device memory, float64 unless noted; E = num_envs */
    const double* jac;                /* E x 4 x 3 x 3 */
    const double* jac_dot;            /* E x 4 x 3 x 3 */
    const double* mass_matrix;        /* E x 4 x 3 x 3 */
    const double* q_dot;              /* E x 4 x 3 */
    const double* foot_pos;           /* E x 4 x 3 */
    const double* foot_vel;           /* E x 4 x 3 */
    const double* qfrc_passive;       /* E x 4 x 3 */
    const double* qfrc_bias;          /* E x 4 x 3 */
    const double* grfs;               /* E x 4 x 3 */
    const double* touch_down;         /* E x 4 x 3 */
    const double* lift_off;           /* E x 4 x 3, or NULL when frg is given */
    const struct srbd_frg* frg;       /* E, or NULL when lift_off is given; only lift_off is read */
    const float* contact;             /* E x 4 float32, as srbd_pgg_run_device writes it */
    double apex_interval;             /* shared */
    /* outputs */
    double* tau;                      /* E x 4 x 3 */
    double* des_foot_pos;             /* E x 4 x 3 */
    double* des_foot_vel;             /* E x 4 x 3 */
    double* des_joint_vel;            /* E x 4 x 3, or NULL */
    int32_t* apex;                    /* E, or NULL */
    int32_t* full_stance;             /* E, or NULL */
} srbd_stc_batch_io;
int srbd_stc_step_device(struct srbd_stc* d_stc, int32_t num_envs, double dt, const srbd_stc_batch_io* io,
                         void* hip_stream);

/* The swing reflex path of the device-resident loop: the early-stance detector, the swing clocks and the stance and
 * swing torques with the 'scipy' spline generator, the one generator that re-plans a swing from the point where the
 * foot hit something (WBInterface.compute_stance_and_swing_torque, wb_interface.py:362-415 and :435-465, with
 * EarlyStanceDetector.update_detection, early_stance_detector.py:36-128, in 'tracking' mode and
 * SwingTrajectoryController(generator="scipy"), swing_generators/scipy_swing_trajectory_generator.py:25-122), for
 * num_envs environments in one launch.  It takes srbd_stc_step_device's place in the loop for a caller that wants the
 * reference's reflexes; srbd_stc_step_device itself is unchanged.
 *   State: d_stc as for srbd_stc_step_device -- the same structs, so srbd_gait_apply_freq_device, srbd_loop_reset_device
 *   and srbd_vfa_step_device work on them unchanged; the `generator` field is not read here -- and d_reflex, an array
 *   of num_envs srbd_reflex structs (srbd_host.h, plain data) in device memory, initialised on the host with
 *   srbd_reflex_init and uploaded: thresholds, reflex_max_step_height, trigger mode, blind flag and the enhancement
 *   switch are per environment.  srbd_loop_reset_device does not know d_reflex: a caller that restarts an environment
 *   copies that environment's struct as srbd_reflex_init left it over d_reflex[e] on the same stream.
 *   Inputs are srbd_stc_step_device's (io->stc) plus previous_contact, E x 4 float32: the contact flags of the previous
 *   control step (WBInterface.previous_contact), read by the detector's touch-down edge.
 *   Order within an environment, as srbd_reflex_step (srbd_host.h): the detector -- on the clocks and
 *   last_des_foot_pos the previous call left, foot_pos, lift_off, touch_down, contact, previous_contact; the clock
 *   update; the leg law with the spline generator; des_foot_pos into d_reflex[e].last_des_foot_pos; apex and full
 *   stance.
 *   Equivalence: for environment e the call does what the host call srbd_reflex_step (srbd_host.h) does on host structs
 *   with the same bytes and the same inputs, the contacts widened to double.  Afterwards d_stc[e] and d_reflex[e] hold
 *   exactly the host structs' bytes and every output row the host's values, bit for bit, NaNs position for position.
 *   Both sides compile the same per-leg functions (csrc/srbd_reflex.h, csrc/srbd_stc.h).  Environments are
 *   independent: a NaN in one changes nothing in another.  An environment whose structs the host call refuses
 *   (swing_period not positive and finite, a trigger mode other than SRBD_REFLEX_OFF and SRBD_REFLEX_TRACKING --
 *   'geom_contact' among them --, a reflex_max_step_height that is not finite) is left as found and its output rows
 *   are not written.  The deviations from the reference are the host function's: Jinv as in srbd_stc_step_device
 *   (np.linalg.pinv there, the cofactor inverse and the zero matrix for a singular Jacobian here), the spline solved by
 *   elimination in a fixed order where scipy calls LAPACK, and the no-hit curve for a leg whose hit moment is not
 *   below swing_period, where scipy raises.
 *   Enqueue contract (the producers' above, srbd_prepare_state_device's): exactly one launch on hip_stream, no
 *   synchronising HIP call, no device memory touched from the host; the stream handle is read as
 *   srbd_prepare_state_device reads it (NULL and hipStreamLegacy both select the legacy null stream); every pointer is
 *   memory of the current device; no event and no ordering rule.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL d_stc, d_reflex, io, io->previous_contact or required pointer of
 *   io->stc (every pointer except lift_off, frg, des_joint_vel, apex and full_stance); both or neither of lift_off
 *   and frg; num_envs outside 1..4096; a dt or apex_interval that is not finite.  A failed launch: SRBD_E_HIP, or
 *   SRBD_E_NODEVICE where no device exists. */
struct srbd_reflex;
typedef struct srbd_reflex_batch_io {
    srbd_stc_batch_io stc;            /* the arrays of srbd_stc_step_device, read and written as there */
    const float* previous_contact;    /* E x 4 float32: the previous control step's contact flags */
} srbd_reflex_batch_io;
int srbd_reflex_step_device(struct srbd_stc* d_stc, struct srbd_reflex* d_reflex, int32_t num_envs, double dt,
                            const srbd_reflex_batch_io* io, void* hip_stream);

/* The velocity modulator and the terrain estimate with the reference row of the device-resident loop: what
 * WBInterface.update_state_and_reference builds from the velocity command before and after the foothold reference
 * generator (wb_interface.py:168-172 with velocity_modulator.py:19-46; wb_interface.py:250-291 with
 * terrain_estimator.py:13-106), for num_envs environments in one launch each, so that the loop needs only measurements
 * and a velocity command from the simulator: modulate -> srbd_frg_step_device -> terrain / reference ->
 * srbd_prepare_state_device.
 *   srbd_vm_modulate_device: lin_out[e], ang_out[e] are what the host call srbd_vm_modulate (srbd_host.h) returns for
 *   lin[e], ang[e], feet[e], hips[e] and the shared max_distance, bit for bit.  lin_out is what srbd_frg_step_device
 *   then reads as ref_lin_vel.  The modulator has no state.
 *   srbd_terrain_ref_step_device: estimator state d_terrain is an array of num_envs srbd_terrain_est structs
 *   (srbd_host.h, plain data) in device memory, initialised on the host with srbd_terrain_est_init and uploaded.  The
 *   feet are given either as an array or through frg, the device state of srbd_frg_step_device, whose lift_off table
 *   is read (the positions the reference passes); exactly one of the two.
 *   Equivalence: for environment e the call does what these two host calls do in order on a host struct with the same
 *   bytes: srbd_terrain_estimate(g, base_pos[e], yaws[e], feet[e], terrain[e]) and srbd_reference_assemble(g, ref_z,
 *   base_pos[e][2], com_pos[e][2], com_pos_offset_w ? com_pos_offset_w[e][2] : 0.0, lin[e], ang[e], ref[e][0:12]).
 *   Afterwards d_terrain[e] holds exactly the host struct's bytes and entries 0..11 of row e of ref the host's values,
 *   bit for bit, NaNs position for position; entries 12..23 are not written.  Both sides compile the same functions
 *   (csrc/srbd_terrain.h, csrc/yaw_sincos.h), none of which calls libm or the device library for cos, sin or arctan.
 *   Environments are independent: a NaN in one changes nothing in another.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; NULL and hipStreamLegacy both select the legacy null stream; every pointer is memory
 *   of the current device.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL io or required pointer (every pointer except com_pos_offset_w, feet,
 *   frg and terrain; d_terrain too); both or neither of feet and frg; a ref_z that is not finite; a max_distance that
 *   is NaN; num_envs outside 1..4096.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
typedef struct srbd_vm_batch_io {
    /* inputs: device memory, float64; E = num_envs */
    const double* lin;                /* E x 3: ref_base_lin_vel, the command */
    const double* ang;                /* E x 3: ref_base_ang_vel */
    const double* feet;               /* E x 4 x 3 */
    const double* hips;               /* E x 4 x 3 */
    double max_distance;              /* shared; the reference's value is 0.2 */
    /* outputs */
    double* lin_out;                  /* E x 3 */
    double* ang_out;                  /* E x 3 */
} srbd_vm_batch_io;
int srbd_vm_modulate_device(int32_t num_envs, const srbd_vm_batch_io* io, void* hip_stream);

struct srbd_terrain_est;
typedef struct srbd_terrain_ref_batch_io {
    /* inputs: device memory, float64; E = num_envs */
    const double* base_pos;           /* E x 3 */
    const double* com_pos;            /* E x 3, z used */
    const double* com_pos_offset_w;   /* E x 3, z used, or NULL (+0.0) */
    const double* yaws;               /* E */
    const double* lin;                /* E x 3: the modulated ref_base_lin_vel */
    const double* ang;                /* E x 3: the modulated ref_base_ang_vel */
    const double* feet;               /* E x 4 x 3, or NULL when frg is given */
    const struct srbd_frg* frg;       /* E, or NULL when feet is given; only lift_off is read */
    double ref_z;                     /* shared */
    /* outputs */
    double* ref;                      /* E x 24: entries 0..11 of row e are written */
    double* terrain;                  /* E x 3 or NULL: roll, pitch, height */
} srbd_terrain_ref_batch_io;
int srbd_terrain_ref_step_device(struct srbd_terrain_est* d_terrain, int32_t num_envs,
                                 const srbd_terrain_ref_batch_io* io, void* hip_stream);

/* The gait adaptation loop of the device-resident step (mpc_params['optimize_step_freq']): the trigger that decides
 * per environment and step whether to optimise the step frequency, the device form of srbd_batch_set_gait, and the
 * write-back of the sampler's best frequency, so that run -> contact sequence -> trigger -> set gait ->
 * srbd_batch_step_device -> write-back never leaves the GPU.  Reference lines restated per environment:
 *   srbd_stc_touch_down_device  <- SwingTrajectoryController.check_touch_down_condition
 *                                  swing_trajectory_controller.py:148-165 (called wb_interface.py:298)
 *   srbd_batch_set_gait_device  <- the gait arguments of the gait-adaptive compute_control and its candidate set,
 *                                  centroidal_nmpc_jax_gait_adaptive.py:687-692 (random sampling), :834-838 (MPPI)
 *   srbd_gait_apply_freq_device <- wb_interface.py:354-358
 *   srbd_stc_touch_down_device: d_rising_edge (num_envs int32, caller-owned state, zero at start) is the reference's
 *   rising_edge_detected per environment; d_current, d_previous num_envs x 4 float32 as srbd_pgg_run_device writes
 *   them; d_contacts num_envs x 4 x contact_stride float32 as srbd_pgg_contact_sequence_device writes them, the first
 *   `horizon` columns read; d_optimize (num_envs int32) receives 0 or 1.  One lane per environment.
 *   srbd_gait_apply_freq_device: d_pgg, d_frg, d_stc are the device state arrays of srbd_pgg_run_device,
 *   srbd_frg_step_device and srbd_stc_step_device; d_frg and d_stc may each be NULL, for a caller that keeps only
 *   some of the stages.  d_optimize is the trigger's output, d_best_freq (num_envs float32) the best_freq array of
 *   srbd_batch_step_device.  One lane per environment.  An environment with d_optimize[e] != 1, or with a best
 *   frequency that is zero, negative or not finite, is left untouched.
 *   srbd_batch_set_gait_device is the device form of srbd_batch_set_gait: the gait fields of every environment's step
 *   input are written by one launch from device arrays, and the next enqueued step runs the gait-adaptive rollout.
 *   The leg phases come from exactly one of io->pgg (the device state of srbd_pgg_run_device: phase_signal[l] rounded
 *   to float32, round to nearest, as np.asarray(timing, dtype=float32) rounds it) or io->timings (num_envs x 4
 *   float32).  The nominal step frequency comes from io->nominal_freqs (num_envs float32) when given, else from
 *   io->pgg's step_freq rounded to float32; io->timings without io->nominal_freqs is refused.  Environment e's
 *   candidate set is formed as the reference forms it: MPPI takes available[0..n_freq); random sampling takes them
 *   when optimize[e] != 0 and n_freq copies of the nominal frequency otherwise.  available, n_freq, pgg_dt and
 *   duty_factor travel by value and are shared.  io->freq_rows (num_envs x N float32 device memory, or NULL) are
 *   injected per-sample frequencies (the parity mode): the launch copies environment e's N rows into the batch's
 *   frequency array.  That array is allocated on the first call that needs it; that first call may block (a
 *   hipMalloc), every other call does not.
 *   Equivalence: environment e after these calls holds, byte for byte, what the host calls leave: d_optimize[e] and
 *   d_rising_edge[e] are srbd_stc_touch_down's (srbd_host.h) for the contacts widened to double; d_pgg[e], d_frg[e],
 *   d_stc[e] hold the bytes srbd_gait_apply_freq leaves.  A srbd_batch_step_device after srbd_batch_set_gait_device
 *   returns, bit for bit, what it returns after srbd_batch_set_gait with the same values (timings the float32 phases,
 *   freq_sets[e] the set formed as above, the same freq_rows), best_freq included.
 *   Enqueue contract: each call enqueues exactly one launch on hip_stream and returns; it makes no synchronising HIP
 *   call and touches no device memory from the host (the first srbd_batch_set_gait_device with freq_rows excepted, as
 *   said).  srbd_stc_touch_down_device and srbd_gait_apply_freq_device read the stream handle as
 *   srbd_prepare_state_device reads it (NULL and hipStreamLegacy both select the legacy null stream), use none of a
 *   batch's buffers and enter no ordering rule.  srbd_batch_set_gait_device reads it as srbd_batch_step_device does
 *   (NULL: the batch's own stream; the legacy null stream by hipStreamLegacy) and joins the batch's event protocol as
 *   a device step does: it makes its stream wait on the event of the last device call on another stream and records
 *   the event behind its launch, so a set on stream A followed by srbd_batch_step_device on stream B is ordered
 *   exactly as two device steps are.  It sets the batch's gait-adaptive mode on the host at once.
 *   Stale staging: after srbd_batch_set_gait_device the host staging of the gait fields is stale.  Until
 *   srbd_batch_set_gait or srbd_batch_clear_gait is called, srbd_batch_step (the host step) returns SRBD_E_INVALID
 *   with a message naming those two calls, and changes nothing.  srbd_batch_step_device is not affected.
 *   SRBD_E_INVALID (before any HIP call): a NULL required pointer (d_frg, d_stc, io->freq_rows and one of io->pgg /
 *   io->timings excepted); num_envs outside 1..4096; horizon outside 2..SRBD_MAX_HORIZON; contact_stride < horizon;
 *   lookahead outside 1..horizon-1; both or neither of io->pgg and io->timings; io->timings without
 *   io->nominal_freqs; and srbd_batch_set_gait's refusals: n_freq outside 1..SRBD_MAX_FREQS, num_splines + 1 > 33,
 *   the opt-in cost terms active.  A failed launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
struct srbd_stc;
typedef struct srbd_batch_gait_io {
    const struct srbd_pgg* pgg;        /* E device structs, or NULL when timings is given */
    const float* timings;              /* E x 4 leg phases, or NULL when pgg is given */
    const float* nominal_freqs;        /* E, or NULL: pgg's step_freq rounded to float32 */
    const int32_t* optimize;           /* E: the trigger's flags */
    const float* freq_rows;            /* E x N injected frequencies, or NULL: device draws */
    float available[SRBD_MAX_FREQS];   /* the configured candidates, n_freq used */
    int32_t n_freq;
    float pgg_dt, duty_factor;
    int32_t pad;
} srbd_batch_gait_io;
int srbd_stc_touch_down_device(int32_t* d_rising_edge, int32_t num_envs, const float* d_current,
                               const float* d_previous, const float* d_contacts, int32_t contact_stride,
                               int32_t horizon, int32_t lookahead, int32_t* d_optimize, void* hip_stream);
int srbd_batch_set_gait_device(srbd_batch* b, const srbd_batch_gait_io* io, void* hip_stream);
int srbd_gait_apply_freq_device(struct srbd_pgg* d_pgg, struct srbd_frg* d_frg, struct srbd_stc* d_stc,
                                int32_t num_envs, const int32_t* d_optimize, const float* d_best_freq,
                                void* hip_stream);

/* ---- The controller interface's step of the batched loop, device-resident: the sampling branch of
 * SRBDControllerInterface.compute_control (quadruped_pympc/interfaces/srbd_controller_interface.py:113-180, :225-229;
 * SCI below) for every environment of a batch in one call -- the batch form of srbd_interface_step above, statement for
 * statement: prepare_state_and_reference (SCI:118-126), then per sampling iteration with_newkey (SCI:128, NMPC:498-501),
 * CEM's with_newsigma(sigma_cem_mppi) at iteration 0 (SCI:129-130) and the step (SCI:131-168), then the footholds from
 * the reference (SCI:170-175), the GRFs times current_contact (SCI:225-229) and previous_contact_mpc = current_contact.
 *   Batches: one from srbd_batch_create (MPPI or random sampling; io->gait NULL, or the gait setting of this control
 *   step, enqueued once ahead of the iterations as srbd_batch_set_gait_device enqueues it) and one from
 *   srbd_batch_create_cem (io->gait must be NULL; io->sigma required).  The batch's rng (srbd_batch_set_rng) selects the
 *   key rule; the cost terms and per-environment parameters set on the batch apply as they do to any step.
 *   Keys: keys[e] = (key[0], key[1]) with srbd_interface_io::key's meaning.  Per iteration, as srbd_interface_step:
 *     SRBD_RNG_PHILOX        key[1] += 1 (uint64, wrapping); the step runs (key[0], key[1])
 *     SRBD_RNG_JAX[_LEGACY]  key[0] = split(key[0])[0] in the stream's counter layout, key[1] += 1 (the call count);
 *                            the step runs (key[0], key[1])
 *   The prologue writes the `iterations` step keys of every environment into an array the batch owns (allocated at
 *   create for SRBD_MAX_IFACE_ITERS rows, each row E seeds then E counters: the unit-stride arrays the step reads) and
 *   the advanced key back to keys[e].  srbd_selftest_interface_keys runs the same function on the host.
 *   Launches: one prologue launch (one lane per (environment, leg) runs srbd_prepare_state_device's body with
 *   current_contact read from column 0 of contacts; the leg-0 lane of an environment runs its key schedule), then
 *   srbd_batch_set_gait_device's launch when io->gait is given, then `iterations` times the five launches of
 *   srbd_batch_step_device / srbd_batch_step_cem_device (iteration i reads row i of the key array; the CEM form gets
 *   sigma_reset at i == 0 and 0 afterwards), then one epilogue launch (one lane per (environment, leg)):
 *   grf[e][3 l + c] = (double)grf_raw[e][3 l + c] * (double)contacts[e][l][0], float64 and unfused (srbd_host.cpp's
 *   mask line); footholds[e][3 l + c] = ref_in[e][12 + 3 l + c]; previous_contact[e][l] = contacts[e][l][0].  No
 *   other launch or copy is enqueued.  contacts is only read, and read in stream order: the epilogue sees the column the prologue saw
 *   as long as the caller rewrites contacts by later work on the stream (or after the call has completed), never by
 *   work on another stream or from the host while the call is in flight.
 *   Outputs: states / refs (prepare_state's outputs as the step stages them, float32), grf (masked, float64),
 *   footholds, and the last iteration's srbd_batch_device_io outputs (grf_raw is its unmasked grf); best_params, sigma,
 *   keys and previous_contact are updated in place.  Only the last iteration's outputs are returned, as the reference
 *   keeps only the last.
 *   Equivalence: environment e afterwards holds, byte for byte, what srbd_interface_step leaves on a context
 *   srbd_create(cfg) with the same rng, state_in, ref_in, contact columns, key, previous contact, warm start (and
 *   sigma_reset): state_out / ref_out rounded to float32, grf, key, best_params, sigma, the last srbd_result; with
 *   io->gait, what srbd_batch_set_gait_device + `iterations` x srbd_batch_step_device with keys advanced by the rule
 *   above + the mask leave.  Environments are independent.
 *   Contracts: the enqueue contract, the stream handle (NULL: the batch's own stream; hipStreamLegacy: the legacy null
 *   stream), the event protocol and "no synchronising HIP call, no host touch of device memory" are
 *   srbd_batch_step_device's.  The batch's event is recorded behind the epilogue as well, so a following call on
 *   another stream, which waits on it, follows this call's stores of keys, best_params, sigma and previous_contact --
 *   the in / out state that lives between calls; every other caller-owned array is ordered across streams by the
 *   caller, as for srbd_batch_step_device.  Capturing the call into a HIP graph is not supported.  The arrays must not
 *   overlap.
 *   SRBD_E_INVALID (with a message, before anything is enqueued, nothing changed): b or io NULL; a required pointer
 *   NULL (every pointer but gait, costs and -- off a CEM batch -- sigma); iterations outside 1..SRBD_MAX_IFACE_ITERS;
 *   contact_stride < H; params_per_leg < 1 or 4 * params_per_leg != P; on a CEM batch sigma NULL, sigma_reset not
 *   positive and finite, or gait given; gait together with active cost terms; and every refusal srbd_batch_set_gait_device
 *   and the step make.
 *   srbd_selftest_interface_keys: the key schedule on the host, for n keys: keys_io (n x 2, in / out) advanced
 *   `iterations` times by the rule of `rng` (SRBD_RNG_*); step_keys (iterations x n x 2) receives the (seed, counter)
 *   pair each iteration's step runs.  SRBD_E_INVALID: a NULL pointer, n < 1, rng not an SRBD_RNG_* value, iterations
 *   outside 1..SRBD_MAX_IFACE_ITERS.  No device is needed. */
#define SRBD_MAX_IFACE_ITERS 8
typedef struct srbd_batch_interface_io {
    /* inputs, device memory of the batch's device */
    const double* state_in;        /* E x 24, srbd_prepare_state's layout */
    const double* ref_in;          /* E x 24 */
    const float*  contacts;        /* E x 4 x contact_stride; first H columns used; column 0 = current_contact */
    int32_t contact_stride, iterations;   /* iterations = num_sampling_iterations, 1..SRBD_MAX_IFACE_ITERS */
    int32_t params_per_leg, pad;
    const srbd_batch_gait_io* gait;       /* host struct of device pointers, or NULL (plain / CEM batch) */
    /* state, in / out, device memory, caller-owned */
    uint64_t* keys;                /* E x 2, srbd_interface_io::key's meaning for the batch's rng */
    float*    previous_contact;    /* E x 4: previous_contact_mpc; ones at start; out: this call's current_contact */
    float*    best_params;         /* E x P */
    float*    sigma;               /* E x P, CEM batch only (else NULL) */
    float     sigma_reset; int32_t pad2;  /* CEM: mpc_params['sigma_cem_mppi'], > 0 */
    /* outputs */
    float*  states; float* refs;   /* E x 24: prepare_state's outputs as the step stages them */
    double* grf;                   /* E x 12: last iteration's GRFs times current_contact, float64 */
    double* footholds;             /* E x 12: ref_in's feet (SCI:170-175) */
    float* grf_raw; float* predicted_state; float* best_cost; int32_t* best_index;
    float* best_freq; int32_t* status; float* costs;   /* the last iteration's, as srbd_batch_device_io; costs may be NULL */
} srbd_batch_interface_io;
int srbd_batch_interface_step_device(srbd_batch* b, const srbd_batch_interface_io* io, void* hip_stream);

/* ---- The due mask: the three device steps for the environments whose MPC is due, and no others.  The reference does
 * not solve on every simulation step: QuadrupedPyMPC_Wrapper.compute_actions (quadruped_pympc_wrapper.py
 * :134) runs compute_control when step_num % round(1 / (mpc_frequency * simulation_dt)) == 0 -- a 100 Hz MPC in a
 * 500 Hz loop solves every 5th step -- and between solves holds the last GRFs, footholds, best step frequency and
 * predicted state.  step_num is the environment's own counter and restarts with its episode, so after per-environment
 * resets (srbd_loop_reset_device) the environments of a batch are due on different steps.
 *   srbd_batch_step_masked_device, srbd_batch_step_cem_masked_device and srbd_batch_interface_step_masked_device are
 *   srbd_batch_step_device, srbd_batch_step_cem_device and srbd_batch_interface_step_device with `due`: E int32 words
 *   in device memory of the batch's device, read in stream order; non-zero: step this environment.
 *   Launches: the launches of the unmasked call, on the same grids, each with the mask -- the interface prologue
 *   (prepare_state and the key schedule), the gait setter, pack, the draws or the transpose, the rollouts (every
 *   instantiation, the per-environment-parameter and CEM ones included), the merges, unpack and the interface
 *   epilogue.  The environment is uniform over a block (over a lane in the prologue and the epilogue), so a block of
 *   an environment that is not due loads due[e] and returns before any other global access: its draws and rollouts do
 *   not run.  Nothing is compacted and the due count never reaches the host.  The kernels are the unmasked calls'
 *   (one body each, the mask a trailing argument that those calls pass as NULL).
 *   Arrival count: the merge blocks count themselves up to E before the last one resets the counter and stores the
 *   step's sequence word.  A block that is not due skips its merge and still takes part in the arrival count, so
 *   behind a masked call -- with no environment due as well -- the counter is zero and the word stored, and the next
 *   step of any kind (host srbd_batch_step included, which waits on that word) finds them as it expects.  No other
 *   counter or word on the path is shared between blocks: the rollouts of a batch write leaf records only, and the
 *   merge's own publish word per environment is written by its block and never read.
 *   Equivalence, an environment with due[e] != 0: every in / out and output array holds exactly the bytes the
 *   unmasked call leaves for that environment, for every batch kind and setting the unmasked call accepts (MPPI,
 *   random sampling, CEM; the three parametrizations; io->gait; the cost terms; per-environment parameters; the three
 *   key streams; 1..SRBD_MAX_IFACE_ITERS iterations).  Environments are independent, so the mask of the others does
 *   not matter.
 *   An environment with due[e] == 0 is neither written nor read: the caller's rows keys[e], previous_contact[e],
 *   best_params[e], sigma[e], states[e], refs[e], grf[e], footholds[e], grf_raw[e], predicted_state[e], best_cost[e],
 *   best_index[e], best_freq[e], status[e] and costs[e] keep their bytes, and so does the batch's own state of it that
 *   outlives a call -- its step input with the gait fields, its injected-frequency rows and its costs row
 *   (srbd_batch_copy_costs returns the costs of its last solve).  Its key does not advance, CEM's sigma_reset is not
 *   applied to it, previous_contact[e] keeps the contact of its last solve (the reference's previous_contact_mpc
 *   between solves), and none of its inputs is read: NaNs in them change nothing anywhere.  Holding the last solve is
 *   therefore handing the same output arrays to every call.
 *   Contracts: the enqueue contract, the stream handles, the event protocol, "no synchronising HIP call, no host
 *   touch of device memory" and every refusal (made before anything is enqueued) are the unmasked call's.  Added:
 *   due == NULL is SRBD_E_INVALID with a message that names the unmasked call; io and due are looked at before b, so
 *   either is named whatever b is.
 *   Out of scope: a masked host srbd_batch_step; the single context; compacting the due environments into a smaller
 *   grid; graph capture; a device-side step counter (step_num is the simulator's; the mask is one comparison on it);
 *   and every refusal the unmasked calls make stays (gait-adaptive sampling with the cost terms, gait-adaptive CEM,
 *   shift_solution).  srbd_batch_set_gait_device itself takes no mask: inside the masked interface step the gait
 *   setting is masked with the rest. */
int srbd_batch_step_masked_device(srbd_batch* b, const srbd_batch_device_io* io, const int32_t* due, void* hip_stream);
int srbd_batch_step_cem_masked_device(srbd_batch* b, const srbd_batch_device_io* io, const srbd_batch_cem_io* cem,
                                      const int32_t* due, void* hip_stream);
int srbd_batch_interface_step_masked_device(srbd_batch* b, const srbd_batch_interface_io* io, const int32_t* due,
                                            void* hip_stream);
int srbd_selftest_interface_keys(uint64_t* keys_io, int32_t n, int32_t rng, int32_t iterations, uint64_t* step_keys);

/* ---- Restarting single environments of the batched loop, device-resident: the episode's end of the reference's
 * simulation loop (simulation/simulation.py:773-781: on is_terminated, is_truncated or the step limit, env.reset and
 * quadrupedpympc_wrapper.reset(initial_feet_pos), which reaches WBInterface.reset, quadruped_pympc/interfaces/
 * wb_interface.py:469-484, and controller.reset()) for the environments a mask names, in one launch.  srbd_host.h
 * (srbd_loop_reset) and csrc/srbd_reset.h state the two levels; this is their device form.
 *   io->mask (num_envs int32) chooses per environment:
 *     0      not reset: no byte of environment e is written, not even with the value it holds, and none of its inputs
 *            is read (io->initial_feet[e], the snapshots' entry e): a NaN there changes nothing anywhere.
 *     2      SRBD_RESET_EPISODE: io->pgg[e], stc[e], terrain_est[e], vfa[e] take the bytes of their snapshot's entry e
 *            (the same arrays as they were when the loop was built: clone them then); io->frg[e] becomes
 *            srbd_frg_init(snapshot stance_time, snapshot hip_height, initial_feet[e]) with the snapshot's hip_offset;
 *            io->rising_edge[e] = 0; io->best_params[e][0..num_params) = 0.0f.
 *     other  SRBD_RESET_REFERENCE, WBInterface.reset statement for statement: srbd_pgg_reset on pgg[e] (step_freq left
 *            alone), frg[e].lift_off = initial_feet[e] (that table only), vfa[e].initialized[0..3] = 0.  stc,
 *            terrain_est, rising_edge and best_params are not touched.
 *     at both levels every io->contact_rows[i][e][0..4) = 1.0f (self.current_contact = [1, 1, 1, 1], :483): the
 *     caller names which of its num_envs x 4 float32 contact tensors these are (the loop's previous-contact rows).
 *   Every struct array, rising_edge and best_params may be NULL: that piece is not part of the caller's loop.  A
 *   snapshot is required for every struct that is given, whatever the mask holds: the levels live in device memory, so
 *   the host call's rule (a snapshot at level 2 only) cannot be applied here.  initial_feet (num_envs x 4 x 3 float64)
 *   is required with frg.  The struct arrays are 8-byte aligned (any device allocation is).
 *   Launch shape: one wave per environment, four waves per 256-thread block, ceil(num_envs / 4) blocks.  The wave
 *   loads its mask word once, makes it wave-uniform and leaves at once when it is 0; otherwise a struct's 8-byte words
 *   are spread over the 64 lanes (srbd_frg, 104 words, takes two rounds) as 8-byte loads and stores.  No LDS, no
 *   atomics, no scratch; waves share nothing.
 *   Equivalence: environment e afterwards holds, byte for byte, what srbd_loop_reset leaves on host copies of its
 *   structs at the level its mask word selects, and every contact row holds ones.  Environments are independent.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it -- and as
 *   srbd_batch_step_device reads an explicit one (hipStreamLegacy selects the legacy null stream; NULL selects it too,
 *   there being no batch whose stream it could mean).  The call touches no srbd_batch: the gait fields of a batch's
 *   step input are rewritten by srbd_batch_set_gait_device every step, so it enters no ordering rule of the batch.
 *   SRBD_E_INVALID (before any HIP call, with a message for srbd_last_error(NULL)): num_envs outside 1..4096; a NULL
 *   io or io->mask; n_contact_rows outside 0..4 or a NULL row among them; frg without initial_feet; a struct without
 *   its snapshot; best_params with num_params < 1; a struct array or snapshot that is not 8-byte aligned.  A failed
 *   launch: SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists.
 *   Out of scope: the simulator's own reset; advancing or re-seeding the per-environment keys (the caller's tensor);
 *   compacting the reset environments into a smaller grid (their count would have to reach the host). */
struct srbd_terrain_est;
typedef struct srbd_loop_reset_io {
    const int32_t* mask;          /* E */
    const double* initial_feet;   /* E x 4 x 3, or NULL when frg is */
    struct srbd_pgg* pgg;         /* E device structs each, or NULL */
    struct srbd_frg* frg;
    struct srbd_stc* stc;
    struct srbd_terrain_est* terrain_est;
    struct srbd_vfa* vfa;
    const struct srbd_pgg* pgg_snapshot; /* E device structs each: required where the struct array is given */
    const struct srbd_frg* frg_snapshot;
    const struct srbd_stc* stc_snapshot;
    const struct srbd_terrain_est* terrain_est_snapshot;
    const struct srbd_vfa* vfa_snapshot;
    int32_t* rising_edge;         /* E, or NULL */
    float* best_params;           /* E x num_params, or NULL */
    float* contact_rows[4];       /* n_contact_rows tensors of E x 4 */
    int32_t num_params, n_contact_rows;
} srbd_loop_reset_io;
int srbd_loop_reset_device(int32_t num_envs, const srbd_loop_reset_io* io, void* hip_stream);

/* ---- Start-and-stop, and the whole of WBInterface.update_state_and_reference in one launch.
 *   srbd_pgg_start_stop_device <- PeriodicGaitGenerator.update_start_and_stop, periodic_gait_generator.py:128-196
 *                                 (called wb_interface.py:175-189)
 *   srbd_wb_update_device      <- WBInterface.update_state_and_reference, wb_interface.py:168-298, the visual foothold
 *                                 adaptation (:230-246) excepted
 *   srbd_pgg_start_stop_device: for every environment what the host call srbd_pgg_start_stop (srbd_host.h) does on a
 *   host srbd_pgg with the same bytes, with feet[e], hips[e], base_pos[e], euler[e] (roll, pitch, yaw), base_lin_vel[e],
 *   base_ang_vel[e], the (modulated) command ref_lin[e] / ref_ang[e] and current_contact[e] widened to double (float32
 *   as srbd_pgg_run_device writes it).  The hip offset is read either from io->frg (the device srbd_frg array's
 *   hip_offset field, per environment) or from *io->hip_offset (a host double shared by the environments); exactly one
 *   of the two is given.  Afterwards d_pgg[e] holds exactly the bytes the host call leaves, and action[e] (optional)
 *   its return value: 0 untouched, 1 stopped (full stance), 2 restored.  One quad of lanes per environment: lane l
 *   forms leg l's two horizontal-frame points and its distance, the four verdicts are combined by quad shuffles, and
 *   the lane that owns field l of the struct writes it (lane 0 the gait type besides).  Environments are independent:
 *   a NaN in one makes that one's condition false and changes nothing in another.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it (NULL and
 *   hipStreamLegacy both select the legacy null stream); no event and no ordering rule.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL d_pgg, io or required pointer (every pointer except frg, hip_offset
 *   and action); both or neither of frg and hip_offset; num_envs outside 1..4096.  A failed launch: SRBD_E_HIP, or
 *   SRBD_E_NODEVICE where no device exists. */
typedef struct srbd_start_stop_batch_io {
    /* inputs: device memory, float64 unless noted; E = num_envs */
    const double* feet;               /* E x 4 x 3 */
    const double* hips;               /* E x 4 x 3 */
    const double* base_pos;           /* E x 3 */
    const double* euler;              /* E x 3: roll, pitch, yaw */
    const double* base_lin_vel;       /* E x 3 */
    const double* base_ang_vel;       /* E x 3 */
    const double* ref_lin;            /* E x 3: the (modulated) command */
    const double* ref_ang;            /* E x 3 */
    const float* current_contact;     /* E x 4 float32, as srbd_pgg_run_device writes it */
    const struct srbd_frg* frg;       /* E, or NULL when hip_offset is given; only hip_offset is read */
    const double* hip_offset;         /* HOST memory: one shared value, or NULL when frg is given */
    /* output */
    int32_t* action;                  /* E, or NULL: 0 untouched, 1 stopped, 2 restored */
} srbd_start_stop_batch_io;
int srbd_pgg_start_stop_device(struct srbd_pgg* d_pgg, int32_t num_envs, const srbd_start_stop_batch_io* io,
                               void* hip_stream);

/*   srbd_wb_update_device: one call, exactly one launch, that runs for every environment what these existing device
 *   calls do, in this order -- the reference's, wb_interface.py:168-298:
 *     1. srbd_vm_modulate_device, if SRBD_WB_VM is set in io->stages; otherwise the command passes through to lin_out /
 *        ang_out unchanged.
 *     2. srbd_pgg_start_stop_device, if SRBD_WB_START_STOP is set, on the modulated command and on the contact state
 *        d_contact as the previous call left it, with the hip offset of d_frg.
 *     3. srbd_pgg_run_device(dt) with each environment's own step frequency; its flags are discarded, as the reference
 *        discards them.
 *     4. srbd_pgg_contact_sequence_device into contacts (E x 4 x contact_stride float32); dts / lens are host arrays and
 *        travel by value, as for that call.
 *     5. the contact bookkeeping of wb_interface.py:196-199: previous_contact[e] receives the contact state; the
 *        contact state d_contact[e] (E x 4 float32, caller-owned, all ones at start) becomes column 0 of the sequence;
 *        current_contact receives a copy.
 *     6. srbd_frg_step_device with that previous / current pair and pgg given (gait_type as step 2 left it): seeds and
 *        ref[:, 12:24].
 *     7. srbd_terrain_ref_step_device with frg given (its lift-off table, after step 6) and the modulated command:
 *        ref[:, 0:12] and the optional terrain rows.
 *     8. srbd_stc_touch_down_device(lookahead) into optimize, if SRBD_WB_TOUCH_DOWN is set; otherwise optimize[e] = 0 and
 *        d_rising_edge is neither read nor written (it may then be NULL).
 *   The visual foothold adaptation (wb_interface.py:230-246) is not part of it: srbd_vfa_step_device stays the separate
 *   launch behind this call and rewrites ref[:, 12:24].
 *   State: d_pgg, d_frg, d_terrain (the struct arrays of the calls above), d_contact and d_rising_edge, all device
 *   memory, caller-owned, plain data.  The yaw the chain's calls take as `yaws` is euler[e][2].
 *   Equivalence: after the call every state array holds the bytes, and every output the values, that the chain above
 *   leaves -- bit for bit, NaNs position for position, for every combination of stages -- and so, through those
 *   calls' own equivalences, what the host functions of srbd_host.h leave.  The kernel runs the same per-leg functions
 *   (csrc/srbd_frg.h, srbd_terrain.h, srbd_gait_adapt.h, srbd_start_stop.h and the gait generator's helpers), unfused
 *   and in the same order, through device functions it shares with the kernels of the single calls.  Lane 4 e + l is
 *   leg l of environment e, 64 environments per 256-thread block.  What a later stage needs from an earlier one stays
 *   in registers or crosses the quad by shuffles (the modulated command, the gait type after start-and-stop, the
 *   leg's phase state, column 0 of the sequence, the previous contact); the intermediate arrays lin_out, ang_out,
 *   current_contact and previous_contact are written where given and never read back.
 *   Enqueue contract (the producers' above): exactly one launch on hip_stream, no synchronising HIP call, no device
 *   memory touched from the host; the stream handle is read as srbd_prepare_state_device reads it; no event and no
 *   ordering rule.  Arrays must not overlap.
 *   SRBD_E_INVALID (before any HIP call): a NULL d_pgg, d_frg, d_terrain, d_contact, io or required pointer (every
 *   pointer except com_pos_offset_w, lin_out, ang_out, current_contact, previous_contact, terrain and action; and
 *   d_rising_edge when the trigger is off); num_envs outside 1..4096; horizon outside 2..SRBD_MAX_HORIZON;
 *   contact_stride < horizon; lookahead outside 1..horizon-1 when the trigger is on; n_dts outside 1..32 or lens that
 *   would run past n_dts before step horizon - 1; a dt, ref_z, com_height_nominal or gravity that is not finite;
 *   gravity <= 0; a max_distance that is NaN when the modulator is on; unknown bits in stages.  A failed launch:
 *   SRBD_E_HIP, or SRBD_E_NODEVICE where no device exists. */
enum { SRBD_WB_VM = 1, SRBD_WB_START_STOP = 2, SRBD_WB_TOUCH_DOWN = 4 };
typedef struct srbd_wb_update_io {
    /* inputs: device memory, float64; E = num_envs */
    const double* com_pos;            /* E x 3, z used */
    const double* base_pos;           /* E x 3 */
    const double* base_lin_vel;       /* E x 3 */
    const double* euler;              /* E x 3: roll, pitch, yaw */
    const double* base_ang_vel;       /* E x 3 */
    const double* feet;               /* E x 4 x 3 */
    const double* hips;               /* E x 4 x 3 */
    const double* ref_lin;            /* E x 3: ref_base_lin_vel, the command */
    const double* ref_ang;            /* E x 3: ref_base_ang_vel */
    const double* com_pos_offset_w;   /* E x 3, or NULL */
    /* shared by the environments */
    const double* dts;                /* HOST memory, n_dts entries: the contact sequence's time steps */
    const int32_t* lens;              /* HOST memory, n_dts entries: dts[j] holds for the steps i < lens[j] */
    double dt;                        /* simulation_dt of srbd_pgg_run_device */
    double max_distance;              /* the modulator's; the reference's value is 0.2 */
    double com_height_nominal, gravity; /* srbd_frg_step_device's */
    double ref_z;                     /* srbd_terrain_ref_step_device's */
    /* outputs: device memory */
    double* lin_out;                  /* E x 3 or NULL: the modulated command */
    double* ang_out;                  /* E x 3 or NULL */
    float* contacts;                  /* E x 4 x contact_stride float32: columns 0..horizon-1 written */
    float* current_contact;           /* E x 4 float32 or NULL: a copy of the new contact state */
    float* previous_contact;          /* E x 4 float32 or NULL: the contact state as it was found */
    double* seeds;                    /* E x 4 x 3 */
    double* ref;                      /* E x 24: every entry written */
    double* terrain;                  /* E x 3 or NULL: roll, pitch, height */
    int32_t* optimize;                /* E */
    int32_t* action;                  /* E or NULL: start-and-stop's 0 / 1 / 2 (0 when that stage is off) */
    int32_t n_dts, horizon, contact_stride, lookahead;
    int32_t stages;                   /* SRBD_WB_* bits */
    int32_t pad;                      /* 0: the sixth word, so that no padding is left to chance */
} srbd_wb_update_io;
struct srbd_terrain_est;
int srbd_wb_update_device(struct srbd_pgg* d_pgg, struct srbd_frg* d_frg, struct srbd_terrain_est* d_terrain,
                          float* d_contact, int32_t* d_rising_edge, int32_t num_envs, const srbd_wb_update_io* io,
                          void* hip_stream);

/* Diagnostic: enable != 0 stamps the phases of the following TAMOLS calls; out_us[5] (may be NULL)
 * receives the last call's mean per-block durations of (patch, queries, scores, slice argmin + count)
 * and the span from the first block's start to the last leg's end, in us.  enable == 0 turns it off. */
int srbd_tamols_phases(srbd_tamols_ctx* ctx, int32_t enable, float* out_us);
/* Diagnostic: the last call's raw stamps, 4 legs x 16 blocks x 8 uint64 (100 MHz). */
int srbd_tamols_phases_raw(srbd_tamols_ctx* ctx, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SRBD_MPC_H */
