// Stand-alone ASan + UBSan driver of the batch C-ABI's refusal paths (srbd_batch_*; include/srbd_mpc.h,
// csrc/srbd_api_batch.hip): the ones that return before any device work, so the program runs on the CPU.  They and
// their error texts are what crosses the boundary between srbd_api_batch.hip and srbd_api.hip (fail, the calling
// thread's error text, build_model).  Linked against the sanitizer build of the library (make asan):
//
//   cd quadruped-pympc-tamols_amd && make asan && /opt/rocm/bin/hipcc -O1 -g -std=c++17 -x c++ \
//       -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       -shared-libsan ../scripts/batch_api_host_sanitize.cpp -o build/batch_api_host_sanitize \
//       -Lquadruped_pympc_amd -l:libsrbd_hip_asan.so -Wl,-rpath,'$ORIGIN/../quadruped_pympc_amd' \
//       -Wl,-rpath,"$(dirname "$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)")" && \
//       build/batch_api_host_sanitize
//
// (-shared-libsan: the library was linked against the shared sanitizer runtime, and a process holds one runtime.)
//
// Every io structure is heap-allocated at its exact size and every pointer in it points at one heap word: the refusals
// look at the pointers and never through them.  A NULL batch, a NULL io, each required pointer by name, num_envs 0
// and 4097, CEM-MPPI through srbd_batch_create (and MPPI through srbd_batch_create_cem), a sharded configuration and a
// configuration build_model turns away; the code and the text each leaves are checked.  Exit status 0 and "ok" when
// nothing fired.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>

#include "../include/srbd_mpc.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

// the calling thread's error text (what a NULL batch leaves)
static bool said(const char* want) { return !strcmp(srbd_batch_last_error(nullptr), want); }
static bool said(const std::string& want) { return said(want.c_str()); }

int main() {
    std::unique_ptr<uint64_t> word(new uint64_t(0));
    void* const w = word.get();

    // ---- srbd_batch_create / srbd_batch_create_cem
    auto cfg = std::make_unique<srbd_config>();
    memset(cfg.get(), 0, sizeof(srbd_config));
    cfg->num_samples = 64, cfg->horizon = 12, cfg->method = SRBD_MPPI, cfg->parametrization = SRBD_ZERO_ORDER;
    cfg->world_size = 1, cfg->mass = 12.0f, cfg->mg = 117.72f, cfg->grf_max = 200.0f, cfg->mu = 0.5f;
    cfg->inertia[0] = cfg->inertia[4] = cfg->inertia[8] = 0.1f;
    for (float& d : cfg->dts) d = 0.02f;
    srbd_batch* b = reinterpret_cast<srbd_batch*>(w);
    CHECK(srbd_batch_create(nullptr, 1, &b) == SRBD_E_INVALID && said("null argument"));
    CHECK(srbd_batch_create(cfg.get(), 1, nullptr) == SRBD_E_INVALID && said("null argument"));
    for (int n : {0, 4097, -1}) {
        b = reinterpret_cast<srbd_batch*>(w);
        CHECK(srbd_batch_create(cfg.get(), n, &b) == SRBD_E_INVALID && b == nullptr);
        CHECK(said("num_envs must be in [1, 4096]"));
        b = reinterpret_cast<srbd_batch*>(w);
        CHECK(srbd_batch_create_cem(cfg.get(), n, &b) == SRBD_E_INVALID && b == nullptr);
        CHECK(said("num_envs must be in [1, 4096]"));
    }
    cfg->num_samples = 16385;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID);
    const char* const too_many = "num_samples per environment must be <= 16384 (256 leaves, what one merge block folds)";
    CHECK(!strncmp(srbd_batch_last_error(nullptr), too_many, strlen(too_many)));
    cfg->num_samples = 64;
    cfg->method = SRBD_CEM_MPPI;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID && b == nullptr);
    CHECK(said("srbd_batch_create does not take CEM-MPPI (sigma is part of every step): create the batch with "
               "srbd_batch_create_cem and step it with srbd_batch_step_cem / srbd_batch_step_cem_device"));
    cfg->method = SRBD_MPPI;
    CHECK(srbd_batch_create_cem(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_create_cem takes method SRBD_CEM_MPPI only: MPPI and random sampling go through "
               "srbd_batch_create"));
    cfg->world_size = 2;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("a batch is unsharded: rank / world_size must be 0 / 1"));
    cfg->world_size = 1, cfg->rank = 1;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("a batch is unsharded: rank / world_size must be 0 / 1"));
    cfg->rank = 0;
    // build_model's refusals (srbd_api.hip) through the batch file's fail
    cfg->horizon = 0;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("unsupported horizon/parametrization/num_splines"));
    cfg->horizon = 12, cfg->grf_min = 300.0f;
    CHECK(srbd_batch_create(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("need 0 <= grf_min <= grf_max and mu >= 0"));
    cfg->grf_min = 0.0f, cfg->method = SRBD_CEM_MPPI, cfg->num_elite = 1;
    CHECK(srbd_batch_create_cem(cfg.get(), 2, &b) == SRBD_E_INVALID);
    CHECK(said("num_elite must be in [2, SRBD_MAX_ELITE] (sample variance over the elite set)"));
    // the same thread's text through the single context's reader: one text behind both
    CHECK(!strcmp(srbd_last_error(nullptr), srbd_batch_last_error(nullptr)));

    // ---- a NULL batch where no text is promised
    CHECK(srbd_batch_num_envs(nullptr) == SRBD_E_INVALID);
    CHECK(srbd_batch_set_rng(nullptr, SRBD_RNG_PHILOX) == SRBD_E_INVALID);
    CHECK(srbd_batch_set_gait(nullptr, nullptr, 0.0f, 0.0f, nullptr, 1, nullptr) == SRBD_E_INVALID);
    CHECK(srbd_batch_clear_gait(nullptr) == SRBD_E_INVALID);
    CHECK(srbd_batch_set_cost_terms(nullptr, nullptr, 0.0f, 0.0f) == SRBD_E_INVALID);
    CHECK(srbd_batch_copy_costs(nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(srbd_batch_step(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == SRBD_E_INVALID);
    CHECK(srbd_batch_step_cem(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr) == SRBD_E_INVALID);
    srbd_batch_destroy(nullptr);
    // ---- and where one is
    CHECK(srbd_batch_set_env_params(nullptr, nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_env_params: null batch"));
    CHECK(srbd_batch_set_env_params_device(nullptr, nullptr, nullptr, nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_env_params_device: null batch"));
    CHECK(srbd_batch_get_env_params(nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_get_env_params: null batch"));
    CHECK(srbd_batch_clear_env_params(nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_clear_env_params: null batch"));

    // ---- the device steps: the arguments are looked at before the batch
    auto io = std::make_unique<srbd_batch_device_io>();
    memset(io.get(), 0, sizeof(*io));
    auto cem = std::make_unique<srbd_batch_cem_io>();
    cem->sigma = (float*)w, cem->sigma_reset = 0.0f, cem->pad = 0;
    CHECK(srbd_batch_step_device(nullptr, nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_step_device: null io"));
    CHECK(srbd_batch_step_cem_device(nullptr, nullptr, cem.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_step_cem_device: null io"));
    CHECK(srbd_batch_step_cem_device(nullptr, io.get(), nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_step_cem_device: null cem"));
    cem->sigma = nullptr;
    CHECK(srbd_batch_step_cem_device(nullptr, io.get(), cem.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_step_cem_device: null required pointer: sigma"));
    cem->sigma = (float*)w, cem->sigma_reset = NAN;
    CHECK(srbd_batch_step_cem_device(nullptr, io.get(), cem.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_step_cem_device: sigma_reset must be finite and >= 0"));
    cem->sigma_reset = 0.0f;
    {  // each required pointer by name, in the order the table lists them
        const struct {
            const void** p;
            const char* name;
        } req[] = {{(const void**)&io->states, "states"},
                   {(const void**)&io->refs, "refs"},
                   {(const void**)&io->contacts, "contacts"},
                   {(const void**)&io->seeds, "seeds"},
                   {(const void**)&io->counters, "counters"},
                   {(const void**)&io->best_params, "best_params"},
                   {(const void**)&io->grf, "grf"},
                   {(const void**)&io->predicted_state, "predicted_state"},
                   {(const void**)&io->best_cost, "best_cost"},
                   {(const void**)&io->best_index, "best_index"},
                   {(const void**)&io->best_freq, "best_freq"},
                   {(const void**)&io->status, "status"}};
        for (const auto& r : req) {  // everything before r set, r and everything after it NULL: r is the first
            CHECK(srbd_batch_step_device(nullptr, io.get(), nullptr) == SRBD_E_INVALID);
            CHECK(said(std::string("srbd_batch_step_device: null required pointer: ") + r.name));
            CHECK(srbd_batch_step_cem_device(nullptr, io.get(), cem.get(), nullptr) == SRBD_E_INVALID);
            CHECK(said(std::string("srbd_batch_step_cem_device: null required pointer: ") + r.name));
            *r.p = w;
        }
        // noise and costs are optional: with the rest set it is the batch that is missing
        CHECK(srbd_batch_step_device(nullptr, io.get(), nullptr) == SRBD_E_INVALID);
        CHECK(said("srbd_batch_step_device: null batch"));
        CHECK(srbd_batch_step_cem_device(nullptr, io.get(), cem.get(), nullptr) == SRBD_E_INVALID);
        CHECK(said("srbd_batch_step_cem_device: null batch"));
        *req[9].p = nullptr;  // one in the middle of an otherwise full table
        CHECK(srbd_batch_step_device(nullptr, io.get(), nullptr) == SRBD_E_INVALID);
        CHECK(said("srbd_batch_step_device: null required pointer: best_index"));
    }

    // ---- the device gait setter
    auto gio = std::make_unique<srbd_batch_gait_io>();
    memset(gio.get(), 0, sizeof(*gio));
    CHECK(srbd_batch_set_gait_device(nullptr, nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_gait_device: null io"));
    CHECK(srbd_batch_set_gait_device(nullptr, gio.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_gait_device: null required pointer: optimize"));
    gio->optimize = (const int32_t*)w;
    CHECK(srbd_batch_set_gait_device(nullptr, gio.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_gait_device: exactly one of pgg and timings must be given"));
    gio->timings = (const float*)w;
    CHECK(srbd_batch_set_gait_device(nullptr, gio.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_gait_device: timings need nominal_freqs"));
    gio->nominal_freqs = (const float*)w;
    for (int n : {0, SRBD_MAX_FREQS + 1}) {
        gio->n_freq = n;
        CHECK(srbd_batch_set_gait_device(nullptr, gio.get(), nullptr) == SRBD_E_INVALID);
        CHECK(said("n_freq must be in [1, " + std::to_string(SRBD_MAX_FREQS) + "]"));
    }
    gio->n_freq = 1;
    CHECK(srbd_batch_set_gait_device(nullptr, gio.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_set_gait_device: null batch"));

    // ---- the interface step looks at the batch first
    auto iio = std::make_unique<srbd_batch_interface_io>();
    memset(iio.get(), 0, sizeof(*iio));
    CHECK(srbd_batch_interface_step_device(nullptr, iio.get(), nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_interface_step_device: null batch"));
    CHECK(srbd_batch_interface_step_device(nullptr, nullptr, nullptr) == SRBD_E_INVALID);
    CHECK(said("srbd_batch_interface_step_device: null batch"));
    printf("ok\n");
    return 0;
}
