// Stand-alone ASan + UBSan driver of the host twin of the batch interface step's key schedule
// (srbd_selftest_interface_keys; include/srbd_mpc.h, csrc/srbd_iface.h).  Host code only, run on the CPU:
//
//   cd quadruped-pympc-tamols_amd && mkdir -p build && /opt/rocm/bin/hipcc -O1 -g -std=c++17 -ffp-contract=off -x c++ \
//       -ffunction-sections -Wl,--gc-sections \
//       -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       ../scripts/batch_interface_host_sanitize.cpp csrc/srbd_host.cpp -o build/batch_interface_host_sanitize && \
//       build/batch_interface_host_sanitize
//
// (srbd_host.cpp also holds the plugin-API glue, which calls into the device library; --gc-sections drops those
// functions, which nothing here references, so the program links without it.)
//
// keys_io and step_keys are heap-allocated at their exact sizes (n x 2 and iterations x n x 2 words), so a read or
// write past either is a report.  Every stream, iterations 1..8, n = 1 and 65, keys 0, all ones and a counter at
// 2^64 - 1; the results are checked against srbd_jax_split and counter + 1, then every refusal.  Exit status 0 and
// "ok" when nothing fired.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "../include/srbd_host.h"
#include "../include/srbd_mpc.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    const uint64_t ones = ~0ull;
    const uint64_t edge[5][2] = {{0, 0}, {ones, ones}, {42, ones}, {ones, 0}, {0x0123456789ABCDEFull, 7}};
    for (int rng = SRBD_RNG_PHILOX; rng <= SRBD_RNG_JAX_LEGACY; ++rng)
        for (int it = 1; it <= SRBD_MAX_IFACE_ITERS; ++it)
            for (int n : {1, 65})
                for (int shift = 0; shift < (n == 1 ? 5 : 1); ++shift) {
                    std::unique_ptr<uint64_t[]> keys(new uint64_t[2 * (size_t)n]);
                    std::unique_ptr<uint64_t[]> k0(new uint64_t[2 * (size_t)n]);
                    std::unique_ptr<uint64_t[]> steps(new uint64_t[2 * (size_t)n * it]);
                    for (int e = 0; e < n; ++e) {
                        const int j = (e + shift) % 5;
                        keys[2 * e] = e < 5 ? edge[j][0] : 0x9E3779B97F4A7C15ull * (uint64_t)(e + 1);
                        keys[2 * e + 1] = e < 5 ? edge[j][1] : (uint64_t)e * 3;
                    }
                    memcpy(k0.get(), keys.get(), sizeof(uint64_t) * 2 * n);
                    CHECK(srbd_selftest_interface_keys(keys.get(), n, rng, it, steps.get()) == SRBD_OK);
                    for (int e = 0; e < n; ++e) {
                        uint64_t a = k0[2 * e], b = k0[2 * e + 1];
                        for (int i = 0; i < it; ++i) {
                            if (rng != SRBD_RNG_PHILOX) {
                                const uint32_t k[2] = {(uint32_t)(a >> 32), (uint32_t)a};
                                uint32_t o[4];
                                CHECK(srbd_jax_split(k, 2, rng == SRBD_RNG_JAX ? 1 : 0, o) == SRBD_OK);
                                a = ((uint64_t)o[0] << 32) | o[1];
                            }
                            b += 1;
                            CHECK(steps[2 * ((size_t)i * n + e)] == a && steps[2 * ((size_t)i * n + e) + 1] == b);
                        }
                        CHECK(keys[2 * e] == a && keys[2 * e + 1] == b);
                    }
                }
    uint64_t k[2] = {1, 2}, s[2 * SRBD_MAX_IFACE_ITERS] = {0};
    CHECK(srbd_selftest_interface_keys(nullptr, 1, 0, 1, s) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 1, 0, 1, nullptr) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 0, 0, 1, s) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 1, 3, 1, s) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 1, -1, 1, s) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 1, 0, 0, s) == SRBD_E_INVALID);
    CHECK(srbd_selftest_interface_keys(k, 1, 0, SRBD_MAX_IFACE_ITERS + 1, s) == SRBD_E_INVALID);
    CHECK(k[0] == 1 && k[1] == 2 && s[0] == 0);
    printf("ok\n");
    return 0;
}
