// srbd_enqueue.h -- what every producer launch of the device-resident loop shares (srbd_producers.hip,
// reflex_kernel.hip): the block size and grid of the one-lane-per-(environment, leg) kernels, the range of num_envs,
// how the caller's stream handle is read and how a launch's outcome becomes a return code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srbd_mpc.h"

namespace srbd {

constexpr int PROD_BLOCK = 256;
constexpr int PROD_MAX_ENVS = 4096;  // srbd_batch_create's range

// NULL and hipStreamLegacy both name the legacy null stream: there is no batch here to own one.
inline hipStream_t stream_of(void* hip_stream) {
    hipStream_t s = (hipStream_t)hip_stream;
    return s == hipStreamLegacy ? nullptr : s;
}

inline int launch_status() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SRBD_OK;
    int ndev = 0;
    return (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) ? SRBD_E_NODEVICE : SRBD_E_HIP;
}

inline unsigned blocks_of(int E) { return (unsigned)((4 * E + PROD_BLOCK - 1) / PROD_BLOCK); }

inline bool envs_ok(int32_t E) { return E >= 1 && E <= PROD_MAX_ENVS; }

}  // namespace srbd
