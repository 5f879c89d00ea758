// srbd_iface.h -- the per-iteration key schedule of the controller interface's step, for host and device.
//
// Reference (paths relative to the reference repository root; SCI = quadruped_pympc/interfaces/
// srbd_controller_interface.py, NMPC = quadruped_pympc/controllers/sampling/centroidal_nmpc_jax.py):
//   self.controller = self.controller.with_newkey()   SCI:128, once per sampling iteration
//   master_key <- jax.random.split(master_key)[0]     NMPC:498-501
// srbd_interface_step (srbd_host.cpp) states it for one context; this is that statement as one function, which the
// prologue kernel of srbd_batch_interface_step_device (srbd_producers.hip iface_prologue_kernel) and the host twin
// srbd_selftest_interface_keys both run:
//   RNG_PHILOX             key = (seed, counter): counter + 1 (uint64, wrapping); the step runs (seed, counter)
//   RNG_JAX / _JAX_LEGACY  key = (packed JAX key, call count): key <- split(key)[0] in the stream's counter layout
//                          (srbd_jaxrng.h jax_next_key), call count + 1; the step runs (packed key, call count)
#pragma once

#include "srbd_jaxrng.h"

namespace srbd {

constexpr int IFACE_MAX_ITERS = 8;  // == SRBD_MAX_IFACE_ITERS (include/srbd_mpc.h)

// One with_newkey: (k0, k1) in / out; afterwards they are also the (seed, counter) the iteration's step runs.
SRBD_HD void iface_next_key(int rng, uint64_t& k0, uint64_t& k1) {
    if (rng != RNG_PHILOX) k0 = jax_next_key(k0, rng == RNG_JAX);
    k1 += 1;
}

}  // namespace srbd
