// srbd_vfa.h -- the apex gate around the foothold search: when the loop searches, when it holds the last search's
// footholds and when it passes the seeds through, and what each of the three leaves in the state.  Plain functions
// compiled by the host C++ (srbd_host.cpp srbd_vfa_*) and by the HIP kernel (tamols_kernel.hip
// tamols_batch_kernel<true>, srbd_vfa_step_device), so both sides leave the same bytes: the state machine is
// comparisons and copies, and its only arithmetic is srbd_stc.h's apex window (float64, unfused).
//   WBI = quadruped_pympc/interfaces/wb_interface.py (the gate :230-246)
//   VFA = quadruped_pympc/helpers/visual_foothold_adaptation.py (update_footholds_adaptation :59-61, reset :63-64,
//         get_footholds_adapted :66-72, the per-leg stores of compute_adaptation :193-228)
//   STC = quadruped_pympc/helpers/swing_trajectory_controller.py (check_apex_condition :129-138,
//         check_full_stance_condition :140-146)
// The reference's three statements, and the mode each path gets here:
//   if apex and not initialized: compute_adaptation      SEARCH: initialized = 1, the search's footholds are stored
//   if full stance: reset                                PASS (with the last line): initialized = 0
//   get_footholds_adapted                                PASS stores and returns the seeds; HOLD and SEARCH return
//                                                        footholds_adaptation
// An apex needs a leg in swing (contact == 0) and full stance needs none, so SEARCH and the reset never coincide: a
// step is exactly one of the three, and after a SEARCH the same step's get_footholds_adapted returns what the search
// stored.
// The conditions are formed on the swing clocks as the last leg-controller step left them (WBI:232 runs before this
// step's update_swing_time, WBI:369).
// Stale constraint: VFA:209-222 assigns footholds_constraints[leg] only for a leg with a feasible candidate, and
// neither reset nor get_footholds_adapted touches it, so an infeasible leg keeps the box of its last feasible search
// (NaN here where the reference still holds None) while its foothold is the seed at its terrain height (VFA:223-228).
// The 'height' strategy's search (VFA:145-151: each seed's z becomes its patch's nearest-point height + 0.02) is stated
// here too, vfa_height_*, for the host twin srbd_vfa_height_search and the kernel of srbd_vfa_height_step_device
// (vfa_height_kernel.hip): the gate and the commit around it are the ones above.
// Out of scope: the 'vfa' strategy; the early-stance detector and inverse kinematics (start-and-stop is
// the gait generator's, srbd_start_stop.h);
// compacting the searching environments into a smaller grid (the count would have to reach the host).  The
// per-environment reset of this state is srbd_reset.h's.
#pragma once

#include <stdint.h>

#include "../../include/srbd_host.h"
#include "srbd_stc.h"

namespace srbd {

// The step's mode for a state whose `initialized` word is `initialized` (WBI:232, :243).  contact: a leg is in swing
// iff its flag == 0 (STC's comparison; a NaN flag is neither swing nor, for full stance, a reason to deny it).
YAW_HD inline int32_t vfa_mode(int32_t initialized, const srbd_stc* stc, const double* contact, double interval) {
    if (initialized == 0)
        return stc_apex(stc->swing_time, stc->swing_period, contact, interval) ? SRBD_VFA_SEARCH : SRBD_VFA_PASS;
    return stc_full_stance(contact) ? SRBD_VFA_PASS : SRBD_VFA_HOLD;
}

// One of a leg's ten slots -- d = 0..2 the foothold's coordinates, 3..8 the box's, 9 the two words valid and
// initialized -- so that a kernel may give each slot a lane of its own: the slots share nothing.  seed: the leg's 3
// doubles; sf / sb / sv: the leg's searched foothold (3), box (6) and validity, read only in SEARCH.  out_f (3),
// out_b (6), out_v (1): the leg's returned values, the state's after the store.  Returns the foothold coordinate for
// d < 3 (what the reference row's feet receive), else 0.
YAW_HD inline double vfa_commit_slot(srbd_vfa* g, int leg, int32_t mode, int d, const double* seed, const double* sf,
                                     const double* sb, int32_t sv, double* out_f, double* out_b, int32_t* out_v) {
    if (d < 3) {
        double* f = g->footholds + 3 * leg + d;
        // VFA:59-61 the search's result, VFA:68-70 the seed, else what is held
        const double v = mode == SRBD_VFA_SEARCH ? sf[d] : mode == SRBD_VFA_PASS ? seed[d] : *f;
        if (mode != SRBD_VFA_HOLD) *f = v;
        out_f[d] = v;
        return v;
    }
    if (d < 9) {
        double* b = g->boxes + 6 * leg + (d - 3);
        const bool store = mode == SRBD_VFA_SEARCH && sv != 0;  // VFA:209-222: a feasible leg only
        const double v = store ? sb[d - 3] : *b;
        if (store) *b = v;
        out_b[d - 3] = v;
        return 0.0;
    }
    if (mode == SRBD_VFA_SEARCH) {
        g->valid[leg] = sv;
        g->initialized[leg] = 1;
        *out_v = sv;
    } else {
        if (mode == SRBD_VFA_PASS) g->initialized[leg] = 0;  // VFA:63-64, or already 0
        *out_v = g->valid[leg];
    }
    return 0.0;
}

// The whole leg: its ten slots in order.  Unrolled, so that the slot index is a constant in each copy: a caller's
// sf / sb held in registers (the kernel's search result) then stay there instead of going through scratch memory.
YAW_HD inline void vfa_commit_leg(srbd_vfa* g, int leg, int32_t mode, const double* seed, const double* sf,
                                  const double* sb, int32_t sv, double* out_f, double* out_b, int32_t* out_v) {
#pragma unroll
    for (int d = 0; d < 10; ++d) vfa_commit_slot(g, leg, mode, d, seed, sf, sb, sv, out_f, out_b, out_v);
}

YAW_HD inline bool vfa_mode_ok(int32_t mode) {
    return mode == SRBD_VFA_PASS || mode == SRBD_VFA_SEARCH || mode == SRBD_VFA_HOLD;
}

// The four replicated words agree (what the host calls refuse otherwise).
YAW_HD inline bool vfa_struct_ok(const srbd_vfa* g) {
    return g->initialized[0] == g->initialized[1] && g->initialized[0] == g->initialized[2] &&
           g->initialized[0] == g->initialized[3];
}

// ---- the 'height' strategy: the seed at the height of its patch's nearest point (PatchHeightMap.get_height)
// Squared xy distance of patch point (x, y) from the seed (sx, sy): float64, unfused, the one expression both sides
// evaluate.
YAW_HD inline double vfa_height_d2(double x, double y, double sx, double sy) {
#pragma clang fp contract(off)
    const double dx = x - sx, dy = y - sy;
    return dx * dx + dy * dy;
}

// numpy.argmin's order on (distance, index) pairs: does (da, ia) come before (db, ib)?  A NaN distance comes before
// every number, and among equals (two NaNs, two equal numbers) the lower index: a total order, so the minimum may be
// folded in any grouping -- the host's serial scan and the kernel's wave shuffles find the same point.
YAW_HD inline bool vfa_height_before(double da, int ia, double db, int ib) {
    const bool na = da != da, nb = db != db;
    if (na != nb) return na;
    if (na) return ia < ib;
    return da < db || (da == db && ia < ib);
}

// The index of the nearest of a patch's n points (x, y, z triples) to the seed, serially.
YAW_HD inline int vfa_height_nearest(const double* patch, int n, double sx, double sy) {
    int bi = 0;
    double bd = vfa_height_d2(patch[0], patch[1], sx, sy);
    for (int i = 1; i < n; ++i) {
        const double d = vfa_height_d2(patch[3 * i], patch[3 * i + 1], sx, sy);
        if (vfa_height_before(d, i, bd, bi)) {
            bd = d;
            bi = i;
        }
    }
    return bi;
}

// The leg's foothold from its nearest point's height z: the seed's x and y, z + 0.02; a ray that missed on a scene
// whose miss_z is NaN gives a NaN height and valid 0.
YAW_HD inline void vfa_height_result(double sx, double sy, double z, double* foothold, int32_t* valid) {
    foothold[0] = sx;
    foothold[1] = sy;
    foothold[2] = z + 0.02;
    *valid = z != z ? 0 : 1;
}

}  // namespace srbd
