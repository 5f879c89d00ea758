// srbd_reset.h -- restarting one environment of the batched loop: the statements of the reference's reset at its two
// levels, per struct.  Plain functions compiled by the host C++ (srbd_host.cpp srbd_loop_reset, and the constructors
// and resets they share: srbd_pgg_reset, srbd_frg_init, srbd_vfa_reset) and by the HIP kernel (srbd_producers.hip
// loop_reset_kernel, srbd_loop_reset_device), so both sides leave the same bytes: the reset is copies and constants,
// there is no arithmetic in it.
//   SIM = simulation/simulation.py (the episode's end :773-781: env.reset, quadrupedpympc_wrapper.reset)
//   WBI = quadruped_pympc/interfaces/wb_interface.py (reset :469-484)
//   PGG = quadruped_pympc/helpers/periodic_gait_generator.py (reset :22-46)
//   FRG = quadruped_pympc/helpers/foothold_reference_generator.py (__init__ :15-51)
//   VFA = quadruped_pympc/helpers/visual_foothold_adaptation.py (reset :63-64)
// Two levels:
//   SRBD_RESET_REFERENCE  WBI:469-484 statement for statement: pgg.reset() (step_freq is left alone), frg.lift_off =
//                         the new feet (that table only; the reference has the other resets commented out),
//                         vfa.reset(), current_contact = [1, 1, 1, 1] (the caller's rows, see loop_reset_contact).
//   SRBD_RESET_EPISODE    every struct becomes what its constructor call produced: the bytes of a snapshot taken when
//                         the loop was built, and for the foothold generator srbd_frg_init on the new feet with the
//                         snapshot's three scalars; the touch-down trigger word and the warm-start row are cleared.
//                         The reference never needs this, one process being one robot; a batch does, so that a
//                         restarted episode does not inherit the last one's velocity history and swing clocks.
// A work item is a (first, step) pair: the host walks every index (0, 1), a wave gives lane l the indices l, l + 64, ..
// (l, 64).  Every struct's size is a multiple of 8 and its arrays are 8-byte aligned, so a struct is moved as 8-byte
// words.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "yaw_sincos.h"

namespace srbd {

typedef uint64_t __attribute__((may_alias)) reset_word;

static_assert(sizeof(srbd_pgg) % 8 == 0 && sizeof(srbd_frg) % 8 == 0 && sizeof(srbd_stc) % 8 == 0 &&
                  sizeof(srbd_terrain_est) % 8 == 0 && sizeof(srbd_vfa) % 8 == 0,
              "the structs are moved as 8-byte words");
constexpr int FRG_WORDS = (int)(sizeof(srbd_frg) / 8);
constexpr int FRG_TABLES_FIRST = (int)(offsetof(srbd_frg, lift_off) / 8);                 // the four position tables,
constexpr int FRG_TABLES_END = (int)(offsetof(srbd_frg, last_reference_footholds) / 8);   // 12 words each
static_assert(FRG_TABLES_FIRST == 3 && FRG_TABLES_END == FRG_TABLES_FIRST + 48, "srbd_frg layout");

// The mask word of srbd_loop_reset_device: 0 not reset, 2 the episode reset, anything else the reference's reset.
YAW_HD inline int32_t loop_reset_level(int32_t mask) {
    return mask == 0 ? 0 : mask == SRBD_RESET_EPISODE ? SRBD_RESET_EPISODE : SRBD_RESET_REFERENCE;
}

// PGG:24-41: leg l's phase offset for a gait type.
YAW_HD inline double pgg_gait_offset(int32_t gait, int l) {
    const double tab[8][4] = {{0.5, 1.0, 1.0, 0.5},   {0.8, 0.3, 0.8, 0.3},   {0.5, 0.5, 0.0, 0.0},
                              {0.0, 0.25, 0.75, 0.5}, {0.0, 0.25, 0.5, 0.75}, {0.0, 0.5, 0.75, 0.25},
                              {0.5, 1.0, 0.75, 1.25}, {0.0, 0.5, 0.5, 0.0}};
    return tab[(gait >= 0 && gait < 7) ? gait : 7][l];
}

// PGG:22-46 for one leg: the offset from the gait type, the phase back to it, the start-up hold cleared.
YAW_HD inline void pgg_reset_leg(srbd_pgg* g, int l) {
    const double off = pgg_gait_offset(g->gait_type, l);
    g->phase_offset[l] = off;
    g->phase_signal[l] = off;
    g->init[l] = 0;
}

// VFA:63-64 for one leg's replicated word.
YAW_HD inline void vfa_reset_leg(srbd_vfa* g, int l) { g->initialized[l] = 0; }

YAW_HD inline uint64_t reset_bits(double v) { return (uint64_t)__builtin_bit_cast(uint64_t, v); }

// Word i of the struct FRG:15-51 builds: the three scalars; the four position tables as copies of the feet (the _h
// tables too: the reference's "TODO wrong", reproduced); last_reference_footholds, the velocity ring and its two
// counters zero.
YAW_HD inline uint64_t frg_init_word(int i, double stance_time, double hip_height, double hip_offset,
                                     const double* feet /* 4 x 3 */) {
    if (i == 0) return reset_bits(stance_time);
    if (i == 1) return reset_bits(hip_height);
    if (i == 2) return reset_bits(hip_offset);
    if (i < FRG_TABLES_END) return reset_bits(feet[(i - FRG_TABLES_FIRST) % 12]);
    return 0;
}

YAW_HD inline void frg_init_words(srbd_frg* g, double stance_time, double hip_height, double hip_offset,
                                  const double* feet, int first, int step) {
    reset_word* w = reinterpret_cast<reset_word*>(g);
    for (int i = first; i < FRG_WORDS; i += step) w[i] = frg_init_word(i, stance_time, hip_height, hip_offset, feet);
}

YAW_HD inline void reset_copy_words(void* dst, const void* src, int words, int first, int step) {
    reset_word* d = static_cast<reset_word*>(dst);
    const reset_word* s = static_cast<const reset_word*>(src);
    for (int i = first; i < words; i += step) d[i] = s[i];
}

// One environment's pointers: its own structs (each may be NULL: not part of the caller's loop), their snapshots, its
// 12 new feet, its trigger word and its warm-start row.
struct LoopResetEnv {
    const double* __restrict__ feet;
    srbd_pgg* __restrict__ pgg;
    srbd_frg* __restrict__ frg;
    srbd_stc* __restrict__ stc;
    srbd_terrain_est* __restrict__ terr;
    srbd_vfa* __restrict__ vfa;
    const srbd_pgg* __restrict__ pgg0;
    const srbd_frg* __restrict__ frg0;
    const srbd_stc* __restrict__ stc0;
    const srbd_terrain_est* __restrict__ terr0;
    const srbd_vfa* __restrict__ vfa0;
    int32_t* __restrict__ rising_edge;
    float* __restrict__ best;
    int32_t num_params;
};

// What both callers refuse, as a message (NULL: nothing to refuse).  level < 0: the level is not known (the device
// call, whose levels are in device memory), so every given struct needs its snapshot.
YAW_HD inline const char* loop_reset_refusal(const LoopResetEnv& x, int32_t level) {
    if (level >= 0 && level != SRBD_RESET_REFERENCE && level != SRBD_RESET_EPISODE) return "level must be 1 or 2";
    if (x.frg && !x.feet) return "frg is given without initial_feet";
    if (level != SRBD_RESET_REFERENCE &&
        ((x.pgg && !x.pgg0) || (x.frg && !x.frg0) || (x.stc && !x.stc0) || (x.terr && !x.terr0) || (x.vfa && !x.vfa0)))
        return "a struct is given without its snapshot";
    if (x.best && x.num_params < 1) return "best_params is given with num_params < 1";
    return nullptr;
}

// The reset of one environment at `level` (SRBD_RESET_REFERENCE or SRBD_RESET_EPISODE), work item (first, step).
YAW_HD inline void loop_reset_env(const LoopResetEnv& x, int32_t level, int first, int step) {
    if (level == SRBD_RESET_EPISODE) {
        if (x.pgg) reset_copy_words(x.pgg, x.pgg0, (int)(sizeof(srbd_pgg) / 8), first, step);
        if (x.stc) reset_copy_words(x.stc, x.stc0, (int)(sizeof(srbd_stc) / 8), first, step);
        if (x.terr) reset_copy_words(x.terr, x.terr0, (int)(sizeof(srbd_terrain_est) / 8), first, step);
        if (x.vfa) reset_copy_words(x.vfa, x.vfa0, (int)(sizeof(srbd_vfa) / 8), first, step);
        if (x.frg)
            frg_init_words(x.frg, x.frg0->stance_time, x.frg0->hip_height, x.frg0->hip_offset, x.feet, first, step);
        if (x.rising_edge && first == 0) *x.rising_edge = 0;
        if (x.best)
            for (int i = first; i < x.num_params; i += step) x.best[i] = 0.0f;
        return;
    }
    for (int k = first; k < 12; k += step) {  // WBI:469-484
        if (x.pgg && k < 4) pgg_reset_leg(x.pgg, k);           // self.pgg.reset()
        if (x.frg) x.frg->lift_off[k / 3][k % 3] = x.feet[k];  // self.frg.lift_off_positions = initial_feet_pos
        if (x.vfa && k < 4) vfa_reset_leg(x.vfa, k);           // self.vfa.reset()
    }
}

// self.current_contact = np.array([1, 1, 1, 1]) (WBI:483) on one of the caller's float32 contact rows, both levels.
YAW_HD inline void loop_reset_contact(float* row, int first, int step) {
    for (int k = first; k < 4; k += step) row[k] = 1.0f;
}

}  // namespace srbd
