// srbd_gait_adapt.h -- the gait adaptation loop around the gait-adaptive sampler (mpc_params['optimize_step_freq']):
// the touch-down trigger that decides when to optimise the step frequency, the write-back of the sampler's best
// frequency into the gait generator, the foothold reference generator and the swing controller, and the gait fields
// of one StepInput.  Plain functions compiled by the host C++ (srbd_host.cpp srbd_stc_touch_down,
// srbd_gait_apply_freq; srbd_api.hip fill_gait) and by the HIP kernels (srbd_producers.hip touch_down_kernel,
// gait_apply_freq_kernel; srbd_batch.hip batch_set_gait_kernel), so both sides leave the same bytes.
//   STC = quadruped_pympc/helpers/swing_trajectory_controller.py (check_touch_down_condition :148-165)
//   WBI = quadruped_pympc/interfaces/wb_interface.py (the trigger's call :298, the write-back :354-358)
//   GA  = quadruped_pympc/controllers/sampling/centroidal_nmpc_jax_gait_adaptive.py (the candidate set :687-692
//         random sampling, :834-838 MPPI)
//
// Write-back arithmetic (WBI:355-358).  best_sample_freq reaches WBI:355 as a float32 scalar, and
// `np.array([best_sample_freq])[0]` keeps it one, so pgg.step_freq becomes a numpy.float32.  The recorded fixture
// (tests/golden/gait_adapt_ref.npz) was made under NumPy 2.2.6, i.e. under NEP 50 promotion ("weak" Python scalars: a
// Python int or float meeting a float32 scalar is converted to float32, it does not widen the result):
//   inv          = float32(1) / f                      `1 / self.pgg.step_freq`, one float32 division
//   stance_time  = inv * float32(duty)                 `(1 / f) * duty`, duty rounded to float32, one float32 product
//   swing_period = float32(1.0 - duty) * inv           `1 - duty` formed in double first (two Python floats), then
//                                                      rounded to float32, one float32 product
// The three float32 results are widened exactly to the structs' doubles.  Under NumPy 1.x (value-based promotion of
// scalars) the same lines give float32 too; under a float64 best_sample_freq they would be double products, which is
// not what the sampler returns.
// Refused values: a best_freq that is zero, negative or not finite (NaN included), or a duty factor for which the
// swing period is not positive and finite (what srbd_stc_set_timing refuses), leaves all three structs untouched.
// The reference would divide by it and store inf, a negative time or NaN.
// Deviation, not changed here: after the first write-back the reference's pgg.step_freq is a numpy.float32, so under
// NumPy 2 its `dt * new_step_freq` (PGG:53) is a float32 product added to the float64 phase.  srbd_pgg_run and
// srbd_pgg_run_device keep the float64 product dt * step_freq with step_freq the exactly widened float32: the phase
// increments agree to float32 rounding (relative 6e-8), not to the bit.
#pragma once

#include <stdint.h>

#include "../../include/srbd_host.h"
#include "../../include/srbd_mpc.h"
#include "yaw_sincos.h"

namespace srbd {

// STC:148-165, statement for statement.  T is the contacts' element type (double on the host, float32 on the device:
// the values compared are 0 and 1, exact in both).  seq is 4 x stride, row l at seq + l * stride.  The caller has
// checked 1 <= lookahead <= horizon - 1 <= stride - 1 (the reference raises IndexError at column `lookahead`).
// It is cut into one leg's share of the two np.all over the sequence (ga_leg_window) and the decision from the four
// conjunctions (ga_trigger), so that a kernel whose lanes each hold one leg's row (srbd_producers.hip wb_update_kernel)
// runs the same statements.
template <class T>
YAW_HD inline void ga_leg_window(const T* row, int lookahead, bool& stable, bool& next_all) {
    for (int i = 0; i < lookahead; ++i) stable = stable && row[i] == (T)1;  // STC:158
    next_all = next_all && row[lookahead] == (T)1;                           // STC:159
}

YAW_HD inline int32_t ga_trigger(int32_t* rising_edge, bool cur, bool prev, bool stable, bool next_all) {
    if (cur && !prev) *rising_edge = 1;              // STC:154-155
    if (*rising_edge != 0 && stable && !next_all) {  // STC:161-163
        *rising_edge = 0;
        return 1;
    }
    return 0;
}

template <class T>
YAW_HD inline int32_t ga_touch_down(int32_t* rising_edge, const T* current, const T* previous, const T* seq,
                                    int stride, int lookahead) {
    bool cur = true, prev = true;
    for (int l = 0; l < 4; ++l) {
        cur = cur && current[l] == (T)1;
        prev = prev && previous[l] == (T)1;
    }
    bool stable = true, next_all = true;
    for (int l = 0; l < 4; ++l) ga_leg_window(seq + (size_t)l * stride, lookahead, stable, next_all);
    return ga_trigger(rising_edge, cur, prev, stable, next_all);
}

// The three timing values of WBI:355-358 for a float32 best frequency (see the header comment).  false: a value the
// write-back refuses, nothing to store.
YAW_HD inline bool ga_timing_values(float best_freq, double duty, double* step_freq, double* stance_time,
                                    double* swing_period) {
#pragma clang fp contract(off)
    if (!(best_freq > 0.0f) || !(best_freq <= 3.4028234663852886e38f)) return false;
    const float inv = 1.0f / best_freq;
    const float stance = inv * (float)duty;
    const double one_minus = 1.0 - duty;
    const float swing = (float)one_minus * inv;
    if (!(swing > 0.0f) || !(swing <= 3.4028234663852886e38f)) return false;  // srbd_stc_set_timing's refusal
    *step_freq = (double)best_freq;
    *stance_time = (double)stance;
    *swing_period = (double)swing;
    return true;
}

// WBI:354-358 for one environment.  frg and stc may be NULL (a caller that keeps only some of the stages); the duty
// factor is pgg's.  optimize != 1 (the reference's `== 1`) writes nothing.  Returns 1 when the structs were written.
YAW_HD inline int32_t ga_apply_freq(srbd_pgg* pgg, srbd_frg* frg, srbd_stc* stc, int32_t optimize, float best_freq) {
    if (optimize != 1) return 0;
    double f, stance, swing;
    if (!ga_timing_values(best_freq, pgg->duty_factor, &f, &stance, &swing)) return 0;
    pgg->step_freq = f;                  // WBI:355
    if (frg) frg->stance_time = stance;  // WBI:356
    if (stc) stc->swing_period = swing;  // WBI:357-358: srbd_stc_set_timing with step_height unchanged
    return 1;
}

// The array jax.random.choice draws the sample frequencies from (GA:687-692, :834-838): MPPI takes the configured
// candidates; random sampling takes them when optimize_swing is set and n_freq copies of the nominal frequency
// otherwise (np.where(bool(optimize_swing), available, float32(nominal))).  Entries past n_freq are zero.
YAW_HD inline void ga_freq_set(int random_sampling, int32_t optimize, float nominal, const float* available, int n_freq,
                               float* out /* SRBD_MAX_FREQS */) {
    const bool own = !random_sampling || optimize != 0;
    for (int i = 0; i < SRBD_MAX_FREQS; ++i) out[i] = i < n_freq ? (own ? available[i] : nominal) : 0.0f;
}

// The gait fields of one StepInput (In: srbd_core.h StepInput; a template so that this header needs no device
// header): leg phases, generator dt and duty factor, the candidate set, the chunk boundaries cb[0..ncb) (formed once
// on the host, srbd_api.hip ga_chunk_bounds) and whether the sample frequencies are injected.
template <class In>
YAW_HD inline void ga_write_fields(In* in, const float* timing, float pgg_dt, float duty_factor, const float* freq_set,
                                   int n_freq, const int32_t* cb, int ncb, bool explicit_rows) {
    for (int l = 0; l < 4; ++l) in->ga_timing[l] = timing[l];
    in->ga_dt = pgg_dt;
    in->ga_duty = duty_factor;
    in->ga_nfreq = n_freq;
    for (int i = 0; i < SRBD_MAX_FREQS; ++i) in->ga_freqs[i] = i < n_freq ? freq_set[i] : 0.0f;
    for (int i = 0; i < ncb; ++i) in->ga_cb[i] = cb[i];
    in->ga_explicit = explicit_rows ? 1 : 0;
}

}  // namespace srbd
