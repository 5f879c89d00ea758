// Stand-alone ASan + UBSan driver of the per-environment reset's host call (srbd_loop_reset; include/srbd_host.h) and
// of the constructors and resets that share its statements (srbd_pgg_reset, srbd_frg_init, srbd_vfa_reset).  Host
// code only, run on the CPU:
//
//   cd quadruped-pympc-tamols_amd && mkdir -p build && /opt/rocm/bin/hipcc -O1 -g -std=c++17 -ffp-contract=off -x c++ \
//       -ffunction-sections -Wl,--gc-sections \
//       -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       ../scripts/loop_reset_host_sanitize.cpp csrc/srbd_host.cpp -o build/loop_reset_host_sanitize && \
//       build/loop_reset_host_sanitize
//
// (srbd_host.cpp also holds the plugin-API glue, which calls into the device library; --gc-sections drops those
// functions, which nothing here references, so the program links without it.)
//
// Every struct and array is heap-allocated at its exact size, so a read or write past a struct's last word, the 12
// feet or the num_params warm-start entries is a report.  The driver makes the call at both levels over all 32
// combinations of given and NULL structs, with and without the trigger word and the warm start, then every refusal,
// and checks what the header promises as it goes.  Exit status 0 and "ok" when nothing fired.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "../include/srbd_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

template <class T>
static bool same(const T& a, const T& b) {
    return memcmp(&a, &b, sizeof(T)) == 0;
}

int main() {
    const int E_INVALID = -1, P = 37;
    auto pgg = std::make_unique<srbd_pgg>(), pgg0 = std::make_unique<srbd_pgg>(), pggd = std::make_unique<srbd_pgg>();
    auto frg = std::make_unique<srbd_frg>(), frg0 = std::make_unique<srbd_frg>(), frgd = std::make_unique<srbd_frg>();
    auto stc = std::make_unique<srbd_stc>(), stc0 = std::make_unique<srbd_stc>(), stcd = std::make_unique<srbd_stc>();
    auto ter = std::make_unique<srbd_terrain_est>(), ter0 = std::make_unique<srbd_terrain_est>(),
         terd = std::make_unique<srbd_terrain_est>();
    auto vfa = std::make_unique<srbd_vfa>(), vfa0 = std::make_unique<srbd_vfa>(), vfad = std::make_unique<srbd_vfa>();
    std::unique_ptr<double[]> feet0(new double[12]), feet(new double[12]);
    std::unique_ptr<float[]> best(new float[P]);
    std::unique_ptr<int32_t> edge(new int32_t(1));
    for (int i = 0; i < 12; ++i) {
        feet0[i] = 0.01 * i - 0.05;
        feet[i] = 0.3 - 0.02 * i;
    }
    for (int gait = -1; gait <= 8; ++gait) {
        // the snapshots: constructor output
        CHECK(srbd_pgg_init(pgg0.get(), gait, 0.65, 1.4, 12) == 0);
        CHECK(srbd_frg_init(frg0.get(), 0.46, 0.28, feet0.get()) == 0);
        CHECK(srbd_stc_init(stc0.get(), 0.06, 0.25, 100.0, 10.0, SRBD_SWING_BEZIER_REF) == 0);
        CHECK(srbd_terrain_est_init(ter0.get()) == 0);
        CHECK(srbd_vfa_init(vfa0.get()) == 0);
        CHECK(frg0->hip_offset == 0.1 && frg0->hist_len == 0 && frg0->lift_off_h[3][2] == feet0[11]);
        // dirty structs: every byte set, then the fields the statements read made sane
        memset(pggd.get(), 0x5a, sizeof(srbd_pgg));
        memset(frgd.get(), 0x5a, sizeof(srbd_frg));
        memset(stcd.get(), 0x5a, sizeof(srbd_stc));
        memset(terd.get(), 0x5a, sizeof(srbd_terrain_est));
        memset(vfad.get(), 0x5a, sizeof(srbd_vfa));
        pggd->gait_type = gait;
        for (int level = 1; level <= 2; ++level)
            for (int combo = 0; combo < 32; ++combo)
                for (int extras = 0; extras < 4; ++extras) {
                    *pgg = *pggd, *frg = *frgd, *stc = *stcd, *ter = *terd, *vfa = *vfad;
                    *edge = 1;
                    for (int i = 0; i < P; ++i) best[i] = 1.5f;
                    srbd_pgg* a = combo & 1 ? pgg.get() : nullptr;
                    srbd_frg* b = combo & 2 ? frg.get() : nullptr;
                    srbd_stc* c = combo & 4 ? stc.get() : nullptr;
                    srbd_terrain_est* d = combo & 8 ? ter.get() : nullptr;
                    srbd_vfa* e = combo & 16 ? vfa.get() : nullptr;
                    int32_t* ed = extras & 1 ? edge.get() : nullptr;
                    float* be = extras & 2 ? best.get() : nullptr;
                    // level 1 needs no snapshot; level 2 one per given struct
                    const bool snaps = level == 2 || (combo & 1);
                    CHECK(srbd_loop_reset(level, b ? feet.get() : nullptr, a, b, c, d, e, snaps ? pgg0.get() : nullptr,
                                          snaps ? frg0.get() : nullptr, snaps ? stc0.get() : nullptr,
                                          snaps ? ter0.get() : nullptr, snaps ? vfa0.get() : nullptr, ed, be,
                                          be ? P : 0) == 0);
                    if (level == 2) {
                        CHECK(a ? same(*pgg, *pgg0) : same(*pgg, *pggd));
                        CHECK(c ? same(*stc, *stc0) : same(*stc, *stcd));
                        CHECK(d ? same(*ter, *ter0) : same(*ter, *terd));
                        CHECK(e ? same(*vfa, *vfa0) : same(*vfa, *vfad));
                        if (b) {
                            auto want = std::make_unique<srbd_frg>();
                            CHECK(srbd_frg_init(want.get(), 0.46, 0.28, feet.get()) == 0);
                            CHECK(same(*frg, *want));
                        } else {
                            CHECK(same(*frg, *frgd));
                        }
                        CHECK(*edge == (ed ? 0 : 1));
                        for (int i = 0; i < P; ++i) CHECK(best[i] == (be ? 0.0f : 1.5f));
                    } else {
                        auto p = std::make_unique<srbd_pgg>(*pggd);
                        if (a) CHECK(srbd_pgg_reset(p.get()) == 0);
                        CHECK(same(*pgg, *p) && pgg->step_freq == pggd->step_freq);
                        auto f = std::make_unique<srbd_frg>(*frgd);
                        if (b) memcpy(f->lift_off, feet.get(), sizeof(f->lift_off));
                        CHECK(same(*frg, *f));
                        auto v = std::make_unique<srbd_vfa>(*vfad);
                        if (e) CHECK(srbd_vfa_reset(v.get()) == 0);
                        CHECK(same(*vfa, *v));
                        CHECK(same(*stc, *stcd) && same(*ter, *terd) && *edge == 1);
                        for (int i = 0; i < P; ++i) CHECK(best[i] == 1.5f);
                    }
                }
    }
    // refusals: nothing changes
    *pgg = *pggd, *frg = *frgd, *stc = *stcd, *ter = *terd, *vfa = *vfad;
    *edge = 1;
    for (int i = 0; i < P; ++i) best[i] = 1.5f;
    auto untouched = [&] {
        bool ok = same(*pgg, *pggd) && same(*frg, *frgd) && same(*stc, *stcd) && same(*ter, *terd) &&
                  same(*vfa, *vfad) && *edge == 1;
        for (int i = 0; i < P; ++i) ok = ok && best[i] == 1.5f;
        return ok;
    };
    const int32_t levels[] = {0, 3, -1, 7, INT32_MAX, INT32_MIN};
    for (int32_t level : levels)
        CHECK(srbd_loop_reset(level, feet.get(), pgg.get(), frg.get(), stc.get(), ter.get(), vfa.get(), pgg0.get(),
                              frg0.get(), stc0.get(), ter0.get(), vfa0.get(), edge.get(), best.get(), P) == E_INVALID &&
              untouched());
    for (int level = 1; level <= 2; ++level) {
        CHECK(srbd_loop_reset(level, nullptr, pgg.get(), frg.get(), stc.get(), ter.get(), vfa.get(), pgg0.get(),
                              frg0.get(), stc0.get(), ter0.get(), vfa0.get(), edge.get(), best.get(), P) == E_INVALID &&
              untouched());
        for (int n : {0, -1, INT32_MIN})
            CHECK(srbd_loop_reset(level, feet.get(), pgg.get(), frg.get(), stc.get(), ter.get(), vfa.get(), pgg0.get(),
                                  frg0.get(), stc0.get(), ter0.get(), vfa0.get(), edge.get(), best.get(), n) ==
                      E_INVALID &&
                  untouched());
    }
    for (int missing = 0; missing < 5; ++missing)
        CHECK(srbd_loop_reset(2, feet.get(), pgg.get(), frg.get(), stc.get(), ter.get(), vfa.get(),
                              missing == 0 ? nullptr : pgg0.get(), missing == 1 ? nullptr : frg0.get(),
                              missing == 2 ? nullptr : stc0.get(), missing == 3 ? nullptr : ter0.get(),
                              missing == 4 ? nullptr : vfa0.get(), edge.get(), best.get(), P) == E_INVALID &&
              untouched());
    // srbd_frg_init on a table of the struct itself
    CHECK(srbd_frg_init(frg0.get(), 0.5, 0.3, &frg0->touch_down[0][0]) == 0 && frg0->lift_off[0][0] == feet0[0]);
    printf("ok\n");
    return 0;
}
