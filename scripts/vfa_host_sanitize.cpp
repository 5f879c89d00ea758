// Stand-alone ASan + UBSan driver of the apex gate's host calls (srbd_vfa_init, srbd_vfa_mode, srbd_vfa_commit,
// srbd_vfa_reset; include/srbd_host.h).  Host code only, run on the CPU:
//
//   cd quadruped-pympc-tamols_amd && mkdir -p build && /opt/rocm/bin/hipcc -O1 -g -std=c++17 -ffp-contract=off -x c++ \
//       -ffunction-sections -Wl,--gc-sections \
//       -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
//       ../scripts/vfa_host_sanitize.cpp csrc/srbd_host.cpp -o build/vfa_host_sanitize && build/vfa_host_sanitize
//
// (srbd_host.cpp also holds the plugin-API glue, which calls into the device library; --gc-sections drops those
// functions, which nothing here references, so the program links without it.)
//
// Every array is heap-allocated at its exact size, so a read or write past the 12 / 24 / 4 entries the header promises
// is a report.  The driver walks a trot through the gate with a stand-in search, every refusal, and the cases of
// srbd_vfa_commit, and checks the state machine's invariants as it goes.  Exit status 0 and "ok" when nothing fired.
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

int main() {
    const int E_INVALID = -1;
    auto g = std::make_unique<srbd_vfa>();
    auto stc = std::make_unique<srbd_stc>();
    auto pgg = std::make_unique<srbd_pgg>();
    std::unique_ptr<double[]> contact(new double[4]), seeds(new double[12]), sf(new double[12]), sb(new double[24]),
        of(new double[12]), ob(new double[24]);
    std::unique_ptr<int32_t[]> sv(new int32_t[4]), ov(new int32_t[4]);
    std::unique_ptr<int32_t> mode(new int32_t(-7));

    CHECK(srbd_vfa_init(g.get()) == 0);
    CHECK(srbd_stc_init(stc.get(), 0.06, 0.25, 500.0, 10.0, SRBD_SWING_BEZIER_REF) == 0);
    CHECK(srbd_pgg_init(pgg.get(), SRBD_GAIT_TROT, 0.65, 1.4, 12) == 0);
    for (int k = 0; k < 24; ++k) CHECK(isnan(g->boxes[k]));

    // a trot through the gate: 3 gait cycles of dt = 0.004
    const double dt = 0.004;
    int seen[3] = {0, 0, 0}, searches = 0;
    for (int step = 0; step < 540; ++step) {
        CHECK(srbd_pgg_run(pgg.get(), dt, 1.4, contact.get()) == 0);
        for (int k = 0; k < 12; ++k) seeds[k] = 0.01 * k + 0.001 * step;
        CHECK(srbd_vfa_mode(g.get(), stc.get(), contact.get(), 0.01, mode.get()) == 0);
        const int m = *mode;
        CHECK(m == SRBD_VFA_PASS || m == SRBD_VFA_SEARCH || m == SRBD_VFA_HOLD);
        const int apex = srbd_stc_apex(stc.get(), contact.get(), 0.01), full = srbd_stc_full_stance(contact.get());
        CHECK((m == SRBD_VFA_SEARCH) == (apex == 1 && g->initialized[0] == 0));
        CHECK(!(apex == 1 && full == 1));  // a search and the reset never fall on one step
        const int was = g->initialized[0];
        double held[12];
        memcpy(held, g->footholds, sizeof(held));
        if (m == SRBD_VFA_SEARCH) {
            for (int k = 0; k < 12; ++k) sf[k] = seeds[k] + 0.05;
            for (int k = 0; k < 24; ++k) sb[k] = 100.0 + k + step;
            for (int l = 0; l < 4; ++l) sv[l] = !(searches % 2 == 1 && l == (searches / 2) % 4);
            ++searches;
            CHECK(srbd_vfa_commit(g.get(), m, seeds.get(), sf.get(), sb.get(), sv.get(), of.get(), ob.get(),
                                  ov.get()) == 0);
            for (int k = 0; k < 12; ++k) CHECK(of[k] == sf[k]);
            for (int l = 0; l < 4; ++l) CHECK(ov[l] == sv[l] && g->initialized[l] == 1);
        } else {  // the searched pointers may be NULL
            CHECK(srbd_vfa_commit(g.get(), m, seeds.get(), nullptr, nullptr, nullptr, of.get(), ob.get(), ov.get()) == 0);
            for (int k = 0; k < 12; ++k) CHECK(of[k] == (m == SRBD_VFA_PASS ? seeds[k] : held[k]));
            for (int l = 0; l < 4; ++l) CHECK(g->initialized[l] == (m == SRBD_VFA_HOLD ? was : 0));
        }
        for (int k = 0; k < 12; ++k) CHECK(of[k] == g->footholds[k]);
        for (int k = 0; k < 24; ++k) CHECK((isnan(ob[k]) && isnan(g->boxes[k])) || ob[k] == g->boxes[k]);
        ++seen[m];
        CHECK(srbd_stc_update_swing_time(stc.get(), contact.get(), dt) == 0);
    }
    CHECK(seen[0] > 0 && seen[1] >= 4 && seen[2] > 0);

    // refusals: nothing written
    auto before = std::make_unique<srbd_vfa>(*g);
    *mode = -7;
    CHECK(srbd_vfa_init(nullptr) == E_INVALID && srbd_vfa_reset(nullptr) == E_INVALID);
    CHECK(srbd_vfa_mode(nullptr, stc.get(), contact.get(), 0.01, mode.get()) == E_INVALID);
    CHECK(srbd_vfa_mode(g.get(), nullptr, contact.get(), 0.01, mode.get()) == E_INVALID);
    CHECK(srbd_vfa_mode(g.get(), stc.get(), nullptr, 0.01, mode.get()) == E_INVALID);
    CHECK(srbd_vfa_mode(g.get(), stc.get(), contact.get(), 0.01, nullptr) == E_INVALID);
    CHECK(srbd_vfa_mode(g.get(), stc.get(), contact.get(), NAN, mode.get()) == E_INVALID);
    CHECK(srbd_vfa_mode(g.get(), stc.get(), contact.get(), INFINITY, mode.get()) == E_INVALID);
    for (int bad : {-1, 3, 1 << 30})
        CHECK(srbd_vfa_commit(g.get(), bad, seeds.get(), sf.get(), sb.get(), sv.get(), of.get(), ob.get(), ov.get()) ==
              E_INVALID);
    CHECK(srbd_vfa_commit(nullptr, SRBD_VFA_PASS, seeds.get(), nullptr, nullptr, nullptr, of.get(), ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_PASS, nullptr, nullptr, nullptr, nullptr, of.get(), ob.get(), ov.get()) ==
          E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_PASS, seeds.get(), nullptr, nullptr, nullptr, nullptr, ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_PASS, seeds.get(), nullptr, nullptr, nullptr, of.get(), nullptr,
                          ov.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_PASS, seeds.get(), nullptr, nullptr, nullptr, of.get(), ob.get(),
                          nullptr) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_SEARCH, seeds.get(), nullptr, sb.get(), sv.get(), of.get(), ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_SEARCH, seeds.get(), sf.get(), nullptr, sv.get(), of.get(), ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_SEARCH, seeds.get(), sf.get(), sb.get(), nullptr, of.get(), ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(*mode == -7 && memcmp(g.get(), before.get(), sizeof(srbd_vfa)) == 0);
    g->initialized[2] ^= 1;  // the four words differ
    *before = *g;
    CHECK(srbd_vfa_mode(g.get(), stc.get(), contact.get(), 0.01, mode.get()) == E_INVALID);
    CHECK(srbd_vfa_commit(g.get(), SRBD_VFA_PASS, seeds.get(), nullptr, nullptr, nullptr, of.get(), ob.get(),
                          ov.get()) == E_INVALID);
    CHECK(*mode == -7 && memcmp(g.get(), before.get(), sizeof(srbd_vfa)) == 0);
    CHECK(srbd_vfa_reset(g.get()) == 0);
    for (int l = 0; l < 4; ++l) CHECK(g->initialized[l] == 0);
    printf("ok: %d pass, %d search, %d hold steps\n", seen[0], seen[1], seen[2]);
    return 0;
}
