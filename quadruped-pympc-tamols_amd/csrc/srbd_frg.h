// srbd_frg.h -- the foothold reference generator's arithmetic, one leg at a time, for the host functions
// (srbd_host.cpp srbd_frg_*) and the device kernel (srbd_producers.hip frg_step_kernel).  Both sides compile these
// same float64 operations unfused, and cos / sin of the yaw come from yaw_sincos.h, so they leave the same bits.
//   FRG = quadruped_pympc/helpers/foothold_reference_generator.py
// The 3 x 3 yaw rotation R_W2H = [[c, s, 0], [-s, c, 0], [0, 0, 1]] is written out element by element:
//   R_W2H   @ v = (c x + s y, -s x + c y, z)          R_W2H.T @ v = (c x + (-s) y, s x + c y, z)
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/srbd_host.h"
#include "yaw_sincos.h"

namespace srbd {

// FRG:166-178, leg l.  Contacts compare with == 1 and == 0 as the reference compares them.
YAW_HD inline void frg_leg_lift_off(srbd_frg* g, int l, double prev, double cur, const double* foot, bool full_stance,
                                    const double* base, double c, double s) {
#pragma clang fp contract(off)
    double* w = g->lift_off[l];
    double* h = g->lift_off_h[l];
    if (full_stance) {
        w[0] = foot[0], w[1] = foot[1], w[2] = foot[2];
    } else if (prev == 1.0 && cur == 0.0) {
        w[0] = foot[0], w[1] = foot[1], w[2] = foot[2];
        const double x = w[0] - base[0], y = w[1] - base[1], z = w[2] - base[2];
        h[0] = c * x + s * y;
        h[1] = -s * x + c * y;
        h[2] = z;
    } else if (prev == 0.0 && cur == 0.0) {
        const double x = h[0], y = h[1], z = h[2];
        w[0] = (c * x + -s * y) + base[0];
        w[1] = (s * x + c * y) + base[1];
        w[2] = z + base[2];
    }
}

// FRG:187-199, leg l.
YAW_HD inline void frg_leg_touch_down(srbd_frg* g, int l, double prev, double cur, const double* foot,
                                      bool full_stance, const double* base, double c, double s) {
#pragma clang fp contract(off)
    double* w = g->touch_down[l];
    double* h = g->touch_down_h[l];
    if (full_stance) {
        w[0] = foot[0], w[1] = foot[1], w[2] = foot[2];
    } else if (prev == 0.0 && cur == 1.0) {
        w[0] = foot[0], w[1] = foot[1], w[2] = foot[2];
        const double x = w[0] - base[0], y = w[1] - base[1], z = w[2] - base[2];
        h[0] = c * x + s * y;
        h[1] = -s * x + c * y;
        h[2] = z;
    } else if (prev == 1.0 && cur == 1.0) {
        const double x = h[0], y = h[1], z = h[2];
        w[0] = (c * x + -s * y) + base[0];
        w[1] = (s * x + c * y) + base[1];
        w[2] = z + base[2];
    }
}

// The slot the next entry goes to, and the ring after it: (len, head) -> (len', head').  While the ring fills, head
// == len and the oldest entry is slot 0; once full, head is the oldest entry, which the push evicts.
// A len or head outside that rule (a struct edited by hand) is read as the nearest state inside it, so no index leaves
// vel_hist and the slot written is never one the mean reads.
YAW_HD inline void frg_ring_sane(int& len, int& head) {
    len = len < 0 ? 0 : len > SRBD_FRG_HIST ? SRBD_FRG_HIST : len;
    if (len < SRBD_FRG_HIST)
        head = len;
    else if (head < 0 || head >= SRBD_FRG_HIST)
        head = 0;
}

YAW_HD inline int frg_ring_next(int len, int head, int& len_out, int& head_out) {
    frg_ring_sane(len, head);
    const int slot = head;
    head_out = head + 1 == SRBD_FRG_HIST ? 0 : head + 1;
    len_out = len < SRBD_FRG_HIST ? len + 1 : len;
    return slot;
}

// FRG:97-98: the mean of the ring after (vx, vy) is pushed, formed from the ring as it is and the new value: the
// sum starts from the oldest entry that stays, adds oldest to newest, the new value last, and is divided by the
// count (np.mean of the deque's rows).  The slot frg_ring_next names -- unused, or the evicted entry -- is not read.
YAW_HD inline void frg_mean_with(const srbd_frg* g, int len, int head, double vx, double vy, double& mx, double& my) {
#pragma clang fp contract(off)
    frg_ring_sane(len, head);
    const bool full = len == SRBD_FRG_HIST;
    const int kept = full ? SRBD_FRG_HIST - 1 : len;  // entries that stay
    int i = full ? (head + 1 == SRBD_FRG_HIST ? 0 : head + 1) : 0;
    double sx = vx, sy = vy;
    if (kept > 0) {
        sx = g->vel_hist[i][0];
        sy = g->vel_hist[i][1];
        for (int k = 1; k < kept; ++k) {
            i = i + 1 == SRBD_FRG_HIST ? 0 : i + 1;
            sx = sx + g->vel_hist[i][0];
            sy = sy + g->vel_hist[i][1];
        }
        sx = sx + vx;
        sy = sy + vy;
    }
    const double n = (double)(kept + 1);
    mx = sx / n;
    my = sy / n;
}

// np.clip(x, lo, hi): a NaN x passes.
YAW_HD inline double frg_clip(double x, double lo, double hi) {
    const double t = x != x ? x : (x > lo ? x : lo);
    return t != t ? t : (t < hi ? t : hi);
}

// FRG:103-111: vel_offset + error_compensation in the horizontal frame (the z entries are 0 + 0), from the rotated
// reference velocity (rx, ry), the moving average (mx, my) and root = sqrt(com_height_nominal / gravity).
YAW_HD inline void frg_compensation(const srbd_frg* g, double rx, double ry, double mx, double my, double root,
                                    double& ox, double& oy) {
#pragma clang fp contract(off)
    const double half = g->stance_time / 2.0, lim = g->hip_height * 1.5;
    const double dx = frg_clip(half * rx, -lim, lim), dy = frg_clip(half * ry, -lim, lim);
    double ex = root * (mx - rx), ey = root * (my - ry);
    ex = ex > 0.05 ? 0.05 : ex;  // the two np.where limits: a NaN passes both
    ey = ey > 0.05 ? 0.05 : ey;
    ex = ex < -0.05 ? -0.05 : ex;
    ey = ey < -0.05 ? -0.05 : ey;
    ox = dx + ex;
    oy = dy + ey;
}

// FRG:117-155, leg l: the foothold into out[3] and last_reference_footholds[l].  off: com_pos_offset_w or NULL (+0.0).
YAW_HD inline void frg_leg_foothold(srbd_frg* g, int l, const double* hip, const double* base, double c, double s,
                                    double ox, double oy, const double* off, double* out) {
#pragma clang fp contract(off)
    const double x = hip[0] - base[0], y = hip[1] - base[1];
    double fx = c * x + s * y;
    double fy = -s * x + c * y;
    fy = (l == 0 || l == 2) ? fy + g->hip_offset : fy - g->hip_offset;  // FL, RL: +; FR, RR: -
    fx = fx + ox;
    fy = fy + oy;
    double wx = (c * fx + -s * fy) + base[0];
    double wy = (s * fx + c * fy) + base[1];
    wx = wx + (off ? off[0] : 0.0);
    wy = wy + (off ? off[1] : 0.0);
    const double wz = g->lift_off[l][2];
    out[0] = wx, out[1] = wy, out[2] = wz;
    double* last = g->last_reference_footholds[l];
    last[0] = wx, last[1] = wy, last[2] = wz;
}

}  // namespace srbd
