"""NumPy restatement of the reference's FootholdReferenceGenerator, the expected side of tests/test_frg_host.py.

FRG = quadruped_pympc/helpers/foothold_reference_generator.py (reference); the three methods are restated line by
line with FRG:line citations, float64 throughout.  The reference module itself cannot be imported here (mujoco and
gym_quadruped are absent).

What is pinned is this restatement, not the reference's own ``@`` products: the rotation products are written out
element by element in the row order NumPy's definition of the product gives --
    R_W2H   @ v = (c x + s y, -s x + c y, z)        R_W2H.T @ v = (c x + (-s) y, s x + c y, z)
-- because a BLAS that fuses a multiply-add differs from that in the last place (the standing
tests/golden/make_golden.py describes for every other fixture), and the 3 x 3 product's "+ 0 z" terms, which change
nothing but the sign of a zero and a non-finite z's spread into x and y, are left out.

cos and sin of the yaw are np.cos / np.sin here; the C functions use the correctly rounded csrc/yaw_sincos.h.  A test
keeps the yaws where the two agree (``agreeing_yaws``) and asserts that few were dropped.
"""
import collections
import copy

import numpy as np

LEGS = ("FL", "FR", "RL", "RR")
HIST = 20


def rot(c, s, v):
    """R_W2H @ v, element by element (v of 2 or 3 entries)."""
    out = np.array(v, dtype=np.float64)
    x, y = np.float64(v[0]), np.float64(v[1])
    out[0] = c * x + s * y
    out[1] = -s * x + c * y
    return out


def rot_t(c, s, v):
    """R_W2H.T @ v, element by element."""
    out = np.array(v, dtype=np.float64)
    x, y = np.float64(v[0]), np.float64(v[1])
    out[0] = c * x + -s * y
    out[1] = s * x + c * y
    return out


def mean_rows(rows):
    """np.mean(rows, axis=0) of FRG:98 as the sum it is: the rows added oldest to newest, divided by the count.
    The sum starts from the oldest row, not from zero, so an all -0.0 history has a -0.0 mean (IEEE: -0.0 + -0.0 =
    -0.0).  np.mean returns the same bits for every history but that one kind: NumPy's add.reduce over axis 0 starts
    from the identity +0.0 (2.2 does), which turns a -0.0 sum into +0.0 and changes nothing else.  The sign of a
    zero mean does not reach the footholds for a positive stance time (0.0 + -0.0 = 0.0 in vel_offset +
    error_compensation).  tests/test_frg_host.py compares this with np.mean itself on random histories."""
    acc = np.array(rows[0], dtype=np.float64)
    for r in rows[1:]:
        acc = acc + r
    return acc / np.float64(len(rows))


class FrgModel:
    def __init__(self, stance_time, lift_off_positions, hip_height):  # FRG:15-51
        self.base_vel_hist = collections.deque(maxlen=HIST)            # FRG:25
        self.stance_time = np.float64(stance_time)                     # FRG:26
        self.hip_height = np.float64(hip_height)                       # FRG:27
        lift = np.array(lift_off_positions, dtype=np.float64).reshape(4, 3)
        self.lift_off_positions = copy.deepcopy(lift)                  # FRG:28
        self.touch_down_positions = copy.deepcopy(lift)                # FRG:29
        self.com_pos_offset_w = np.zeros((3,))                         # FRG:33
        self.lift_off_positions_h = copy.deepcopy(lift)                # FRG:39 ("TODO wrong")
        self.touch_down_positions_h = copy.deepcopy(lift)              # FRG:40
        self.hip_offset = np.float64(0.1)                              # FRG:44
        self.last_reference_footholds = np.zeros((4, 3))               # FRG:47-49

    def compute_footholds_reference(self, base_position, yaw, base_xy_lin_vel, ref_base_xy_lin_vel, hips_position,
                                    com_height_nominal, gravity):
        base_position = np.asarray(base_position, dtype=np.float64)
        hips_position = np.asarray(hips_position, dtype=np.float64)
        c, s = np.cos(np.float64(yaw)), np.sin(np.float64(yaw))        # FRG:88-90
        base_lin_vel_H = rot(c, s, base_xy_lin_vel)                    # FRG:93
        ref_base_lin_vel_H = rot(c, s, ref_base_xy_lin_vel)            # FRG:94
        self.base_vel_hist.append(base_lin_vel_H)                      # FRG:97
        with np.errstate(all="ignore"):
            base_vel_mvg = mean_rows(list(self.base_vel_hist))         # FRG:98
            delta_ref_H = (self.stance_time / 2.0) * ref_base_lin_vel_H                             # FRG:103
            delta_ref_H = np.clip(delta_ref_H, -self.hip_height * 1.5, self.hip_height * 1.5)       # FRG:104
            vel_offset = np.concatenate((delta_ref_H, np.zeros(1)))                                 # FRG:105
            error_compensation = np.sqrt(np.float64(com_height_nominal) / np.float64(gravity)) * (
                base_vel_mvg - ref_base_lin_vel_H)                                                  # FRG:108
            error_compensation = np.where(error_compensation > 0.05, 0.05, error_compensation)      # FRG:109
            error_compensation = np.where(error_compensation < -0.05, -0.05, error_compensation)    # FRG:110
            error_compensation = np.concatenate((error_compensation, np.zeros(1)))                  # FRG:111
            # kept for the tests' coverage checks (which limits were reached); not part of the reference
            self.last_mean, self.last_delta, self.last_err = base_vel_mvg, delta_ref_H, error_compensation[:2]
            ref_feet = np.zeros((4, 3))                                                             # FRG:114
            for l in range(4):
                ref_feet[l, 0:2] = rot(c, s, hips_position[l, 0:2] - base_position[0:2])            # FRG:117-120
            ref_feet[0, 1] += self.hip_offset                                                       # FRG:126-129
            ref_feet[1, 1] -= self.hip_offset
            ref_feet[2, 1] += self.hip_offset
            ref_feet[3, 1] -= self.hip_offset
            ref_feet += vel_offset + error_compensation                                             # FRG:132
            for l in range(4):
                ref_feet[l, 0:2] = rot_t(c, s, ref_feet[l, :2]) + base_position[0:2]                # FRG:135-138
                ref_feet[l, 0:2] += self.com_pos_offset_w[0:2]                                      # FRG:143-146
                ref_feet[l, 2] = self.lift_off_positions[l][2]                                      # FRG:150-151
        self.last_reference_footholds = copy.deepcopy(ref_feet)                                     # FRG:155
        return ref_feet

    def update_lift_off_positions(self, previous_contact, current_contact, feet_pos, full_stance, base_position,
                                  yaw):
        base_position = np.asarray(base_position, dtype=np.float64)
        feet_pos = np.asarray(feet_pos, dtype=np.float64)
        c, s = np.cos(np.float64(yaw)), np.sin(np.float64(yaw))        # FRG:162-164
        with np.errstate(all="ignore"):
            for l in range(4):                                         # FRG:166
                if full_stance:                                        # FRG:167-169
                    self.lift_off_positions[l] = feet_pos[l]
                    continue
                if previous_contact[l] == 1 and current_contact[l] == 0:                            # FRG:172-174
                    self.lift_off_positions[l] = feet_pos[l]
                    self.lift_off_positions_h[l] = rot(c, s, self.lift_off_positions[l] - base_position)
                elif previous_contact[l] == 0 and current_contact[l] == 0:                          # FRG:176-178
                    self.lift_off_positions[l] = rot_t(c, s, self.lift_off_positions_h[l]) + base_position

    def update_touch_down_positions(self, previous_contact, current_contact, feet_pos, full_stance, base_position,
                                    yaw):
        base_position = np.asarray(base_position, dtype=np.float64)
        feet_pos = np.asarray(feet_pos, dtype=np.float64)
        c, s = np.cos(np.float64(yaw)), np.sin(np.float64(yaw))        # FRG:183-185
        with np.errstate(all="ignore"):
            for l in range(4):                                         # FRG:187
                if full_stance:                                        # FRG:188-190
                    self.touch_down_positions[l] = feet_pos[l]
                    continue
                if previous_contact[l] == 0 and current_contact[l] == 1:                            # FRG:193-195
                    self.touch_down_positions[l] = feet_pos[l]
                    self.touch_down_positions_h[l] = rot(c, s, self.touch_down_positions[l] - base_position)
                elif previous_contact[l] == 1 and current_contact[l] == 1:                          # FRG:197-199
                    self.touch_down_positions[l] = rot_t(c, s, self.touch_down_positions_h[l]) + base_position

    def history(self):
        """The deque's rows, oldest first: (n, 2)."""
        return np.array(list(self.base_vel_hist), dtype=np.float64).reshape(len(self.base_vel_hist), 2)


def struct_history(g):
    """The same rows read from a srbd_frg ctypes struct."""
    n, head = g.hist_len, g.hist_head
    first = head if n == HIST else 0
    return np.array([list(g.vel_hist[(first + i) % HIST]) for i in range(n)], dtype=np.float64).reshape(n, 2)


def agreeing_yaws(lib, yaws):
    """(yaws where np.cos and np.sin both equal the library's correctly rounded values, share dropped)."""
    y = np.ascontiguousarray(yaws, dtype=np.float64).reshape(-1)
    cs = np.zeros((y.size, 2))
    assert lib.srbd_selftest_yaw_sincos(y.ctypes.data, y.size, cs.ctypes.data) == 0
    keep = (cs[:, 0] == np.cos(y)) & (cs[:, 1] == np.sin(y))
    return y[keep], 1.0 - keep.mean()


def contact_script(steps, phase=0):
    """(steps + 1, 4) contact flags in which every leg meets all four (previous, current) pairs within any five
    consecutive rows: the period-4 pattern 1 1 0 0, shifted by one row per leg."""
    k = (np.arange(steps + 1)[:, None] + np.arange(4)[None, :] + phase) % 4
    return (k < 2).astype(np.float64)
