"""The maps the map-warp tests share (tests/test_gpu_warp.py, tests/test_warp_chain_maps.py): a destination of 200 x 136 cells at
5 cm -- ragged in 64-cell words, with NaN, 0.0 and -0.0 holes --, a source of 150 x 90 cells at 4 cm with another corner, and the two
maps of the locate -> align -> compare chain."""
import math

import numpy as np

import _warp_expect as wx

L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
RES_D, W_D, H_D, POS_D = 0.05, 200, 136, (-1.0, 0.5)
RES_S, W_S, H_S, POS_S = 0.04, 150, 90, (0.3, -0.7)
GUARD = -12345.678


def metres(cells, res):
    """a width in metres that gms_grid_size's float ceil turns into `cells`"""
    return cells * res - res * 0.4


def dst_log():
    rng = np.random.default_rng(200136)
    log = np.zeros((H_D, W_D))                                                 # never observed
    log[10:121, 10:181] = L_FREE                                               # a room ...
    log[10, 10:181] = log[120, 10:181] = L_OCC                                 # ... with walls
    log[10:121, 10] = log[10:121, 180] = L_OCC
    log[10:90, 70] = L_OCC
    log[60, 100:181] = 3 * L_OCC
    log[126:136, :] = 2 * L_FREE                                               # a free strip along the top edge, corner to corner
    log[0:6, 0:40] = L_FREE
    room = np.zeros((H_D, W_D), bool)
    room[11:120, 11:180] = True
    log[room & (rng.random((H_D, W_D)) < 0.01)] = L_OCC                        # clutter
    log[30:40, 100:112] = 0.0                                                  # holes in the room: never observed,
    log[80:90, 140:150] = np.nan                                               # NaN
    log[95:100, 30:44] = -0.0                                                  # and -0.0
    return log


def src_log():
    rng = np.random.default_rng(15090)
    log = rng.choice([0.0, L_FREE, 2 * L_FREE, L_OCC, 4 * L_OCC], size=(H_S, W_S), p=[0.3, 0.35, 0.1, 0.2, 0.05])
    log[0, :] = log[-1, :] = L_OCC                                             # a frame: the source's outline shows in the destination
    log[:, 0] = log[:, -1] = 2 * L_OCC
    log[20:30, 40:60] = np.nan
    log[50:55, 100:120] = -0.0
    log[70:80, 10:30] = 0.0
    return log


def quarter_turn_pose(gd, gs, ox, oy):
    """c = 0, s = 1 with the source's corner cell (0, 0) landing in destination cell (ox + H_s - 1, oy): for grids of one
    resolution whose corners are whole cells of the pose apart, destination [oy : oy + W_s, ox : ox + H_s] = rot90(source, -1).
    p_dst = (-y_src, x_src) + t: the source's world origin goes to t"""
    tx = gd.px + (ox + gs.H) * gd.res + gs.py
    ty = gd.py + oy * gd.res - gs.px
    return (tx, ty, 0.0, 1.0)


# ---- the chain: A, a map of rooms; B, a window of A whose world origin is the centre of one of A's cells ------------------------------
W_A, H_A, POS_A = 160, 120, (0.0, 0.0)
W_B, H_B = 64, 48
B_AT = (52, 37)                                                                 # B's cell (0, 0) is A's cell B_AT
B_ORIGIN = (20, 15)                                                             # B's world origin is the centre of its cell B_ORIGIN
POS_B = (-(B_ORIGIN[0] + 0.5) * RES_D, -(B_ORIGIN[1] + 0.5) * RES_D)
N_THETA = 4


def chain_a():
    log = np.zeros((H_A, W_A))
    log[5:115, 5:155] = L_FREE
    log[5, 5:155] = log[114, 5:155] = L_OCC
    log[5:115, 5] = log[5:115, 154] = L_OCC
    log[5:80, 60] = L_OCC                                                      # rooms of different sizes, doors at different places
    log[30:34, 60] = L_FREE
    log[50, 60:154] = L_OCC
    log[50, 100:105] = L_FREE
    log[50:115, 110] = L_OCC
    log[90:95, 110] = L_FREE
    log[80, 5:60] = L_OCC
    log[80, 20:26] = L_FREE
    rng = np.random.default_rng(7)
    for _ in range(40):                                                        # furniture: what makes a window of the map unlike every other
        x, y = int(rng.integers(8, 150)), int(rng.integers(8, 110))
        log[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = L_OCC
    return log


def chain_geometry():
    ga = wx.Geometry.make(W_A, H_A, RES_D, *POS_A)
    gb = wx.Geometry.make(W_B, H_B, RES_D, *POS_B)
    return ga, gb


def chain_true_pose():
    """the pose of B's world frame in A's world: the centre of A's cell B_AT + B_ORIGIN, heading 0"""
    ga, _ = chain_geometry()
    return ((B_AT[0] + B_ORIGIN[0] + 0.5) * ga.res, (B_AT[1] + B_ORIGIN[1] + 0.5) * ga.res, 0.0)


def chain_b(a_log):
    """B: the window of A, made by the expectation -- A read through the inverse pose into B's grid"""
    ga, gb = chain_geometry()
    tx, ty, _ = chain_true_pose()
    b, stats = wx.expect(np.zeros((H_B, W_B)), gb, a_log, ga, (-tx, -ty, 1.0, 0.0), "replace")
    assert stats["n_outside"] == 0
    return b


def exhaustive_locate(a_log, offsets):
    """SCORE(k, x, y) of gridmapslam.h "global scan matching" with tol = 0 over every cell of A, in numpy: [n_theta][H][W]"""
    occ = a_log > 0
    H, W = occ.shape
    score = np.zeros((offsets.shape[0], H, W), np.int32)
    for k in range(offsets.shape[0]):
        for dx, dy in offsets[k]:
            dx, dy = int(dx), int(dy)
            if dx == -32768:
                continue
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            score[k][ys, xs] += occ[yd, xd]
    return score


def turned(theta, about, to):
    """(tx, ty, c, s): the source's world point `about` lands on the destination's world point `to` under a turn by theta"""
    c, s = math.cos(theta), math.sin(theta)
    return (to[0] - (c * about[0] - s * about[1]), to[1] - (s * about[0] + c * about[1]), c, s)
