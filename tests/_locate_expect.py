"""Expected global scan matches (include/gridmapslam.h "global scan matching") from a downloaded logData, on the host: the HIT cells are
the blocked cells of _reach_expect.blocked at inflate = tol (a brute-force d2 <= tol^2 over the obstacle list), the SCORE of every
candidate comes from plain loops over the heading index, the row and the column (the column's cells looked up together, beam by beam in
one numpy index), and the result is `sorted` on the key (-score, k, y, x).  Nothing here knows about pyramids, bounds, work lists or
bit planes."""
import math

import numpy as np

import _reach_expect as rx

SKIP = -32768
OFF_MAX = 4095
DTYPE = np.dtype([("score", "<i4"), ("k", "<i4"), ("x", "<i4"), ("y", "<i4")])
FILLER = (0, -1, -1, -1)


def offsets_of(local_x, local_y, hit, n_theta, resolution, theta0=0.0, dtheta=None):
    """gms_locate_offsets' formula with math.cos / math.sin, python floats (doubles, never fused): int16 [n_theta][B][2]"""
    if dtheta is None:
        dtheta = 2.0 * math.pi / n_theta
    B = len(local_x)
    out = np.empty((n_theta, B, 2), dtype=np.int16)
    res = float(resolution)
    for k in range(n_theta):
        theta = float(theta0) + float(k) * float(dtheta)
        c, s = math.cos(theta), math.sin(theta)
        for b in range(B):
            lx, ly = float(local_x[b]), float(local_y[b])
            pair = (SKIP, SKIP)
            if hit[b] and math.isfinite(lx) and math.isfinite(ly):
                xc, ys, xs, yc = lx * c, ly * s, lx * s, ly * c
                ex, ey = xc - ys, xs + yc
                fx, fy = ex / res + 0.5, ey / res + 0.5
                if math.isfinite(fx) and math.isfinite(fy):
                    dx, dy = math.floor(fx), math.floor(fy)
                    if abs(dx) <= OFF_MAX and abs(dy) <= OFF_MAX:
                        pair = (dx, dy)
            out[k, b] = pair
    return out


def hit_cells(log, tol=0, not_free=False):
    """bool [H][W]: an obstacle cell of the mode's predicate within tol cells"""
    return rx.blocked(np.asarray(log, dtype=np.float64), tol, not_free)


def scores(log, offsets, rect=None, tol=0, not_free=False, hit=None):
    """int64 [n_theta][h][w]: SCORE of every candidate of the rectangle, free or not (hit: the hit cells, where the caller has them)"""
    if hit is None:
        hit = hit_cells(log, tol, not_free)
    H, W = hit.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    off = np.asarray(offsets).astype(np.int64)
    out = np.zeros((off.shape[0], h, w), dtype=np.int64)
    xs = np.arange(x0, x0 + w, dtype=np.int64)
    for k in range(off.shape[0]):
        dx, dy = off[k, :, 0], off[k, :, 1]
        use = ~((dx == SKIP) & (dy == SKIP))
        assert (np.abs(dx[use]) <= OFF_MAX).all() and (np.abs(dy[use]) <= OFF_MAX).all(), "an offset that is neither SKIP nor in range"
        dx, dy = dx[use], dy[use]
        for yi in range(h):
            py = y0 + yi + dy                                              # [b]
            px = xs[:, None] + dx[None, :]                                 # [w][b]
            inside = ((py >= 0) & (py < H))[None, :] & (px >= 0) & (px < W)
            cell = hit[np.clip(py, 0, H - 1)[None, :], np.clip(px, 0, W - 1)]
            out[k, yi, :] = (cell & inside).sum(axis=1)
    return out


def expect(log, offsets, rect=None, tol=0, not_free=False, min_score=1, cap=64, free_only=True, hit=None):
    """(records [cap] with the fillers, n_out, N)"""
    log = np.asarray(log, dtype=np.float64)
    H, W = log.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    sc = scores(log, offsets, (x0, y0, w, h), tol, not_free, hit)
    with np.errstate(invalid="ignore"):
        free = log < 0
    found = []
    for k in range(sc.shape[0]):
        for yi in range(h):
            for xi in range(w):
                s = int(sc[k, yi, xi])
                if s >= min_score and (not free_only or free[y0 + yi, x0 + xi]):
                    found.append((-s, k, y0 + yi, x0 + xi))
    found = sorted(found)
    rec = np.array([FILLER] * cap, dtype=DTYPE)
    n_out = min(cap, len(found))
    for i in range(n_out):
        s, k, y, x = found[i]
        rec[i] = (-s, k, x, y)
    return rec, n_out, len(found)
