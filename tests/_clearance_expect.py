"""Expected clearance fields (include/gridmapslam.h "clearance fields"), brute force in numpy from a downloaded logData: the list of
obstacle cells under the mode's predicate, d2 = the minimum of (x - ox)^2 + (y - oy)^2 over that list in int64, then the cap.  Nothing
here is separable, and nothing knows about bit planes or tiles.

expect_plain takes the minimum over the WHOLE list for every cell.  expect does the same per block of 16 x 16 output cells over the part
of the list that lies within max_radius of the block in both axes: an obstacle further away than that in x or in y is more than
max_radius from every cell of the block, so it can neither supply a value <= max_radius^2 nor turn one into FAR -- the capped result is
the same (tests/test_clearance_args.py holds the two against each other), and a map that is mostly obstacles stays affordable."""
import numpy as np

FAR, OUTSIDE = 0xFFFF, 0xFFFE
BIG = np.int64(1) << 40


def obstacles(log, not_free):
    """the mode's predicate, cell by cell: logData > 0 (NaN, 0, -0.0 are none), or !(logData < 0) (NaN is one)"""
    log = np.asarray(log, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~(log < 0) if not_free else (log > 0)


def _cap(d2, R):
    return np.where(d2 <= np.int64(R) * R, d2, FAR).astype(np.uint16)


def _min_over(ys, xs, oy, ox):
    """min over the list (oy, ox) of the squared distance from every cell of ys x xs, int64 [len(ys)][len(xs)]"""
    d2 = np.full((len(ys), len(xs)), BIG, dtype=np.int64)
    for a in range(0, len(oy), 256):
        dy2 = (ys[:, None] - oy[None, a:a + 256]) ** 2
        dx2 = (xs[:, None] - ox[None, a:a + 256]) ** 2
        d2 = np.minimum(d2, (dy2[:, None, :] + dx2[None, :, :]).min(axis=2))
    return d2


def _rect(log, rect):
    H, W = log.shape
    return (0, 0, W, H) if rect is None else tuple(int(c) for c in rect)


def expect_plain(log, R, not_free=False, rect=None):
    x0, y0, w, h = _rect(log, rect)
    o = np.argwhere(obstacles(log, not_free)).astype(np.int64)
    ys, xs = np.arange(y0, y0 + h, dtype=np.int64), np.arange(x0, x0 + w, dtype=np.int64)
    return _cap(_min_over(ys, xs, o[:, 0], o[:, 1]), R)


def expect(log, R, not_free=False, rect=None, block=16):
    x0, y0, w, h = _rect(log, rect)
    o = np.argwhere(obstacles(log, not_free)).astype(np.int64)
    oy, ox = o[:, 0], o[:, 1]
    out = np.empty((h, w), dtype=np.uint16)
    for ya in range(y0, y0 + h, block):
        yb = min(ya + block, y0 + h)
        rows = (oy >= ya - R) & (oy < yb + R)
        for xa in range(x0, x0 + w, block):
            xb = min(xa + block, x0 + w)
            near = rows & (ox >= xa - R) & (ox < xb + R)
            d2 = _min_over(np.arange(ya, yb, dtype=np.int64), np.arange(xa, xb, dtype=np.int64), oy[near], ox[near])
            out[ya - y0:yb - y0, xa - x0:xb - x0] = _cap(d2, R)
    return out


def cells_of(poses, pos_x, pos_y, resolution):
    """probabilityOf's cell of every pose (GridMap.java:273-274): (int)((x - position.x) / resolution) in double -- the pose's floats and
    the map's float position and resolution widened --, Java's cast: toward zero, NaN -> 0, saturating"""
    p = np.asarray(poses, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    out = []
    for col, pos in ((0, pos_x), (1, pos_y)):
        with np.errstate(invalid="ignore", over="ignore"):
            q = (p[:, col] - np.float64(np.float32(pos))) / np.float64(np.float32(resolution))
        q = np.where(np.isnan(q), 0.0, np.clip(np.trunc(q), -2147483648.0, 2147483647.0))
        out.append(q.astype(np.int64))
    return out[0], out[1]


def expect_poses(field, poses, pos_x, pos_y, resolution):
    """field [H][W] of the whole map -> the value under every pose's cell, OUTSIDE where the cell is off the map (:276)"""
    H, W = field.shape
    gx, gy = cells_of(poses, pos_x, pos_y, resolution)
    inside = (gx >= 0) & (gy >= 0) & (gx < W) & (gy < H)
    out = np.full(len(gx), OUTSIDE, dtype=np.uint16)
    out[inside] = field[gy[inside], gx[inside]]
    return out
