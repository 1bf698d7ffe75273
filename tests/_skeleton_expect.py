"""Expected sites and skeletons (include/gridmapslam.h "sites and skeleton"), brute force in numpy int64 from a downloaded logData: for
every cell the minimum of d2 * 2^32 + index over the list of obstacle cells, then the three skeleton rules literally, by whole-array
shifts.  Nothing here is separable, and nothing knows about bit planes, tiles or tie-breaking by scan order: the key IS the definition.

sites() takes the minimum per block of 16 x 16 cells over the part of the list that lies within max_radius of the block in both axes:
an obstacle further away than that in x or in y is more than max_radius from every cell of the block and cannot be a site of it
(tests/test_skeleton_args.py holds it against the whole list)."""
import numpy as np

from _clearance_expect import cells_of, obstacles  # noqa: F401  (the predicates and the poses' cells are the clearance fields')

NONE, OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE
CLEAR_FAR, CLEAR_OUTSIDE = 0xFFFF, 0xFFFE
TOTALS = ("sited", "skeleton", "min_d2", "max_d2")


def sites(log, R, not_free=False, block=16, rect=None):
    """the site of every cell of the WHOLE map, uint32 [H][W]; block=None: every cell against the whole list; rect = (x0, y0, w, h):
    only the blocks that meet it are computed (the others stay NONE): cut() the result"""
    H, W = log.shape
    rx0, ry0, rw, rh = (0, 0, W, H) if rect is None else rect
    o = np.argwhere(obstacles(log, not_free)).astype(np.int64)
    oy, ox = o[:, 0], o[:, 1]
    idx = oy * W + ox
    out = np.full((H, W), NONE, dtype=np.uint32)
    by, bx = (H, W) if block is None else (block, block)
    for ya in range(0, H, by):
        yb = min(ya + by, H)
        for xa in range(0, W, bx):
            xb = min(xa + bx, W)
            if xb <= rx0 or xa >= rx0 + rw or yb <= ry0 or ya >= ry0 + rh:
                continue
            near = np.ones(len(oy), bool) if block is None else (oy >= ya - R) & (oy < yb + R) & (ox >= xa - R) & (ox < xb + R)
            ny, nx, ni = oy[near], ox[near], idx[near]
            ys, xs = np.arange(ya, yb, dtype=np.int64), np.arange(xa, xb, dtype=np.int64)
            best = np.full((len(ys), len(xs)), np.iinfo(np.int64).max, dtype=np.int64)
            for a in range(0, len(ni), 256):
                d2 = (ys[:, None, None] - ny[None, None, a:a + 256]) ** 2 + (xs[None, :, None] - nx[None, None, a:a + 256]) ** 2
                best = np.minimum(best, (d2 * (np.int64(1) << 32) + ni[None, None, a:a + 256]).min(axis=2))
            ok = (best >> 32) <= np.int64(R) * R
            out[ya:yb, xa:xb] = np.where(ok, best & 0xFFFFFFFF, NONE).astype(np.uint32)
    return out


def d2_of(site):
    """the squared distance from every cell of a WHOLE-MAP site field to its site, int64 [H][W]; -1 where there is none"""
    H, W = site.shape
    s = site.astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    return np.where(s != NONE, (ys - s // W) ** 2 + (xs - s % W) ** 2, -1)


def clearance_of(site):
    """what gms_map_clearance returns for the same mode and radius: d2 as uint16, GMS_CLEAR_FAR where there is no site"""
    d2 = d2_of(site)
    return np.where(d2 >= 0, d2, CLEAR_FAR).astype(np.uint16)


def skeleton(site, min_clear=1, min_gap=2):
    """the skeleton of the WHOLE map from its site field, uint16 [H][W]: d2 on the skeleton cells, else 0"""
    H, W = site.shape
    s = site.astype(np.int64)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    has = s != NONE
    obst = has & (s == idx)
    sy, sx = s // W, s % W
    d2 = d2_of(site)
    cand = has & ~obst & (d2 >= np.int64(min_clear) ** 2)                     # rule 1
    mark = np.zeros((H, W), bool)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        c = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))       # the cells whose neighbour lies inside the map
        n = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))       # ... and those neighbours
        gap = (sy[c] - sy[n]) ** 2 + (sx[c] - sx[n]) ** 2
        rule2 = has[n] & ~obst[n] & (gap >= np.int64(min_gap) ** 2)
        rule3 = (d2[c] > d2[n]) | ((d2[c] == d2[n]) & (idx[c] < idx[n]))
        mark[c] |= cand[c] & rule2 & rule3
    return np.where(mark, d2, 0).astype(np.uint16)


def cut(field, rect):
    x0, y0, w, h = rect
    return field[y0:y0 + h, x0:x0 + w]


def totals(site, skel):
    """(sited, skeleton, min_d2, max_d2) over a rectangle's site and skeleton fields"""
    k = skel[skel != 0].astype(np.int64)
    return (int((site != NONE).sum()), int(len(k)), int(k.min()) if len(k) else 0, int(k.max()) if len(k) else 0)


def totals_of(record):
    """a SKELETON_TOTALS_DTYPE record as the same tuple; its padding must be zero"""
    assert list(np.asarray(record["pad"]).ravel()) == [0, 0]
    return tuple(int(record[n]) for n in TOTALS)


def expect_poses(site, poses, pos_x, pos_y, resolution):
    """WHOLE-MAP site field -> (site, d2) under every pose's cell, uint32 [P] each; (OUTSIDE, CLEAR_OUTSIDE) off the map, (NONE,
    CLEAR_FAR) without a site"""
    H, W = site.shape
    gx, gy = cells_of(poses, pos_x, pos_y, resolution)
    inside = (gx >= 0) & (gy >= 0) & (gx < W) & (gy < H)
    s = np.full(len(gx), OUTSIDE, dtype=np.uint32)
    d = np.full(len(gx), CLEAR_OUTSIDE, dtype=np.uint32)
    s[inside] = site[gy[inside], gx[inside]]
    d[inside] = clearance_of(site)[gy[inside], gx[inside]]
    return s, d
