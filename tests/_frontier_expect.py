"""The expectation for frontier regions (include/gridmapslam.h "frontier regions"), in the plainest form: the mask from numpy shifts of
the three cell classes, the regions from a breadth-first flood fill over the mask's cells in linear order, records and labels from the
member lists.  Shares nothing with the library's tiles, planes, unions or scans."""
import collections

import numpy as np

NONE = 0xFFFFFFFF
FAR = 0xFFFF
DTYPE = np.dtype([("anchor_x", "<i4"), ("anchor_y", "<i4"), ("count", "<i4"), ("goal_cost", "<i4"), ("min_x", "<i4"), ("min_y", "<i4"),
                  ("max_x", "<i4"), ("max_y", "<i4"), ("goal_x", "<i4"), ("goal_y", "<i4"), ("sum_x", "<i8"), ("sum_y", "<i8")])


def classes(log):
    """(free, occupied, unknown): logData < 0, > 0, neither (0, -0.0, NaN)"""
    with np.errstate(invalid="ignore"):
        free, occ = log < 0, log > 0
    return free, occ, ~(free | occ)


def near_occupied(occ, inflate):
    """cells with an occupied cell within `inflate` cells: d2 <= inflate^2"""
    H, W = occ.shape
    out = np.zeros((H, W), dtype=bool)
    if inflate <= 0:
        return out
    R = int(inflate)
    dy, dx = np.mgrid[-R:R + 1, -R:R + 1]
    disc = dy * dy + dx * dx <= R * R
    for y, x in np.argwhere(occ):
        ya, yb, xa, xb = max(0, y - R), min(H, y + R + 1), max(0, x - R), min(W, x + R + 1)
        out[ya:yb, xa:xb] |= disc[ya - y + R:yb - y + R, xa - x + R:xb - x + R]
    return out


def mask(log, inflate=0):
    """the frontier cells: free, an unknown axis neighbour inside the map, no occupied cell within inflate"""
    free, occ, unk = classes(np.asarray(log))
    beside = np.zeros(unk.shape, dtype=bool)
    beside[:, 1:] |= unk[:, :-1]
    beside[:, :-1] |= unk[:, 1:]
    beside[1:, :] |= unk[:-1, :]
    beside[:-1, :] |= unk[1:, :]
    return free & beside & ~near_occupied(occ, inflate)


def regions(m):
    """the maximal 8-connected sets of m's cells, each a list of (y, x) -- in ascending order of their smallest linear index"""
    H, W = m.shape
    seen = np.zeros((H, W), dtype=bool)
    out = []
    for y, x in np.argwhere(m):
        if seen[y, x]:
            continue
        seen[y, x] = True
        cells, queue = [], collections.deque([(int(y), int(x))])
        while queue:
            cy, cx = queue.popleft()
            cells.append((cy, cx))
            for ny in (cy - 1, cy, cy + 1):
                for nx in (cx - 1, cx, cx + 1):
                    if 0 <= ny < H and 0 <= nx < W and m[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        queue.append((ny, nx))
        out.append(cells)
    return out


def expect(log, min_size=1, inflate=0, cost=None, rect=None):
    """(records of the regions with count >= min_size, in anchor order; n_found; the label field of rect = (x0, y0, w, h), None: whole)"""
    log = np.asarray(log)
    H, W = log.shape
    labels = np.full((H, W), NONE, dtype=np.uint32)
    recs = []
    for cells in regions(mask(log, inflate)):
        ys, xs = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
        lin = ys * W + xs
        a = int(lin.min())
        labels[ys, xs] = a
        if len(cells) < min_size:
            continue
        goal = (-1, -1, FAR)
        if cost is not None:
            c = np.asarray(cost)[ys, xs].astype(np.int64)
            if (c != FAR).any():
                key = np.where(c != FAR, c * (1 << 32) + lin, np.iinfo(np.int64).max)
                g = int(lin[np.argmin(key)])
                goal = (g % W, g // W, int(c.min()))
        recs.append((a % W, a // W, len(cells), goal[2], xs.min(), ys.min(), xs.max(), ys.max(), goal[0], goal[1], xs.sum(), ys.sum()))
    rec = np.array(recs, dtype=DTYPE) if recs else np.zeros(0, dtype=DTYPE)
    assert (np.diff(rec["anchor_y"].astype(np.int64) * W + rec["anchor_x"]) > 0).all()
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    return rec, len(rec), labels[y0:y0 + h, x0:x0 + w].copy()
