"""Rooms and doors, restated plainly from include/gridmapslam.h "rooms and doors": the blocked planes by brute force over the obstacle
list, the cores by flood fill, the growth by a heap Dijkstra over (cost, rank) tuples, records and doors by Python loops.  Shares nothing
with the device code; tests/test_rooms_expect.py holds it against answers written out by hand."""
import heapq

import numpy as np

NONE, FAR = 0xFFFFFFFF, 0xFFFF
AXIS, DIAG = 5, 7
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
ROOM_DTYPE = np.dtype([("anchor_x", "<i4"), ("anchor_y", "<i4"), ("core_count", "<i4"), ("count", "<i4"), ("min_x", "<i4"), ("min_y", "<i4"),
                       ("max_x", "<i4"), ("max_y", "<i4"), ("max_depth", "<i4"), ("doors", "<i4"), ("sum_x", "<i8"), ("sum_y", "<i8")])
DOOR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("count", "<i4"), ("min_x", "<i4"), ("min_y", "<i4"), ("max_x", "<i4"), ("max_y", "<i4"),
                       ("pad", "<i4"), ("sum_x2", "<i8"), ("sum_y2", "<i8")])


def blocked(log, R, not_free):
    """BLOCKED for (mode, R): an obstacle cell within R cells, d2 <= R^2; cells off the map are no obstacles"""
    log = np.asarray(log, dtype=np.float64)
    H, W = log.shape
    obstacle = ~(log < 0) if not_free else (log > 0)
    d = np.arange(-R, R + 1)
    disc = (d[:, None] ** 2 + d[None, :] ** 2) <= R * R
    out = np.zeros((H, W), dtype=bool)
    for y, x in np.argwhere(obstacle).tolist():
        ya, yb, xa, xb = max(0, y - R), min(H, y + R + 1), max(0, x - R), min(W, x + R + 1)
        out[ya:yb, xa:xb] |= disc[ya - y + R:yb - y + R, xa - x + R:xb - x + R]
    return out


def cores(core_cell):
    """[(anchor (y, x), [cells (y, x)])] of the maximal 4-connected sets, in ascending anchor order"""
    H, W = core_cell.shape
    seen = np.zeros((H, W), dtype=bool)
    out = []
    for y0, x0 in np.argwhere(core_cell).tolist():                              # (row-major: the first cell met of a core is its anchor)
        if seen[y0, x0]:
            continue
        seen[y0, x0] = True
        stack, cells = [(y0, x0)], []
        while stack:
            y, x = stack.pop()
            cells.append((y, x))
            for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= ny < H and 0 <= nx < W and core_cell[ny, nx] and not seen[ny, nx]:
                    seen[ny, nx] = True
                    stack.append((ny, nx))
        out.append(((y0, x0), cells))
    return out


def expect(log, core=15, inflate=5, not_free=True, min_core=1, max_cost=0xFFFE, rect=None):
    """{"labels", "depth" (of rect = (x0, y0, w, h), None: the whole map), "rooms", "doors", "n_rooms", "n_doors"}"""
    log = np.asarray(log, dtype=np.float64)
    H, W = log.shape
    assert 0 <= inflate < core <= 255 and min_core >= 1 and 1 <= max_cost <= 0xFFFE
    free = ~blocked(log, inflate, not_free)
    core_cell = ~blocked(log, core, not_free)
    assert not (core_cell & ~free).any(), "every core cell is traversable"
    rooms = [c for c in cores(core_cell) if len(c[1]) >= min_core]
    best = {}
    heap = []
    for rank, (_, cells) in enumerate(rooms):
        for c in cells:
            best[c] = (0, rank)
            heap.append((0, rank, c[0], c[1]))
    heapq.heapify(heap)
    while heap:
        cost, rank, y, x = heapq.heappop(heap)
        if best[(y, x)] != (cost, rank):
            continue
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ny, nx = y + dy, x + dx
                if (dy == 0 and dx == 0) or not (0 <= ny < H and 0 <= nx < W) or not free[ny, nx]:
                    continue
                if dy != 0 and dx != 0 and not (free[y, nx] and free[ny, x]):   # no corner cutting: both squeezed cells
                    continue
                cand = (cost + (DIAG if dy != 0 and dx != 0 else AXIS), rank)
                if cand[0] <= max_cost and cand < best.get((ny, nx), (1 << 30, 0)):
                    best[(ny, nx)] = cand
                    heapq.heappush(heap, (cand[0], cand[1], ny, nx))
    anchors = [a[0] * W + a[1] for a, _ in rooms]
    labels = np.full((H, W), NONE, dtype=np.uint32)
    depth = np.full((H, W), FAR, dtype=np.uint16)
    rank_of = np.full((H, W), -1, dtype=np.int64)
    rec = np.zeros(len(rooms), dtype=ROOM_DTYPE)
    for k, ((ay, ax), cells) in enumerate(rooms):
        rec[k] = (ax, ay, len(cells), 0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0, 0, 0, 0)
    for (y, x), (cost, rank) in best.items():
        labels[y, x], depth[y, x], rank_of[y, x] = anchors[rank], cost, rank
        r = rec[rank]
        r["count"] += 1
        r["min_x"], r["min_y"], r["max_x"], r["max_y"] = min(r["min_x"], x), min(r["min_y"], y), max(r["max_x"], x), max(r["max_y"], y)
        r["max_depth"] = max(r["max_depth"], cost)
        r["sum_x"] += x
        r["sum_y"] += y
    pairs = {}
    for y in range(H):
        for x in range(W):
            a = rank_of[y, x]
            if a < 0:
                continue
            for qy, qx in ((y, x + 1), (y + 1, x)):                             # east and south: every contact once
                if qy < H and qx < W and rank_of[qy, qx] >= 0 and rank_of[qy, qx] != a:
                    b = rank_of[qy, qx]
                    pairs.setdefault((min(a, b), max(a, b)), []).append((x, y, qx, qy))
    doors = np.zeros(len(pairs), dtype=DOOR_DTYPE)
    for i, (a, b) in enumerate(sorted(pairs)):
        c = pairs[(a, b)]
        xs = [v for p in c for v in (p[0], p[2])]
        ys = [v for p in c for v in (p[1], p[3])]
        doors[i] = (anchors[a], anchors[b], len(c), min(xs), min(ys), max(xs), max(ys), 0, sum(xs), sum(ys))
        rec["doors"][a] += 1
        rec["doors"][b] += 1
    x0, y0, w, h = (0, 0, W, H) if rect is None else rect
    return {"labels": labels[y0:y0 + h, x0:x0 + w].copy(), "depth": depth[y0:y0 + h, x0:x0 + w].copy(), "rooms": rec, "doors": doors, "n_rooms": len(rec),
            "n_doors": len(doors)}


def same(got, want, where):
    """the dict of GridMap.rooms (or of a particle's) against expect()'s, with the first difference named"""
    assert (got["n_rooms"], got["n_doors"]) == (want["n_rooms"], want["n_doors"]), f"{where}: {got['n_rooms']} rooms, {got['n_doors']} doors != {want['n_rooms']}, {want['n_doors']}"
    for name in ("labels", "depth"):
        if got[name] is None:
            continue
        g, w_ = got[name], want[name]
        assert g.dtype == w_.dtype and g.shape == w_.shape, f"{where}: {name}"
        bad = np.argwhere(g != w_)
        assert np.array_equal(g, w_), f"{where}: {len(bad)} of {w_.size} {name} differ, first at (y, x) = {bad[0].tolist()}: {g[tuple(bad[0])]} != {w_[tuple(bad[0])]}"
    for name in ("rooms", "doors"):
        g, w_ = got[name], want[name]
        assert g.dtype == w_.dtype and g.shape == w_.shape, f"{where}: {name} {g.shape} != {w_.shape}"
        bad = np.nonzero(g != w_)[0]
        assert np.array_equal(g, w_), f"{where}: {len(bad)} of {len(w_)} {name} differ, first {bad[0]}: {g[bad[0]]} != {w_[bad[0]]}"


# ---- the maps the tests share ------------------------------------------------------------------------------------------------------------
def walls(W, H):
    """an all-occupied map to carve free space out of"""
    return np.full((H, W), L_OCC)


def carve(log, x0, y0, x1, y1, value=L_FREE):
    """the inclusive cell box (x0, y0) .. (x1, y1) set to value"""
    log[min(y0, y1):max(y0, y1) + 1, min(x0, x1):max(x0, x1) + 1] = value
    return log


def two_boxes(W=46, H=24, ox=0, oy=0, gap=(10, 12)):
    """two 20 x 20 free boxes at (2 + ox, 2 + oy) and (23 + ox, 2 + oy), the wall column x = 22 + ox between them open at rows
    gap[0] + oy .. gap[1] + oy"""
    log = walls(W, H)
    carve(log, 2 + ox, 2 + oy, 21 + ox, 21 + oy)
    carve(log, 23 + ox, 2 + oy, 42 + ox, 21 + oy)
    carve(log, 22 + ox, gap[0] + oy, 22 + ox, gap[1] + oy)
    return log


def random_floor(seed, W=200, H=136):
    """a floor plan: 4 x 3 rooms behind jittered one-cell walls, a door of 2 .. 7 cells in most shared walls, a few pillars and a few
    never-observed patches (0.0, -0.0, NaN)"""
    rng = np.random.default_rng(seed)
    log = np.full((H, W), L_FREE)
    xs = [0] + [int(W * k / 4 + rng.integers(-9, 10)) for k in (1, 2, 3)] + [W - 1]
    ys = [0] + [int(H * k / 3 + rng.integers(-7, 8)) for k in (1, 2)] + [H - 1]
    for x in xs:
        log[:, x] = L_OCC
    for y in ys:
        log[y, :] = L_OCC
    for i in range(4):
        for j in range(3):
            if i < 3 and rng.random() < 0.8:                                    # a door in the wall to the east
                y = int(rng.integers(ys[j] + 2, ys[j + 1] - 8))
                log[y:y + int(rng.integers(2, 8)), xs[i + 1]] = L_FREE
            if j < 2 and rng.random() < 0.8:                                    # ... and to the south
                x = int(rng.integers(xs[i] + 2, xs[i + 1] - 8))
                log[ys[j + 1], x:x + int(rng.integers(2, 8))] = L_FREE
    for _ in range(6):
        x, y = int(rng.integers(3, W - 6)), int(rng.integers(3, H - 6))
        log[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = L_OCC
    for v in (0.0, -0.0, np.nan):
        x, y = int(rng.integers(3, W - 8)), int(rng.integers(3, H - 8))
        log[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 5))] = v
    return log


def corridor(tall_right=False):
    """two 9 x 9 rooms joined by a one-cell corridor of 11 cells along y = 7 whose middle cell (15, 7) is equally far from both cores;
    tall_right: the right room reaches two rows further up, so its anchor is the smaller one"""
    log = walls(31, 13)
    carve(log, 1, 3, 9, 11)
    carve(log, 21, 1 if tall_right else 3, 29, 11)
    carve(log, 10, 7, 20, 7)
    return log
