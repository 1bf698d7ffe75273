"""Expected cost-to-go fields (include/gridmapslam.h "cost-to-go fields") from a downloaded logData, on the host: the blocked cells are
the cells within `inflate` of an obstacle of _clearance_expect.obstacles (a brute-force d2 <= inflate^2 over the obstacle list), then
plain Dijkstra with heapq over the 8-neighbour graph -- an axis step 5, a diagonal step 7 and only between two traversable side cells
--, then the cap.  Nothing here knows about tiles, rounds or bit planes."""
import heapq

import numpy as np

import _clearance_expect as xe

FAR, AXIS, DIAG = 0xFFFF, 5, 7
_STEPS = ((1, 0, AXIS), (-1, 0, AXIS), (0, 1, AXIS), (0, -1, AXIS), (1, 1, DIAG), (1, -1, DIAG), (-1, 1, DIAG), (-1, -1, DIAG))


def blocked(log, inflate=0, not_free=True):
    """bool [H][W]: an obstacle cell of the mode's predicate within `inflate` cells (d2 <= inflate^2)"""
    obs = xe.obstacles(log, not_free)
    if inflate == 0:
        return obs
    H, W = obs.shape
    o = np.argwhere(obs).astype(np.int64)
    if len(o) == 0:
        return obs
    d2 = xe._min_over(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), o[:, 0], o[:, 1])
    return d2 <= np.int64(inflate) * inflate


def costs(block, seeds):
    """int64 [H][W]: the cheapest path's cost from any seed, -1 where there is none (no cap)"""
    H, W = block.shape
    free = (~block).tolist()
    INF = 1 << 60
    dist = [[INF] * W for _ in range(H)]
    heap = []
    for x, y in np.asarray(seeds, dtype=np.int64).reshape(-1, 2).tolist():
        if 0 <= x < W and 0 <= y < H and free[y][x] and dist[y][x] != 0:
            dist[y][x] = 0
            heap.append((0, x, y))
    heapq.heapify(heap)
    while heap:
        d, x, y = heapq.heappop(heap)
        if d != dist[y][x]:
            continue
        for dx, dy, c in _STEPS:
            nx, ny = x + dx, y + dy
            if not (0 <= nx < W and 0 <= ny < H) or not free[ny][nx]:
                continue
            if c == DIAG and not (free[y][nx] and free[ny][x]):         # the two cells the step squeezes between
                continue
            if d + c < dist[ny][nx]:
                dist[ny][nx] = d + c
                heapq.heappush(heap, (d + c, nx, ny))
    out = np.array(dist, dtype=np.int64)
    out[out == INF] = -1
    return out


def cap(cost, max_cost=0xFFFE, rect=None):
    f = np.where((cost >= 0) & (cost <= max_cost), cost, FAR).astype(np.uint16)
    if rect is not None:
        x0, y0, w, h = rect
        f = f[y0:y0 + h, x0:x0 + w]
    return f


def expect(log, seeds, max_cost=0xFFFE, inflate=0, not_free=True, rect=None):
    return cap(costs(blocked(log, inflate, not_free), seeds), max_cost, rect)


def closed_form(W, H, seed):
    """an empty map: 7 min(|dx|, |dy|) + 5 ||dx| - |dy||"""
    dx = np.abs(np.arange(W, dtype=np.int64) - seed[0])[None, :]
    dy = np.abs(np.arange(H, dtype=np.int64) - seed[1])[:, None]
    return DIAG * np.minimum(dx, dy) + AXIS * np.abs(dx - dy)
