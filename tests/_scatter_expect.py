"""Expected particle seeding (include/gridmapslam.h "particle seeding") from a downloaded logData, on the host: the eligible cells are
log < 0 inside the rectangle and not within `inflate` of an obstacle (_reach_expect.blocked: a brute-force d2 <= inflate^2 over the
obstacle list), ranked by y * W + x; the draw is the oracle's Philox block on {global slot + (map << 40), sequence}; the rank is formed
with Python integers and the pose with np.float32 / np.float64 operations in the header's order.  Nothing here knows about bit planes,
scans or searches.  Every pose produced is also held against the cell rule of gms_map_clearance_poses: it must lie in the drawn cell."""
import functools

import numpy as np

import _reach_expect as rx
from oracle import oracle as orc

M32 = 0xFFFFFFFF


def eligible(log, rect=None, inflate=0, not_free=True):
    """bool [H][W]"""
    log = np.asarray(log, dtype=np.float64)
    H, W = log.shape
    x0, y0, w, h = (0, 0, W, H) if rect is None else (int(c) for c in rect)
    with np.errstate(invalid="ignore"):
        e = log < 0
    inside = np.zeros((H, W), bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    e = e & inside
    if inflate > 0:
        e = e & ~rx.blocked(log, inflate, not_free)
    return e


def ranked(elig):
    """(cx, cy) int64 arrays of the eligible cells in ascending y * W + x"""
    cy, cx = np.nonzero(elig)                                  # row-major: ascending y, then x
    return cx.astype(np.int64), cy.astype(np.int64)


@functools.lru_cache(maxsize=1 << 16)
def philox(seed, g, sequence):
    """the four output words of the block with key `seed` and counter {g, sequence}"""
    return tuple(orc.philox4x32([g & M32, (g >> 32) & M32, sequence & M32, (sequence >> 32) & M32], [seed & M32, (seed >> 32) & M32]))


def rank_of(c, M):
    """mulhi64(c0:c1, M) in Python integers"""
    return (((c[0] << 32) | c[1]) * M) >> 64


def jitter_of(c2):
    """(jx, jy) as np.float32, exact"""
    return (np.float32(32768 + 7 * (c2 >> 16)) * np.float32(2.0 ** -19), np.float32(32768 + 7 * (c2 & 0xFFFF)) * np.float32(2.0 ** -19))


def pose_of(c, cx, cy, pos, res, jitter=True):
    """float32 [3] of the draw c in cell (cx, cy) of a map at `pos` (float32 values) with resolution `res`"""
    jx, jy = jitter_of(c[2]) if jitter else (np.float32(0.5), np.float32(0.5))
    out = np.empty(3, np.float32)
    for k, (cell, j) in enumerate(((cx, jx), (cy, jy))):
        f = np.float32(np.float32(cell) + j)                                   # one float add
        v = np.float32(np.float64(np.float32(pos[k])) + np.float64(f) * np.float64(np.float32(res)))
        back = int((np.float64(v) - np.float64(np.float32(pos[k]))) / np.float64(np.float32(res)))     # gms_map_clearance_poses' cell
        assert back == cell, f"the pose {v!r} of cell {cell} (axis {k}) lies in cell {back}"
        out[k] = v
    out[2] = np.float32((np.float64(c[3] >> 8) - 8388607.5) * (np.pi * 2.0 ** -23))
    assert -np.pi < float(out[2]) < np.pi
    return out


def expect(log, pos, res, first, count, seed, sequence, rect=None, inflate=0, not_free=True, jitter=True, offset=0, mi=0):
    """(poses float32 [count][3] of slots first .. first + count - 1, cells int64 [count][2], M) for map mi's filter of a handle whose
    slot 0 is the global slot `offset`; M == 0: (None, None, 0)"""
    cx, cy = ranked(eligible(log, rect, inflate, not_free))
    M = len(cx)
    if M == 0:
        return None, None, 0
    poses = np.empty((count, 3), np.float32)
    cells = np.empty((count, 2), np.int64)
    for i in range(count):
        c = philox(seed, (offset + first + i) + (mi << 40), sequence)
        r = rank_of(c, M)
        assert 0 <= r < M
        cells[i] = cx[r], cy[r]
        poses[i] = pose_of(c, int(cx[r]), int(cy[r]), pos, res, jitter)
    return poses, cells, M
