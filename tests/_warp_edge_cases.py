"""The inputs of tests/test_gpu_warp_edges.py: map warps (include/gridmapslam.h "map warps") across resolutions, with cell centres
exactly on a source cell's edge, under poses at the ends of what gms_warp_check accepts.  Builders only, numpy, no device; what the
cases must contain, and the answers derived by hand, are held against the restatement (tests/_warp_expect.py) in
tests/test_warp_edge_inputs.py.

Dyadic grids -- resolution and corner powers of two and small multiples of them -- survive the float storage of gms_params, and every
product, sum and quotient of the warp's arithmetic on them is exact.  A destination centre can then sit exactly on a source cell's
edge, where `floor` decides (the cell above and to the right takes the tie) and `0 <= q < W` is met with equality.  Exact arithmetic
cannot tell a fused multiply-add from two roundings, so the 3-4-5 turn keeps the dyadic grids and takes c = 0.8, s = 0.6: the products
are no longer exact, a fifth of the centres' images lie on an edge in real numbers, and on the source's first edges, where the two
products cancel, the separately rounded `c * dx + s * dy` and a fused one fall on different sides."""
import functools
from collections import namedtuple

import numpy as np

import _warp_cases as wc
import _warp_expect as wx

L_OCC, L_FREE = wc.L_OCC, wc.L_FREE
VALUES = np.array([0.0, -0.0, np.nan, L_FREE, 2 * L_FREE, L_OCC, 4 * L_OCC])
START = np.array([L_FREE, 0.0, 3 * L_OCC, np.nan, -0.0, 2 * L_FREE, L_OCC])       # what a destination holds before the call
OPS = ("compare", "replace", "add", "fill")
ADD_CLAMP = 1.0

# a grid: (W, H, resolution, (corner x, corner y))
FINE = (96, 70, 0.0625, (-1.5, 0.25))
COARSE = (48, 35, 0.125, (-1.5, 0.25))
GRID = (70, 66, 0.125, (0.5, -2.0))
CORNER = (40, 36, 0.125, (0.0, 0.0))
THREE_FOUR_FIVE = "3-4-5 turn onto the source's corner"
RAGGED = (63, 1, 3, 64)                                 # columns 63 .. 65: both sides of a 64-lane row boundary; 64 rows: a wavefront's last
CM1, CM8 = (400, 300, 0.01, (-2.0, -1.5)), (60, 45, 0.08, (0.3, -0.7))
CM20, MM25 = (12, 9, 0.2, (1.0, 2.0)), (130, 70, 0.025, (-0.5, 0.25))

# hand: None, or (values [H_d][W_d], mask [H_d][W_d]) -- the source value every destination cell sees and whether it sees one, derived
# from the geometry by slices alone; n_outside: the count over the whole map (None: whatever the restatement says)
Case = namedtuple("Case", "name dst src seed pose rect hand n_outside")


def geometry(grid):
    W, H, res, pos = grid
    return wx.Geometry.make(W, H, res, *pos)


def size_of(grid):
    """the metres GridMap takes for the grid's cells"""
    W, H, res, _ = grid
    return wc.metres(W, res), wc.metres(H, res)


@functools.lru_cache(maxsize=None)
def source_log(grid, seed):
    """[H][W] drawn from VALUES; read-only, shared"""
    W, H = grid[:2]
    log = VALUES[np.random.default_rng(seed).integers(0, len(VALUES), size=(H, W))]
    log.setflags(write=False)
    return log


@functools.lru_cache(maxsize=None)
def start_log(grid):
    """[H][W]: a pattern with every class and every kind of unknown in every row and column; read-only, shared"""
    W, H = grid[:2]
    log = START[np.add.outer(3 * np.arange(H), np.arange(W)) % len(START)]
    log.setflags(write=False)
    return log


def _hand(grid, dst_slices, src_view):
    W, H = grid[:2]
    vals, mask = np.zeros((H, W)), np.zeros((H, W), bool)
    vals[dst_slices] = src_view
    mask[dst_slices] = True
    return vals, mask


def _all(grid, src_view):
    return _hand(grid, (slice(None), slice(None)), src_view)


def _none(grid):
    W, H = grid[:2]
    return np.zeros((H, W)), np.zeros((H, W), bool)


def by_hand(case):
    """(the destination after REPLACE, n_outside) from case.hand, over case.rect"""
    vals, mask = case.hand
    W, H = case.dst[:2]
    x0, y0, w, h = case.rect or (0, 0, W, H)
    rect = np.zeros((H, W), bool)
    rect[y0:y0 + h, x0:x0 + w] = True
    out = start_log(case.dst).copy()
    put = mask & rect
    wx.bits(out)[put] = wx.bits(vals)[put]
    return out, int((rect & ~mask).sum())


NEAR_UNIT = 1.0 + 3e-7                                  # |c*c + s*s - 1| = 6e-7: inside gms_warp_check's 1e-6
REFUSED_UNIT = 1.0 + 1e-6                               # 2e-6: outside


def near_unit_pose(k):
    """(0.6 k, 0.8 k) with a fractional t that lays GRID's middle, turned, (ox, oy) beside GRID's middle.  The centres' images under
    k = 1 repeat every tenth of a cell in u, and 0.6 ox + 0.8 oy is a tenth of a cell and 0.2 micrometres: hundreds of images lie
    that close to an edge, and the 0.3 micrometres per metre by which k stretches them decide their cell"""
    g = geometry(GRID)
    c, s = 0.6 * k, 0.8 * k
    ax, ay = g.px + 35 * g.res, g.py + 33 * g.res
    return (ax + 0.049235 - (c * ax - s * ay), ay - 0.0213 - (s * ax + c * ay), c, s)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    r = 0.125
    W, H = GRID[:2]
    px, py = GRID[3]

    def add(name, dst, src, seed, pose, rect=None, hand=None, n_outside=None):
        out.append(Case(name, dst, src, seed, tuple(float(v) for v in pose), rect, hand, n_outside))

    # across resolutions, identity pose on one corner: every coarse centre is a fine cell's corner
    fine = source_log(FINE, 9670)
    add("2:1 fine into coarse", COARSE, FINE, 9670, (0.0, 0.0, 1.0, 0.0), hand=_all(COARSE, fine[1::2, 1::2]), n_outside=0)
    coarse = source_log(COARSE, 4835)
    add("1:2 coarse into fine", FINE, COARSE, 4835, (0.0, 0.0, 1.0, 0.0), hand=_all(FINE, np.repeat(np.repeat(coarse, 2, 0), 2, 1)), n_outside=0)
    # one grid on both sides: every centre on the corner of four source cells
    src = source_log(GRID, 7066)
    turned = src[::-1, ::-1]
    middle = (2 * (px + 35 * r), 2 * (py + 33 * r))
    lower, upper = (slice(0, H - 1), slice(0, W - 1)), (slice(1, H), slice(1, W))
    ties = [("half a cell up and right", (r / 2, r / 2, 1.0, 0.0), _all(GRID, src), 0),
            ("half a cell down and left", (-r / 2, -r / 2, 1.0, 0.0), _hand(GRID, lower, src[1:, 1:]), W + H - 1),
            ("half turn about the middle", (*middle, -1.0, 0.0), _all(GRID, turned), 0),
            ("half turn and half a cell", (middle[0] + r / 2, middle[1] + r / 2, -1.0, 0.0), _hand(GRID, upper, turned[:-1, :-1]), W + H - 1)]
    for name, pose, hand, n_out in ties:
        add(name, GRID, GRID, 7066, pose, hand=hand, n_outside=n_out)
    for name, pose, hand, n_out in ties:
        add(name + ", ragged", GRID, GRID, 7066, pose, rect=RAGGED, hand=hand, n_outside=n_out)
    # c = 0.8, s = 0.6 and a dyadic t that is whole cells from the centres: the source's corner, and with it the lines u = 0 and v = 0,
    # cross the destination, and on them c * dx and s * dy cancel -- what is left is their rounding, and its sign picks the side
    add(THREE_FOUR_FIVE, GRID, CORNER, 4036, (4.5625, 0.5625, 0.8, 0.6))
    # ratios that are no power of two, both directions
    g1, g8 = geometry(CM1), geometry(CM8)
    add("1 cm into 8 cm, 0.3 rad", CM8, CM1, 400300,
        wc.turned(0.3, (g1.px + 200 * g1.res, g1.py + 150 * g1.res), (g8.px + 30.3 * g8.res, g8.py + 22.8 * g8.res)))
    g20, g25 = geometry(CM20), geometry(MM25)
    add("20 cm into 2.5 cm, -1.1 rad", MM25, CM20, 1209,
        wc.turned(-1.1, (g20.px + 6 * g20.res, g20.py + 4.5 * g20.res), (g25.px + 65.3 * g25.res, g25.py + 34.8 * g25.res)))
    # finite poses whose arithmetic overflows, or leaves every integer format: nothing is inside, nothing is gathered
    for pose in ((1e300, 0.0, 1.0, 0.0), (1.7e308, -1.7e308, 0.6, 0.8), (1e19, 1e19, 0.0, 1.0)):
        add(f"far away {pose[0]:g}", GRID, GRID, 7066, pose, hand=_none(GRID), n_outside=W * H)
    # (c, s) not quite unit: accepted, and used as it is
    add("near-unit (c, s)", GRID, GRID, 7066, near_unit_pose(NEAR_UNIT))
    return tuple(out)


def names():
    return [c.name for c in cases()]


def expect(case, op):
    """the restatement's (destination afterwards, counts) for case under op, from start_log"""
    return wx.expect(start_log(case.dst), geometry(case.dst), source_log(case.src, case.seed), geometry(case.src), case.pose, op, rect=case.rect,
                     clamp=ADD_CLAMP if op == "add" else 0.0)
