"""The clearance fields and the sites are ONE separable transform (gms_nearest_device.h) under two policies -- the distance alone, and
the site -- in a field form and a poses form each.  The four must tell the same story: d2 recomputed from a site is the clearance, and
the value under a pose is the field's at the pose's cell.  Every expectation is the brute force of tests/_clearance_expect.py and
tests/_skeleton_expect.py, which share nothing with the kernels, so agreeing with each other is not enough to pass.  All integers,
array_equal everywhere.

The map is 70 x 67 cells: three plane words per row, the last one ragged, behind them the row's padding; H is just over the smallest
tile height of 64, so the whole map at R = 1 is two bands (rows 0 .. 63 and 64 .. 66) whose halos are clipped by the map.  At R = 33
and R = 255 a tile is the whole rectangle, and at 255 the staged rows are clipped to H.  The rectangle (33, 1) + 36 x 65 starts off a
word and has its own band boundary at R = 1, between rows 64 and 65.

About 1 % of the cells are occupied and about 1 % unknown (obstacles under "not free" alone), plus the four corners.  Planted at d = 1,
where every R decides them:
  the tie rule   across the bands: a free cell between an obstacle above and one below (the upper one is the site) at rows 63 and 64;
                 across the words: a free cell between an obstacle left and one right (the left one) at columns 31, 32, 63 and 64;
  the exit tests a free cell with an obstacle beside it in its row and one straight above it, at rows 64 and 65: after the row itself
                 the best d2 is 1, and at k = 1 the distance may leave on k^2 >= best while the site must not (k^2 > d2(best)): the
                 upper obstacle ties on d2 and wins on the index."""
import functools

import numpy as np
import pytest

import _clearance_expect as xe
import _reach_expect as rx
import _skeleton_expect as xs
from gridmap_slam_robot_amd import GridMap

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 70, 67
WM, HM = 3.48, 3.33                                     # metres: 69.6 and 66.6 cells, rounded up
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
RECT = (33, 1, 36, 65)
# (the free cell, its site, the other obstacle at the same distance): (x, y) each
BAND_TIES = [((40, 63), (40, 62), (40, 64)), ((50, 64), (50, 63), (50, 65))]
WORD_TIES = [((31, 20), (30, 20), (32, 20)), ((32, 26), (31, 26), (33, 26)), ((63, 32), (62, 32), (64, 32)), ((64, 38), (63, 38), (65, 38))]
EXIT_TRAPS = [((58, 64), (58, 63), (59, 64)), ((44, 65), (44, 64), (45, 65))]
PLANTED = BAND_TIES + WORD_TIES + EXIT_TRAPS


@functools.lru_cache(maxsize=None)
def _log():
    rng = np.random.default_rng(7067)
    u = rng.random((H, W))
    log = np.where(u < 0.01, L_OCC, np.where(u < 0.02, 0.0, L_FREE))
    log[0, 0] = log[0, W - 1] = log[H - 1, 0] = log[H - 1, W - 1] = L_OCC
    for (cx, cy), a, b in PLANTED:
        log[cy - 1:cy + 2, cx - 1:cx + 2] = L_FREE      # nothing else at d2 <= 2 of the cell
        log[a[1], a[0]] = log[b[1], b[0]] = L_OCC
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def _want(R, not_free):
    """(clearance [H][W], sites [H][W]) of the whole map, brute force, each from its own helper"""
    c, s = xe.expect(_log(), R, not_free), xs.sites(_log(), R, not_free)
    c.flags.writeable = s.flags.writeable = False
    return c, s


@functools.lru_cache(maxsize=None)
def _centres():
    """a pose at the centre of every cell, row by row"""
    ys, xs_ = np.mgrid[0:H, 0:W]
    p = np.column_stack([(xs_.ravel() + 0.5) * RES, (ys.ravel() + 0.5) * RES, np.zeros(W * H)]).astype(np.float32)
    p.flags.writeable = False
    return p


def _map():
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=128)
    assert (m.W, m.H) == (W, H)
    m.upload_log(_log())
    return m


def _same(got, want, where):
    assert got.dtype == want.dtype and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{where}: {len(bad)} of {want.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _the_cases_occur(R, not_free):
    """what the brute-force expectation must contain for the comparison to mean something"""
    clear, site = _want(R, not_free)
    assert (site != xs.NONE).any() and (clear == 0).any(), "sites are found"
    if R == 1:
        assert (site == xs.NONE).any() and (clear == xe.FAR).any(), "the FAR case"
        assert (clear[63:65] != xe.FAR).any() and (clear[:, 31:33] != xe.FAR).any() and (clear[:, 63:65] != xe.FAR).any()
    else:
        ys, xs_ = np.mgrid[0:H, 0:W]
        assert ((site != xs.NONE) & (site // W != ys) & (site % W != xs_)).any(), "sites off the cell's row and column"
    for (cx, cy), a, b in PLANTED:
        assert (a[0] - cx) ** 2 + (a[1] - cy) ** 2 == 1 == (b[0] - cx) ** 2 + (b[1] - cy) ** 2 and a[1] * W + a[0] < b[1] * W + b[0]
        assert clear[cy, cx] == 1 and site[cy, cx] == a[1] * W + a[0], f"two obstacles at d2 = 1 of ({cx}, {cy}): the smaller index is the site"
    for (cx, cy), a, b in BAND_TIES:
        assert a[0] == b[0] == cx and a[1] == cy - 1 and b[1] == cy + 1 and cy in (63, 64)
    for (cx, cy), a, b in WORD_TIES:
        assert a[1] == b[1] == cy and a[0] == cx - 1 and b[0] == cx + 1 and (a[0] // 32 != cx // 32 or b[0] // 32 != cx // 32)
    for (cx, cy), a, b in EXIT_TRAPS:
        assert a == (cx, cy - 1) and b == (cx + 1, cy) and cy in (64, 65)
    assert all(RECT[0] <= cx < RECT[0] + RECT[2] for (cx, cy), _, _ in BAND_TIES + EXIT_TRAPS), "the rectangle holds them as well"


@pytest.mark.parametrize("not_free", [False, True], ids=["occupied", "not_free"])
@pytest.mark.parametrize("R", [1, 33, 255])
def test_fields_and_poses_of_both_policies_agree(R, not_free):
    _the_cases_occur(R, not_free)
    clear, site = _want(R, not_free)
    assert np.array_equal(xs.clearance_of(site), clear), "the two brute forces tell the same story"
    m = _map()
    for rect in ((0, 0, W, H), RECT):
        where = f"R = {R}, {'not free' if not_free else 'occupied'}, rect {rect}"
        got_clear = m.clearance(rect, R, not_free)
        got_site = m.skeleton(rect, R, not_free, skel=False, totals=False)[0]
        print(f"{where}: clearance {int((got_clear != xs.cut(clear, rect)).sum())}, sites {int((got_site != xs.cut(site, rect)).sum())} of {got_site.size} differ")
        _same(got_clear, xe.expect(_log(), R, not_free, rect), where + ": clearance")
        _same(got_site, xs.cut(site, rect), where + ": sites")
        whole = np.full((H, W), xs.NONE, dtype=np.uint32)
        whole[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = got_site
        _same(xs.cut(xs.clearance_of(whole), rect), got_clear, where + ": d2 from the sites against the clearance field")
    poses = _centres()
    gx, gy = xe.cells_of(poses, 0.0, 0.0, RES)
    assert np.array_equal(gy * W + gx, np.arange(W * H)), "a pose per cell, in the field's order"
    got_c = m.clearance_poses(poses, R, not_free)
    got_n = m.nearest_poses(poses, R, not_free)
    _same(got_c, xe.expect_poses(clear, poses, 0.0, 0.0, RES), f"R = {R}: clearance_poses against the field")
    want_s, want_d = xs.expect_poses(site, poses, 0.0, 0.0, RES)
    _same(got_n["site"], want_s, f"R = {R}: nearest_poses' sites against the field")
    _same(got_n["d2"], want_d, f"R = {R}: nearest_poses' d2 against the field")
    _same(got_n["d2"].astype(np.uint16), got_c, f"R = {R}: the two poses forms")
    m.close()


def test_inflated_reach_runs_the_same_transform():
    """inflate > 0 blocks the cells within 3 of an obstacle through gms_clear_launch"""
    seeds = np.array([[20, 10]], dtype=np.int32)
    want = rx.expect(_log(), seeds, inflate=3, not_free=False)
    assert (want == rx.FAR).any() and ((want != rx.FAR) & (want > 0)).any() and not rx.blocked(_log(), 3, False)[10, 20]
    m = _map()
    _same(m.reach(seeds, inflate=3, not_free=False), want, "reach, inflate = 3")
    m.close()
