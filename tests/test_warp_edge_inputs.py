"""What the inputs of tests/test_gpu_warp_edges.py must contain for its comparisons to reach the warp's edges: the restatement
(tests/_warp_expect.py, unchanged) against the answers derived by hand on the dyadic cases of tests/_warp_edge_cases.py, the conditions
on the other cases, and which slip in the kernel's arithmetic each case can tell from the definition -- all without a device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import _warp_edge_cases as ec
import _warp_expect as wx
from gridmap_slam_robot_amd import _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsWarp

CASES = {c.name: c for c in ec.cases()}
BY_HAND = [c.name for c in ec.cases() if c.hand is not None]
# every quotient of these is a whole number: each destination centre lies on a source cell's edge in both directions
ON_EDGES = ["2:1 fine into coarse", "half a cell up and right", "half a cell down and left", "half turn and half a cell"]
ON_EDGES += [n + ", ragged" for n in ON_EDGES[1:]]
INEXACT = [ec.THREE_FOUR_FIVE, "1 cm into 8 cm, 0.3 rad", "20 cm into 2.5 cm, -1.1 rad", "near-unit (c, s)"]
FAR = [n for n in CASES if n.startswith("far away")]


def _fused(a, b, c):
    """a * b + c with one rounding, elementwise: exact in rationals, then the nearest double"""
    flat = [float(Fraction(float(a)) * Fraction(float(x)) + Fraction(float(y))) for x, y in zip(np.ravel(b), np.ravel(c))]
    return np.array(flat).reshape(np.shape(b))


def _quotients(case, fused=False):
    """the header's arithmetic up to the quotients, over the whole destination: ((u - px_s) / r_s, (v - py_s) / r_s) [H][W];
    fused: u as fma(c, dx, s * dy)"""
    gd, gs = ec.geometry(case.dst), ec.geometry(case.src)
    tx, ty, c, s = (np.float64(v) for v in case.pose)
    x = np.arange(gd.W, dtype=np.float64)[None, :]
    y = np.arange(gd.H, dtype=np.float64)[:, None]
    dx = np.broadcast_to(np.float64(gd.px) + (x + 0.5) * np.float64(gd.res) - tx, (gd.H, gd.W))
    dy = np.broadcast_to(np.float64(gd.py) + (y + 0.5) * np.float64(gd.res) - ty, (gd.H, gd.W))
    with np.errstate(invalid="ignore", over="ignore"):
        u = _fused(c, dx, s * dy) if fused else c * dx + s * dy
        v = c * dy - s * dx
        return (u - np.float64(gs.px)) / np.float64(gs.res), (v - np.float64(gs.py)) / np.float64(gs.res)


def _cells(case, rounding=np.floor, fused=False, closed=False):
    """(inside, qx, qy) as wx.source_cells gives them for the whole destination, with the rounding and the sum to choose; closed:
    `q <= W` in place of `q < W`"""
    gs = ec.geometry(case.src)
    a, b = _quotients(case, fused)
    with np.errstate(invalid="ignore"):
        qx, qy = rounding(a), rounding(b)
        inside = (qx >= 0) & (qx < gs.W + closed) & (qy >= 0) & (qy < gs.H + closed)
    return inside, np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)


def _differ(a, b):
    return int(((a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2])).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_is_well_formed(name):
    case = CASES[name]
    gd, gs = ec.geometry(case.dst), ec.geometry(case.src)
    for grid, g in ((case.dst, gd), (case.src, gs)):
        assert abs(g.res - grid[2]) < 1e-8 and ec.size_of(grid)[0] > 0
    W, H = case.dst[:2]
    x0, y0, w, h = case.rect or (0, 0, W, H)
    assert 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H
    tx, ty, c, s = case.pose
    assert np.isfinite([tx, ty, c, s]).all() and abs(c * c + s * s - 1.0) <= 1e-6
    start, src = ec.start_log(case.dst), ec.source_log(case.src, case.seed)
    for a in (start, src):                               # every class, and every kind of unknown by its bits
        assert {0, 1, 2} == set(wx.classes(a).ravel().tolist())
        assert np.isnan(a).any() and (wx.bits(a) == wx.bits(np.array(-0.0))).any() and (wx.bits(a) == 0).any()
    assert np.array_equal(wx.source_cells(gd, gs, *case.pose)[0], _cells(case)[0]), "this module's arithmetic is the restatement's"
    assert _differ(wx.source_cells(gd, gs, *case.pose), _cells(case)) == 0
    outside = np.ones((H, W), bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    for op in ec.OPS:
        out, st = ec.expect(case, op)
        assert st["pair"].sum() + st["n_outside"] == w * h
        assert np.array_equal(wx.bits(out)[outside], wx.bits(start)[outside])
        if op == "compare":
            assert np.array_equal(wx.bits(out), wx.bits(start))


@pytest.mark.parametrize("name", BY_HAND)
def test_restatement_gives_the_hand_answer(name):
    case = CASES[name]
    want, n_outside = ec.by_hand(case)
    out, st = ec.expect(case, "replace")
    assert np.array_equal(wx.bits(out), wx.bits(want)), "REPLACE is the slice"
    assert st["n_outside"] == n_outside
    if case.rect is None:
        assert n_outside == case.n_outside, "the count derived from the geometry"
    else:
        assert case.hand[1].size - int(case.hand[1].sum()) == case.n_outside
    for op in ("compare", "add", "fill"):
        assert ec.expect(case, op)[1] == st, "every op counts what REPLACE counts"


def test_hand_answers_are_the_slices_of_the_issue():
    """the four answers spelled out once more, from the arrays alone"""
    fine, coarse, src = ec.source_log(ec.FINE, 9670), ec.source_log(ec.COARSE, 4835), ec.source_log(ec.GRID, 7066)
    start = ec.start_log(ec.GRID)
    assert np.array_equal(wx.bits(ec.expect(CASES["2:1 fine into coarse"], "replace")[0]), wx.bits(fine[1::2, 1::2]))
    assert np.array_equal(wx.bits(ec.expect(CASES["1:2 coarse into fine"], "replace")[0]), wx.bits(np.repeat(np.repeat(coarse, 2, 0), 2, 1)))
    assert np.array_equal(wx.bits(ec.expect(CASES["half a cell up and right"], "replace")[0]), wx.bits(src))
    want = start.copy()
    want[:-1, :-1] = src[1:, 1:]
    assert np.array_equal(wx.bits(ec.expect(CASES["half a cell down and left"], "replace")[0]), wx.bits(want))
    assert np.array_equal(wx.bits(ec.expect(CASES["half turn about the middle"], "replace")[0]), wx.bits(src[::-1, ::-1]))
    want = start.copy()
    want[1:, 1:] = src[::-1, ::-1][:-1, :-1]
    out, st = ec.expect(CASES["half turn and half a cell"], "replace")
    assert np.array_equal(wx.bits(out), wx.bits(want)) and st["n_outside"] == 70 + 66 - 1 == 135


@pytest.mark.parametrize("name", ON_EDGES)
def test_centres_sit_exactly_on_source_edges(name):
    case = CASES[name]
    gs = ec.geometry(case.src)
    a, b = _quotients(case)
    assert np.array_equal(a, np.floor(a)) and np.array_equal(b, np.floor(b)), "whole numbers: no slack on either side of the tie"
    if case.n_outside:                                   # ... and the bounds are met with equality, one cell beyond them
        assert {-1.0, float(gs.W)} & set(a.ravel().tolist()) and {-1.0, float(gs.H)} & set(b.ravel().tolist())
        assert a.min() >= -1 and a.max() <= gs.W
    # exact: the same quotient in rationals, at the four corners and along a diagonal
    gd = ec.geometry(case.dst)
    tx, ty, c, s = (Fraction(v) for v in case.pose)
    for x, y in [(0, 0), (gd.W - 1, 0), (0, gd.H - 1), (gd.W - 1, gd.H - 1)] + [(i, i) for i in range(1, min(gd.W, gd.H), 7)]:
        dx = Fraction(gd.px) + (x + Fraction(1, 2)) * Fraction(gd.res) - tx
        dy = Fraction(gd.py) + (y + Fraction(1, 2)) * Fraction(gd.res) - ty
        assert Fraction(float(a[y, x])) == (c * dx + s * dy - Fraction(gs.px)) / Fraction(gs.res)
        assert Fraction(float(b[y, x])) == (c * dy - s * dx - Fraction(gs.py)) / Fraction(gs.res)


@pytest.mark.parametrize("name", INEXACT)
def test_other_cases_have_every_class_pair_and_cells_outside(name):
    case = CASES[name]
    st = ec.expect(case, "compare")[1]
    assert st["n_outside"] > 0 and (st["pair"] > 0).all(), "every class pair occurs"
    assert case.hand is None


def test_resolution_ratios_skip_and_repeat_source_cells():
    inside, qx, qy = _cells(CASES["1 cm into 8 cm, 0.3 rad"])
    seen = len(set(zip(qx[inside].tolist(), qy[inside].tolist())))
    assert seen == int(inside.sum()) and seen * 40 < 400 * 300, "no source cell twice, most never"
    rows = [len(set(qy[y][inside[y]].tolist())) for y in range(inside.shape[0])]
    assert rows == inside.sum(axis=1).tolist() and max(rows) >= 50, "a destination row's cells come from a source row each: a line per cell"
    inside, qx, qy = _cells(CASES["20 cm into 2.5 cm, -1.1 rad"])
    _, counts = np.unique(qy[inside] * 12 + qx[inside], return_counts=True)
    assert len(counts) > 80 and np.median(counts) >= 62, "most source cells show, each as a turned block of 8 x 8 centres"


@pytest.mark.parametrize("name", FAR)
def test_far_poses_leave_every_number_format(name):
    case = CASES[name]
    a, b = _quotients(case)
    assert not _cells(case)[0].any()
    with np.errstate(invalid="ignore"):
        assert ((np.abs(a) >= 2.0 ** 63) | np.isnan(a)).all() or ((np.abs(b) >= 2.0 ** 63) | np.isnan(b)).all(), "no integer holds them"
    if case.pose[0] == 1.7e308:
        assert np.isinf(a).any() or np.isinf(b).any(), "the sum of the two products overflows"
    for op in ec.OPS:
        out, st = ec.expect(case, op)
        assert np.array_equal(wx.bits(out), wx.bits(ec.start_log(case.dst))) and st["n_outside"] == case.n_outside == 70 * 66


def test_unit_bound_on_either_side():
    L = _lib.load()

    def req(pose):
        return GmsWarp(tx=pose[0], ty=pose[1], c=pose[2], s=pose[3], clamp=0.0, x0=0, y0=0, w=70, h=66, op=1, pad=0)
    near, refused = ec.near_unit_pose(ec.NEAR_UNIT), ec.near_unit_pose(ec.REFUSED_UNIT)
    assert CASES["near-unit (c, s)"].pose == near
    assert 5e-7 < near[2] ** 2 + near[3] ** 2 - 1.0 < 7e-7 and L.gms_warp_check(C.byref(req(near))) == GMS_OK
    assert refused[2] ** 2 + refused[3] ** 2 - 1.0 > 1e-6 and L.gms_warp_check(C.byref(req(refused))) == GMS_ERR_INVALID
    unit = CASES["near-unit (c, s)"]._replace(pose=ec.near_unit_pose(1.0))
    assert _differ(_cells(unit), _cells(CASES["near-unit (c, s)"])) > 100, "the scale shows: (c, s) is used as it is"
    assert (_cells(unit)[0] != _cells(CASES["near-unit (c, s)"])[0]).any(), "... in the counts as well"
    assert near[0] != round(near[0], 3) and near[1] != round(near[1], 3), "a fractional t"


def test_which_slips_each_case_can_tell_from_the_definition():
    """a truncation in place of floor, a rounding to nearest, and a fused c * dx + s * dy, each against the restatement on the CPU.
    Exact arithmetic hides a fused sum and whole quotients hide the rounding mode: the dyadic cases hold the geometry, the strides
    and the bounds; the 3-4-5 turn and the fractional cases hold the arithmetic."""
    for name, case in CASES.items():
        if case.rect is not None or name in FAR:
            continue
        ref = _cells(case)
        trunc, nearest, fused = (_differ(ref, _cells(case, rounding=np.trunc)), _differ(ref, _cells(case, rounding=np.rint)),
                                 _differ(ref, _cells(case, fused=True)))
        if name in INEXACT:
            assert trunc > 0 and nearest > 0, name
        if name in ON_EDGES:
            assert trunc == nearest == fused == 0, name
        if name == "half turn and half a cell":          # q == W_s and q == H_s exactly, along the first column and row
            assert int((ref[0] != _cells(case, closed=True)[0]).sum()) == 70 + 66 - 1
        if name in ("1:2 coarse into fine", "half turn about the middle"):
            assert nearest > 0 and fused == 0, name      # centres a quarter or a half cell inside: exact, but not whole
        if name == ec.THREE_FOUR_FIVE:
            assert fused > 0, "the separately rounded sum and the fused one pick different cells"
            src = ec.source_log(case.src, case.seed)
            a = wx.bits(src)[ref[2], ref[1]][ref[0]]
            f = _cells(case, fused=True)
            assert (ref[0] != f[0]).any(), "... and disagree on whether there is one: the counts differ as well"
            both = ref[0] & f[0]
            assert (wx.bits(src)[ref[2], ref[1]][both] != wx.bits(src)[f[2], f[1]][both]).any() and a.size
