"""Map warps (include/gridmapslam.h "map warps") without a device: the structs' layout in header, ctypes and dtype, the exported
symbols, gms_warp_pose and every argument gms_warp_check refuses, the Python helpers, and the expectation module
(tests/_warp_expect.py) against answers derived by hand on a map of 9 x 7 cells."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _warp_expect as wx
from gridmap_slam_robot_amd import BEAM_DTYPE, WARP_STATS_DTYPE, _lib, map_as_scan, warp_agreement
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsWarp, GmsWarpStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_warp_pose", "gms_warp_check", "gms_map_warp", "gms_map_warp_dev", "gms_slam_warp", "gms_slam_warp_dev"]
REQ = ("tx", "ty", "c", "s", "clamp", "x0", "y0", "w", "h", "op", "pad")
REQ_OFF = [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]
RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643


def test_structs_in_header_ctypes_and_dtype(tmp_path):
    assert C.sizeof(GmsWarp) == 64 and [getattr(GmsWarp, n).offset for n in REQ] == REQ_OFF
    assert C.sizeof(GmsWarpStats) == 80 and GmsWarpStats.pair.offset == 0 and GmsWarpStats.n_outside.offset == 72
    assert WARP_STATS_DTYPE is _lib.WARP_STATS_DTYPE and WARP_STATS_DTYPE.itemsize == 80 and WARP_STATS_DTYPE.names == ("pair", "n_outside")
    assert WARP_STATS_DTYPE.fields["pair"][1] == 0 and WARP_STATS_DTYPE.fields["n_outside"][1] == 72
    assert WARP_STATS_DTYPE.fields["pair"][0] == np.dtype(("<i8", (3, 3))) and WARP_STATS_DTYPE.fields["n_outside"][0] == np.dtype("<i8")
    every = (["sizeof(gms_warp)", "sizeof(gms_warp_stats)"] + [f"offsetof(gms_warp, {n})" for n in REQ]
             + ["offsetof(gms_warp_stats, pair)", "offsetof(gms_warp_stats, pair[1][2])", "offsetof(gms_warp_stats, n_outside)"]
             + ["(size_t)GMS_WARP_COMPARE", "(size_t)GMS_WARP_REPLACE", "(size_t)GMS_WARP_ADD", "(size_t)GMS_WARP_FILL"])
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\n'
                   f'int main(void) {{ printf("{" ".join(["%zu"] * len(every))}", {", ".join(every)}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [64, 80] + REQ_OFF + [0, 40, 72] + [0, 1, 2, 3]
    assert (_lib.GMS_WARP_COMPARE, _lib.GMS_WARP_REPLACE, _lib.GMS_WARP_ADD, _lib.GMS_WARP_FILL) == (0, 1, 2, 3)
    assert (wx.COMPARE, wx.REPLACE, wx.ADD, wx.FILL) == (0, 1, 2, 3)
    rec = np.zeros((), WARP_STATS_DTYPE)
    rec["pair"][1, 2] = 7                              # the dtype's pair[a][b] is the struct's
    assert np.frombuffer(rec.tobytes(), "<i8")[5] == 7


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    assert header.index("---- trajectory rollouts") < header.index("---- map warps") < header.index("---- device-resident inputs")
    for name in ("gms_map_warp(", "gms_slam_warp("):
        assert name in mirror, name
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])


def _req(**kw):
    return GmsWarp(**{**dict(tx=0.25, ty=-1.5, c=1.0, s=0.0, clamp=0.0, x0=0, y0=0, w=4, h=3, op=1, pad=0), **kw})


def test_pose_fills_the_four_doubles_with_libm():
    L = _lib.load()
    w = _req(clamp=2.5, x0=3, op=2)
    assert L.gms_warp_pose(C.byref(w), 1.25, -0.5, 0.3) == GMS_OK
    assert (w.tx, w.ty, w.c, w.s) == (1.25, -0.5, math.cos(0.3), math.sin(0.3))
    assert (w.clamp, w.x0, w.y0, w.w, w.h, w.op) == (2.5, 3, 0, 4, 3, 2), "the other fields stay"
    assert L.gms_warp_pose(C.byref(w), 0.0, 0.0, 0.0) == GMS_OK and (w.c, w.s) == (1.0, 0.0)
    assert L.gms_warp_pose(None, 0.0, 0.0, 0.0) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf), (0.0, 0.0, math.nan)):
        before = (w.tx, w.ty, w.c, w.s)
        assert L.gms_warp_pose(C.byref(w), *bad) == GMS_ERR_INVALID and b"finite" in L.gms_last_error()
        assert (w.tx, w.ty, w.c, w.s) == before


def test_check_refuses_every_bad_field():
    L = _lib.load()
    assert L.gms_warp_check(C.byref(_req())) == GMS_OK
    for op in (0, 1, 2, 3):
        assert L.gms_warp_check(C.byref(_req(op=op, clamp=0.0))) == GMS_OK, "clamp == 0: no clamp"
    assert L.gms_warp_check(C.byref(_req(clamp=1e-300))) == GMS_OK and L.gms_warp_check(C.byref(_req(clamp=1e300))) == GMS_OK
    assert L.gms_warp_check(C.byref(_req(c=0.0, s=1.0))) == GMS_OK and L.gms_warp_check(C.byref(_req(c=0.0, s=-1.0))) == GMS_OK
    assert L.gms_warp_check(C.byref(_req(c=math.cos(0.3), s=math.sin(0.3)))) == GMS_OK
    inside_hi, inside_lo = math.sqrt(1.0 + 9.9e-7), math.sqrt(1.0 - 9.9e-7)         # c*c + s*s just inside the bound, on both sides
    for c, s in ((inside_hi, 0.0), (0.0, inside_lo), (inside_lo * math.cos(1.0), inside_lo * math.sin(1.0))):
        assert abs(c * c + s * s - 1.0) < 1e-6 and L.gms_warp_check(C.byref(_req(c=c, s=s))) == GMS_OK, (c, s)
    assert L.gms_warp_check(C.byref(_req(x0=1 << 30, y0=1 << 30, w=1 << 30, h=1))) == GMS_OK, "the rectangle is held against a map by the entry points"

    def refused(req, word):
        assert L.gms_warp_check(None if req is None else C.byref(req)) == GMS_ERR_INVALID, word
        assert word in L.gms_last_error(), (word, L.gms_last_error())
    refused(None, b"null")
    for op in (-1, 4, 7, 1 << 30):
        refused(_req(op=op), b"op")
    for name in ("tx", "ty"):
        for v in (math.nan, math.inf, -math.inf):
            refused(_req(**{name: v}), b"tx and ty")
    for name in ("c", "s"):
        for v in (math.nan, math.inf, -math.inf):
            refused(_req(**{name: v}), b"c and s")
    for v in (math.nan, math.inf, -math.inf, -1e-300, -1.0):
        refused(_req(clamp=v), b"clamp")
    outside_hi, outside_lo = math.sqrt(1.0 + 1.1e-6), math.sqrt(1.0 - 1.1e-6)
    for c, s in ((outside_hi, 0.0), (outside_lo, 0.0), (0.0, 0.0), (1.0, 1.0), (1e200, 0.0)):
        refused(_req(c=c, s=s), b"cosine")
    for kw in (dict(x0=-1), dict(y0=-1), dict(w=0), dict(h=0), dict(w=-3), dict(h=-(1 << 31))):
        refused(_req(**kw), b"rectangle")


def test_entry_points_refuse_null_pointers_and_bad_requests():
    """checked before anything is touched: the fake handles are blocks of zero bytes (n_maps 0), so behind the request every map index
    is bad as well; each refusal is told apart by its message"""
    L = _lib.load()
    zeros = np.zeros((2, 16384), np.uint8)             # (kept alive: the handles are this memory)
    fake, other = zeros[0].ctypes.data, zeros[1].ctypes.data
    stats = np.full(80, 7, np.uint8)
    shown = C.c_int32(-7)
    st, g = stats.ctypes.data, C.byref(_req())

    def refused(fn, args, word):
        assert fn(*args) == GMS_ERR_INVALID, args
        assert word in L.gms_last_error(), (word, L.gms_last_error())
    for fn in (L.gms_map_warp, L.gms_map_warp_dev):
        refused(fn, (None, 0, other, 0, g, st), b"null")
        refused(fn, (fake, 0, None, 0, g, st), b"null")
        refused(fn, (fake, 0, other, 0, None, st), b"null")
        refused(fn, (fake, 0, other, 0, C.byref(_req(op=9)), st), b"op")
        refused(fn, (fake, 0, other, 0, C.byref(_req(clamp=-1.0)), st), b"clamp")
        refused(fn, (fake, 0, other, 0, C.byref(_req(c=0.5)), st), b"cosine")
        refused(fn, (fake, 0, other, 0, C.byref(_req(w=0)), st), b"rectangle")
        refused(fn, (fake, 0, other, 0, g, st), b"map index")
        refused(fn, (fake, -1, other, 0, g, None), b"map index")
    for fn in (L.gms_slam_warp, L.gms_slam_warp_dev):
        refused(fn, (None, 0, 0, fake, 0, g, st, C.byref(shown)), b"null")
        refused(fn, (None, -1, 0, None, 0, g, None, None), b"null")
    assert (stats == 7).all() and shown.value == -7, "a refused request writes nothing"


def test_agreement_of_a_hand_filled_record():
    rec = np.zeros((), WARP_STATS_DTYPE)
    rec["pair"] = [[1, 2, 3], [4, 50, 6], [7, 8, 90]]
    rec["n_outside"] = 11
    assert warp_agreement(rec) == dict(overlap=50 + 6 + 8 + 90, agree=140, conflict=14, gained=5, outside=11)
    assert warp_agreement(np.zeros((), WARP_STATS_DTYPE)) == dict(overlap=0, agree=0, conflict=0, gained=0, outside=0)
    assert warp_agreement(rec.reshape(1)) == warp_agreement(rec)


def test_map_as_scan_lists_the_occupied_cells_and_strides():
    log = np.full((7, 9), L_FREE)
    log[0, 0] = log[2, 5] = log[6, 8] = L_OCC
    log[3, 3], log[3, 4], log[3, 5] = 0.0, -0.0, np.nan
    b = map_as_scan(log, (-0.25, 0.5), RES)
    r, px, py = (float(np.float32(v)) for v in (RES, -0.25, 0.5))
    assert b.dtype == BEAM_DTYPE and len(b) == 3 and (b["hit"] == 1).all()
    assert b["local_x"].tolist() == [px + 0.5 * r, px + 5.5 * r, px + 8.5 * r] and b["local_y"].tolist() == [py + 0.5 * r, py + 2.5 * r, py + 6.5 * r]
    assert b["distance"].tolist() == [math.hypot(x, y) for x, y in zip(b["local_x"], b["local_y"])]
    assert len(map_as_scan(np.full((7, 9), L_FREE), (0, 0), RES)) == 0
    log[:] = L_OCC                                     # 63 cells
    every = map_as_scan(log, (0.0, 0.0), RES, max_beams=63)
    assert len(every) == 63 and every["local_x"][:10].tolist() == [(i % 9 + 0.5) * r for i in range(10)]
    for cap, stride in ((62, 2), (32, 2), (31, 3), (21, 3), (20, 4), (1, 63)):
        part = map_as_scan(log, (0.0, 0.0), RES, max_beams=cap)
        assert len(part) == -(-63 // stride) <= cap and np.array_equal(part, every[::stride]), (cap, stride)
    with pytest.raises(ValueError):
        map_as_scan(log.reshape(-1), (0, 0), RES)


# ---- the expectation against answers derived by hand -----------------------------------------------------------------------------
def _src97():
    rng = np.random.default_rng(5)
    src = rng.choice([L_OCC, L_FREE, 2 * L_OCC, 0.0], size=(7, 9))
    src[1, 2], src[4, 7], src[6, 0] = np.nan, -0.0, 3 * L_FREE
    return src


def _pairs(d, v, inside_count, total):
    st = np.zeros((), WARP_STATS_DTYPE)
    st["pair"] = np.bincount(wx.classes(d).ravel() * 3 + wx.classes(v).ravel(), minlength=9).reshape(3, 3)
    st["n_outside"] = total - inside_count
    return st


def test_expectation_identity_is_the_array_itself():
    src = _src97()
    g = wx.Geometry.make(9, 7, RES, -0.2, 0.35)
    dst = np.full((7, 9), 5.0)
    out, st = wx.expect(dst, g, src, g, (0.0, 0.0, 1.0, 0.0), "replace")
    assert np.array_equal(wx.bits(out), wx.bits(src)), "bit for bit: NaN and -0.0 included"
    assert st == _pairs(dst, src, 63, 63) and st["pair"][2].sum() == 63 and st["n_outside"] == 0
    same, st2 = wx.expect(dst, g, src, g, (0.0, 0.0, 1.0, 0.0), "compare")
    assert np.array_equal(wx.bits(same), wx.bits(dst)) and st2 == st


def test_expectation_whole_cell_shift_is_a_slice():
    src = _src97()
    g = wx.Geometry.make(9, 7, RES, -0.2, 0.35)
    dst = np.full((7, 9), -7.0)
    out, st = wx.expect(dst, g, src, g, (2 * g.res, -1 * g.res, 1.0, 0.0), "replace")       # the source's frame two cells east, one south
    want = dst.copy()
    want[0:6, 2:9] = src[1:7, 0:7]                     # destination cell (x, y) sees source cell (x - 2, y + 1)
    assert np.array_equal(wx.bits(out), wx.bits(want))
    assert st == _pairs(dst[0:6, 2:9], src[1:7, 0:7], 42, 63) and st["n_outside"] == 21


def test_expectation_quarter_turn_is_rot90_placed_by_hand():
    src = _src97()
    gs = wx.Geometry.make(9, 7, RES, 0.0, 0.0)
    gd = wx.Geometry.make(11, 12, RES, 0.0, 0.0)
    ox, oy = 3, 2
    # c = 0, s = 1: p_dst = (-y_src, x_src) + t.  With t = ((7 + ox) r, oy r) source cell (qx, qy) lands in destination cell
    # (7 - 1 - qy + ox, qx + oy): the 9 x 7 source becomes 7 columns by 9 rows, the array turned clockwise in index space
    dst = np.full((12, 11), 0.25)
    out, st = wx.expect(dst, gd, src, gs, ((7 + ox) * gd.res, oy * gd.res, 0.0, 1.0), "replace")
    want = dst.copy()
    want[oy:oy + 9, ox:ox + 7] = np.rot90(src, -1)
    assert want[oy + 4, ox + 7 - 1 - 1] == src[1, 4], "source cell (4, 1)"
    assert np.array_equal(wx.bits(out), wx.bits(want))
    assert st["n_outside"] == 12 * 11 - 63 and st["pair"].sum() == 63
    # and back: the destination's frame in the source's is the inverse pose, t' = -R^T t = (-oy r, (7 + ox) r), c = 0, s = -1
    again, st3 = wx.expect(np.zeros((7, 9)), gs, out, gd, (-oy * gd.res, (7 + ox) * gd.res, 0.0, -1.0), "replace")
    assert np.array_equal(wx.bits(again), wx.bits(src)) and st3["n_outside"] == 0


def test_expectation_half_the_resolution_shows_every_cell_as_a_block():
    src = _src97()
    gs = wx.Geometry.make(9, 7, RES, -0.2, 0.35)
    gd = wx.Geometry.make(18, 14, RES / 2, -0.2, 0.35)
    assert gd.res * 2 == gs.res
    out, st = wx.expect(np.zeros((14, 18)), gd, src, gs, (0.0, 0.0, 1.0, 0.0), "replace")
    assert np.array_equal(wx.bits(out), wx.bits(np.repeat(np.repeat(src, 2, axis=0), 2, axis=1)))
    assert st["n_outside"] == 0 and st["pair"][0].sum() == 4 * 63
    coarse, st2 = wx.expect(np.zeros((7, 9)), gs, out, gd, (0.0, 0.0, 1.0, 0.0), "replace")      # the other way: the centre's cell, one of the four
    assert np.array_equal(wx.bits(coarse), wx.bits(src)) and st2["n_outside"] == 0


def test_expectation_add_and_fill_by_hand():
    g = wx.Geometry.make(3, 3, RES, 0.0, 0.0)
    ident = (0.0, 0.0, 1.0, 0.0)
    d = np.array([[0.0, -0.0, np.nan], [-1.0, -1.0, -1.0], [2.0, 2.0, 2.0]])
    v = np.array([[0.0, -1.5, 2.5], [np.nan, -1.5, 2.5], [-0.0, -1.5, 2.5]])
    fill, st = wx.expect(d, g, v, g, ident, "fill")
    want = d.copy()
    want[0, 1], want[0, 2] = -1.5, 2.5                 # unknown destination, known source: the only stores
    assert np.array_equal(wx.bits(fill), wx.bits(want)) and (st["pair"] == 1).all() and st["n_outside"] == 0, "each of the nine class pairs once"
    add, _ = wx.expect(d, g, v, g, ident, "add")
    want = np.array([[0.0, -1.5, np.nan], [-1.0, -2.5, 1.5], [2.0, 0.5, 4.5]])
    want[0, 1] = -0.0 + -1.5
    assert np.array_equal(wx.bits(add), wx.bits(want)), "an unknown source cell changes nothing, a NaN destination stays"
    assert np.array_equal(wx.bits(add)[0, :1], wx.bits(d)[0, :1]) and wx.bits(add)[0, 2] == wx.bits(d)[0, 2]
    clamped, _ = wx.expect(d, g, v, g, ident, "add", clamp=2.0)
    want = np.array([[0.0, -1.5, np.nan], [-1.0, -2.0, 1.5], [2.0, 0.5, 2.0]])
    assert np.array_equal(wx.bits(clamped), wx.bits(want))
    one, st1 = wx.expect(d, g, v, g, ident, "replace", rect=(1, 2, 2, 1))
    want = d.copy()
    want[2, 1:3] = v[2, 1:3]
    assert np.array_equal(wx.bits(one), wx.bits(want)) and st1["pair"].sum() == 2 and st1["pair"][2, 1] == 1 and st1["pair"][2, 2] == 1
