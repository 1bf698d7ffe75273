"""Frontier regions (include/gridmapslam.h "frontier regions") without a device: the request's and the record's layout in header and
mirror, the exported symbols, gms_frontiers_size and every refused argument, the expectation module against hand-derived answers, and
the numpy helper frontier_centroids."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _frontier_expect as fx
from gridmap_slam_robot_amd import _lib, frontier_centroids
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsFrontier, GmsFrontiers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_frontiers_size", "gms_map_frontiers", "gms_map_frontiers_dev", "gms_slam_frontiers", "gms_slam_frontiers_dev"]
REQ = ("x0", "y0", "w", "h", "min_size", "inflate", "filter", "pad")
REC = ("anchor_x", "anchor_y", "count", "goal_cost", "min_x", "min_y", "max_x", "max_y", "goal_x", "goal_y", "sum_x", "sum_y")
REC_OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48]
FAR = 0xFFFF


def test_structs_and_constants_in_header_and_mirror(tmp_path):
    assert C.sizeof(GmsFrontiers) == 32 and [getattr(GmsFrontiers, n).offset for n in REQ] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert C.sizeof(GmsFrontier) == 56 and [getattr(GmsFrontier, n).offset for n in REC] == REC_OFFSETS
    assert _lib.FRONTIER_DTYPE.itemsize == 56 and [_lib.FRONTIER_DTYPE.fields[n][1] for n in REC] == REC_OFFSETS
    assert _lib.FRONTIER_DTYPE == fx.DTYPE
    src = tmp_path / "size.c"
    fmt = " ".join(["%zu"] * (2 + len(REQ) + len(REC)))
    args = ", ".join(["sizeof(gms_frontiers)", "sizeof(gms_frontier)"] + [f"offsetof(gms_frontiers, {n})" for n in REQ] + [f"offsetof(gms_frontier, {n})" for n in REC])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\n'
                   f'int main(void) {{ printf("{fmt} %u", {args}, GMS_FRONTIER_NONE); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [32, 56, 0, 4, 8, 12, 16, 20, 24, 28] + REC_OFFSETS + [0xFFFFFFFF]
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert _lib.GMS_FRONTIER_NONE == 0xFFFFFFFF == fx.NONE


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    for name in ("gms_map_frontiers(", "gms_slam_frontiers(", "gms_frontiers_size("):
        assert name in mirror, name
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])


def _size(*fields):
    f = GmsFrontiers(*fields)
    w, h, n = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc = _lib.load().gms_frontiers_size(C.byref(f), C.byref(w), C.byref(h), C.byref(n))
    return rc, w.value, h.value, n.value


def test_frontiers_size_and_every_refused_argument():
    assert _size(0, 0, 200, 136, 1, 0, 0, 0) == (GMS_OK, 200, 136, 200 * 136 * 4)
    assert _size(3, 5, 1, 1, 1000000, 255, 2, 99) == (GMS_OK, 1, 1, 4)
    assert _size(100, 7, 2048, 2048, 3, 25, 0, 0) == (GMS_OK, 2048, 2048, 2048 * 2048 * 4)
    L = _lib.load()
    f = GmsFrontiers(0, 0, 4, 3, 1, 0, 0, 0)
    assert L.gms_frontiers_size(C.byref(f), None, None, None) == GMS_OK, "every output may be NULL"
    assert L.gms_frontiers_size(None, None, None, None) == GMS_ERR_INVALID
    for bad in ((0, 0, 0, 3, 1, 0, 0, 0), (0, 0, 4, 0, 1, 0, 0, 0), (0, 0, -1, 3, 1, 0, 0, 0), (0, 0, 4, -1, 1, 0, 0, 0),      # w, h < 1
                (-1, 0, 4, 3, 1, 0, 0, 0), (0, -1, 4, 3, 1, 0, 0, 0),                                                    # x0, y0 < 0
                (0, 0, 4, 3, 0, 0, 0, 0), (0, 0, 4, 3, -5, 0, 0, 0),                                                     # min_size < 1
                (0, 0, 4, 3, 1, -1, 0, 0), (0, 0, 4, 3, 1, 256, 0, 0)):                                                  # inflate
        assert _size(*bad) == (GMS_ERR_INVALID, -7, -7, -7), bad


def test_entry_points_refuse_null_handles_and_bad_requests():
    """checked before anything is touched: the fake handles are blocks of zero bytes (n_maps 0, W = H = 0), so every index and every
    rectangle -- one off the map -- is bad"""
    L = _lib.load()
    fake = np.zeros(16384, np.uint8).ctypes.data
    lab = np.full((3, 4), 7, np.uint32)
    rec = np.zeros(4, _lib.FRONTIER_DTYPE)
    rec["count"] = 7
    n = C.c_int32(-7)
    f = C.byref(GmsFrontiers(0, 0, 4, 3, 1, 0, 0, 0))
    lp, rp = lab.ctypes.data, rec.ctypes.data
    for fn in (L.gms_map_frontiers, L.gms_map_frontiers_dev):
        for args in ((None, 0, f, None, lp, rp, 4, C.byref(n)), (fake, 0, None, None, lp, rp, 4, C.byref(n))):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        assert fn(fake, 0, f, None, lp, rp, 4, C.byref(n)) == GMS_ERR_INVALID and fn(fake, -1, f, None, lp, rp, 4, C.byref(n)) == GMS_ERR_INVALID
    for fn in (L.gms_slam_frontiers, L.gms_slam_frontiers_dev):
        for args in ((None, 0, f, None, lp, rp, 4, C.byref(n), None), (fake, 0, None, None, lp, rp, 4, C.byref(n), None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    assert n.value == -7 and (lab == 7).all() and (rec["count"] == 7).all(), "a refused request writes nothing"


def _ring_log(H, W, x0, y0, a, b):
    log = np.zeros((H, W))
    log[y0:y0 + b, x0:x0 + a] = -0.4
    return log


def test_expectation_ring_of_a_free_rectangle():
    a, b = 9, 6
    rec, n, lab = fx.expect(_ring_log(30, 40, 5, 7, a, b))
    assert n == 1 and rec["count"][0] == 2 * (a + b) - 4
    r = rec[0]
    assert (r["anchor_x"], r["anchor_y"], r["min_x"], r["min_y"], r["max_x"], r["max_y"]) == (5, 7, 5, 7, 13, 12)
    assert (r["goal_x"], r["goal_y"], r["goal_cost"]) == (-1, -1, FAR), "no cost field: no goal"
    ring = np.zeros((30, 40), bool)
    ring[7:13, 5:14] = True
    ring[8:12, 6:13] = False
    assert np.array_equal(lab != fx.NONE, ring) and (lab[ring] == 7 * 40 + 5).all()
    xs, ys = np.nonzero(ring)[1], np.nonzero(ring)[0]
    assert (r["sum_x"], r["sum_y"]) == (xs.sum(), ys.sum())
    assert frontier_centroids(rec).tolist() == [[9.0, 9.5]], "the ring's centre"


def test_expectation_rectangle_flush_with_the_edge_loses_the_edge_run():
    a, b = 9, 6
    rec, n, lab = fx.expect(_ring_log(30, 40, 0, 7, a, b))                     # flush with x = 0: the map's border makes no frontier
    assert n == 1 and rec["count"][0] == 2 * (a + b) - 4 - (b - 2), "the left column's inner run has no unknown neighbour"
    assert lab[9, 0] == fx.NONE and lab[7, 0] != fx.NONE and lab[12, 0] != fx.NONE, "its two corners keep their unknown neighbour above / below"
    rec, n, lab = fx.expect(_ring_log(30, 40, 0, 0, a, b))                     # in the corner: the right column and the top row
    assert n == 1 and rec["count"][0] == a + b - 1 and (rec["anchor_x"][0], rec["anchor_y"][0]) == (8, 0)
    rec, n, _ = fx.expect(np.full((30, 40), -0.4))
    assert n == 0 and len(rec) == 0, "an all-free map has no frontier"
    assert fx.expect(np.zeros((30, 40)))[1] == 0, "... and neither has a fresh one"


def test_expectation_diagonal_unknown_and_occupied_neighbours():
    log = np.full((12, 12), -0.4)
    log[5, 5] = 0.0
    rec, n, lab = fx.expect(log)
    assert n == 1 and rec["count"][0] == 4, "the four axis neighbours; the four diagonal ones see the unknown cell at a corner only"
    assert sorted(map(tuple, np.argwhere(lab != fx.NONE).tolist())) == [(4, 5), (5, 4), (5, 6), (6, 5)]
    assert (lab[lab != fx.NONE] == 4 * 12 + 5).all(), "they touch diagonally: one region, anchored at (5, 4)"
    log[5, 5] = 0.85
    assert fx.expect(log)[1] == 0, "an occupied cell next to a free cell makes no frontier"
    for v in (np.nan, -0.0):
        log[5, 5] = v
        assert fx.expect(log)[0]["count"].tolist() == [4]
    log[5, 5] = 0.0
    log[8, 5] = 0.85
    assert fx.expect(log, inflate=1)[0]["count"].tolist() == [4] and fx.expect(log, inflate=2)[0]["count"].tolist() == [3]
    assert fx.expect(log, inflate=3)[0]["count"].tolist() == [3] and fx.expect(log, inflate=4)[1] == 0, "d2 = 4, 10, 10 and 16"
    two = np.full((12, 12), -0.4)
    two[2, 2] = two[2, 6] = 0.0                                                # (2, 3) and (2, 5): one cell apart
    assert fx.expect(two)[1] == 2
    assert fx.expect(two, min_size=4)[1] == 2 and fx.expect(two, min_size=5)[1] == 0


def test_expectation_goal_and_ties():
    log = _ring_log(20, 20, 4, 4, 5, 5)
    cost = np.full((20, 20), FAR, np.uint16)
    rec = fx.expect(log, cost=cost)[0]
    assert (rec["goal_x"][0], rec["goal_y"][0], rec["goal_cost"][0]) == (-1, -1, FAR), "every member FAR"
    cost[8, 6] = cost[4, 8] = cost[6, 4] = 35
    cost[6, 6] = 0                                                             # (not a member)
    rec = fx.expect(log, cost=cost)[0]
    assert (rec["goal_x"][0], rec["goal_y"][0], rec["goal_cost"][0]) == (8, 4, 35), "a tie goes to the smallest linear index"
    cost[8, 8] = 34
    rec = fx.expect(log, cost=cost)[0]
    assert (rec["goal_x"][0], rec["goal_y"][0], rec["goal_cost"][0]) == (8, 8, 34)


def test_frontier_centroids():
    rec = np.zeros(3, _lib.FRONTIER_DTYPE)
    rec["count"] = [1, 4, 3]
    rec["sum_x"] = [7, 10, 2 ** 40]
    rec["sum_y"] = [0, 3, 1]
    got = frontier_centroids(rec)
    assert got.dtype == np.float64 and got.shape == (3, 2)
    assert got.tolist() == [[7.0, 0.0], [2.5, 0.75], [2 ** 40 / 3, 1 / 3]]
    assert frontier_centroids(rec[:0]).shape == (0, 2)
