"""Cost-to-go fields (include/gridmapslam.h "cost-to-go fields") without a device: the request's layout in header and mirror, the
exported symbols, gms_reach_size and every refused argument, the expectation module against the closed form of an empty map, and the
numpy helpers reach_metres, cells_of_poses and descend."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _clearance_expect as xe
import _reach_expect as rx
from gridmap_slam_robot_amd import _lib, cells_of_poses, descend, reach_metres
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsReach

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_reach_size", "gms_map_reach", "gms_map_reach_dev", "gms_slam_reach", "gms_slam_reach_dev", "gms_map_reach_stats"]
FAR = 0xFFFF


def test_request_and_constants_in_header_and_mirror(tmp_path):
    assert C.sizeof(GmsReach) == 32
    assert [getattr(GmsReach, n).offset for n in ("x0", "y0", "w", "h", "max_cost", "inflate", "mode", "filter")] == [0, 4, 8, 12, 16, 20, 24, 28]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d", '
                   'sizeof(gms_reach), offsetof(gms_reach, max_cost), offsetof(gms_reach, inflate), offsetof(gms_reach, mode), offsetof(gms_reach, filter), '
                   'GMS_REACH_AXIS, GMS_REACH_DIAG, GMS_REACH_FAR, GMS_REACH_MAX_SEEDS, GMS_ERR_INTERNAL); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["32", "16", "20", "24", "28", "5", "7", "65535", "4096", "-6"]
    assert (_lib.GMS_REACH_AXIS, _lib.GMS_REACH_DIAG, _lib.GMS_REACH_FAR, _lib.GMS_REACH_MAX_SEEDS) == (5, 7, 0xFFFF, 4096) == (rx.AXIS, rx.DIAG, rx.FAR, 4096)
    assert _lib.GMS_ERR_INTERNAL == -6


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    for name in ("gms_map_reach(", "gms_slam_reach(", "gms_map_reach_stats("):
        assert name in mirror, name
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])


def _size(*fields):
    r = GmsReach(*fields)
    w, h, n = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc = _lib.load().gms_reach_size(C.byref(r), C.byref(w), C.byref(h), C.byref(n))
    return rc, w.value, h.value, n.value


def test_reach_size_and_every_refused_argument():
    assert _size(0, 0, 200, 136, 0xFFFE, 0, 1, 0) == (GMS_OK, 200, 136, 200 * 136 * 2)
    assert _size(3, 5, 1, 1, 1, 255, 0, 0) == (GMS_OK, 1, 1, 2)
    assert _size(100, 7, 2048, 2048, 1000, 25, 1, 3) == (GMS_OK, 2048, 2048, 2048 * 2048 * 2)
    L = _lib.load()
    r = GmsReach(0, 0, 4, 3, 100, 0, 0, 0)
    assert L.gms_reach_size(C.byref(r), None, None, None) == GMS_OK, "every output may be NULL"
    assert L.gms_reach_size(None, None, None, None) == GMS_ERR_INVALID
    for bad in ((0, 0, 0, 3, 100, 0, 0, 0), (0, 0, 4, 0, 100, 0, 0, 0), (0, 0, -1, 3, 100, 0, 0, 0), (0, 0, 4, -1, 100, 0, 0, 0),    # w, h < 1
                (-1, 0, 4, 3, 100, 0, 0, 0), (0, -1, 4, 3, 100, 0, 0, 0),                                                        # x0, y0 < 0
                (0, 0, 4, 3, 0, 0, 0, 0), (0, 0, 4, 3, 0xFFFF, 0, 0, 0), (0, 0, 4, 3, -1, 0, 0, 0), (0, 0, 4, 3, 0x10000, 0, 0, 0),  # max_cost
                (0, 0, 4, 3, 100, -1, 0, 0), (0, 0, 4, 3, 100, 256, 0, 0),                                                       # inflate
                (0, 0, 4, 3, 100, 0, 2, 0), (0, 0, 4, 3, 100, 0, -1, 0)):                                                        # the mode
        assert _size(*bad) == (GMS_ERR_INVALID, -7, -7, -7), bad


def test_entry_points_refuse_null_handles_and_bad_requests():
    """checked before anything is touched: the fake handles are blocks of zero bytes (n_maps 0, W = H = 0), so every index and every
    rectangle -- one off the map -- is bad"""
    L = _lib.load()
    fake = np.zeros(16384, np.uint8).ctypes.data
    out = np.zeros((3, 4), np.uint16)
    seeds = np.zeros((2, 2), np.int32)
    r = C.byref(GmsReach(0, 0, 4, 3, 100, 0, 0, 0))
    o, sd = out.ctypes.data, seeds.ctypes.data
    for fn in (L.gms_map_reach, L.gms_map_reach_dev):
        for args in ((None, 0, r, sd, 2, o), (fake, 0, None, sd, 2, o), (fake, 0, r, None, 2, o), (fake, 0, r, sd, 2, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        assert fn(fake, 0, r, sd, 2, o) == GMS_ERR_INVALID and fn(fake, -1, r, sd, 2, o) == GMS_ERR_INVALID
    for fn in (L.gms_slam_reach, L.gms_slam_reach_dev):
        for args in ((None, 0, r, sd, 2, o, None), (fake, 0, None, sd, 2, o, None), (fake, 0, r, sd, 2, None, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        for args in ((fake, 0, r, sd, 0, o, None), (fake, 0, r, None, 2, o, None), (fake, 0, r, sd, 4097, o, None), (fake, 0, r, sd, -1, o, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"seeds" in L.gms_last_error(), "K = 0 goes with no seeds only"
    assert L.gms_map_reach_stats(None, None, None) == GMS_ERR_INVALID
    assert (out == 0).all(), "a refused request writes nothing"


def test_expectation_on_an_empty_map_is_the_closed_form():
    W, H = 57, 41
    log = np.full((H, W), -0.4)
    for seed in ((10, 10), (0, 0), (W - 1, H - 1), (30, 0)):
        want = rx.closed_form(W, H, seed)
        assert np.array_equal(rx.costs(rx.blocked(log), [seed]), want), seed
        assert np.array_equal(rx.expect(log, [seed]), want.astype(np.uint16))
        assert np.array_equal(rx.expect(log, [seed], max_cost=100), np.where(want <= 100, want, FAR).astype(np.uint16))
    two = np.minimum(rx.closed_form(W, H, (3, 4)), rx.closed_form(W, H, (50, 30)))
    assert np.array_equal(rx.costs(rx.blocked(log), [(3, 4), (50, 30), (-1, 5), (W, 0), (3, 4)]), two), "seeds off the map contribute nothing"
    assert (rx.expect(log, [(-1, 0), (0, H)]) == FAR).all()
    log[20, 20] = 0.85
    f = rx.expect(log, [(19, 19)], not_free=False)
    assert (f[20, 20], f[20, 19], f[19, 20], f[21, 21], f[20, 21], f[21, 20]) == (FAR, 5, 5, 20, 15, 15), "around a corner, never across it"
    g = rx.expect(log, [(19, 20)], inflate=1, not_free=False)
    assert (g == FAR).all() and rx.blocked(log, 1, False).sum() == 5 and rx.blocked(log, 2, False).sum() == 13, "the seed itself is within 1 of the obstacle"


def test_reach_metres():
    f = np.array([[0, 5, 7], [0xFFFF, 0xFFFE, 12]], dtype=np.uint16)
    got = reach_metres(f, 0.05)
    assert got.dtype == np.float64 and got.shape == f.shape
    assert got[0].tolist() == [0.0, 5 / 5 * 0.05, 7 / 5 * 0.05]
    assert got[1, 0] == np.inf and got[1, 1] == 0xFFFE / 5 * 0.05 and got[1, 2] == 12 / 5 * 0.05


def test_cells_of_poses():
    res, pos = 0.05, (-1.0, 0.25)
    f32 = np.float32
    pts = [(-1.0 + 0.05 * 3.5, 0.25 + 0.05 * 7.2), (-1.0 - 0.2 * res, 0.25 - 0.9 * res), (-1.0 - 0.999 * res, 0.25), (-1.0 - 1.5 * res, 0.25 - 2.5 * res),
           (np.nan, 1.0), (1.0, np.nan), (np.inf, -np.inf), (-np.inf, np.inf), (1e30, -1e30), (0.0, 0.0)]
    poses = np.array([(x, y, 0.7) for x, y in pts], dtype=f32)
    gx, gy = cells_of_poses(poses, pos, res)
    wx, wy = xe.cells_of(poses, pos[0], pos[1], res)
    assert gx.dtype == np.int64 and np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert (gx[0], gy[0]) == (3, 7)
    assert (gx[1], gy[1], gx[2]) == (0, 0, 0), "(-1, 0) cells: truncated toward zero"
    assert (gx[3], gy[3]) == (-1, -2)
    assert gx[4] == 0 and gy[5] == 0, "NaN -> 0"
    assert (gx[6], gy[6], gx[7], gy[7]) == (2147483647, -2147483648, -2147483648, 2147483647), "the cast saturates"
    assert (gx[8], gy[8]) == (2147483647, -2147483648)
    one = cells_of_poses(poses[0], pos, res)
    assert one[0].shape == (1,) and one[0][0] == 3


def _legal(path, block):
    for (x, y), (nx, ny) in zip(path, path[1:]):
        assert max(abs(nx - x), abs(ny - y)) == 1 and not block[ny, nx]
        if nx != x and ny != y:
            assert not block[y, nx] and not block[ny, x], "a diagonal step between two free cells only"


def test_descend_on_hand_made_fields():
    # straight
    log = np.full((9, 12), -0.4)
    f = rx.expect(log, [(2, 4)])
    assert descend(f, (7, 4)) == [(7, 4), (6, 4), (5, 4), (4, 4), (3, 4), (2, 4)]
    assert descend(f, (2, 4)) == [(2, 4)]
    assert descend(f, (5, 7)) == [(5, 7), (4, 6), (3, 5), (2, 4)], "a pure diagonal"
    p = descend(f, (11, 0))
    assert p[0] == (11, 0) and p[-1] == (2, 4) and len(p) == 10 and sum(7 if a[0] != b[0] and a[1] != b[1] else 5 for a, b in zip(p, p[1:])) == f[0, 11]
    assert p[1] == (10, 0), "axis moves are tried before diagonal ones, W before S"
    # around a corner: a wall with its end at (6, 4); the seed behind it
    log = np.full((9, 12), -0.4)
    log[0:5, 6] = 0.85
    block = rx.blocked(log)
    f = rx.expect(log, [(3, 1)])
    p = descend(f, (9, 1))
    _legal(p, block)
    assert p[0] == (9, 1) and p[-1] == (3, 1) and (6, 5) in p, "through the cell below the wall's end"
    assert sum(7 if a[0] != b[0] and a[1] != b[1] else 5 for a, b in zip(p, p[1:])) == f[1, 9]
    # refusing a cut corner: the hand-made field offers a diagonal predecessor of the right cost across a blocked side cell
    f = np.full((3, 3), FAR, dtype=np.uint16)
    f[0, 0], f[0, 1], f[1, 0], f[1, 1] = 0, FAR, 5, 7                        # (1, 1) = 7 claims the diagonal from (0, 0) past the FAR cell (1, 0)
    try:
        descend(f, (1, 1))
        assert False, "the only predecessor is across a cut corner"
    except ValueError:
        pass
    f[0, 1] = 5
    assert descend(f, (1, 1)) == [(1, 1), (0, 0)]
    # a FAR start, and one off the map
    assert descend(f, (2, 2)) == [] and descend(f, (3, 0)) == [] and descend(f, (0, -1)) == []
