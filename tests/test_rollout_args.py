"""Trajectory rollouts (include/gridmapslam.h "trajectory rollouts") without a device: the structs' layout in header, mirror and dtype,
the exported symbols, every refused argument, gms_rollout_arcs against hand values, the Python helpers, and the expectation module
(tests/_rollout_expect.py) against hand-derived records on a map of 9 x 7 cells."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _rollout_expect as rx
from gridmap_slam_robot_amd import ROLLOUT_DTYPE, ROLLOUT_RISK_DTYPE, ROLLOUT_STEP_DTYPE, _lib, footprint_box, rollout_arcs, rollout_pick
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GMS_ROLLOUT_CANDIDATES, GmsError, GmsRollout, GmsRolloutRec, GmsRolloutRisk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_rollout_check", "gms_rollout_arcs", "gms_rollout_candidates_per_workgroup", "gms_map_rollout", "gms_map_rollout_dev", "gms_slam_rollout",
           "gms_slam_rollout_dev", "gms_pf_rollout", "gms_pf_rollout_dev"]
REQ = ("max_range", "inflate", "mode", "filter")
REC = ("first_hit", "hit_point", "min_d2", "best_step", "best_cost", "end_cost", "flags", "pad", "last_x", "last_y", "start_x", "start_y")
REC_OFF = [0, 2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28]
RISK = ("n_hit", "n_start_blocked", "min_first_hit", "pad", "sum_first_hit", "pad2")
RISK_OFF = [0, 4, 8, 12, 16, 24]
STEP = ("dx", "dy", "c", "s")
RES = 0.05
FAR = 0xFFFF


def test_structs_in_header_mirror_and_dtype(tmp_path):
    assert C.sizeof(GmsRollout) == 16 and [getattr(GmsRollout, n).offset for n in REQ] == [0, 4, 8, 12]
    assert C.sizeof(GmsRolloutRec) == 32 and [getattr(GmsRolloutRec, n).offset for n in REC] == REC_OFF
    assert C.sizeof(GmsRolloutRisk) == 32 and [getattr(GmsRolloutRisk, n).offset for n in RISK] == RISK_OFF
    assert ROLLOUT_DTYPE is _lib.ROLLOUT_DTYPE and ROLLOUT_DTYPE.itemsize == 32 and ROLLOUT_DTYPE.names == REC
    assert [ROLLOUT_DTYPE.fields[n][1] for n in REC] == REC_OFF
    assert all(ROLLOUT_DTYPE.fields[n][0] == np.dtype("<u2") for n in REC[:8]) and all(ROLLOUT_DTYPE.fields[n][0] == np.dtype("<i4") for n in REC[8:])
    assert ROLLOUT_RISK_DTYPE.itemsize == 32 and ROLLOUT_RISK_DTYPE.names == RISK and [ROLLOUT_RISK_DTYPE.fields[n][1] for n in RISK] == RISK_OFF
    assert ROLLOUT_STEP_DTYPE.itemsize == 16 and ROLLOUT_STEP_DTYPE.names == STEP and [ROLLOUT_STEP_DTYPE.fields[n][1] for n in STEP] == [0, 4, 8, 12]
    sizes = ["sizeof(gms_rollout)", "sizeof(gms_rollout_rec)", "sizeof(gms_rollout_risk)", "sizeof(gms_rollout_step)"]
    offs = ([f"offsetof(gms_rollout, {n})" for n in REQ] + [f"offsetof(gms_rollout_rec, {n})" for n in REC] + [f"offsetof(gms_rollout_risk, {n})" for n in RISK]
            + [f"offsetof(gms_rollout_step, {n})" for n in STEP])
    consts = ["(size_t)GMS_ROLLOUT_MAX_K", "(size_t)GMS_ROLLOUT_MAX_T", "(size_t)GMS_ROLLOUT_MAX_F", "(size_t)GMS_ROLLOUT_CANDIDATES", "(size_t)GMS_ROLLOUT_HIT_OUTSIDE",
              "(size_t)GMS_ROLLOUT_HIT_RANGE", "(size_t)GMS_ROLLOUT_HIT_BLOCKED", "(size_t)GMS_ROLLOUT_START_BLOCKED"]
    every = sizes + offs + consts
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\n'
                   f'int main(void) {{ printf("{" ".join(["%zu"] * len(every))}", {", ".join(every)}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [16, 32, 32, 16] + [0, 4, 8, 12] + REC_OFF + RISK_OFF + [0, 4, 8, 12] + [4096, 256, 64, GMS_ROLLOUT_CANDIDATES, 1, 2, 4, 8]
    assert (_lib.GMS_ROLLOUT_MAX_K, _lib.GMS_ROLLOUT_MAX_T, _lib.GMS_ROLLOUT_MAX_F) == (4096, 256, 64)
    assert (rx.OUTSIDE, rx.RANGE, rx.BLOCKED, rx.START_BLOCKED) == (1, 2, 4, 8)


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    assert header.index("continuous scan alignment") < header.index("---- trajectory rollouts") < header.index("---- device-resident inputs")
    for name in ("gms_map_rollout(", "gms_slam_rollout(", "gms_pf_rollout("):
        assert name in mirror, name
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])
    assert L.gms_rollout_candidates_per_workgroup() == GMS_ROLLOUT_CANDIDATES


def test_check_refuses_every_bad_argument():
    L = _lib.load()
    ok = lambda **kw: GmsRollout(**{**dict(max_range=20, inflate=3, mode=1, filter=0), **kw})
    assert L.gms_rollout_check(C.byref(ok()), 1, 1, 0) == GMS_OK and L.gms_rollout_check(C.byref(ok(max_range=255, inflate=255, mode=0)), 4096, 256, 64) == GMS_OK
    assert L.gms_rollout_check(C.byref(ok(max_range=1, inflate=0)), 17, 65, 8) == GMS_OK

    def refused(req, K, T, F, word):
        assert L.gms_rollout_check(None if req is None else C.byref(req), K, T, F) == GMS_ERR_INVALID, (K, T, F)
        assert word in L.gms_last_error(), (word, L.gms_last_error())
    refused(None, 1, 1, 0, b"null")
    for K in (0, -1, 4097, 1 << 30):
        refused(ok(), K, 8, 4, b"K")
    for T in (0, -1, 257, 1 << 30):
        refused(ok(), 8, T, 4, b"T")
    for F in (-1, 65, 1 << 30):
        refused(ok(), 8, 8, F, b"F")
    for R in (0, -1, 256, 1 << 20):
        refused(ok(max_range=R), 8, 8, 4, b"max_range")
    for inf in (-1, 256, 1 << 20):
        refused(ok(inflate=inf), 8, 8, 4, b"inflate")
    for mode in (-1, 2, 7):
        refused(ok(mode=mode), 8, 8, 4, b"mode")


def test_entry_points_refuse_null_pointers_and_bad_requests():
    """checked before anything is touched: the fake map is a block of zero bytes (n_maps 0), so behind the request, P and the alignment
    every map index is bad as well; each refusal is told apart by its message"""
    L = _lib.load()
    zeros = np.zeros(16384, np.uint8)                  # (kept alive: the handle is this memory)
    fake = zeros.ctypes.data
    poses = np.zeros((2, 3), np.float32)
    arcs = np.zeros((3, 4), ROLLOUT_STEP_DTYPE)
    pts = np.zeros((2, 2), np.float32)
    out = np.full((2, 3), 7, np.uint8).repeat(32).view(ROLLOUT_DTYPE).reshape(2, 3)
    risk = np.full(3 * 32, 7, np.uint8).view(ROLLOUT_RISK_DTYPE)
    shown = C.c_int32(-7)
    p, a, f, o, rk = poses.ctypes.data, arcs.ctypes.data, pts.ctypes.data, out.ctypes.data, risk.ctypes.data
    assert o % 16 == 0 and a % 16 == 0 and rk % 16 == 0
    g = lambda **kw: C.byref(GmsRollout(**{**dict(max_range=10, inflate=0, mode=0, filter=0), **kw}))

    def refused(fn, args, word):
        assert fn(*args) == GMS_ERR_INVALID, args
        assert word in L.gms_last_error(), (word, L.gms_last_error())
    for fn in (L.gms_map_rollout, L.gms_map_rollout_dev):
        for args in ((None, 0, g(), p, 2, a, 3, 4, f, 2, None, None, o), (fake, 0, None, p, 2, a, 3, 4, f, 2, None, None, o),
                     (fake, 0, g(), None, 2, a, 3, 4, f, 2, None, None, o), (fake, 0, g(), p, 2, None, 3, 4, f, 2, None, None, o),
                     (fake, 0, g(), p, 2, a, 3, 4, None, 2, None, None, o), (fake, 0, g(), p, 2, a, 3, 4, f, 2, None, None, None)):
            refused(fn, args, b"null")
        refused(fn, (fake, 0, g(max_range=0), p, 2, a, 3, 4, f, 2, None, None, o), b"max_range")
        refused(fn, (fake, 0, g(inflate=256), p, 2, a, 3, 4, f, 2, None, None, o), b"inflate")
        refused(fn, (fake, 0, g(mode=2), p, 2, a, 3, 4, f, 2, None, None, o), b"mode")
        refused(fn, (fake, 0, g(), p, 2, a, 0, 4, f, 2, None, None, o), b"K")
        refused(fn, (fake, 0, g(), p, 2, a, 3, 257, f, 2, None, None, o), b"T")
        refused(fn, (fake, 0, g(), p, 2, a, 3, 4, f, 65, None, None, o), b"F")
        for P in (0, -1, (1 << 20) + 1):
            refused(fn, (fake, 0, g(), p, P, a, 3, 4, f, 2, None, None, o), b"poses")
        refused(fn, (fake, 0, g(), p, 2, a, 3, 4, None, 0, None, None, o), b"map index")     # F == 0 needs no points; the fake handle has no map
    for off in (4, 8, 1):
        refused(L.gms_map_rollout_dev, (fake, 0, g(), p, 2, a, 3, 4, f, 2, None, None, o + off), b"aligned")
        refused(L.gms_map_rollout_dev, (fake, 0, g(), p, 2, a + off, 3, 4, f, 2, None, None, o), b"aligned")
    refused(L.gms_map_rollout_dev, (fake, 0, g(), p, 2, a, 3, 4, f, 2, p + 1, None, o), b"aligned")
    refused(L.gms_map_rollout, (fake, 0, g(), p, 2, a, 3, 4, f, 2, None, None, o + 4), b"map index")       # the host form takes any alignment
    for fn in (L.gms_slam_rollout, L.gms_slam_rollout_dev):
        refused(fn, (None, 0, g(), p, 2, a, 3, 4, f, 2, None, None, o, C.byref(shown)), b"null")
        refused(fn, (None, -1, g(), None, 0, a, 3, 4, f, 2, None, None, o, None), b"null")
    for fn in (L.gms_pf_rollout, L.gms_pf_rollout_dev):
        for args in ((None, g(), a, 3, 4, f, 2, rk), (fake, None, a, 3, 4, f, 2, rk), (fake, g(), None, 3, 4, f, 2, rk), (fake, g(), a, 3, 4, None, 2, rk),
                     (fake, g(), a, 3, 4, f, 2, None)):
            refused(fn, args, b"null")
        refused(fn, (fake, g(), a, 4097, 4, f, 2, rk), b"K")
        refused(fn, (fake, g(max_range=256), a, 3, 4, f, 2, rk), b"max_range")
    assert (out.view(np.uint8) == 7).all() and (risk.view(np.uint8) == 7).all() and shown.value == -7, "a refused request writes nothing"


def test_arcs_on_a_straight_line_and_a_quarter_circle():
    f32 = np.float32
    line = rollout_arcs([0.5, -0.25], [0.0, 1e-10], 0.1, 3)
    assert line.dtype == ROLLOUT_STEP_DTYPE and line.shape == (2, 3)
    assert line["dx"].tolist() == [[f32(0.5 * 0.1), f32(0.5 * 0.2), f32(0.5 * (3 * 0.1))], [f32(-0.25 * 0.1), f32(-0.25 * 0.2), f32(-0.25 * (3 * 0.1))]]
    assert (line["dy"] == 0).all() and (line["s"][0] == 0).all() and (line["c"] == 1).all(), "the straight line where |omega| < 1e-9"
    assert line["s"][1].tolist() == [f32(1e-10 * 0.1), f32(1e-10 * 0.2), f32(1e-10 * (3 * 0.1))]
    quarter = rollout_arcs([1.0], [math.pi / 2], 0.5, 2)[0]              # radius 2 / pi; after 0.5 s an eighth, after 1 s a quarter of the circle
    r = 2 / math.pi
    assert np.allclose([quarter["dx"][0], quarter["dy"][0], quarter["c"][0], quarter["s"][0]],
                       [0.45015815807855303, 0.18646161428902837, 0.7071067811865476, 0.7071067811865476], rtol=0, atol=3e-8)
    assert np.allclose([quarter["dx"][1], quarter["dy"][1], quarter["s"][1]], [0.6366197723675814, 0.6366197723675814, 1.0], rtol=0, atol=3e-8)
    assert abs(float(quarter["c"][1])) < 1e-16
    th = (math.pi / 2) * (2 * 0.5)
    assert quarter[1].tolist() == (f32((1.0 / (math.pi / 2)) * math.sin(th)), f32((1.0 / (math.pi / 2)) * (1.0 - math.cos(th))), f32(math.cos(th)), f32(math.sin(th)))
    assert abs(r - 1.0 / (math.pi / 2)) < 1e-15
    back = rollout_arcs([-1.0], [-math.pi / 2], 0.5, 2)[0]
    assert back["dx"][1] < 0 and back["dy"][1] > 0 and back["s"][1] == -1, "reversing while turning right ends behind and to the left"
    for bad in (dict(dt=0.0), dict(dt=float("nan")), dict(T=0), dict(T=257)):
        with pytest.raises(GmsError) as e:
            rollout_arcs([1.0], [0.0], **{**dict(dt=0.1, T=4), **bad})
        assert e.value.code == GMS_ERR_INVALID


def test_footprint_box_and_pick():
    box = footprint_box(0.4, 0.2, 0.1)
    assert box.dtype == np.float32 and box.shape == (12, 2), "four parts along x, two along y, each corner once"
    assert len({(float(x), float(y)) for x, y in box}) == 12
    assert np.allclose(box[0], [-0.2, -0.1]) and np.allclose(box[4], [0.2, -0.1]) and np.allclose(box[6], [0.2, 0.1]) and np.allclose(box[10], [-0.2, 0.1])
    assert np.allclose(np.maximum(np.abs(box[:, 0]) / 0.2, np.abs(box[:, 1]) / 0.1), 1.0), "every point on the outline"
    with pytest.raises(ValueError):
        footprint_box(2.0, 2.0, 0.05)
    rec = np.zeros(4, ROLLOUT_DTYPE)
    rec["first_hit"] = [8, 8, 5, 8]
    rec["best_cost"] = [40, 30, 10, 20]
    rec["min_d2"] = [FAR, 9, 25, 1]
    rec["flags"] = [0, 0, 4, 0]
    assert rollout_pick(rec, T=8) == 3, "the cheapest collision-free arc"
    assert rollout_pick(rec, T=8, min_d2=4) == 1, "... that keeps two cells clear"
    assert rollout_pick(rec, T=8, w_cost=0.0, w_clear=1.0) == 0
    assert rollout_pick(rec, T=9) == -1 and rollout_pick(rec[:0]) == -1
    rec["flags"][3] = 8
    assert rollout_pick(rec) == 1, "a footprint that collides at the start pose is not admissible"


# ---- the expectation against answers derived by hand -----------------------------------------------------------------------------
# A 9 x 7 map at the origin, cells of 5 cm.  The start pose is the middle of cell (2, 3), heading east; step j of the arc moves the
# centre j + 1 cells east, to the middle of cell (3 + j, 3).
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
GEO = rx.Geometry(9, 7, RES, 0.0, 0.0)
POSE = np.array([0.125, 0.175, 0.0], np.float32)
SIDES = np.array([[0.0, 0.05], [0.0, -0.05]], np.float32)     # point 0 one cell to the left (y + 1), point 1 one to the right; the centre is point 2


def _east(T):
    j = np.arange(T)
    return rx.steps(((j + 1) * RES).astype(np.float32), np.zeros(T), np.ones(T), np.zeros(T)).reshape(1, T)


def _rec(**kw):
    r = np.zeros((), ROLLOUT_DTYPE)
    r["hit_point"], r["min_d2"], r["best_step"], r["best_cost"], r["end_cost"] = 0xFFFF, FAR, 0xFFFF, FAR, FAR
    r["start_x"], r["start_y"] = 2, 3
    for k, v in kw.items():
        r[k] = v
    return r


def _one(log, T, points=(), R=20, **kw):
    got = rx.expect(GEO, log, POSE, _east(T), np.asarray(points, np.float32).reshape(-1, 2), R, **kw)
    assert got.shape == (1, 1) and got.dtype == ROLLOUT_DTYPE
    return got[0, 0]


def test_expectation_hits_at_step_0_at_the_last_step_and_none():
    log = np.full((7, 9), L_FREE)
    assert _one(log, 5) == _rec(first_hit=5, last_x=7, last_y=3), "no hit: first_hit = T, the last cell is step T - 1's"
    assert _one(log, 1) == _rec(first_hit=1, last_x=3, last_y=3)
    log[3, 3] = L_OCC
    assert _one(log, 5) == _rec(first_hit=0, hit_point=0, flags=rx.BLOCKED, last_x=2, last_y=3), "a hit at step 0: the last cell is the start cell"
    log[3, 3] = L_FREE
    log[3, 7] = L_OCC
    assert _one(log, 5) == _rec(first_hit=4, hit_point=0, flags=rx.BLOCKED, last_x=6, last_y=3), "a hit at step T - 1"
    assert _one(log, 4) == _rec(first_hit=4, last_x=6, last_y=3), "one step shorter: none"
    for unknown in (0.0, -0.0, np.nan):
        log[3, 7] = L_FREE
        log[3, 5] = unknown
        assert _one(log, 5, not_free=True) == _rec(first_hit=2, hit_point=0, flags=rx.BLOCKED, last_x=4, last_y=3), "never observed blocks a planner's mode"
        assert _one(log, 5, not_free=False) == _rec(first_hit=5, last_x=7, last_y=3), "... and not the casts'"


def test_expectation_two_points_at_one_step_the_smaller_index_wins():
    log = np.full((7, 9), L_FREE)
    log[4, 5] = log[2, 5] = L_OCC                      # left and right of the centre's path, both reached at step 2
    assert _one(log, 5, SIDES) == _rec(first_hit=2, hit_point=0, flags=rx.BLOCKED, last_x=4, last_y=3)
    log[4, 5] = L_FREE
    assert _one(log, 5, SIDES) == _rec(first_hit=2, hit_point=1, flags=rx.BLOCKED, last_x=4, last_y=3)
    log[2, 5] = L_FREE
    log[3, 5] = L_OCC
    assert _one(log, 5, SIDES) == _rec(first_hit=2, hit_point=2, flags=rx.BLOCKED, last_x=4, last_y=3), "the centre is point F, tested last"
    assert _one(log, 5) == _rec(first_hit=2, hit_point=0, flags=rx.BLOCKED, last_x=4, last_y=3), "... and point 0 without a footprint"
    log[3, 5] = L_FREE
    log[4, 2] = L_OCC                                  # beside the start pose: under point 0 at the identity step only
    assert _one(log, 5, SIDES) == _rec(first_hit=5, flags=rx.START_BLOCKED, last_x=7, last_y=3), "START_BLOCKED is independent of first_hit"
    log[4, 4] = L_OCC
    assert _one(log, 5, SIDES) == _rec(first_hit=1, hit_point=0, flags=rx.START_BLOCKED | rx.BLOCKED, last_x=3, last_y=3)
    log[:] = L_FREE
    log[3, 6] = L_OCC                                  # inflated by one cell it blocks (5, 3) as well -- d2 = 1 --, not (5, 2) and (5, 4): d2 = 2
    assert _one(log, 5, SIDES, inflate=1) == _rec(first_hit=2, hit_point=2, flags=rx.BLOCKED, last_x=4, last_y=3)
    log[3, 6], log[4, 6] = L_FREE, L_OCC               # ... and from (6, 4) it blocks (5, 4), under point 0
    assert _one(log, 5, SIDES, inflate=1) == _rec(first_hit=2, hit_point=0, flags=rx.BLOCKED, last_x=4, last_y=3)
    log[3, 6], log[4, 6] = L_OCC, L_FREE
    assert _one(log, 5, SIDES, inflate=0) == _rec(first_hit=3, hit_point=2, flags=rx.BLOCKED, last_x=5, last_y=3)


def test_expectation_leaving_the_map_and_the_range():
    log = np.full((7, 9), L_FREE)
    assert _one(log, 7) == _rec(first_hit=6, hit_point=0, flags=rx.OUTSIDE, last_x=8, last_y=3), "step 6 is cell (9, 3): off the map"
    assert _one(log, 7, R=3) == _rec(first_hit=3, hit_point=0, flags=rx.RANGE, last_x=5, last_y=3), "cell (6, 3) is four cells from the start cell"
    assert _one(log, 7, R=6) == _rec(first_hit=6, hit_point=0, flags=rx.OUTSIDE, last_x=8, last_y=3), "off the map is tested before the range"
    far_sides = np.array([[0.0, 0.2], [0.0, -0.1]], np.float32)       # point 0 four cells to the left: row 7, off the map, at every step and at the start
    assert _one(log, 5, far_sides) == _rec(first_hit=0, hit_point=0, flags=rx.OUTSIDE | rx.START_BLOCKED, last_x=2, last_y=3)
    assert _one(log, 5, far_sides[1:], R=1) == _rec(first_hit=0, hit_point=0, flags=rx.RANGE | rx.START_BLOCKED, last_x=2, last_y=3), "two cells aside: out of range"
    off = rx.expect(GEO, log, np.array([-0.3, 0.175, 0.0], np.float32), _east(8), np.zeros((0, 2)), 20)[0, 0]
    assert (off["start_x"], off["start_y"]) == (-6, 3) and off["flags"] == rx.OUTSIDE | rx.START_BLOCKED and off["first_hit"] == 0
    nan = rx.expect(GEO, log, np.array([np.nan, 0.175, 0.0], np.float32), _east(3), np.zeros((0, 2)), 20)[0, 0]
    assert (nan["start_x"], nan["start_y"], nan["first_hit"], nan["last_x"], nan["flags"]) == (0, 3, 3, 0, 0), "a NaN coordinate is cell 0, at every step"


def test_expectation_fields_along_the_arc():
    log = np.full((7, 9), L_FREE)
    clear = np.full((7, 9), FAR, np.uint16)
    cost = np.full((7, 9), FAR, np.uint16)
    clear[3, 3:8] = [9, 4, 1, 4, 9]
    cost[3, 3:8] = [30, 20, 20, 40, 50]
    cost[3, 2] = 5                                     # the start cell is no step
    assert _one(log, 5, clear=clear, cost=cost) == _rec(first_hit=5, min_d2=1, best_step=1, best_cost=20, end_cost=50, last_x=7, last_y=3), "ties: the smaller step"
    assert _one(log, 5, cost=cost) == _rec(first_hit=5, best_step=1, best_cost=20, end_cost=50, last_x=7, last_y=3)
    assert _one(log, 5, clear=clear) == _rec(first_hit=5, min_d2=1, last_x=7, last_y=3)
    log[3, 5] = L_OCC
    assert _one(log, 5, clear=clear, cost=cost) == _rec(first_hit=2, hit_point=0, flags=rx.BLOCKED, min_d2=4, best_step=1, best_cost=20, end_cost=20, last_x=4,
                                                        last_y=3), "only the steps in front of the hit count"
    log[3, 3] = L_OCC
    assert _one(log, 5, clear=clear, cost=cost) == _rec(first_hit=0, hit_point=0, flags=rx.BLOCKED, last_x=2, last_y=3), "no step in front of the hit: FAR"
    log[:] = L_FREE
    cost[3, 3:8] = FAR
    assert _one(log, 5, cost=cost) == _rec(first_hit=5, best_step=0, best_cost=FAR, end_cost=FAR, last_x=7, last_y=3), "every cell FAR: the smallest step holds the least"
    two = rx.expect(GEO, log, np.stack([POSE, POSE]), np.concatenate([_east(5), _east(5)]), np.zeros((0, 2)), 20)
    assert two.shape == (2, 2) and (two == two[0, 0]).all()
    risk = rx.risk_of(np.array([[_rec(first_hit=5), _rec(first_hit=2)], [_rec(first_hit=3, flags=8), _rec(first_hit=0, flags=12)]]), 5)
    assert risk.dtype == ROLLOUT_RISK_DTYPE and risk["n_hit"].tolist() == [1, 2] and risk["n_start_blocked"].tolist() == [1, 1]
    assert risk["min_first_hit"].tolist() == [3, 0] and risk["sum_first_hit"].tolist() == [8, 2] and (risk["pad"] == 0).all() and (risk["pad2"] == 0).all()
