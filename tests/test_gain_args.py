"""View gain (include/gridmapslam.h "view gain") without a device: the request's and the record's layout in header, mirror and dtype,
the exported symbols, every refused argument, the helper probe_fan, and the expectation module (tests/_gain_expect.py) against
hand-derived answers on tiny maps."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import _gain_expect as gx
from gridmap_slam_robot_amd import BEAM_DTYPE, GAIN_DTYPE, _lib, probe_fan
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsGain, GmsGainRec
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_map_gain", "gms_map_gain_dev", "gms_slam_gain", "gms_slam_gain_dev"]
REC = ("unknown", "free_cells", "occupied", "hits", "walked", "start_x", "start_y", "pad")
RES = 0.05


def test_structs_in_header_mirror_and_dtype(tmp_path):
    assert C.sizeof(GmsGain) == 8 and [getattr(GmsGain, n).offset for n in ("max_range", "filter")] == [0, 4]
    assert C.sizeof(GmsGainRec) == 32 and [getattr(GmsGainRec, n).offset for n in REC] == list(range(0, 32, 4))
    assert GAIN_DTYPE is _lib.GAIN_DTYPE and GAIN_DTYPE.itemsize == 32 and GAIN_DTYPE.names == REC
    assert [GAIN_DTYPE.fields[n][1] for n in REC] == list(range(0, 32, 4)) and all(GAIN_DTYPE.fields[n][0] == np.dtype("<i4") for n in REC)
    src = tmp_path / "size.c"
    fmt = " ".join(["%zu"] * (4 + len(REC)))
    args = ", ".join(["sizeof(gms_gain)", "sizeof(gms_gain_rec)", "offsetof(gms_gain, max_range)", "offsetof(gms_gain, filter)"]
                     + [f"offsetof(gms_gain_rec, {n})" for n in REC])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\n'
                   f'int main(void) {{ printf("{fmt}", {args}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == [8, 32, 0, 4] + list(range(0, 32, 4))


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    for name in ("gms_map_gain(", "gms_slam_gain("):
        assert name in mirror, name
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])


def test_entry_points_refuse_null_pointers_and_bad_requests():
    """checked before anything is touched: the fake map is a block of zero bytes (max_beams 0, n_maps 0), so after the request, P and
    the alignment every B and every map index is bad as well; each refusal is told apart by its message"""
    L = _lib.load()
    zeros = np.zeros(16384, np.uint8)                  # (kept alive: the handle is this memory)
    fake = zeros.ctypes.data
    poses = np.zeros((2, 3), np.float32)
    probes = np.zeros(4, BEAM_DTYPE)
    out = np.full(4, 7, GAIN_DTYPE)                    # (16-byte aligned: numpy allocates so)
    shown = C.c_int32(-7)
    p, b, o = poses.ctypes.data, probes.ctypes.data, out.ctypes.data
    assert o % 16 == 0
    g = lambda r=10: C.byref(GmsGain(r, 0))

    def refused(fn, args, word):
        assert fn(*args) == GMS_ERR_INVALID, args
        assert word in L.gms_last_error(), (word, L.gms_last_error())
    for fn in (L.gms_map_gain, L.gms_map_gain_dev):
        for args in ((None, 0, g(), p, 2, b, 4, o), (fake, 0, None, p, 2, b, 4, o), (fake, 0, g(), None, 2, b, 4, o), (fake, 0, g(), p, 2, None, 4, o),
                     (fake, 0, g(), p, 2, b, 4, None)):
            refused(fn, args, b"null")
        for r in (0, 256, -1, 1 << 20):
            refused(fn, (fake, 0, g(r), p, 2, b, 4, o), b"max_range")
        for P in (0, -1, (1 << 20) + 1):
            refused(fn, (fake, 0, g(), p, P, b, 4, o), b"poses")
        for B in (0, -1, 1, 4):                        # (the fake handle's max_beams is 0)
            refused(fn, (fake, 0, g(), p, 2, b, B, o), b"probes")
    for off in (4, 8, 12, 1):
        refused(L.gms_map_gain_dev, (fake, 0, g(), p, 2, b, 4, o + off), b"aligned")
    refused(L.gms_map_gain, (fake, 0, g(), p, 2, b, 4, o + 4), b"probes")       # the host form takes any alignment
    for fn in (L.gms_slam_gain, L.gms_slam_gain_dev):
        for args in ((None, 0, g(), p, 2, b, 4, o, C.byref(shown)), (None, -1, g(), p, 2, b, 4, o, None)):
            refused(fn, args, b"null")
    assert (out.view(np.int32) == 7).all() and shown.value == -7, "a refused request writes nothing"


def test_probe_fan():
    f = probe_fan(8, 2.0)
    assert f.dtype == BEAM_DTYPE and f.shape == (8,) and (f["hit"] == 0).all() and (f["distance"] == 2.0).all()
    assert np.allclose(np.hypot(f["local_x"], f["local_y"]), 2.0, rtol=1e-15)
    ang = np.arctan2(f["local_y"], f["local_x"])
    assert np.allclose(ang, (np.arange(8) - 3.5) * (2 * math.pi / 8), atol=1e-15), "evenly spaced, centred on the heading, no probe twice"
    q = probe_fan(4, 0.5, fov=math.pi / 2)
    assert np.allclose(np.arctan2(q["local_y"], q["local_x"]), (np.arange(4) - 1.5) * (math.pi / 8), atol=1e-15)
    one = probe_fan(1, 3.0, fov=1.0)
    assert (one["local_x"][0], one["local_y"][0], one["distance"][0]) == (3.0, 0.0, 3.0), "a single probe looks straight ahead"
    assert len(probe_fan(720, 10.0)) == 720


# ---- the expectation against answers derived by hand -----------------------------------------------------------------------------
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643


def _grid_9x7():
    g = orc.Grid(0.43, 0.33, RES, 0.0, 0.0)
    assert (g.W, g.H) == (9, 7)
    return g


def _axis_probes(cells=10):
    """+x, -x, +y, -y, each `cells` cells long: with theta = 0 they walk a row or a column"""
    d = cells * RES
    b = np.zeros(4, BEAM_DTYPE)
    b["local_x"], b["local_y"], b["distance"] = [d, -d, 0, 0], [0, 0, d, -d], d
    return b


def _rec(**kw):
    r = np.zeros((), GAIN_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def test_expectation_one_wall_cell_on_a_9_x_7_map():
    g = _grid_9x7()
    log = np.full((7, 9), L_FREE)
    log[3, 6] = L_OCC                                  # the wall: four cells east of the pose
    pose = np.array([0.1, 0.15, 0.0], np.float32)      # the centre of cell (2, 3)
    probes = _axis_probes()
    # max_range 3: east (2..5, 3) -- the wall is one cell beyond the cut --, west (1, 3), (0, 3) and off the map, north (2, 4..6) and
    # off the map, south (2, 2..0): 4 + 2 + 3 + 3 = 12 cells, the start cell counted once
    assert gx.expect(g, log, probes, pose, 3) == _rec(free_cells=12, walked=4, start_x=2, start_y=3)
    # max_range 4: the east walk reaches the wall, which ends it and is counted
    want4 = _rec(free_cells=12, occupied=1, hits=1, walked=4, start_x=2, start_y=3)
    assert gx.expect(g, log, probes, pose, 4) == want4
    assert gx.expect(g, log, probes, pose, 255) == want4, "nothing is seen behind the wall, and the other walks end at the map's edge"
    # max_range 1: the start cell and its four axis neighbours
    assert gx.expect(g, log, probes, pose, 1) == _rec(free_cells=5, walked=4, start_x=2, start_y=3)
    # a probe twice: the cells count once, the probes twice
    twice = np.concatenate([probes, probes[:1]])
    assert gx.expect(g, log, twice, pose, 4) == _rec(free_cells=12, occupied=1, hits=2, walked=5, start_x=2, start_y=3)
    # unknown cells are walked through: 0, -0.0 and NaN
    log[5, 2], log[6, 2], log[3, 0] = 0.0, np.nan, -0.0
    assert gx.expect(g, log, probes, pose, 3) == _rec(unknown=3, free_cells=9, walked=4, start_x=2, start_y=3)
    # a short probe ends where it ends: two cells east, no extra steps past the end point
    short = _axis_probes(2)[:1]
    assert gx.expect(g, log, short, pose, 255) == _rec(free_cells=3, walked=1, start_x=2, start_y=3)
    rec, total = gx.Walks(g, probes, pose).record(log, 3)
    assert total == 4 + 3 + 4 + 4 and rec["unknown"] + rec["free_cells"] == 12, "the start cell is walked four times and counted once"


def test_expectation_pose_in_an_occupied_cell_and_outside_the_map():
    g = _grid_9x7()
    log = np.full((7, 9), L_FREE)
    log[3, 2] = L_OCC
    probes = _axis_probes()
    inside = np.array([0.1, 0.15, 0.0], np.float32)
    assert gx.expect(g, log, probes, inside, 5) == _rec(occupied=1, hits=4, walked=4, start_x=2, start_y=3), "every walk ends in its first cell"
    for outside in ([-1.0, 0.15, 0.0], [0.1, 0.36, 1.0], [0.46, -0.2, 2.0]):
        assert gx.expect(g, log, probes, np.array(outside, np.float32), 5) == _rec(start_x=-1, start_y=-1), outside
    both = gx.expect_poses(g, log, probes, np.array([inside, [-1.0, 0.15, 0.0]], np.float32), 5)
    assert both.dtype == GAIN_DTYPE and both.shape == (2,) and both[0]["hits"] == 4 and both[1]["start_x"] == -1
