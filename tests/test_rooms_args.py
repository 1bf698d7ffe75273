"""Rooms and doors (include/gridmapslam.h "rooms and doors") without a device: the records' layout in header and mirror, the exported
symbols, gms_rooms_check / gms_rooms_size at every bound of every field, and the Python helpers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _rooms_expect as rx
from gridmap_slam_robot_amd import DOOR_DTYPE, ROOM_DTYPE, _lib, door_points, room_centroids, room_graph, rooms_of_cells
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsDoor, GmsRoom, GmsRooms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_rooms_check", "gms_rooms_size", "gms_map_rooms", "gms_map_rooms_dev", "gms_slam_rooms", "gms_slam_rooms_dev", "gms_map_rooms_stats",
           "gms_map_rooms_stage_us"]


def test_records_and_constants_in_header_and_mirror(tmp_path):
    assert C.sizeof(GmsRooms) == 48 and C.sizeof(GmsRoom) == ROOM_DTYPE.itemsize == 56 and C.sizeof(GmsDoor) == DOOR_DTYPE.itemsize == 48
    names = ("x0", "y0", "w", "h", "core", "inflate", "mode", "min_core", "max_cost", "filter", "pad")
    assert [getattr(GmsRooms, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    assert [(n, getattr(GmsRoom, n).offset) for n in ROOM_DTYPE.names] == [(n, ROOM_DTYPE.fields[n][1]) for n in ROOM_DTYPE.names]
    assert [(n, getattr(GmsDoor, n).offset) for n in DOOR_DTYPE.names] == [(n, DOOR_DTYPE.fields[n][1]) for n in DOOR_DTYPE.names]
    assert ROOM_DTYPE == rx.ROOM_DTYPE and DOOR_DTYPE == rx.DOOR_DTYPE, "the restatement's records are the library's"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d", '
                   'sizeof(gms_rooms), sizeof(gms_room), sizeof(gms_door), offsetof(gms_rooms, core), offsetof(gms_rooms, max_cost), offsetof(gms_rooms, filter), '
                   'offsetof(gms_room, core_count), offsetof(gms_room, max_depth), offsetof(gms_room, doors), offsetof(gms_room, sum_x), offsetof(gms_door, count), '
                   'offsetof(gms_door, sum_x2), GMS_ROOM_NONE, GMS_ROOMS_MAX); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["48", "56", "48", "16", "32", "36", "8", "32", "36", "40", "8", "32", str(0xFFFFFFFF), str(0xFFFF)]
    assert (_lib.GMS_ROOM_NONE, _lib.GMS_ROOMS_MAX) == (0xFFFFFFFF, 0xFFFF) and rx.NONE == _lib.GMS_ROOM_NONE and rx.FAR == _lib.GMS_REACH_FAR
    assert (rx.AXIS, rx.DIAG) == (_lib.GMS_REACH_AXIS, _lib.GMS_REACH_DIAG)


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None


def _size(*fields):
    q = GmsRooms(*fields)
    w, h, a, b = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7), C.c_int64(-7)
    rc = _lib.load().gms_rooms_size(C.byref(q), C.byref(w), C.byref(h), C.byref(a), C.byref(b))
    assert _lib.load().gms_rooms_check(C.byref(q)) == rc, "gms_rooms_check is gms_rooms_size's verdict"
    return rc, w.value, h.value, a.value, b.value


#       x0 y0 w  h  core inflate mode min_core max_cost filter
GOOD = [(0, 0, 200, 136, 15, 5, 1, 1, 0xFFFE, 0), (3, 5, 1, 1, 1, 0, 0, 1, 1, 0), (0, 0, 4, 3, 255, 254, 1, 1 << 30, 0xFFFE, 7), (100, 7, 2048, 2048, 255, 0, 0, 1, 5, 3)]
BAD = [((0, 0, 4, 3, 5, 5, 0, 1, 100, 0), "core"), ((0, 0, 4, 3, 4, 5, 0, 1, 100, 0), "core"),                    # core <= inflate
       ((0, 0, 4, 3, 256, 5, 0, 1, 100, 0), "core"), ((0, 0, 4, 3, 0, 0, 0, 1, 100, 0), "core"),                  # core = 256, core = 0
       ((0, 0, 4, 3, 255, 255, 0, 1, 100, 0), "inflate"), ((0, 0, 4, 3, 5, -1, 0, 1, 100, 0), "inflate"),         # inflate = 255 and negative
       ((0, 0, 4, 3, 5, 1, 0, 1, 0, 0), "max_cost"), ((0, 0, 4, 3, 5, 1, 0, 1, 0xFFFF, 0), "max_cost"),           # max_cost = 0 and 0xFFFF
       ((0, 0, 4, 3, 5, 1, 0, 1, -3, 0), "max_cost"),
       ((0, 0, 4, 3, 5, 1, 0, 0, 100, 0), "min_core"), ((0, 0, 4, 3, 5, 1, 0, -1, 100, 0), "min_core"),           # min_core = 0
       ((0, 0, 4, 3, 5, 1, 2, 1, 100, 0), "mode"), ((0, 0, 4, 3, 5, 1, -1, 1, 100, 0), "mode"),                   # a bad mode
       ((0, 0, 0, 3, 5, 1, 0, 1, 100, 0), "w and h"), ((0, 0, 4, 0, 5, 1, 0, 1, 100, 0), "w and h"), ((0, 0, -1, 3, 5, 1, 0, 1, 100, 0), "w and h"),
       ((-1, 0, 4, 3, 5, 1, 0, 1, 100, 0), "x0 and y0"), ((0, -1, 4, 3, 5, 1, 0, 1, 100, 0), "x0 and y0")]


def test_rooms_size_and_check():
    for f in GOOD:
        assert _size(*f) == (GMS_OK, f[2], f[3], f[2] * f[3] * 4, f[2] * f[3] * 2), f
    L = _lib.load()
    for f, word in BAD:
        assert _size(*f) == (GMS_ERR_INVALID, -7, -7, -7, -7), f
        assert word in L.gms_last_error().decode(), (f, L.gms_last_error())
    q = GmsRooms(*GOOD[0])
    assert L.gms_rooms_size(C.byref(q), None, None, None, None) == GMS_OK, "every output may be NULL"
    assert L.gms_rooms_size(None, None, None, None, None) == GMS_ERR_INVALID and L.gms_rooms_check(None) == GMS_ERR_INVALID


def test_entry_points_refuse_null_handles_before_anything_else():
    L = _lib.load()
    q = GmsRooms(*GOOD[0])
    n = C.c_int32(-7)
    assert L.gms_map_rooms(None, 0, C.byref(q), None, None, None, 0, C.byref(n), None, 0, C.byref(n)) == GMS_ERR_INVALID
    assert L.gms_map_rooms_dev(None, 0, C.byref(q), None, None, None, 0, None, None, 0, None) == GMS_ERR_INVALID
    assert L.gms_slam_rooms(None, 0, C.byref(q), None, None, None, 0, None, None, 0, None, None) == GMS_ERR_INVALID
    assert L.gms_slam_rooms_dev(None, 0, C.byref(q), None, None, None, 0, None, None, 0, None, None) == GMS_ERR_INVALID
    assert L.gms_map_rooms_stats(None, None, None, None) == GMS_ERR_INVALID and L.gms_map_rooms_stage_us(None, None) == GMS_ERR_INVALID and n.value == -7


def test_helpers_on_the_hand_derived_boxes():
    e = rx.expect(rx.two_boxes(), core=2, inflate=0, not_free=False)
    assert room_centroids(e["rooms"]).tolist() == [[(20 * 230 + 66) / 403, (20 * 230 + 33) / 403], [32.5, 11.5]]
    p = door_points(e["doors"], (1.0, -2.0), 0.05)
    assert p.shape == (1, 2) and p[0] == pytest.approx([1.0 + (22.5 + 0.5) * np.float64(np.float32(0.05)), -2.0 + (11.0 + 0.5) * np.float64(np.float32(0.05))], abs=1e-12)
    cells = [(4, 4), (30, 20), (22, 11), (0, 0), (22, 9), (-1, 3), (46, 3), (3, 24)]
    assert rooms_of_cells(e["labels"], cells).tolist() == [188, 209, 188, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]
    r = rx.expect(rx.two_boxes(), core=2, inflate=0, not_free=False, rect=(20, 9, 5, 3))
    assert rooms_of_cells(r["labels"], [(22, 11), (24, 9), (19, 9), (25, 9)], x0=20, y0=9).tolist() == [188, 209, 0xFFFFFFFF, 0xFFFFFFFF]
    assert room_graph(e["rooms"], e["doors"]) == {188: {209: 3}, 209: {188: 3}}
    lone = rx.expect(rx.corridor(), core=2, inflate=0, not_free=False, max_cost=20)
    assert room_graph(lone["rooms"], lone["doors"]) == {} and room_graph(lone["rooms"], lone["doors"], W=31) == {158: {}, 178: {}}
