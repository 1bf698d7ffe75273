"""Rooms and doors of the shared maps on the device (include/gridmapslam.h "rooms and doors"): gms_map_rooms[_dev] against the plain
restatement of tests/_rooms_expect.py (flood fill, heap Dijkstra over (cost, rank), Python loops) on logData that was constructed or
downloaded.  Every comparison is array_equal: the feature is all-integer and every output is unique.  A request must see the map as a
download would return it at that moment and must change no later result of its handle.

The usual map is 200 x 136 cells: 4 x 3 tiles of 64 x 64 cells, ragged on both far edges (8 columns, 8 rows)."""
import functools
import math

import numpy as np
import pytest

import _rooms_expect as rx
from gridmap_slam_robot_amd import GridMap, Observation, _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
FAR, NONE = 0xFFFF, 0xFFFFFFFF
CAP = 4096
BOX = dict(core=2, inflate=0, not_free=False)          # the hand-derived maps' request (tests/test_rooms_expect.py)


def _map(w=W, h=H, **kw):
    m = GridMap((w - 0.4) * RES, (h - 0.4) * RES, RES, (0.0, 0.0), max_beams=128, **kw)
    assert (m.W, m.H) == (w, h)
    return m


def _check(m, log, where, upload=True, mi=0, rect=None, **kw):
    if upload:
        m.upload_log(log)
    want = rx.expect(log, rect=rect, **kw)
    rx.same(m.rooms(labels=True, depth=True, cap_rooms=CAP, cap_doors=CAP, rect=rect, mi=mi, **kw), want, where)
    return want


def _embed(small, x, y, w=W, h=H):
    log = rx.walls(w, h)
    log[y:y + small.shape[0], x:x + small.shape[1]] = small
    return log


# ---- 1: trivial maps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (64, 64), (65, 65), (150, 100)])
def test_fresh_maps(w, h):
    m = _map(w, h)
    r = m.rooms(core=1, inflate=0, not_free=True, depth=True)
    assert r["n_rooms"] == 0 and r["n_doors"] == 0 and len(r["rooms"]) == 0 and len(r["doors"]) == 0
    assert (r["labels"] == NONE).all() and (r["depth"] == FAR).all() and r["labels"].shape == (h, w), "never observed: every cell an obstacle"
    r = m.rooms(core=1, inflate=0, not_free=False, depth=True)
    assert r["n_rooms"] == 1 and r["n_doors"] == 0 and (r["labels"] == 0).all() and not r["depth"].any(), "nothing occupied: one room, all core"
    room = r["rooms"][0]
    assert (room["anchor_x"], room["anchor_y"], room["core_count"], room["count"], room["doors"], room["max_depth"]) == (0, 0, w * h, w * h, 0, 0)
    assert (room["min_x"], room["min_y"], room["max_x"], room["max_y"]) == (0, 0, w - 1, h - 1)
    assert (room["sum_x"], room["sum_y"]) == (h * w * (w - 1) // 2, w * h * (h - 1) // 2)
    rx.same(r, rx.expect(np.zeros((h, w)), core=1, inflate=0, not_free=False), "the restatement agrees")
    m.close()


# ---- 2: two rooms and a door, hand-derived (tests/test_rooms_expect.py) -----------------------------------------------------------------
@pytest.mark.parametrize("w,h,ox,oy,where", [(W, H, 0, 0, "inside a tile"), (W, H, 41, 30, "the contacts across x = 63 | 64"),
                                             (W, H, 41, 53, "the gap on the tile corner (63 | 64, 63 .. 65)"), (150, 100, 106, 70, "in the ragged last tile")])
def test_two_boxes_and_a_door(w, h, ox, oy, where):
    m = _map(w, h)
    e = _check(m, rx.two_boxes(w, h, ox, oy), where, **BOX)
    assert e["rooms"]["core_count"].tolist() == [260, 260] and e["rooms"]["count"].tolist() == [403, 400] and e["rooms"]["doors"].tolist() == [1, 1]
    d = e["doors"]
    assert len(d) == 1 and (d["a"][0], d["b"][0]) == ((4 + oy) * w + 4 + ox, (4 + oy) * w + 25 + ox)
    assert (d["count"][0], d["min_x"][0], d["min_y"][0], d["max_x"][0], d["max_y"][0]) == (3, 22 + ox, 10 + oy, 23 + ox, 12 + oy)
    assert (d["sum_x2"][0], d["sum_y2"][0]) == (135 + 6 * ox, 66 + 6 * oy)
    m.close()


def test_two_gaps_one_door_and_chains():
    m = _map()
    log = rx.two_boxes(W, H, 41, 50)
    rx.carve(log, 63, 66, 63, 69)                                               # a second opening of 4 cells in the same wall
    e = _check(m, log, "two gaps between the same rooms", **BOX)
    assert e["n_doors"] == 1 and e["doors"]["count"][0] == 3 + 4 and (e["doors"]["min_y"][0], e["doors"]["max_y"][0]) == (60, 69)
    # three rooms in a chain: two doors, doors per room 1, 2, 1
    log = rx.walls(W, H)
    for k in range(3):
        rx.carve(log, 40 + 25 * k, 50, 60 + 25 * k, 75)
    rx.carve(log, 61, 60, 64, 62)
    rx.carve(log, 86, 63, 89, 66)
    e = _check(m, log, "a chain of three", **BOX)
    assert e["n_rooms"] == 3 and e["n_doors"] == 2 and e["rooms"]["doors"].tolist() == [1, 2, 1]
    # a T-junction: three rooms meeting in a hall
    log = rx.walls(W, H)
    rx.carve(log, 50, 56, 80, 72)                                               # the hall
    rx.carve(log, 20, 50, 46, 80)                                               # west
    rx.carve(log, 84, 50, 110, 80)                                              # east
    rx.carve(log, 55, 20, 75, 52)                                               # north
    rx.carve(log, 47, 62, 49, 65)
    rx.carve(log, 81, 63, 83, 66)
    rx.carve(log, 63, 53, 66, 55)
    e = _check(m, log, "a T-junction", **BOX)
    assert e["n_rooms"] == 4 and e["n_doors"] == 3 and sorted(e["rooms"]["doors"].tolist()) == [1, 1, 1, 3]
    m.close()


# ---- 3: the tie rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", ["none", "x", "y", "transpose", "transpose_y"])
@pytest.mark.parametrize("tall", [False, True])
def test_the_contested_cell_goes_to_the_smaller_anchor(flip, tall):
    small = rx.corridor(tall_right=tall)
    small = {"none": small, "x": small[:, ::-1], "y": small[::-1], "transpose": small.T, "transpose_y": small.T[::-1]}[flip]
    m = _map()
    log = _embed(np.ascontiguousarray(small), 50, 55)                           # the corridor crosses x = 63 | 64 or y = 63 | 64
    e = _check(m, log, f"corridor, flip {flip}, tall {tall}", **BOX)
    assert e["n_rooms"] == 2 and e["n_doors"] == 1 and e["doors"]["count"][0] == 1
    mid = {"none": (15, 7), "x": (15, 7), "y": (15, 5), "transpose": (7, 15), "transpose_y": (7, 15)}[flip]
    assert e["depth"][55 + mid[1], 50 + mid[0]] == 35, "equally far from both cores"
    assert e["labels"][55 + mid[1], 50 + mid[0]] == e["doors"]["a"][0], "the smaller anchor wins"
    m.close()


# ---- 4: many rounds ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _snake():
    """a one-cell corridor through all twelve tiles of 256 x 192, a 7 x 7 room (the only core) at its start"""
    w, h = 256, 192
    log = rx.walls(w, h)
    rows = list(range(8, h, 16))
    for k, y in enumerate(rows):
        rx.carve(log, 4, y, w - 5, y)
        if k + 1 < len(rows):
            x = w - 5 if k % 2 == 0 else 4
            rx.carve(log, x, y, x, rows[k + 1])
    rx.carve(log, 4, 5, 10, 11)
    end = (4, rows[-1]) if len(rows) % 2 == 0 else (w - 5, rows[-1])
    log.flags.writeable = False
    return log, rx.expect(log, core=1, inflate=0, not_free=False), end


@pytest.mark.parametrize("batch", [None, "1"])
def test_a_snake_through_every_tile(batch, monkeypatch):
    if batch:
        monkeypatch.setenv("GMS_ROOMS_BATCH", batch)
    log, want, end = _snake()
    m = _map(256, 192)
    m.upload_log(np.array(log))
    got = m.rooms(core=1, inflate=0, not_free=False, depth=True)
    rx.same(got, want, f"the snake, batch {batch}")
    assert want["n_rooms"] == 1 and got["labels"][end[1], end[0]] == want["rooms"]["anchor_y"][0] * 256 + want["rooms"]["anchor_x"][0]
    assert 10000 < got["depth"][end[1], end[0]] < FAR, "the far end is reached"
    st = m.rooms_stats()
    assert 12 < st["rounds"] <= 0xFFFE // 5 + 2 and st["tile_runs"] >= st["rounds"] and st["door_rebuilds"] == 0, st
    m.close()


# ---- 5: min_core, max_cost, corners, cell classes ------------------------------------------------------------------------------------------
def test_min_core_max_cost_and_corners():
    m = _map()
    log = rx.two_boxes(W, H, 41, 30)
    rx.carve(log, 64, 32, 83, 51, rx.L_OCC)
    rx.carve(log, 64, 37, 71, 45)                                               # the right box shrunk: a core of 24 cells
    assert _check(m, log, "two cores", **BOX)["rooms"]["core_count"].tolist() == [260, 24]
    e = _check(m, log, "a small core absorbed by its neighbour", min_core=25, **BOX)
    assert e["n_rooms"] == 1 and e["n_doors"] == 0 and e["rooms"]["count"][0] == 403 + 72
    e = _check(m, log, "no qualifying core at all", min_core=261, **BOX)
    assert e["n_rooms"] == 0 and (e["labels"] == NONE).all()
    log = _embed(rx.corridor(), 50, 55)
    e = _check(m, log, "max_cost cuts the corridor", max_cost=20, **BOX)
    assert e["n_rooms"] == 2 and e["n_doors"] == 0 and (e["labels"][62, 63:68] == NONE).all() and e["labels"][62, 62] != NONE
    e = _check(m, log, "max_cost = 34: one step short of the contested cell", max_cost=34, **BOX)
    assert e["n_doors"] == 0 and e["labels"][62, 65] == NONE and e["labels"][62, 64] != NONE and e["labels"][62, 66] != NONE
    assert _check(m, log, "max_cost = 35", max_cost=35, **BOX)["n_doors"] == 1
    # areas touching only diagonally between two blocked cells, the corner on the tile corner (63 | 64, 63 | 64)
    log = rx.walls(W, H)
    rx.carve(log, 55, 59, 63, 63)
    rx.carve(log, 64, 64, 70, 68)
    e = _check(m, log, "two rooms touching diagonally: no door", core=1, inflate=0, not_free=False, min_core=8)
    assert e["n_rooms"] == 2 and e["n_doors"] == 0
    e = _check(m, log, "nothing grows across the corner", core=1, inflate=0, not_free=False, min_core=20)
    assert e["n_rooms"] == 1 and (e["labels"][64:69, 64:71] == NONE).all()
    m.close()


@pytest.mark.parametrize("not_free", [False, True])
def test_cell_classes(not_free):
    log = rx.two_boxes(W, H, 41, 30)
    log[40, 50], log[45, 55], log[50, 48] = np.nan, 0.0, -0.0                   # inside the left box
    log[40:43, 70] = np.nan
    log[48, 64:68] = -0.0
    m = _map()
    e = _check(m, log, f"NaN, 0.0 and -0.0, not_free = {not_free}", core=2, inflate=0, not_free=not_free)
    assert (e["labels"][40, 50] == NONE) == not_free and (e["labels"][45, 55] == NONE) == not_free and (e["labels"][50, 48] == NONE) == not_free
    m.close()


# ---- 6: limits -------------------------------------------------------------------------------------------------------------------------------
def _comb():
    """a hall with 3 x 3 cells behind one-cell doors on both sides: 98 rooms touching the hall, more than the door table holds at first"""
    log = rx.walls(W, 40)
    rx.carve(log, 1, 15, W - 2, 24)
    for k in range(49):
        x = 2 + 4 * k
        for y0, door in ((10, 14), (26, 25)):
            rx.carve(log, x, y0, x + 2, y0 + 3)
            rx.carve(log, x + 1, door, x + 1, door)
    return log


def test_caps_and_door_table_growth():
    log = _comb()
    want = rx.expect(log, core=1, inflate=0, not_free=False)
    assert want["n_rooms"] == 99 and want["n_doors"] == 98
    m = _map(W, 40)
    m.upload_log(log)
    got = m.rooms(core=1, inflate=0, not_free=False, depth=True, cap_rooms=CAP, cap_doors=CAP)
    rx.same(got, want, "the comb")
    assert m.rooms_stats()["door_rebuilds"] >= 1, "98 pairs do not fit the first table"
    got = m.rooms(core=1, inflate=0, not_free=False, depth=True, cap_rooms=CAP, cap_doors=CAP)
    rx.same(got, want, "again, the table grown")
    assert m.rooms_stats()["door_rebuilds"] == 0
    few = m.rooms(core=1, inflate=0, not_free=False, cap_rooms=7, cap_doors=5)
    assert (few["n_rooms"], few["n_doors"]) == (99, 98) and np.array_equal(few["rooms"], want["rooms"][:7]) and np.array_equal(few["doors"], want["doors"][:5])
    none = m.rooms(core=1, inflate=0, not_free=False, labels=False, cap_rooms=0, cap_doors=0)
    assert (none["n_rooms"], none["n_doors"]) == (99, 98) and len(none["rooms"]) == 0 and len(none["doors"]) == 0 and none["labels"] is None
    m.close()


def _lattice(n):
    log = np.full((n, n), rx.L_FREE)
    log[::4, :] = rx.L_OCC
    log[:, ::4] = rx.L_OCC
    return log


def test_the_rank_limit():
    m = _map(1020, 1020)
    m.upload_log(_lattice(1020))                                                # 255 x 255 cells of 3 x 3 behind closed walls: the core is the centre
    r = m.rooms(core=1, inflate=0, not_free=False, rect=(0, 0, 9, 5), depth=True, cap_rooms=0xFFFF, cap_doors=4)
    assert r["n_rooms"] == 255 * 255 == 65025 and r["n_doors"] == 0
    rooms = r["rooms"]
    assert (rooms["anchor_x"][0], rooms["anchor_y"][0]) == (2, 2) and (rooms["anchor_x"][-1], rooms["anchor_y"][-1]) == (1018, 1018)
    # (the map's far edges are no obstacles: in the last column and row of cells the core reaches the edge, 2 cells, 4 in the corner)
    edge = (np.arange(255) == 254) + 1
    assert (rooms["count"] == 9).all() and np.array_equal(rooms["core_count"], np.outer(edge, edge).ravel()) and (rooms["max_depth"] == 7).all()
    assert np.array_equal(rooms["anchor_x"], np.tile(2 + 4 * np.arange(255), 255)) and np.array_equal(rooms["anchor_y"], np.repeat(2 + 4 * np.arange(255), 255))
    a, b, n = 2 * 1020 + 2, 2 * 1020 + 6, NONE
    assert r["labels"].tolist() == [[n] * 9, [n, a, a, a, n, b, b, b, n], [n, a, a, a, n, b, b, b, n], [n, a, a, a, n, b, b, b, n], [n] * 9]
    assert r["depth"][1:4, 1:4].tolist() == [[7, 5, 7], [5, 0, 5], [7, 5, 7]]
    m.close()
    m = _map(1028, 1028)
    m.upload_log(_lattice(1028))
    with pytest.raises(GmsError) as e:
        m.rooms(core=1, inflate=0, not_free=False)
    assert e.value.code == GMS_ERR_INVALID and "66049" in str(e.value), "257 x 257 rooms are named in the message"
    r = m.rooms(core=1, inflate=0, not_free=False, min_core=2, labels=False)
    assert r["n_rooms"] == 2 * 256 + 1, "a valid request on the same handle: the cores that reach the far edges have 2 cells, the corner's 4"
    r = m.rooms(core=1, inflate=0, not_free=False, min_core=5)
    assert r["n_rooms"] == 0 and (r["labels"] == NONE).all()
    m.upload_log(rx.two_boxes(1028, 1028, 500, 700))                            # ... and another map: the hand-derived numbers
    r = m.rooms(**BOX)
    assert r["rooms"]["count"].tolist() == [403, 400] and r["rooms"]["core_count"].tolist() == [260, 260] and r["n_doors"] == 1
    assert (r["doors"]["a"][0], r["doors"]["b"][0], r["doors"]["count"][0]) == (704 * 1028 + 504, 704 * 1028 + 525, 3)
    assert (r["doors"]["sum_x2"][0], r["doors"]["sum_y2"][0]) == (135 + 6 * 500, 66 + 6 * 700) and (r["labels"] != NONE).sum() == 803
    m.close()


# ---- 7: random floors -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,not_free,inflate,core,min_core", [(1, False, 0, 2, 1), (2, True, 1, 3, 1), (3, False, 2, 6, 10), (1, True, 0, 4, 30),
                                                                 (2, True, 3, 8, 1), (3, True, 1, 3, 1)])
def test_random_floors(seed, not_free, inflate, core, min_core):
    m = _map()
    e = _check(m, rx.random_floor(seed), f"floor {seed}", core=core, inflate=inflate, not_free=not_free, min_core=min_core)
    assert e["n_rooms"] >= 3 and e["n_doors"] >= 2
    m.close()


# ---- 8: rectangles, handles, forms ---------------------------------------------------------------------------------------------------------
def test_rectangles_and_map_2_of_3():
    logs = np.stack([rx.random_floor(4), rx.two_boxes(W, H, 41, 53), rx.random_floor(5)])
    m = _map(n_maps=3)
    m.upload_log(logs)
    kw = dict(core=3, inflate=1, not_free=True)
    for rect in ((77, 66, 1, 1), (40, 63, 100, 1), (150, 100, 50, 36), (0, 0, W, H)):
        _check(m, logs[2], f"map 2, rect {rect}", upload=False, mi=2, rect=rect, **kw)
    _check(m, logs[0], "map 0", upload=False, mi=0, **kw)
    _check(m, logs[1], "map 1", upload=False, mi=1, **BOX)
    for bad in (dict(mi=3), dict(rect=(0, 0, W + 1, H)), dict(rect=(190, 130, 11, 6)), dict(core=1, inflate=1), dict(max_cost=0)):
        with pytest.raises(GmsError) as e:
            m.rooms(**{**kw, **bad})
        assert e.value.code == GMS_ERR_INVALID, bad
    m.close()


POSE = np.array([5.0, 3.4, 0.0], dtype=np.float32)     # cell (100, 68)


def _fan(a0, a1, n, d):
    ang = np.linspace(a0, a1, n)
    return Observation.from_polar(ang, np.full(n, d), np.ones(n, dtype=bool))


FRONT, BACK, LEFT = _fan(-1.0, 1.0, 64, 1.5), _fan(math.pi - 1.0, math.pi + 1.0, 64, 1.1), _fan(0.6, 2.4, 48, 0.8)


def test_a_call_sees_what_a_download_sees():
    m = _map()
    kw = dict(core=3, inflate=1, not_free=True, min_core=4)
    m.integrate_observation(FRONT, POSE)
    first = _check(m, m.download_log(), "after integrate_observation", upload=False, **kw)
    assert first["n_rooms"] >= 1
    m.update(BACK, POSE); m.update(BACK, POSE)
    m.update(LEFT, POSE)                               # the steady state of update(): this scan's apply pass is still owed
    then = _check(m, m.download_log(), "after update() with its apply pass deferred", upload=False, **kw)
    assert then["n_rooms"] >= 1 and (then["labels"] != first["labels"]).any(), "the later scans changed the answer"
    m.close()


def _flat(x):
    """the arrays of a nest of tuples, in order"""
    return [a for y in x for a in _flat(y)] if isinstance(x, tuple) else [np.asarray(x)]


def test_a_call_changes_no_later_result():
    m = _map()
    m.upload_log(rx.random_floor(2))
    seeds = [(30, 30), (150, 100)]

    def others():
        return (m.reach(seeds, inflate=3), m.reach(seeds, inflate=0, not_free=False), m.frontiers(labels=True, inflate=2), m.clearance(max_radius=20),
                m.skeleton(max_radius=12), m.download_log())

    before = others()
    m.rooms(core=8, inflate=3, not_free=True)
    m.rooms(core=2, inflate=0, not_free=False)
    after = others()
    m.rooms(core=4, inflate=3, not_free=True)
    third = m.reach(seeds, inflate=3)                                           # (the scratch plane this call also uses)
    assert np.array_equal(third, before[0])
    for a, b in zip(_flat(before), _flat(after)):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    m.close()


def test_device_form_on_a_stream_of_the_callers():
    import torch
    m = _map()
    log = rx.random_floor(3)
    m.upload_log(log)
    kw = dict(core=3, inflate=1, not_free=True)
    rect = (13, 7, 150, 101)
    host = m.rooms(rect=rect, depth=True, cap_rooms=64, cap_doors=64, **kw)
    n = host["labels"].size
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        lab = torch.full((n + 40,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        dep = torch.full((n + 40,), 0x5A5A, dtype=torch.int16, device="cuda")
        rooms = torch.full((64 * 7 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        doors = torch.full((64 * 6 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        stream.synchronize()
        for bad in (dict(labels=lab.view(torch.uint8)[2:]), dict(depth=dep.view(torch.uint8)[1:]), dict(rooms=rooms.view(torch.uint8)[4:]),
                    dict(doors=doors.view(torch.uint8)[4:])):
            with pytest.raises(GmsError) as e:
                m.rooms_dev(rect=rect, **kw, **bad)
            assert e.value.code == GMS_ERR_INVALID, "a misaligned output is refused"
        nr, nd = m.rooms_dev(lab, dep, rooms[:64 * 7], doors[:64 * 6], rect=rect, **kw)
        stream.synchronize()
    assert (nr, nd) == (host["n_rooms"], host["n_doors"]) and 3 <= nr <= 64 and 2 <= nd <= 64
    raw_lab, raw_dep = lab.cpu().numpy().view(np.uint32), dep.cpu().numpy().view(np.uint16)
    assert np.array_equal(raw_lab[:n].reshape(host["labels"].shape), host["labels"]) and (raw_lab[n:] == 0x5A5A5A5A).all()
    assert np.array_equal(raw_dep[:n].reshape(host["depth"].shape), host["depth"]) and (raw_dep[n:] == 0x5A5A).all()
    raw_rooms, raw_doors = rooms.cpu().numpy(), doors.cpu().numpy()
    assert np.array_equal(raw_rooms[:7 * nr].view(_lib.ROOM_DTYPE), host["rooms"]) and (raw_rooms[7 * nr:] == 0x5A5A5A5A5A5A5A5A).all()
    assert np.array_equal(raw_doors[:6 * nd].view(_lib.DOOR_DTYPE), host["doors"]) and (raw_doors[6 * nd:] == 0x5A5A5A5A5A5A5A5A).all()
    rx.same(host, rx.expect(log, rect=rect, **kw), "the host form")
    m.close()
