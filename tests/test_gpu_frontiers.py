"""Frontier regions of the shared maps on the device (include/gridmapslam.h "frontier regions"): gms_map_frontiers[_dev] against the
flood-fill expectation of tests/_frontier_expect.py on logData that was constructed or downloaded.  Every comparison is array_equal:
the feature is all-integer and every output is unique.  A request must see the map as a download would return it at that moment and
must change no later result of its handle.

The map is 200 x 136 cells: 4 x 3 tiles of 64 x 64 cells, ragged on both far edges (8 columns, 8 rows).  That is 544 plane words: the
scan of the root plane stays inside one block of GMS_SCAN words here.  tests/test_gpu_scan_levels.py runs the regions on maps of more
than one scan block."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import _frontier_expect as fx
from gridmap_slam_robot_amd import GridMap, Observation, ParticleFilter, _lib, frontier_centroids
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_OK, GmsError, GmsFrontiers

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
FAR, NONE = 0xFFFF, 0xFFFFFFFF
CAP = 8192


def _map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=128, **kw)
    assert (m.W, m.H) == (W, H)
    return m


def _same(got, want, where):
    """(records, n_found, labels) against the expectation's"""
    assert got[1] == want[1], f"{where}: n_found {got[1]} != {want[1]}"
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape, where
    bad = np.nonzero(got[0] != want[0])[0]
    assert np.array_equal(got[0], want[0]), f"{where}: {len(bad)} of {len(want[0])} records differ, first {bad[0]}: {got[0][bad[0]]} != {want[0][bad[0]]}"
    assert got[2].dtype == np.uint32 and got[2].shape == want[2].shape, where
    bad = np.argwhere(got[2] != want[2])
    assert np.array_equal(got[2], want[2]), (f"{where}: {len(bad)} of {want[2].size} labels differ, first at (y, x) = {bad[0].tolist()}: "
                                             f"{got[2][tuple(bad[0])]} != {want[2][tuple(bad[0])]}")


def _check(m, log, where, upload=True, **kw):
    if upload:
        m.upload_log(log)
    want = fx.expect(log, **kw)
    _same(m.frontiers(labels=True, cap=CAP, **kw), want, where)
    return want


def _unknown():
    return np.zeros((H, W))


def _free():
    return np.full((H, W), L_FREE)


def _carve(points, log=None):
    """a one-cell-wide free corridor along the axis-parallel polyline through points, in never-observed space: every cell a frontier cell"""
    log = _unknown() if log is None else log
    for (xa, ya), (xb, yb) in zip(points, points[1:]):
        assert xa == xb or ya == yb
        log[min(ya, yb):max(ya, yb) + 1, min(xa, xb):max(xa, xb) + 1] = L_FREE
    return log


def _cells(log, cells):
    for x, y in cells:
        log[y, x] = L_FREE
    return log


# ---- 1: empty results ----------------------------------------------------------------------------------------------------------------
def test_fresh_and_all_free_maps_have_no_region():
    m = _map()
    for log, name in ((None, "a fresh map"), (_free(), "an all-free map")):
        if log is not None:
            m.upload_log(log)
        rec, n, lab = m.frontiers(labels=True)
        assert n == 0 and len(rec) == 0 and lab.shape == (H, W) and (lab == NONE).all(), name
    m.close()


# ---- 2: hand-derived shapes ----------------------------------------------------------------------------------------------------------
def test_ring_and_edge_flush_rectangle():
    m = _map()
    a, b = 70, 20                                                              # across the border x = 64
    log = _unknown()
    log[50:50 + b, 30:30 + a] = L_FREE
    rec = _check(m, log, "a free rectangle in unknown space")[0]
    assert len(rec) == 1 and rec["count"][0] == 2 * (a + b) - 4 and (rec["anchor_x"][0], rec["anchor_y"][0]) == (30, 50)
    assert frontier_centroids(rec).tolist() == [[30 + (a - 1) / 2, 50 + (b - 1) / 2]]
    log = _unknown()
    log[50:50 + b, 0:a] = L_FREE
    rec = _check(m, log, "flush with x = 0")[0]
    assert rec["count"].tolist() == [2 * (a + b) - 4 - (b - 2)], "the map's border makes no frontier"
    log = _unknown()
    log[H - b:, W - a:] = L_FREE
    rec = _check(m, log, "in the far corner")[0]
    assert rec["count"].tolist() == [a + b - 1] and (rec["anchor_x"][0], rec["anchor_y"][0]) == (W - a, H - b)
    m.close()


def test_four_neighbour_rule_and_diagonal_contact():
    m = _map()
    log = _free()
    log[70, 100] = 0.0
    rec, _, lab = _check(m, log, "one unknown cell in free space")
    assert rec["count"].tolist() == [4] and sorted(map(tuple, np.argwhere(lab != NONE).tolist())) == [(69, 100), (70, 99), (70, 101), (71, 100)]
    log[70, 100] = L_OCC
    assert _check(m, log, "an occupied cell next to free cells")[1] == 0
    two = _cells(_unknown(), [(20, 20), (21, 21), (40, 20), (42, 20), (60, 20), (61, 19)])
    rec = _check(m, two, "single cells touching diagonally, and one cell apart")[0]
    assert rec["count"].tolist() == [2, 2, 1, 1] and rec["anchor_x"].tolist() == [61, 20, 40, 42], "one cell apart: two regions"
    m.close()


# ---- 3: tile borders and long chains -----------------------------------------------------------------------------------------------------
def test_pairs_across_tile_borders():
    m = _map()
    pairs = [[(63, 10), (64, 10)], [(10, 63), (10, 64)], [(127, 63), (128, 64)], [(64, 127), (63, 128)], [(127, 20), (128, 21)], [(128, 30), (127, 31)],
             [(30, 127), (31, 128)], [(41, 127), (40, 128)], [(191, 63), (192, 64)], [(199, 127), (198, 128)]]
    log = _cells(_unknown(), [c for p in pairs for c in p])
    rec = _check(m, log, "pairs straddling x = 63|64, y = 63|64, corners on both diagonals")[0]
    assert len(rec) == len(pairs) and (rec["count"] == 2).all()
    quad = _cells(_unknown(), [(63, 63), (64, 64), (64, 63), (63, 64)])
    assert _check(m, quad, "four tiles meet")[0]["count"].tolist() == [4]
    for a, b in ([(63, 63), (64, 64)], [(64, 63), (63, 64)]):
        rec = _check(m, _cells(_unknown(), [a, b]), f"{a} - {b} alone")[0]
        assert rec["count"].tolist() == [2] and (rec["anchor_x"][0], rec["anchor_y"][0]) == min(a, b, key=lambda c: (c[1], c[0]))
    m.close()


def test_snake_through_all_twelve_tiles():
    pts = [(195, 3), (195, 20), (5, 20), (5, 90), (195, 90), (195, 132), (5, 132)]         # the anchor ends a spur in the LAST tile of row 0
    log = _carve(pts)
    m = _map()
    rec, _, lab = _check(m, log, "a snake")
    assert rec["count"].tolist() == [(log < 0).sum()] and (rec["anchor_x"][0], rec["anchor_y"][0]) == (195, 3)
    tiles = {(int(x) // 64, int(y) // 64) for y, x in np.argwhere(lab != NONE)}
    assert len(tiles) == 12
    m.close()


def test_spiral_inside_one_tile_and_comb_across_a_border():
    pts, lo, hi = [(1, 1)], 1, 61
    while hi - lo >= 4:
        pts += [(hi, lo), (hi, hi), (lo, hi), (lo, lo + 2), (lo + 2, lo + 2)]
        lo, hi = lo + 2, hi - 2
    log = _carve(pts)
    assert (log < 0).sum() > 1500 and (log[:, 63:] == 0).all() and (log[63:, :] == 0).all()
    m = _map()
    assert _check(m, log, "a spiral")[0]["count"].tolist() == [(log < 0).sum()]
    comb = _unknown()
    comb[2:61, 70] = L_FREE                                                    # the spine is right of the border, the teeth reach left across it
    for y in range(2, 61, 2):
        comb[y, 58:71] = L_FREE
    rec = _check(m, comb, "a comb across x = 64")[0]
    assert rec["count"].tolist() == [(comb < 0).sum()] and (rec["anchor_x"][0], rec["anchor_y"][0]) == (58, 2)
    comb[2:61, 70] = 0.0                                                       # without the spine: thirty teeth
    for y in range(2, 61, 2):
        comb[y, 70] = L_FREE
    assert len(_check(m, comb, "the teeth alone")[0]) == 30
    m.close()


# ---- 4: many regions, cap and min_size ---------------------------------------------------------------------------------------------------
def test_many_regions_cap_and_min_size():
    log = _unknown()
    log[0::2, 0::2] = L_FREE
    m = _map()
    want = _check(m, log, "isolated cells at every (even, even)")
    assert want[1] == 6800 and (want[0]["count"] == 1).all()
    rec, n = m.frontiers(cap=100)
    assert n == 6800 and np.array_equal(rec, want[0][:100]), "the first cap in anchor order, n_found whole"
    rec, n = m.frontiers(cap=0)
    assert n == 6800 and len(rec) == 0
    cnt, guard = C.c_int32(-1), np.full(4, 7, np.int64)
    f = GmsFrontiers(0, 0, W, H, 1, 0, 0, 0)
    assert _lib.load().gms_map_frontiers(m._h, 0, C.byref(f), None, None, None, 0, C.byref(cnt)) == GMS_OK and cnt.value == 6800
    assert _lib.load().gms_map_frontiers(m._h, 0, C.byref(f), None, None, None, 3, C.byref(cnt)) == GMS_ERR_INVALID, "cap > 0 needs records"
    assert _lib.load().gms_map_frontiers(m._h, 0, C.byref(f), None, None, guard.ctypes.data, -1, C.byref(cnt)) == GMS_ERR_INVALID and (guard == 7).all()
    log = _unknown()
    log[10:17, 10:18] = L_FREE                                                 # a ring of 26
    log[40, 40] = log[40, 42] = log[41, 41] = L_FREE                           # 3
    log[100, 150] = L_FREE                                                     # 1
    m.upload_log(log)
    for min_size, counts in ((1, [26, 3, 1]), (2, [26, 3]), (3, [26, 3]), (4, [26]), (25, [26]), (26, [26]), (27, [])):
        want = _check(m, log, f"min_size = {min_size}", upload=False, min_size=min_size)
        assert want[0]["count"].tolist() == counts
        assert (want[2] != NONE).sum() == 30, "every frontier cell is labelled, whatever min_size is"
    m.close()


# ---- 5: cell classes ------------------------------------------------------------------------------------------------------------------
def test_cell_classes_on_special_values():
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0])
    unknown = [True, True, True, False, False, False, False, False, False]
    log = np.full((H, W), -1.0)
    log[3, 10:100:10] = vals                                                   # one of each in free space
    m = _map()
    m.upload_log(log)
    assert np.array_equal(m.download_log(), log, equal_nan=True)
    want = _check(m, log, "one of each value", upload=False)
    assert [bool(want[2][2, x] != NONE) for x in range(10, 100, 10)] == unknown, "the free cell above each: a frontier cell iff the value is UNKNOWN"
    assert want[0]["count"].tolist() == [4, 4, 4]
    rng = np.random.default_rng(9)
    log = np.where(rng.random((H, W)) < 0.1, rng.choice(vals, size=(H, W)), -1.0)
    log[H - 1, W - 9:] = vals
    for inflate in (0, 2):
        assert _check(m, log, f"special values at random, inflate = {inflate}", inflate=inflate)[1] > 50
    m.close()


# ---- 6: inflation ----------------------------------------------------------------------------------------------------------------------
def test_inflation_cuts_a_region_and_removes_one():
    log = _unknown()
    log[50, 20:121] = L_FREE                                                   # a corridor of 101 cells
    log[52, 70] = L_OCC                                                        # two cells below it
    log[100, 150] = L_FREE
    log[103, 150] = L_OCC
    log[130, 5] = L_FREE                                                       # farther than 64 from both
    m = _map()
    m.upload_log(log)
    counts = {0: [101, 1, 1], 1: [101, 1, 1], 3: [48, 48, 1], 64: [1]}
    for inflate, cnt in counts.items():
        want = _check(m, log, f"inflate = {inflate}", upload=False, inflate=inflate)
        assert want[0]["count"].tolist() == cnt, inflate
    with pytest.raises(GmsError):
        m.frontiers(inflate=256)
    m.close()


# ---- 7: the cost field and the goal ------------------------------------------------------------------------------------------------------
def test_goal_from_reach_and_hand_made_costs():
    log = _unknown()
    log[20:60, 30:120] = L_FREE                                                # a room around the seed
    log[35:45, 70] = L_OCC
    log[100:110, 150:170] = L_FREE                                             # another that no path leads to
    m = _map()
    m.upload_log(log)
    cost = m.reach([(40, 30)])
    assert cost.shape == (H, W) and cost[100, 150] == FAR and cost[20, 30] != FAR
    want = fx.expect(log, cost=cost)
    _same(m.frontiers(cost=cost, labels=True), want, "cost from reach()")
    assert want[0]["goal_cost"].tolist() == [int(cost[20:60, 30:120][(want[2] != NONE)[20:60, 30:120]].min()), FAR]
    assert (want[0]["goal_x"][1], want[0]["goal_y"][1]) == (-1, -1), "every member FAR"
    hand = np.full((H, W), FAR, np.uint16)
    hand[59, 100] = hand[20, 119] = hand[30, 30] = 35                          # ties: the smallest linear index wins
    hand[40, 50] = 0                                                           # (not a member)
    hand[109, 169] = hand[109, 150] = 0xFFFE
    want = fx.expect(log, cost=hand)
    assert [(int(r["goal_x"]), int(r["goal_y"]), int(r["goal_cost"])) for r in want[0]] == [(119, 20, 35), (150, 109, 0xFFFE)]
    _same(m.frontiers(cost=hand, labels=True), want, "a hand-made cost field")
    _same(m.frontiers(labels=True), fx.expect(log), "... and none")
    with pytest.raises(ValueError):
        m.frontiers(cost=hand[:-1])
    m.close()


# ---- 8: label rectangles -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_log():
    rng = np.random.default_rng(20250211)
    log = np.where(rng.random((H, W)) < 0.01, L_OCC, L_FREE)
    for _ in range(60):                                                        # unknown islands
        x, y, w, h = rng.integers(0, W), rng.integers(0, H), rng.integers(1, 14), rng.integers(1, 10)
        log[y:y + h, x:x + w] = rng.choice([0.0, -0.0, np.nan])
    for _ in range(25):                                                        # free blobs inside them
        x, y, w, h = rng.integers(0, W), rng.integers(0, H), rng.integers(1, 6), rng.integers(1, 5)
        log[y:y + h, x:x + w] = L_FREE
    log[70, 96] = L_FREE
    log.flags.writeable = False
    return log


def test_label_rectangles():
    log = np.array(_random_log())
    whole = fx.expect(log)
    m = _map()
    m.upload_log(log)
    rects = {"1 x 1": (150, 41, 1, 1), "left edge": (0, 20, 33, 50), "right edge": (W - 9, 0, 9, H), "top edge": (10, 0, 150, 3),
             "bottom edge": (31, H - 65, 66, 65), "one column": (64, 0, 1, H)}
    fy, fx_ = np.argwhere(whole[2] != NONE)[7]
    rects["1 x 1 on a frontier cell"] = (int(fx_), int(fy), 1, 1)
    for name, r in rects.items():
        rec, n, lab = m.frontiers(rect=r, labels=True, cap=CAP)
        assert n == whole[1] and np.array_equal(rec, whole[0]), "the regions are the whole map's, whatever the rectangle"
        assert np.array_equal(lab, whole[2][r[1]:r[1] + r[3], r[0]:r[0] + r[2]]), name
    for r in ((0, 0, W + 1, H), (0, 0, W, H + 1), (W, 0, 1, 1), (0, H, 1, 1), (190, 130, 11, 6), (190, 130, 10, 7), (-1, 0, 5, 5), (0, 0, 0, 5)):
        lab = np.full((max(r[3], 1) + 1, max(r[2], 1) + 1), 7, dtype=np.uint32)
        rec = np.zeros(4, _lib.FRONTIER_DTYPE)
        n = C.c_int32(-7)
        f = GmsFrontiers(*r, 1, 0, 0, 0)
        assert _lib.load().gms_map_frontiers(m._h, 0, C.byref(f), None, lab.ctypes.data, rec.ctypes.data, 4, C.byref(n)) == GMS_ERR_INVALID, r
        assert (lab == 7).all() and n.value == -7 and (rec["count"] == 0).all(), "a refused rectangle writes nothing"
    m.close()


# ---- 9: randomised -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate,min_size", [(0, 1), (2, 1), (0, 3)])
def test_random_map(inflate, min_size):
    log = np.array(_random_log())
    m = _map()
    m.upload_log(log)
    cost = m.reach([(96, 70)], inflate=inflate, not_free=False)
    want = fx.expect(log, min_size=min_size, inflate=inflate, cost=cost)
    assert want[1] >= 10 and (want[0]["goal_cost"] != FAR).any()
    _same(m.frontiers(min_size=min_size, inflate=inflate, cost=cost, labels=True, cap=CAP), want, f"inflate = {inflate}, min_size = {min_size}")
    m.close()


# ---- 10: other handles and forms ---------------------------------------------------------------------------------------------------------
def test_map_2_of_a_batched_handle():
    logs = np.stack([_free(), np.array(_random_log()[::-1]), np.array(_random_log()[:, ::-1])])
    logs[0][40, 40] = 0.0
    m = _map(n_maps=3)
    m.upload_log(logs)
    for mi in (2, 0, 1):
        for inflate in (0, 2):
            _same(m.frontiers(inflate=inflate, labels=True, cap=CAP, mi=mi), fx.expect(logs[mi], inflate=inflate), f"map {mi}, inflate = {inflate}")
    with pytest.raises(GmsError):
        m.frontiers(mi=3)
    m.close()


def test_device_form_on_a_stream_of_the_callers():
    import torch
    log = np.array(_random_log())
    m = _map()
    m.upload_log(log)
    rect = (13, 7, 150, 101)
    cost = m.reach([(96, 70)], not_free=False)
    host = m.frontiers(cost=cost, rect=rect, labels=True, cap=CAP)
    _same(host, fx.expect(log, cost=cost, rect=rect), "host form")
    cap, nlab = 8, rect[2] * rect[3]
    assert host[1] > cap
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        lab = torch.full((nlab + 40,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        rec = torch.full((56 * cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        d_cost = torch.from_numpy(cost.view(np.int16)).to("cuda")
        odd = torch.zeros((W * H + 8,), dtype=torch.int16, device="cuda").view(torch.uint8)[1:]
        stream.synchronize()
        for bad in ({"labels": lab.view(torch.uint8)[2:]}, {"records": rec[4:]}, {"cost": odd}):
            kw = dict({"records": rec[8:8 + 56 * cap], "labels": lab[20:], "cost": d_cost}, **bad)
            with pytest.raises(GmsError) as e:
                m.frontiers_dev(rect=rect, **kw)
            assert e.value.code == GMS_ERR_INVALID
        stream.synchronize()
        assert (lab.cpu().numpy() == 0x5A5A5A5A).all() and (rec.cpu().numpy() == 0x5A).all(), "a misaligned pointer is refused untouched"
        n = m.frontiers_dev(records=rec[8:8 + 56 * cap], labels=lab[20:20 + nlab], cost=d_cost, rect=rect)
        assert n == host[1], "n_found is complete when the call returns"
        assert m.frontiers_dev(rect=rect) == host[1], "both outputs omitted"
        stream.synchronize()
    raw_l, raw_r = lab.cpu().numpy().view(np.uint32), rec.cpu().numpy()
    assert np.array_equal(raw_l[20:20 + nlab].reshape(host[2].shape), host[2]) and (raw_l[:20] == 0x5A5A5A5A).all() and (raw_l[20 + nlab:] == 0x5A5A5A5A).all()
    assert np.array_equal(raw_r[8:8 + 56 * cap].view(_lib.FRONTIER_DTYPE), host[0][:cap]), "the first cap records"
    assert (raw_r[:8] == 0x5A).all() and (raw_r[8 + 56 * cap:] == 0x5A).all(), "guard bytes around the records"
    m.set_stream(None)
    _same(m.frontiers(cost=cost, rect=rect, labels=True, cap=CAP), host, "back on the handle's own stream")
    m.close()


# ---- 11: state ---------------------------------------------------------------------------------------------------------------------------
POSE = np.array([5.0, 3.4, 0.0], dtype=np.float32)     # cell (100, 68)


def _fan(a0, a1, n, d):
    ang = np.linspace(a0, a1, n)
    return Observation.from_polar(ang, np.full(n, d), np.ones(n, dtype=bool))


FRONT, BACK, LEFT = _fan(-1.0, 1.0, 64, 1.5), _fan(math.pi - 1.0, math.pi + 1.0, 64, 1.1), _fan(0.6, 2.4, 48, 0.8)


def _check_against_download(m, where):
    got = [m.frontiers(labels=True, cap=CAP), m.frontiers(inflate=2, min_size=2, labels=True, cap=CAP)]
    log = m.download_log()
    _same(got[0], fx.expect(log), where)
    _same(got[1], fx.expect(log, inflate=2, min_size=2), where + ": inflate = 2, min_size = 2")
    return got[0]


def test_a_request_sees_what_a_download_sees():
    m = _map()
    m.integrate_observation(FRONT, POSE)
    a = _check_against_download(m, "after integrate_observation")
    assert a[1] >= 1 and (a[2] != NONE).sum() > 20, "the fan's sides border never-observed space"
    m.update(BACK, POSE); m.update(BACK, POSE)
    m.update(LEFT, POSE)                               # the steady state of update(): this scan's apply pass is still owed
    b = _check_against_download(m, "after update() with its apply pass deferred")
    assert not np.array_equal(a[2], b[2])
    hole = _free()
    hole[20:30, 150:160] = 0.0
    m.upload_log(hole)
    c = _check_against_download(m, "after upload_log")
    assert c[0]["count"].tolist() == [40]
    m.reset()
    assert _check_against_download(m, "after reset")[1] == 0
    m.close()


def test_a_request_shares_the_casts_plane():
    from _cast_expect import probes_from
    log = _random_log()
    m = _map()
    m.upload_log(log)
    probes = probes_from([1.0, 0.0, -1.0], [0.0, 1.0, 0.5])
    first = m.cast(POSE, probes)
    assert m.cast_plane_builds() == 1
    want = fx.expect(log)
    _same(m.frontiers(labels=True, cap=CAP), want, "between two casts")
    assert m.cast_plane_builds() == 1, "the request reads the plane the cast packed"
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 1, "cast, frontiers, cast: one pre-pass"
    m.upload_log(log)
    _same(m.frontiers(labels=True, cap=CAP), want, "the request packs the plane itself")
    assert m.cast_plane_builds() == 2
    _same(m.frontiers(labels=True, cap=CAP, inflate=1), fx.expect(log, inflate=1), "a second request")
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 2, "a cast after a request packs none"
    m.close()


def test_a_request_changes_no_later_result():
    """twins through the same calls, one of them asked for regions between every two steps: logData, the likelihood field, a cost-to-go
    field and one fused scan step end bit-identical"""
    N = 64
    rng = np.random.default_rng(77)
    P = (POSE + rng.normal(0, [0.03, 0.03, 0.02], (N, 3))).astype(np.float32)
    results = []
    for ask in (False, True):
        m = _map()
        ask_now = lambda: (m.frontiers(labels=True), m.frontiers(inflate=3, min_size=2, cost=m.reach([(100, 68)]))) if ask else None
        m.update(BACK, POSE); ask_now()
        m.update(LEFT, POSE); ask_now()                # (with the apply pass owed)
        pf = ParticleFilter(m, N)
        ask_now()
        pf.slam_update(P, FRONT, 0.41, 0.9, True)
        ask_now()
        log, lik = m.download_log(), m.download_likelihood()
        ask_now()
        results.append((log, lik, pf.get_poses(), pf.get_weights(), m.download_log(), pf.last_step()["strongest_pose"],
                        m.reach([(100, 68)], inflate=2), m.clearance(max_radius=9)))
        pf.close(); m.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b, equal_nan=True)
    assert (results[0][0] > 0).any()
