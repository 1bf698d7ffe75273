"""The map queries on maps at the plane-word and tile edges: clearance fields, cost-to-go fields, rooms and doors, frontier regions, view
gain and the beam sensor model of the shared maps, each against its plain expectation (tests/_clearance_expect.py, _reach_expect.py,
_rooms_expect.py, _frontier_expect.py, _gain_expect.py, _beams_expect.py), on thirteen shapes -- the smallest on each side of each edge of the units'
arithmetic: one cell, one 32-bit plane word, one 64-bit plane word / one 64 x 64 tile, two tiles, and one cell past each.  The other
device tests of these units all run on 200 x 136 cells.

Every comparison is array_equal (the doubles of the beam model as uint64 views): the units are integer, or bit-exact by their
stated summation order.  Per shape three logs, seeded by W * 1000 + H (and SEED_TURN): all free and all unknown (what the planes' padding must not
change), and a random one: 12 % occupied, 10 % unknown drawn from {0.0, -0.0, NaN}, the rest free, cell (0, 0) free."""
import functools
import math
import os

import numpy as np
import pytest

import _beams_expect as bx
import _clearance_expect as xe
import _frontier_expect as fx
import _gain_expect as gx
import _reach_expect as rx
import _rooms_expect as ro
import test_gpu_frontiers as tf
from gridmap_slam_robot_amd import GAIN_DTYPE, GridMap, ParticleFilter, beam_model_factors, probe_fan
from gridmap_slam_robot_amd._lib import BEAM_DTYPE
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
SHAPES = [(1, 1), (1, 70), (70, 1), (31, 3), (32, 32), (33, 2), (63, 65), (64, 64), (65, 64), (64, 65), (128, 128), (129, 65), (192, 7)]
BORDERED = [(63, 65), (65, 64), (64, 65), (128, 128), (129, 65)]           # the shapes with a 64-cell border inside the map
LOGS = ("free", "unknown", "random")
RADII = (1, 9, 255)
RANGES = (1, 40, 255)
WINDOWS = ((0, 0), (3, 2), (255, 255))                                   # (behind, ahead) of the beam model
T = 64                                                                     # the tile edge of gms_reach.hip and gms_frontier.hip
FAR, NONE = 0xFFFF, 0xFFFFFFFF
# The random log of a shape is seeded by W * 1000 + H + 1000000 * turn, turn being the first at which the seed cell (0, 0) reaches 95 %
# of the traversable cells under BOTH predicates (test_the_expectations_contain_what_they_are_meant_to): with the unknown cells
# blocked as well, 22 % of the cells, turn 0 walls the seed in on 128 x 128 and cuts the seven rows of 192 x 7.
SEED_TURN = {(128, 128): 1, (192, 7): 7}
# ... and the second log by W * 1000 + H + 500000 + 1000000 * turn: on 129 x 65 the first turn that occupies cell (128, 64), the only cell
# of the last, ragged word of a sixteen-cell grouping of the map (tests/test_slam_query_inputs.py)
SECOND_TURN = {(129, 65): 4}
CAP = 8192
N_BEAMS, N_PARTICLES = 48, 65

shapes = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")


# ---- maps and logs --------------------------------------------------------------------------------------------------------------------
def _size(shape):
    return (shape[0] - 0.4) * RES, (shape[1] - 0.4) * RES


def _map(shape, **kw):
    m = GridMap(*_size(shape), RES, (0.0, 0.0), **kw)
    assert (m.W, m.H) == shape
    return m


@functools.lru_cache(maxsize=None)
def _grid(shape):
    g = orc.Grid(*_size(shape), RES, 0.0, 0.0)
    assert (g.W, g.H) == shape
    return g


def _random_log(shape, seed):
    W, H = shape
    rng = np.random.default_rng(seed)
    u = rng.random((H, W))
    log = np.where(u < 0.12, L_OCC, np.where(u < 0.22, rng.choice([0.0, -0.0, np.nan], size=(H, W)), L_FREE))
    log[0, 0] = L_FREE
    return log


@functools.lru_cache(maxsize=None)
def log_of(shape, name):
    W, H = shape
    if name == "free":
        log = np.full((H, W), L_FREE)
    elif name == "unknown":
        log = np.zeros((H, W))
    elif name == "random":
        log = _random_log(shape, W * 1000 + H + 1000000 * SEED_TURN.get(shape, 0))
    elif name == "second":                                                 # another random log, for the handle that is reused
        log = _random_log(shape, W * 1000 + H + 500000 + 1000000 * SECOND_TURN.get(shape, 0))
    else:                                                                  # "last column": column W - 1 never observed, the rest free
        log = np.full((H, W), L_FREE)
        log[:, W - 1] = 0.0
    log.flags.writeable = False
    return log


def _same(got, want, where):
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{where}: {len(bad)} of {want.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _with_env(name, mem, make):
    old = os.environ.pop(name, None)
    if mem:
        os.environ[name] = "mem"                                           # read when the handle is created
    try:
        return make()
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


# ---- 1: clearance -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clearance_of(shape, name, R, not_free):
    """the two constant logs need no search: a map without an obstacle is all FAR, a map of nothing but obstacles all 0"""
    W, H = shape
    if name == "free" or (name == "unknown" and not not_free):
        f = np.full((H, W), xe.FAR, dtype=np.uint16)
    elif name == "unknown":
        f = np.zeros((H, W), dtype=np.uint16)
    else:
        f = xe.expect(log_of(shape, name), R, not_free)
    f.flags.writeable = False
    return f


def _odd_rect(shape):
    """from an odd column (column 0 where the map has one column) to the last column, the lower half of the rows"""
    W, H = shape
    x0 = ((W - 1) // 2) | 1
    if x0 > W - 1:
        x0 = W - 1
    return (x0, H // 2, W - x0, H - H // 2)


@functools.lru_cache(maxsize=None)
def clearance_poses_of(shape):
    """the centres of the four corner cells, then 60 poses of which about one in ten lies just off the map"""
    W, H = shape
    rng = np.random.default_rng(W * 1000 + H + 1)
    corners = [((x + 0.5) * RES, (y + 0.5) * RES, 0.0) for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))]
    p = np.column_stack([rng.uniform(0.0, W * RES, 60), rng.uniform(0.0, H * RES, 60), rng.uniform(-3.0, 3.0, 60)])
    off = np.flatnonzero(rng.random(60) < 0.1)
    off = np.union1d(off, [7, 23, 41, 59])                                 # ... at the least one beyond each side
    side = np.arange(len(off)) % 4
    p[off[side == 0], 0] = -0.06                                           # (-0.01 would still be cell 0: the cast truncates toward zero)
    p[off[side == 1], 0] = W * RES + 0.01
    p[off[side == 2], 1] = -0.06
    p[off[side == 3], 1] = H * RES + 0.01
    poses = np.array(corners + p.tolist(), dtype=np.float32)
    poses.flags.writeable = False
    return poses


@shapes
def test_clearance(shape):
    W, H = shape
    m = _map(shape)
    rect = _odd_rect(shape)
    poses = clearance_poses_of(shape)
    for name in LOGS:
        m.upload_log(log_of(shape, name))
        for not_free in (False, True):
            for R in RADII:
                where = f"{shape}, {name}, not_free = {not_free}, R = {R}"
                want = clearance_of(shape, name, R, not_free)
                got = m.clearance(max_radius=R, not_free=not_free)
                if name == "free":
                    assert (got == xe.FAR).all(), where + ": the planes' padding is no obstacle"
                if name == "unknown":
                    assert (got == (0 if not_free else xe.FAR)).all(), where
                _same(got, want, where)
                _same(m.clearance(rect=rect, max_radius=R, not_free=not_free), want[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]], where + f", {rect}")
                _same(m.clearance_poses(poses, R, not_free), xe.expect_poses(want, poses, 0.0, 0.0, RES), where + ", poses")
    m.close()


# ---- 2: cost-to-go ----------------------------------------------------------------------------------------------------------------------
def _thin(shape):
    return shape[0] <= 2 or shape[1] <= 2


def _run_starts(free):
    """the first cell of every run of free cells along the lines of a thin map (rows where H <= 2, columns otherwise)"""
    H, W = free.shape
    lines = free if H <= 2 else free.T
    before = np.zeros_like(lines)
    before[:, 1:] = lines[:, :-1]
    at = np.argwhere(lines & ~before)
    return [(int(k), int(l)) if H <= 2 else (int(l), int(k)) for l, k in at]


@functools.lru_cache(maxsize=None)
def seeds_of(shape, name, not_free, which):
    """"last": (W - 1, H - 1); "first": (0, 0) -- on a thin map, where the obstacles split the line, the first cell of every run of
    free cells; "both": the two together"""
    W, H = shape
    if which == "last":
        return ((W - 1, H - 1),)
    if which == "both":
        return seeds_of(shape, name, not_free, "first") + seeds_of(shape, name, not_free, "last")
    if not _thin(shape):
        return ((0, 0),)
    return tuple(_run_starts(~rx.blocked(log_of(shape, name), 0, not_free))) or ((0, 0),)


@functools.lru_cache(maxsize=None)
def blocked_of(shape, name, not_free, inflate):
    b = rx.blocked(log_of(shape, name), inflate, not_free)
    b.flags.writeable = False
    return b


@functools.lru_cache(maxsize=None)
def cost_of(shape, name, not_free, inflate, which):
    """the uncapped cost (int64, -1: none) of the seed set `which`.  The two constant logs have no Dijkstra: a map without an
    obstacle is _reach_expect.closed_form (whatever the inflation), a map of nothing but obstacles has no traversable cell"""
    W, H = shape
    seeds = seeds_of(shape, name, not_free, which)
    if name == "free" or (name == "unknown" and not not_free):
        c = np.minimum.reduce([rx.closed_form(W, H, s) for s in seeds])
    elif name == "unknown":
        c = np.full((H, W), -1, dtype=np.int64)
    else:
        c = rx.costs(blocked_of(shape, name, not_free, inflate), seeds)
    c.flags.writeable = False
    return c


def _small_cap(shape):
    return 5 * max(shape) // 2


def _reach_all(m, shape, names=LOGS, inflates=(0, 2)):
    """every field of the shape on m.  The seed sets go far corner first: the field of the second request must not keep what the
    first one left in the working field's last cell"""
    for name in names:
        m.upload_log(log_of(shape, name))
        for not_free in (True, False):
            for inflate in inflates:
                for which in ("last", "first", "both"):
                    cost, seeds = cost_of(shape, name, not_free, inflate, which), seeds_of(shape, name, not_free, which)
                    for max_cost in (0xFFFE, _small_cap(shape)):
                        where = f"{shape}, {name}, not_free = {not_free}, inflate = {inflate}, seeds {which}, max_cost = {max_cost}"
                        _same(m.reach(seeds, max_cost=max_cost, inflate=inflate, not_free=not_free), rx.cap(cost, max_cost), where)


@shapes
def test_cost_to_go(shape):
    m = _map(shape)
    _reach_all(m, shape)
    m.close()


@pytest.mark.parametrize("shape", [(65, 64), (64, 65), (128, 128)], ids=str)
def test_cost_to_go_one_round_per_read_back(shape, monkeypatch):
    monkeypatch.setenv("GMS_REACH_BATCH", "1")                                 # rounds launched = rounds needed
    W, H = shape
    m = _map(shape)
    _reach_all(m, shape, inflates=(0,))
    m.upload_log(log_of(shape, "free"))
    _same(m.reach([(0, 0)]), rx.closed_form(W, H, (0, 0)).astype(np.uint16), f"{shape}, all free")
    st = m.reach_stats()
    tiles = ((W + T - 1) // T) * ((H + T - 1) // T)
    assert tiles > 1 and st["tile_runs"] >= tiles and st["rounds"] >= 2, f"every tile of the open map ran: {st}"
    m.close()


# A diagonal step across the corner where four tiles meet, as the ONLY way a lower cost reaches the tile across the corner.
# Tiles: S the tile of A, D the tile diagonally across, N and E the two beside both.  A = (63, 64), B = (63, 63), C = (64, 64),
# D = (64, 63) before the flips.  Three one-cell corridors, 5 per step: from s1 46 steps to B, from s3 46 steps to C, from s2 45
# steps to A -- through the tile of C and back, so that A settles two rounds after B and C have.  B and C are then final at
# A + 5 and never change again, their tiles have nothing to hand on, and D = A + 7 arrives over the corner alone (B + 5 = A + 10).
CORNER_A, CORNER_B, CORNER_C, CORNER_D = (63, 64), (63, 63), (64, 64), (64, 63)
CORNER_SEEDS = ((63, 17), (110, 64), (60, 100))


@functools.lru_cache(maxsize=None)
def corner_case(flip_x, flip_y):
    """(logData [128][128], seeds, the cells A, B, C, D) of the corner case mirrored in x and / or y: one case per corner mark"""
    log = np.full((128, 128), L_OCC)
    for (xa, ya), (xb, yb) in (((63, 17), (63, 63)), ((64, 64), (110, 64)),                                    # s1 .. B, C .. s3
                               ((60, 100), (66, 100)), ((66, 100), (66, 90)), ((66, 90), (63, 90)), ((63, 90), (63, 64))):      # s2 .. A
        log[min(ya, yb):max(ya, yb) + 1, min(xa, xb):max(xa, xb) + 1] = L_FREE
    log[CORNER_D[1], CORNER_D[0]] = L_FREE
    fl = lambda c: (127 - c[0] if flip_x else c[0], 127 - c[1] if flip_y else c[1])
    if flip_x:
        log = log[:, ::-1]
    if flip_y:
        log = log[::-1, :]
    log = np.ascontiguousarray(log)
    log.flags.writeable = False
    return log, tuple(fl(s) for s in CORNER_SEEDS), tuple(fl(c) for c in (CORNER_A, CORNER_B, CORNER_C, CORNER_D))


@pytest.mark.parametrize("flip_x,flip_y", [(False, False), (True, False), (False, True), (True, True)])
def test_cost_to_go_over_the_corner_where_four_tiles_meet(flip_x, flip_y, monkeypatch):
    log, seeds, (A, B, C, D) = corner_case(flip_x, flip_y)
    want = rx.expect(log, seeds)
    at = lambda c: int(want[c[1], c[0]])
    assert at(A) == 225 and at(B) == at(C) == 230 and at(D) == 232, "the diagonal over the corner is the cheapest way to D"
    assert len({(c[0] // T, c[1] // T) for c in (A, B, C, D)}) == 4
    for batch in ("1", None):
        if batch:
            monkeypatch.setenv("GMS_REACH_BATCH", batch)
        else:
            monkeypatch.delenv("GMS_REACH_BATCH", raising=False)
        m = _map((128, 128))
        m.upload_log(log)
        for not_free in (True, False):
            _same(m.reach(seeds, not_free=not_free), want, f"flip_x = {flip_x}, flip_y = {flip_y}, GMS_REACH_BATCH = {batch}, not_free = {not_free}")
        m.close()


# ---- 2b: rooms and doors, the same relaxation on (cost, rank) keys and the 4-connected labelling ------------------------------------------
ROOMS = dict(core=2, inflate=0, not_free=False, min_core=1)                 # a 5 x 5 free box in walls has ONE core cell, its centre


def _rooms_same(m, log, where, **kw):
    want = ro.expect(log, **kw)
    m.upload_log(log)
    ro.same(m.rooms(labels=True, depth=True, cap_rooms=CAP, cap_doors=CAP, **kw), want, where)
    return want


@functools.lru_cache(maxsize=None)
def two_rooms_of(shape):
    """walls with two free boxes, (2, 2) .. (12, 12) in the first tile and the 9 x 9 box in the far corner, which on 65 x 64 and 64 x 65
    reaches into the ragged column / row, joined by a one-cell corridor along y = 7 and x = W - 5"""
    W, H = shape
    log = ro.walls(W, H)
    ro.carve(log, 2, 2, 12, 12)
    ro.carve(log, W - 9, H - 9, W - 1, H - 1)
    ro.carve(log, 13, 7, W - 5, 7)
    ro.carve(log, W - 5, 7, W - 5, H - 10)
    log.flags.writeable = False
    return log


@pytest.mark.parametrize("shape", [(65, 64), (64, 65), (128, 128)], ids=str)
def test_rooms_one_round_per_read_back(shape, monkeypatch):
    monkeypatch.setenv("GMS_ROOMS_BATCH", "1")                                 # rounds launched = rounds needed
    W, H = shape
    m = _map(shape)
    want = _rooms_same(m, two_rooms_of(shape), f"{shape}, two rooms", **ROOMS)
    assert want["n_rooms"] == 2 and want["n_doors"] == 1 and want["labels"][H - 1, W - 1] == want["doors"]["b"][0], "the far room holds the last cell"
    st = m.rooms_stats()
    assert st["rounds"] >= 2, f"the growth crossed a tile border: {st}"
    m.close()


@functools.lru_cache(maxsize=None)
def rooms_corner_case(flip_x, flip_y):
    """corner_case's corridors in a 130 x 130 map of walls, a 5 x 5 free box around each of its three seeds: three rooms whose cores
    are the seed and the cell beside it towards the corridor, so that the depth is corner_case's cost-to-go less one step.  A = (63, 64)
    settles two rounds after B and C have, B and C keep their smaller keys (depth 225 against 225, then 230 from A at 220) and hand
    nothing on, and D's key (227, the rank of A's room; 230 from B or C) arrives over the corner where the four tiles meet alone"""
    small, seeds, cells = corner_case(flip_x, flip_y)
    log = ro.walls(130, 130)
    log[:128, :128] = small
    for x, y in seeds:
        ro.carve(log, x - 2, y - 2, x + 2, y + 2)
    if flip_y:
        # A's room now lies above the other two and would rank first: a tie at B or C (225 from either side) would go to it, B and C
        # would change and hand D on themselves.  Five-cell-wide arms, away from the corridors, carry the other two rooms' cores up to
        # row 2, so that A's room ranks last as it does without the flip.
        (x1, y1), (x3, y3) = seeds[0], seeds[1]
        xa = 7 if flip_x else 120                                              # a free column beyond the third seed's box
        ro.carve(log, min(x1, xa) - 2, y1 - 2, max(x1, xa) + 2, y1 + 2)
        ro.carve(log, xa - 2, 0, xa + 2, y1 + 2)
        ro.carve(log, x3 - 2, 0, x3 + 2, y3 + 2)
    log.flags.writeable = False
    return log, seeds, cells


@pytest.mark.parametrize("flip_x,flip_y", [(False, False), (True, False), (False, True), (True, True)])
def test_rooms_over_the_corner_where_four_tiles_meet(flip_x, flip_y, monkeypatch):
    monkeypatch.setenv("GMS_ROOMS_BATCH", "1")
    log, seeds, (A, B, C, D) = rooms_corner_case(flip_x, flip_y)
    want = ro.expect(log, **ROOMS)
    depth, label = (lambda c: int(want["depth"][c[1], c[0]])), (lambda c: int(want["labels"][c[1], c[0]]))
    assert want["n_rooms"] == 3 and (flip_y or want["rooms"]["core_count"].tolist() == [2, 2, 2])
    assert depth(A) == 220 and depth(B) == depth(C) == 225 and depth(D) == 227, "the diagonal over the corner is the cheapest way to D"
    assert label(D) == label(A) != NONE and len({label(A), label(B), label(C), NONE}) == 4, "D is reached, and from A's room, not from B's or C's"
    assert [label(c) for c in (B, C, A)] == [want["labels"][s[1], s[0]] for s in seeds], "each of A, B, C belongs to the room at the end of its corridor"
    assert len({(c[0] // T, c[1] // T) for c in (A, B, C, D)}) == 4
    m = _map((130, 130))
    m.upload_log(log)
    ro.same(m.rooms(labels=True, depth=True, cap_rooms=CAP, cap_doors=CAP, **ROOMS), want, f"flip_x = {flip_x}, flip_y = {flip_y}")
    m.close()


def test_rooms_cores_touching_diagonally_across_a_tile_border_are_two():
    """core cells (63, y) and (64, y + 1) and no other: two cores under the rooms' 4-connectivity, and -- the same plane as a
    frontier plane -- ONE region under the frontiers' 8-connectivity"""
    y = 40
    log = ro.walls(130, 130)
    for cx, cy in ((63, y), (64, y + 1)):                                      # at core = 1 the centre of a free plus is its only core cell
        ro.carve(log, cx - 1, cy, cx + 1, cy)
        ro.carve(log, cx, cy - 1, cx, cy + 1)
    m = _map((130, 130))
    want = _rooms_same(m, log, "two pluses", core=1, inflate=0, not_free=False, min_core=1)
    m.close()
    assert want["n_rooms"] == 2 and want["rooms"]["core_count"].tolist() == [1, 1]
    assert (want["rooms"]["anchor_x"].tolist(), want["rooms"]["anchor_y"].tolist()) == ([63, 64], [y, y + 1])
    m = tf._map()
    rec = tf._check(m, tf._cells(tf._unknown(), [(63, y), (64, y + 1)]), "the two cells as a frontier plane")[0]
    m.close()
    assert rec["count"].tolist() == [2] and (rec["anchor_x"][0], rec["anchor_y"][0]) == (63, y)


# ---- 3: frontiers -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_of(shape):
    """the cost-to-go field the frontier requests are given: the random log's, not free, from the first seed set"""
    f = rx.cap(cost_of(shape, "random", True, 0, "first"))
    f.flags.writeable = False
    return f


@functools.lru_cache(maxsize=None)
def frontiers_of(shape, name, min_size, inflate, with_cost):
    return fx.expect(log_of(shape, name), min_size=min_size, inflate=inflate, cost=field_of(shape) if with_cost else None)


def _same_regions(got, want, where):
    assert got[1] == want[1], f"{where}: n_found {got[1]} != {want[1]}"
    _same(got[0], want[0], where + ", records")
    _same(got[2], want[2], where + ", labels")


def _frontiers_all(m, shape, names):
    for name in names:
        m.upload_log(log_of(shape, name))
        for min_size in (1, 3):
            for inflate in (0, 1):
                for with_cost in (False, True):
                    where = f"{shape}, {name}, min_size = {min_size}, inflate = {inflate}, cost = {with_cost}"
                    want = frontiers_of(shape, name, min_size, inflate, with_cost)
                    got = m.frontiers(min_size=min_size, inflate=inflate, cost=field_of(shape) if with_cost else None, labels=True, cap=CAP)
                    if name in ("free", "unknown"):
                        assert got[1] == 0 and len(got[0]) == 0 and (got[2] == NONE).all(), where + ": neither the map's edge nor the padding is unknown"
                    _same_regions(got, want, where)


@shapes
def test_frontiers(shape):
    W, H = shape
    m = _map(shape)
    _frontiers_all(m, shape, LOGS)
    if W >= 2:
        m.upload_log(log_of(shape, "last column"))
        want = frontiers_of(shape, "last column", 1, 0, False)
        assert want[0]["count"].tolist() == [H] and (want[0]["anchor_x"][0], want[0]["anchor_y"][0]) == (W - 2, 0)
        assert (want[0]["min_x"][0], want[0]["max_x"][0], want[0]["min_y"][0], want[0]["max_y"][0]) == (W - 2, W - 2, 0, H - 1)
        _same_regions(m.frontiers(labels=True, cap=CAP), want, f"{shape}, column {W - 1} unknown: column {W - 2} is one region")
    m.close()


# ---- 4: view gain ---------------------------------------------------------------------------------------------------------------------------
def _fan(n, lengths):
    """n evenly spaced probes over the full circle whose lengths (metres) cycle through `lengths`"""
    f = probe_fan(n, 1.0)
    d = np.resize(np.asarray(lengths, dtype=np.float64), n)
    f["local_x"] *= d
    f["local_y"] *= d
    f["distance"] = d
    return f


def _cell_pose(cx, cy, theta, fx_=0.5, fy_=0.5):
    """a pose in cell (cx, cy), the fraction (fx_, fy_) of a cell from its lower corner: the walks start in floor(pose / RES + 0.5)"""
    return [(cx + fx_ - 0.5) * RES, (cy + fy_ - 0.5) * RES, theta]


PROBES = _fan(96, [2.0, 5.0, 20.0])


@functools.lru_cache(maxsize=None)
def gain_poses_of(shape):
    """the centres of the four corner cells and of the middle cell, a pose on a cell corner, a pose outside the map"""
    W, H = shape
    poses = [_cell_pose(0, 0, 0.3), _cell_pose(W - 1, 0, 2.0), _cell_pose(0, H - 1, -1.0), _cell_pose(W - 1, H - 1, -2.5),
             _cell_pose(W // 2, H // 2, 0.7), _cell_pose(W // 2, H // 2, -0.4, 0.0, 0.0), [-0.5, H * RES / 2, 0.0]]
    poses = np.array(poses, dtype=np.float32)
    poses.flags.writeable = False
    return poses


@functools.lru_cache(maxsize=None)
def walks_of(shape):
    return gx.walks_of(_grid(shape), PROBES, gain_poses_of(shape))


@functools.lru_cache(maxsize=None)
def gain_of(shape, name, R):
    rec = gx.expect_walks(walks_of(shape), log_of(shape, name), R)
    rec.flags.writeable = False
    return rec


def _gain_all(m, shape, names, where):
    for name in names:
        m.upload_log(log_of(shape, name))
        for R in RANGES:
            got = m.gain(gain_poses_of(shape), PROBES, R)
            assert got.dtype == GAIN_DTYPE
            _same(got, gain_of(shape, name, R), f"{shape}, {name}, max_range = {R}{where}")


@shapes
def test_view_gain(shape):
    for mem in (False, True):
        m = _with_env("GMS_GAIN_WALK", mem, lambda: _map(shape, max_beams=96))
        _gain_all(m, shape, LOGS, ", GMS_GAIN_WALK=mem" if mem else "")
        m.close()


# ---- 5: the beam model ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def beam_case(shape):
    """(poses [65][3], beams [48]): 60 poses in free cells of the random log (drawn with repetition: the smallest maps have fewer) and
    5 just outside the map; beams of mixed length -- a third of them longer than the longest map is wide -- and mixed hit"""
    W, H = shape
    rng = np.random.default_rng(W * 1000 + H + 2)
    free = np.argwhere(log_of(shape, "random") < 0)
    pick = free[rng.integers(0, len(free), N_PARTICLES - 5)]
    xy = (pick[:, ::-1] + rng.uniform(-0.4, 0.4, (len(pick), 2))) * RES        # the walks start in floor(pose / RES + 0.5)
    poses = np.column_stack([xy, rng.uniform(-math.pi, math.pi, len(pick))]).tolist()
    poses += [[-0.06, H * RES / 2, 0.2], [(W + 0.2) * RES, H * RES / 2, 3.0], [W * RES / 2, -0.06, 1.5], [W * RES / 2, (H + 0.2) * RES, -1.5], [-0.06, -0.06, 0.8]]
    ang = rng.uniform(-math.pi, math.pi, N_BEAMS)
    dist = np.where(np.arange(N_BEAMS) % 3 == 0, rng.uniform(7.0, 12.0, N_BEAMS), rng.uniform(0.03, 1.5, N_BEAMS))
    beams = np.zeros(N_BEAMS, dtype=BEAM_DTYPE)
    beams["local_x"], beams["local_y"], beams["distance"] = dist * np.cos(ang), dist * np.sin(ang), dist
    beams["hit"] = rng.random(N_BEAMS) < 0.6
    poses = np.array(poses, dtype=np.float32)
    assert poses.shape == (N_PARTICLES, 3)
    poses.flags.writeable = False
    beams.flags.writeable = False
    return poses, beams


@functools.lru_cache(maxsize=None)
def remaining_of(shape, name, ahead):
    poses, beams = beam_case(shape)
    r = np.stack([bx.remaining(_grid(shape), log_of(shape, name), beams, p, ahead) for p in poses])
    r.flags.writeable = False
    return r


def _score_all(m, pf, shape, name, where):
    """weights, log-weights and residuals of every window, bit for bit, in the map as it stands: name is the log in force"""
    poses, beams = beam_case(shape)
    pf.set_poses(poses)
    for behind, ahead in WINDOWS:
        factors = beam_model_factors(RES, behind, ahead, 0.05)
        idx = bx.indices_from(remaining_of(shape, name, ahead), behind, ahead)
        w, lw = bx.weights_of(idx, beams["hit"] != 0, factors)
        res = pf.score_beams(beams, factors, behind, ahead, residuals=True)
        at = f"{shape}, {name}, behind = {behind}, ahead = {ahead}{where}"
        _same(res, idx, at + ", residuals")
        assert bx.same_bits(pf.get_weights(), w), at + ", weights"
        assert bx.same_bits(pf.get_log_weights(), lw), at + ", log-weights"


@shapes
def test_beam_model(shape):
    for mem in (False, True):
        m = _with_env("GMS_CAST_WALK", mem, lambda: _map(shape, max_beams=N_BEAMS))
        pf = ParticleFilter(m, N_PARTICLES)
        m.upload_log(log_of(shape, "random"))
        _score_all(m, pf, shape, "random", ", GMS_CAST_WALK=mem" if mem else "")
        pf.close(); m.close()


# ---- 6: one handle through every query --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 64), (33, 2)], ids=str)
def test_one_handle_through_every_query(shape):
    """the scratch the units share on a handle (the inflation's clearance field and blocked plane, the frontier planes, the staging)
    survives being used by the neighbouring unit, on two logs in turn"""
    m = _map(shape, max_beams=96)
    pf = ParticleFilter(m, N_PARTICLES)
    rect = _odd_rect(shape)
    for name in ("random", "second", "random"):
        log = log_of(shape, name)
        m.upload_log(log)
        for turn in (0, 1):
            where = f"{shape}, {name}, turn {turn}"
            _same(m.clearance(rect=rect, max_radius=9, not_free=True), xe.expect(log, 9, True, rect=rect), where + ", clearance")
            seeds = seeds_of(shape, name, True, "both")
            _same(m.reach(seeds, inflate=2), rx.expect(log, seeds, inflate=2), where + ", reach")
            cost = rx.expect(log, seeds)
            _same_regions(m.frontiers(inflate=1, cost=cost, labels=True, cap=CAP), fx.expect(log, inflate=1, cost=cost), where + ", frontiers")
            _same(m.gain(gain_poses_of(shape), PROBES, 40), gx.expect_walks(walks_of(shape), log, 40), where + ", gain")
            _score_all(m, pf, shape, name, f", turn {turn}")
    pf.close(); m.close()


# ---- preconditions: what the expectations must contain for the comparisons above to mean something ---------------------------------------------
def _forbidden_diagonals(block, field):
    """diagonal steps between two reached cells of different tiles that squeeze past a blocked cell"""
    H, W = block.shape
    ok = field != FAR
    ys, xs = np.mgrid[0:H - 1, 0:W - 1]
    n = 0
    for ax, ay, bx_, by in ((xs, ys, xs + 1, ys + 1), (xs + 1, ys, xs, ys + 1)):
        ends = ok[ay, ax] & ok[by, bx_]
        tiles = (ax // T != bx_ // T) | (ay // T != by // T)
        squeezed = block[ay, bx_] | block[by, ax]
        n += int((ends & tiles & squeezed).sum())
    return n


def test_the_expectations_contain_what_they_are_meant_to():
    """preconditions on the expectations, none on the device"""
    for shape in SHAPES:
        W, H = shape
        log = log_of(shape, "random")
        assert log[0, 0] < 0 and (log > 0).any() == (W * H > 8)
        if W >= 3 and H >= 3:
            for not_free in (True, False):
                reached = (rx.cap(cost_of(shape, "random", not_free, 0, "first")) != FAR).sum()
                free = (~blocked_of(shape, "random", not_free, 0)).sum()
                assert reached >= 0.95 * free, (shape, not_free, reached, free, "the seed at (0, 0) reaches the map")
            assert (rx.cap(cost_of(shape, "random", True, 0, "first"), _small_cap(shape)) == FAR).sum() > (field_of(shape) == FAR).sum(), (shape, "the small cap cuts")
        if shape in BORDERED:
            for not_free in (True, False):
                n = _forbidden_diagonals(blocked_of(shape, "random", not_free, 0), rx.cap(cost_of(shape, "random", not_free, 0, "first")))
                assert n >= 10, (shape, not_free, n, "forbidden diagonals across a tile border")
            rec = frontiers_of(shape, "random", 1, 0, True)[0]
            spans = ((rec["min_x"] < T) & (rec["max_x"] >= T)) | ((rec["min_y"] < T) & (rec["max_y"] >= T))
            assert spans.any(), (shape, "a region across a 64-cell border")
            assert (rec["goal_x"] >= 0).any()
        # view gain: a window that is the whole map, clipped on both sides at once
        rec = gain_of(shape, "random", 255)
        whole = (rec["walked"] > 0) & (rec["start_x"] - 255 <= 0) & (rec["start_x"] + 255 >= W - 1) & (rec["start_y"] - 255 <= 0) & (rec["start_y"] + 255 >= H - 1)
        assert whole.sum() >= 5 and rec["walked"][6] == 0 and rec["start_x"][6] == -1, (shape, "the poses inside see the whole map, the one outside nothing")
        assert (rec["start_x"][:4].tolist(), rec["start_y"][:4].tolist()) == ([0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1])
        if W * H >= 64:
            assert (gain_of(shape, "random", 255)["unknown"] > 0).any() and (gain_of(shape, "random", 255)["hits"] > 0).any()
            for behind, ahead in WINDOWS[1:]:
                idx = bx.indices_from(remaining_of(shape, "random", ahead), behind, ahead)
                assert len(np.unique(idx)) >= 3, (shape, behind, ahead, np.unique(idx))
            assert (remaining_of(shape, "random", 2)[-5:] == 0).all(), "a pose outside the map starts no walk"
