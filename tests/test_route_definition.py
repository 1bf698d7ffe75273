"""Routes (include/gridmapslam.h "routes") without a device: the restatement tests/_route_expect.py against answers derived by hand --
corridors, the corner rule of VISIBLE, the cuts -- and its descent against gridmap.descend() on Dijkstra fields of
tests/_reach_expect.py."""
import numpy as np
import pytest

import _reach_expect as rch
import _route_expect as rt
from gridmap_slam_robot_amd import descend, route_points

FAR = 0xFFFF


def _walls(W, H, free):
    b = np.ones((H, W), bool)
    for x, y in free:
        b[y, x] = False
    return b


def _field(W, H, costs):
    f = np.full((H, W), FAR, np.uint16)
    for (x, y), c in costs.items():
        f[y, x] = c
    return f


def test_a_straight_corridor_gives_two_waypoints():
    free = [(x, 1) for x in range(1, 8)]
    blocked = _walls(9, 3, free)
    field = _field(9, 3, {(x, 1): 5 * (7 - x) for x in range(1, 8)})           # the seed is (7, 1)
    cells, flags, start_cost, end_cost = rt.descent(field, (1, 1), 100)
    assert cells == free and (flags, start_cost, end_cost) == (0, 30, 0)
    for see in (rt.visible, rt.visible_box):
        assert rt.pull(cells, blocked, 64, 8, see) == ([(1, 1), (7, 1)], 0)
        assert rt.pull(cells, blocked, 4, 8, see) == ([(1, 1), (5, 1), (7, 1)], 0), "look caps a leg at four path cells"
        assert rt.pull(cells, blocked, 1, 8, see) == (cells, 0), "look = 1: the waypoints are the cells"
    rec, ways, paths = rt.expect(field, blocked, [(1, 1), (7, 1), (0, 1), (-1, 1), (3, 9)], 64, 100, 8, clear=np.full((3, 9), 9, np.uint16))
    assert rec["n_cells"].tolist() == [7, 1, 0, 0, 0] and rec["n_waypoints"].tolist() == [2, 1, 0, 0, 0]
    assert rec["flags"].tolist() == [0, 0, rt.NO_PATH, rt.NO_PATH, rt.NO_PATH], "on a seed: one cell, one waypoint; on a wall and off the map: no path"
    assert rec["start_cost"].tolist() == [30, 0, FAR, FAR, FAR] and rec["end_cost"].tolist() == [0, 0, FAR, FAR, FAR]
    assert rec["min_d2"].tolist() == [9, 9, FAR, FAR, FAR] and rec["min_d2_at"].tolist() == [0] * 5, "a tie: the smallest index"
    assert rec["end_x"].tolist() == [7, 7, 0, -1, 3] and rec["end_y"].tolist() == [1, 1, 1, 1, 9] and (rec["pad"] == 0).all()
    assert ways[1] == [(7, 1)] and paths[2] == []


def test_an_l_shaped_corridor_turns_at_the_corner_cell():
    """east along y = 1 to (5, 1), then north along x = 5 to the seed (5, 5).  The diagonal (4, 1) -> (5, 2) squeezes past the wall
    cell (4, 2), so the descent goes through the corner.  From (1, 1) the cell (5, 2) is not visible: dx = 4, dy = 1, and the wall cell
    (3, 2) has 2 |2 * 1 - 1 * 4| = 4 <= 5, inside the band; (5, 1) is, along the row.  From (5, 1) the column is clear to the seed."""
    row, col = [(x, 1) for x in range(1, 6)], [(5, y) for y in range(2, 6)]
    blocked = _walls(7, 7, row + col)
    field = _field(7, 7, {**{(x, 1): 20 + 5 * (5 - x) for x in range(1, 6)}, **{(5, y): 5 * (5 - y) for y in range(1, 6)}})
    cells, flags, _, _ = rt.descent(field, (1, 1), 100)
    assert cells == row + col and flags == 0
    assert not rt.visible(blocked, (1, 1), (5, 2)) and rt.visible(blocked, (1, 1), (5, 1)) and rt.visible(blocked, (5, 1), (5, 5))
    for see in (rt.visible, rt.visible_box):
        assert rt.pull(cells, blocked, 64, 8, see) == ([(1, 1), (5, 1), (5, 5)], 0)
    clear = np.full((7, 7), 16, np.uint16)
    clear[1, 3] = clear[3, 5] = 4
    rec, ways, _ = rt.expect(field, blocked, [(1, 1)], 64, 100, 8, clear=clear)
    assert (rec["min_d2"][0], rec["min_d2_at"][0]) == (4, 2), "the minimum is taken twice: the smaller path index"
    assert np.array_equal(route_points(np.array(ways[0]), 3, (-1.0, 2.0), 0.5), [[-0.25, 2.75], [1.75, 2.75], [1.75, 4.75]])


def test_the_cuts_and_a_broken_field():
    free = [(x, 1) for x in range(1, 8)]
    blocked = _walls(9, 3, free)
    field = _field(9, 3, {(x, 1): 5 * (7 - x) for x in range(1, 8)})
    assert rt.descent(field, (1, 1), 7)[:2] == (free, 0) and rt.descent(field, (1, 1), 8)[:2] == (free, 0)
    assert rt.descent(field, (1, 1), 6) == (free[:6], rt.CELLS_CUT, 30, 5), "cut to its first max_cells cells; end_cost is the last one's"
    assert rt.pull(free, blocked, 2, 4) == ([(1, 1), (3, 1), (5, 1), (7, 1)], 0)
    assert rt.pull(free, blocked, 2, 3) == ([(1, 1), (3, 1), (5, 1)], rt.WAYPOINTS_CUT) and rt.pull(free, blocked, 2, 1) == ([(1, 1)], rt.WAYPOINTS_CUT)
    assert rt.pull(free[:1], blocked, 2, 1) == ([(1, 1)], 0), "one cell needs one waypoint"
    field[1, 4] += 1                                                           # (4, 1): 15 -> 16; (3, 1) holds 20 and finds no neighbour of 15
    assert rt.descent(field, (1, 1), 100) == (free[:3], rt.BROKEN, 30, 20)
    field[1, 4] -= 1
    blocked[1, 4] = True                                                       # a field of another map: (4, 1) is a wall now
    w, flags = rt.pull(free, blocked, 64, 8)
    assert w == [(1, 1), (3, 1), (4, 1), (5, 1), (7, 1)] and flags == rt.MISMATCH, "nothing visible from (3, 1) nor from the wall cell: one cell on, flagged"


def test_no_line_of_sight_between_two_blocked_cells_that_touch_at_a_corner():
    free = _walls(4, 4, [(x, y) for x in range(4) for y in range(4)])
    for see in (rt.visible, rt.visible_box):
        b = free.copy()
        b[2, 1] = b[1, 2] = True                                               # (1, 2) and (2, 1)
        assert not see(b, (1, 1), (2, 2)) and not see(b, (2, 2), (1, 1)) and not see(b, (0, 0), (3, 3))
        b = free.copy()
        b[1, 1] = b[2, 2] = True                                               # the other diagonal: (1, 1) and (2, 2)
        assert not see(b, (1, 2), (2, 1)) and not see(b, (2, 1), (1, 2)) and not see(b, (0, 3), (3, 0))
        assert see(free, (0, 0), (3, 3)) and see(free, (0, 3), (3, 0))


def test_a_legal_diagonal_step_is_visible_and_one_with_a_blocked_side_cell_is_not():
    free = _walls(3, 3, [(x, y) for x in range(3) for y in range(3)])
    for see in (rt.visible, rt.visible_box):
        for a, b in (((1, 1), (2, 2)), ((1, 1), (0, 2)), ((1, 1), (0, 0)), ((1, 1), (2, 0))):
            assert see(free, a, b)
            for side in ((b[0], a[1]), (a[0], b[1])):
                blk = free.copy()
                blk[side[1], side[0]] = True
                assert not see(blk, a, b), (a, b, side)
        blk = free.copy()
        blk[1, 1] = True
        assert not see(blk, (1, 1), (1, 2)) and not see(blk, (1, 0), (1, 1)), "both ends count"


def _dijkstra_case():
    rng = np.random.default_rng(4827)
    W, H = 37, 29
    log = np.where(rng.random((H, W)) < 0.22, 0.85, -0.4)
    log[3:9, 20] = np.nan
    log[14, 14] = -0.4
    return log, rch.blocked(log, 0, True), rch.expect(log, [(14, 14), (30, 5)])


def test_both_forms_of_visible_agree():
    _, blocked, _ = _dijkstra_case()
    rng = np.random.default_rng(77)
    a = rng.integers(0, (37, 29), size=(600, 2))
    b = np.clip(a + rng.integers(-5, 6, size=(600, 2)), 0, (36, 28))          # short segments: in this clutter a long one is hardly ever free
    got = [(rt.visible(blocked, p, q), rt.visible_box(blocked, p, q)) for p, q in zip(a, b)]
    assert all(x == y for x, y in got) and 60 < sum(x for x, _ in got) < 540, "both answers occur"


def test_the_descent_is_descend_on_a_dijkstra_field():
    _, blocked, field = _dijkstra_case()
    starts = [(x, y) for y in range(0, 29, 3) for x in range(0, 37, 3)]
    n_paths = 0
    for s in starts:
        cells, flags, start_cost, end_cost = rt.descent(field, s, 16384)
        assert cells == descend(field, s), s
        assert flags == (0 if cells else rt.NO_PATH) and start_cost == int(field[s[1], s[0]]) and end_cost == (0 if cells else FAR)
        n_paths += len(cells) > 3
        w, more = rt.pull(cells, blocked, 4096, 16384)
        assert more == 0 and (not cells or (w[0] == cells[0] and w[-1] == cells[-1])), "a field of its own map never mismatches"
        assert all(rt.visible(blocked, a, b) for a, b in zip(w, w[1:]))
    assert n_paths > 40
    # one cell of a path raised by 1: descend() refuses the field exactly where the restatement says BROKEN, and follows it elsewhere
    start = max(starts, key=lambda s: len(descend(field, s)))
    path = descend(field, start)
    assert len(path) > 12
    n_broken = 0
    for k in range(1, len(path)):
        bad = field.copy()
        bad[path[k][1], path[k][0]] += 1
        cells, flags, _, _ = rt.descent(bad, start, 16384)
        assert cells[:k] == path[:k]
        if flags & rt.BROKEN:
            n_broken += 1
            with pytest.raises(ValueError):
                descend(bad, start)
        else:
            assert flags == 0 and cells == descend(bad, start)
    assert n_broken > 0
