"""The evidence that tests/test_gpu_route_edges.py can fail: every input family of tests/_route_cases.py has the property it exists for,
shown with the definition restated in tests/_route_expect.py alone.  Host only."""
import numpy as np
import pytest

import _route_cases as rc
import _route_expect as rt


def _one(case, start, look=64, max_cells=16384, max_waypoints=64):
    rec, ways, paths = rt.expect(case.field, case.blocked, [start], look, max_cells, max_waypoints)
    return rec[0], ways[0], paths[0]


def test_a_every_gadget_takes_the_step_it_was_built_for():
    a = rc.family_a()
    nxt = a.meta["next"]
    winners = set()
    for name, start in a.starts.items():
        rec, _, path = _one(a, start)
        assert path[0] == tuple(start)
        if name.startswith(("exit", "border")):                            # (tests of their own below)
            continue
        if nxt[name] is None:
            want = 0 if a.field[start[1], start[0]] == 0 else rt.BROKEN
            assert (len(path), rec["flags"]) == (1, want), (name, path, rec)
        else:
            assert path[1] == nxt[name] and not rec["flags"] & rt.BROKEN or name == "sum fffe", (name, path)
        if name.startswith("subset"):
            mask = int(name.split()[1], 16)
            k = rt.ORDER.index((path[1][0] - start[0], path[1][1] - start[1]))
            assert k == min(i for i in range(8) if mask >> i & 1), name
            dx, dy = rt.ORDER[k]
            r = 5 if dx and dy else 7
            assert path == [(start[0] + i * dx, start[1] + i * dy) for i in range(r + 1)] and rec["end_cost"] == 0, (name, "its own arm to its own seed")
            for i in range(8):                                                 # exactly the subset is admissible, each on its own
                alone = a.field.copy()
                for j, (ex, ey) in enumerate(rt.ORDER):
                    if j != i:
                        alone[start[1] + ey, start[0] + ex] = rc.FILL
                p = rt.descent(alone, start, 64)[0]
                assert (len(p) > 1) == bool(mask >> i & 1), (name, i)
                if len(p) > 1:
                    assert p[1] == (start[0] + rt.ORDER[i][0], start[1] + rt.ORDER[i][1]) and alone[p[-1][1], p[-1][0]] == 0
            winners.add(k)
    assert winners == set(range(8)), "every direction wins somewhere"
    assert sum(n.startswith("subset") for n in a.starts) == 255 and sum(n.startswith("single") for n in a.starts) == 8
    rec, _, path = _one(a, a.starts["sum fffe"])
    assert (rec["start_cost"], rec["end_cost"], len(path), rec["flags"]) == (0xFFFE, 0xFFF9, 2, rt.BROKEN)


def test_a_squeezed_diagonals_and_wrapping_sums_would_be_taken_by_a_wrong_rule():
    a = rc.family_a()
    for name, start in a.starts.items():
        x, y = start
        if name.startswith("squeeze"):
            k = rc.NAMES.index(name.split()[1].split("-")[0])
            dx, dy = rt.ORDER[k]
            assert int(a.field[y + dy, x + dx]) + rt.DIAG == int(a.field[y, x]), "cost-consistent"
            assert rt.FAR in (a.field[y, x + dx], a.field[y + dy, x]), "a side is FAR"
            open_ = a.field.copy()
            open_[y, x + dx] = open_[y + dy, x] = rc.FILL
            assert rt.descent(open_, start, 8)[0][1] == (x + dx, y + dy), (name, "with both sides open the diagonal is the step")
        if name.startswith("sum") and name != "sum fffe":
            cur = int(a.field[y, x])
            wraps = [(ex, ey) for ex, ey in rt.ORDER if a.field[y + ey, x + ex] not in (rt.FAR, rc.FILL)
                     and (int(a.field[y + ey, x + ex]) + (rt.DIAG if ex and ey else rt.AXIS)) & 0xFFFF == cur]
            assert wraps or cur in (4, 6), (name, "a neighbour that a 16-bit sum would admit")
            if cur == 2:
                assert a.field[y, x - 1] == 65533
    names = [n for n in a.starts if n.startswith("squeeze")]
    assert len([n for n in names if n.endswith("alone")]) == 12 and len(names) >= 19
    assert {n.split()[1] for n in names if "then" in n} >= {"NE-a", "NE-b", "NE-ab", "NW-a", "NW-b", "NW-ab", "SW-a"}


def test_a_border_cells_see_what_a_wrapped_index_would_reach():
    a = rc.family_a()
    W, H = a.W, a.H
    borders = [n for n in a.starts if n.startswith("border")]
    assert len(borders) == 12
    placed = 0
    for name in borders:
        x, y = a.starts[name]
        assert x in (0, W - 1) or y in (0, H - 1)
        rec, _, path = _one(a, (x, y))
        if name.endswith("none"):
            assert (len(path), rec["flags"]) == (1, rt.BROKEN), name
        else:
            assert path[1] == a.meta["next"][name] and len(path) == 2 and rec["flags"] == rt.BROKEN, name
        first_wrapped = None
        for k, (dx, dy) in enumerate(rt.ORDER):
            nx, ny = x + dx, y + dy
            idx = ny * W + nx
            if (0 <= nx < W and 0 <= ny < H) or not 0 <= idx < W * H:
                continue
            v = int(a.field[idx // W, idx % W])
            if v + (rt.DIAG if dx and dy else rt.AXIS) == 20:
                placed += 1
                first_wrapped = k if first_wrapped is None else first_wrapped
        if name.split()[2] == "one" and name.split()[1] in ("west", "east"):
            assert first_wrapped is not None and first_wrapped < rt.ORDER.index((path[1][0] - x, path[1][1] - y)), "the wrapped cell would win"
    assert placed >= 14


def test_a_exits_in_the_definitions_order():
    a = rc.family_a()
    for n in rc.EXIT_N:
        rec, ways, paths = rt.expect(a.field, a.blocked, a.cells_of([f"exit {n} {k}" for k in ("broken", "seed", "next")]), 64, n, n)
        assert rec["n_cells"].tolist() == [n] * 3 and rec["flags"].tolist() == [rt.BROKEN, 0, rt.CELLS_CUT], n
        assert rec["end_cost"].tolist() == [3, 0, 5]


@pytest.mark.parametrize("two", [False, True])
def test_b_the_chain_is_the_longest_descent(two):
    b = rc.family_b(two)
    chain = b.meta["chain"]
    rec, _, path = _one(b, chain[0], look=4096)
    assert rec["n_cells"] == 13107 == 0xFFFE // 5 + 1 and path == chain and rec["flags"] == 0
    assert rec["start_cost"] == (0xFFFE if two else 65530) and rec["end_cost"] == 0
    if two:
        steps = [(q[0] - p[0], q[1] - p[1]) for p, q in zip(chain, chain[1:])]
        assert sum(1 for s in steps if s[0] and s[1]) == 2
    for n in (1, 63, 64, 65, 4096, 4097):
        assert _one(b, b.starts[f"n={n}"])[0]["n_cells"] == n
    assert _one(b, chain[0], look=4096, max_cells=13106)[0]["flags"] == rt.CELLS_CUT


def test_b_clearance_minima_sit_where_the_key_is_decided():
    b = rc.family_b()
    chain = b.meta["chain"]
    seen = set()
    for name, _ in rc.B_CLEAR:
        clear, d2, at = rc.clear_b(name)
        rec = rt.expect(b.field, b.blocked, [chain[0]], 4096, 16384, 8, clear)[0][0]
        assert (rec["min_d2"], rec["min_d2_at"]) == (d2, at), name
        along = np.array([clear[y, x] for x, y in chain])
        assert (along == d2).sum() == (13107 if name == "ffff everywhere" else 2 if name.startswith("equal") else 1), name
        seen.add((d2, at))
    assert {(100, i) for i in (0, 63, 64, 127, 128, 8191, 8192, 13106)} <= seen and {(0, 8191), (0xFFFE, 8192), (0xFFFF, 0)} <= seen


def test_c_every_band_cell_blocks_and_no_other():
    c = rc.family_c()
    g = c.meta["gadgets"]
    rec, ways, paths = rt.expect(c.field, c.blocked, c.cells_of(range(len(g))), 64, 32, 8)
    ties, near, octants, majors, squares = 0, 0, set(), set(), 0
    for i, (a, b, occ, x_first) in enumerate(g):
        dx, dy = b[0] - a[0], b[1] - a[1]
        assert paths[i] == [(a[0] + x, a[1] + y) for x, y in rc.l_path(dx, dy, x_first)] and rec["flags"][i] == 0
        assert rt.visible(c.blocked, a, b) == rt.visible_box(c.blocked, a, b)
        if occ is None:
            assert ways[i] == [a, b]
            continue
        ex = rc.band_excess(dx, dy, occ)
        if ex <= 0:
            assert ways[i] != [a, b] and len(ways[i]) > 2, (a, b, occ)
            if ex == 0:
                ties += 1
                octants.add((dx > 0, dy > 0, abs(dx) > abs(dy)))
                majors.add(abs(dx) > abs(dy))
                squares += abs(dx) == abs(dy)
        else:
            assert ways[i] == [a, b], (a, b, occ)
            near += ex in (1, 2)
    small = [(b[0] - a[0], b[1] - a[1], x_first) for a, b, _, x_first in g if max(abs(b[0] - a[0]), abs(b[1] - a[1])) <= 6]
    assert len(set(small)) == 2 * 168, "every displacement within +-6, along x first and along y first"
    assert ties >= 400 and near >= 100 and len(octants) == 8 and majors == {True, False} and squares >= 8, (ties, near, octants, squares)
    print(f"\n{len(g)} gadgets, {ties} with a tie cell occupied, {near} with a cell 1 or 2 outside the band")


def test_c_long_segments_blockers_are_the_nearest_the_band_has():
    c = rc.family_c_long()
    chain = c.meta["chain"]
    a, b = chain[0], chain[-1]
    assert (a, b, len(chain)) == ((0, 0), (4096, 30), 4097) and c.field[0, 0] == 20540
    assert _one(c, a, look=4096, max_cells=4100)[1] == [a, b]
    assert _one(c, a, look=4095, max_cells=4100)[1] == [a, chain[4095], b], "the far end is out of reach"
    # 2 |30 x - 4096 y| is a multiple of 4 and |dx| + |dy| = 4126 is not: this segment has no tie cell; the margins are the smallest it has
    assert all(ex != 0 for t in range(4097) for _, ex in rc.segment_columns(a, b, t))
    # columns 1 .. 67 hold one band cell each, the path's own: the blockers near the start come from a window of one period
    assert all([cc for cc, ex in rc.segment_columns(a, b, t) if ex <= 0] == [chain[t]] for t in range(1, 68))
    for t in (1, 2048, 4095):
        inner, edge, out = rc.long_blockers(a, b, t, c.W, c.H, chain)
        assert inner[1] < -rc.CL_DEEP and -rc.CL_RIM < edge[1] <= 0 < out[1] < rc.CL_RIM, "deep inside the band, and within 50 of 4126 on either side of its edge"
        assert all(cell not in chain and abs(cell[0] - t) <= rc.CL_WINDOW for cell, _ in (inner, edge, out))
        assert not rt.visible_box(rc.family_c_long(blocker=edge[0]).blocked, a, b) and not rt.visible_box(rc.family_c_long(blocker=inner[0]).blocked, a, b)
        assert rt.visible_box(rc.family_c_long(blocker=out[0]).blocked, a, b)
    ends = rc.long_end_cells(a, b, c.W, c.H, chain)
    assert [e[0] for e in ends] == [1, 4095] and all(rt.visible_box(rc.family_c_long(blocker=e).blocked, a, b) for e in ends)
    for kw in (dict(reverse=True), dict(mirror=True), dict(transpose=True), dict(reverse=True, mirror=True, transpose=True)):
        cc = rc.family_c_long(**kw)
        ch = cc.meta["chain"]
        assert _one(cc, ch[0], look=4096, max_cells=4100)[2] == ch
        assert (cc.W, cc.H) == ((40, 4100) if kw.get("transpose") else (4100, 40))


def test_d_the_corner_is_the_largest_visible_index():
    d = rc.family_d()
    for leg in rc.D_LEGS:
        cells = d.meta["corridors"][leg]
        assert len(cells) - leg - 1 >= 700 and _one(d, cells[0], max_cells=1024)[2] == cells
        assert rt.visible_box(d.blocked, cells[0], cells[leg])
        assert not any(rt.visible_box(d.blocked, cells[0], cells[j]) for j in range(leg + 1, len(cells)))
        for h in rc.D_EXTRA:
            ways = _one(d, cells[0], look=leg + h, max_cells=1024)[1]
            assert ways[1] == cells[leg], (leg, h)


def test_d_the_staircase_is_its_own_supercover():
    """the closed band of (cells[0], cells[k]) for odd k is exactly the staircase between them: the whole corridor is one line of sight,
    and one occupied cell of it hides everything behind"""
    s = rc.family_d_stairs()
    cells = s.meta["corridors"][0]
    rec, ways, path = _one(s, cells[0], look=4096, max_cells=1024, max_waypoints=700)
    assert path == cells and ways == [cells[0], cells[-1]] and rec["flags"] == 0
    assert all(not rt.visible_box(s.blocked, cells[0], cells[k]) for k in range(2, 700, 2)), "a square diagonal's tie cells are walls"
    o = rc.family_d_stairs(occupied=41)
    rec, ways, _ = _one(o, cells[0], look=4096, max_cells=1024, max_waypoints=700)
    assert rec["flags"] == rt.MISMATCH and cells[40] in ways and cells[41] in ways and cells[42] in ways
    full = len(ways)
    rec, cut, _ = _one(o, cells[0], look=4096, max_cells=1024, max_waypoints=full - 1)
    assert rec["flags"] & rt.WAYPOINTS_CUT and cut == ways[:-1]


def test_d_the_meander_is_pulled_in_steps_of_three_at_most():
    """what the staircase cannot give: hundreds of waypoints, each found after many empty passes.  A search from index i has
    699 - i candidates, so ten empty passes need i < 57: of the 281 searches 23 run ten or more and 228 two or more"""
    m = rc.family_d_meander()
    cells = m.meta["corridors"][0]
    rec, ways, paths = rc.expect_meander(m, [0], 4096, 1024, 700)
    assert paths[0] == cells and rec["flags"][0] == 0 and len(ways[0]) >= 250
    idx = [cells.index(w) for w in ways[0]]
    assert all(0 < j - i <= 3 for i, j in zip(idx, idx[1:])), "from no waypoint is more than 3 ahead visible"
    for i in idx[:-1]:
        assert not any(rt.visible_box(m.blocked, cells[i], cells[j]) for j in range(i + 4, min(i + 12, len(cells))))
    empty = [(min(i + 4096, len(cells) - 1) - j) // 64 for i, j in zip(idx, idx[1:])]
    assert sum(e >= 10 for e in empty) >= 18 and sum(e >= 2 for e in empty) >= 200, "(56 / 3 = 18 searches start below index 57)"
    cut = rc.expect_meander(m, [0], 4096, 1024, len(ways[0]) - 1)
    assert cut[0]["flags"][0] == rt.WAYPOINTS_CUT and cut[1][0] == ways[0][:-1]
    o = rc.family_d_meander(occupied=M_OCC)
    rec, w, _ = rt.expect(o.field, o.blocked, o.cells_of(["late"]), 4096, 1024, 700)
    k = [cells.index(c) for c in w[0]]
    assert rec["flags"][0] == rt.MISMATCH and M_OCC - 1 in k and M_OCC in k, "the step onto the occupied cell alone finds nothing visible"


M_OCC = 650


def test_a_corners_with_one_true_neighbour():
    c = rc.family_a_corners()
    for name, start in c.starts.items():
        rec, _, path = _one(c, start)
        assert path == [start, c.meta["next"][name]] and rec["flags"] == rt.BROKEN, name


def test_e_launch_starts_repeat_and_leave_the_map():
    a = rc.family_a()
    st = rc.launch_starts(65536)
    assert len({tuple(s) for s in st.tolist()}) == len(a.starts) + len(rc.OFF_MAP)
    rec, _, _ = rc.expect_memo("A", st[:700], 64, 1, 1)
    assert (rec["flags"] == rt.NO_PATH).sum() >= 8 and (rec["flags"] & rt.CELLS_CUT).any() and (rec["flags"] & rt.BROKEN).any()
