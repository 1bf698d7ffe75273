"""What the inputs of tests/test_gpu_rollout_edges.py must contain for its comparisons to reach the rollouts' edges: conditions on the
cases of tests/_rollout_edge_cases.py and their plain expectations alone, none on the device."""
import numpy as np
import pytest

import _rollout_edge_cases as ec
import _rollout_expect as rx

NONE = np.zeros((0, 2), np.float32)
ONE_OF = rx.OUTSIDE | rx.RANGE | rx.BLOCKED


def _probed(geo, pose, steps):
    """the cells a call's steps ask about from one pose, as a set"""
    x, y = rx.cells(geo, pose, steps, NONE)
    return set(zip(x[:, 0, 0].tolist(), y[:, 0, 0].tolist()))


def _overhang(W, H, R, sx, sy):
    return (sx - R < 0, sx + R > W - 1, sy - R < 0, sy + R > H - 1)


# ---- A ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.CENSUS_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_census_starts_and_probes_reach_every_edge(shape):
    W, H = shape
    geo = ec.census_geo(shape)
    wants = {mode: ec.census_want(shape, mode) for mode in ec.census_modes(shape)}
    for R in ec.CENSUS_RANGES:
        starts = ec.census_starts(W, H, R)
        calls = ec.census_calls(shape, R)
        assert all(len(steps) <= ec.MAX_K and steps.shape[1] == 1 for _, _, steps in calls)
        assert R > 30 or len(calls[0][1]) > 1 or all(s[1] < 0 or s[2] < 0 for s in starts), "start cells share one call where they can"
        # every pose stands in its start cell, negative ones too (rx.cells: Java's cast)
        probed = {}
        for whats, poses, steps in calls:
            for what, pose in zip(whats, poses):
                x0, y0 = rx.cells(geo, pose, rx.IDENTITY.reshape(1, 1), NONE)
                cell = [s[1:] for s in starts if s[0] == what]
                assert cell == [(int(x0[0, 0, 0]), int(y0[0, 0, 0]))], (R, what)
                probed.setdefault(what, set()).update(_probed(geo, pose, steps))
        assert set(probed) == {s[0] for s in starts}
        # the probes: the window and the ring outside it, or the three rings and a thousand cells inside
        for what, sx, sy in starts:
            if R <= 30:
                a = range(-(R + 1), R + 2)
                need = {(sx + i, sy + j) for i in a for j in a}
            else:
                need = {(sx + i, sy + j) for d in (R - 1, R, R + 1) for i, j in ec._ring(d).tolist()}
                inside = {c for c in probed[what] if max(abs(c[0] - sx), abs(c[1] - sy)) <= R - 2}
                # (1024 distinct offsets; where a table is shared, two offsets on either side of coordinate 0 may meet in cell 0)
                assert len(inside) >= (1024 if sx < 0 or sy < 0 else 960), (R, what, len(inside))
            assert need <= probed[what], (R, what, sorted(need - probed[what])[:4])
        # the residues of the window's first bit that this map and range allow at all, the three of them on any map but the smallest
        cells = {s[1:] for s in starts}
        allowed = {r for r in ec.RESIDUES if any((sx - R) % 32 == r for sx in range(-R, W + R))}
        assert allowed <= {(sx - R) % 32 for sx, _ in cells} and (2 * R + W < 32 or allowed == set(ec.RESIDUES)), (R, allowed)
        assert any(sx - R < 0 for sx, _ in cells) and any(sx < 0 for sx, _ in cells) and any(sx >= W for sx, _ in cells)
        assert {(-R, H // 2), (-R - 1, H // 2), (W - 1 + R, H // 2), (W + R, H // 2), (W // 2, -R), (W // 2, -R - 1), (W // 2, H - 1 + R), (W // 2, H + R)} <= cells
        # the window over each edge alone and over all four, wherever a start cell ON the map can have it so
        on_map = {_overhang(W, H, R, sx, sy) for sx in range(W) for sy in range(H)}
        have = {_overhang(W, H, R, sx, sy) for sx, sy in cells}
        for pattern in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (True, True, True, True)):
            assert pattern not in on_map or pattern in have, (R, pattern)
        # the outcomes
        seen = set()
        for mode, want in wants.items():
            by_start = {}
            for (whats, _, _), rec in zip(calls, want[R]):
                for what, row in zip(whats, rec):
                    by_start.setdefault(what, []).append(row["flags"] & ONE_OF)
                    assert ((row["first_hit"] == 0) == ((row["flags"] & ONE_OF) != 0)).all() and (row["first_hit"] <= 1).all()
            by_start = {k: np.concatenate(v) for k, v in by_start.items()}
            kinds = set(np.concatenate(list(by_start.values())).tolist())
            assert kinds <= {0, rx.OUTSIDE, rx.RANGE, rx.BLOCKED} and {rx.OUTSIDE, rx.RANGE} <= kinds
            assert W * H < 6 or kinds == {0, rx.OUTSIDE, rx.RANGE, rx.BLOCKED}, (R, mode, kinds)
            seen |= kinds
            # one start cell of each pair has a window, the other has none: nothing it asks about is on the map and in range
            for near, far in (("x = -R", "x = -R - 1"), ("x = W - 1 + R", "x = W + R"), ("y = -R", "y = -R - 1"), ("y = H - 1 + R", "y = H + R")):
                assert np.isin(by_start[near], (0, rx.BLOCKED)).any(), (R, near)
                assert np.isin(by_start[far], (rx.OUTSIDE, rx.RANGE)).all() and (by_start[far] == rx.RANGE).any(), (R, far)
        assert seen == {0, rx.OUTSIDE, rx.RANGE, rx.BLOCKED}, "free, off the map, out of range and blocked, over the modes"


def test_census_logs_block_about_half_the_cells():
    for shape in ec.CENSUS_MAPS[2:]:
        for mode in ec.census_modes(shape):
            assert 0.3 < ec.census_blocked(shape, mode).mean() < 0.7, (shape, mode)
    assert not ec.census_blocked((1, 1), ("dense", False, 0))[0, 0] and ec.census_blocked((1, 1), ("dense", True, 0))[0, 0]


def test_the_probe_expectation_is_the_expectation():
    for shape, R in (((33, 2), 1), ((33, 2), 15), ((31, 3), 32)):
        for mode in ec.census_modes(shape):
            geo, blocked = ec.census_geo(shape), ec.census_blocked(shape, mode)
            for (_, poses, steps), want in zip(ec.census_calls(shape, R), ec.census_want(shape, mode)[R]):
                assert np.array_equal(want, rx.expect(geo, None, poses, steps, NONE, R, blocked=blocked))


# ---- B ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("name", list(ec.ROUND_MAPS))
def test_rounding_probes_tell_the_reciprocal_from_the_division(name, axis):
    W, H, res, origin, log, poses, steps = ec.round_case(name, axis)
    by_rinv, by_div = ec.round_quotients(name, axis)
    differ = np.trunc(by_rinv) != np.trunc(by_div)
    assert differ.sum() >= 64 and differ[0].sum() >= 32 and differ[1].sum() >= 32, differ.sum(axis=1)
    n = np.arange(1, ec.ROUND_N + 1)
    assert np.array_equal(by_div[0, :ec.ROUND_N], n) and np.array_equal(by_div[1, :ec.ROUND_N], n + ec.ROUND_SHIFT), "the multiples are exact"
    geo = rx.Geometry(W, H, res, *origin)
    want = ec.round_want(name, axis)
    field, other = ("last_x", "last_y") if axis == 0 else ("last_y", "last_x")
    for p, first in ((0, 0), (1, ec.ROUND_SHIFT)):
        assert (want[p]["start_x" if axis == 0 else "start_y"] == first).all() and (want[p][other] == 0).all()
        cell = rx.cells(geo, poses[p], steps, NONE)[axis][:, 0, 0]
        assert np.array_equal(cell, np.concatenate([n, n - 1, n]) + first), "n * resolution and the float above lie in cell n, the float below in n - 1"
        assert cell.max() < max(W, H) and np.array_equal((want[p]["flags"] & ONE_OF) != 0, cell % 2 == 1), "neighbouring cells differ"
        free = cell % 2 == 0
        assert np.array_equal(want[p][field][free], cell[free]) and (want[p]["first_hit"][free] == 1).all()


# ---- C ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [0, 3])
@pytest.mark.parametrize("T", ec.SWEEP_T)
def test_sweep_hits_at_every_step_and_the_minima_lie_where_they_should(T, F):
    want = ec.sweep_want(T, F, "steps")[0]
    h = np.arange(T + 1)
    assert np.array_equal(want["first_hit"], h), "candidate h hits at step h, candidate T never"
    assert np.array_equal(want["hit_point"][:T], [ec.sweep_hit(i, F)[1] for i in range(T)]) and want["hit_point"][T] == 0xFFFF
    assert (want["flags"][:T] == rx.BLOCKED).all() and want["flags"][T] == 0
    assert np.array_equal(np.column_stack([want["last_x"][1:], want["last_y"][1:]]), [ec.sweep_path(i - 1) for i in range(1, T + 1)])
    if F:
        assert (want["hit_point"][:T] < F).sum() == T // 2, "in half the candidates a footprint point collides, not the centre"
        geo, arcs = ec.sweep_geo(), ec.sweep_arcs(T, F)
        x, y = rx.cells(geo, ec.cell_poses([ec.SWEEP_START])[0], arcs, ec.SWEEP_POINTS)
        kd = rx.kinds(geo, rx.blocked_plane(ec.sweep_log(), 0, True), *ec.SWEEP_START, 255, x, y)
        at = kd[np.arange(T), np.arange(T)] != 0                                # [h][point] at step h
        assert set(map(tuple, at.tolist())) == {(False, False, False, True), (True, True, False, False), (False, True, True, False), (False, False, True, False)}
        assert (kd.sum(axis=2) != 0).sum() == T, "nothing else collides, in front of the hit or behind it"
    bs, bc = want["best_step"].astype(int), want["best_cost"].astype(int)
    assert bs[0] == 0xFFFF and (bs[1:64] == 0).all() and bs[64] == 63 and (bc[1:64] == 900).all()
    if T >= 65:
        assert bs[65] == 64 and bc[65] == 700
    assert (want["end_cost"][1:] != 0xFFFF).all() and want["end_cost"][0] == 0xFFFF
    if T == 256:
        clear, cost = ec.sweep_fields()["steps"]
        along = cost[tuple(np.array([ec.sweep_path(j) for j in range(256)]).T[::-1])].astype(int)
        assert along[64] == along[140] == along[:150].min() and (bs[141:151] == 64).all(), "equal minima in two passes: the earlier step"
        assert np.array_equal(bs[152:182], np.arange(151, 181)), "the minimum at first_hit - 1"
        assert along[205] == along[210] == along.min() and (bs[211:] == 205).all() and bs[206] == 205, "equal minima in one pass"
        assert (want["min_d2"][129:] == 50).all() and want["min_d2"][70] == 3000 - 69, "min_d2 from a pass in front of the hit's"
        last = ec.sweep_want(T, F, "last")[0]
        assert (last["best_step"][1:256] == 0).all() and (last["best_cost"][1:256] == 0xFFFF).all()
        assert (last["best_step"][256], last["best_cost"][256], last["end_cost"][256]) == (255, 0xFFFE, 0xFFFE) and (last["min_d2"] == 0xFFFF).all()
    far = ec.sweep_want(T, F, "far")[0]
    assert (far["best_step"][1:] == 0).all() and (far["best_cost"] == 0xFFFF).all() and far["best_step"][0] == 0xFFFF
    alone = ec.sweep_want(T, F, "clear alone")[0]
    assert (alone["best_step"] == 0xFFFF).all() and np.array_equal(alone["min_d2"], want["min_d2"])


# ---- D ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 63])
def test_one_point_alone_collides_at_each_start(F):
    log, poses, steps, points = ec.one_point_case(F)
    assert len(poses) == F + 2 and len(points) == F
    geo, blocked = rx.Geometry(ec.ONE_W, ec.ONE_H, ec.RES, 0.0, 0.0), rx.blocked_plane(log, 0, True)
    for p, pose in enumerate(poses):
        x, y = rx.cells(geo, pose, rx.IDENTITY.reshape(1, 1), points)
        assert len(set(zip(x[0, 0].tolist(), y[0, 0].tolist()))) == F + 1, "the points and the centre lie in distinct cells"
        hits = np.flatnonzero(rx.kinds(geo, blocked, int(x[0, 0, -1]), int(y[0, 0, -1]), 255, x, y)[0, 0])
        assert hits.tolist() == ([p] if p <= F else []), p
    want = ec.one_point_want(F)
    sb = (want["flags"] & rx.START_BLOCKED) != 0
    assert sb[:F + 1].all() and not sb[F + 1:].any() and np.array_equal(sb[:, 0], sb[:, 1])
    assert np.array_equal(want["first_hit"][:, 0] == 0, sb[:, 0]) and (want["first_hit"][F + 1, 0] == 2), "staying in place: the hit is the start's"
    assert np.array_equal(want["hit_point"][:F + 1, 0], np.arange(F + 1))
    assert (want["first_hit"][:, 1] == 2).all(), "moving away: no hit, whatever the start"


# ---- E ----------------------------------------------------------------------------------------------------------------------------------
def test_the_batched_filter_rows_differ():
    logs, poses = ec.risk_logs(), ec.risk_poses()
    assert logs.shape == (3, 128, 128) and poses.shape == (3, ec.RISK_N, 3) and (logs[1] == 0).all()
    assert not np.array_equal(poses[0], poses[1]) and not np.array_equal(poses[1], poses[2])
    for inflate, not_free in ec.RISK_MODES:
        want = ec.risk_want(inflate, not_free)
        assert want.shape == (3, len(ec.RISK_ARCS))
        for a, b in ((0, 1), (0, 2), (1, 2)):
            for f in ("n_hit", "n_start_blocked", "sum_first_hit"):
                assert (want[a][f] != want[b][f]).any(), (inflate, a, b, f)
        assert (want["n_hit"] > 0).all() and (want["min_first_hit"] == 0).all()
    assert not np.array_equal(ec.risk_want(0, False), ec.risk_want(2, True))
