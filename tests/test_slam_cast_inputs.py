"""What the inputs of tests/_slam_cast_cases.py must contain, asserted with the oracle alone (no device): every family does what its
name says, the oracle's expectation is SENSITIVE to it -- replaced by its naive reading, a compared quantity (refined pose, weight,
touched cells) changes --, and the two conditions the device test relies on hold: the oracle's weights are finite wherever weights
are compared numerically, and at most half of the special particles are ones whose map the oracle leaves untouched.

The naive readings: a NaN pose component (or the NaN trig of an infinite heading) read as a pose outside the map, where the cast
makes cell 0; a saturating component read as wrapping to cell 0 -- "outside" is what saturation itself gives, so that reading
changes nothing and the one a conversion through unsigned or modulo 2^32 would give is taken; a hit end point in (-1, 0) read as
outside; a start cell in (-1, 0) truncated to cell 0; gx == W read as W - 1 (and W - 1 as outside); a pose a cell outside the map
whose rays are walked from where they enter it; a quotient within 2^-19 of an integer decided the other way."""
import numpy as np
import pytest

import _slam_cast_cases as cc
from oracle import oracle as orc

MAP_NAMES = tuple(cc.MAPS)
INT_MAX, INT_MIN = 2147483647, -2147483648


def _outcome(name, i, pose, z, refine):
    """what SLAM.update does to particle i alone (SLAM.java:93-105): (pose, weight before the normalisation, touched cells)"""
    g = cc.scene(name).g
    lik = cc.warm_fields(name)[i]
    p = np.asarray(pose, np.float32)
    if refine:
        p, _, _ = g.find_best_pose(lik, z, p)
    w = g.probability_of(lik, z, p)
    log = np.array(cc.warm_logs(name)[i])
    g.integrate(log, z, p)
    return p, w, log != cc.warm_logs(name)[i]


def _differs(a, b):
    return not (np.array_equal(a[0], b[0], equal_nan=True) and a[1] == b[1] and np.array_equal(a[2], b[2]))


def _sensitive(name, family, pose=None, z=None, modes=(False, True)):
    """the family's outcome against its naive reading's (another pose, another scan), plain and refined"""
    i = cc.slot_of(family)
    P, z0 = cc.special_poses(name), cc.special_scan(name)
    for refine in modes:
        assert _differs(_outcome(name, i, P[i], z0, refine), _outcome(name, i, P[i] if pose is None else pose, z0 if z is None else z, refine)), \
            f"{name} {family} refine={refine}: the naive reading changes nothing"


def _cleared(z, beams):
    z = z.copy()
    z["hit"][list(beams)] = 0
    return z


def _walk_counts(name, i, P=None):
    return np.array([len(c) for c, _ in cc.walks(name, i, P)])


@pytest.mark.parametrize("name", MAP_NAMES)
def test_the_layout(name):
    g = cc.scene(name).g
    assert g.W * g.H <= 4000 and cc.N <= 48 and cc.B <= 128
    assert all(any(abs(s - o) == 1 for o in cc.ORDINARY) for s in cc.SLOTS), "every special slot has an ordinary neighbour"
    assert all((l != 0).sum() > 100 for l in cc.warm_logs(name)), "no map is blank in front of the special update"
    P = cc.special_poses(name)
    for i in cc.ORDINARY:
        assert np.isfinite(P[i]).all() and cc.start_cell(g, P[i])[0] in range(g.W) and cc.start_cell(g, P[i])[1] in range(g.H)
        assert _walk_counts(name, i).sum() > 10 * cc.B / 2


@pytest.mark.parametrize("name", MAP_NAMES)
def test_non_finite_poses_are_cell_zero(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    for f in cc.NAN_CELL:
        i, comp = cc.slot_of(f), {"x": 0, "y": 1, "th": 2}[f.split("_")[1]]
        assert not np.isfinite(P[i, comp]) and np.isfinite(np.delete(P[i], comp)).all()
        sc_ = cc.start_cell(g, P[i])
        if comp == 2:                                                  # NaN trig: 0 * NaN is NaN in both coordinates
            assert np.isnan(orc.pose_trig(P[i, 2])).all() and sc_ == (0, 0)
        else:
            assert sc_[comp] == 0 and 0 < sc_[1 - comp]
        ws = cc.walks(name, i)
        assert all(len(c) == 0 or tuple(c[0]) == sc_ for c, _ in ws), f"{f}: every ray starts in the cell the cast makes of NaN"
        assert sum(len(c) > 0 for c, _ in ws) >= cc.B - len(cc.family_beams()), f"{f}: ... and the ordinary ones do start"
        ex, ey = cc.end_cell(g, P[i], z["local_x"][cc.A], z["local_y"][cc.A])
        assert (ex, ey)[comp if comp < 2 else 0] == 0
        assert g.probability_of(cc.warm_fields(name)[i], z, P[i]) != 1.0, f"{f}: the end points score"
        outside = P[i].copy()
        outside[comp if comp < 2 else 0] = 1e6
        if comp == 2:
            outside[2] = 0.0
        assert cc.end_cell(g, outside, 0.1, 0.1)[comp if comp < 2 else 0] > g.W + g.H
        _sensitive(name, f, pose=outside)


@pytest.mark.parametrize("name", MAP_NAMES)
def test_saturating_poses_start_no_walk(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    for f in cc.SATURATING:
        i, comp = cc.slot_of(f), {"x": 0, "y": 1}[f.split("_")[1]]
        assert abs(float(P[i, comp])) >= 1e30
        assert cc.start_cell(g, P[i])[comp] == (INT_MAX if P[i, comp] > 0 else INT_MIN)
        assert cc.end_cell(g, P[i], z["local_x"][cc.A], z["local_y"][cc.A])[comp] == (INT_MAX if P[i, comp] > 0 else INT_MIN)
        assert _walk_counts(name, i).sum() == 0
        # (a beam at the opposite infinity meets the pose in a NaN, which is cell 0: the families' beams aside)
        assert g.probability_of(cc.warm_fields(name)[i], _cleared(z, cc.family_beams()), P[i]) == 1.0, f"{f}: every ordinary beam is skipped (GridMap.java:276)"
        wrapped = P[i].copy()
        wrapped[comp] = np.nan                                         # the reading that lands in cell 0
        _sensitive(name, f, pose=wrapped)
    for f in ("p1e30_th", "m1e30_th"):
        i = cc.slot_of(f)
        assert abs(float(P[i, 2])) >= 1e30 and np.isfinite(orc.pose_trig(P[i, 2])).all()
        assert _walk_counts(name, i).sum() > cc.B
        zero = P[i].copy()
        zero[2] = 0.0
        _sensitive(name, f, pose=zero)


@pytest.mark.parametrize("name", MAP_NAMES)
def test_end_points_just_below_zero_score_as_cell_zero_and_are_never_walked_to(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    for f, axes in (("end_x", (0,)), ("end_y", (1,)), ("end_xy", (0, 1))):
        i = cc.slot_of(f)
        q = cc.quotients(g, P[i], z["local_x"][cc.A], z["local_y"][cc.A])
        cell = cc.end_cell(g, P[i], z["local_x"][cc.A], z["local_y"][cc.A])
        ray = g.scan_rays(z[cc.A:cc.A + 1], P[i])[0]
        for a in axes:
            assert -1.0 < q[a] < -0.5 and cell[a] == 0, (f, q)
            assert np.floor(np.float64(ray[2 + a] + np.float32(0.5))) == -1.0, "the iterator's last cell is -1 (RayIterator.java:83-100)"
        assert all(0 <= c < n for c, n in zip(cell, (g.W, g.H))), (f, cell)
        cells, _ = cc.walks(name, i)[cc.A]
        assert len(cells) > 3 and (cells >= 0).all()
        lik = cc.warm_fields(name)[i]
        assert g.probability_of(lik, z, P[i]) != g.probability_of(lik, _cleared(z, [cc.A]), P[i]), f"{f}: the beam is scored, in cell 0"
        # (the naive reading, "outside", is the scan without that factor: the weight of the plain update changes)


@pytest.mark.parametrize("name", MAP_NAMES)
def test_start_cells_outside_start_no_walk_while_the_end_points_score(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    res = cc.geometry(g)[0]
    want = {"start_x": (-1, None), "start_y": (None, -1), "outside_w": (-1, None), "outside_e": (g.W, None), "outside_s": (None, -1),
            "outside_n": (None, g.H)}
    inward = {"start_x": (0.5, 0), "start_y": (0, 0.5), "outside_w": (1.5, 0), "outside_e": (-1.5, 0), "outside_s": (0, 1.5), "outside_n": (0, -1.5)}
    for f, (wx, wy) in want.items():
        i = cc.slot_of(f)
        sc_ = cc.start_cell(g, P[i])
        assert (wx is None or sc_[0] == wx) and (wy is None or sc_[1] == wy), (f, sc_)
        assert (wx is not None or 0 <= sc_[0] < g.W) and (wy is not None or 0 <= sc_[1] < g.H), (f, sc_)
        ray = g.scan_rays(z[:1], P[i])[0]
        if f.startswith("start"):
            a = 0 if wx is not None else 1
            assert -1.0 < float(ray[a] + np.float32(0.5)) < 0.0, "a truncation would say cell 0"
            assert len(g.trace_ray(ray[0] + np.float32(0.5), ray[1] + np.float32(0.5), ray[2] + np.float32(0.5), ray[3] + np.float32(0.5))) == 0
        assert _walk_counts(name, i).sum() == 0, f"{f}: no ray starts (RayIterator.java:108)"
        assert g.probability_of(cc.warm_fields(name)[i], z, P[i]) != 1.0, f"{f}: the end points score"
        moved = P[i].copy()
        moved[0] += np.float32(inward[f][0] * res); moved[1] += np.float32(inward[f][1] * res)
        sm = cc.start_cell(g, moved)
        assert 0 <= sm[0] < g.W and 0 <= sm[1] < g.H
        _sensitive(name, f, pose=moved, modes=(False,))


@pytest.mark.parametrize("name", MAP_NAMES)
def test_end_points_in_the_last_column_and_row_and_one_beyond(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    for f, a, cell in (("gx_last", 0, g.W - 1), ("gx_W", 0, g.W), ("gy_last", 1, g.H - 1), ("gy_H", 1, g.H)):
        i = cc.slot_of(f)
        lik = cc.warm_fields(name)[i]
        got = cc.end_cell(g, P[i], z["local_x"][cc.A], z["local_y"][cc.A])
        assert got[a] == cell and 0 <= got[1 - a] < (g.H, g.W)[a], (f, got)
        scored = g.probability_of(lik, z, P[i]) != g.probability_of(lik, _cleared(z, [cc.A]), P[i])
        assert scored == (cell < (g.W, g.H)[a]), f"{f}: cell {cell} is {'inside' if cell < (g.W, g.H)[a] else 'outside'} (GridMap.java:276)"
        if f in ("gx_W", "gy_H"):                                       # read as the last cell: the beam half a cell further in
            zn = cc.nudged_scan(g, z, cc.A, P[i], a, -0.5)
            assert cc.end_cell(g, P[i], zn["local_x"][cc.A], zn["local_y"][cc.A])[a] == cell - 1
            _sensitive(name, f, z=zn, modes=(False,))
        # (W - 1 read as outside is the scan without that factor: `scored` above says that the plain update's weight changes)


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("side", ["below", "above"])
def test_guard_poses_have_a_quotient_within_2_to_the_minus_19_of_an_integer(name, side):
    g, z = cc.scene(name).g, cc.special_scan(name)
    start, b, axis, m = cc.guard_design(name, side)
    i = cc.slot_of("guard_" + side)
    assert np.array_equal(cc.special_poses(name)[i], start) and z["hit"][b] == 1
    refined = cc.expect(name, "special", True).poses[i]
    k = cc.lattice_index(start, refined)
    assert k is not None and not np.array_equal(refined, start), "the search moved the pose onto a lattice pose"
    f, mm = cc.guard_distance(g, refined, z["local_x"][b], z["local_y"][b], axis)
    assert mm == m and 0 < m < (g.W, g.H)[axis] - 1
    assert (-cc.GUARD <= f < 0.0) if side == "below" else (0.0 < f <= cc.GUARD), f
    assert cc.end_cell(g, refined, z["local_x"][b], z["local_y"][b])[axis] == (m - 1 if side == "below" else m)
    # decided the other way: the end point 2^-17 of a cell further on
    zn = cc.nudged_scan(g, z, b, refined, axis, 2.0 ** -17 * (1 if side == "below" else -1))
    assert cc.end_cell(g, refined, zn["local_x"][b], zn["local_y"][b])[axis] == (m if side == "below" else m - 1)
    _sensitive(name, "guard_" + side, z=zn, modes=(True,))


@pytest.mark.parametrize("name", MAP_NAMES)
def test_beam_families(name):
    g, P, z = cc.scene(name).g, cc.special_poses(name), cc.special_scan(name)
    base = cc.scene(name).tr.scans[cc.WARM]
    for fam, lx, ly, dist in cc.BEAM_FAMILIES:
        idx = [cc.beam_index(fam, 1), cc.beam_index(fam, 0)]
        assert list(z["hit"][idx]) == [1, 0]
        for col, v in (("local_x", lx), ("local_y", ly), ("distance", dist)):
            if v is not None:
                assert np.array_equal(z[col][idx], [v, v], equal_nan=True), (fam, col)
            elif fam != "zero_length":
                assert np.isfinite(z[col][idx]).all() and (col == "distance" or (z[col][idx] != 0).all())
        # mixed into an ordinary scan, and the oracle's outcome of an ordinary particle depends on them
        zo = z.copy()
        zo[idx] = base[idx]
        zo["hit"][idx] = [1, 0]
        assert any(_differs(_outcome(name, i, P[i], z, r), _outcome(name, i, P[i], zo, r)) for i in cc.ORDINARY[:4] for r in (False, True)), fam
    assert len(set(cc.family_beams()) | {cc.A, cc.BQ} | set(range(cc.AXIS0, cc.AXIS0 + 4))) == 2 * len(cc.BEAM_FAMILIES) + 6
    assert len(cc.plain_hits(name)) > cc.B // 2 and (z["hit"] == 0).sum() >= len(cc.BEAM_FAMILIES)
    # exact axis directions: from a heading of exactly 0 the ray has dy == 0 or dx == 0 (RayIterator.java:78, :91)
    assert P[0, 2] == 0.0 and 0 in cc.ORDINARY
    rays = g.scan_rays(z, P[0])
    for k in range(4):
        r = rays[cc.AXIS0 + k]
        assert (r[3] == r[1] and r[2] != r[0]) if k < 2 else (r[2] == r[0] and r[3] != r[1]), (k, r)
        assert len(cc.walks(name, 0)[cc.AXIS0 + k][0]) > 3
    assert sorted(z["hit"][cc.AXIS0:cc.AXIS0 + 4]) == [0, 0, 1, 1]
    # a zero-length ray emits its one cell 1 + additionalSteps times (RayIterator.java:75)
    cells, _ = cc.walks(name, 0)[cc.beam_index("zero_length", 1)]
    assert len(cells) == 3 and (cells == cells[0]).all()


@pytest.mark.parametrize("name", MAP_NAMES)
def test_the_empty_box_scan(name):
    g, P, z = cc.scene(name).g, cc.empty_box_poses(name), cc.special_scan(name)
    logs = cc.warm_logs(name)
    assert sum(not np.isfinite(p).all() or np.abs(p).max() >= 1e30 for p in P) >= 4
    scoring = 0
    for i in range(cc.N):
        sx, sy = cc.start_cell(g, P[i])
        assert not (0 <= sx < g.W and 0 <= sy < g.H), f"particle {i}: its start cell is inside the map"
        assert _walk_counts(name, i, P).sum() == 0, f"particle {i}: a ray starts"
        inside = [b for b in range(cc.B) if z["hit"][b] and all(0 <= c < n for c, n in zip(cc.end_cell(g, P[i], z["local_x"][b], z["local_y"][b]), (g.W, g.H)))]
        scoring += len(inside) > 0
    assert scoring >= cc.N // 2, "most particles see a hit end inside the map"
    for refine in (False, True):
        e = cc.expect(name, "empty_box", refine)
        assert all(np.array_equal(e.log(i), logs[i]) for i in range(cc.N)), "the oracle's maps stay bit-identical"
        assert np.isfinite(e.weights).all() and len(np.unique(e.weights)) > cc.N // 2, "... while the weights move"
        assert not np.array_equal(e.weights, np.full(cc.N, 1.0 / cc.N))
    assert np.array_equal(cc.expect(name, "empty_box", False).poses, P)


@pytest.mark.parametrize("name", MAP_NAMES)
@pytest.mark.parametrize("refine", [False, True])
def test_the_two_conditions_of_the_device_test(name, refine):
    """(1) the oracle's weights are finite for every group whose weights are compared numerically: all of them, here -- no update of
    these cases divides 0 by 0; (2) at most half of the special particles keep the map they had"""
    e = cc.expect(name, "special", refine)
    assert np.isfinite(e.weights).all() and (e.weights > 1e-290).any()
    logs = cc.warm_logs(name)
    untouched = [f for f in cc.SPECIAL if np.array_equal(e.log(cc.slot_of(f)), logs[cc.slot_of(f)])]
    assert 2 * len(untouched) <= len(cc.SPECIAL), untouched
    assert all(not np.array_equal(e.log(i), logs[i]) for i in cc.ORDINARY)
    if refine:
        P = cc.special_poses(name)
        moved = sum(not np.array_equal(e.poses[i], P[i], equal_nan=True) for i in range(cc.N))
        assert moved > cc.N // 2, "the search moves most poses"
        assert np.isnan(e.poses[cc.slot_of("nan_x"), 0]) and np.isfinite(e.poses[cc.slot_of("nan_x"), 1:]).all()
    else:
        assert np.array_equal(e.poses, cc.special_poses(name), equal_nan=True)
