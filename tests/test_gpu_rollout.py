"""Trajectory rollouts of the shared maps on the device (include/gridmapslam.h "trajectory rollouts"): gms_map_rollout[_dev] against the
definition restated in numpy (tests/_rollout_expect.py).  Every comparison is array_equal on the whole record array: every result is
an integer, there is no tolerance.  A rollout must see the map as a download would return it at that moment.

The base map is 200 x 136 cells (the cost-to-go fields' size): ragged in 32- and 64-cell words, with NaN, 0.0 and -0.0 holes."""
import functools
import math
import os

import numpy as np
import pytest

import _rollout_expect as rx
from gridmap_slam_robot_amd import ROLLOUT_DTYPE, GridMap, probe_fan, rollout_arcs, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ROLLOUT_CANDIDATES, GmsError
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
CPW = GMS_ROLLOUT_CANDIDATES
GUARD = 0xA5
# (T, F, K, max_range, P): every T of {1, 63, 64, 65, 256} -- below, at and above a pass of 64 steps, and four passes --, every F of
# {0, 1, 64}, K one below, at and one above a workgroup's candidates (and past two workgroups), every range of {1, 7, 255}, P of {1, 3}
SHAPES = [(1, 0, CPW - 1, 7, 3), (63, 1, CPW, 255, 1), (64, 64, CPW + 1, 7, 3), (65, 1, CPW + 1, 255, 3), (256, 64, CPW - 1, 255, 1), (256, 0, 2 * CPW + 3, 1, 3),
          (65, 64, CPW, 1, 1), (64, 0, 1, 255, 3)]
MAPS = [(False, 0), (False, 3), (True, 0), (True, 3)]     # (not_free, inflate)


def _same(got, want, where=""):
    assert got.dtype == ROLLOUT_DTYPE and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"{where}: {len(bad)} of {want.size} records differ, first at {bad[:1].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _with_walk(mem, make):
    old = os.environ.pop("GMS_ROLLOUT_WALK", None)
    if mem:
        os.environ["GMS_ROLLOUT_WALK"] = "mem"                             # read when the handle is created
    try:
        return make()
    finally:
        os.environ.pop("GMS_ROLLOUT_WALK", None)
        if old is not None:
            os.environ["GMS_ROLLOUT_WALK"] = old


def _cell_pose(cx, cy, theta, fx=0.5, fy=0.5):
    """a pose in cell (cx, cy), the fraction (fx, fy) of a cell from its lower corner"""
    return [(cx + fx) * RES, (cy + fy) * RES, theta]


def _arcs(K, T, seconds=4.0):
    """K unicycle commands, forwards and backwards, left and right, rolled for `seconds`: up to 4.8 m, 96 cells"""
    k = np.arange(K)
    v = np.where(k % 5 == 4, -0.4, 0.3 + 0.9 * ((k * 7) % 11) / 10.0)
    omega = np.where(k % 4 == 0, 0.0, -1.5 + 3.0 * ((k * 5) % 13) / 12.0)
    return rollout_arcs(v, omega, seconds / T, T)


def _points(F):
    """F outline points of an ellipse of 0.6 x 0.4 m (12 x 8 cells), the first straight ahead"""
    a = 2 * math.pi * np.arange(F) / max(F, 1)
    return np.column_stack([0.3 * np.cos(a), 0.2 * np.sin(a)]).astype(np.float32)


def _base_log():
    rng = np.random.default_rng(200136)
    log = np.zeros((H, W))                                                     # never observed
    log[10:121, 10:181] = L_FREE                                               # a room ...
    log[10, 10:181] = log[120, 10:181] = L_OCC                                 # ... with walls,
    log[10:121, 10] = log[10:121, 180] = L_OCC
    log[60:64, 0:11] = L_FREE                                                  # a door in the west wall and a passage to the map's edge,
    log[10:90, 70] = L_OCC                                                     # an inner wall with a gap at its end,
    log[60, 100:181] = L_OCC
    log[60, 130:136] = L_FREE
    log[126:136, :] = L_FREE                                                   # a free strip along the top edge, corner to corner
    log[0:6, 0:40] = L_FREE                                                    # ... and a free corner at the origin
    room = np.zeros((H, W), bool)
    room[11:120, 11:180] = True
    log[room & (rng.random((H, W)) < 0.0008)] = L_OCC                           # clutter
    log[30:40, 100:112] = 0.0                                                  # holes in the room: never observed,
    log[80:90, 140:150] = np.nan                                               # NaN
    log[95:100, 30:44] = -0.0                                                  # and -0.0
    log[100, 120] = L_OCC                                                      # the pose on a wall
    return log


POSES = np.array([_cell_pose(45, 75, 0.3),                                     # in the room
                  _cell_pose(0, 0, 0.6),                                       # in the map's corner cell
                  _cell_pose(120, 100, 0.7),                                   # on a wall cell
                  [-0.5, 3.0, 0.0],                                            # off the map, within reach of it
                  [np.nan, 3.1, 1.0],                                          # a NaN coordinate
                  _cell_pose(199, 135, -2.5, fx=0.99, fy=0.99),                # the far corner, at the cell's edge
                  _cell_pose(150, 30, math.pi / 2), _cell_pose(105, 35, -1.0),  # in the room's other half; inside a never-observed hole
                  [30.0, -40.0, 1.0],                                          # farther from the map than any range
                  [5.0, 3.0, np.nan], _cell_pose(64, 32, 2.0, fx=0.0, fy=0.0), _cell_pose(20, 62, math.pi)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def base_case():
    """(geometry, logData, {(not_free, inflate): (blocked plane, clear field, cost field)})"""
    g = orc.Grid(WM, HM, RES, 0.0, 0.0)
    assert (g.W, g.H) == (W, H)
    log = _base_log()
    log.flags.writeable = False
    return rx.Geometry(W, H, RES, 0.0, 0.0), log, {key: rx.blocked_plane(log, key[1], key[0]) for key in MAPS}


def _base_map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=360, **kw)
    assert (m.W, m.H) == (W, H)
    return m


@functools.lru_cache(maxsize=None)
def fields():
    """the whole-map fields of the base map, made by the library itself: clearance() and reach() per (not_free, inflate)"""
    _, log, _ = base_case()
    m = _base_map()
    m.upload_log(log)
    out = {}
    for not_free, inflate in MAPS:
        clear = m.clearance(max_radius=40, not_free=not_free)
        cost = m.reach([(40, 100), (150, 30)], max_cost=0xFFFE, inflate=inflate, not_free=not_free)
        assert clear.shape == cost.shape == (H, W) and (cost < 0xFFFF).sum() > 1000 and (clear < 0xFFFF).sum() > 1000
        out[(not_free, inflate)] = (clear, cost)
    m.close()
    return out


def test_the_base_case_contains_what_it_is_meant_to():
    """preconditions on the input, none on the device"""
    geo, log, blocked = base_case()
    want = rx.expect(geo, log, POSES, _arcs(CPW + 1, 256), _points(64), 255, blocked=blocked[(False, 0)])
    fh = want["first_hit"]
    assert (fh == 256).any() and (fh == 0).any() and ((fh > 0) & (fh < 64)).any() and ((fh >= 64) & (fh < 256)).any(), "no hit, at once, in the first pass, in a later one"
    assert len(np.unique(want["hit_point"])) > 8, "many points of the footprint are the first to collide"
    edge = rx.expect(geo, log, POSES, _arcs(CPW + 1, 64), _points(0), 255, blocked=blocked[(True, 0)])
    assert {int(f) & 7 for f in np.unique(edge["flags"])} >= {0, rx.OUTSIDE, rx.BLOCKED}
    assert (want[2]["flags"] & rx.START_BLOCKED).all() and (want[3]["flags"] & rx.START_BLOCKED).all() and not (want[0]["flags"] & rx.START_BLOCKED).any()
    assert (want[1]["start_x"] == 0).all() and (want[1]["start_y"] == 0).all() and (want[3]["start_x"] == -9).all() and (want[4]["start_x"] == 0).all()
    near = rx.expect(geo, log, POSES[:1], _arcs(CPW, 64), _points(1), 7, blocked=blocked[(False, 0)])
    assert ((near["flags"] & 7) == rx.RANGE).any(), "the range cuts an arc"
    assert not np.array_equal(blocked[(True, 0)], blocked[(False, 0)]) and blocked[(False, 3)].sum() > 3 * blocked[(False, 0)].sum()


@pytest.mark.parametrize("not_free,inflate", MAPS)
@pytest.mark.parametrize("form", ["lds", "GMS_ROLLOUT_WALK=mem"])
def test_base_case(form, not_free, inflate):
    geo, log, blocked = base_case()
    clear, cost = fields()[(not_free, inflate)]
    m = _with_walk("mem" in form, _base_map)
    m.upload_log(log)
    for i, (T, F, K, R, P) in enumerate(SHAPES):
        poses = POSES[(3 * i) % 9:][:3] if P == 3 else POSES[i:i + 1]
        arcs, pts = _arcs(K, T), _points(F)
        cl, co = (clear if i % 2 == 0 else None), (cost if i % 3 != 1 else None)
        want = rx.expect(geo, log, poses, arcs, pts, R, clear=cl, cost=co, blocked=blocked[(not_free, inflate)])
        got = m.rollout(poses, arcs, pts if F else None, max_range=R, inflate=inflate, not_free=not_free, clear=cl, cost=co)
        _same(got, want, f"{form}, not_free = {not_free}, inflate = {inflate}, T = {T}, F = {F}, K = {K}, max_range = {R}, P = {len(poses)}")
    m.close()


def test_every_pose_with_and_without_the_fields():
    geo, log, blocked = base_case()
    clear, cost = fields()[(True, 3)]
    m = _base_map()
    m.upload_log(log)
    arcs, pts = _arcs(2 * CPW + 1, 65), _points(64)
    for cl, co in ((clear, cost), (None, cost), (clear, None), (None, None)):
        want = rx.expect(geo, log, POSES, arcs, pts, 255, clear=cl, cost=co, blocked=blocked[(True, 3)])
        _same(m.rollout(POSES, arcs, pts, max_range=255, inflate=3, clear=cl, cost=co), want, f"clear {cl is not None}, cost {co is not None}")
    assert (want["min_d2"] == 0xFFFF).all() and (want["best_step"] == 0xFFFF).all()
    full = rx.expect(geo, log, POSES, arcs, pts, 255, clear=clear, cost=cost, blocked=blocked[(True, 3)])
    assert (full["min_d2"] < 0xFFFF).any() and ((full["best_step"] > 0) & (full["best_step"] < 0xFFFF)).any() and (full["end_cost"] < 0xFFFF).any()
    for bad in (dict(clear=clear[:-1]), dict(cost=cost.astype(np.int32))):
        with pytest.raises(ValueError):
            m.rollout(POSES, arcs, pts, **bad)
    m.close()


def test_a_non_square_map_with_a_far_origin():
    ox, oy = -37.5, 12.25
    g = orc.Grid(7.48, 4.23, RES, ox, oy)
    m = GridMap(7.48, 4.23, RES, (ox, oy), max_beams=360)
    assert (m.W, m.H) == (g.W, g.H) and m.W != m.H and m.W % 32 and m.H % 32
    rng = np.random.default_rng(15085)
    u = rng.random((m.H, m.W))
    log = np.where(u < 0.002, L_OCC, np.where(u < 0.995, L_FREE, 0.0))
    log[m.H // 2 - 10:m.H // 2 + 11, 10:50] = L_FREE
    m.upload_log(log)
    geo = rx.Geometry(m.W, m.H, RES, ox, oy)
    poses = np.array([[ox + 25.5 * RES, oy + (m.H // 2 + 0.5) * RES, 0.2], [ox + 0.01, oy + 0.01, 0.8], [ox + (m.W - 0.5) * RES, oy + (m.H - 0.5) * RES, -2.4],
                      [0.0, 0.0, 0.0]], np.float32)
    arcs, pts = _arcs(CPW + 1, 65, seconds=2.0), _points(9)
    for not_free, inflate, R in ((True, 0, 255), (False, 2, 30), (True, 1, 7)):
        want = rx.expect(geo, log, poses, arcs, pts, R, inflate, not_free)
        assert (want[0]["first_hit"] > 0).any() and (want[3]["flags"] == (rx.OUTSIDE | rx.START_BLOCKED)).all()
        _same(m.rollout(poses, arcs, pts, max_range=R, inflate=inflate, not_free=not_free), want, f"not_free = {not_free}, inflate = {inflate}, max_range = {R}")
    m.close()


def test_device_form_equals_the_host_form():
    import torch
    geo, log, blocked = base_case()
    clear, cost = fields()[(True, 3)]
    T, F, K, R, P = 65, 64, CPW + 1, 255, len(POSES)
    arcs, pts = _arcs(K, T), _points(F)
    m = _base_map()
    m.upload_log(log)
    host = m.rollout(POSES, arcs, pts, max_range=R, inflate=3, clear=clear, cost=cost)
    _same(host, rx.expect(geo, log, POSES, arcs, pts, R, clear=clear, cost=cost, blocked=blocked[(True, 3)]), "the host form")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_poses, d_arcs, d_pts = dev(POSES), dev(arcs), dev(pts)
    d_clear, d_cost = torch.from_numpy(clear.view(np.int16).copy()).to("cuda"), torch.from_numpy(cost.view(np.int16).copy()).to("cuda")
    out = torch.full((32 * P * K + 80,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0 and d_arcs.data_ptr() % 16 == 0
    torch.cuda.synchronize()                                                   # (the handle has a stream of its own)
    with pytest.raises(GmsError) as e:
        m.rollout_dev(d_poses.data_ptr(), P, d_arcs.data_ptr(), K, T, d_pts.data_ptr(), F, out[4:], max_range=R, inflate=3, clear=d_clear, cost=d_cost)
    assert e.value.code == GMS_ERR_INVALID
    m.synchronize(); torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all(), "a refused request writes nothing"
    m.rollout_dev(d_poses.data_ptr(), P, d_arcs.data_ptr(), K, T, d_pts.data_ptr(), F, out, max_range=R, inflate=3, clear=d_clear, cost=d_cost)
    m.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy()
    _same(raw[:32 * P * K].view(ROLLOUT_DTYPE).reshape(P, K), host, "the device form")
    assert (raw[32 * P * K:] == GUARD).all(), "bytes past the records"
    m.close()


def test_batched_handle_names_its_map():
    geo, log, blocked = base_case()
    m = _base_map(n_maps=3)
    logs = np.zeros((3, H, W))
    logs[1] = log
    logs[2] = L_FREE
    m.upload_log(logs)
    arcs, pts = _arcs(CPW, 64), _points(8)
    for mi, inflate in ((1, 0), (1, 3), (2, 3), (0, 0)):
        _same(m.rollout(POSES[:3], arcs, pts, max_range=60, inflate=inflate, mi=mi), rx.expect(geo, logs[mi], POSES[:3], arcs, pts, 60, inflate), f"map {mi}")
    assert (m.rollout(POSES[:1], arcs, pts, max_range=60, mi=0)["first_hit"] == 0).all(), "map 0 was never observed: a planner's mode blocks all of it"
    for bad in (-1, 3):
        with pytest.raises(GmsError) as e:
            m.rollout(POSES[:3], arcs, pts, mi=bad)
        assert e.value.code == GMS_ERR_INVALID
    m.close()


# ---- plane reuse and map changes -----------------------------------------------------------------------------------------------
def test_a_rollout_after_a_cast_packs_no_plane_and_one_after_an_update_sees_it():
    ext = 6.4
    tr = synth.make_trace(ext, RES, 180, T=6, seed=9)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=360)
    geo = rx.Geometry(m.W, m.H, RES, -ext / 2, -ext / 2)
    poses = np.concatenate([tr.poses[:3], [[0.9, -0.7, 2.0], [-2.9, 2.9, 0.0]]]).astype(np.float32)
    arcs, pts = _arcs(CPW + 1, 64, seconds=3.0), _points(12)
    m.update(tr.scans[0], tr.poses[0])
    m.cast(poses[:2], probe_fan(50, 3.0))
    builds = m.cast_plane_builds()
    first = m.rollout(poses, arcs, pts, max_range=80, not_free=False)
    assert m.cast_plane_builds() == builds, "the casts' plane is current: a rollout at inflate = 0 packs none"
    _same(first, rx.expect(geo, m.download_log(), poses, arcs, pts, 80, 0, False), "after the first update")
    assert (first["first_hit"] < 64).any() and (first["first_hit"] == 64).any()
    _same(m.rollout(poses, arcs, pts, max_range=80, not_free=False), first, "again")
    assert m.cast_plane_builds() == builds
    for k in (1, 2, 3):                                                        # the steady state: the last scan's apply pass is owed
        m.update(tr.scans[k], tr.poses[k])
    second = m.rollout(poses, arcs, pts, max_range=80, not_free=False)         # ... when the rollout comes, with no download in between
    assert m.cast_plane_builds() == builds + 1, "the moved map's plane is packed once"
    third = m.rollout(poses, arcs, pts, max_range=80, inflate=2)
    log = m.download_log()
    _same(second, rx.expect(geo, log, poses, arcs, pts, 80, 0, False), "after three more updates")
    _same(third, rx.expect(geo, log, poses, arcs, pts, 80, 2, True), "... inflated, in the planner's mode")
    assert not np.array_equal(first, second), "the scans changed what the arcs meet"
    m.close()


def test_a_handle_that_ran_rollouts_ends_bit_equal_to_a_twin_that_did_not():
    ext = 6.4
    tr = synth.make_trace(ext, RES, 180, T=6, seed=9)
    a, b = (GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=360) for _ in range(2))
    arcs, pts = _arcs(CPW + 1, 65, seconds=3.0), _points(12)
    for k in range(5):
        a.update(tr.scans[k], tr.poses[k])
        b.update(tr.scans[k], tr.poses[k])
        a.rollout(tr.poses[k:k + 2], arcs, pts, max_range=80, inflate=k % 3, not_free=bool(k % 2))
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    assert np.array_equal(bits(a.download_log()), bits(b.download_log()))
    assert np.array_equal(bits(a.download_likelihood()), bits(b.download_likelihood()))
    sc = tr.scans[5]
    probe = tr.poses[5:6]
    assert np.array_equal(a.cast(probe, probe_fan(90, 3.0)), b.cast(probe, probe_fan(90, 3.0)))
    a.update(sc, tr.poses[5]); b.update(sc, tr.poses[5])
    assert np.array_equal(bits(a.download_log()), bits(b.download_log()))
    a.close(); b.close()
