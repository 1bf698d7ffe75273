"""Routes on the device (include/gridmapslam.h "routes"): gms_map_route[_dev] and gms_slam_route[_dev] against the definition restated in
Python (tests/_route_expect.py) and, for the cell lists, against gridmap.descend().  Every comparison is array_equal on whole arrays:
every result is an integer, there is no tolerance.  The fields come from GridMap.reach / clearance on the same handle.

The base map is 200 x 136 cells (the rollouts' and the cost-to-go fields'): ragged in 32- and 64-cell words, with NaN, 0.0 and -0.0
holes; the door of six cells in the wall y = 60 closes at inflate = 3."""
import ctypes as C
import functools

import numpy as np
import pytest

import _rollout_expect as rx
import _route_expect as rt
from gridmap_slam_robot_amd import ROUTE_DTYPE, GridMap, SLAMParticleMaps, cells_of_poses, descend, probe_fan, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError, GmsRoute, load, ptr

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
FAR = 0xFFFF
GUARD = 0xA5
MAPS = [(False, 0), (False, 3), (True, 0), (True, 3)]     # (not_free, inflate)
SEEDS = [(40, 100), (150, 30)]
# in the room (both halves, beside the door's wall), on a seed (the other one last), on a wall, off the map on each side, in the three holes, the corners
KINDS = [(45, 75), (150, 100), (160, 20), (40, 100), (10, 50), (120, 100), (-1, 50), (200, 50), (50, -1), (50, 136), (105, 35), (145, 85), (35, 97), (0, 0),
         (199, 135), (20, 62), (2, 61), (140, 40), (150, 30)]
STARTS = np.array(KINDS + [(13 + 21 * (i % 8), 14 + 17 * (i // 8)) for i in range(65 - len(KINDS))], np.int32)


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
    log[100, 120] = L_OCC                                                      # the start on a wall
    return log


def _base_map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=360, **kw)
    assert (m.W, m.H) == (W, H)
    return m


@functools.lru_cache(maxsize=None)
def base_case():
    """(logData, {(not_free, inflate): (blocked plane, clear field, cost field)}): the planes restated, the fields the library's own"""
    log = _base_log()
    log.flags.writeable = False
    m = _base_map()
    m.upload_log(log)
    out = {}
    for not_free, inflate in MAPS:
        clear = m.clearance(max_radius=40, not_free=not_free)
        cost = m.reach(SEEDS, max_cost=0xFFFE, inflate=inflate, not_free=not_free)
        assert clear.shape == cost.shape == (H, W) and (cost < FAR).sum() > 1000
        for a in (clear, cost):
            a.flags.writeable = False
        out[(not_free, inflate)] = (rx.blocked_plane(log, inflate, not_free), clear, cost)
    m.close()
    return log, out


@functools.lru_cache(maxsize=None)
def loaded_map():
    """one handle with the base map for the tests that only read it"""
    m = _base_map()
    m.upload_log(base_case()[0])
    return m


def _arrays(rec, ways, paths, max_waypoints, max_cells, fill=0):
    """what the outputs hold: the lists in front of the counts, `fill` behind them"""
    w = np.full((len(rec), max_waypoints, 2), fill, np.int32)
    c = np.full((len(rec), max_cells, 2), fill, np.int32)
    for p in range(len(rec)):
        w[p, :len(ways[p])] = np.asarray(ways[p], np.int32).reshape(-1, 2)
        c[p, :len(paths[p])] = np.asarray(paths[p], np.int32).reshape(-1, 2)
    return w, c


def _same(got, want, where):
    rec, ways = got[0], got[1]
    wrec, wways, wcells = want
    assert rec.dtype == ROUTE_DTYPE and rec.shape == wrec.shape, where
    bad = np.argwhere(rec != wrec)
    assert np.array_equal(rec, wrec), f"{where}: {len(bad)} of {wrec.size} records differ, first at {bad[:1].tolist()}: {rec[tuple(bad[0])]} != {wrec[tuple(bad[0])]}"
    assert np.array_equal(ways, wways), f"{where}: waypoints of starts {sorted(set(np.argwhere(ways != wways)[:, 0].tolist()))[:8]}"
    if len(got) > 2:
        assert np.array_equal(got[2], wcells), f"{where}: cells of starts {sorted(set(np.argwhere(got[2] != wcells)[:, 0].tolist()))[:8]}"


def _want(key, starts, look, max_cells, max_waypoints, clear=True, field=None, blocked=None):
    plane, cl, cost = base_case()[1][key]
    rec, ways, paths = rt.expect(cost if field is None else field, plane if blocked is None else blocked, starts, look, max_cells, max_waypoints, cl if clear else None)
    return (rec,) + _arrays(rec, ways, paths, max_waypoints, max_cells), ways, paths


@pytest.mark.parametrize("P", [1, 3, 65])
@pytest.mark.parametrize("not_free,inflate", MAPS)
def test_every_kind_of_start_in_every_mode(not_free, inflate, P):
    key = (not_free, inflate)
    starts = STARTS[[0, 3, 4][:P]] if P <= 3 else STARTS[:P]                  # P <= 3: in the room, on a seed, on a wall
    want, ways, paths = _want(key, starts, 64, 512, 48)
    rec = want[0]
    m = loaded_map()
    got = m.route(base_case()[1][key][2], starts, look=64, inflate=inflate, not_free=not_free, max_cells=512, max_waypoints=48, clear=base_case()[1][key][1],
                  cells=True)
    _same(got, want, f"{key} P = {P}")
    for p, s in enumerate(starts):
        assert paths[p] == descend(base_case()[1][key][2], s), f"start {s}: the whole staircase is descend()'s"
    assert ((rec["flags"] | rt.NO_PATH) == rt.NO_PATH).all(), "a field of this map and these arguments: no cut, not broken, no mismatch"
    if P == 65:
        assert (rec["n_cells"] > 64).any() and (rec["n_waypoints"] > 2).any() and (rec["n_cells"] == 0).sum() >= 6
        on_seed = [p for p in range(P) if base_case()[1][key][2][starts[p][1] % H, starts[p][0] % W] == 0 and rec["n_cells"][p]]
        assert on_seed and all((rec[p]["n_cells"], rec[p]["n_waypoints"], rec[p]["end_cost"], rec[p]["flags"]) == (1, 1, 0, 0) for p in on_seed)
        assert (rec["flags"][[4, 5, 6, 7, 8, 9]] == rt.NO_PATH).all(), "on a wall and off the map on each side"
        if inflate == 0:
            assert (rec["flags"][[10, 11, 12]] == (rt.NO_PATH if not_free else 0)).all(), "never observed, NaN and -0.0 block a planner's mode alone"
        ties = [p for p in range(P) if paths[p] and sum(base_case()[1][key][1][y, x] == rec["min_d2"][p] for x, y in paths[p]) > 1]
        assert ties, "a minimum of the clearance that is taken twice"
    none = m.route(base_case()[1][key][2], starts, look=64, inflate=inflate, not_free=not_free, max_cells=512, max_waypoints=48)
    assert len(none) == 2
    _same(none, _want(key, starts, 64, 512, 48, clear=False)[0], "without a clearance field")
    assert (none[0]["min_d2"] == FAR).all() and (none[0]["min_d2_at"] == 0).all()


@pytest.mark.parametrize("look", [1, 63, 64, 65, 4096])
def test_paths_at_the_edges_of_a_pass_of_64(look):
    """the free strip along the top edge is a corridor of ten rows: from (12 + n - 1, 130) the descent to a seed at (12, 130) runs straight
    west, n cells"""
    plane, clear, _ = base_case()[1][(True, 0)]
    m = loaded_map()
    cost = m.reach([(12, 130)], max_cost=0xFFFE, inflate=0, not_free=True)
    starts = np.array([(12 + n - 1, 130) for n in (63, 64, 65, 128, 129)] + [(199, 135), (60, 126), (150, 100)], np.int32)
    rec, ways, paths = rt.expect(cost, plane, starts, look, 256, 256, clear)
    assert rec["n_cells"].tolist()[:5] == [63, 64, 65, 128, 129] and rec["n_cells"][5] > 129 and rec["flags"].tolist() == [0] * 7 + [rt.NO_PATH]
    got = m.route(cost, starts, look=look, inflate=0, not_free=True, max_cells=256, max_waypoints=256, clear=clear, cells=True)
    _same(got, (rec,) + _arrays(rec, ways, paths, 256, 256), f"look = {look}")
    if look == 1:
        assert np.array_equal(got[1], got[2]) and np.array_equal(got[0]["n_waypoints"], got[0]["n_cells"]), "look = 1: the waypoints are the cells"
    else:
        assert (got[0]["n_waypoints"][:7] < got[0]["n_cells"][:7]).all()
        assert got[0]["n_waypoints"][:5].tolist() == [1 + -(-(n - 1) // look) for n in (63, 64, 65, 128, 129)], "straight legs of `look` cells"


def test_cuts_appear_exactly_where_they_should():
    key = (True, 3)
    start = np.array([(150, 100)], np.int32)
    plane, clear, cost = base_case()[1][key]
    full, ways, paths = _want(key, start, 16, 512, 512)
    n, nw = len(paths[0]), len(ways[0])
    assert n > 70 and nw > 5 and full[0]["flags"][0] == 0
    m = loaded_map()
    for max_cells, flag in ((n - 1, rt.CELLS_CUT), (n, 0), (n + 1, 0)):
        want = _want(key, start, 16, max_cells, max_cells)[0]
        got = m.route(cost, start, look=16, inflate=3, not_free=True, max_cells=max_cells, max_waypoints=max_cells, clear=clear, cells=True)
        _same(got, want, f"max_cells = {max_cells}")
        assert got[0]["flags"][0] == flag and got[0]["n_cells"][0] == min(n, max_cells)
    for max_wp, flag in ((1, rt.WAYPOINTS_CUT), (nw - 1, rt.WAYPOINTS_CUT), (nw, 0), (nw + 1, 0)):
        want = _want(key, start, 16, 512, max_wp)[0]
        got = m.route(cost, start, look=16, inflate=3, not_free=True, max_cells=512, max_waypoints=max_wp, clear=clear, cells=True)
        _same(got, want, f"max_waypoints = {max_wp}")
        assert got[0]["flags"][0] == flag and got[0]["n_waypoints"][0] == min(nw, max_wp) and got[0]["n_cells"][0] == n


def test_device_forms_equal_the_host_forms_and_leave_the_guard():
    import torch
    key = (True, 3)
    plane, clear, cost = base_case()[1][key]
    P, max_cells, max_wp = 65, 100, 10
    want = _want(key, STARTS, 8, max_cells, max_wp)[0]
    assert all(0 < (want[0]["flags"] & f != 0).sum() < P for f in (rt.WAYPOINTS_CUT, rt.CELLS_CUT, rt.NO_PATH)), "cut and whole lists, and none"
    m = loaded_map()
    req = GmsRoute(max_cells, max_wp, 8, 3, 1, 0)
    # the host form of the C-ABI on the caller's own buffers: what lies behind the counts stays
    rec = np.zeros(P, ROUTE_DTYPE)
    ways = np.full((P, max_wp, 2), GUARD * 0x01010101, np.uint32).view(np.int32)
    cells = np.full((P, max_cells, 2), GUARD * 0x01010101, np.uint32).view(np.int32)
    assert load().gms_map_route(m._h, 0, C.byref(req), ptr(STARTS), P, ptr(cost), ptr(clear), ptr(rec), ptr(ways), ptr(cells)) == 0
    guarded = (want[0],) + _arrays(want[0], *_want(key, STARTS, 8, max_cells, max_wp)[1:], max_wp, max_cells, fill=np.int32(np.uint32(GUARD * 0x01010101).view(np.int32)))
    _same((rec, ways, cells), guarded, "the host form on guarded buffers")
    # the device form
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_cost, d_clear, d_starts = dev(cost).view(torch.int16), dev(clear).view(torch.int16), dev(STARTS).view(torch.int32)
    d_rec = torch.full((32 * P + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_ways = torch.full((8 * P * max_wp + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_cells = torch.full((8 * P * max_cells + 64,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                                   # (the handle has a stream of its own)
    kw = dict(look=8, inflate=3, not_free=True, max_cells=max_cells, max_waypoints=max_wp)
    with pytest.raises(GmsError) as e:
        m.route_dev(d_cost, d_starts, d_rec[4:], d_ways.view(torch.int32), clear=d_clear, cells=d_cells.view(torch.int32), **kw)
    assert e.value.code == GMS_ERR_INVALID
    m.synchronize(); torch.cuda.synchronize()
    assert all((t.cpu().numpy() == GUARD).all() for t in (d_rec, d_ways, d_cells)), "a refused request writes nothing"
    for with_cells in (True, False):                                           # the path in the caller's cells, and in the handle's scratch
        d_rec.fill_(GUARD); d_ways.fill_(GUARD)
        torch.cuda.synchronize()
        m.route_dev(d_cost, d_starts, d_rec, d_ways.view(torch.int32), clear=d_clear, cells=d_cells.view(torch.int32) if with_cells else None, **kw)
        m.synchronize(); torch.cuda.synchronize()
        raw = [t.cpu().numpy() for t in (d_rec, d_ways, d_cells)]
        got = (raw[0][:32 * P].view(ROUTE_DTYPE), raw[1][:8 * P * max_wp].view(np.int32).reshape(P, max_wp, 2), raw[2][:8 * P * max_cells].view(np.int32).reshape(P, max_cells, 2))
        _same(got, guarded, f"the device form, cells {with_cells}")
        assert (raw[0][32 * P:] == GUARD).all() and (raw[1][8 * P * max_wp:] == GUARD).all() and (raw[2][8 * P * max_cells:] == GUARD).all(), "bytes past the outputs"


def test_a_field_of_another_inflation_is_flagged_past_the_door():
    """the field of inflate = 0 leads through the door in the wall y = 60, six cells wide; at inflate = 3 the door is closed"""
    plane0, clear, cost0 = base_case()[1][(True, 0)]
    plane3 = base_case()[1][(True, 3)][0]
    assert plane3[60, 130:136].all() and not plane0[60, 130:136].any()
    starts = np.array([(125, 78), (150, 100), (133, 63), (45, 75)], np.int32)
    rec, ways, paths = rt.expect(cost0, plane3, starts, 64, 512, 512, clear)
    assert (rec["flags"][:3] == rt.MISMATCH).all() and all(60 in [y for _, y in p] for p in paths[:3]), "three starts above the wall, their seed below it"
    got = loaded_map().route(cost0, starts, look=64, inflate=3, not_free=True, max_cells=512, max_waypoints=512, clear=clear, cells=True)
    _same(got, (rec,) + _arrays(rec, ways, paths, 512, 512), "inflate = 0's field at inflate = 3")


def test_a_field_that_is_no_cost_to_go_field_is_flagged():
    key = (True, 0)
    plane, clear, cost = base_case()[1][key]
    starts = np.array([(150, 100), (160, 20), (45, 75)], np.int32)
    path = descend(cost, starts[0])
    assert len(path) > 40
    for k in range(20, len(path)):                                             # a cell of the first start's path, raised by 1, that leaves no other way on
        bad = cost.copy()
        bad[path[k][1], path[k][0]] += 1
        if rt.descent(bad, starts[0], 512)[1] == rt.BROKEN:
            break
    rec, ways, paths = rt.expect(bad, plane, starts, 64, 512, 64, clear)
    assert rec["flags"][0] == rt.BROKEN and rec["n_cells"][0] == k and paths[0] == path[:k] and rec["end_cost"][0] == cost[path[k - 1][1], path[k - 1][0]]
    assert (rec["flags"][1:] == 0).all()
    got = loaded_map().route(bad, starts, look=64, inflate=0, not_free=True, max_cells=512, max_waypoints=64, clear=clear, cells=True)
    _same(got, (rec,) + _arrays(rec, ways, paths, 64, 512), "one cell raised")


def test_batched_handle_names_its_map():
    log, cases = base_case()
    m = _base_map(n_maps=3)
    logs = np.zeros((3, H, W))
    logs[1] = log
    logs[2] = L_FREE
    m.upload_log(logs)
    for key in ((True, 3), (False, 0)):
        not_free, inflate = key
        cost = m.reach(SEEDS, inflate=inflate, not_free=not_free, mi=1)
        assert np.array_equal(cost, cases[key][2])
        got = m.route(cost, STARTS[:9], look=4096, inflate=inflate, not_free=not_free, max_cells=400, max_waypoints=40, cells=True, mi=1)
        _same(got, _want(key, STARTS[:9], 4096, 400, 40, clear=False)[0], f"map 1 {key}")
    open_cost = m.reach(SEEDS, inflate=3, not_free=True, mi=2)
    rec, ways = m.route(open_cost, [(190, 130)], look=4096, inflate=3, max_cells=400, max_waypoints=40, mi=2)
    assert rec["n_waypoints"][0] == 2 and rec["flags"][0] == 0 and ways[0, 1].tolist() in [list(s) for s in SEEDS], "an empty map: one leg"
    for bad in (-1, 3):
        with pytest.raises(GmsError) as e:
            m.route(open_cost, [(5, 5)], mi=bad)
        assert e.value.code == GMS_ERR_INVALID
    m.close()


def test_a_route_sees_the_map_as_it_stands_and_changes_nothing():
    ext = 6.4
    tr = synth.make_trace(ext, RES, 180, T=6, seed=9)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=360)
    gx, gy = cells_of_poses(tr.poses[:1], (-ext / 2, -ext / 2), RES)
    seed = [(int(gx[0]), int(gy[0]))]
    starts = np.array([(x, y) for y in range(8, 128, 17) for x in range(8, 128, 17)], np.int32)

    def check(where, inflate=0, not_free=False):
        cost = m.reach(seed, inflate=inflate, not_free=not_free)
        got = m.route(cost, starts, look=64, inflate=inflate, not_free=not_free, max_cells=600, max_waypoints=64, cells=True)
        rec, ways, paths = rt.expect(cost, rx.blocked_plane(m.download_log(), inflate, not_free), starts, 64, 600, 64)
        _same(got, (rec,) + _arrays(rec, ways, paths, 64, 600), where)
        assert ((rec["flags"] | rt.NO_PATH) == rt.NO_PATH).all(), "a fresh field and a fresh plane never mismatch"
        return cost, got

    m.update(tr.scans[0], tr.poses[0])
    m.cast(tr.poses[:2], probe_fan(50, 3.0))
    builds = m.cast_plane_builds()
    cost, first = check("after the first update")
    assert m.cast_plane_builds() == builds, "the casts' plane is current: a route at inflate = 0 packs none"
    assert (first[0]["n_cells"] > 1).sum() > 3
    check("inflated, in the planner's mode", 2, True)
    assert np.array_equal(m.reach(seed, inflate=0, not_free=False), cost), "a following reach returns what it returned before"
    assert m.cast_plane_builds() == builds
    for k in (1, 2, 3):                                                        # the steady state: the last scan's apply pass is owed
        m.update(tr.scans[k], tr.poses[k])
    stale = m.route(cost, starts, look=64, inflate=0, not_free=False, max_cells=600, max_waypoints=64, cells=True)
    assert m.cast_plane_builds() == builds + 1, "the moved map's plane is packed once"
    assert np.array_equal(stale[2], first[2]), "the old field still descends as it did"
    _, second = check("after three more updates")
    assert m.cast_plane_builds() == builds + 1
    assert not np.array_equal(first[0], second[0]), "the scans changed where the routes go"
    m.close()


def _far_free_cell(log, inflate, not_free, own):
    """the known-free cell that is not blocked and lies farthest from `own` (the first of them): a seed the particle can be routed to"""
    ok = np.argwhere(~rx.blocked_plane(log, inflate, not_free) & (np.asarray(log) < 0))
    assert len(ok) > 50
    y, x = ok[np.argmax((ok[:, 1] - int(own[0])) ** 2 + (ok[:, 0] - int(own[1])) ** 2)]
    return [(int(x), int(y))]


def test_a_particles_own_map_and_its_own_cell():
    ext, n = 6.0, 12
    s = SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=300)
    tr = synth.make_trace(ext, RES, 90, T=8, seed=23)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    dummy = np.full((s.H, s.W), FAR, np.uint16)
    with pytest.raises(GmsError) as e:
        s.route(dummy)
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    for k in range(3):
        s.update(tr.scans[k], (0.02, 0.1), seed=5, sequence=k)
        if k == 1:
            s.resample(0.37)
    poses = s.pf.get_poses()
    strongest = s.view("strongest")[1]
    starts = np.array([(x, y) for y in range(10, 120, 25) for x in range(10, 120, 25)], np.int32)
    for which in (4, "strongest"):
        k = strongest if which == "strongest" else which
        log = s.map_of(k)
        gx, gy = cells_of_poses(poses[k:k + 1], (-ext / 2, -ext / 2), RES)
        own = np.array([(gx[0], gy[0])], np.int32)
        for inflate, not_free in ((0, False), (2, True)):
            blocked = rx.blocked_plane(log, inflate, not_free)
            home, shown = s.reach(which, max_cost=0xFFFE, inflate=inflate, not_free=not_free)      # seeded at the particle's own cell
            assert shown == k
            got = s.route(home, starts, which, look=64, inflate=inflate, not_free=not_free, max_cells=400, max_waypoints=40, cells=True)
            assert got[3] == k
            rec, ways, paths = rt.expect(home, blocked, starts, 64, 400, 40)
            _same(got[:3], (rec,) + _arrays(rec, ways, paths, 40, 400), f"particle {which} from the caller's starts")
            # the pose mode: on its own seed the route is that one cell; over a field seeded elsewhere it leads there
            rec1, ways1, cells1, shown = s.route(home, None, which, inflate=inflate, not_free=not_free, max_cells=400, max_waypoints=40, cells=True)
            assert shown == k and rec1.shape == (1,)
            if not blocked[own[0, 1], own[0, 0]]:
                assert (rec1["n_cells"][0], rec1["n_waypoints"][0], rec1["flags"][0]) == (1, 1, 0)
            assert (rec1["end_x"][0], rec1["end_y"][0]) == (own[0, 0], own[0, 1]), "the shown particle's cell is cells_of_poses of its pose"
            away = s.reach(which, seeds=_far_free_cell(log, inflate, not_free, own[0]), inflate=inflate, not_free=not_free)[0]
            got = s.route(away, None, which, inflate=inflate, not_free=not_free, max_cells=400, max_waypoints=40, cells=True)
            rec, ways, paths = rt.expect(away, blocked, own, 64, 400, 40)
            assert inflate or (rec["n_cells"][0] > 10 and rec["flags"][0] == 0), "the particle stands in the room it mapped: a route of some length"
            _same(got[:3], (rec,) + _arrays(rec, ways, paths, 40, 400), f"particle {which} from its own cell")
    for bad in (-2, n):
        with pytest.raises(GmsError) as e:
            s.route(dummy, starts, which=bad)
        assert e.value.code == GMS_ERR_INVALID
    s.close()


def _slam_route_dev(h, field, starts, max_cells, max_wp, **kw):
    """route_dev of a gms_slam handle into guard-filled tensors with shown_out given: (records, waypoints, cells, the shown words);
    what lies behind the counts must come back as the guard, so the arrays are compared whole against guard-filled expectations"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    n = 1 if starts is None else len(starts)
    d_field = dev(field).view(torch.int16)
    d_starts = None if starts is None else dev(np.asarray(starts, np.int32)).view(torch.int32)
    d_rec = torch.full((32 * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_ways = torch.full((8 * n * max_wp + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_cells = torch.full((8 * n * max_cells + 64,), GUARD, dtype=torch.uint8, device="cuda")
    shw = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                                   # (the handle has a stream of its own)
    got = h.route_dev(d_field, d_rec, d_ways.view(torch.int32), d_starts, max_cells=max_cells, max_waypoints=max_wp, cells=d_cells.view(torch.int32), shown_out=shw, **kw)
    assert len(got) == 4 and got[3] is shw
    h.grid_map.synchronize(); torch.cuda.synchronize()
    raw = [t.cpu().numpy() for t in (d_rec, d_ways, d_cells)]
    assert (raw[0][32 * n:] == GUARD).all() and (raw[1][8 * n * max_wp:] == GUARD).all() and (raw[2][8 * n * max_cells:] == GUARD).all(), "bytes past the outputs"
    return (raw[0][:32 * n].view(ROUTE_DTYPE), raw[1][:8 * n * max_wp].view(np.int32).reshape(n, max_wp, 2),
            raw[2][:8 * n * max_cells].view(np.int32).reshape(n, max_cells, 2), shw.cpu().tolist())


def _guarded(host, max_wp, max_cells):
    """a host form's (records, waypoints, cells) with the guard word behind the counts instead of the host form's zeros"""
    rec, ways, cells = (a.copy() for a in host[:3])
    word = np.uint32(GUARD * 0x01010101).view(np.int32)
    for p in range(len(rec)):
        ways[p, rec["n_waypoints"][p]:] = word
        cells[p, rec["n_cells"][p]:] = word
    return rec, ways, cells


def test_a_particles_device_forms_equal_its_host_forms():
    ext, n = 6.0, 12
    s = SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=300)
    tr = synth.make_trace(ext, RES, 90, T=8, seed=23)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    for k in range(3):
        s.update(tr.scans[k], (0.02, 0.1), seed=5, sequence=k)
        if k == 1:
            s.resample(0.37)
    strongest = s.view("strongest")[1]
    starts = np.array([(x, y) for y in range(10, 120, 25) for x in range(10, 120, 25)], np.int32)
    poses = s.pf.get_poses()
    for which in (4, "strongest"):
        k = strongest if which == "strongest" else which
        gx, gy = cells_of_poses(poses[k:k + 1], (-ext / 2, -ext / 2), RES)
        for inflate, not_free in ((0, False), (2, True)):
            kw = dict(which=which, look=64, inflate=inflate, not_free=not_free)
            away = s.reach(which, seeds=_far_free_cell(s.map_of(k), inflate, not_free, (gx[0], gy[0])), inflate=inflate, not_free=not_free)[0]
            for st in (starts, None):                                          # the caller's starts, and the shown particle's own cell
                host = s.route(away, st, max_cells=400, max_waypoints=40, cells=True, **kw)
                assert host[3] == k
                got = _slam_route_dev(s, away, st, 400, 40, **kw)
                _same(got[:3], _guarded(host, 40, 400), f"particle {which}, starts {'given' if st is not None else 'its own cell'}, {kw}")
                assert got[3] == [k, -7, -7, -7], "the shown word, and nothing behind it"
                assert inflate or (host[0]["n_cells"] > 10).any(), "routes of some length, from the starts and from the particle's own cell"
    s.close()


def test_a_batched_filters_routes_name_their_filter():
    from gridmap_slam_robot_amd import SLAMParticleMapsBatch
    ext, S, n = 6.0, 3, 4
    tr = synth.make_trace(ext, RES, 90, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=300)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    dummy = np.full((bat.H, bat.W), FAR, np.uint16)
    with pytest.raises(GmsError) as e:
        bat.route(dummy, filter=1)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [(0.02, 0.1)] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    starts = np.array([(x, y) for y in range(10, 120, 25) for x in range(10, 120, 25)], np.int32)
    poses = bat.pf.get_poses().reshape(-1, 3)
    for which, f in (("strongest", 1), (3, 0), (1, 2)):
        field, shown = bat.reach(which, filter=f, not_free=False)              # seeded at the shown particle's own cell
        assert f * n <= shown < (f + 1) * n and (which == "strongest" or shown == f * n + which)
        blocked = rx.blocked_plane(bat.map_of(f, shown - f * n), 0, False)
        gx, gy = cells_of_poses(poses[shown:shown + 1], (-ext / 2, -ext / 2), RES)
        assert field[gy[0], gx[0]] == 0, "the field's seed is the shown particle's cell"
        kw = dict(which=which, filter=f, look=64, inflate=0, not_free=False)
        host = bat.route(field, starts, max_cells=400, max_waypoints=40, cells=True, **kw)
        rec, ways, paths = rt.expect(field, blocked, starts, 64, 400, 40)
        assert host[3] == shown and (rec["n_cells"] > 1).any()
        _same(host[:3], (rec,) + _arrays(rec, ways, paths, 40, 400), f"filter {f}, particle {which}")
        own = bat.route(field, None, max_cells=400, max_waypoints=40, cells=True, **kw)
        assert own[3] == shown and (own[0]["n_cells"][0], own[0]["end_x"][0], own[0]["end_y"][0]) == (1, gx[0], gy[0]), "its own cell is the seed"
        for st, h in ((starts, host), (None, own)):
            got = _slam_route_dev(bat, field, st, 400, 40, **kw)
            _same(got[:3], _guarded(h, 40, 400), f"filter {f}, particle {which}, the device form")
            assert got[3] == [shown, -7, -7, -7]
    with pytest.raises(IndexError):
        bat.route(dummy, starts, filter=S)
    bat.close()


def test_a_far_end_hidden_behind_a_wall_takes_more_than_one_pass():
    """the inner wall x = 70 stands between the starts west of it and the seed (150, 30): the descent runs north along the wall, through
    the gap above y = 90 and back south, so from most path cells the far end of a window of 129 or more cells lies behind the wall and
    the search has to go on to the next 64 candidates"""
    key = (True, 0)
    plane, clear, _ = base_case()[1][key]
    m = loaded_map()
    cost = m.reach([(150, 30)], max_cost=0xFFFE, inflate=0, not_free=True)
    starts = np.array([(60, 20), (30, 15), (65, 50), (15, 85), (60, 40), (40, 30)], np.int32)
    for look in (129, 200, 4096):
        rec, ways, paths = rt.expect(cost, plane, starts, look, 512, 64, clear)
        assert (rec["n_cells"] > 120).all() and (rec["flags"] == 0).all()
        hidden = 0                                                             # searches whose first 64 candidates are all hidden
        for w, p in zip(ways, paths):
            for a in w[:-1]:
                i = p.index(a)
                top = min(i + look, len(p) - 1)
                hidden += top - i > 64 and not any(rt.visible_box(plane, a, p[j]) for j in range(top, top - 64, -1))
        assert hidden >= 6, "the pull's second pass is taken"
        got = m.route(cost, starts, look=look, inflate=0, not_free=True, max_cells=512, max_waypoints=64, clear=clear, cells=True)
        _same(got, (rec,) + _arrays(rec, ways, paths, 64, 512), f"behind the wall, look = {look}")
