"""Map warps on the device at their edges (include/gridmapslam.h "map warps"): the cases of tests/_warp_edge_cases.py -- fine into
coarse and back, cell centres exactly on source cell edges, a ragged rectangle over them, ratios that are no power of two, finite
poses whose arithmetic overflows, (c, s) not quite unit -- through GridMap.warp_from for all four ops, against the restatement
(tests/_warp_expect.py) and, where there is one, the answer derived by hand.  Every comparison is array_equal on the doubles viewed
as uint64 and on the ten counters.  What the cases contain is asserted without a device in tests/test_warp_edge_inputs.py."""
import numpy as np
import pytest

import _warp_edge_cases as ec
import _warp_expect as wx
from gridmap_slam_robot_amd import WARP_STATS_DTYPE, GridMap, probe_fan
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in ec.cases()}


def _map(grid, log=None, **kw):
    m = GridMap(*ec.size_of(grid), grid[2], grid[3], **kw)
    assert wx.Geometry.of(m) == ec.geometry(grid), "the handle's grid is the case's"
    if log is not None:
        m.upload_log(log)
    return m


def _same(got, want, where):
    got_log, got_st = got
    want_log, want_st = want
    bad = np.argwhere(wx.bits(got_log) != wx.bits(want_log))
    assert len(bad) == 0, f"{where}: {len(bad)} of {want_log.size} cells differ, first at {bad[0].tolist()}: {got_log[tuple(bad[0])]!r} != {want_log[tuple(bad[0])]!r}"
    assert got_st.dtype == WARP_STATS_DTYPE and np.array_equal(got_st["pair"], want_st["pair"]) and got_st["n_outside"] == want_st["n_outside"], \
        f"{where}: {got_st} != {want_st}"


@pytest.mark.parametrize("name", ec.names())
def test_every_op_on_every_case(name):
    case = CASES[name]
    start = ec.start_log(case.dst)
    dst, src = _map(case.dst), _map(case.src, ec.source_log(case.src, case.seed))
    try:
        for op in ec.OPS:
            dst.upload_log(start)
            st = dst.warp_from(src, case.pose[:2], c=case.pose[2], s=case.pose[3], op=op, rect=case.rect, clamp=ec.ADD_CLAMP if op == "add" else 0.0)
            got = dst.download_log()
            _same((got, st), ec.expect(case, op), f"{name}, {op}")
            if case.hand is None:
                continue
            by_hand, n_outside = ec.by_hand(case)
            assert st["n_outside"] == n_outside, f"{name}, {op}: the count derived by hand"
            if op == "replace":
                assert np.array_equal(wx.bits(got), wx.bits(by_hand)), f"{name}: the slice derived by hand"
            if not case.hand[1].any():
                assert np.array_equal(wx.bits(got), wx.bits(start)) and st["pair"].sum() == 0, f"{name}, {op}: nothing inside, nothing written"
    finally:
        dst.close(); src.close()


def test_scale_beyond_the_bound_is_refused_with_nothing_touched():
    case = CASES["near-unit (c, s)"]
    start = ec.start_log(case.dst)
    dst, src = _map(case.dst, start), _map(case.src, ec.source_log(case.src, case.seed))
    pose = ec.near_unit_pose(ec.REFUSED_UNIT)
    try:
        for op in ec.OPS:
            with pytest.raises(GmsError) as e:
                dst.warp_from(src, pose[:2], c=pose[2], s=pose[3], op=op)
            assert e.value.code == GMS_ERR_INVALID
        assert np.array_equal(wx.bits(dst.download_log()), wx.bits(start))
    finally:
        dst.close(); src.close()


def test_add_and_fill_between_two_maps_of_a_batched_handle_behind_a_pending_update():
    """map 1 into a rectangle of map 2 of one GridMap(n_maps=3), on centres that sit on map 1's cell edges; update() has left its
    `logData +=` pass pending on the handle, so the source and the destination are both the applied values"""
    W, H, res, pos = ec.GRID
    rng = np.random.default_rng(31)
    logs = ec.VALUES[rng.integers(0, len(ec.VALUES), size=(3, H, W))]
    g = ec.geometry(ec.GRID)
    fan = probe_fan(90, 2.5)
    scans = np.stack([fan, fan[::-1], fan])
    robots = np.array([[4.0, 2.0, 0.4], [5.5, 1.0, -1.0], [3.0, 3.0, 2.0]], np.float32)
    rect = (5, 2, 64, 63)
    pose = CASES["half turn and half a cell"].pose
    outside = np.ones((H, W), bool)
    outside[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = False
    m, twin = _map(ec.GRID, n_maps=3), _map(ec.GRID, n_maps=3)
    try:
        for op, clamp in (("add", ec.ADD_CLAMP), ("fill", 0.0)):
            for h in (m, twin):
                h.upload_log(logs)
                h.update(scans, robots)
                h.update(scans, robots)
            st = m.warp_from(m, pose[:2], c=pose[2], s=pose[3], op=op, rect=rect, clamp=clamp, mi=2, src_mi=1)
            applied = twin.download_log()
            assert all(not np.array_equal(wx.bits(applied[i]), wx.bits(logs[i])) for i in range(3)), "the updates changed every map"
            got = m.download_log()
            want = wx.expect(applied[2], g, applied[1], g, pose, op, rect=rect, clamp=clamp)
            _same((got[2], st), want, f"map 1 into map 2, {op}")
            assert not np.array_equal(wx.bits(want[0]), wx.bits(applied[2])) and want[1]["n_outside"] == 0
            assert np.array_equal(wx.bits(got[:2]), wx.bits(applied[:2])), f"{op}: maps 0 and 1 are the applied values"
            assert np.array_equal(wx.bits(got[2])[outside], wx.bits(applied[2])[outside]), f"{op}: map 2 outside the rectangle"
    finally:
        m.close(); twin.close()
