"""View gain of the shared maps on the device (include/gridmapslam.h "view gain"): gms_map_gain[_dev] against records built from the
oracle's own ray set-up and cell walk (tests/_gain_expect.py).  Every comparison is array_equal on the whole record array: the
feature is all-integer, there is no tolerance.  A gain must see the map as a download would return it at that moment.

The base map is 200 x 136 cells (the cost-to-go fields' size): ragged in 32- and 64-cell words."""
import functools
import math
import os

import numpy as np
import pytest

import _gain_expect as gx
from gridmap_slam_robot_amd import GAIN_DTYPE, GridMap, probe_fan, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78
LW, LH = 600, 520
LWM, LHM = 29.98, 25.98
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
BS = (1, 255, 256, 300, 720)                           # k_gain's workgroup is 256 lanes: below, at and above it, and the strided loop
RANGES = (1, 7, 64, 255)
GUARD = 0xA5


def _same(got, want, where=""):
    assert got.dtype == GAIN_DTYPE and got.shape == want.shape, where
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), f"{where}: {len(bad)} of {want.size} records differ, first at {bad[:1].tolist()}: {got[bad[:1]]} != {want[bad[:1]]}"


def _with_walk(mem, make):
    old = os.environ.pop("GMS_GAIN_WALK", None)
    if mem:
        os.environ["GMS_GAIN_WALK"] = "mem"                                # read when the handle is created
    try:
        return make()
    finally:
        os.environ.pop("GMS_GAIN_WALK", None)
        if old is not None:
            os.environ["GMS_GAIN_WALK"] = old


def _fan(n, lengths):
    """n evenly spaced probes over the full circle whose lengths (metres) cycle through `lengths`"""
    f = probe_fan(n, 1.0)
    d = np.resize(np.asarray(lengths, dtype=np.float64), n)
    f["local_x"] *= d
    f["local_y"] *= d
    f["distance"] = d
    return f


def _cell_pose(cx, cy, theta, fx=0.5, fy=0.5):
    """a pose in cell (cx, cy), the fraction (fx, fy) of a cell from its lower corner: the walks start in floor(pose / RES + 0.5)"""
    return [(cx + fx - 0.5) * RES, (cy + fy - 0.5) * RES, theta]


def _base_log():
    rng = np.random.default_rng(200136)
    log = np.zeros((H, W))                                                     # never observed
    log[10:121, 10:181] = L_FREE                                               # a room ...
    log[10, 10:181] = log[120, 10:181] = L_OCC                                 # ... with walls,
    log[10:121, 10] = log[10:121, 180] = L_OCC
    log[60:64, 10] = L_FREE                                                    # a door in the west wall,
    log[60:64, 0:10] = L_FREE                                                  # a passage from it to the map's edge,
    log[10:90, 70] = L_OCC                                                     # an inner wall with a gap at its end,
    log[60, 100:181] = L_OCC
    log[60, 130:136] = L_FREE
    log[126:136, :] = L_FREE                                                   # a free strip along the top edge, corner to corner
    room = np.zeros((H, W), bool)
    room[11:120, 11:180] = True
    log[room & (rng.random((H, W)) < 0.01)] = L_OCC                            # clutter
    log[30:40, 100:112] = 0.0                                                  # holes in the room: never observed,
    log[80:90, 140:150] = np.nan                                               # NaN
    log[95:100, 30:44] = -0.0                                                  # and -0.0
    log[100, 120] = L_OCC                                                      # the pose on a wall
    return log


@functools.lru_cache(maxsize=None)
def base_case():
    """(grid, logData [136][200], poses [40][3], probes [720], {(B, max_range): (records [40], walked cells summed over the probes)})"""
    g = orc.Grid(WM, HM, RES, 0.0, 0.0)
    assert (g.W, g.H) == (W, H)
    log = _base_log()
    rng = np.random.default_rng(40)
    poses = [_cell_pose(0, 0, 0.3), _cell_pose(199, 0, 2.0), _cell_pose(0, 135, -1.0), _cell_pose(199, 135, -2.5),        # the map's corners
             _cell_pose(100, 0, 1.2), _cell_pose(0, 62, 0.0), _cell_pose(199, 130, 3.0), _cell_pose(100, 135, -1.6),     # ... and edges
             _cell_pose(50, 30, 0.0), _cell_pose(100, 90, math.pi / 2),            # max_range 7: x0 = 43; 64: x0 = 36 -- neither on a word boundary
             _cell_pose(32, 64, math.pi, fx=0.01, fy=0.01), _cell_pose(64, 32, -math.pi / 2, fx=0.99, fy=0.99),       # on word boundaries, at the cells' edges
             [-0.5, 3.0, 0.0], [11.0, 3.0, 1.0], [5.0, 7.5, 2.0], [5.0, -0.03, 2.0],                                    # outside the map
             _cell_pose(120, 100, 0.7), _cell_pose(70, 40, 0.0),                   # on a wall cell
             _cell_pose(150, 100, 1.0), _cell_pose(150, 100, 1.0),                 # twice the same
             _cell_pose(105, 35, 0.5), _cell_pose(144, 85, -0.5), _cell_pose(35, 97, 2.2)]                           # inside the never-observed holes
    n_rand = 40 - len(poses)
    xy = np.column_stack([rng.uniform(0.0, WM, n_rand), rng.uniform(0.0, HM, n_rand)])
    th = np.concatenate([[0.4, 2.0, -2.0, -0.4], rng.uniform(-math.pi, math.pi, n_rand - 4)])                         # every quadrant
    poses = np.array(poses + np.column_stack([xy, th]).tolist(), dtype=np.float32)
    assert poses.shape == (40, 3)
    probes = _fan(720, [13.0, 2.0, 0.6, 5.0, 0.04])                        # longer than max_range 255, down to inside the start cell
    walks = [gx.Walks(g, probes, p) for p in poses]
    want = {}
    for B in BS:
        for R in RANGES:
            recs = [w.record(log, R, B) for w in walks]
            want[(B, R)] = (np.array([r for r, _ in recs], dtype=GAIN_DTYPE), sum(t for _, t in recs))
    log.flags.writeable = False
    return g, log, poses, probes, want


def _base_map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=720, **kw)
    assert (m.W, m.H) == (W, H)
    return m


def test_the_base_case_contains_what_it_is_meant_to():
    """preconditions on the input, none on the device"""
    g, log, poses, probes, want = base_case()
    for R in RANGES:
        rec, total = want[(720, R)]
        distinct = int(rec["unknown"].sum() + rec["free_cells"].sum() + rec["occupied"].sum())
        assert total >= 2 * distinct > 0, (R, total, distinct, "the probes of a pose overlap: deduplication is exercised")
    rec = want[(720, 255)][0]
    assert (rec["unknown"] > 0).sum() >= 10 and (rec["free_cells"] > 0).sum() >= 20 and (rec["occupied"] > 1).sum() >= 10
    assert ((rec["hits"] > 0) & (rec["hits"] < rec["walked"])).any()
    outside = rec[12:16]
    assert (outside["walked"] == 0).all() and (outside["start_x"] == -1).all() and (outside.view(np.int32).reshape(-1, 8)[:, :5] == 0).all()
    for k in (16, 17):
        assert log[rec["start_y"][k], rec["start_x"][k]] > 0 and rec[k]["occupied"] == 1 and rec[k]["hits"] == rec[k]["walked"] == 720
        assert rec[k]["unknown"] == rec[k]["free_cells"] == 0
    assert rec[18] == rec[19]
    assert (rec["start_x"][:4].tolist(), rec["start_y"][:4].tolist()) == ([0, 199, 0, 199], [0, 0, 135, 135])
    assert want[(720, 255)][0]["unknown"].sum() > want[(720, 64)][0]["unknown"].sum() > want[(720, 7)][0]["unknown"].sum(), "the range cut matters"
    assert not np.array_equal(want[(255, 64)][0], want[(256, 64)][0]), "the probe past the workgroup's last lane matters"


@pytest.mark.parametrize("R", RANGES)
def test_base_case(R):
    g, log, poses, probes, want = base_case()
    m = _base_map()
    m.upload_log(log)
    for B in BS:
        _same(m.gain(poses, probes[:B], R), want[(B, R)][0], f"B = {B}, max_range = {R}")
    _same(m.gain(poses[9], probes[:300], R), want[(300, R)][0][9:10], "one pose")
    m.close()


def test_lds_against_memory():
    g, log, poses, probes, want = base_case()
    m = _with_walk(True, _base_map)
    m.upload_log(log)
    for R in RANGES:
        for B in (300, 720):
            _same(m.gain(poses, probes[:B], R), want[(B, R)][0], f"GMS_GAIN_WALK=mem, B = {B}, max_range = {R}")
    m.close()


# ---- the full window, and both sides of the staging threshold -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def large_case():
    g = orc.Grid(LWM, LHM, RES, 0.0, 0.0)
    assert (g.W, g.H) == (LW, LH)
    rng = np.random.default_rng(600520)
    u = rng.random((LH, LW))
    log = np.where(u < 0.003, L_OCC, np.where(u < 0.75, L_FREE, 0.0))
    log[255:266, 295:306] = L_FREE                                             # the central pose sees out of its cell
    log[100:420, 480] = L_OCC                                                  # a long wall east of it
    poses = np.array([_cell_pose(300, 260, 0.3),                               # central: max_range 255 gives columns 45 .. 555, 17 words x 511 rows
                      _cell_pose(40, 500, -1.0),                               # near a corner: the window clipped on two sides
                      _cell_pose(575, 20, 2.0)], dtype=np.float32)
    probes = _fan(720, [20.0, 16.0, 9.0])
    walks = [gx.Walks(g, probes, p) for p in poses]
    log.flags.writeable = False
    return g, log, poses, probes, walks


@pytest.mark.parametrize("form", ["lds", "GMS_GAIN_WALK=mem"])
def test_full_window_and_the_staging_threshold(form):
    """on a map larger than every window, 3 x 4 x (2 R + 31) / 32 + 1 words x (2 R + 1) rows fit 64 KiB less 128 bytes up to max_range
    194 (14 x 389 = 5446 words each): 194 is staged, 195 and 255 read the planes from memory"""
    g, log, poses, probes, walks = large_case()
    words = lambda R: ((2 * R + 31) // 32 + 1) * (2 * R + 1)
    assert 3 * 4 * words(194) <= 64 * 1024 - 128 < 3 * 4 * words(195) and 4 * words(255) == 17 * 511 * 4 == 34748
    m = _with_walk("mem" in form, lambda: GridMap(LWM, LHM, RES, (0.0, 0.0), max_beams=720))
    assert (m.W, m.H) == (LW, LH)
    m.upload_log(log)
    for R in (194, 195, 255):
        want = np.array([w.record(log, R)[0] for w in walks], dtype=GAIN_DTYPE)
        assert (want["unknown"] > 1000).all() and (want["hits"] > 100).all() and (want["hits"] < 720).all(), want
        _same(m.gain(poses, probes, R), want, f"{form}, max_range = {R}")
    m.close()


# ---- plane reuse and map changes -----------------------------------------------------------------------------------------------
def test_a_gain_after_a_cast_packs_no_plane_and_a_gain_after_an_update_sees_it():
    ext = 6.4
    g = orc.Grid(ext, ext, RES, -ext / 2, -ext / 2)
    tr = synth.make_trace(ext, RES, 180, T=6, seed=9)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=360)
    probes = _fan(360, [3.0, 1.0])
    poses = np.concatenate([tr.poses[:3], [[0.9, -0.7, 2.0], [-2.9, 2.9, 0.0]]]).astype(np.float32)
    m.update(tr.scans[0], tr.poses[0])
    m.cast(poses[:2], probes[:50])
    builds = m.cast_plane_builds()
    first = m.gain(poses, probes, 40)
    assert m.cast_plane_builds() == builds, "the casts' plane is current: a gain packs none"
    _same(first, gx.expect_poses(g, m.download_log(), probes, poses, 40), "after the first update")
    assert (first["free_cells"] > 0).any() and (first["occupied"] > 0).any()
    _same(m.gain(poses, probes, 40), first, "again")
    assert m.cast_plane_builds() == builds
    for k in (1, 2, 3):                                                        # the steady state: the last scan's apply pass is owed
        m.update(tr.scans[k], tr.poses[k])
    second = m.gain(poses, probes, 40)                                         # ... when the gain comes
    assert m.cast_plane_builds() == builds + 1, "the moved map's plane is packed once"
    _same(second, gx.expect_poses(g, m.download_log(), probes, poses, 40), "after three more updates")
    assert not np.array_equal(first, second), "the scans changed what the poses see"
    m.close()


# ---- other forms -----------------------------------------------------------------------------------------------------------------
def test_batched_handle_names_its_map():
    g, log, poses, probes, want = base_case()
    m = _base_map(n_maps=3)
    logs = np.zeros((3, H, W))
    logs[1] = log
    logs[2] = L_FREE
    m.upload_log(logs)
    _same(m.gain(poses, probes[:300], 64, mi=1), want[(300, 64)][0], "map 1")
    got0, got2 = m.gain(poses, probes[:300], 64, mi=0), m.gain(poses, probes[:300], 64, mi=2)
    assert (got0["free_cells"] == 0).all() and (got0["occupied"] == 0).all() and (got0["unknown"] > 0).any(), "map 0 was never observed"
    assert (got2["unknown"] == 0).all() and (got2["hits"] == 0).all() and (got2["free_cells"] > 0).any(), "map 2 is all free"
    _same(got2, gx.expect_poses(g, logs[2], probes[:300], poses, 64), "map 2")
    for bad in (-1, 3):
        with pytest.raises(GmsError) as e:
            m.gain(poses, probes[:300], 64, mi=bad)
        assert e.value.code == GMS_ERR_INVALID
    with pytest.raises(GmsError) as e:
        m.gain(poses, np.concatenate([probes, probes[:1]]), 64)
    assert e.value.code == GMS_ERR_INVALID, "one probe more than max_beams"
    m.close()


def test_device_form():
    import torch
    g, log, poses, probes, want = base_case()
    B, R, P = 300, 64, len(poses)
    m = _base_map()
    m.upload_log(log)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_poses, d_probes = dev(poses), dev(probes[:B])
    out = torch.full((32 * P + 80,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()                                                   # (the handle has a stream of its own)
    with pytest.raises(GmsError) as e:
        m.gain_dev(d_poses.data_ptr(), P, d_probes.data_ptr(), B, out[4:], R)
    assert e.value.code == GMS_ERR_INVALID
    m.synchronize(); torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all(), "a refused request writes nothing"
    m.gain_dev(d_poses.data_ptr(), P, d_probes.data_ptr(), B, out, R)
    m.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy()
    _same(raw[:32 * P].view(GAIN_DTYPE), want[(B, R)][0], "the device form")
    assert (raw[32 * P:] == GUARD).all(), "bytes past the records"
    m.close()


# ---- non-finite inputs: every call returns, and matches wherever Grid.trace_ray defines the walk ---------------------------------
def test_non_finite_poses_and_probes_terminate_and_match():
    g, log, poses, probes, want = base_case()
    wild = probes[:300].copy()
    wild["local_x"][[3, 40, 77, 290]] = [np.inf, np.nan, -np.inf, 1e30]
    wild["local_y"][[5, 41, 77, 291]] = [np.nan, np.inf, np.inf, -1e30]
    wild["distance"][[7, 8]] = [np.nan, np.inf]                                # (read, and without a part in the walk)
    bad_poses = np.array([[np.nan, 3.0, 0.0], [5.0, np.inf, 1.0], [5.0, 3.0, np.nan], [5.0, 3.0, np.inf], [-np.inf, np.nan, 0.5], [3e38, 3.0, 0.0],
                          [5.2, 2.0, 1.0]], dtype=np.float32)
    m = _base_map()
    m.upload_log(log)
    for R in (7, 255):
        with np.errstate(all="ignore"):
            w_fin = gx.expect_poses(g, log, wild, poses[:12], R)
            w_bad = gx.expect_poses(g, log, probes[:300], bad_poses, R)
            w_both = gx.expect_poses(g, log, wild, bad_poses, R)
        assert not np.array_equal(w_fin, want[(300, R)][0][:12]), "the non-finite probes change a record"
        _same(m.gain(poses[:12], wild, R), w_fin, f"non-finite probes, max_range = {R}")
        _same(m.gain(bad_poses, probes[:300], R), w_bad, f"non-finite poses, max_range = {R}")
        _same(m.gain(bad_poses, wild, R), w_both, f"both, max_range = {R}")
    m.close()
