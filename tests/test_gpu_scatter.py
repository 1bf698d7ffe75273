"""Particle seeding on the device (include/gridmapslam.h "particle seeding"): gms_pf_scatter against tests/_scatter_expect.py -- the
eligible cells by brute force from the downloaded logData, the oracle's Philox block, Python-integer ranks and numpy float arithmetic
in the header's order.  Every comparison is array_equal on the float32 bits of the poses and the float64 bits of the weights: there is
no tolerance.

The small maps are the ones where the word logic can break: 64 x 5 (exactly one word per row), 100 x 70 (two words, the second
ragged), 130 x 33 (a ragged third word), 65 x 64 (one cell in the second word).  The large map is derived from the unit's constants."""
import functools
import os
import re

import numpy as np
import pytest

import _clearance_expect as xe
import _scatter_expect as sx
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, synth
from gridmap_slam_robot_amd._lib import GMS_CLEAR_NOT_FREE, GMS_CLEAR_OCCUPIED, GMS_ERR_INVALID, GMS_ERR_STATE, GmsError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
MAPS = ((64, 5), (100, 70), (130, 33), (65, 64))
NS = (1, 255, 256, 257, 1000)                          # k_scat_draw's workgroup is 256 lanes: below, at and above it, several workgroups
SEED, SEQ = 0x123456789ABCDEF, 0xFEDCBA9876543210      # both halves of key and counter carry bits


def _unit_constant(name, unit="gms_scatter.hip"):
    src = open(os.path.join(ROOT, "gridmap_slam_robot_amd", "csrc", unit)).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got, want, where=""):
    assert got.dtype == want.dtype and got.shape == want.shape, where
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(axis=1))
    assert len(bad) == 0, f"{where}: {len(bad)} of {len(want)} slots differ, first at {bad[:1].tolist()}: {got[bad[:1]]} != {want[bad[:1]]}"


def _make_map(W, H, pos=(0.0, 0.0), **kw):
    m = GridMap((W - 0.4) * RES, (H - 0.4) * RES, RES, pos, max_beams=360, **kw)
    assert (m.W, m.H) == (W, H)
    return m


@functools.lru_cache(maxsize=None)
def _random_log(W, H, seed=0):
    """free 60 %, occupied 15 %, the rest never observed as 0, -0.0 and NaN"""
    rng = np.random.default_rng(1000 * W + H + seed)
    u = rng.random((H, W))
    log = np.where(u < 0.6, L_FREE, np.where(u < 0.75, L_OCC, 0.0))
    log[(u >= 0.75) & (u < 0.83)] = -0.0
    log[(u >= 0.83) & (u < 0.91)] = np.nan
    log[H // 2, W // 2] = L_FREE                          # (the single-cell rectangle's cell)
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def _want(W, H, rect, count, inflate=0, not_free=True, jitter=True, first=0, offset=0, pos=(0.0, 0.0), seed=0):
    return sx.expect(_random_log(W, H, seed), pos, RES, first, count, SEED, SEQ, rect=rect, inflate=inflate, not_free=not_free, jitter=jitter,
                     offset=offset)


def _scatter(m, n, **kw):
    """a fresh filter of n on m, scattered: (poses, weights, M)"""
    pf = ParticleFilter(m, n)
    M = pf.scatter(seed=SEED, sequence=SEQ, want_count=True, **kw)
    out = pf.get_poses(), pf.get_weights(), M
    pf.close()
    return out


@pytest.mark.parametrize("W,H", MAPS)
def test_word_shapes_rectangles_and_populations(W, H):
    m = _make_map(W, H)
    m.upload_log(_random_log(W, H))
    rects = (None, (W // 3, 1, W // 2 + 3, H - 2), (W // 2, H // 2, 1, 1))        # whole; cutting words on both sides; a single cell
    for rect in rects:
        want, cells, M = _want(W, H, rect, max(NS))
        assert M > 0 and (rect is None or rect[2] > 1 or M == 1)
        assert (_random_log(W, H)[cells[:, 1], cells[:, 0]] < 0).all(), "NaN, 0 and -0.0 are never drawn"
        for n in NS:
            poses, w, got_M = _scatter(m, n, rect=rect)
            assert got_M == M
            _same(poses, want[:n], f"{W} x {H}, rect {rect}, n = {n}")
            _same(w, np.full(n, 1.0 / n), "weights")
    m.close()


def test_a_map_that_needs_every_level_of_scan_and_search(monkeypatch):
    """The unit scans blocks of GMS_SCAN plane words and then the blocks' totals, and stages every 2^SCT_SHIFT_MIN-th word's prefix:
    a map of more than GMS_SCAN words has several scan blocks, block offsets that are not zero, several staged entries and a search
    that ends in memory.  1100 x 1030 cells are 1030 rows of 18 words.  GMS_SCATTER_SHIFT=9 makes the staged level coarser (the form
    planes of more than SCT_STAGE << SCT_SHIFT_MIN words take): the same poses."""
    scan, shift = _unit_constant("GMS_SCAN", "gms_internal.h"), _unit_constant("SCT_SHIFT_MIN")
    W, H = 1100, 1030
    words = H * ((W + 63) // 64)
    assert words > 4 * scan and words >> shift > 64 and words < scan * scan
    log = _random_log(W, H)
    want, cells, M = _want(W, H, None, 1000)
    assert len(np.unique((cells[:, 1] * ((W + 63) // 64) + cells[:, 0] // 64) // scan)) > 10, "the draws spread over the scan blocks"
    for env in (None, "9"):
        monkeypatch.delenv("GMS_SCATTER_SHIFT", raising=False)
        if env:
            monkeypatch.setenv("GMS_SCATTER_SHIFT", env)                       # read when the handle is created
        m = _make_map(W, H)
        monkeypatch.delenv("GMS_SCATTER_SHIFT", raising=False)
        m.upload_log(log)
        poses, w, got_M = _scatter(m, 1000)
        assert got_M == M
        _same(poses, want, f"1100 x 1030, GMS_SCATTER_SHIFT={env}")
        if env is None:                                    # free cells only in the last word of the last row
            last = np.zeros((H, W))
            last[H - 1, 1088:1100:2] = L_FREE
            m.upload_log(last)
            poses, _, got_M = _scatter(m, 257)
            want_last, cells_last, _ = sx.expect(last, (0.0, 0.0), RES, 0, 257, SEED, SEQ)
            assert got_M == 6 and (cells_last[:, 1] == H - 1).all() and set(cells_last[:, 0]) == set(range(1088, 1100, 2))
            _same(poses, want_last, "the last word of the last row")
        m.close()


def test_contents_none_one_and_every_cell():
    W, H = 100, 70
    m = _make_map(W, H)
    pf = ParticleFilter(m, 300)
    before = np.random.default_rng(5).normal(size=(300, 3)).astype(np.float32)
    pf.set_poses(before)
    for log in (np.zeros((H, W)), np.full((H, W), np.nan), np.full((H, W), L_OCC), -np.zeros((H, W))):
        m.upload_log(log)
        assert pf.scatter(seed=SEED, sequence=SEQ, want_count=True) == 0, "nothing is eligible"
        _same(pf.get_poses(), before, "M = 0: the poses are untouched")
    one = np.zeros((H, W))
    one[69, 99] = L_FREE                                   # the last cell of the map
    m.upload_log(one)
    assert pf.scatter(seed=SEED, sequence=SEQ, want_count=True) == 1
    want, cells, _ = sx.expect(one, (0.0, 0.0), RES, 0, 300, SEED, SEQ)
    assert (cells == [99, 69]).all()
    _same(pf.get_poses(), want, "M = 1")
    every = np.full((H, W), L_FREE)
    m.upload_log(every)
    assert pf.scatter(seed=SEED, sequence=SEQ, want_count=True) == W * H
    want, cells, _ = sx.expect(every, (0.0, 0.0), RES, 0, 300, SEED, SEQ)
    _same(pf.get_poses(), want, "every cell free")
    assert len(np.unique(cells[:, 1])) > 40 and cells[:, 0].max() > 90 and cells[:, 0].min() < 10, "the draws cover the map"
    pf.close(); m.close()


@pytest.mark.parametrize("not_free", [False, True])
def test_inflation_and_jitter_against_the_brute_force_rule(not_free):
    W, H = 100, 70
    rng = np.random.default_rng(70)
    log = np.full((H, W), L_FREE)
    log[rng.random((H, W)) < 0.01] = L_OCC                  # sparse obstacles: inflate 3 leaves room
    log[20:24, 50:60] = 0.0                                 # never observed: an obstacle of NOT_FREE only
    log[40:42, 10:14] = np.nan
    m = _make_map(W, H)
    m.upload_log(log)
    mode = GMS_CLEAR_NOT_FREE if not_free else GMS_CLEAR_OCCUPIED
    for inflate in (0, 1, 3):
        for jitter in (True, False):
            want, cells, M = sx.expect(log, (0.0, 0.0), RES, 0, 257, SEED, SEQ, inflate=inflate, not_free=not_free, jitter=jitter)
            poses, _, got_M = _scatter(m, 257, inflate=inflate, mode=mode, jitter=jitter)
            assert got_M == M and M > 0
            _same(poses, want, f"inflate {inflate}, not_free {not_free}, jitter {jitter}")
            d2 = m.clearance_poses(poses, max_radius=max(inflate, 1), not_free=not_free)
            assert (d2 != xe.OUTSIDE).all()
            if inflate:
                assert (d2 == xe.FAR).all(), "no written pose lies within `inflate` cells of an obstacle"
            else:
                assert (d2 != 0).all(), "no written pose lies on an obstacle"
    rect = (37, 9, 41, 50)
    want, _, M = sx.expect(log, (0.0, 0.0), RES, 0, 257, SEED, SEQ, rect=rect, inflate=3, not_free=not_free)
    poses, _, got_M = _scatter(m, 257, rect=rect, inflate=3, mode=mode)
    assert got_M == M
    _same(poses, want, "a rectangle: the obstacles of the whole map still block")
    m.close()


def test_cell_guarantee_near_the_stated_bound():
    """(|position| + extent) / resolution just below 2^18 cells on both axes, one origin negative: every written pose's cell under
    gms_map_clearance_poses' rule is the drawn cell (never outside the map, never an obstacle); just above the bound is refused"""
    W, H = 100, 70
    log = _random_log(W, H)
    far = float(np.float32(RES * (2 ** 18 - 200)))
    pos = (far, -far)
    m = _make_map(W, H, pos=pos)
    m.upload_log(log)
    want, cells, M = sx.expect(log, pos, RES, 0, 1000, SEED, SEQ)
    poses, _, got_M = _scatter(m, 1000)
    assert got_M == M
    _same(poses, want, "an origin near the bound")
    gx, gy = xe.cells_of(poses, pos[0], pos[1], RES)
    assert np.array_equal(gx, cells[:, 0]) and np.array_equal(gy, cells[:, 1])
    d2 = m.clearance_poses(poses, max_radius=1, not_free=True)
    assert (d2 != xe.OUTSIDE).all() and (d2 != 0).all()
    m.close()
    beyond = _make_map(W, H, pos=(float(np.float32(RES * 2 ** 18)), 0.0))
    pf = ParticleFilter(beyond, 10)
    with pytest.raises(GmsError) as e:
        pf.scatter(seed=1, sequence=2)
    assert e.value.code == GMS_ERR_INVALID and "2^18" in str(e.value)
    pf.close(); beyond.close()


def test_sub_range_leaves_the_other_slots_alone():
    W, H = 130, 33
    m = _make_map(W, H)
    m.upload_log(_random_log(W, H))
    n, first, count = 1000, 250, 300
    rng = np.random.default_rng(9)
    before_p = rng.normal(size=(n, 3)).astype(np.float32)
    before_w = rng.random(n)
    pf = ParticleFilter(m, n)
    pf.set_poses(before_p); pf.set_weights(before_w)
    assert pf.scatter(first=first, count=count, seed=SEED, sequence=SEQ, want_count=True) > 0
    want, _, _ = _want(W, H, None, n)
    p, w = pf.get_poses(), pf.get_weights()
    _same(p[first:first + count], want[first:first + count], "the written slots equal a whole-filter scatter's")
    _same(w[first:first + count], np.full(count, 1.0 / n), "their weights")
    keep = np.r_[0:first, first + count:n]
    _same(p[keep], before_p[keep], "the other slots' poses")
    _same(w[keep], before_w[keep], "the other slots' weights")
    for bad in (dict(first=n, count=1), dict(first=n - 1, count=2), dict(first=0, count=n + 1), dict(rect=(0, 0, W + 1, H)), dict(rect=(1, 0, W, H))):
        with pytest.raises(GmsError) as e:
            pf.scatter(seed=1, sequence=2, **bad)
        assert e.value.code == GMS_ERR_INVALID
    _same(pf.get_poses(), p, "a refused request touches nothing")
    pf.scatter(first=first, seed=SEED, sequence=SEQ)       # count=None: to the end of the filter
    _same(pf.get_poses()[first:], want[first:], "count = None")
    pf.close(); m.close()


def _scan_setup():
    import torch
    ext, B = 12.8, 180
    tr = synth.make_trace(ext, RES, B, T=8, seed=11)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=B)
    for t in range(3):
        m.update(tr.scans[t], tr.poses[t])
    beams = torch.from_numpy(tr.scans[3].view(np.uint8).copy()).to("cuda")
    return m, tr, beams, B


def test_state_after_a_scatter_is_set_poses_then_set_weights():
    """a filter that was scored and normalised, then scattered, then stepped == a fresh filter given the same poses and weights
    through gms_pf_set_poses / gms_pf_set_weights, then stepped: a stale cs or a stale flag would show"""
    import torch
    m, tr, beams, B = _scan_setup()
    n = 700
    filters = []
    for k in range(2):                                      # [0] is read in between (to feed the twin), [1] is not
        pf = ParticleFilter(m, n)
        pf.set_poses(synth.make_particles(tr.poses[3], n, seed=4, sigma_xy=0.05, sigma_theta_deg=3.0))
        pf.score(tr.scans[3])
        pf.normalize()
        M = pf.scatter(rect=(90, 90, 80, 80), seed=SEED, sequence=SEQ, want_count=k == 0)
        assert M is None or M > 100
        filters.append(pf)
    twin = ParticleFilter(m, n)
    twin.set_poses(filters[0].get_poses())
    twin.set_weights(filters[0].get_weights())
    for pf in filters + [twin]:
        pf.slam_update_dev(0, beams.data_ptr(), B, 0.37, 0.9, False)
    torch.cuda.synchronize()
    for pf in filters:
        assert pf.stats() == twin.stats()
        _same(pf.get_poses(), twin.get_poses(), "poses after the step")
        _same(pf.get_weights(), twin.get_weights(), "weights after the step")
    assert twin.stats()["weight_sum"] > 0
    for x in filters + [twin, m]:
        x.close()


def test_table_cache_and_plane_reuse():
    m, tr, beams, B = _scan_setup()
    pf = ParticleFilter(m, 300)
    assert m.scatter_table_builds() == 0
    pf.scatter(seed=1, sequence=2)
    first = pf.get_poses()
    assert m.scatter_table_builds() == 1
    pf.scatter(seed=1, sequence=2)
    pf.scatter(seed=1, sequence=3, first=10, count=20, jitter=False)
    assert m.scatter_table_builds() == 1, "an unchanged map and the same request: the draw alone"
    pf.scatter(seed=1, sequence=2)
    _same(pf.get_poses(), first, "the cached table gives the same poses")
    pf.scatter(rect=(0, 0, m.W, m.H - 1), seed=1, sequence=2)
    assert m.scatter_table_builds() == 2, "another rectangle"
    pf.scatter(rect=(0, 0, m.W, m.H - 1), inflate=2, seed=1, sequence=2)
    assert m.scatter_table_builds() == 3, "another inflate"
    pf.scatter(rect=(0, 0, m.W, m.H - 1), inflate=2, seed=1, sequence=2)
    assert m.scatter_table_builds() == 3
    m.update(tr.scans[4], tr.poses[4])
    pf.scatter(rect=(0, 0, m.W, m.H - 1), inflate=2, seed=1, sequence=2)
    assert m.scatter_table_builds() == 4, "logData moved"
    # a scatter after a cast packs no plane, and a cast after a scatter with inflate under OCCUPIED packs none either
    m.cast(tr.poses[4][None, :], tr.scans[4])
    builds = m.cast_plane_builds()
    pf.scatter(seed=1, sequence=2)
    pf.scatter(inflate=1, mode=GMS_CLEAR_OCCUPIED, seed=1, sequence=2)
    m.cast(tr.poses[4][None, :], tr.scans[4])
    assert m.cast_plane_builds() == builds
    pf.close(); m.close()


def test_deferred_apply_pass_is_applied_first():
    m, tr, beams, B = _scan_setup()
    pf = ParticleFilter(m, 500)
    pf.scatter(seed=SEED, sequence=SEQ)                    # a table of the map before the scan
    m.update(tr.scans[5], tr.poses[5])                     # leaves its `logData +=` pass pending
    M = pf.scatter(seed=SEED, sequence=SEQ, want_count=True)
    got = pf.get_poses()
    log = m.download_log()
    want, _, want_M = sx.expect(log, (-6.4, -6.4), RES, 0, 500, SEED, SEQ)
    assert M == want_M
    _same(got, want, "right after gms_map_update")
    pf.close(); m.close()


def test_two_shards_equal_the_stand_alone_filter():
    W, H = 100, 70
    m = _make_map(W, H)
    m.upload_log(_random_log(W, H))
    whole = ParticleFilter(m, 512)
    whole.scatter(seed=SEED, sequence=SEQ)
    a, b = ParticleFilter(m, 256), ParticleFilter(m, 256)
    a.set_shard(0, 512); b.set_shard(256, 512)
    a.scatter(seed=SEED, sequence=SEQ); b.scatter(seed=SEED, sequence=SEQ)
    _same(np.concatenate([a.get_poses(), b.get_poses()]), whole.get_poses(), "the shards' poses")
    _same(np.concatenate([a.get_weights(), b.get_weights()]), np.full(512, 1.0 / 512), "the shards' weights")
    _same(whole.get_poses(), _want(W, H, None, 1000)[0][:512], "the stand-alone filter")
    for x in (whole, a, b, m):
        x.close()


def test_batched_maps_draw_from_their_own_map_without_a_read_back():
    W, H = 65, 64
    logs = np.stack([_random_log(W, H), _random_log(W, H, seed=1), np.zeros((H, W))])
    m = _make_map(W, H, n_maps=3)
    m.upload_log(logs)
    n = 257
    pf = ParticleFilter(m, n)
    before = pf.get_poses()
    assert pf.scatter(seed=SEED, sequence=SEQ) is None      # n_eligible = NULL: nothing read back
    got = pf.get_poses()
    M = pf.scatter(seed=SEED, sequence=SEQ, want_count=True)
    _same(pf.get_poses().reshape(-1, 3), got.reshape(-1, 3), "with and without n_eligible")
    for mi in range(2):
        want, _, want_M = sx.expect(logs[mi], (0.0, 0.0), RES, 0, n, SEED, SEQ, mi=mi)
        assert M[mi] == want_M
        _same(got[mi], want, f"map {mi}")
    assert not np.array_equal(got[0], got[1])
    assert M[2] == 0
    _same(got[2], before[2], "a map without a free cell: its filter untouched")
    _same(pf.get_weights()[:2].reshape(-1), np.full(2 * n, 1.0 / n), "weights")
    pf.close(); m.close()


def test_the_filter_of_a_gms_slam_is_refused():
    s = SLAMParticleMaps(6.0, 6.0, RES, (-3.0, -3.0), num_particles=16, max_beams=64)
    before = s.pf.get_poses()
    with pytest.raises(GmsError) as e:
        s.pf.scatter(seed=1, sequence=2)
    assert e.value.code == GMS_ERR_STATE
    _same(s.pf.get_poses(), before, "nothing touched")
    s.close()
