"""Sites and skeleton of the shared maps on the device (include/gridmapslam.h "sites and skeleton"): gms_map_skeleton[_dev] and
gms_map_nearest_poses[_dev] against the brute-force expectation of tests/_skeleton_expect.py on logData that was constructed or
downloaded.  Every comparison is array_equal on whole fields: the feature is all-integer and has no tolerance anywhere.

The map is the clearance suite's, 200 x 136 cells: W a multiple of neither 32 nor 64 (a ragged last word), H a multiple of no tile
height."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

import _skeleton_expect as xs
from gridmap_slam_robot_amd import GridMap, Observation, ParticleFilter, _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78                                     # metres: 199.6 and 135.6 cells, rounded up
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
WHOLE = (0, 0, W, H)


def _map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=128, **kw)
    assert (m.W, m.H) == (W, H)
    return m


def _same(got, want, where=""):
    assert got.dtype == want.dtype and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (f"{where}: {len(bad)} of {want.size} cells differ, first at (y, x) = {bad[0].tolist()}: "
                                       f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _check(m, site_whole, where, rect=WHOLE, R=25, not_free=False, min_clear=1, min_gap=2, mi=0):
    """all three outputs of one request against the expectation cut from the whole map's"""
    site, skel, tot = m.skeleton(rect, R, not_free, min_clear, min_gap, mi)
    want_site, want_skel = xs.cut(site_whole, rect), xs.cut(xs.skeleton(site_whole, min_clear, min_gap), rect)
    _same(site, want_site, where + ": site")
    _same(skel, want_skel, where + ": skel")
    assert xs.totals_of(tot) == xs.totals(want_site, want_skel), where + ": totals"
    return site, skel, tot


def _free():
    return np.full((H, W), L_FREE)


@functools.lru_cache(maxsize=None)
def _sparse_log():
    """the clearance suite's: about 1 % of the cells occupied, plus the four corner cells and one full row; everything else free"""
    rng = np.random.default_rng(20250117)
    log = np.where(rng.random((H, W)) < 0.01, L_OCC, L_FREE)
    log[0, 0] = log[0, W - 1] = log[H - 1, 0] = log[H - 1, W - 1] = L_OCC
    log[97, :] = L_OCC
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def _sparse_sites(R, not_free=False):
    f = xs.sites(_sparse_log(), R, not_free)
    f.flags.writeable = False
    return f


# ---- 1: hand-derived ----------------------------------------------------------------------------------------------------------------
def _corridor(upper, lower):
    log = _free()
    log[upper, :] = log[lower, :] = L_OCC
    return log


def test_corridor_and_ties_by_hand():
    m = _map()
    x = np.arange(W)
    m.upload_log(_corridor(10, 20))
    site, skel, tot = m.skeleton(max_radius=8)
    assert np.array_equal(site[15], 10 * W + x) and np.array_equal(site[16], 20 * W + x), "5 and 5: the upper wall; row 16: the lower one is nearer"
    assert (skel[15] == 25).all() and not np.delete(skel, 15, axis=0).any(), "the skeleton is exactly row 15"
    assert xs.totals_of(tot) == (27 * W, W, 25, 25)
    _check(m, xs.sites(_corridor(10, 20), 8), "walls at 10 and 20", R=8)
    m.upload_log(_corridor(10, 21))
    s21 = xs.sites(_corridor(10, 21), 8)
    for kw, there in (({}, True), (dict(min_gap=11), True), (dict(min_gap=12), False), (dict(min_clear=5), True), (dict(min_clear=6), False)):
        site, skel, tot = _check(m, s21, f"walls at 10 and 21, {kw}", R=8, **kw)
        assert (site[15] // W == 10).all() and (site[16] // W == 21).all()
        assert not np.delete(skel, 15, axis=0).any() and ((skel[15] == 25).all() if there else not skel[15].any()), kw
        assert xs.totals_of(tot)[1:] == ((W, 25, 25) if there else (0, 0, 0))
    log = _free()
    for dx, dy in ((5, 0), (0, 5), (-3, -4), (-4, -3)):
        log[70 + dy, 100 + dx] = L_OCC
    m.upload_log(log)
    for R in (5, 9):
        assert m.skeleton(max_radius=R, skel=False, totals=False)[0][70, 100] == 66 * W + 97, "four obstacles at d2 = 25: the smallest index"
        _check(m, xs.sites(log, R), f"four at the same distance, R = {R}", R=R)
    m.close()


TRAP = "a row at dy^2 == the best d2 so far with a zero offset ties on d2 and wins on the index when it lies ABOVE"


@pytest.mark.parametrize("d", [1, 5, 31, 32, 33])
def test_early_exit_trap(d):
    """obstacles exactly at (x, y - d) and (x, y + d), and at (x + d, y) and (x, y - d): a stage 2 that left on dy^2 >= best (right for
    the distance alone) would keep the wrong site"""
    R, x, y = max(d, 2), 96, 68                             # column 0 of a plane word
    m = _map()
    for a, b in (((x, y - d), (x, y + d)), ((x + d, y), (x, y - d))):
        log = _free()
        log[a[1], a[0]] = log[b[1], b[0]] = L_OCC
        m.upload_log(log)
        site, skel, tot = _check(m, xs.sites(log, R), f"d = {d}, obstacles at {a} and {b}", R=R)
        assert site[y, x] == min(a[1] * W + a[0], b[1] * W + b[0]) == (y - d) * W + x, TRAP
    m.close()


def test_early_exit_trap_255():
    """d = 255 does not fit the suite's map: the same two cases on 264 x 520 cells, with the tallest tile and the largest LDS request"""
    Wt, Ht, d, x, y = 264, 520, 255, 4, 257
    m = GridMap(13.2, 26.0, RES, (0.0, 0.0), max_beams=128)
    assert (m.W, m.H) == (Wt, Ht)
    for a, b in (((x, y - d), (x, y + d)), ((x + d, y), (x, y - d))):
        log = np.full((Ht, Wt), L_FREE)
        log[a[1], a[0]] = log[b[1], b[0]] = L_OCC
        m.upload_log(log)
        want = xs.sites(log, 255)
        want_skel = xs.skeleton(want)
        site, skel, tot = m.skeleton(max_radius=255)
        _same(site, want, f"obstacles at {a} and {b}: site")
        _same(skel, want_skel, f"obstacles at {a} and {b}: skel")
        assert xs.totals_of(tot) == xs.totals(want, want_skel)
        assert site[y, x] == min(a[1] * Wt + a[0], b[1] * Wt + b[0]) == (y - d) * Wt + x, TRAP
    m.close()


def test_left_against_right_across_a_word_boundary():
    m = _map()
    for xa, xb in ((31, 33), (0, 64)):
        log = _free()
        log[50, xa] = log[50, xb] = L_OCC
        m.upload_log(log)
        site, _, _ = _check(m, xs.sites(log, 40), f"bits at {xa} and {xb}", R=40)
        assert site[50, 32] == 50 * W + xa, "at equal distance the LEFT bit wins: smaller x, smaller index"
        assert site[58, 32] == 50 * W + xa and site[50, 33] == 50 * W + xb, "eight rows below, the same tie; one cell right, the right bit is nearer"
    m.close()


@pytest.mark.parametrize("R", [31, 32, 33, 64, 65, 200, 255])
def test_few_obstacles_far_apart(R):
    log = _free()
    log[3, 3] = log[130, 190] = log[70, 96] = L_OCC
    m = _map()
    m.upload_log(log)
    want = xs.sites(log, R)
    assert (want == xs.NONE).any() == (R < 125)
    _check(m, want, f"R = {R}", R=R, min_clear=2, min_gap=min(2 * R, 40))
    m.close()


# ---- 2: seeded sparse obstacles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7, 64, 255])
def test_sparse_obstacles_whole_map(R):
    want = _sparse_sites(R)
    m = _map()
    m.upload_log(_sparse_log())
    site, skel, tot = _check(m, want, f"R = {R}", R=R)
    _same(xs.clearance_of(site), m.clearance(max_radius=R), "the d2 recomputed from site equals the clearance field, cell for cell")
    has = site != xs.NONE
    assert (_sparse_log().ravel()[site[has]] > 0).all(), "every site is an obstacle cell"
    if R >= 7:
        assert (skel != 0).sum() > 100, "a skeleton between the obstacles"
        _check(m, want, f"R = {R}, thresholds", R=R, min_clear=3, min_gap=6)
    _check(m, _sparse_sites(R, True), f"R = {R}, not free", R=R, not_free=True)
    m.close()


def test_empty_and_full_maps():
    m = _map()
    m.upload_log(_free())
    site, skel, tot = m.skeleton(max_radius=255)
    assert (site == xs.NONE).all() and not skel.any() and xs.totals_of(tot) == (0, 0, 0, 0), "an empty map"
    m.upload_log(np.full((H, W), L_OCC))
    for R in (1, 255):
        site, skel, tot = m.skeleton(max_radius=R)
        assert np.array_equal(site, np.arange(W * H, dtype=np.uint32).reshape(H, W)), "a full map: every cell its own site"
        assert not skel.any() and xs.totals_of(tot) == (W * H, 0, 0, 0)
    m.close()


def test_modes_on_special_values():
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0])
    rng = np.random.default_rng(9)
    log = np.where(rng.random((H, W)) < 0.03, rng.choice(vals, size=(H, W)), -1.0)
    log[3, :9] = vals
    log[H - 1, W - 9:] = vals
    m = _map()
    m.upload_log(log)
    own = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for not_free in (False, True):
        site, _, _ = _check(m, xs.sites(log, 12, not_free), f"not_free = {not_free}", R=12, not_free=not_free)
        assert np.array_equal(site == own, xs.obstacles(log, not_free))
        assert (site[3, :9] == own[3, :9]).tolist() == ([True, True, True, True, False, True, False, True, False] if not_free else
                                                        [False, False, False, True, False, True, False, True, False])
    m.close()


# ---- 3: rectangles and outputs ------------------------------------------------------------------------------------------------------
def test_rectangles():
    m = _map()
    cor = _corridor(10, 20)
    m.upload_log(cor)
    s = xs.sites(cor, 8)
    _, skel, tot = _check(m, s, "the rectangle ends at row 15: the neighbour that decides lies outside it", rect=(20, 3, 100, 13), R=8)
    assert (skel[12] == 25).all() and xs.totals_of(tot)[1] == 100
    _, skel, _ = _check(m, s, "... and begins at row 15", rect=(20, 15, 100, 1), R=8)
    assert (skel == 25).all()
    log = _free()
    for (x, y) in ((38, 30), (95, 27), (40, 75), (99, 80), (66, 22), (70, 84)):      # a loose ring AROUND (45 .. 90) x (35 .. 70)
        log[y, x] = L_OCC
    m.upload_log(log)
    s = xs.sites(log, 40)
    site, skel, _ = _check(m, s, "every obstacle outside the rectangle", rect=(45, 35, 46, 36), R=40)
    assert (site != xs.NONE).any() and skel.any()
    m.upload_log(_sparse_log())
    s = _sparse_sites(20)
    for name, r in {"1 x 1": (77, 41, 1, 1), "left edge": (0, 20, 33, 50), "right edge": (W - 9, 0, 9, H), "top edge": (10, 0, 150, 3),
                    "bottom edge": (31, H - 65, 66, 65), "one column": (64, 0, 1, H), "one row across a word boundary": (30, 50, 5, 1)}.items():
        _check(m, s, name, rect=r, R=20)
    for r in ((0, 0, W + 1, H), (0, 0, W, H + 1), (W, 0, 1, 1), (190, 130, 11, 6), (190, 130, 10, 7), (-1, 0, 5, 5), (0, 0, 0, 5)):
        n = (max(r[3], 1) + 1) * (max(r[2], 1) + 1)
        site, skel, tot = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5, np.uint16), np.full(8, 0xA5A5A5A5, np.uint32)
        q = _lib.GmsSkeleton(*r, 5, 0, 1, 2, 0)
        assert _lib.load().gms_map_skeleton(m._h, 0, C.byref(q), site.ctypes.data, skel.ctypes.data, tot.ctypes.data) == GMS_ERR_INVALID, r
        assert (site == 0xA5A5A5A5).all() and (skel == 0xA5A5).all() and (tot == 0xA5A5A5A5).all(), "a refused rectangle writes nothing"
        with pytest.raises(GmsError):
            m.skeleton(rect=r, max_radius=5)
    for kw in (dict(max_radius=0), dict(max_radius=256), dict(min_clear=0), dict(max_radius=5, min_clear=6), dict(min_gap=1), dict(max_radius=5, min_gap=11)):
        with pytest.raises(GmsError) as e:
            m.skeleton(**kw)
        assert e.value.code == GMS_ERR_INVALID, kw
    m.close()


def test_every_subset_of_outputs():
    m = _map()
    m.upload_log(_sparse_log())
    rect, R = (13, 7, 150, 101), 20
    full = m.skeleton(rect, R)
    _same(full[0], xs.cut(_sparse_sites(R), rect), "all three")
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            with pytest.raises(GmsError) as e:
                m.skeleton(rect, R, site=False, skel=False, totals=False)
            assert e.value.code == GMS_ERR_INVALID, "all NULL is refused"
            continue
        got = m.skeleton(rect, R, site=want[0], skel=want[1], totals=want[2])
        for k in range(3):
            assert (got[k] is None) == (not want[k])
        if want[0]: _same(got[0], full[0], f"{want}: site")
        if want[1]: _same(got[1], full[1], f"{want}: skel")
        if want[2]: assert xs.totals_of(got[2]) == xs.totals_of(full[2]), want
    m.close()


# ---- 4: state -----------------------------------------------------------------------------------------------------------------------
POSE = np.array([5.0, 3.4, 0.0], dtype=np.float32)     # cell (100, 68)


def _fan(a0, a1, n, d):
    ang = np.linspace(a0, a1, n)
    return Observation.from_polar(ang, np.full(n, d), np.ones(n, dtype=bool))


FRONT, BACK, LEFT = _fan(-1.0, 1.0, 64, 1.5), _fan(math.pi - 1.0, math.pi + 1.0, 64, 1.1), _fan(0.6, 2.4, 48, 0.8)


def _check_against_download(m, where, R=12, mi=0):
    log = m.download_log()
    log = log[mi] if log.ndim == 3 else log
    out = []
    for not_free in (False, True):
        out.append(_check(m, xs.sites(log, R, not_free), f"{where}, not_free = {not_free}", R=R, not_free=not_free, mi=mi)[0])
    return out


def test_a_call_sees_what_a_download_sees():
    m = _map()
    m.integrate_observation(FRONT, POSE)               # no likelihood rebuild: nothing has made the field settle
    occ, nf = _check_against_download(m, "after integrate_observation")
    assert (occ != xs.NONE).any()
    m.update(BACK, POSE); m.update(BACK, POSE)
    m.update(LEFT, POSE)                               # the steady state of update(): this scan's apply pass is still owed
    occ2, _ = _check_against_download(m, "after update() with its apply pass deferred")
    assert (occ2 != occ).any()
    m.close()


@pytest.mark.parametrize("mover", ["upload_log", "reset", "copy_from"])
def test_a_call_after_a_mover_follows_the_new_map(mover):
    wall = _free()
    wall[20:110, 150] = L_OCC
    wall[20, 30:150] = 0.0
    m = _map()
    m.upload_log(_sparse_log())
    before = _check_against_download(m, "before")      # both planes are built
    if mover == "upload_log":
        m.upload_log(wall)
    elif mover == "reset":
        m.reset()
    else:
        other = _map()
        other.upload_log(wall[::-1].copy())
        m.copy_from(other)
        other.close()
    after = _check_against_download(m, f"after {mover}")
    assert (after[0] != before[0]).any() and (after[1] != before[1]).any(), "the mover changed both fields"
    m.close()


def test_map_2_of_3():
    logs = np.stack([_free(), np.array(_sparse_log()[::-1]), np.array(_sparse_log()[:, ::-1])])
    logs[0][40, 40] = L_OCC
    m = _map(n_maps=3)
    m.upload_log(logs)
    for mi in (2, 0, 1):
        _check(m, xs.sites(logs[mi], 20), f"map {mi}", R=20, mi=mi)
    p = np.array([[2.0, 2.0, 0.0], [9.9, 6.7, 0.0]], dtype=np.float32)
    got = m.nearest_poses(p, 20, mi=2)
    s, d = xs.expect_poses(xs.sites(logs[2], 20), p, 0.0, 0.0, RES)
    assert np.array_equal(got["site"], s) and np.array_equal(got["d2"], d)
    with pytest.raises(GmsError):
        m.skeleton(max_radius=20, mi=3)
    m.close()


def test_a_call_shares_the_casts_plane():
    from _cast_expect import probes_from
    m = _map()
    m.upload_log(_sparse_log())
    probes = probes_from([1.0, 0.0, -1.0], [0.0, 1.0, 0.5])
    first = m.cast(POSE, probes)
    assert m.cast_plane_builds() == 1
    _check(m, _sparse_sites(7), "between two casts", R=7)
    _check(m, _sparse_sites(7, True), "the second plane", R=7, not_free=True)
    m.nearest_poses(POSE, 7)
    assert m.cast_plane_builds() == 1, "GMS_CLEAR_OCCUPIED reads the plane the cast packed; the other mode packs its own"
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 1, "cast, skeleton, cast: one pre-pass"
    m.upload_log(_sparse_log())
    _check(m, _sparse_sites(7), "the call packs the plane itself", R=7)
    assert m.cast_plane_builds() == 2
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 2, "a cast after a skeleton packs none"
    m.close()


def test_a_call_changes_no_later_result():
    """twins through the same calls, one of them asked for skeletons at every turn: logData, the likelihood field and one fused scan
    step (poses, weights, the step's statistics) end bit-identical"""
    N = 64
    rng = np.random.default_rng(77)
    P = (POSE + rng.normal(0, [0.03, 0.03, 0.02], (N, 3))).astype(np.float32)
    results = []
    for ask in (False, True):
        m = _map()
        calls = lambda: (m.skeleton(max_radius=9), m.skeleton(max_radius=9, not_free=True, skel=False, totals=False), m.nearest_poses(P, 9)) if ask else None
        m.update(BACK, POSE); calls()
        m.update(LEFT, POSE); calls()                  # (with the apply pass owed)
        pf = ParticleFilter(m, N)
        calls()
        pf.slam_update(P, FRONT, 0.41, 0.9, True)
        calls()
        log, lik = m.download_log(), m.download_likelihood()
        calls()
        results.append((log, lik, pf.get_poses(), pf.get_weights(), m.download_log(), pf.last_step()["strongest_pose"]))
        pf.close(); m.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b, equal_nan=True)
    assert (results[0][0] > 0).any()


# ---- 5: the device forms ------------------------------------------------------------------------------------------------------------
def test_device_forms_on_a_stream_of_the_callers():
    import torch
    m = _map()
    m.upload_log(_sparse_log())
    rect, R = (13, 7, 150, 101), 30
    host = m.skeleton(rect, R)
    n = host[0].size
    poses = np.column_stack([np.random.default_rng(1).uniform(-0.3, 10.2, 500), np.random.default_rng(2).uniform(-0.3, 7.0, 500), np.zeros(500)]).astype(np.float32)
    host_p = m.nearest_poses(poses, R)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        site = torch.full((n + 40,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        skel = torch.full((n + 40,), 0x5A5A, dtype=torch.int16, device="cuda")
        tot = torch.full((4 + 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        out_p = torch.full((2 * 500 + 12,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_poses = torch.from_numpy(poses).to("cuda")
        stream.synchronize()
        for bad in (dict(site=site.view(torch.uint8)[2:]), dict(skel=skel.view(torch.uint8)[1:]), dict(totals=tot.view(torch.uint8)[4:])):
            with pytest.raises(GmsError) as e:
                m.skeleton_dev(rect=rect, max_radius=R, **bad)
            assert e.value.code == GMS_ERR_INVALID, "a misaligned output is refused"
        with pytest.raises(GmsError) as e:
            m.nearest_poses_dev(d_poses.data_ptr(), 500, out_p.view(torch.uint8)[2:], max_radius=R)
        assert e.value.code == GMS_ERR_INVALID
        with pytest.raises(GmsError) as e:
            m.skeleton_dev(rect=rect, max_radius=R)
        assert e.value.code == GMS_ERR_INVALID, "all NULL"
        m.skeleton_dev(site, skel, tot, rect=rect, max_radius=R)
        m.nearest_poses_dev(d_poses.data_ptr(), 500, out_p, max_radius=R)
        only = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        m.skeleton_dev(only, rect=rect, max_radius=R)
        stream.synchronize()
    raw_site, raw_skel = site.cpu().numpy().view(np.uint32), skel.cpu().numpy().view(np.uint16)
    _same(raw_site[:n].reshape(host[0].shape), host[0], "site: the device form against the host form")
    _same(raw_skel[:n].reshape(host[1].shape), host[1], "skel")
    assert (raw_site[n:] == 0x5A5A5A5A).all() and (raw_skel[n:] == 0x5A5A).all(), "cells past the fields"
    raw_tot = tot.cpu().numpy()
    assert xs.totals_of(raw_tot[:4].view(_lib.SKELETON_TOTALS_DTYPE)[0]) == xs.totals_of(host[2]) and (raw_tot[4:] == 0x5A5A5A5A5A5A5A5A).all()
    raw_only = only.cpu().numpy().view(np.uint32)
    _same(raw_only[:n].reshape(host[0].shape), host[0], "site alone")
    assert (raw_only[n:] == 0x5A5A5A5A).all()
    raw_p = out_p.cpu().numpy().view(np.uint32)
    assert np.array_equal(raw_p[:1000].view(_lib.NEAREST_DTYPE), host_p) and (raw_p[1000:] == 0x5A5A5A5A).all()
    m.set_stream(None)
    _same(m.skeleton(rect, R)[0], host[0], "back on the handle's own stream")
    m.close()


# ---- 6: the nearest obstacle under poses --------------------------------------------------------------------------------------------
def test_nearest_under_poses():
    f32 = np.float32
    corner = lambda cx, cy: (f32(cx) * f32(RES), f32(cy) * f32(RES))       # a float product: on the corner up to rounding, either side of it
    pts = [corner(cx, cy) for cx in (0, 1, 31, 32, 33, 64, 100, 199, 200) for cy in (0, 1, 68, 97, 135, 136)]
    pts += [(-0.2 * RES, 1.0), (1.0, -0.9 * RES), (-0.999 * RES, -0.999 * RES), (-1e-30, 3.0)]        # (-1, 0) cells: truncated to cell 0
    pts += [(-1.0 * RES - 1e-4, 1.0), (1.0, -0.06), (WM + 0.03, 1.0), (1.0, HM + 0.03), (-50.0, -50.0), (1e30, 1.0), (np.inf, 1.0), (1.0, -np.inf)]   # outside
    pts += [(np.nan, np.nan), (np.nan, 3.0), (4.0, np.nan)]                                           # NaN -> cell 0
    rng = np.random.default_rng(31)
    pts += list(zip(rng.uniform(0, WM, 300), rng.uniform(0, HM, 300)))
    poses = np.array([(x, y, 0.3) for x, y in pts], dtype=np.float32)
    n0 = 54
    m = _map()
    m.upload_log(_sparse_log())
    for R in (2, 7, 64, 255):
        for not_free in (False, True):
            s, d = xs.expect_poses(_sparse_sites(R, not_free), poses, 0.0, 0.0, RES)
            assert (s[n0 + 4:n0 + 12] == xs.OUTSIDE).all() and (d[n0 + 4:n0 + 12] == xs.CLEAR_OUTSIDE).all() and (s[n0 + 12:] != xs.OUTSIDE).all()
            assert (R > 7) or ((s == xs.NONE) & (d == xs.CLEAR_FAR)).any()
            got = m.nearest_poses(poses, R, not_free)
            bad = np.flatnonzero((got["site"] != s) | (got["d2"] != d))
            assert len(bad) == 0, (R, not_free, bad[:5], poses[bad[:5]], got[bad[:5]], s[bad[:5]], d[bad[:5]])
            assert np.array_equal(got["d2"].astype(np.uint16), m.clearance_poses(poses, R, not_free)), "the distances are clearance_poses'"
    one = m.nearest_poses(poses[100], 7)
    assert one.shape == (1,) and one["site"][0] == xs.expect_poses(_sparse_sites(7), poses[100:101], 0.0, 0.0, RES)[0][0]
    for bad_r in (0, 256):
        with pytest.raises(GmsError) as e:
            m.nearest_poses(poses, bad_r)
        assert e.value.code == GMS_ERR_INVALID
    m.close()
