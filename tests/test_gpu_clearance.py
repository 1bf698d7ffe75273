"""Clearance fields of the shared maps on the device (include/gridmapslam.h "clearance fields"): gms_map_clearance[_dev] and
gms_map_clearance_poses[_dev] against the brute-force expectation of tests/_clearance_expect.py on logData that was constructed or
downloaded.  Every comparison is array_equal on whole fields: the feature is all-integer and has no tolerance anywhere.  A field must
see the map as a download would return it at that moment and must change no later result of its handle.

The map is 200 x 136 cells: W a multiple of neither 32 nor 64 (a ragged last word, rows padded to 256 bits), H a multiple of no
tile height."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import _clearance_expect as xe
from gridmap_slam_robot_amd import GridMap, Observation, ParticleFilter, _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 200, 136
WM, HM = 9.98, 6.78                                     # metres: 199.6 and 135.6 cells, rounded up
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
GUARD = 0xA5A5


def _map(**kw):
    m = GridMap(WM, HM, RES, (0.0, 0.0), max_beams=128, **kw)
    assert (m.W, m.H) == (W, H)
    return m


def _same(got, want, where=""):
    assert got.dtype == np.uint16 and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (f"{where}: {len(bad)} of {want.size} cells differ, first at (y, x) = {bad[0].tolist()}: "
                                       f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


@functools.lru_cache(maxsize=None)
def _sparse_log():
    """about 1 % of the cells occupied, plus the four corner cells and one full row; everything else free"""
    rng = np.random.default_rng(20250117)
    log = np.where(rng.random((H, W)) < 0.01, L_OCC, L_FREE)
    log[0, 0] = log[0, W - 1] = log[H - 1, 0] = log[H - 1, W - 1] = L_OCC
    log[97, :] = L_OCC
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def _sparse_want(R, not_free=False):
    f = xe.expect(_sparse_log(), R, not_free)
    f.flags.writeable = False
    return f


# ---- 1: hand-derived ----------------------------------------------------------------------------------------------------------------
def test_hand_derived_cases():
    m = _map()
    log = np.full((H, W), L_FREE)
    assert (m.clearance(max_radius=255) == xe.FAR).all(), "a fresh map (all 0) has no occupied cell"
    m.upload_log(log)
    assert (m.clearance(max_radius=255) == xe.FAR).all(), "an empty map is all FAR"
    log[60, 100] = L_OCC
    m.upload_log(log)
    f5, f4 = m.clearance(max_radius=5), m.clearance(max_radius=4)
    assert f5[64, 103] == 25 and f4[64, 103] == xe.FAR, "3-4-5"
    assert f5[65, 100] == 25 and f5[60, 100] == 0 and f4[60, 100] == 0
    assert f5[66, 100] == xe.FAR and f5[60, 106] == xe.FAR and f5[60, 95] == 25 and f5[55, 100] == 25
    assert (f5 != xe.FAR).sum() == 81, "the 81 lattice points of a disc of radius 5"
    _same(f5, xe.expect(log, 5), "one obstacle, R = 5")
    m.upload_log(np.full((H, W), L_OCC))
    assert (m.clearance(max_radius=1) == 0).all() and (m.clearance(max_radius=255) == 0).all(), "every cell an obstacle: all 0"
    m.close()


# ---- 2: seeded sparse obstacles, the whole map --------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7, 64, 255])
def test_sparse_obstacles_whole_map(R):
    """64 reaches a whole plane word away (and two 32-bit words); 255 exceeds both sides of the map: every halo is clipped"""
    want = _sparse_want(R)
    assert (want == 0).sum() > 400 and ((want != 0) & (want != xe.FAR)).any()
    if R <= 7:
        assert (want == xe.FAR).any(), "cells beyond the radius"
    if R >= 64:
        assert (want != xe.FAR).all(), "at this density no cell is that far from an obstacle: the radius only bounds the search"
    m = _map()
    m.upload_log(_sparse_log())
    _same(m.clearance(max_radius=R), want, f"R = {R}")
    m.close()


@pytest.mark.parametrize("R", [31, 32, 33, 64, 65, 200, 255])
def test_few_obstacles_far_apart(R):
    """three obstacles in an otherwise free map: the distances that count span several plane words and most of the map, on either side
    of the 32-cell and 64-cell word boundaries"""
    log = np.full((H, W), L_FREE)
    log[3, 3] = log[130, 190] = log[70, 96] = L_OCC
    want = xe.expect(log, R)
    assert want[want != xe.FAR].max() == min(R * R, 15509) and (want == xe.FAR).any() == (R < 125), "the farthest cell is sqrt(15509) = 124.5 away"
    m = _map()
    m.upload_log(log)
    _same(m.clearance(max_radius=R), want, f"R = {R}")
    poses = np.array([[0.2, 6.7, 0.0], [9.9, 0.1, 0.0], [5.0, 0.2, 0.0], [0.17, 0.17, 0.0]], dtype=np.float32)
    assert np.array_equal(m.clearance_poses(poses, R), xe.expect_poses(want, poses, 0.0, 0.0, RES))
    m.close()


# ---- 3: rectangles ------------------------------------------------------------------------------------------------------------------
def test_rectangles():
    log = np.full((H, W), L_FREE)
    for (x, y) in ((38, 30), (95, 27), (40, 75), (99, 80), (66, 22), (70, 84)):      # a loose ring AROUND (45 .. 90) x (35 .. 70)
        log[y, x] = L_OCC
    inner = (45, 35, 46, 36)
    whole = xe.expect(log, 40)
    m = _map()
    m.upload_log(log)
    _same(m.clearance(max_radius=40), whole, "whole map")
    cut = lambda r: whole[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]
    assert (cut(inner) != 0).all() and (cut(inner) != xe.FAR).any(), "no obstacle inside the rectangle, all of them outside it"
    rects = {"interior": inner, "1 x 1": (77, 41, 1, 1), "left edge": (0, 20, 33, 50), "right edge": (W - 9, 0, 9, H), "top edge": (10, 0, 150, 3),
             "bottom edge": (31, H - 65, 66, 65), "one column": (64, 0, 1, H), "one row across a word boundary": (30, 50, 5, 1)}
    for name, r in rects.items():
        _same(m.clearance(rect=r, max_radius=40), cut(r), name)
        _same(m.clearance(rect=r, max_radius=40), xe.expect(log, 40, rect=r), name + " (expectation made for the rectangle)")
    sparse = _sparse_log()
    m.upload_log(sparse)
    for r in ((0, 0, W, H), (150, 100, 50, 36), (33, 95, 100, 5)):
        _same(m.clearance(rect=r, max_radius=255), _sparse_want(255)[r[1]:r[1] + r[3], r[0]:r[0] + r[2]], f"sparse {r}")
    for r in ((0, 0, W + 1, H), (0, 0, W, H + 1), (W, 0, 1, 1), (0, H, 1, 1), (190, 130, 11, 6), (190, 130, 10, 7), (-1, 0, 5, 5), (0, 0, 0, 5)):
        out = np.full((max(r[3], 1) + 1, max(r[2], 1) + 1), GUARD, dtype=np.uint16)
        c = _lib.GmsClearance(*r, 5, 0, 0)
        assert _lib.load().gms_map_clearance(m._h, 0, C.byref(c), out.ctypes.data) == GMS_ERR_INVALID, r
        assert (out == GUARD).all(), "a refused rectangle writes nothing"
        with pytest.raises(GmsError):
            m.clearance(rect=r, max_radius=5)
    for bad in (0, 256):
        with pytest.raises(GmsError) as e:
            m.clearance(max_radius=bad)
        assert e.value.code == GMS_ERR_INVALID
    m.close()


# ---- 4: the two predicates ----------------------------------------------------------------------------------------------------------
def test_modes_on_special_values():
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0])
    rng = np.random.default_rng(9)
    log = np.where(rng.random((H, W)) < 0.06, rng.choice(vals, size=(H, W)), -1.0)          # islands of every value in a free map
    log[3, :9] = vals
    log[H - 1, W - 9:] = vals
    occ, nf = xe.obstacles(log, False), xe.obstacles(log, True)
    assert occ[3, :9].tolist() == [False, False, False, True, False, True, False, True, False]
    assert nf[3, :9].tolist() == [True, True, True, True, False, True, False, True, False]
    assert (nf & ~occ).sum() > 100 and not (occ & ~nf).any()
    m = _map()
    m.upload_log(log)
    assert np.array_equal(m.download_log(), log, equal_nan=True)
    for R in (3, 30):
        got_occ, got_nf = m.clearance(max_radius=R), m.clearance(max_radius=R, not_free=True)
        _same(got_occ, xe.expect(log, R, False), f"occupied, R = {R}")
        _same(got_nf, xe.expect(log, R, True), f"not free, R = {R}")
        assert np.array_equal(got_occ == 0, occ) and np.array_equal(got_nf == 0, nf)
    all_unknown = _map()
    assert (all_unknown.clearance(max_radius=9, not_free=True) == 0).all(), "a fresh map is nowhere known free"
    all_unknown.close()
    m.close()


# ---- 5: state -----------------------------------------------------------------------------------------------------------------------
POSE = np.array([5.0, 3.4, 0.0], dtype=np.float32)     # cell (100, 68)


def _fan(a0, a1, n, d):
    ang = np.linspace(a0, a1, n)
    return Observation.from_polar(ang, np.full(n, d), np.ones(n, dtype=bool))


FRONT, BACK, LEFT = _fan(-1.0, 1.0, 64, 1.5), _fan(math.pi - 1.0, math.pi + 1.0, 64, 1.1), _fan(0.6, 2.4, 48, 0.8)


def _both(m, R=12):
    return m.clearance(max_radius=R), m.clearance(max_radius=R, not_free=True)


def _check_against_download(m, where, R=12):
    occ, nf = _both(m, R)
    log = m.download_log()
    _same(occ, xe.expect(log, R, False), where + ": occupied")
    _same(nf, xe.expect(log, R, True), where + ": not free")
    return occ, nf


def test_a_field_sees_what_a_download_sees():
    m = _map()
    m.integrate_observation(FRONT, POSE)               # no likelihood rebuild: nothing has made the field settle
    occ, nf = _check_against_download(m, "after integrate_observation")
    assert (occ == 0).sum() >= 20 and (nf != 0).any(), "the scan drew a wall and freed the cells in front of it"
    m.update(BACK, POSE); m.update(BACK, POSE)
    m.update(LEFT, POSE)                               # the steady state of update(): this scan's apply pass is still owed
    occ2, _ = _check_against_download(m, "after update() with its apply pass deferred")
    assert (occ2 != occ).any()
    m.close()


def _movers():
    wall = np.full((H, W), L_FREE)
    wall[20:110, 150] = L_OCC
    wall[20, 30:150] = 0.0
    def copy_from(m):
        other = _map()
        other.upload_log(wall[::-1].copy())
        m.copy_from(other)
        other.close()
    return {"upload_log": lambda m: m.upload_log(wall), "reset": lambda m: m.reset(), "copy_from": copy_from,
            "update": lambda m: m.update(FRONT, POSE)}


@pytest.mark.parametrize("mover", ["upload_log", "reset", "copy_from", "update"])
def test_a_field_after_a_mover_follows_the_new_map(mover):
    m = _map()
    m.upload_log(_sparse_log())
    before = _both(m)                                  # both planes are built
    _same(before[0], _sparse_want(12), "before")
    _movers()[mover](m)
    after = _check_against_download(m, f"after {mover}")
    assert (after[0] != before[0]).any() and (after[1] != before[1]).any(), "the mover changed both fields"
    m.close()


def test_a_field_shares_the_casts_plane():
    from _cast_expect import probes_from
    m = _map()
    m.upload_log(_sparse_log())
    probes = probes_from([1.0, 0.0, -1.0], [0.0, 1.0, 0.5])
    first = m.cast(POSE, probes)
    assert m.cast_plane_builds() == 1
    _same(m.clearance(max_radius=7), _sparse_want(7), "between two casts")
    _same(m.clearance(max_radius=7, not_free=True), _sparse_want(7, True), "the second plane")
    assert m.cast_plane_builds() == 1, "a field of GMS_CLEAR_OCCUPIED reads the plane the cast packed; the other mode packs its own"
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 1, "cast, clearance, cast: one pre-pass"
    m.upload_log(_sparse_log())
    _same(m.clearance(max_radius=7), _sparse_want(7), "the field packs the plane itself")
    assert m.cast_plane_builds() == 2
    assert np.array_equal(m.cast(POSE, probes), first) and m.cast_plane_builds() == 2, "a cast after a field packs none"
    m.close()


def test_a_field_changes_no_later_result():
    """twins through the same calls, one of them asked for fields at every turn: logData, the likelihood field and one fused scan step
    (poses, weights, the step's statistics) end bit-identical"""
    N = 64
    rng = np.random.default_rng(77)
    P = (POSE + rng.normal(0, [0.03, 0.03, 0.02], (N, 3))).astype(np.float32)
    results = []
    for ask in (False, True):
        m = _map()
        fields = lambda: _both(m, 9) + (m.clearance_poses(P, 9),) if ask else None
        m.update(BACK, POSE); fields()
        m.update(LEFT, POSE); fields()                 # (with the apply pass owed)
        pf = ParticleFilter(m, N)
        fields()
        pf.slam_update(P, FRONT, 0.41, 0.9, True)
        fields()
        log, lik = m.download_log(), m.download_likelihood()
        fields()
        results.append((log, lik, pf.get_poses(), pf.get_weights(), m.download_log(), pf.last_step()["strongest_pose"]))
        pf.close(); m.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b, equal_nan=True)
    assert (results[0][0] > 0).any()


# ---- 6: a batched handle ------------------------------------------------------------------------------------------------------------
def test_batched_handle():
    logs = np.stack([np.full((H, W), L_FREE), np.array(_sparse_log()[::-1]), np.array(_sparse_log()[:, ::-1])])
    logs[0][40, 40] = L_OCC
    m = _map(n_maps=3)
    m.upload_log(logs)
    for mi in (2, 0, 1):
        _same(m.clearance(max_radius=20, mi=mi), xe.expect(logs[mi], 20), f"map {mi}")
    _same(m.clearance(max_radius=20, not_free=True, mi=2), xe.expect(logs[2], 20, True), "map 2, not free")
    assert not np.array_equal(m.clearance(max_radius=20, mi=2), m.clearance(max_radius=20, mi=1))
    p = np.array([[2.0, 2.0, 0.0], [9.9, 6.7, 0.0]], dtype=np.float32)
    assert np.array_equal(m.clearance_poses(p, 20, mi=2), xe.expect_poses(xe.expect(logs[2], 20), p, 0.0, 0.0, RES))
    with pytest.raises(GmsError):
        m.clearance(max_radius=20, mi=3)
    m.close()


# ---- 7: the device forms ------------------------------------------------------------------------------------------------------------
def test_device_forms_on_a_stream_of_the_callers():
    import torch
    m = _map()
    m.upload_log(_sparse_log())
    rect = (13, 7, 150, 101)
    host = m.clearance(rect=rect, max_radius=30)
    _same(host, _sparse_want(30)[7:108, 13:163], "host form")
    poses = np.column_stack([np.random.default_rng(1).uniform(-0.3, 10.2, 500), np.random.default_rng(2).uniform(-0.3, 7.0, 500), np.zeros(500)]).astype(np.float32)
    host_p = m.clearance_poses(poses, 30)
    stream = torch.cuda.Stream()
    m.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        out = torch.full((host.size + 40,), GUARD - 65536, dtype=torch.int16, device="cuda")          # (the same 16 bits)
        out_p = torch.full((500 + 12,), GUARD - 65536, dtype=torch.int16, device="cuda")
        d_poses = torch.from_numpy(poses).to("cuda")
        stream.synchronize()
        with pytest.raises(GmsError) as e:
            m.clearance_dev(out.view(torch.uint8)[1:], rect=rect, max_radius=30)
        assert e.value.code == GMS_ERR_INVALID
        m.clearance_dev(out, rect=rect, max_radius=30)
        m.clearance_poses_dev(d_poses.data_ptr(), 500, out_p, max_radius=30)
        stream.synchronize()
    raw, raw_p = out.cpu().numpy().view(np.uint16), out_p.cpu().numpy().view(np.uint16)
    _same(raw[:host.size].reshape(host.shape), host, "the device form against the host form")
    assert (raw[host.size:] == GUARD).all(), "cells past the field"
    assert np.array_equal(raw_p[:500], host_p) and (raw_p[500:] == GUARD).all()
    m.set_stream(None)
    _same(m.clearance(rect=rect, max_radius=30), host, "back on the handle's own stream")
    m.close()


# ---- 8: the clearance under poses ---------------------------------------------------------------------------------------------------
def test_clearance_under_poses():
    log = _sparse_log()
    f32 = np.float32
    corner = lambda cx, cy: (f32(cx) * f32(RES), f32(cy) * f32(RES))       # a float product: on the corner up to rounding, either side of it
    pts = [corner(cx, cy) for cx in (0, 1, 31, 32, 33, 64, 100, 199, 200) for cy in (0, 1, 68, 97, 135, 136)]
    pts += [(-0.2 * RES, 1.0), (1.0, -0.9 * RES), (-0.999 * RES, -0.999 * RES), (-1e-30, 3.0)]        # (-1, 0) cells: truncated to cell 0
    pts += [(-1.0 * RES - 1e-4, 1.0), (1.0, -0.06), (WM + 0.03, 1.0), (1.0, HM + 0.03), (-50.0, -50.0), (1e30, 1.0), (np.inf, 1.0), (1.0, -np.inf)]   # outside
    pts += [(np.nan, np.nan), (np.nan, 3.0), (4.0, np.nan)]                                           # NaN -> cell 0 (tests/test_gpu_parity.py)
    rng = np.random.default_rng(31)
    pts += list(zip(rng.uniform(0, WM, 300), rng.uniform(0, HM, 300)))
    poses = np.array([(x, y, 0.3) for x, y in pts], dtype=np.float32)
    gx, gy = xe.cells_of(poses, 0.0, 0.0, RES)
    n0 = 54
    assert gx[n0] == 0 and gy[n0 + 1] == 0 and gx[n0 + 2] == 0 and gy[n0 + 2] == 0 and gx[n0 + 3] == 0, "truncation toward zero"
    assert gx[n0 + 12] == 0 and gy[n0 + 12] == 0 and gx[n0 + 13] == 0 and gy[n0 + 14] == 0, "NaN -> 0"
    m = _map()
    m.upload_log(log)
    for R in (2, 7, 64, 255):
        for not_free in (False, True):
            field = _sparse_want(R, not_free)
            want = xe.expect_poses(field, poses, 0.0, 0.0, RES)
            assert (want[n0 + 4:n0 + 12] == xe.OUTSIDE).all() and (want[:n0 + 4] != xe.OUTSIDE).sum() >= 40 and (want[n0 + 12:] != xe.OUTSIDE).all()
            got = m.clearance_poses(poses, R, not_free)
            bad = np.flatnonzero(got != want)
            assert np.array_equal(got, want), (R, not_free, bad[:5], poses[bad[:5]], got[bad[:5]], want[bad[:5]])
            inside = want != xe.OUTSIDE
            assert np.array_equal(got[inside], m.clearance(max_radius=R, not_free=not_free)[gy[inside], gx[inside]]), "values equal field[gy, gx]"
    one = m.clearance_poses(poses[100], 7)
    assert one.shape == (1,) and one[0] == xe.expect_poses(_sparse_want(7), poses[100:101], 0.0, 0.0, RES)[0]
    for bad_r in (0, 256):
        with pytest.raises(GmsError) as e:
            m.clearance_poses(poses, bad_r)
        assert e.value.code == GMS_ERR_INVALID
    m.close()
