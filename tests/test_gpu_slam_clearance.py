"""Clearance fields of the per-particle filter (include/gridmapslam.h "clearance fields"): gms_slam_clearance[_dev] against the
brute-force expectation of tests/_clearance_expect.py on every particle's downloaded logData.  Every comparison is array_equal.
8 particles x 120 x 120 cells, 90 beams, a few updates of the synthetic room with a resampling in between (the generation of the
maps flips); then the handle shapes that take other paths: a 256 x 256 map, no class planes (an eager field; a plane over 24 KiB) and a batched handle."""
import numpy as np
import pytest

import _clearance_expect as xe
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError
from test_gpu_slam_no_planes import _planes_kept

pytestmark = pytest.mark.gpu

RES, B, N, R = 0.05, 90, 8, 10
ODO = (0.02, 0.1)                                      # |dTheta| = 5.7 degrees: every update integrates (SLAM.java:82)


def _same(got, want, where=""):
    assert got.dtype == np.uint16 and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (f"{where}: {len(bad)} of {want.size} cells differ, first at (y, x) = {bad[0].tolist()}: "
                                       f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _handle(ext=6.0, n=N, **kw):
    s = SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=128, **kw)
    tr = synth.make_trace(ext, RES, B, T=8, seed=23)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    return s, tr


def _drive(s, tr, updates=3):
    for k in range(updates):
        s.update(tr.scans[k], ODO, seed=5, sequence=k)
        if k == 1:
            s.resample(0.37)


def _check_every_particle(s, n, modes=(False, True), rect=None):
    logs = [s.map_of(k) for k in range(n)]
    assert any((l > 0).any() for l in logs) and any(not np.array_equal(logs[0], l, equal_nan=True) for l in logs[1:]), "walls, and maps that differ"
    for not_free in modes:
        wants = [xe.expect(l, R, not_free, rect) for l in logs]
        assert any(((w != 0) & (w != xe.FAR)).any() for w in wants)
        for k in range(n):
            got, shown = s.clearance(k, rect=rect, max_radius=R, not_free=not_free)
            assert shown == k
            _same(got, wants[k], f"particle {k}, not_free = {not_free}")
    return logs


def test_every_particle_both_modes_and_strongest():
    assert _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle()
    assert (s.W, s.H) == (120, 120)
    with pytest.raises(GmsError) as e:
        s.clearance("strongest", max_radius=R)
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    _same(s.clearance(3, max_radius=R)[0], np.full((120, 120), xe.FAR, np.uint16), "a fresh map has no occupied cell")
    _same(s.clearance(3, max_radius=R, not_free=True)[0], np.zeros((120, 120), np.uint16), "... and is nowhere known free")
    _drive(s, tr)
    logs = _check_every_particle(s, N)
    for not_free in (False, True):
        got, shown = s.clearance("strongest", max_radius=R, not_free=not_free)
        assert shown == s.view("strongest")[1] == s.last_stats["strongest"]
        _same(got, xe.expect(logs[shown], R, not_free), "strongest")
    rect = (37, 61, 50, 33)
    got, shown = s.clearance(5, rect=rect, max_radius=R)
    _same(got, xe.expect(logs[5], R, rect=rect), "a rectangle")
    for bad in ((0, 0, 121, 120), (100, 100, 20, 21)):
        with pytest.raises(GmsError) as e:
            s.clearance(0, rect=bad, max_radius=R)
        assert e.value.code == GMS_ERR_INVALID
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            s.clearance(bad, max_radius=R)
        assert e.value.code == GMS_ERR_INVALID
    s.reset()
    with pytest.raises(GmsError) as e:
        s.clearance("strongest", max_radius=R)
    assert e.value.code == GMS_ERR_STATE, "... and none after a reset"
    s.close()


def test_a_field_changes_no_later_result_of_the_filter():
    """twins through the same updates and resampling, one of them asked for fields at every turn: poses, weights and every map equal"""
    ends = []
    for ask in (False, True):
        s, tr = _handle()
        for k in range(4):
            s.update(tr.scans[k], ODO, seed=5, sequence=k)
            if ask:
                s.clearance("strongest", max_radius=R); s.clearance(k, max_radius=R, not_free=True)
            if k in (1, 2):
                s.resample(0.37 + 0.1 * k)
                if ask:
                    s.clearance(7 - k, max_radius=R)
        poses, weights = s.get_particles()
        ends.append((poses, weights, s.maps(), s.maps(likelihood=True)))
        s.close()
    for a, b in zip(*ends):
        assert np.array_equal(a, b, equal_nan=True)


def test_a_resampling_copy_that_is_still_owed():
    s, tr = _handle()
    for k in range(3):
        s.update(tr.scans[k], ODO, seed=5, sequence=k)
    before = [s.map_of(k) for k in range(N)]
    idx, _ = s.resample(0.21, want_indices=True)
    got = [s.clearance(k, max_radius=R) for k in range(N)]                 # nothing in between: likelihoodData's copies are still owed
    moved = [k for k in range(N) if idx[k] != k and not np.array_equal(before[k], before[idx[k]], equal_nan=True)]
    assert moved, "the draw put another particle's map into at least one slot"
    for k in range(N):
        assert got[k][1] == k
        _same(got[k][0], xe.expect(before[idx[k]], R), f"slot {k} holds the map of particle {idx[k]}")
    got_nf = s.clearance(0, max_radius=R, not_free=True)[0]
    _same(got_nf, xe.expect(before[idx[0]], R, True), "not free")
    for k in range(N):
        assert np.array_equal(s.map_of(k), before[idx[k]], equal_nan=True), "... and the downloads agree"
    s.close()


def test_no_planes_eager_field(monkeypatch):
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")
    assert not _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle(n=4)
    _drive(s, tr)
    _check_every_particle(s, 4)
    got, shown = s.clearance("strongest", max_radius=R)
    assert shown == s.last_stats["strongest"]
    _same(got, xe.expect(s.map_of(shown), R), "strongest")
    s.close()


def test_256_x_256():
    """256 x 256 cells: rows of four 64-bit words, several bands and words of k_clear_field per field.  (Its class plane is 16 KiB,
    under the 24 KiB cap: the handle keeps its planes; the plane-less side of the cap is the next test.)"""
    ext = 12.8
    assert _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=3)
    assert (s.W, s.H) == (256, 256)
    _drive(s, tr)
    rect = (64, 50, 150, 160)
    _check_every_particle(s, 3, rect=rect)
    got, shown = s.clearance(1, max_radius=40)
    _same(got, xe.expect(s.map_of(1), 40), "the whole map, R = 40")
    s.close()


def test_no_planes_plane_over_24_kib():
    """314 x 314 cells x 2 bits = 24 649 bytes, the first size over the 24 KiB cap (tests/test_gpu_cast_edges.py holds both sides of
    it): the handle keeps no planes and the pre-pass reads logData; W a multiple of neither 32 nor 64"""
    ext = 15.68
    assert _planes_kept(15.62, 15.62, RES, max_beams=128) and not _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=2)
    assert (s.W, s.H) == (314, 314)
    _drive(s, tr)
    _check_every_particle(s, 2, rect=(90, 100, 224, 140))
    got, shown = s.clearance("strongest", max_radius=40)
    assert shown == s.last_stats["strongest"]
    _same(got, xe.expect(s.map_of(shown), 40), "strongest, the whole map, R = 40")
    s.close()


def test_batched_handle():
    S, n, ext = 3, 4, 6.0
    tr = synth.make_trace(ext, RES, B, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    with pytest.raises(GmsError) as e:
        bat.clearance("strongest", filter=1, max_radius=R)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    for f in range(S):
        for k in range(n):
            log = bat.map_of(f, k)
            got, shown = bat.clearance(k, filter=f, max_radius=R, not_free=bool((f + k) & 1))
            assert shown == f * n + k
            _same(got, xe.expect(log, R, bool((f + k) & 1)), f"filter {f}, particle {k}")
        got, shown = bat.clearance("strongest", filter=f, max_radius=R)
        assert shown == bat.view("strongest", filter=f)[1] and f * n <= shown < (f + 1) * n
        _same(got, xe.expect(bat.map_of(f, shown - f * n), R), f"filter {f}, strongest")
    assert not np.array_equal(bat.map_of(0, 0), bat.map_of(2, 0), equal_nan=True)
    with pytest.raises(IndexError):
        bat.clearance("strongest", filter=S, max_radius=R)
    bat.close()


def test_device_form():
    import torch
    s, tr = _handle()
    _drive(s, tr)
    host, shown = s.clearance("strongest", rect=(3, 5, 101, 77), max_radius=R)
    out = torch.full((host.size + 24,), 0x5A5A, dtype=torch.int16, device="cuda")
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GmsError) as e:
        s.clearance("strongest", rect=(3, 5, 101, 77), max_radius=R, out=out.view(torch.uint8)[1:], shown_out=sh)
    assert e.value.code == GMS_ERR_INVALID
    s.clearance("strongest", rect=(3, 5, 101, 77), max_radius=R, out=out, shown_out=sh)
    s.grid_map.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy().view(np.uint16)
    _same(raw[:host.size].reshape(host.shape), host, "the device form against the host form")
    assert (raw[host.size:] == 0x5A5A).all() and sh.cpu().tolist() == [shown, -7, -7, -7]
    s.close()
