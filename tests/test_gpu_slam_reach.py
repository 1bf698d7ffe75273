"""Cost-to-go fields of the per-particle filter (include/gridmapslam.h "cost-to-go fields"): gms_slam_reach[_dev] against the Dijkstra
expectation of tests/_reach_expect.py on every particle's downloaded logData.  Every comparison is array_equal.  8 particles x 120 x
120 cells, 90 beams, a few updates of the synthetic room with a resampling in between; then the handle shapes that take other paths:
an eager field, 256 x 256 (planes kept), 314 x 314 (none kept) and a batched handle."""
import numpy as np
import pytest

import _reach_expect as rx
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, cells_of_poses, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError
from test_gpu_slam_no_planes import _planes_kept

pytestmark = pytest.mark.gpu

RES, B, N = 0.05, 90, 8
ODO = (0.02, 0.1)
FAR = 0xFFFF


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


def _own_cell(s, k, ext=6.0, poses=None):
    poses = s.get_particles()[0] if poses is None else poses
    gx, gy = cells_of_poses(poses[k], (-ext / 2, -ext / 2), RES)
    return [(int(gx[0]), int(gy[0]))]


def _check_every_particle(s, n, ext=6.0, rect=None, inflate=1):
    logs = [s.map_of(k) for k in range(n)]
    assert any((l > 0).any() for l in logs) and any(not np.array_equal(logs[0], l, equal_nan=True) for l in logs[1:]), "walls, and maps that differ"
    reached = 0
    for not_free in (True, False):
        for k in range(n):
            seeds = _own_cell(s, k, ext)
            want = rx.expect(logs[k], seeds, inflate=inflate, not_free=not_free, rect=rect)
            reached += int((want != FAR).sum())
            got, shown = s.reach(k, seeds, inflate=inflate, not_free=not_free, rect=rect)
            assert shown == k
            _same(got, want, f"particle {k}, not_free = {not_free}")
            own, shown = s.reach(k, inflate=inflate, not_free=not_free, rect=rect)
            assert shown == k
            _same(own, want, f"particle {k}, not_free = {not_free}, its own cell")
    assert reached > 100 * n
    return logs


def test_every_particle_both_modes_and_strongest():
    assert _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle()
    assert (s.W, s.H) == (120, 120)
    with pytest.raises(GmsError) as e:
        s.reach("strongest")
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    assert (s.reach(3, [(60, 60)])[0] == FAR).all(), "a fresh map is nowhere known free"
    _same(s.reach(3, [(60, 60)], not_free=False)[0], rx.closed_form(120, 120, (60, 60)).astype(np.uint16), "... and nowhere occupied")
    _drive(s, tr)
    logs = _check_every_particle(s, N)
    for not_free in (True, False):
        got, shown = s.reach("strongest", not_free=not_free)
        assert shown == s.view("strongest")[1] == s.last_stats["strongest"]
        _same(got, rx.expect(logs[shown], _own_cell(s, shown), not_free=not_free), "strongest, its own cell")
        assert (got == 0).sum() == 1
        far_seeds = [(40, 40), (80, 75), (-3, 7)]
        got, shown2 = s.reach("strongest", far_seeds, not_free=not_free, max_cost=300)
        assert shown2 == shown
        _same(got, rx.expect(logs[shown], far_seeds, not_free=not_free, max_cost=300), "strongest, explicit seeds")
    st = s.grid_map.reach_stats()
    assert st["rounds"] >= 1 and st["tile_runs"] >= 1
    rect = (37, 61, 50, 33)
    _same(s.reach(5, rect=rect)[0], rx.expect(logs[5], _own_cell(s, 5), rect=rect), "a rectangle")
    for bad in ((0, 0, 121, 120), (100, 100, 20, 21)):
        with pytest.raises(GmsError) as e:
            s.reach(0, rect=bad)
        assert e.value.code == GMS_ERR_INVALID
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            s.reach(bad)
        assert e.value.code == GMS_ERR_INVALID
    s.reset()
    with pytest.raises(GmsError) as e:
        s.reach("strongest")
    assert e.value.code == GMS_ERR_STATE, "... and none after a reset"
    s.close()


def test_a_field_changes_no_later_result_of_the_filter():
    ends = []
    for ask in (False, True):
        s, tr = _handle()
        for k in range(4):
            s.update(tr.scans[k], ODO, seed=5, sequence=k)
            if ask:
                s.reach("strongest"); s.reach(k, inflate=2, not_free=False)
            if k in (1, 2):
                s.resample(0.37 + 0.1 * k)
                if ask:
                    s.reach(7 - k)
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
    got = [s.reach(k) for k in range(N)]                                      # nothing in between: likelihoodData's copies are still owed
    poses = s.get_particles()[0]
    moved = [k for k in range(N) if idx[k] != k and not np.array_equal(before[k], before[idx[k]], equal_nan=True)]
    assert moved, "the draw put another particle's map into at least one slot"
    for k in range(N):
        assert got[k][1] == k
        _same(got[k][0], rx.expect(before[idx[k]], _own_cell(s, k, poses=poses)), f"slot {k} holds the map of particle {idx[k]}")
    s.close()


def test_no_planes_eager_field(monkeypatch):
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")
    assert not _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle(n=4)
    _drive(s, tr)
    _check_every_particle(s, 4)
    got, shown = s.reach("strongest")
    assert shown == s.last_stats["strongest"]
    _same(got, rx.expect(s.map_of(shown), _own_cell(s, shown)), "strongest")
    s.close()


def test_256_x_256():
    ext = 12.8
    assert _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=3)
    assert (s.W, s.H) == (256, 256)
    _drive(s, tr)
    _check_every_particle(s, 3, ext=ext, rect=(64, 50, 150, 160), inflate=0)        # (the expectation's brute-force inflation is what costs time here)
    got, shown = s.reach(1, inflate=2, not_free=False)
    _same(got, rx.expect(s.map_of(1), _own_cell(s, 1, ext), inflate=2, not_free=False), "the whole map, inflate = 2, occupied")
    s.close()


def test_no_planes_plane_over_24_kib():
    ext = 15.68
    assert not _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=2)
    assert (s.W, s.H) == (314, 314)
    _drive(s, tr)
    _check_every_particle(s, 2, ext=ext, rect=(90, 100, 224, 140), inflate=0)
    got, shown = s.reach("strongest", inflate=4, not_free=False)
    assert shown == s.last_stats["strongest"]
    _same(got, rx.expect(s.map_of(shown), _own_cell(s, shown, ext), inflate=4, not_free=False), "strongest, the whole map, inflate = 4, occupied")
    s.close()


def test_batched_handle():
    S, n, ext = 3, 4, 6.0
    tr = synth.make_trace(ext, RES, B, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    with pytest.raises(GmsError) as e:
        bat.reach("strongest", filter=1)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    poses = np.asarray(bat.get_particles()[0]).reshape(S * n, 3)
    for f in range(S):
        for k in range(n):
            log = bat.map_of(f, k)
            got, shown = bat.reach(k, filter=f, not_free=bool((f + k) & 1))
            assert shown == f * n + k
            _same(got, rx.expect(log, _own_cell(bat, f * n + k, poses=poses), not_free=bool((f + k) & 1)), f"filter {f}, particle {k}")
        got, shown = bat.reach("strongest", filter=f)
        assert shown == bat.view("strongest", filter=f)[1] and f * n <= shown < (f + 1) * n
        _same(got, rx.expect(bat.map_of(f, shown - f * n), _own_cell(bat, shown, poses=poses)), f"filter {f}, strongest")
    with pytest.raises(IndexError):
        bat.reach("strongest", filter=S)
    bat.close()


def test_device_form():
    import torch
    s, tr = _handle()
    _drive(s, tr)
    rect = (3, 5, 101, 77)
    host, shown = s.reach("strongest", rect=rect, inflate=1)
    assert (host != FAR).sum() > 100
    out = torch.full((host.size + 24,), 0x5A5A, dtype=torch.int16, device="cuda")
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GmsError) as e:
        s.reach("strongest", rect=rect, inflate=1, out=out.view(torch.uint8)[1:], shown_out=sh)
    assert e.value.code == GMS_ERR_INVALID
    s.reach("strongest", rect=rect, inflate=1, out=out, shown_out=sh)
    s.grid_map.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy().view(np.uint16)
    _same(raw[:host.size].reshape(host.shape), host, "the device form against the host form")
    assert (raw[host.size:] == 0x5A5A).all() and sh.cpu().tolist() == [shown, -7, -7, -7]
    s.close()
