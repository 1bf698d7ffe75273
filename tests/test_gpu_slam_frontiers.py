"""Frontier regions of the per-particle filter (include/gridmapslam.h "frontier regions"): gms_slam_frontiers[_dev] against the
flood-fill expectation of tests/_frontier_expect.py on every particle's downloaded logData.  Every comparison is array_equal.  8
particles x 120 x 120 cells, 90 beams, a few updates of the synthetic room with a resampling in between; then the handle shapes that
take other paths: an eager field, 256 x 256 (planes kept), 314 x 314 (none kept) and a batched handle."""
import numpy as np
import pytest

import _frontier_expect as fx
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, _lib, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError
from test_gpu_slam_no_planes import _planes_kept

pytestmark = pytest.mark.gpu

RES, B, N = 0.05, 90, 8
ODO = (0.02, 0.1)
FAR, NONE = 0xFFFF, 0xFFFFFFFF


def _same(got, want, where):
    assert got[1] == want[1], f"{where}: n_found {got[1]} != {want[1]}"
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), f"{where}: the records differ"
    bad = np.argwhere(got[2] != want[2])
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2]), f"{where}: {len(bad)} labels differ, first at (y, x) = {bad[:1].tolist()}"


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


def _check_every_particle(s, n, rect=None, inflate=1, min_size=2):
    logs = [s.map_of(k) for k in range(n)]
    assert any((l > 0).any() for l in logs) and any(not np.array_equal(logs[0], l, equal_nan=True) for l in logs[1:]), "walls, and maps that differ"
    cells = 0
    for k in range(n):
        cost, shown = s.reach(k, inflate=inflate, not_free=False)
        assert shown == k
        want = fx.expect(logs[k], min_size=min_size, inflate=inflate, cost=cost, rect=rect)
        cells += int(want[0]["count"].sum())
        *got, shown = s.frontiers(k, min_size=min_size, inflate=inflate, cost=cost, rect=rect, labels=True)
        assert shown == k
        _same(got, want, f"particle {k}")
    assert cells > 20 * n
    return logs


def test_every_particle_and_strongest():
    assert _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle()
    assert (s.W, s.H) == (120, 120)
    with pytest.raises(GmsError) as e:
        s.frontiers("strongest")
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    rec, n, lab, shown = s.frontiers(3, labels=True)
    assert n == 0 and len(rec) == 0 and (lab == NONE).all() and shown == 3, "a fresh map has no free cell"
    _drive(s, tr)
    logs = _check_every_particle(s, N)
    rec, n, lab, shown = s.frontiers("strongest", labels=True)
    assert shown == s.view("strongest")[1] == s.last_stats["strongest"]
    _same((rec, n, lab), fx.expect(logs[shown]), "strongest")
    assert n >= 1 and (rec["goal_cost"] == FAR).all() and (rec["goal_x"] == -1).all(), "no cost field: no goal"
    rect = (37, 61, 50, 33)
    *got, _ = s.frontiers(5, rect=rect, labels=True, min_size=3)
    _same(got, fx.expect(logs[5], rect=rect, min_size=3), "a rectangle")
    rec2, n2, _ = s.frontiers(5, cap=1)
    assert n2 == fx.expect(logs[5])[1] and np.array_equal(rec2, fx.expect(logs[5])[0][:1])
    for bad in ((0, 0, 121, 120), (100, 100, 20, 21)):
        with pytest.raises(GmsError) as e:
            s.frontiers(0, rect=bad)
        assert e.value.code == GMS_ERR_INVALID
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            s.frontiers(bad)
        assert e.value.code == GMS_ERR_INVALID
    s.reset()
    with pytest.raises(GmsError) as e:
        s.frontiers("strongest")
    assert e.value.code == GMS_ERR_STATE, "... and none after a reset"
    s.close()


def test_a_request_changes_no_later_result_of_the_filter():
    ends = []
    for ask in (False, True):
        s, tr = _handle()
        for k in range(4):
            s.update(tr.scans[k], ODO, seed=5, sequence=k)
            if ask:
                s.frontiers("strongest", labels=True); s.frontiers(k, inflate=2, min_size=2)
            if k in (1, 2):
                s.resample(0.37 + 0.1 * k)
                if ask:
                    s.frontiers(7 - k)
        poses, weights = s.get_particles()
        ends.append((poses, weights, s.maps(), s.maps(likelihood=True), s.reach(2)[0], s.clearance(1)[0]))
        s.close()
    for a, b in zip(*ends):
        assert np.array_equal(a, b, equal_nan=True)


def test_a_resampling_copy_that_is_still_owed():
    s, tr = _handle()
    for k in range(3):
        s.update(tr.scans[k], ODO, seed=5, sequence=k)
    before = [s.map_of(k) for k in range(N)]
    idx, _ = s.resample(0.21, want_indices=True)
    got = [s.frontiers(k, labels=True) for k in range(N)]                     # nothing in between: likelihoodData's copies are still owed
    moved = [k for k in range(N) if idx[k] != k and not np.array_equal(before[k], before[idx[k]], equal_nan=True)]
    assert moved, "the draw put another particle's map into at least one slot"
    for k in range(N):
        assert got[k][3] == k
        _same(got[k][:3], fx.expect(before[idx[k]]), f"slot {k} holds the map of particle {idx[k]}")
    s.close()


def test_no_planes_eager_field(monkeypatch):
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")
    assert not _planes_kept(6.0, 6.0, RES, max_beams=128)
    s, tr = _handle(n=4)
    _drive(s, tr)
    _check_every_particle(s, 4)
    *got, shown = s.frontiers("strongest", labels=True)
    assert shown == s.last_stats["strongest"]
    _same(got, fx.expect(s.map_of(shown)), "strongest")
    s.close()


def test_256_x_256():
    ext = 12.8
    assert _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=3)
    assert (s.W, s.H) == (256, 256)
    _drive(s, tr)
    _check_every_particle(s, 3, rect=(64, 50, 150, 160), inflate=0, min_size=1)
    s.close()


def test_no_planes_plane_over_24_kib():
    ext = 15.68
    assert not _planes_kept(ext, ext, RES, max_beams=128)
    s, tr = _handle(ext=ext, n=2)
    assert (s.W, s.H) == (314, 314)
    _drive(s, tr)
    _check_every_particle(s, 2, rect=(90, 100, 224, 140), inflate=0, min_size=1)
    *got, shown = s.frontiers("strongest", inflate=4, labels=True)
    assert shown == s.last_stats["strongest"]
    _same(got, fx.expect(s.map_of(shown), inflate=4), "strongest, inflate = 4")
    s.close()


def test_batched_handle():
    S, n, ext = 3, 4, 6.0
    tr = synth.make_trace(ext, RES, B, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    with pytest.raises(GmsError) as e:
        bat.frontiers("strongest", filter=1)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    for f in range(S):
        for k in range(n):
            *got, shown = bat.frontiers(k, filter=f, labels=True, min_size=1 + (k & 1))
            assert shown == f * n + k
            _same(got, fx.expect(bat.map_of(f, k), min_size=1 + (k & 1)), f"filter {f}, particle {k}")
        *got, shown = bat.frontiers("strongest", filter=f, labels=True)
        assert shown == bat.view("strongest", filter=f)[1] and f * n <= shown < (f + 1) * n
        _same(got, fx.expect(bat.map_of(f, shown - f * n)), f"filter {f}, strongest")
    with pytest.raises(IndexError):
        bat.frontiers("strongest", filter=S)
    bat.close()


def test_device_form():
    import torch
    s, tr = _handle()
    _drive(s, tr)
    rect = (3, 5, 101, 77)
    cost, _ = s.reach("strongest", not_free=False)
    rec, n, lab, shown = s.frontiers("strongest", cost=cost, rect=rect, labels=True)
    assert n >= 1 and (rec["goal_cost"] != FAR).any()
    cap = 2
    d_lab = torch.full((lab.size + 24,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_rec = torch.full((56 * cap + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_cost = torch.from_numpy(cost.view(np.int16)).to("cuda")
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GmsError) as e:
        s.frontiers("strongest", cost=d_cost, rect=rect, labels_out=d_lab.view(torch.uint8)[1:], records_out=d_rec[:56 * cap], shown_out=sh)
    assert e.value.code == GMS_ERR_INVALID
    got_n = s.frontiers("strongest", cost=d_cost, rect=rect, labels_out=d_lab, records_out=d_rec[:56 * cap], shown_out=sh)
    assert got_n == n
    s.grid_map.synchronize(); torch.cuda.synchronize()
    raw_l, raw_r = d_lab.cpu().numpy().view(np.uint32), d_rec.cpu().numpy()
    assert np.array_equal(raw_l[:lab.size].reshape(lab.shape), lab) and (raw_l[lab.size:] == 0x5A5A5A5A).all()
    k = min(cap, n)
    assert np.array_equal(raw_r[:56 * k].view(_lib.FRONTIER_DTYPE), rec[:k]) and (raw_r[56 * cap:] == 0x5A).all()
    assert sh.cpu().tolist() == [shown, -7, -7, -7]
    s.close()
