"""Rooms and doors of the per-particle filter (include/gridmapslam.h "rooms and doors"): gms_slam_rooms[_dev] against the plain
restatement of tests/_rooms_expect.py on every particle's downloaded logData.  Every comparison is array_equal.  8 particles x
120 x 120 cells, 90 beams, a few updates of the synthetic room with a resampling in between (the generation of the maps flips); then a
batched handle and the device form."""
import numpy as np
import pytest

import _rooms_expect as rx
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, _lib, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError

pytestmark = pytest.mark.gpu

RES, B, N = 0.05, 90, 8
ODO = (0.02, 0.1)                                      # |dTheta| = 5.7 degrees: every update integrates (SLAM.java:82)
KW = dict(core=3, inflate=1, min_core=4, max_cost=400)
NONE = 0xFFFFFFFF


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


def _against(got, log, where, not_free, rect=None):
    want = rx.expect(log, not_free=not_free, rect=rect, **KW)
    rx.same(got, want, where)
    return want


def _ask(s, which, not_free, rect=None, **kw):
    return s.rooms(which, not_free=not_free, rect=rect, depth=True, cap_rooms=512, cap_doors=512, **KW, **kw)


def test_every_particle_both_modes_and_strongest():
    s, tr = _handle()
    assert (s.W, s.H) == (120, 120)
    with pytest.raises(GmsError) as e:
        _ask(s, "strongest", True)
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    r = _ask(s, 3, True)
    assert r["shown"] == 3 and r["n_rooms"] == 0 and (r["labels"] == NONE).all(), "a fresh map is nowhere known free"
    r = _ask(s, 3, False)
    assert r["n_rooms"] == 1 and (r["labels"] == 0).all() and r["rooms"]["count"][0] == 120 * 120, "... and nowhere occupied"
    _drive(s, tr)
    logs = [s.map_of(k) for k in range(N)]
    assert any((l > 0).any() for l in logs) and any(not np.array_equal(logs[0], l, equal_nan=True) for l in logs[1:]), "walls, and maps that differ"
    rooms = 0
    for not_free in (False, True):
        for k in range(N):
            got = _ask(s, k, not_free)
            assert got["shown"] == k
            rooms += _against(got, logs[k], f"particle {k}, not_free = {not_free}", not_free)["n_rooms"]
        got = _ask(s, "strongest", not_free)
        assert got["shown"] == s.view("strongest")[1] == s.last_stats["strongest"]
        _against(got, logs[got["shown"]], "strongest", not_free)
    assert rooms >= 2 * N, "a room in every map under both modes"
    rect = (37, 61, 50, 33)
    _against(_ask(s, 5, True, rect), logs[5], "a rectangle", True, rect)
    for bad in ((0, 0, 121, 120), (100, 100, 20, 21)):
        with pytest.raises(GmsError) as e:
            _ask(s, 0, True, bad)
        assert e.value.code == GMS_ERR_INVALID
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            _ask(s, bad, True)
        assert e.value.code == GMS_ERR_INVALID
    s.reset()
    with pytest.raises(GmsError) as e:
        _ask(s, "strongest", True)
    assert e.value.code == GMS_ERR_STATE, "... and none after a reset"
    s.close()


def test_a_shard_serves_a_named_particle_only():
    shard = SLAMParticleMaps.__new__(SLAMParticleMaps)
    shard._init_shard(3.2, 3.2, RES, (-1.6, -1.6), 256, 0, 512, max_beams=64)
    assert (shard.W, shard.H) == (64, 64)
    for not_free in (False, True):
        with pytest.raises(GmsError) as e:
            _ask(shard, "strongest", not_free)
        assert e.value.code == GMS_ERR_STATE, "its filter's strongest particle may live on another rank"
    log = shard.map_of(7)
    got = _ask(shard, 7, False)
    assert got["shown"] == 7 and got["n_rooms"] == 1 and got["rooms"]["count"][0] == 64 * 64
    _against(got, log, "a shard's particle 7, occupied", False)
    _against(_ask(shard, 7, True), log, "a shard's particle 7, not free", True)
    rect = (60, 3, 4, 61)
    _against(_ask(shard, 255, False, rect), shard.map_of(255), "its last particle, a rectangle flush with the far edges", False, rect)
    with pytest.raises(GmsError) as e:
        _ask(shard, 256, False)
    assert e.value.code == GMS_ERR_INVALID, "a particle of another rank"
    shard.close()


def test_a_call_changes_no_later_result_of_the_filter():
    """twins through the same updates and resampling, one of them asked for rooms at every turn: poses, weights and every map equal"""
    ends = []
    for ask in (False, True):
        s, tr = _handle()
        for k in range(4):
            s.update(tr.scans[k], ODO, seed=5, sequence=k)
            if ask:
                _ask(s, "strongest", True); _ask(s, k, False)
            if k in (1, 2):
                s.resample(0.37 + 0.1 * k)
                if ask:
                    _ask(s, 7 - k, True)
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
    got = [_ask(s, k, True) for k in range(N)]                             # nothing in between: likelihoodData's copies are still owed
    moved = [k for k in range(N) if idx[k] != k and not np.array_equal(before[k], before[idx[k]], equal_nan=True)]
    assert moved, "the draw put another particle's map into at least one slot"
    for k in range(N):
        assert got[k]["shown"] == k
        _against(got[k], before[idx[k]], f"slot {k} holds the map of particle {idx[k]}", True)
    s.close()


def test_batched_handle():
    S, n, ext = 3, 4, 6.0
    tr = synth.make_trace(ext, RES, B, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    with pytest.raises(GmsError) as e:
        _ask(bat, "strongest", True, filter=1)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    for f in range(S):
        for k in range(n):
            got = _ask(bat, k, bool((f + k) & 1), filter=f)
            assert got["shown"] == f * n + k
            _against(got, bat.map_of(f, k), f"filter {f}, particle {k}", bool((f + k) & 1))
        got = _ask(bat, "strongest", True, filter=f)
        assert got["shown"] == bat.view("strongest", filter=f)[1] and f * n <= got["shown"] < (f + 1) * n
        _against(got, bat.map_of(f, got["shown"] - f * n), f"filter {f}, strongest", True)
    with pytest.raises(IndexError):
        _ask(bat, "strongest", True, filter=S)
    bat.close()


def test_device_form():
    import torch
    s, tr = _handle()
    _drive(s, tr)
    rect = (3, 5, 101, 77)
    host = _ask(s, "strongest", True, rect)
    n = host["labels"].size
    lab = torch.full((n + 24,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    dep = torch.full((n + 24,), 0x5A5A, dtype=torch.int16, device="cuda")
    rooms = torch.full((7 * 512,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    doors = torch.full((6 * 512,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GmsError) as e:
        s.rooms_dev("strongest", lab.view(torch.uint8)[1:], dep, rooms, doors, sh, not_free=True, rect=rect, **KW)
    assert e.value.code == GMS_ERR_INVALID
    nr, nd = s.rooms_dev("strongest", lab, dep, rooms, doors, sh, not_free=True, rect=rect, **KW)
    s.grid_map.synchronize(); torch.cuda.synchronize()
    assert (nr, nd) == (host["n_rooms"], host["n_doors"]) and sh.cpu().tolist() == [host["shown"], -7, -7, -7]
    raw_lab, raw_dep = lab.cpu().numpy().view(np.uint32), dep.cpu().numpy().view(np.uint16)
    assert np.array_equal(raw_lab[:n].reshape(host["labels"].shape), host["labels"]) and (raw_lab[n:] == 0x5A5A5A5A).all()
    assert np.array_equal(raw_dep[:n].reshape(host["depth"].shape), host["depth"]) and (raw_dep[n:] == 0x5A5A).all()
    assert np.array_equal(rooms.cpu().numpy()[:7 * nr].view(_lib.ROOM_DTYPE), host["rooms"])
    assert np.array_equal(doors.cpu().numpy()[:6 * nd].view(_lib.DOOR_DTYPE), host["doors"])
    s.close()
