"""Trajectory rollouts of the per-particle filter (include/gridmapslam.h "trajectory rollouts"): gms_slam_rollout[_dev] -- the caller's
start poses, or the shown particle's own, in the shown particle's own map -- against the expectation of tests/_rollout_expect.py on
that particle's downloaded logData.  Every comparison is array_equal.  24 particles x 120 x 120 cells, 90 beams, a few updates of the
synthetic room with resampling in between (the maps' generation flips, so it has to be picked from the epoch counters)."""
import numpy as np
import pytest

import _rollout_expect as rx
from gridmap_slam_robot_amd import ROLLOUT_DTYPE, SLAMParticleMaps, SLAMParticleMapsBatch, rollout_arcs, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GMS_ROLLOUT_CANDIDATES, GmsError

pytestmark = pytest.mark.gpu

RES, B, N, EXT = 0.05, 90, 24, 6.0
ODO = (0.02, 0.1)
GEO = rx.Geometry(120, 120, RES, -EXT / 2, -EXT / 2)
K, T, R = GMS_ROLLOUT_CANDIDATES + 1, 65, 50
ARCS = rollout_arcs(np.linspace(0.2, 1.0, K), np.linspace(-1.2, 1.2, K), 3.0 / T, T)
PTS = np.array([[0.15, 0.1], [0.15, -0.1], [-0.15, 0.1], [-0.15, -0.1], [0.2, 0.0]], np.float32)


def _same(got, want, where):
    assert got.dtype == ROLLOUT_DTYPE and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"{where}: {len(bad)} of {want.size} records differ, first at {bad[:1].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _handle(n=N, **kw):
    s = SLAMParticleMaps(EXT, EXT, RES, (-EXT / 2, -EXT / 2), num_particles=n, max_beams=300, **kw)
    tr = synth.make_trace(EXT, RES, B, T=8, seed=23)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    return s, tr


def _starts(tr):
    """the trace's own poses, the map's corner and a pose outside"""
    return np.concatenate([tr.poses[:3], [[-2.99, -2.99, 0.7], [3.5, 0.0, 0.0]]]).astype(np.float32)


def _want(log, poses, inflate=0, not_free=False, **kw):
    return rx.expect(GEO, log, poses, ARCS, PTS, R, inflate, not_free, **kw)


def test_named_particles_the_strongest_and_the_particles_own_pose():
    s, tr = _handle()
    assert (s.W, s.H) == (120, 120)
    starts = _starts(tr)
    with pytest.raises(GmsError) as e:
        s.rollout(ARCS, PTS, starts, max_range=R)
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    with pytest.raises(GmsError) as e:
        s.rollout(ARCS, PTS, max_range=R)
    assert e.value.code == GMS_ERR_STATE
    rec, shown = s.rollout(ARCS, PTS, starts, which=3, max_range=R)
    assert shown == 3 and (rec["first_hit"] == 0).all(), "a fresh map is all unknown: the planner's mode blocks it"
    for k in range(3):
        s.update(tr.scans[k], ODO, seed=5, sequence=k)
        if k == 1:
            s.resample(0.37)
    logs = [s.map_of(k) for k in range(N)]
    poses = s.pf.get_poses()
    wants = [_want(logs[k], starts) for k in range(N)]
    assert any(not np.array_equal(wants[0], w) for w in wants[1:]), "maps that differ in what the arcs meet"
    assert all((w["first_hit"] > 0).any() and (w["first_hit"] < T).any() for w in wants)
    for k in range(N):
        got, shown = s.rollout(ARCS, PTS, starts, which=k, max_range=R, not_free=False)
        assert shown == k
        _same(got, wants[k], f"particle {k}")
        own, shown = s.rollout(ARCS, PTS, which=k, max_range=R, not_free=False)
        assert shown == k and own.shape == (1, K)
        _same(own, _want(logs[k], poses[k:k + 1]), f"particle {k} from its own pose")
    strongest = s.view("strongest")[1]
    assert strongest == s.last_stats["strongest"]
    got, shown = s.rollout(ARCS, PTS, starts, max_range=R, inflate=2)
    assert shown == strongest
    _same(got, _want(logs[strongest], starts, 2, True), "strongest, inflated, the planner's mode")
    own, shown = s.rollout(ARCS, PTS, max_range=R, inflate=2, not_free=False)
    assert shown == strongest
    _same(own, _want(logs[strongest], poses[strongest:strongest + 1], 2, False), "strongest from its own pose")
    clear, cost = s.clearance(strongest, max_radius=30)[0], s.reach(strongest, max_cost=0xFFFE, not_free=False)[0]
    got, _ = s.rollout(ARCS, PTS, starts, which=strongest, max_range=R, not_free=False, clear=clear, cost=cost)
    want = _want(logs[strongest], starts, clear=clear, cost=cost)
    assert (want["min_d2"] < 0xFFFF).any() and (want["best_cost"] < 0xFFFF).any()
    _same(got, want, "with the particle's own fields")
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            s.rollout(ARCS, PTS, starts, which=bad, max_range=R)
        assert e.value.code == GMS_ERR_INVALID
    with pytest.raises(GmsError) as e:
        s.rollout(ARCS, PTS, starts[:0], which=0, max_range=R)
    assert e.value.code == GMS_ERR_INVALID, "poses without a pose"
    again = [s.map_of(k) for k in range(N)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(logs, again)), "a rollout changes no map"
    s.reset()
    with pytest.raises(GmsError) as e:
        s.rollout(ARCS, PTS, max_range=R)
    assert e.value.code == GMS_ERR_STATE, "... and no strongest particle after a reset"
    s.close()


def test_after_a_conditional_resample_that_drew_and_one_that_did_not():
    s, tr = _handle(n=8)
    starts = _starts(tr)
    for k, fraction in enumerate((2.0, 0.0, 2.0, 0.0)):                        # Neff < 2 n always holds, Neff < 0 never
        s.update(tr.scans[k], ODO, seed=7, sequence=k)
        s.resample_if(0.41, fraction)                                          # ... and nothing is read back before the rollouts
        got = [s.rollout(ARCS, PTS, starts, which=j, max_range=R, not_free=False) for j in (0, 5)]
        own, shown = s.rollout(ARCS, PTS, max_range=R, not_free=False)
        assert bool(np.asarray(s.pf.did_resample()).reshape(-1)[0]) == (fraction > 1), k
        poses = s.pf.get_poses()
        for j, (rec, sh) in zip((0, 5), got):
            assert sh == j
            _same(rec, _want(s.map_of(j), starts), f"update {k}, particle {j}, drew: {fraction > 1}")
        _same(own, _want(s.map_of(shown), poses[shown:shown + 1]), f"update {k}, the shown particle's own pose")
    s.close()


def test_batched_handle_and_the_device_form():
    import torch
    S, n = 3, 4
    tr = synth.make_trace(EXT, RES, B, T=12, seed=23)
    bat = SLAMParticleMapsBatch(S, EXT, EXT, RES, (-EXT / 2, -EXT / 2), num_particles=n, max_beams=300)
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    starts = _starts(tr)
    with pytest.raises(GmsError) as e:
        bat.rollout(ARCS, PTS, starts, filter=1, max_range=R)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    got, shown = bat.rollout(ARCS, PTS, starts, filter=1, max_range=R, not_free=False)
    assert shown == bat.view("strongest", filter=1)[1] and n <= shown < 2 * n, "a slot of filter 1"
    want1 = _want(bat.map_of(1, shown - n), starts)
    _same(got, want1, "filter 1, strongest")
    own, sh = bat.rollout(ARCS, PTS, filter=2, max_range=R, not_free=False)
    assert 2 * n <= sh < 3 * n
    _same(own, _want(bat.map_of(2, sh - 2 * n), bat.pf.get_poses().reshape(-1, 3)[sh:sh + 1]), "filter 2's strongest from its own pose")
    for f, k in ((0, 3), (2, 1)):
        got, sh = bat.rollout(ARCS, PTS, starts, which=k, filter=f, max_range=R, not_free=False)
        assert sh == f * n + k
        _same(got, _want(bat.map_of(f, k), starts), f"filter {f}, particle {k}")
    with pytest.raises(IndexError):
        bat.rollout(ARCS, PTS, starts, filter=S, max_range=R)
    # the device form: records, the shown slot, nothing past either
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_poses, d_arcs, d_pts, P = dev(starts), dev(ARCS), dev(PTS), len(starts)
    out = torch.full((32 * P * K + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    shw = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = ((d_arcs.data_ptr(), K, T), (d_pts.data_ptr(), len(PTS)), (d_poses.data_ptr(), P))
    with pytest.raises(GmsError) as e:
        bat.rollout_dev(out[8:], *args, filter=1, max_range=R, not_free=False, shown_out=shw)
    assert e.value.code == GMS_ERR_INVALID
    bat.rollout_dev(out, *args, filter=1, max_range=R, not_free=False, shown_out=shw)
    bat.grid_map.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy()
    _same(raw[:32 * P * K].view(ROLLOUT_DTYPE).reshape(P, K), want1, "the device form")
    assert (raw[32 * P * K:] == 0xA5).all() and shw.cpu().tolist() == [shown, -7, -7, -7]
    bat.close()
