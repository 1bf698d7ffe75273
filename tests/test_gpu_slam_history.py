"""Every particle's path through resampling (include/gridmapslam.h "trajectories"): gms_slam_set_history, gms_slam_trajectory[_dev] and
gms_slam_trajectories against a host model (_history_expect) built only from the getters that were there before -- the poses after every
update, did_resample / the indices after every resampling step -- and, for the property the feature exists for, against the oracle:
integrating the scans along a returned trajectory reproduces that particle's map.  Poses and ancestors compare with array_equal.
Maps of 24 x 24 cells (1.2 m at 0.05), scans of 8 beams."""
import ctypes as C
import math

import numpy as np
import pytest

from _history_expect import HistoryModel
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError, load, ptr
from gridmap_slam_robot_amd.replay import ParticleMapsReplay
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
EXT, RES, B = 1.2, 0.05, 8
GEO = (EXT, EXT, RES, (-EXT / 2, -EXT / 2))
TRACE = synth.make_trace(EXT, RES, B, T=64, seed=11, n_scans=16)          # sixteen scans of a slow circle: 5.6 degrees a step
ODO = [(float(math.hypot(*(TRACE.poses[(t + 1) % 16][:2] - TRACE.poses[t][:2]))), 2 * math.pi / 64) for t in range(16)]


def _single(n, cap=None):
    s = SLAMParticleMaps(*GEO, num_particles=n, max_beams=64)
    if cap is not None:
        s.set_history(cap)
    return s


def _poses(s):
    return s.pf.get_poses()


def _step(s, model, k, seed, odometry=None, sample_motion=True):
    """update number k, then the poses a caller could always read"""
    z, u = TRACE.scans[k % 16], (ODO[k % 16] if odometry is None else odometry)
    if isinstance(s, SLAMParticleMapsBatch):
        s.update([z] * s.num_filters, [u] * s.num_filters, seeds=seed, sequence=k, fetch=False, sample_motion=sample_motion)
    else:
        s.update(z, u, seed=seed, sequence=k, fetch=False, sample_motion=sample_motion)
    if model is not None:
        model.update(_poses(s))


def _skewed(rng, n, power=6):
    w = rng.random(n) ** power
    return w / w.sum()


def _draw(s, model, rng, r01):
    """resample() over random weights (set through the handle's filter, so that the draws do not depend on the scan); the indices feed the model"""
    s.pf.set_weights(_skewed(rng, s.num_particles))
    idx, _ = s.resample(r01, want_indices=True)
    model.resample([True], idx)
    return idx


def _check_against(s, model, f=0, batch=False):
    """trajectories(ancestors), every single trajectory and history_len against the model; returns (xy, anc)"""
    want_xy, want_anc = model.trajectories(f)
    assert s.history_len() == (model.total, model.kept)
    xy, anc = s.trajectories(f, ancestors=True) if batch else s.trajectories(ancestors=True)
    assert xy.shape == want_xy.shape and np.array_equal(xy, want_xy)
    assert np.array_equal(anc, want_anc)
    plain = s.trajectories(f) if batch else s.trajectories()
    assert np.array_equal(plain, want_xy)
    return xy, anc


def _not_vacuous(idx_seen, anc):
    assert any((i != np.arange(i.shape[-1])).any() for i in idx_seen), "no draw with non-identity indices"
    assert any(np.unique(row).size >= 2 for row in anc), "a single ancestor at every kept depth"
    assert any(np.unique(row).size < row.size for row in anc), "no two particles share an ancestor anywhere"


def test_three_call_path_with_draws_between_and_after_updates():
    n, cap, steps = 70, 32, 12
    s, model, rng = _single(n, cap), HistoryModel(1, n, cap), np.random.default_rng(1)
    assert s.history_len() == (0, 0) and s.trajectories().shape == (0, n, 3)
    draws_after = {2: 1, 3: 2, 7: 1, 11: 1}                   # two draws between updates 3 and 4: the compose; one after the last update
    seen = []
    for k in range(steps):
        # update 5 turns by more than 30 degrees (its scan is not integrated), update 6 draws no motion sample: steps like any other
        _step(s, model, k, seed=5, odometry=(0.01, 0.6) if k == 5 else None, sample_motion=k != 6)
        for _ in range(draws_after.get(k + 1, 0)):
            seen.append(_draw(s, model, rng, float(rng.random())))
    xy, anc = _check_against(s, model)
    assert xy.shape == (steps, n, 3)
    for k in range(n):
        t, shown = s.trajectory(k)
        assert shown == k and np.array_equal(t, xy[:, k])
    assert np.array_equal(_poses(s), xy[-1]), "the present pose of every slot is the last entry of its trajectory"
    _not_vacuous(seen, anc)
    # the device forms write the same values
    import torch
    out, sh = torch.zeros((cap, 3), dtype=torch.float32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                  # (the handle has a stream of its own)
    s.trajectory(n - 1, out=out, shown_out=sh)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:steps], xy[:, n - 1]) and not out.cpu().numpy()[steps:].any() and int(sh.item()) == n - 1
    s.close()


def test_the_rule_decided_on_the_device_and_the_frame_call():
    """resample_if and frame() with fractions 2.0 (always draws) and 0.0 (never), nothing read back in between; the model comes from a second
    handle that takes the same steps as three calls and reads poses, flags and indices back after each"""
    n, cap = 70, 32
    frames, _ = synth.make_recording(EXT, B, T=64, seed=11, n_frames=6)
    fractions = [2.0, 0.0, 2.0, 2.0, 0.0, 2.0]
    r01 = np.random.default_rng(2).random(12)
    a = _single(n, cap)
    for k in range(6):
        _step(a, None, k, seed=9)
        a.resample_if(float(r01[k]), fractions[k])
    for k, f in enumerate(frames):
        a.frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, seed=9, sequence=6 + k, r01=float(r01[6 + k]), fraction=fractions[k])
    b, model, seen = _single(n), HistoryModel(1, n, cap), []

    def rule(k, fraction):
        b.resample_if(float(r01[k]), fraction)
        did = b.pf.did_resample()
        assert did == (fraction > 1.0)
        seen.append(b.pf.last_resample_indices())
        model.resample([did], seen[-1])
    for k in range(6):
        _step(b, model, k, seed=9)
        rule(k, fractions[k])
    for k, f in enumerate(frames):
        obs = b.grid_map.deskew(f.angle, f.distance, f.hit, f.d_center, f.d_theta)
        b.update(obs, (f.d_center, f.d_theta), seed=9, sequence=6 + k, fetch=False)
        model.update(_poses(b))
        rule(6 + k, fractions[k])
    assert np.array_equal(_poses(a), _poses(b)), "frame() is documented to compute what the three calls do"
    _, anc = _check_against(a, model)
    _not_vacuous(seen, anc)
    a.close(); b.close()


_BIG = {}


def _big_run():
    """1100 particles (five workgroups of the streams, more than one turn of the walk's lanes), capacity 80, 100 updates, a draw every
    third: the ring wraps; returns (handle results, model results, rows per chunk)"""
    n, cap, steps = 1100, 80, 100
    s, model, rng = _single(n, cap), HistoryModel(1, n, cap), np.random.default_rng(3)
    seen = []
    for k in range(steps):
        _step(s, model, k, seed=3)
        if k % 3 == 2:
            seen.append(_draw(s, model, rng, float(rng.random())))
    xy, anc = _check_against(s, model)
    assert s.history_len() == (steps, cap) and xy.shape == (cap, n, 3)
    _not_vacuous(seen, anc)
    singles = {k: s.trajectory(k) for k in (0, 63, 64, 1023, 1024, n - 1)}
    for k, (t, shown) in singles.items():
        assert shown == k and np.array_equal(t, xy[:, k])
    rows = s.history_walk_rows()
    s.close()
    return xy, anc, rows


def test_more_than_one_workgroup_per_filter_a_wrapped_ring_and_chunk_boundaries():
    xy, anc, rows = _BIG["lds"] = _big_run()
    assert rows == 8192 // 1100 == 7 and 80 > 2 * rows, "the walk must cross chunk boundaries: 80 kept rows in chunks of 7"


def test_the_memory_form_of_the_walk(monkeypatch):
    monkeypatch.setenv("GMS_SLAM_HISTORY_WALK", "mem")
    xy, anc, rows = _big_run()
    assert rows == 0, "the environment switch must force the memory form"
    monkeypatch.delenv("GMS_SLAM_HISTORY_WALK")
    lds = _BIG.get("lds") or _big_run()
    assert lds[2] == 7 and np.array_equal(xy, lds[0]) and np.array_equal(anc, lds[1])


def test_batched_handle_filters_draw_or_not_on_their_own():
    S, n, cap, steps = 3, 70, 32, 9
    seeds = np.array([21, 22, 23], dtype=np.uint64)
    rng = np.random.default_rng(4)
    # per step and filter: skewed weights (Neff far below n / 2: draws) or uniform ones (Neff = n: does not), under the one fraction 0.5
    draws = rng.random((steps, S)) < 0.5
    draws[0], draws[1] = (True, False, True), (False, True, False)
    W = np.where(draws[:, :, None], np.stack([[_skewed(rng, n) for _ in range(S)] for _ in range(steps)]), 1.0 / n)
    r01 = rng.random((steps, S))
    bt = SLAMParticleMapsBatch(S, *GEO, num_particles=n, max_beams=64)
    bt.set_history(cap)
    for k in range(steps):
        bt.update([TRACE.scans[k]] * S, [ODO[k]] * S, seeds=seeds, sequence=k, fetch=True)
        bt.pf.set_weights(W[k])
        bt.resample_if(r01[k], 0.5)
    for f in range(S):
        one, model, seen = _single(n, cap), HistoryModel(1, n, cap), []
        for k in range(steps):
            one.update(TRACE.scans[k], ODO[k], seed=int(seeds[f]), sequence=k, fetch=True)
            model.update(_poses(one))
            one.pf.set_weights(W[k, f])
            one.resample_if(float(r01[k, f]), 0.5)
            did = one.pf.did_resample()
            assert did == draws[k, f]
            seen.append(one.pf.last_resample_indices())
            model.resample([did], seen[-1])
        xy, anc = _check_against(one, model)
        _not_vacuous(seen, anc)
        got_xy, got_anc = bt.trajectories(f, ancestors=True)
        assert np.array_equal(got_xy, xy) and np.array_equal(got_anc, anc), f"filter {f}"
        for k in (0, n - 1):
            t, shown = bt.trajectory(k, filter=f)
            assert shown == f * n + k and np.array_equal(t, xy[:, k])
        _, viewed = bt.view("strongest", filter=f)
        t, shown = bt.trajectory("strongest", filter=f)
        assert shown == viewed and np.array_equal(t, xy[:, shown - f * n])
        one.close()
    assert bt.history_len() == (steps, steps)
    bt.close()


def test_ring_and_state():
    n, cap, steps = 70, 5, 12
    s, model, rng = _single(n, cap), HistoryModel(1, n, cap), np.random.default_rng(5)
    for k in range(steps):
        _step(s, model, k, seed=6)
        if k % 2:
            _draw(s, model, rng, float(rng.random()))
    xy, _ = _check_against(s, model)                          # the last 5 rows, oldest first
    assert s.history_len() == (12, 5) and xy.shape == (5, n, 3)
    # room for fewer steps than are kept: the error, the count, nothing written
    L, buf, c = load(), np.full((4, 3), -5.0, np.float32), C.c_int32(-1)
    assert L.gms_slam_trajectory(s._h, 3, 0, ptr(buf), 4, C.byref(c), None) == GMS_ERR_INVALID and c.value == 5 and (buf == -5.0).all()
    big = np.full((4, n, 3), -5.0, np.float32)
    assert L.gms_slam_trajectories(s._h, 0, ptr(big), None, 4, C.byref(c)) == GMS_ERR_INVALID and c.value == 5 and (big == -5.0).all()
    with pytest.raises(GmsError) as e:
        s.trajectory(n)
    assert e.value.code == GMS_ERR_INVALID
    # set_poses between updates changes neither the rows already there nor the lineage; the next row starts from the new poses
    before = s.trajectories(ancestors=True)
    s.set_poses(np.tile(np.float32([0.1, -0.1, 0.3]), (n, 1)))
    after = s.trajectories(ancestors=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and s.history_len() == (12, 5)
    _step(s, model, 12, seed=6, sample_motion=False)
    xy, _ = _check_against(s, model)
    assert np.array_equal(xy[-1], np.tile(np.float32([0.1, -0.1, 0.3]), (n, 1)))
    # reset(): nothing kept, still on, the same capacity; the statistics name no strongest particle until the next update
    s.reset(); model.clear()
    assert s.history_len() == (0, 0) and s.trajectory(3)[0].shape == (0, 3)
    with pytest.raises(GmsError) as e:
        s.trajectory("strongest")
    assert e.value.code == GMS_ERR_STATE
    for k in range(7):
        _step(s, model, k, seed=8)
        if k == 3:
            _draw(s, model, rng, float(rng.random()))
    _check_against(s, model)
    assert s.history_len() == (7, 5)
    # off: the calls say so
    s.set_history(0)
    for call in (s.trajectory, s.trajectories, s.history_len):
        with pytest.raises(GmsError) as e:
            call()
        assert e.value.code == GMS_ERR_STATE
    with pytest.raises(GmsError) as e:
        s.set_history(-1)
    assert e.value.code == GMS_ERR_INVALID
    s.close()
    # a shard of a filter is refused
    sh = SLAMParticleMaps.__new__(SLAMParticleMaps)
    sh._init_shard(*GEO, 256, 0, 512, max_beams=64)
    with pytest.raises(GmsError) as e:
        sh.set_history(4)
    assert e.value.code == GMS_ERR_STATE
    sh.close()


def test_the_recorded_pose_is_the_refined_one():
    n, cap = 70, 8
    got = {}
    for refine in (False, True):
        s, model = _single(n, cap), HistoryModel(1, n, cap)
        s.set_refine(refine)
        for k in range(4):
            _step(s, model, k, seed=12)
        got[refine] = _check_against(s, model)[0]
        assert np.array_equal(got[refine][-1], _poses(s))
        s.close()
    assert (got[True] != got[False]).any(), "the refinement moved no pose: the case shows nothing"


# Chosen on the CPU from the oracle's own run (orc.Slam.update / resample with this seed, these scans and r01 = R01_7): Neff falls below
# n / 2 = 32 after updates 8, 10, 12 and 14 there (23.9, 16.7, 29.1, 22.6): no rounding difference of the device closes all four margins.
SEED_7 = 1
R01_7 = np.random.default_rng(77).random(15)


def test_a_trajectory_is_the_path_its_map_was_built_along():
    """64 particles, 15 updates with the weights the scans give, `if (neff < n / 2) resample()` decided on the device: integrating the same
    scans along the returned trajectory (the oracle's integrateObservation; an update that turned by more than 30 degrees integrated
    nothing) into a blank map reproduces map_of(that particle) -- to the tolerance test_gpu_slam_particle_maps.py applies to logData:
    the same cells touched, values to 1e-13 relative."""
    n, cap, steps = 64, 16, 15
    odo = [ODO[k] if k != 8 else (0.01, 0.6) for k in range(steps)]
    s = _single(n, cap)
    drew = 0
    for k in range(steps):
        s.update(TRACE.scans[k], odo[k], seed=SEED_7, sequence=k, fetch=True)
        s.resample_if(float(R01_7[k]), 0.5)
        drew += int(s.pf.did_resample())
    assert drew >= 1, "no resampling step happened: pick another seed"
    g = orc.Grid(*GEO[:3], *GEO[3])
    _, strongest = s.trajectory("strongest")
    anc = s.trajectories(ancestors=True)[1]
    assert any(np.unique(row).size >= 2 for row in anc) and (anc[0] != np.arange(n)).any()
    for which in ("strongest", 0, n - 1):
        traj, shown = s.trajectory(which)
        assert shown == (strongest if which == "strongest" else which) and traj.shape == (steps, 3)
        log = g.new_log()
        for k in range(steps):
            if abs(odo[k][1]) <= math.radians(30):
                g.integrate(log, TRACE.scans[k], traj[k])
        dev = s.map_of(shown).reshape(-1)
        assert np.array_equal(dev != 0, log != 0), f"particle {shown}: another set of cells touched"
        err = np.abs(dev - log)
        assert (err <= 1e-13 * np.maximum(np.abs(log), 1.0)).all(), f"particle {shown}: log-odds off by {err.max():.3e}"
    s.close()


def test_no_result_changes_with_the_history_on():
    n = 70
    got = {}
    for on in (False, True):
        s, rng = _single(n, 4 if on else None), np.random.default_rng(6)
        for k in range(10):
            s.update(TRACE.scans[k], ODO[k], seed=2, sequence=k, fetch=True)
            s.resample_if(float(rng.random()), 0.9)
        if on:
            s.trajectories(ancestors=True); s.trajectory("strongest")           # (reading the history changes nothing either)
        got[on] = (_poses(s), s.pf.get_weights(), s.maps(), s.maps(likelihood=True), s.maps_copied())
        s.close()
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(a, b)


def test_replay_keeps_the_path_of_the_shown_particle():
    frames, _ = synth.make_recording(EXT, B, T=64, seed=11, n_frames=5)
    s = SLAMParticleMaps(*GEO, num_particles=70, max_beams=64)
    rp = ParticleMapsReplay(s, seed=4, resample_fraction=2.0, history=8)
    for k, f in enumerate(frames):
        rp.step(f, 0.1 * k + 0.05)
    traj, shown = rp.trajectory()
    assert traj.shape == (5, 3) and shown == s.view("strongest")[1]
    assert np.array_equal(traj[-1], _poses(s)[shown])
    s.close()
