"""One call per recorded revolution for the filter with a map per particle: gms_slam_frame_per_particle and gms_slam_frame_batch
(GridMapApp.onHandleData, J/app/GridMapApp.java:133-192: de-skew :143-175, SLAM.update :178, `if (neff < n / 2) resample()` :185-186).

  * the scalar frame against the three calls it stands for (gms_map_deskew -> gms_slam_update_per_particle_dev ->
    gms_slam_resample_maps_if): identity, np.array_equal throughout;
  * the scalar frame against the oracle's literal SLAM loop, the oracle fed the device's poses (as test_gpu_slam_particle_maps.py does)
    and orc.deskew of the raw revolution, with that file's helpers and tolerances;
  * the batch frame against stand-alone handles driven by the scalar frame: identity;
  * the batch de-skew's rows against GridMap.deskew with each filter's own (length, odometry);
  * the refusals; the replay classes.

The resampling fractions were picked on the CPU from the oracle's own Neff sequences (see the comments at _REC_FRACTIONS and
_BATCH_FRACTIONS)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError, load
from gridmap_slam_robot_amd.replay import ParticleMapsBatchReplay, ParticleMapsReplay
from gridmap_slam_robot_amd.trace import Frame, read_trace
from oracle import oracle as orc

from _checks import assert_resample_indices
from test_gpu_slam_particle_maps import _compare_maps, _compare_weights

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REC = os.path.join(HERE, "golden", "recording_360.bin")
THREADS = min(16, os.cpu_count() or 1)

# The recording's map: 25.6 m at 5 cm holds the drive (test_gpu_trace_replay.py); 512 x 512 cells x 16 bytes x 2 generations = 8.4 MB a
# particle, so 96 particles keep a handle's maps at 0.8 GB.
REC_EXT, REC_RES, REC_N, REC_SEED = 25.6, 0.05, 96, 99

# The oracle alone over the recording at these sizes (96 particles, seed 99, every particle started at the drive's start pose, the
# rule applied at fraction 0.5), Neff / n per frame:
#   frame 0: NaN (a blank map weighs 360 beams 0.1^360 = 0 for every particle: update() divides 0 by 0, as the reference does)
#   frames 1-63: 0.0104 (= 1 / n: one particle holds all the weight) ... 0.0339; sorted tail 0.021 0.021 0.030 0.034
# 360 beams collapse the weights every revolution, so no fraction lies between the extremes AND 5 % of n away from every frame (the
# whole sequence spans 2.4 % of n).  Hence the two-run form: 0.5 lies 46 % of n above every frame's Neff -- every frame with a defined
# Neff resamples; 0.0 asks `neff < 0`, which no Neff satisfies (Neff = 1 / sum(w^2) >= 1 > 0, a margin of one whole particle that no
# last-ulp difference of a weight reaches) -- the rule is evaluated on the device and never draws; and a third run with fraction < 0
# skips the step and must copy nothing.
_REC_FRACTIONS = {"always": 0.5, "never": 0.0, "skipped": -1.0}


def _rec_frames():
    frames = read_trace(REC)
    assert len(frames) == 64 and all(len(f.angle) == 360 for f in frames)
    return frames


def _rec_start():
    return synth.true_pose(synth.make_world(REC_EXT, 4321), -1, 64)


def _rec_handle(n=REC_N, ext=REC_EXT, max_beams=512):
    return SLAMParticleMaps(ext, ext, REC_RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=max_beams)


def _three_calls(dev, f, seed, k, r01, fraction):
    """what frame() stands for: gms_map_deskew on the handle's map, gms_slam_update_per_particle_dev, gms_slam_resample_maps_if"""
    d, B = dev.grid_map.deskew_dev(f.angle, f.distance, f.hit, f.d_center, f.d_theta)
    dev.update_dev(d, B, (f.d_center, f.d_theta), seed=seed, sequence=k)
    if fraction >= 0:
        dev.resample_if(r01, fraction)


def _same_state(a, b, where, maps=True):
    Pa, Wa = a.get_particles()
    Pb, Wb = b.get_particles()
    assert np.array_equal(Pa, Pb), f"{where}: poses"
    assert np.array_equal(Wa, Wb), f"{where}: weights"
    assert a.maps_copied() == b.maps_copied(), f"{where}: maps copied"
    if maps:
        for lik in (False, True):
            assert np.array_equal(a.maps(likelihood=lik), b.maps(likelihood=lik)), f"{where}: {'likelihoodData' if lik else 'logData'}"


def _frame_against_three_calls(frames, fraction, refine=False, label=""):
    """two handles over `frames`, one frame() call against the three calls; returns did_resample per frame"""
    one, three = _rec_handle(), _rec_handle()
    try:
        start = np.tile(np.asarray(_rec_start(), np.float32), (REC_N, 1))
        one.set_poses(start); three.set_poses(start)
        if refine:
            one.set_refine(True); three.set_refine(True)
        rng = np.random.default_rng(5)
        did, copied = [], 0
        for k, f in enumerate(frames):
            r01 = float(rng.random())
            one.frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, seed=REC_SEED, sequence=k, r01=r01, fraction=fraction)
            _three_calls(three, f, REC_SEED, k, r01, fraction)
            now = one.maps_copied()
            assert now == three.maps_copied(), f"{label} frame {k}: maps copied"
            drew = now != copied
            copied = now
            if fraction >= 0:
                assert one.pf.did_resample() == three.pf.did_resample() == drew, f"{label} frame {k}: did_resample"
            if drew:
                assert np.array_equal(one.pf.last_resample_indices(), three.pf.last_resample_indices()), f"{label} frame {k}: indices"
            did.append(drew)
        assert np.isfinite(one.get_particles()[1]).all(), f"{label}: the last frame's weights must be defined for the comparison to mean something"
        _same_state(one, three, f"{label} after {len(frames)} frames")
        return did
    finally:
        one.close(); three.close()


def test_scalar_frame_equals_the_three_calls_and_takes_both_branches():
    frames = _rec_frames()
    did = _frame_against_three_calls(frames, _REC_FRACTIONS["always"], label="fraction 0.5")
    print("fraction 0.5: resampled on frames", [k for k, d in enumerate(did) if d])
    assert not did[0], "frame 0 weighs every particle 0 over blank maps: Neff is NaN and the rule says no"
    assert all(did[1:]), "every later frame's Neff lies far below n / 2"
    did = _frame_against_three_calls(frames[:16], _REC_FRACTIONS["never"], label="fraction 0.0")
    assert not any(did), "no Neff is below 0: the rule is evaluated and never draws"
    did = _frame_against_three_calls(frames[:8], _REC_FRACTIONS["skipped"], label="fraction < 0")
    assert not any(did), "fraction < 0 skips the resampling step: nothing is copied"


def test_scalar_frame_equals_the_three_calls_with_the_pose_refinement():
    did = _frame_against_three_calls(_rec_frames()[:10], _REC_FRACTIONS["always"], refine=True, label="refine")
    assert any(did) and not all(did)


def test_scalar_frame_against_the_oracle():
    """frame() with fraction < 0, so that the poses read back are the ones the scan was scored and integrated at; the oracle takes
    them (set_poses) and orc.deskew of the raw revolution and runs update(sample_motion = False), deciding skipUpdate from dTheta
    itself.  Every other measurement of the recording (180 per revolution: a blank map's 0.1^180 is still a number, as in
    test_gpu_slam_particle_maps.py), one frame turned past 30 degrees.  Between frames both sides resample by the existing calls."""
    N, T, ext, seed = 64, 10, 12.8, 7
    frames = _rec_frames()[:T]
    for f in frames:
        f.angle, f.distance, f.hit = f.angle[::2].copy(), f.distance[::2].copy(), f.hit[::2].copy()
    frames[4].d_theta = math.radians(31.0)                                               # skipUpdate (SLAM.java:82)
    dev = _rec_handle(N, ext)
    g = orc.Grid(ext, ext, REC_RES, -ext / 2, -ext / 2)
    o = orc.Slam(g, N)
    try:
        P0 = np.tile(np.asarray(_rec_start(), np.float32), (N, 1))
        dev.set_poses(P0); o.set_poses(P0)
        rng = np.random.default_rng(3)
        resampled = 0
        for k, f in enumerate(frames):
            where = f"frame {k}"
            prev, before = o.poses, (dev.maps() if k == 4 else None)
            neff = dev.frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, seed=seed, sequence=k, fraction=-1.0, fetch=True)
            z = orc.deskew(f.angle, f.distance, f.hit, f.d_center, f.d_theta)
            got = dev.last_beams()
            assert np.array_equal(got["hit"], z["hit"])
            for key in ("local_x", "local_y", "distance"):
                assert np.max(np.abs(got[key] - z[key])) <= 1e-13, f"{where}: de-skew {key}"     # (test_gpu_trace_replay.py's bound)
            P = dev.get_particles()[0]
            Po = orc.sample_motion(prev, f.d_center, f.d_theta, seed=seed, sequence=k)
            assert (np.all(P == Po, axis=1)).mean() > 0.99 and np.max(np.abs(P - Po)) <= 2e-6, f"{where}: motion samples"
            o.set_poses(P)
            neff_o = o.update(z, (f.d_center, f.d_theta), sample_motion=False, threads=THREADS)
            st = dev.last_stats
            _compare_weights(dev.get_particles()[1], o.weights, where)
            assert st["strongest"] == o.strongest and st["n_zero"] == int((o.weights == 0).sum())
            print(f"{where}: Neff device {neff:.6f} oracle {neff_o:.6f}")
            assert abs(neff - neff_o) <= 1e-11 * neff_o
            assert np.allclose(dev.get_weighted_pose(), o.weighted_pose(), rtol=0, atol=2e-6)
            if k == 4:
                assert np.array_equal(dev.maps(), before), "a turn past 30 degrees integrates nothing"
            if k in (0, 4, 5, T - 1):
                _compare_maps(dev, o, where)
            if neff_o < N // 2:                                                          # GridMapApp.java:185-186, by the existing calls
                r01 = float(rng.random())
                idx, amb = dev.resample(r01, want_indices=True)
                want, clamped = o.resample(r01)
                assert clamped == 0
                assert_resample_indices(idx, want, amb)
                assert np.array_equal(idx, want), f"{where}: the draw {r01} sits on a rounding boundary; pick another seed"
                resampled += 1
                assert np.array_equal(dev.get_particles()[0], o.poses)
                if resampled == 1:
                    _compare_maps(dev, o, f"{where} after the resampling copy")
        assert resampled >= 1 and dev.maps_copied() == resampled * N
    finally:
        dev.close()


# ---- the batch frame -----------------------------------------------------------------------------------------------------------
BAT_S, BAT_N, BAT_T, BAT_EXT = 4, 500, 12, 6.0
BAT_SEEDS = np.array([11, 12345, 7, 2 ** 40 + 3], dtype=np.uint64)
BAT_SKIP_FILTER, BAT_SKIP_FRAMES = 2, (3, 7)


def _batch_case(S=BAT_S, T=BAT_T):
    """S synthetic recordings of 90 measurements per revolution (synth.make_recording: raw polar measurements with the motion inside
    a revolution left in), cut to ragged lengths that differ frame to frame; odometry, seeds and draws distinct per filter; filter
    BAT_SKIP_FILTER turns 40 degrees on BAT_SKIP_FRAMES (skipUpdate).  Returns (frames [T][S], lengths [T][S], r01 [T][S], starts [S][3])."""
    recs = [synth.make_recording(BAT_EXT, 90, T=48, seed=77 + 13 * f, n_frames=T)[0] for f in range(S)]
    starts = np.stack([synth.true_pose(synth.make_world(BAT_EXT, 77 + 13 * f), -1, 48) for f in range(S)])
    rng = np.random.default_rng(21)
    lengths = rng.integers(17, 91, size=(T, S)).astype(np.int32)
    lengths[0] = [90, 61, 90, 17][:S]
    lengths[:, 0] = 90                                                                   # (one filter always takes the whole revolution)
    jitter = np.stack([rng.uniform(0.0, 0.004, (T, S)), rng.uniform(-0.01, 0.01, (T, S))], axis=-1)
    frames = []
    for k in range(T):
        row = []
        for f in range(S):
            r, n = recs[f][k], int(lengths[k, f])
            dt = math.radians(40.0) if f == BAT_SKIP_FILTER and k in BAT_SKIP_FRAMES else r.d_theta + jitter[k, f, 1]
            row.append(Frame(r.time_stamp, r.d_center + jitter[k, f, 0], dt, r.angle[:n].copy(), r.distance[:n].copy(), r.hit[:n].copy()))
        frames.append(row)
    return frames, lengths, rng.random((T, S)), starts


# The oracle alone over _batch_case() (500 particles per filter, BAT_SEEDS, the rule applied at fraction 0.5), Neff / n per frame
# (lengths in brackets):
#    0 [90 61 90 17]  0.0051 0.0091 0.0037 1.0000      6 [90 90 79 32]  0.0338 0.0245 0.0743 0.1086
#    1 [90 69 42 23]  0.0531 0.0703 0.1047 0.3773      7 [90 80 44 68]  0.0801 0.0212 0.0020 0.0315
#    2 [90 63 62 89]  0.0562 0.0458 0.0670 0.0025      8 [90 33 36 30]  0.0309 0.0981 0.0610 0.1256
#    3 [90 48 87 25]  0.0396 0.0612 0.0122 0.0927      9 [90 87 45 42]  0.0356 0.0213 0.1039 0.0947
#    4 [90 87 84 67]  0.0480 0.0197 0.0033 0.0738     10 [90 49 21 65]  0.0397 0.0936 0.1453 0.0529
#    5 [90 31 72 66]  0.0238 0.0569 0.0937 0.0743     11 [90 49 86 17]  0.0328 0.0737 0.0217 0.1542
# Filter 0 never leaves 0.005 .. 0.080 and filters 1 and 2 stay below 0.15: no fraction has, for EVERY filter, frames on both sides
# that are 5 % of n away.  Hence the two-run form here as well: at 0.5 every value is 12 % of n away or more -- filters 0 to 2 draw
# on every frame, filter 3 on every frame but the first (17 beams over a blank map weigh its particles alike: Neff = n); at 0.0 the
# rule is evaluated and no filter ever draws (Neff >= 1 > 0, see _REC_FRACTIONS); fraction < 0 skips the step.
_BATCH_FRACTIONS = {"mostly": 0.5, "never": 0.0, "skipped": -1.0}


def _block(frames_k, lengths_k):
    S, L = len(frames_k), int(lengths_k.max())
    a, d, h = np.zeros((S, L)), np.zeros((S, L)), np.zeros((S, L), dtype=np.uint8)
    for f, fr in enumerate(frames_k):
        a[f, :lengths_k[f]], d[f, :lengths_k[f]], h[f, :lengths_k[f]] = fr.angle, fr.distance, fr.hit
    return a, d, h


def _batch_handles(S, n=BAT_N, max_beams=128):
    bat = SLAMParticleMapsBatch(S, BAT_EXT, BAT_EXT, 0.05, (-BAT_EXT / 2, -BAT_EXT / 2), num_particles=n, max_beams=max_beams)
    alone = [SLAMParticleMaps(BAT_EXT, BAT_EXT, 0.05, (-BAT_EXT / 2, -BAT_EXT / 2), num_particles=n, max_beams=max_beams) for _ in range(S)]
    return bat, alone


def _same_as_alone(bat, alone, where, drew=None, maps=True):
    S = bat.num_filters
    P, W = bat.get_particles()
    idx = bat.last_resample_indices()
    for f in range(S):
        p, w = alone[f].get_particles()
        assert np.array_equal(P[f], p), f"{where}: filter {f}: poses"
        assert np.array_equal(W[f], w), f"{where}: filter {f}: weights"
        if drew is not None and drew[f]:
            assert np.array_equal(idx[f], alone[f].pf.last_resample_indices()), f"{where}: filter {f}: resampling indices"
    if maps:
        for lik in (False, True):
            M = bat.maps(likelihood=lik)
            for f in range(S):
                assert np.array_equal(M[f], alone[f].maps(likelihood=lik)), f"{where}: filter {f}: {'likelihoodData' if lik else 'logData'}"
    assert bat.maps_copied() == sum(a.maps_copied() for a in alone), f"{where}: maps copied"


def _batch_against_alone(fraction, T, label):
    """returns did_resample [T][S]"""
    frames, lengths, r01, starts = _batch_case()
    S = BAT_S
    bat, alone = _batch_handles(S)
    try:
        bat.set_poses(np.ascontiguousarray(np.broadcast_to(starts[:, None, :], (S, BAT_N, 3)), dtype=np.float32))
        for f in range(S):
            alone[f].set_poses(np.tile(starts[f].astype(np.float32), (BAT_N, 1)))
        did = np.zeros((T, S), dtype=bool)
        copied = np.zeros(S, dtype=np.int64)
        for k in range(T):
            a, d, h = _block(frames[k], lengths[k])
            odo = np.array([(fr.d_center, fr.d_theta) for fr in frames[k]])
            neff = bat.frame(a, d, h, odo, seeds=BAT_SEEDS, sequence=k, r01=r01[k], fraction=fraction, lengths=lengths[k], fetch=True)
            for f, fr in enumerate(frames[k]):
                ne = alone[f].frame(fr.angle, fr.distance, fr.hit, fr.d_center, fr.d_theta, seed=int(BAT_SEEDS[f]), sequence=k,
                                    r01=float(r01[k, f]), fraction=fraction, fetch=True)
                assert ne == neff[f], f"{label} frame {k}: filter {f}: Neff {neff[f]} != {ne}"
            now = np.array([x.maps_copied() for x in alone], dtype=np.int64)
            did[k] = now != copied
            copied = now
            if fraction >= 0:
                assert np.array_equal(bat.did_resample(), did[k]), f"{label} frame {k}: did_resample"
            print(f"{label} frame {k}: Neff / n", np.round(neff / BAT_N, 4), "drew", did[k].astype(int))
            _same_as_alone(bat, alone, f"{label} frame {k}", drew=did[k], maps=(k in (0, 3, 4, T - 1)))
        return did
    finally:
        bat.close()
        for x in alone:
            x.close()


def test_batch_frame_equals_stand_alone_frames_and_every_filter_takes_both_branches():
    did = _batch_against_alone(_BATCH_FRACTIONS["mostly"], BAT_T, "fraction 0.5")
    assert did[:, :3].all() and did[1:, 3].all() and not did[0, 3], "the draws the oracle's Neff sequence predicts"
    never = _batch_against_alone(_BATCH_FRACTIONS["never"], 6, "fraction 0.0")
    assert not never.any(), "no Neff is below 0: the rule is evaluated and no filter draws"
    for f in range(BAT_S):
        assert did[:, f].any() and not never[:, f].all()
    skipped = _batch_against_alone(_BATCH_FRACTIONS["skipped"], 4, "fraction < 0")
    assert not skipped.any(), "fraction < 0 skips the resampling step: nothing is copied"


def test_one_filter_batch_frame_equals_the_scalar_frame():
    frames, lengths, r01, starts = _batch_case()
    bat, (one,) = _batch_handles(1, n=64)
    try:
        for k in range(6):
            fr = frames[k][1]
            a, d, h = _block([fr], lengths[k, 1:2])
            ne = bat.frame(a, d, h, [(fr.d_center, fr.d_theta)], seeds=77, sequence=k, r01=[r01[k, 1]], fraction=0.9, fetch=True)
            n1 = one.frame(fr.angle, fr.distance, fr.hit, fr.d_center, fr.d_theta, seed=77, sequence=k, r01=float(r01[k, 1]), fraction=0.9, fetch=True)
            assert ne[0] == n1
            assert np.array_equal(bat.last_beams(0), one.last_beams())
        _same_as_alone(bat, [one], "S = 1")
    finally:
        bat.close(); one.close()


def test_batch_deskew_rows_use_each_filters_own_length_and_odometry():
    """the beams the batch de-skew produced for every filter against GridMap.deskew on that filter's own (length, odometry): a de-skew
    that divided by L instead of lengths[f] (GridMapApp.java:150), or read another filter's odometry, differs in every beam"""
    frames, lengths, r01, _ = _batch_case(S=3)
    bat, alone = _batch_handles(3, n=32)
    m = GridMap(BAT_EXT, BAT_EXT, 0.05, (-BAT_EXT / 2, -BAT_EXT / 2), max_beams=128)
    try:
        for k in (0, 1, 3):
            a, d, h = _block(frames[k], lengths[k])
            odo = np.array([(fr.d_center, fr.d_theta) for fr in frames[k]])
            bat.frame(a, d, h, odo, seeds=BAT_SEEDS[:3], sequence=k, r01=r01[k, :3], fraction=-1.0, lengths=lengths[k])
            assert bat.maps_copied() == 0
            for f, fr in enumerate(frames[k]):
                want = m.deskew(fr.angle, fr.distance, fr.hit, fr.d_center, fr.d_theta).beams
                got = bat.last_beams(f)
                assert len(got) == lengths[k, f] == len(want)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"frame {k}: filter {f}: de-skewed beams"
            # all L through lengths = None: every row de-skewed with L
            if k == 0:
                full = [Frame(0.0, fr.d_center, fr.d_theta, a[f].copy(), d[f].copy(), h[f].copy()) for f, fr in enumerate(frames[k])]
                bat.frame(a, d, h, odo, seeds=BAT_SEEDS[:3], sequence=100, r01=r01[k, :3], fraction=-1.0)
                for f, fr in enumerate(full):
                    want = m.deskew(fr.angle, fr.distance, fr.hit, fr.d_center, fr.d_theta).beams
                    assert np.array_equal(bat.last_beams(f).view(np.uint8), want.view(np.uint8))
    finally:
        bat.close(); m.close()
        for x in alone:
            x.close()


def test_frame_calls_refuse_what_they_cannot_do():
    L = load()
    a, d, h = np.zeros((2, 8)), np.ones((2, 8)), np.ones((2, 8), np.uint8)
    odo, seeds, r01 = np.zeros((2, 2)), np.zeros(2, np.uint64), np.full(2, 0.5)
    p = lambda x: x.ctypes.data

    def scalar(handle, length, arrays=(a, d, h)):
        return L.gms_slam_frame_per_particle(handle, p(arrays[0]), p(arrays[1]), p(arrays[2]), length, 0.01, 0.0, 1, 0, 0.5, 0.5, None)

    def batch(handle, Lb, lengths=None):
        return L.gms_slam_frame_batch(handle, p(a), p(d), p(h), Lb, None if lengths is None else p(lengths), p(odo), p(seeds), 0, p(r01), 0.5, None)

    one = SLAMParticleMaps(3.2, 3.2, 0.05, (-1.6, -1.6), num_particles=16, max_beams=64)
    bat = SLAMParticleMapsBatch(2, 3.2, 3.2, 0.05, (-1.6, -1.6), num_particles=16, max_beams=64)
    shard = SLAMParticleMaps.__new__(SLAMParticleMaps)
    shard._init_shard(3.2, 3.2, 0.05, (-1.6, -1.6), 256, 0, 512, max_beams=64)
    try:
        # NULL handle / arrays (also without a GPU: tests/test_slam_frame_args.py)
        assert scalar(None, 8) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        assert L.gms_slam_frame_per_particle(one._h, None, p(d), p(h), 8, 0.01, 0.0, 1, 0, 0.5, 0.5, None) == GMS_ERR_INVALID
        assert b"null" in L.gms_last_error()
        assert batch(None, 8) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        assert L.gms_slam_frame_batch(bat._h, p(a), p(d), p(h), 8, None, None, p(seeds), 0, p(r01), 0.5, None) == GMS_ERR_INVALID
        assert b"null" in L.gms_last_error()
        # lengths
        for length in (0, -3, 65):
            assert scalar(one._h, length) == GMS_ERR_INVALID and b"length" in L.gms_last_error()
        for Lb in (0, 65):
            assert batch(bat._h, Lb) == GMS_ERR_INVALID and b"max_beams" in L.gms_last_error()
        for lengths in ([0, 4], [9, 1], [3, -1]):
            assert batch(bat._h, 8, np.array(lengths, np.int32)) == GMS_ERR_INVALID and b"lengths[" in L.gms_last_error()
        # the scalar form on a batched handle; either form on a shard
        assert scalar(bat._h, 8) == GMS_ERR_STATE and b"filters" in L.gms_last_error()
        assert scalar(shard._h, 8) == GMS_ERR_STATE and b"shard" in L.gms_last_error()
        assert batch(shard._h, 8) == GMS_ERR_STATE and b"shard" in L.gms_last_error()
        # nothing ran: no frame to read beams of
        out, c = np.zeros(64, dtype=[("b", "u1", (32,))]), C.c_int32(0)
        assert L.gms_slam_last_beams(one._h, 0, p(out), 64, C.byref(c)) == GMS_ERR_STATE
        assert L.gms_slam_last_beams(bat._h, 2, p(out), 64, C.byref(c)) == GMS_ERR_INVALID
        # ... and the Python layer raises
        with pytest.raises(GmsError):
            bat.frame(a, d, h, odo, lengths=[9, 1])
        with pytest.raises(ValueError):
            bat.frame(a[:1], d[:1], h[:1], odo)
    finally:
        one.close(); bat.close(); shard.close()


def test_replay_classes_follow_the_recording():
    """ParticleMapsReplay over the recording, one frame() call per revolution and nothing read back, ends within 0.25 m of the
    recorded drive's last pose -- what test_gpu_trace_replay.py demands of the shared-map filter.  The oracle's own loop at this
    size (96 particles, two bootstrap frames, seed 99, fraction 0.5) ends 0.094 m from it.  The batch replay steps two copies of the
    recording, one cut to 300 measurements per revolution, and must leave filter 0 exactly where the scalar replay is."""
    frames = _rec_frames()
    truth = np.load(os.path.join(HERE, "golden", "recording_360_poses.npy"))
    BOOT = 2
    dev = _rec_handle()
    try:
        rp = ParticleMapsReplay(dev, seed=REC_SEED, resample_fraction=0.5, start_pose=_rec_start())
        rng = np.random.default_rng(5)
        draws = rng.random(len(frames))
        for f in frames[:BOOT]:
            rp.bootstrap(f)
        for k, f in enumerate(frames[BOOT:]):
            rp.step(f, float(draws[k]))
        est = dev.get_weighted_pose()
        dist = float(np.hypot(*(est[:2] - truth[len(frames) - 1][:2])))
        print(f"ParticleMapsReplay: {dist:.3f} m from the drive's last pose")
        assert dist < 0.25
        assert dev.maps_copied() > 0
        P1, W1 = dev.get_particles()
    finally:
        dev.close()
    T2 = 12
    bat = SLAMParticleMapsBatch(2, REC_EXT, REC_EXT, REC_RES, (-REC_EXT / 2, -REC_EXT / 2), num_particles=REC_N, max_beams=512)
    one = _rec_handle()
    try:
        start = _rec_start()
        rb = ParticleMapsBatchReplay(bat, seeds=[REC_SEED, 5], resample_fraction=0.5, start_poses=[start, start])
        r1 = ParticleMapsReplay(one, seed=REC_SEED, resample_fraction=0.5, start_pose=start)
        for k, f in enumerate(frames[:T2]):
            cut = Frame(f.time_stamp, f.d_center, f.d_theta, f.angle[:300], f.distance[:300], f.hit[:300])
            rb.step([f, cut], [draws[k], 1.0 - draws[k]])
            r1.step(f, float(draws[k]))
        P, W = bat.get_particles()
        p, w = one.get_particles()
        assert np.array_equal(P[0], p) and np.array_equal(W[0], w)
        assert np.array_equal(bat.maps(0), one.maps())
    finally:
        bat.close(); one.close()
