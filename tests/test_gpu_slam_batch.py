"""Several reference-shape filters in one gms_slam handle (gms_params.n_maps = S, SLAMParticleMapsBatch): filter f of the batched
handle must give, bit for bit, what a stand-alone SLAMParticleMaps gives with the same params, scans, odometry and seed seeds[f] --
poses, weights, statistics, resampling indices, both arrays of every particle's map and the combined map.  The stand-alone handles
are themselves pinned to the oracle by test_gpu_slam_particle_maps.py."""
import ctypes as C
import math

import numpy as np
import pytest

from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_INVALID, GMS_ERR_STATE, GmsError, GmsParams, check, load

pytestmark = pytest.mark.gpu

STATS = ("weight_sum", "neff", "strongest", "n_zero", "max_log_weight")


def _scans(ext, res, counts, T, seed0):
    """T frames of differently seeded synthetic traces, filter f's scans of counts[f] beams (0: an empty scan)"""
    out = []
    for f, B in enumerate(counts):
        if B == 0:
            out.append([np.zeros(0, dtype=BEAM_DTYPE)] * T)
        else:
            out.append(list(synth.make_trace(ext, res, B, T=T, seed=seed0 + 17 * f).scans[:T]))
    return out


def _odometry(S, T, seed, skip_filter=1, skip_frames=(2, 5)):
    """per frame and filter (dCenter, dTheta), filter skip_filter turning more than 30 degrees on skip_frames (SLAM.java:82)"""
    rng = np.random.default_rng(seed)
    u = np.stack([rng.uniform(0.0, 0.06, (T, S)), rng.uniform(-0.08, 0.08, (T, S))], axis=-1)
    for k in skip_frames:
        if k < T:
            u[k, skip_filter, 1] = math.radians(40.0)
    return u


def _compare(bat, alone, where, maps=True, indices=True):
    """indices: a resampling step has run on both sides (before the first one the index arrays hold nothing)"""
    S, n = bat.num_filters, bat.num_particles
    P, W = bat.get_particles()
    idx = bat.last_resample_indices()
    for f in range(S):
        p, w = alone[f].get_particles()
        assert np.array_equal(P[f], p), f"{where}: filter {f}: poses"
        assert np.array_equal(W[f], w), f"{where}: filter {f}: weights"
        if indices:
            assert np.array_equal(idx[f], alone[f].pf.last_resample_indices()), f"{where}: filter {f}: resampling indices"
    if hasattr(bat, "last_stats"):
        for f in range(S):
            for k in STATS:
                a, b = bat.last_stats[f][k], alone[f].last_stats[k]
                assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), f"{where}: filter {f}: {k} {a} != {b}"
    if maps:
        for lik in (False, True):
            M = bat.maps(likelihood=lik)
            for f in range(S):
                assert np.array_equal(M[f], alone[f].maps(likelihood=lik)), f"{where}: filter {f}: {'likelihoodData' if lik else 'logData'}"
    assert np.array_equal(bat.get_weighted_pose(), np.stack([a.get_weighted_pose() for a in alone]))


def _sequence(ext, res, n, counts, T, refine=False, label=""):
    """the issue's sequence: per-frame update of S filters with distinct scans, seeds and odometry, then resample_if with a fraction
    that splits the filters on odd frames; every frame compared; last an unconditional resample with per-filter draws"""
    S = len(counts)
    scans = _scans(ext, res, counts, T, seed0=300)
    u = _odometry(S, T, seed=5)
    seeds = np.array([11, 12345, 7, 2 ** 40 + 3], dtype=np.uint64)[:S]
    rng = np.random.default_rng(9)
    bat = SLAMParticleMapsBatch(S, ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=max(counts) + 8)
    alone = [SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=max(counts) + 8) for _ in range(S)]
    try:
        if refine:
            bat.set_refine(True)
            for a in alone:
                a.set_refine(True)
        P0 = synth.make_particles(np.zeros(3), n * S, seed=3, sigma_xy=0.02, sigma_theta_deg=1.0).reshape(S, n, 3)
        bat.set_poses(P0)
        for f in range(S):
            alone[f].set_poses(P0[f])
        mixed = 0
        for k in range(T):
            zs = [scans[f][k] for f in range(S)]
            neff = bat.update(zs, [tuple(u[k, f]) for f in range(S)], seeds=seeds, sequence=k)
            for f in range(S):
                alone[f].update(zs[f], tuple(u[k, f]), seed=int(seeds[f]), sequence=k)
            _compare(bat, alone, f"{label} frame {k} update", maps=False, indices=k > 0)      # (the maps: once per frame, below)
            ratio = np.sort(neff / n)
            frac = 0.5 if k % 2 == 0 or ratio[0] == ratio[-1] else float(ratio[0] + ratio[-1]) / 2
            r01 = rng.random(S)
            bat.resample_if(r01, frac)
            for f in range(S):
                alone[f].resample_if(float(r01[f]), frac)
            did = bat.did_resample()
            assert np.array_equal(did, [a.pf.did_resample() for a in alone])
            mixed += int(did.any() and not did.all())
            _compare(bat, alone, f"{label} frame {k} resample_if")
        assert mixed >= 1, f"{label}: no frame on which some filters resampled and others did not"
        r01 = rng.random(S)
        idx, amb = bat.resample(r01, want_indices=True)
        for f in range(S):
            i1, a1 = alone[f].resample(float(r01[f]), want_indices=True)
            assert np.array_equal(idx[f], i1) and amb[f] == a1
        _compare(bat, alone, f"{label} resample")
        for f in range(S):                                                                # calculateCombined of every filter
            assert np.array_equal(bat.calculate_combined(f), alone[f].calculate_combined())
            assert np.array_equal(bat.calculate_combined(f, likelihood=True), alone[f].grid_map.download_likelihood().reshape(bat.H, bat.W))
        assert bat.maps_copied() == sum(a.maps_copied() for a in alone)
    finally:
        bat.close()
        for a in alone:
            a.close()


def test_four_filters_at_the_reference_operating_point():
    _sequence(6.0, 0.05, 500, [90, 180, 45, 0], T=12, label="500 x 120^2")


@pytest.mark.parametrize("form", ["refine", "refine_lds0", "refine_lds2", "eager", "no_lazy_copy"])
def test_four_filters_other_forms(form, monkeypatch):
    env = {"refine_lds0": ("GMS_SLAM_REFINE_LDS", "0"), "refine_lds2": ("GMS_SLAM_REFINE_LDS", "2"),
           "eager": ("GMS_SLAM_EAGER_LIK", "1"), "no_lazy_copy": ("GMS_SLAM_LAZY_LIK_COPY", "0")}.get(form)
    if env:
        monkeypatch.setenv(*env)
    _sequence(6.0, 0.05, 500, [90, 180, 45, 0], T=8, refine=form.startswith("refine"), label=form)


def test_refinement_with_the_field_in_memory():
    """256^2: the refinement's field does not fit the LDS and is read from memory"""
    _sequence(12.8, 0.05, 24, [90, 60, 30], T=6, refine=True, label="256^2")


@pytest.mark.parametrize("seed", [1, 2])
def test_random_call_sequences_against_stand_alone_handles(seed):
    """calls drawn at random -- update (with and without motion, sometimes a turn over 30 degrees), resample, resample_if, download of
    one or all maps, upload of a log or field into a slot, reset, combined -- on a batched handle and on S stand-alone ones"""
    rng = np.random.default_rng(seed)
    ext, res, n, S = 3.2, 0.05, 24, 3
    scans = _scans(ext, res, [48, 30, 48], 8, seed0=60 + seed)
    bat = SLAMParticleMapsBatch(S, ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=64)
    alone = [SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=64) for _ in range(S)]
    seeds = np.array([seed, seed + 100, seed + 200], dtype=np.uint64)
    W = H = bat.W
    normalised = drawn = False
    try:
        for step in range(40):
            op = rng.choice(["update", "update", "update", "resample", "resample_if", "get_one", "get_all", "put_log", "put_lik", "reset",
                             "combined"])
            where = f"seed {seed} call {step} ({op})"
            if op == "update":
                t = int(rng.integers(0, 8))
                zs = [scans[f][t] for f in range(S)]
                us = [None if rng.random() < 0.3 else (0.01, float(np.radians(rng.choice([1.0, 40.0])))) for _ in range(S)]
                bat.update(zs, us, seeds=seeds, sequence=step)
                for f in range(S):
                    alone[f].update(zs[f], us[f], seed=int(seeds[f]), sequence=step)
                _compare(bat, alone, where, maps=False, indices=drawn)
                normalised = True
            elif op in ("resample", "resample_if") and normalised:
                r01 = rng.random(S)
                if op == "resample":
                    bat.resample(r01)
                    for f in range(S):
                        alone[f].resample(float(r01[f]))
                else:
                    frac = float(rng.choice([0.3, 0.6, 0.9]))
                    bat.resample_if(r01, frac)
                    for f in range(S):
                        alone[f].resample_if(float(r01[f]), frac)
                drawn = True
                _compare(bat, alone, where, maps=False)
            elif op == "get_one":
                f, i = int(rng.integers(0, S)), int(rng.integers(0, n))
                for lik in (False, True):
                    assert np.array_equal(bat.map_of(f, i, likelihood=lik), alone[f].map_of(i, likelihood=lik)), where
            elif op == "get_all":
                _compare(bat, alone, where, indices=drawn)
            elif op in ("put_log", "put_lik"):
                f, i = int(rng.integers(0, S)), int(rng.integers(0, n))
                a = rng.normal(0.0, 1.0, (H, W)) * (rng.random((H, W)) < 0.1)
                if op == "put_log":
                    bat.set_map(f, i, log=a); alone[f].set_map(i, log=a)
                else:
                    bat.set_map(f, i, lik=np.abs(a)); alone[f].set_map(i, lik=np.abs(a))
            elif op == "reset":
                bat.reset()
                for a in alone:
                    a.reset()
                normalised = False
            elif op == "combined":
                f = int(rng.integers(0, S))
                assert np.array_equal(bat.calculate_combined(f), alone[f].calculate_combined()), where
        _compare(bat, alone, f"seed {seed} end", indices=drawn)
    finally:
        bat.close()
        for a in alone:
            a.close()


def test_one_filter_batch_equals_the_scalar_calls():
    """S = 1: the batch entry points are the scalar ones, bit for bit"""
    ext, res, n = 6.0, 0.05, 64
    scans = _scans(ext, res, [90], 6, seed0=400)[0]
    u = _odometry(1, 6, seed=8, skip_filter=0, skip_frames=(3,))
    bat = SLAMParticleMapsBatch(1, ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    one = SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    try:
        for k in range(6):
            bat.update([scans[k]], [tuple(u[k, 0])], seeds=77, sequence=k)
            one.update(scans[k], tuple(u[k, 0]), seed=77, sequence=k)
            _compare(bat, [one], f"frame {k}", indices=k > 0)
            if k % 2:
                bat.resample_if([0.3], 0.9); one.resample_if(0.3, 0.9)
            else:
                idx, amb = bat.resample([0.6], want_indices=True)
                i1, a1 = one.resample(0.6, want_indices=True)
                assert np.array_equal(idx[0], i1) and amb[0] == a1
            _compare(bat, [one], f"frame {k} resampled")
        assert np.array_equal(bat.calculate_combined(0), one.calculate_combined())
    finally:
        bat.close(); one.close()


def _params(S, ext=3.2, res=0.05):
    L = load()
    p = GmsParams()
    check(L.gms_params_default(C.byref(p), ext, ext, res, -ext / 2, -ext / 2))
    p.n_maps = S
    p.max_beams = 64
    return p


def test_state_and_argument_errors():
    L = load()
    bat = SLAMParticleMapsBatch(2, 3.2, 3.2, 0.05, (-1.6, -1.6), num_particles=16, max_beams=64)
    try:
        z = np.zeros(4, dtype=BEAM_DTYPE)
        for call in (lambda: L.gms_slam_update_per_particle(bat._h, z.ctypes.data, 4, 0, 0.0, 0.0, 0, 0, None),
                     lambda: L.gms_slam_update_per_particle_dev(bat._h, z.ctypes.data, 4, 0, 0.0, 0.0, 0, 0, None),
                     lambda: L.gms_slam_resample_maps(bat._h, 0.5, None, None),
                     lambda: L.gms_slam_resample_maps_if(bat._h, 0.5, 0.5),
                     lambda: L.gms_slam_update_local(bat._h, z.ctypes.data, 4, 0, 0.0, 0.0, 0, 0),
                     lambda: L.gms_slam_shard_draw(bat._h, 0.5, -1.0, C.byref(C.c_int32()), np.zeros(32, np.int32).ctypes.data)):
            assert call() == GMS_ERR_STATE
            assert b"batch" in L.gms_last_error() or b"filters" in L.gms_last_error()
        # counts[f] > B, negative counts
        odo = np.zeros((2, 2)); seeds = np.zeros(2, np.uint64); sm = np.ones(2, np.int32)
        blk = np.zeros((2, 8), dtype=z.dtype)
        for counts in ([9, 1], [-1, 2]):
            c = np.array(counts, np.int32)
            rc = L.gms_slam_update_batch(bat._h, blk.ctypes.data, 8, c.ctypes.data, odo.ctypes.data, seeds.ctypes.data, sm.ctypes.data, 0, None)
            assert rc == GMS_ERR_INVALID and b"counts[" in L.gms_last_error()
        rc = L.gms_slam_update_batch(bat._h, blk.ctypes.data, 8, None, None, seeds.ctypes.data, sm.ctypes.data, 0, None)
        assert rc == GMS_ERR_INVALID
    finally:
        bat.close()
    # a sharded create with n_maps > 1; S * n over the handle's limit
    h = C.c_void_p()
    assert L.gms_slam_create_shard(C.byref(_params(2)), 256, 0, 512, C.byref(h)) == GMS_ERR_INVALID and b"n_maps" in L.gms_last_error()
    assert L.gms_slam_create(C.byref(_params(2)), 40000, C.byref(h)) == GMS_ERR_INVALID and b"65535" in L.gms_last_error()
    assert L.gms_slam_create(C.byref(_params(1025)), 8, C.byref(h)) == GMS_ERR_INVALID
    with pytest.raises(GmsError):
        SLAMParticleMapsBatch(1100, 3.2, 3.2, 0.05, (-1.6, -1.6), num_particles=8)
