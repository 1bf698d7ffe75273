"""The per-particle filter WITHOUT its class planes (gms_slam_create: a blur kernel wider than fifteen taps, a plane over 24 KiB --
more than 314 x 313 cells --, or GMS_SLAM_EAGER_LIK=1): every update rebuilds every cell of every particle's likelihoodData
(k_slam_likelihood), k_slam_particle reads the field from memory (its CODES = false forms), and resample() copies likelihoodData as
an array.  Against the oracle's literal loop (orc_slam_update / orc_slam_resample) with the bars of
tests/test_gpu_slam_particle_maps.py: weights to 1e-13, poses, strongest and resampling indices equal, Neff to 1e-11, logData to
1e-13 on the same cells, likelihoodData equal.  Each side of a limit carries a witness: a one-rank shard (gms_slam_create_shard)
moves a particle as logData + its class planes, so it is created exactly where the planes are kept.  The last test runs all eight
instantiations of k_slam_particle (512 / 1024 lanes x 16-bit count tiles on offer or not x planes or not)."""
import os

import numpy as np
import pytest

from gridmap_slam_robot_amd import SLAMParticleMaps, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GmsError
from gridmap_slam_robot_amd.trace import read_trace
from oracle import oracle as orc

from _checks import assert_resample_indices
from test_gpu_slam_particle_maps import _compare_maps, _compare_weights, _frames_to_scans

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = min(16, os.cpu_count() or 1)
TAPS_15 = orc.gaussian_kernel(2.0, 7)           # the widest kernel the planes are kept for (khalf = 7)
TAPS_17 = orc.gaussian_kernel(2.0, 8)           # khalf = 8: no planes, and no compile-time blur (k_slam_likelihood<0>)


def _planes_kept(W, H, res, kernel=None, max_beams=0):
    """whether a handle of this map and kernel keeps the class planes: a one-rank shard of it can be created exactly then"""
    s = SLAMParticleMaps.__new__(SLAMParticleMaps)
    try:
        s._init_shard(W, H, res, (-W / 2, -H / 2), 1, 0, 1, 0, max_beams, kernel)
    except GmsError as e:
        assert e.code == GMS_ERR_INVALID, str(e)
        return False
    s.close()
    return True


def _resample_and_compare(dev, o, r01, where):
    idx, amb = dev.resample(r01, want_indices=True)
    want, clamped = o.resample(r01)
    assert clamped == 0
    assert_resample_indices(idx, want, amb)
    assert np.array_equal(idx, want), f"{where}: the draw {r01} sits on a rounding boundary; pick another"
    assert np.array_equal(dev.get_particles()[0], o.poses)
    _compare_weights(dev.get_particles()[1], o.weights, f"{where} after resampling")
    _compare_maps(dev, o, f"{where} after the resampling copy")


def _drive(dev, o, scans, start, seed, resample_at, check_maps_at, label, refine=False):
    """frames through both sides with the motion sample (drawn on the device; with refinement set by hand, as
    tests/test_gpu_slam_refine.py does), resample() with the given draw at the given frames"""
    n = o.n
    P0 = np.tile(np.asarray(start, np.float32), (n, 1))
    dev.set_poses(P0); o.set_poses(P0)
    dev.set_refine(refine)
    for k, (z, u) in enumerate(scans):
        where = f"{label} frame {k}"
        if refine:
            P_in = orc.sample_motion(o.poses, u[0], u[1], seed=seed, sequence=k)
            dev.set_poses(P_in); o.set_poses(P_in)
            neff = dev.update(z, u, sample_motion=False)
            neff_o = o.update(z, u, sample_motion=False, refine=True, threads=THREADS)
            P = dev.get_particles()[0]
            assert np.array_equal(P, o.poses), f"{where}: {int((P != o.poses).any(axis=1).sum())} of {n} refined poses differ"
            assert (P != P_in).any(), f"{where}: the search moved no pose"
        else:
            prev = o.poses
            neff = dev.update(z, u, seed=seed, sequence=k)
            P = dev.get_particles()[0]
            Po = orc.sample_motion(prev, u[0], u[1], seed=seed, sequence=k)
            assert (np.all(P == Po, axis=1)).mean() > 0.99 and np.max(np.abs(P - Po)) <= 2e-6, f"{where}: motion samples"
            o.set_poses(P)
            neff_o = o.update(z, u, sample_motion=False, threads=THREADS)
        _compare_weights(dev.get_particles()[1], o.weights, where)
        assert dev.last_stats["strongest"] == o.strongest and dev.last_stats["n_zero"] == int((o.weights == 0).sum()), where
        assert abs(neff - neff_o) <= 1e-11 * neff_o, where
        if k in check_maps_at:
            _compare_maps(dev, o, where)
        if k in resample_at:
            _resample_and_compare(dev, o, resample_at[k], where)


def _recording(extent, B, seed, n_frames, half_beams_except=()):
    """a synthetic drive of B beams per revolution; every frame but those listed keeps every other beam"""
    frames, _ = synth.make_recording(extent, B, T=48, seed=seed, n_frames=n_frames)
    for k, f in enumerate(frames):
        if k not in half_beams_except:
            f.angle, f.distance, f.hit = f.angle[::2].copy(), f.distance[::2].copy(), f.hit[::2].copy()
    return _frames_to_scans(frames), synth.true_pose(synth.make_world(extent, seed), -1, 48)


@pytest.mark.parametrize("W, H, kept", [(15.68, 15.62, True), (15.68, 15.68, False)], ids=["314x313_planes", "314x314_no_planes"])
def test_both_sides_of_the_plane_size_limit(W, H, kept):
    """a plane of 314 x 313 cells is exactly 24 576 bytes (kept), one of 314 x 314 is 24 656 (not kept).  Scans of 150 beams (16-bit
    count tiles on offer: the map does not fit a workgroup's LDS as 32-bit cells, so the launch is 1024 lanes) and one of 300 (32-bit
    only), resample() twice; the maps after each copy."""
    N = 32
    dev = SLAMParticleMaps(W, H, 0.05, (-W / 2, -H / 2), num_particles=N, max_beams=320)
    assert (dev.W, dev.H) == ((314, 313) if kept else (314, 314))
    assert _planes_kept(W, H, 0.05, max_beams=320) == kept
    g = orc.Grid(W, H, 0.05, -W / 2, -H / 2)
    o = orc.Slam(g, N)
    scans, start = _recording(12.0, 300, seed=83, n_frames=4, half_beams_except={2})
    assert len(scans[1][0]) == 150 and len(scans[2][0]) == 300
    _drive(dev, o, scans, start, seed=17, resample_at={1: 0.4137, 3: 0.6521}, check_maps_at={0, 2}, label=f"{dev.W}x{dev.H}")
    dev.close()


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refined"])
def test_seventeen_taps(refine):
    """a blur kernel of 17 taps (khalf = 8, one more than the on-demand evaluation takes): no planes, k_slam_likelihood's generic form
    writes every field; with refinement k_slam_refine stages that field in its LDS (no plane to compute it from).  The other side of
    the limit, fifteen taps, keeps its planes (tests/test_gpu_slam_particle_maps.py::test_other_geometries[fifteen_taps])."""
    ext, res, B, N, T = 4.0, 0.05, 90, 16, 5
    assert not _planes_kept(ext, ext, res, kernel=TAPS_17) and _planes_kept(ext, ext, res, kernel=TAPS_15)
    tr = synth.make_trace(ext, res, B, T=T, seed=31)
    g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
    g.set_kernel(TAPS_17)
    dev = SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=N, max_beams=128, kernel=TAPS_17)
    o = orc.Slam(g, N)
    dev.set_refine(refine)
    P = synth.make_particles(tr.poses[0], N, seed=4, sigma_xy=0.03, sigma_theta_deg=2.0)
    dev.set_poses(P); o.set_poses(P)
    for k in range(T):
        where = f"17 taps{' refined' if refine else ''} frame {k}"
        if refine:                                          # (a fresh cloud around each true pose: the search has work every frame)
            P = synth.make_particles(tr.poses[k], N, seed=4 + k, sigma_xy=0.05, sigma_theta_deg=3.0)
            dev.set_poses(P); o.set_poses(P)
        z = tr.scans[k]
        neff = dev.update(z, None)
        neff_o = o.update(z, None, refine=refine, threads=THREADS)
        Pd = dev.get_particles()[0]
        assert np.array_equal(Pd, o.poses), where
        if refine:
            assert (Pd != P).any(), where
        _compare_weights(dev.get_particles()[1], o.weights, where)
        assert dev.last_stats["strongest"] == o.strongest and abs(neff - neff_o) <= 1e-11 * neff_o, where
        _compare_maps(dev, o, where)
        if k == T - 2:
            _resample_and_compare(dev, o, 0.3719, where)
    dev.close()


@pytest.mark.parametrize("refine", [False, True], ids=["plain", "refined"])
def test_eager_likelihood_at_the_reference_operating_point(refine, monkeypatch):
    """GMS_SLAM_EAGER_LIK=1 (bench.py's like-for-like figure): 500 particles x 120 x 120 cells x 90 beams, ten revolutions of
    tests/golden/recording_360.bin (every fourth measurement), resample() at three of them; with refinement the search reads the
    field k_slam_likelihood has just written (k_slam_refine<true, 0>: staged in the LDS)."""
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")
    N, T = 500, 10
    assert not _planes_kept(6.0, 6.0, 0.05, max_beams=128)
    frames = read_trace(os.path.join(HERE, "golden", "recording_360.bin"))[:T]
    for f in frames:
        f.angle, f.distance, f.hit = f.angle[::4].copy(), f.distance[::4].copy(), f.hit[::4].copy()
    scans = _frames_to_scans(frames)
    assert len(scans[0][0]) == 90
    start = synth.true_pose(synth.make_world(25.6, 4321), -1, 64)
    dev = SLAMParticleMaps(6.0, 6.0, 0.05, (-3.0, -3.0), num_particles=N, max_beams=128)
    assert (dev.W, dev.H) == (120, 120)
    o = orc.Slam(orc.Grid(6.0, 6.0, 0.05, -3.0, -3.0), N)
    _drive(dev, o, scans, start, seed=2024, resample_at={2: 0.2893, 5: 0.5717, 8: 0.8311}, check_maps_at={0, T - 1},
           label=f"eager 500x120^2{' refined' if refine else ''}", refine=refine)
    assert dev.maps_copied() == 3 * N
    dev.close()


def test_refinement_whose_field_fits_no_lds():
    """refinement on 314 x 314 cells: no planes, and a field of 790 KB that no LDS holds -- k_slam_refine<false, 0> looks it up in
    memory, where k_slam_likelihood has written it"""
    W, N, B, T = 15.68, 32, 90, 2
    dev = SLAMParticleMaps(W, W, 0.05, (-W / 2, -W / 2), num_particles=N, max_beams=128)
    assert (dev.W, dev.H) == (314, 314)
    o = orc.Slam(orc.Grid(W, W, 0.05, -W / 2, -W / 2), N)
    scans, start = _recording(12.0, 2 * B, seed=84, n_frames=T)
    _drive(dev, o, scans, start, seed=29, resample_at={0: 0.4519}, check_maps_at={T - 1}, label="refined 314x314", refine=True)
    dev.close()


@pytest.mark.parametrize("eager", ["0", "1"], ids=["planes", "eager"])
@pytest.mark.parametrize("na", [False, True], ids=["32bit", "16bit_on_offer"])
@pytest.mark.parametrize("threads", ["512", "1024"])
def test_all_eight_particle_kernels(threads, na, eager, monkeypatch):
    """k_slam_particle<NT, 2, NA, CODES>: the workgroup forced to 512 or 1024 lanes (GMS_SLAM_THREADS); the count tile forced to
    3000 cells, so that 16-bit count cells are on offer to a scan of 128 beams (NA), or the whole map as the tile (not on offer);
    the class planes kept or dropped (GMS_SLAM_EAGER_LIK).  With NA, 10 zero-length beams (the 16-bit tile is taken) and 70 (a
    count can pass 255: the 32-bit fallback), as test_sixteen_bit_count_tiles_and_their_fallback does."""
    monkeypatch.setenv("GMS_SLAM_THREADS", threads)
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", eager)
    if na:
        monkeypatch.setenv("GMS_SLAM_TILE_CELLS", "3000")
    ext, res, B, N = 6.4, 0.05, 128, 16
    assert _planes_kept(ext, ext, res, max_beams=B) == (eager == "0")
    tr = synth.make_trace(ext, res, B, T=3, seed=41)
    g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
    for n_zero in ((10, 70) if na else (10,)):
        dev = SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=N, max_beams=B)
        o = orc.Slam(g, N)
        P = synth.make_particles(tr.poses[0], N, seed=6, sigma_xy=0.04, sigma_theta_deg=2.0)
        dev.set_poses(P); o.set_poses(P)
        for k in range(3):
            where = f"{threads} lanes, {n_zero} zero-length beams, scan {k}"
            z = tr.scans[k].copy()
            z["local_x"][:n_zero] = 0.0; z["local_y"][:n_zero] = 0.0; z["distance"][:n_zero] = 0.0; z["hit"][:n_zero] = 1
            neff = dev.update(z, None)
            neff_o = o.update(z, None, threads=THREADS)
            _compare_weights(dev.get_particles()[1], o.weights, where)
            assert dev.last_stats["strongest"] == o.strongest and abs(neff - neff_o) <= 1e-11 * neff_o, where
            _compare_maps(dev, o, where)
        dev.close()
