"""The opt-in to dynamic LDS (gms_kernel_lds, gms_internal.h) keeps a high-water mark per kernel instantiation and device and calls
the runtime only when a launch asks for more than the mark.  One instantiation launched with growing and shrinking dynamic LDS in one
process -- below the 48 KiB a launch may ask for unasked, over it, higher, below again, over again without a new opt-in -- must compute
what it always computed: a mark that skipped an opt-in it owed shows as a launch failure, one that lost its size as a wrong field."""
import numpy as np
import pytest

from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, _lib, synth
from oracle import oracle as orc

from test_gpu_slam_particle_maps import _compare_weights

pytestmark = pytest.mark.gpu

EXT, RES = 3.2, 0.05                          # 64 x 64 cells
# dynamic LDS of the generic likelihood kernel by taps (gms_likelihood_lds_bytes: a 32 x 64 tile, its halo, the row sums, the taps)
LDS_BYTES = {5: 38632, 25: 69192, 41: 98248}


def _taps(n):
    t = np.hanning(n + 2)[1:-1]
    return list(t / t.sum())


def _likelihood_step(taps, device=0):
    """a map with this blur kernel, one small scan integrated, computeLikelihoodMap: logData as the integration tests compare it,
    likelihoodData equal to the oracle's"""
    tr = synth.make_trace(EXT, RES, 24, T=2, seed=len(taps))
    g = orc.Grid(EXT, EXT, RES, -EXT / 2, -EXT / 2)
    g.set_kernel(taps)
    m = GridMap(EXT, EXT, RES, (-EXT / 2, -EXT / 2), device=device, kernel=taps)
    assert (m.W, m.H) == (g.W, g.H) == (64, 64)
    log = g.new_log()
    g.integrate(log, tr.scans[0], tr.poses[0])
    m.integrate_observation(tr.scans[0], tr.poses[0])
    m.compute_likelihood_map()
    got = m.download_log().reshape(-1)
    assert (log != 0).any() and np.array_equal(got != 0, log != 0)
    assert np.max(np.abs(got[log != 0] - log[log != 0]) / np.abs(log[log != 0])) <= 1e-13
    assert np.array_equal(m.download_likelihood().reshape(-1), g.build_likelihood(log)), f"{len(taps)} taps"
    m.close()


def test_the_generic_likelihood_kernel_below_over_higher_below_and_over_again():
    """k_likelihood<0, false, 1> (no kernel here has the 7 or 11 taps of the compile-time forms) at 38 632, 69 192, 98 248, 38 632 and
    69 192 bytes of dynamic LDS, in that order"""
    for n in (5, 25, 41, 5, 25):
        k = n // 2
        assert ((32 + 2 * k) * (64 + 2 * k + 1) + (32 + 2 * k) * 65 + n) * 8 == LDS_BYTES[n]      # (the sequence crosses 48 KiB where it says)
        _likelihood_step(_taps(n))


@pytest.mark.parametrize("threads", [None, "1024"])
def test_the_per_particle_update_on_small_large_and_small_maps(threads, monkeypatch):
    """k_slam_particle for filters of 4 particles on 32 x 32, 160 x 160 and 32 x 32 cells: the large map's count tile (100 KiB) takes
    the CU's LDS, one 1024-lane workgroup per CU.  By default the small maps run the 512-lane instantiation, which never opts in;
    threads = 1024 (GMS_SLAM_THREADS) makes all three one instantiation, whose dynamic LDS grows past the mark and shrinks again.  One
    update of a 16-beam scan each: poses, weights and one particle's map against the oracle's SLAM.update."""
    if threads:
        monkeypatch.setenv("GMS_SLAM_THREADS", threads)
    N, B = 4, 16
    for cells in (32, 160, 32):
        ext = cells * RES
        tr = synth.make_trace(ext, RES, B, T=2, seed=cells)
        g = orc.Grid(ext, ext, RES, -ext / 2, -ext / 2)
        dev = SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=N, max_beams=64)
        assert (dev.W, dev.H) == (g.W, g.H) == (cells, cells)
        o = orc.Slam(g, N)
        P = synth.make_particles(tr.poses[0], N, seed=3, sigma_xy=0.03, sigma_theta_deg=2.0)
        dev.set_poses(P); o.set_poses(P)
        neff = dev.update(tr.scans[0], None)
        neff_o = o.update(tr.scans[0], None)
        where = f"{cells} x {cells} cells"
        assert np.array_equal(dev.get_particles()[0], o.poses), where
        _compare_weights(dev.get_particles()[1], o.weights, where)
        assert abs(neff - neff_o) <= 1e-11 * neff_o
        i = 2                                                                  # one particle's map, as _compare_maps compares every particle's
        lg, lo = dev.map_of(i).reshape(-1), o.log(i)
        assert (lo != 0).any() and np.array_equal(lg != 0, lo != 0), f"{where}: another set of cells touched"
        assert (np.abs(lg - lo) <= 1e-13 * np.maximum(np.abs(lo), 1.0)).all(), where
        assert np.array_equal(dev.map_of(i, likelihood=True).reshape(-1), o.lik(i)), where
        dev.close()


def test_a_second_device_opts_in_on_its_own():
    """HIP keeps a function's attributes per device: a map on device 0 and one on device 1 in one process, the 41-tap step on both,
    device 0 first -- the mark device 0 raised must not stand for device 1"""
    n = int(_lib.load().gms_device_count())
    if n < 2:
        pytest.skip(f"{n} HIP device(s) visible: the per-device opt-in needs two")
    for device in (0, 1):
        _likelihood_step(_taps(41), device=device)
