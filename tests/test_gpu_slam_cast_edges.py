"""The per-particle update (k_slam_particle) and the pose refinement (k_slam_refine) where the reference's two casts decide --
`(int)(d / res)` in probabilityOf / findBestPose (GridMap.java:273-276: NaN is cell 0, +-Inf and +-1e30 saturate, (-1, 0) is cell
0), `(int) Math.floor(..)` in RayIterator (RayIterator.java:71-100: (-1, 0) is cell -1 and no walk starts) -- against the oracle's
literal loop.  The inputs and the oracle's expectations: tests/_slam_cast_cases.py; that every family does what its name says and
that the expectation depends on it: tests/test_slam_cast_inputs.py.  Both sides make three ordinary updates and then ONE with the
special poses and the special scan (or with the empty-box poses): poses equal (NaN where the oracle's is NaN), weights, strongest,
Neff and EVERY particle's map with the bars of tests/test_gpu_slam_particle_maps.py, the special particles' cell walks equal."""
import numpy as np
import pytest

from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch

import _slam_cast_cases as cc
from test_gpu_slam_particle_maps import _compare_maps, _compare_weights

pytestmark = pytest.mark.gpu

#        id: (map, refine, environment)
FORMS = {
    "plain": ("5cm", False, {}),
    "plain_2cm": ("2cm", False, {}),
    "plain_no_planes": ("5cm", False, {"GMS_SLAM_EAGER_LIK": "1"}),
    "refine_from_class_plane": ("5cm", True, {}),
    "refine_staged": ("5cm", True, {"GMS_SLAM_REFINE_LDS": "2"}),
    "refine_memory_forced": ("5cm", True, {"GMS_SLAM_REFINE_LDS": "0"}),
    "refine_field_codes": ("5cm", True, {"GMS_SLAM_REFINE_FIELD": "codes"}),
    "refine_2cm_11_taps": ("2cm", True, {}),
    "refine_no_planes": ("5cm", True, {"GMS_SLAM_EAGER_LIK": "1"}),
}


def _handle(name, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = cc.scene(name)
    dev = SLAMParticleMaps(sc.size[0], sc.size[1], sc.res, sc.origin, num_particles=cc.N, max_beams=128)
    assert (dev.W, dev.H) == (sc.g.W, sc.g.H)
    return dev


def _warm(dev, name):
    sc = cc.scene(name)
    for P, z in zip(sc.warm_poses(), sc.warm_scans()):
        dev.set_poses(P)
        dev.update(z, None)
    logs = dev.maps().reshape(cc.N, -1)
    for i, want in enumerate(cc.warm_logs(name)):
        assert np.array_equal(logs[i] != 0, want != 0) and (np.abs(logs[i] - want) <= 1e-13 * np.maximum(np.abs(want), 1.0)).all(), f"warm-up: particle {i}"


def _compare(dev, neff, e, where):
    P, w = dev.get_particles()
    nan = np.isnan(e.poses).any(axis=1)
    assert np.array_equal(P[nan], e.poses[nan], equal_nan=True), f"{where}: poses of the particles whose oracle pose is NaN"
    bad = np.flatnonzero((P[~nan] != e.poses[~nan]).any(axis=1))
    assert bad.size == 0, f"{where}: poses differ at {np.flatnonzero(~nan)[bad]}: {P[~nan][bad[:3]]} against {e.poses[~nan][bad[:3]]}"
    _compare_weights(w, e.weights, where)
    assert dev.last_stats["strongest"] == e.strongest, where
    assert abs(neff - e.neff) <= 1e-11 * e.neff, where
    _compare_maps(dev, e, where)


@pytest.mark.parametrize("form", list(FORMS))
def test_special_poses_and_beams_against_the_oracle(form, monkeypatch):
    name, refine, env = FORMS[form]
    dev = _handle(name, env, monkeypatch)
    _warm(dev, name)
    P, z = cc.special_poses(name), cc.special_scan(name)
    dev.set_poses(P)
    if not refine:
        # the walks, at the poses as they are set: counts, cells and classes of every special particle's rays (and of the axis beams' one)
        for i in cc.SLOTS + (0,):
            cells, cls, counts = dev.trace_scan(i, z)
            for b, (oc, ok) in enumerate(cc.walks(name, i)):
                assert counts[b] == len(oc), (form, i, b)
                assert np.array_equal(cells[b, :counts[b]], oc) and np.array_equal(cls[b, :counts[b]], ok), (form, i, b)
    dev.set_refine(refine)
    neff = dev.update(z, None)
    _compare(dev, neff, cc.expect(name, "special", refine), form)
    dev.close()


@pytest.mark.parametrize("name, refine", [("5cm", False), ("5cm", True), ("2cm", False)])
def test_a_scan_of_which_no_ray_starts(name, refine, monkeypatch):
    """every particle's start cell lies outside the map: the scan's box stays empty (k_slam_particle leaves before the count tile),
    every map comes back bit-identical, nothing is copied -- and the end points still score"""
    dev = _handle(name, {}, monkeypatch)
    _warm(dev, name)
    logs, copied = dev.maps().copy(), dev.maps_copied()
    dev.set_poses(cc.empty_box_poses(name))
    dev.set_refine(refine)
    neff = dev.update(cc.special_scan(name), None)
    e = cc.expect(name, "empty_box", refine)
    _compare(dev, neff, e, f"empty box {name} refine={refine}")
    assert np.array_equal(dev.maps(), logs), "a map changed though no ray started"
    assert dev.maps_copied() == copied
    # likelihoodData is the field of the logData the update started from (SLAM.java:93): of the warm-up's last state, on both sides
    assert np.array_equal(dev.maps(likelihood=True).reshape(cc.N, -1), np.stack(cc.warm_fields(name)))
    dev.close()


def test_batched_filter_zero_special_filter_one_ordinary(monkeypatch):
    """two filters in one handle: filter 0 carries the special poses and must equal the oracle, filter 1 is ordinary and must equal a
    stand-alone handle bit for bit"""
    name, refine = "5cm", True
    sc = cc.scene(name)
    bat = SLAMParticleMapsBatch(2, sc.size[0], sc.size[1], sc.res, sc.origin, num_particles=cc.N, max_beams=128)
    one = _handle(name, {}, monkeypatch)
    for P, z in zip(sc.warm_poses(), sc.warm_scans()):
        bat.set_poses(np.stack([P, P]))
        bat.update([z, z])
        one.set_poses(P)
        one.update(z, None)
    z = cc.special_scan(name)
    P1 = sc.particles(cc.WARM)
    bat.set_poses(np.stack([cc.special_poses(name), P1]))
    one.set_poses(P1)
    bat.set_refine(refine); one.set_refine(refine)
    neff = bat.update([z, z])
    neff1 = one.update(z, None)
    e = cc.expect(name, "special", refine)
    P, w = bat.get_particles()
    assert np.array_equal(P[0], e.poses, equal_nan=True)
    fin = ~np.isnan(e.poses).any(axis=1)
    assert np.array_equal(P[0][fin], e.poses[fin])
    _compare_weights(w[0], e.weights, "batched filter 0")
    assert bat.last_stats[0]["strongest"] == e.strongest and abs(neff[0] - e.neff) <= 1e-11 * e.neff
    logs, liks = bat.maps(0).reshape(cc.N, -1), bat.maps(0, likelihood=True).reshape(cc.N, -1)
    for i in range(cc.N):
        lo = e.log(i)
        assert np.array_equal(logs[i] != 0, lo != 0), f"filter 0 particle {i}: another set of cells touched"
        assert (np.abs(logs[i] - lo) <= 1e-13 * np.maximum(np.abs(lo), 1.0)).all(), f"filter 0 particle {i}"
        assert np.array_equal(liks[i], e.lik(i)), f"filter 0 particle {i}: likelihood field"
    Pa, wa = one.get_particles()
    assert np.array_equal(P[1], Pa) and np.array_equal(w[1], wa) and neff[1] == neff1 and (P[1] != P1).any()
    assert bat.last_stats[1] == one.last_stats
    assert np.array_equal(bat.maps(1), one.maps()) and np.array_equal(bat.maps(1, likelihood=True), one.maps(likelihood=True))
    bat.close(); one.close()
