"""Predicted scans on the device (include/gridmapslam.h "predicted scans"): gms_map_cast[_at], gms_slam_cast against records built
from the oracle's own ray set-up and cell walk (tests/_cast_expect.py).  Every comparison is array_equal on the whole record array:
no tolerance, no skipped beams.  A cast must see the map as a download would return it at that moment and must change no later
result of its handle: twins that never cast end bit-identical."""
import math
import os

import numpy as np
import pytest

import _cast_expect as ce
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_INVALID, GMS_ERR_STATE, GmsError
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RES = 0.05
EXTRA = 2                                              # gms_params_default's extra_steps (RayIterator additionalSteps)
TAPS_17 = orc.gaussian_kernel(2.0, 8)                  # khalf = 8: a per-particle handle that keeps no class planes


def _same(got, want, where=""):
    assert got.dtype == want.dtype and got.shape == want.shape, where
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), f"{where}: {len(bad)} of {want.size} records differ, first at {bad[:1].tolist()}: {got[tuple(bad[0])] if len(bad) else ''} != {want[tuple(bad[0])] if len(bad) else ''}"


def _same_nan(got, want):
    """array_equal where a range may be NaN (a NaN distance on a miss): NaN equals NaN, everything else exactly"""
    assert got.shape == want.shape
    for f in ("step", "x", "y"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["range"], want["range"], equal_nan=True)


# ---- 1: the shared map, random -----------------------------------------------------------------------------------------------
W1, H1 = 37, 23                                        # neither a multiple of 32: ragged words and rows of the bit plane


def random_case():
    """(oracle grid, logData [H][W], poses [3][3], probes [70]) -- about 6 % occupied cells, a NaN and a -0.0 cell"""
    g = orc.Grid(1.83, 1.13, RES, -0.915, -0.565)
    assert (g.W, g.H) == (W1, H1) and g.g.extra_steps == EXTRA
    rng = np.random.default_rng(20240611)
    u = rng.random((H1, W1))
    log = np.where(u < 0.06, g.l_occ, np.where(u < 0.60, g.l_free, 0.0))
    log[11, 18] = np.nan
    log[12, 19] = -0.0
    log[11, 17] = log[12, 17] = 0.0                    # the first pose starts in a cell that is not occupied,
    log[5, 29] = g.l_occ                               # the second in one that is: every probe of it hits at step 0
    poses = np.array([[-0.04, 0.01, 0.3], [0.55, -0.3, -2.0], [-1.5, 0.2, 0.0]], dtype=np.float32)      # the last one outside the map
    ang = np.concatenate([np.arange(8) * (math.pi / 4), rng.uniform(-math.pi, math.pi, 56)])             # exact axis and 45 degree directions
    dist = np.concatenate([np.full(8, 0.4), rng.uniform(0.05, 0.7, 40), rng.uniform(2.5, 4.0, 16)])      # ... the last 16 longer than the map
    x, y = dist * np.cos(ang), dist * np.sin(ang)
    x[:8] = np.array([0.4, 0.4, 0.0, -0.4, -0.4, -0.4, 0.0, 0.4])                                       # (exactly on the axes and diagonals)
    y[:8] = np.array([0.0, 0.4, 0.4, 0.4, 0.0, -0.4, -0.4, -0.4])
    x, y = np.concatenate([x, [0.0] * 6]), np.concatenate([y, [0.0] * 6])                               # one zero-length probe ...
    x[65:], y[65:] = [0.05, 0.1, -0.1, 0.15, -0.2], [0.02, -0.1, 0.1, 0.0, 0.05]                         # ... and five short ones: 70 in all
    probes = ce.probes_from(x, y)
    assert len(probes) == 70
    return g, log, poses, probes


def test_shared_map_random():
    g, log, poses, probes = random_case()
    want = ce.expect_poses(g, log, probes, poses)
    # what the oracle's expectation must contain for the comparison to mean something
    hit = want["step"] >= 0
    assert (want["step"] == 0).any(), "no hit at step 0"
    assert (~hit).any() and hit.mean() >= 0.2 and (~hit).mean() >= 0.2, (hit.mean(), "hits and misses: a fifth each")
    tail = clipped = False
    for pose, rec in zip(poses, want):
        for (ray, cells), r in zip(ce.walks(g, probes, pose), rec):
            planned = ce.planned_cells(ray, EXTRA)
            clipped |= 0 < len(cells) < planned                            # the walk entered the map and left it through the clip
            tail |= r["step"] >= planned - EXTRA                           # the hit lies in the extra_steps cells past the end point
    assert tail, "no hit inside the extra_steps tail"
    assert clipped, "no clipped ray"
    assert (want[2]["step"] == -1).all(), "a pose outside the map starts no walk (RayIterator.java:108)"
    m = GridMap(1.83, 1.13, RES, (-0.915, -0.565), max_beams=128)
    assert (m.W, m.H) == (W1, H1)
    m.upload_log(log)
    _same(m.cast(poses, probes), want, "random map")
    _same(m.cast(poses[1], probes[:1]), want[1:2, :1], "one pose, one probe")
    inside = np.column_stack([np.random.default_rng(8).uniform(-0.5, 0.5, (5, 2)), np.linspace(-3.0, 3.0, 5)]).astype(np.float32)
    _same(m.cast(inside, probes), ce.expect_poses(g, log, probes, inside), "five more poses inside the map")
    m.close()


# ---- 2: constructed cases ----------------------------------------------------------------------------------------------------
def _map_64x48(**kw):
    m = GridMap(3.18, 2.38, RES, (0.0, 0.0), **kw)
    g = orc.Grid(3.18, 2.38, RES, 0.0, 0.0)
    assert (m.W, m.H, g.W, g.H) == (64, 48, 64, 48)
    return m, g


def test_constructed_cases():
    m, g = _map_64x48(max_beams=96)
    pose = np.array([0.5, 0.5, 0.0], dtype=np.float32)                     # start (10.0, 10.0): the walk starts in cell floor(10.0 + 0.5) = 10
    cell = lambda cx, cy: ce.probes_from([cx * RES], [cy * RES])           # a probe ending cx, cy cells from the start
    def case(occupied, probes, pose=pose):
        log = np.full((48, 64), g.l_free)
        for (x, y) in occupied:
            log[y, x] = g.l_occ
        m.upload_log(log)
        want = ce.expect(g, log, probes, pose)
        _same(m.cast(pose, probes)[0], want, str(occupied))
        return want
    r = case([(10, 10)], cell(5, 0))
    assert (r["step"][0], r["x"][0], r["y"][0]) == (0, 10, 10), "the start cell occupied"
    r = case([(16, 10)], cell(5, 0))                                       # the end point is cell 15: a wall exactly one step past it
    assert (r["step"][0], r["x"][0]) == (6, 16), r
    r = case([(15 + EXTRA + 1, 10)], cell(5, 0))                           # extra_steps + 1 past it: not on the walk
    assert r["step"][0] == -1 and r["range"][0] == np.float32(cell(5, 0)["distance"][0]) / np.float32(RES), r
    r = case([(15 + EXTRA, 10)], cell(5, 0))                               # ... the last cell that is
    assert (r["step"][0], r["x"][0]) == (5 + EXTRA, 15 + EXTRA), r
    corner = np.array([0.1, 0.1, 0.0], dtype=np.float32)                   # cell (2, 2): a ray leaving through the corner (0, 0)
    r = case([(0, 0)], ce.probes_from([-1.0], [-1.0]), corner)
    assert (r["x"][0], r["y"][0]) == (0, 0), r
    r = case([], ce.probes_from([-1.0], [-1.0]), corner)
    assert r["step"][0] == -1
    # B = the handle's max_beams (one more is refused, nothing enqueued)
    rng = np.random.default_rng(5)
    fan = ce.probes_from(rng.uniform(-1.5, 1.5, 96), rng.uniform(-1.5, 1.5, 96))
    ring = [(x, y) for x in range(4, 60) for y in (4, 40)] + [(x, y) for x in (4, 59) for y in range(4, 41)]
    r = case(ring, fan, np.array([1.6, 1.1, 0.7], dtype=np.float32))
    assert (r["step"] >= 0).sum() > 48
    with pytest.raises(GmsError) as e:
        m.cast(pose, np.concatenate([fan, fan[:1]]))
    assert e.value.code == GMS_ERR_INVALID
    m.close()


# ---- 3: a batched map ----------------------------------------------------------------------------------------------------------
def test_batched_map_casts_in_the_map_it_names():
    m, g = _map_64x48(n_maps=2, max_beams=32)
    logs = np.full((2, 48, 64), g.l_free)
    logs[0, :, 20] = g.l_occ                                               # map 0: a wall at x = 20; map 1: at x = 30
    logs[1, :, 30] = g.l_occ
    m.upload_log(logs)
    pose = np.array([0.525, 1.2, 0.0], dtype=np.float32)
    probes = ce.probes_from(np.full(5, 1.5), np.linspace(-0.3, 0.3, 5))
    for mi in (0, 1):
        want = ce.expect(g, logs[mi], probes, pose)
        assert (want["x"] == (20, 30)[mi]).all()
        _same(m.cast(pose, probes, mi=mi)[0], want, f"map {mi}")
    with pytest.raises(GmsError):
        m.cast(pose, probes, mi=2)
    m.close()


# ---- 4: the deferred apply pass, idempotence, no trace left ------------------------------------------------------------------
def _trace_map(cast_between):
    ext = 3.2
    tr = synth.make_trace(ext, RES, 48, T=8, seed=23)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=64)
    probes = tr.scans[7]
    casts = []
    for t in range(5):
        m.update(tr.scans[t], tr.poses[t])                                 # (from the second one on the apply pass is deferred)
        if cast_between:
            casts.append(m.cast(tr.poses[t + 1], probes))
    return m, tr, casts


def test_deferred_pass_idempotence_and_twins():
    m, tr, casts = _trace_map(True)
    g = orc.Grid(3.2, 3.2, RES, -1.6, -1.6)
    probes, pose = tr.scans[7], tr.poses[6]
    m.update(tr.scans[5], tr.poses[5])                                     # its `logData +=` pass is still owed when the cast comes
    builds = m.cast_plane_builds()
    a = m.cast(pose, probes)
    b = m.cast(pose, probes)
    _same(a, b, "two casts in a row")
    assert m.cast_plane_builds() == builds + 1, "the bit plane of an unchanged map is packed once"
    log = m.download_log()
    assert (a["step"] >= 0).any() and (log > 0).any()
    _same(a[0], ce.expect(g, log, probes, pose), "against the oracle on the downloaded logData")
    fresh = GridMap(3.2, 3.2, RES, (-1.6, -1.6), max_beams=64)
    fresh.upload_log(log)
    _same(fresh.cast(pose, probes), a, "a fresh handle uploaded with the downloaded logData")
    fresh.close(); m.close()
    # twins: the same five updates, one of them casting between every two
    m1, _, casts = _trace_map(True)
    m2, _, _ = _trace_map(False)
    assert len(casts) == 5 and any((c["step"] >= 0).any() for c in casts)
    assert np.array_equal(m1.download_log(), m2.download_log())
    assert np.array_equal(m1.download_likelihood(), m2.download_likelihood())
    m1.close(); m2.close()


# ---- 5: from the filter's device-resident pose -------------------------------------------------------------------------------
def test_cast_at_equals_cast_at_the_reported_pose():
    m, tr, _ = _trace_map(False)
    pf = ParticleFilter(m, 64)
    pf.set_poses(synth.make_particles(tr.poses[5], 64, sigma_xy=0.05, sigma_theta_deg=3.0))
    pf.score(tr.scans[5])
    pf.normalize()
    last = pf.last_step()
    assert not np.array_equal(last["weighted_pose"], last["strongest_pose"])
    probes = tr.scans[6]
    for strongest, key in ((False, "weighted_pose"), (True, "strongest_pose")):
        got = m.cast_at(probes, pf, strongest=strongest)
        assert got.shape == (len(probes),) and (got["step"] >= 0).any()
        _same(got, m.cast(last[key], probes)[0], key)
    pf.close(); m.close()


# ---- 6: the LDS window against the memory form ---------------------------------------------------------------------------------
def _with_walk(mem, make):
    old = os.environ.pop("GMS_CAST_WALK", None)
    if mem:
        os.environ["GMS_CAST_WALK"] = "mem"                                # read when the handle is created
    try:
        return make()
    finally:
        os.environ.pop("GMS_CAST_WALK", None)
        if old is not None:
            os.environ["GMS_CAST_WALK"] = old


def test_lds_window_against_the_memory_form():
    g, log, poses, probes = random_case()
    want = ce.expect_poses(g, log, probes, poses)
    for mem in (False, True):
        m = _with_walk(mem, lambda: GridMap(1.83, 1.13, RES, (-0.915, -0.565), max_beams=128))
        m.upload_log(log)
        _same(m.cast(poses, probes), want, f"memory form {mem}")
        m.close()
    # 1200 x 1200 cells: probes across the whole map, so a workgroup's window (1200 rows of 38 words) exceeds the 64 KiB it may stage
    ext = 59.98
    gl = orc.Grid(ext, ext, RES, -ext / 2, -ext / 2)
    assert (gl.W, gl.H) == (1200, 1200)
    rng = np.random.default_rng(9)
    big = np.where(rng.random((1200, 1200)) < 0.002, gl.l_occ, gl.l_free)
    ang = rng.uniform(-math.pi, math.pi, 64)
    far = ce.probes_from(35.0 * np.cos(ang), 35.0 * np.sin(ang))
    pose = np.array([1.0, -2.0, 0.4], dtype=np.float32)
    wantl = ce.expect(gl, big, far, pose)
    assert (wantl["step"] > 300).any() and (wantl["step"] >= 0).mean() > 0.5
    near = ce.probes_from(2.0 * np.cos(ang), 2.0 * np.sin(ang))            # ... and probes whose window does fit, on the same map
    wantn = ce.expect(gl, big, near, pose)
    ml = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=64)
    ml.upload_log(big)
    _same(ml.cast(pose, far)[0], wantl, "window too large for the LDS")
    _same(ml.cast(pose, near)[0], wantn, "window staged")
    ml.close()


# ---- 7: the per-particle filter --------------------------------------------------------------------------------------------------
ODO = (0.02, 0.1)                                      # |dTheta| = 5.7 degrees: every update integrates (SLAM.java:82)


def _slam_probes():
    rng = np.random.default_rng(3)
    ang = rng.uniform(-math.pi, math.pi, 70)
    d = rng.uniform(0.1, 1.6, 70)
    return ce.probes_from(d * np.cos(ang), d * np.sin(ang))


def _drive_slam(s, scans, cast_between=None):
    """three updates with motion and one forced resample in between (the generation of the maps flips)"""
    for k in range(3):
        s.update(scans[k], ODO, seed=11, sequence=k)
        if cast_between is not None:
            s.cast(cast_between, "all")
        if k == 1:
            s.resample(0.37)
            if cast_between is not None:
                s.cast(cast_between, 0)


def _check_slam(s, g, probes, n):
    poses = s.get_particles()[0].reshape(-1, 3)
    want = np.stack([ce.expect(g, s.map_of(k), probes, poses[k]) for k in range(n)])
    assert (want["step"] >= 0).any() and (want["step"] < 0).any()
    every, none = s.cast(probes, "all")
    assert none is None
    _same(every, want, "all")
    for k in range(n):
        got, shown = s.cast(probes, k)
        assert shown == k
        _same(got, want[k], f"particle {k}")
    got, shown = s.cast(probes, "strongest")
    assert shown == s.last_stats["strongest"]
    _same(got, want[shown], "strongest")


@pytest.mark.parametrize("form", ["planes", "planes, GMS_CAST_WALK=mem", "no planes (17 taps)"])
def test_per_particle_filter(form):
    ext, n = 2.0, 5
    tr = synth.make_trace(ext, RES, 40, T=8, seed=31)
    g = orc.Grid(ext, ext, RES, -ext / 2, -ext / 2)
    assert (g.W, g.H) == (40, 40)
    kernel = TAPS_17 if form.startswith("no planes") else None
    make = lambda: SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=80, kernel=kernel)
    s = _with_walk("mem" in form, make)
    probes = _slam_probes()
    with pytest.raises(GmsError) as e:
        s.cast(probes, "strongest")                                        # before the first update there is none
    assert e.value.code == GMS_ERR_STATE
    with pytest.raises(GmsError) as e:
        s.cast(probes, n)
    assert e.value.code == GMS_ERR_INVALID
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    _drive_slam(s, tr.scans)
    _check_slam(s, g, probes, n)
    # twins: the same calls, one of them casting between every two
    t1, t2 = _with_walk("mem" in form, make), _with_walk("mem" in form, make)
    for t, between in ((t1, probes), (t2, None)):
        t.set_poses(np.tile(tr.poses[0], (n, 1)))
        _drive_slam(t, tr.scans, between)
    assert np.array_equal(t1.maps(), t2.maps()) and np.array_equal(t1.maps(likelihood=True), t2.maps(likelihood=True))
    assert np.array_equal(t1.get_particles()[0], t2.get_particles()[0]) and np.array_equal(t1.get_particles()[1], t2.get_particles()[1])
    for h in (s, t1, t2):
        h.close()


def test_per_particle_filter_batched():
    ext, n, S = 2.0, 5, 2
    tr = synth.make_trace(ext, RES, 40, T=8, seed=31)
    g = orc.Grid(ext, ext, RES, -ext / 2, -ext / 2)
    bat = SLAMParticleMapsBatch(S, ext, ext, RES, (-ext / 2, -ext / 2), num_particles=n, max_beams=80)
    probes = _slam_probes()
    with pytest.raises(GmsError) as e:
        bat.cast(probes, "strongest", filter=1)
    assert e.value.code == GMS_ERR_STATE
    bat.set_poses(np.stack([np.tile(tr.poses[0], (n, 1)), np.tile(tr.poses[3], (n, 1))]))
    for k in range(3):
        bat.update([tr.scans[k], tr.scans[3 + k]], [ODO, ODO], seeds=[11, 12], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.81])
    poses = bat.get_particles()[0]
    want = np.stack([ce.expect(g, bat.map_of(f, k), probes, poses[f, k]) for f in range(S) for k in range(n)])
    assert (want["step"] >= 0).any() and not np.array_equal(want[:n], want[n:])
    _same(bat.cast(probes, "all")[0], want, "all")
    for f in range(S):
        for k in range(n):
            got, shown = bat.cast(probes, k, filter=f)
            assert shown == f * n + k
            _same(got, want[f * n + k], f"filter {f} particle {k}")
        got, shown = bat.cast(probes, "strongest", filter=f)
        assert f * n <= shown < (f + 1) * n
        _same(got, want[shown], f"filter {f} strongest")
        assert np.array_equal(got, bat.cast(probes, shown - f * n, filter=f)[0])
    bat.close()


# ---- 8: non-finite inputs terminate --------------------------------------------------------------------------------------------
def test_non_finite_inputs_return_the_oracles_records():
    """a termination check on defined inputs: the oracle's walk of such a ray is what the device must return"""
    g, log, poses, probes = random_case()
    bad_poses = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, np.nan], poses[0]], dtype=np.float32)
    bad = probes[:8].copy()
    bad["local_x"][0] = np.inf
    bad["local_y"][1] = -np.inf
    bad["local_x"][2] = np.nan
    bad["distance"][3] = np.nan
    want = ce.expect_poses(g, log, bad, bad_poses)
    m = GridMap(1.83, 1.13, RES, (-0.915, -0.565), max_beams=128)
    m.upload_log(log)
    got = m.cast(bad_poses, bad)
    _same_nan(got, want)
    m.close()
    s = SLAMParticleMaps(2.0, 2.0, RES, (-1.0, -1.0), num_particles=2, max_beams=16)
    gs = orc.Grid(2.0, 2.0, RES, -1.0, -1.0)
    s.set_poses(np.array([[np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32))
    got = s.cast(bad, "all")[0]
    wants = np.stack([ce.expect(gs, s.map_of(k), bad, s.get_particles()[0][k]) for k in range(2)])
    _same_nan(got, wants)
    s.close()
