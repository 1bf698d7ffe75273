"""The ray cast's set-up -- beams loaded and slots / tile cleared in front of the pose, the producer walking as soon as it has error, dx,
dy and the step count, every consumer wavefront forming the rays' metas for itself, no set-up barrier -- against the oracle, at the
shapes where a moved barrier or a split set-up can go wrong.

What is compared, and how exactly:
  counts       the oracle's integers (Grid.scan_counts, the visits of integrateObservation per cell and class).  The device keeps them
               only between two launches; they are read back through the log-odds they produce: a cell's value after `update` is
               old + (n_free * l_free + n_occ * l_occ) in doubles (apply_body), which numpy forms from the oracle's integers with the
               same two multiplications and two additions: compared bit for bit.
  log-odds     bit for bit against that; against Grid.integrate -- which adds one increment per visit, in ray order, and so rounds
               differently from the device's counts-times-increment -- the touched cells are the same set and the values agree to
               1e-13 relative (the bound every map test of the suite uses for this sum of at most a few hundred terms of 2^-53 each).
  dirty box    the device keeps no readable copy; the likelihood field after `update` is rebuilt on the box's tiles only, so it equals
               the oracle's every-cell rebuild, bit for bit, only if the box covers every touched cell.
  trace_scan   ordered cells, classes and counts per beam, bit for bit."""
import numpy as np
import pytest

from gridmap_slam_robot_amd import BEAM_DTYPE, GridMap, ParticleFilter, _lib, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EXT, RES, POS = 12.8, 0.05, -6.4              # 256 x 256 cells
NEAR = ("0", "1")                             # GMS_RAYCAST_NEAR=1: near-field workgroups from 32 beams on


def _beams(lx, ly, d, hit):
    s = np.zeros(len(lx), dtype=BEAM_DTYPE)
    s["local_x"], s["local_y"], s["distance"], s["hit"] = lx, ly, d, hit
    return s


def _scan(rng, B, max_range=9.0):
    """hits and misses mixed, a tenth zero-length, a fifth far beyond the map whatever the direction"""
    a = np.sort(rng.uniform(-np.pi, np.pi, B))
    d = rng.uniform(0.0, max_range, B)
    d[rng.random(B) < 0.1] = 0.0
    d[rng.random(B) < 0.2] = 30.0
    return _beams(d * np.cos(a), d * np.sin(a), d, rng.random(B) < 0.6)


def _make(monkeypatch, near, extra=None, max_beams=64):
    """a device map and its oracle; extra: RayIterator's additionalSteps (gms_params.extra_steps) other than the default"""
    monkeypatch.setenv("GMS_RAYCAST_NEAR", near)
    g = orc.Grid(EXT, EXT, RES, POS, POS)
    if extra is not None:
        L = _lib.load()
        real = L.gms_params_default

        def with_extra(p, *a):
            rc = real(p, *a)
            p._obj.extra_steps = extra
            return rc
        monkeypatch.setattr(L, "gms_params_default", with_extra)
        g.g.extra_steps = extra
    m = GridMap(EXT, EXT, RES, (POS, POS), max_beams=max_beams)
    if extra is not None:
        monkeypatch.undo()
        monkeypatch.setenv("GMS_RAYCAST_NEAR", near)
    assert (m.W, m.H) == (g.W, g.H) == (256, 256)
    return m, g


def _expect(g, log, scan, pose):
    """the log-odds after this scan from the oracle's integer counts (module docstring); the oracle's own log advances beside it"""
    c = g.scan_counts(scan, pose).astype(np.float64)
    inc = c[:, 0] * g.l_free + c[:, 2] * g.l_occ
    want = np.where((c[:, 0] != 0) | (c[:, 2] != 0), log["dev"] + inc, log["dev"])
    g.integrate(log["orc"], scan, pose)
    log["dev"] = want
    return want


def _check_map(m, g, log):
    got = m.download_log().reshape(-1)
    assert np.array_equal(got, log["dev"])
    ref = log["orc"]
    assert np.array_equal(got != 0, ref != 0)
    nz = ref != 0
    if nz.any():
        assert np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])) <= 1e-13
    assert np.array_equal(m.download_likelihood().reshape(-1), g.build_likelihood(got))


def _check_trace(m, g, scan, pose):
    cells, cls, counts = m.trace_scan(scan, pose, cap=640)
    rays = g.scan_rays(scan, pose)
    for b in range(len(scan)):
        wc, wcls = g.apply_measurement(None, *rays[b][:5], bool(rays[b][5]))
        assert counts[b] == len(wc), b
        assert np.array_equal(cells[b, :counts[b]], wc) and np.array_equal(cls[b, :counts[b]], wcls), b


def _new_logs(g):
    return {"dev": g.new_log(), "orc": g.new_log()}


POSES = [np.array([0.3, -0.2, 0.3], np.float32),           # mid-map: end points beyond every edge among the 30 m beams
         np.array([-6.39, 6.39, -2.0], np.float32),        # a corner: most rays leave the map at once
         np.array([-7.0, 0.0, 0.0], np.float32)]           # the start cell outside the map: every ray empty


@pytest.mark.parametrize("near", NEAR)
@pytest.mark.parametrize("B", [1, 3, 5, 17, 33])
def test_partly_filled_workgroups_through_the_map_entry_points(monkeypatch, near, B):
    """beam counts that leave the last far-field (4 rays) and near-field (16 rays) workgroup partly empty, through update (host
    beams), update_dev, integrate_dev + a rebuild, and trace_scan; every scan twice in a row on the same handle"""
    import torch
    m, g = _make(monkeypatch, near)
    log = _new_logs(g)
    rng = np.random.default_rng(100 + B)
    for pose in POSES:
        scan = _scan(rng, B)
        _check_trace(m, g, scan, pose)
        d_beams = torch.from_numpy(scan.view(np.uint8).copy()).cuda()
        d_pose = torch.from_numpy(pose).cuda()
        for _ in range(2):
            m.update(scan, pose)
            _expect(g, log, scan, pose)
            _check_map(m, g, log)
        for _ in range(2):
            m.update_dev(d_beams.data_ptr(), B, d_pose.data_ptr())
            _expect(g, log, scan, pose)
            _check_map(m, g, log)
        m.integrate_dev(d_beams.data_ptr(), B, d_pose.data_ptr())
        m.compute_likelihood_map()
        _expect(g, log, scan, pose)
        _check_map(m, g, log)
    m.close()


def _length_scan(ks, cx=40, cy=100):
    """rays along +x from the middle of cell (cx, cy) that end k - 1 cells further: with extra_steps = 0 their walks are k steps"""
    pose = np.array([POS + (cx + 0.25) * RES, POS + (cy + 0.25) * RES, 0.0], np.float32)
    k = np.asarray(ks, dtype=np.float64)
    d = (k - 1.0) * RES
    return _beams(d, np.zeros(len(k)), d, np.arange(len(k)) % 2 == 0), pose


@pytest.mark.parametrize("near", NEAR)
def test_walks_of_exactly_one_word_a_block_and_one_step_more(monkeypatch, near):
    """n_eff = 1, 31, 32, 33, 63, 64, 65 (extra_steps = 0 makes a one-step walk possible): no full word, one word, one block and
    the first step past each; up to 64 the far-field workgroups have nothing to do once the near field counts block 0.  Alone (4 +
    3 rays), and repeated to 35 beams so that GMS_RAYCAST_NEAR=1 sends them through the near field.  n_eff = 0: the start cell
    outside the map (POSES[2]) and the empty lanes of a partly filled workgroup."""
    ks = [1, 31, 32, 33, 63, 64, 65]
    m, g = _make(monkeypatch, near, extra=0)
    log = _new_logs(g)
    scan, pose = _length_scan(ks)
    rays = g.scan_rays(scan, pose)
    lens = [len(g.apply_measurement(None, *r[:5], bool(r[5]))[0]) for r in rays]
    assert lens == ks, lens
    for s in (scan, np.tile(scan, 5)):
        _check_trace(m, g, s, pose)
        for _ in range(2):
            m.update(s, pose)
            _expect(g, log, s, pose)
            _check_map(m, g, log)
    empty = _scan(np.random.default_rng(5), 35)
    m.update(empty, POSES[2])
    _expect(g, log, empty, POSES[2])
    _check_map(m, g, log)
    m.close()


@pytest.mark.parametrize("near", NEAR)
def test_one_workgroup_mixes_an_empty_a_one_word_and_the_longest_ray(monkeypatch, near):
    """three rays from the map's corner: a one-word walk, the diagonal to the opposite corner (the longest walk the map allows: 500+
    steps, 16 words) and a zero-length ray; the workgroup's fourth lane holds no ray (n_eff = 0).  The consumers poll the long
    ray's slots while the short rays' are long published: nothing may be published before every wavefront has seen the slots
    cleared.  Then the same mix repeated to 36 beams (near field with GMS_RAYCAST_NEAR=1)."""
    m, g = _make(monkeypatch, near)
    log = _new_logs(g)
    pose = np.array([POS + 0.26 * RES, POS + 0.26 * RES, 0.0], np.float32)
    far = (256 - 0.5) * RES
    scan = _beams([10 * RES, far, 0.0], [3 * RES, far, 0.0], [0.5, 17.0, 0.0], [True, False, True])
    rays = g.scan_rays(scan, pose)
    lens = [len(g.apply_measurement(None, *r[:5], bool(r[5]))[0]) for r in rays]
    assert lens[0] <= 32 and lens[1] >= 500 and lens[2] == 3, lens
    for s in (scan, np.tile(scan, 12)):
        _check_trace(m, g, s, pose)
        for _ in range(2):
            m.update(s, pose)
            _expect(g, log, s, pose)
            _check_map(m, g, log)
    m.close()


def _sharded_step(pf, m, d_P, d_beams, B, r01, frac):
    """the sharded kernel on one rank: begin, (nothing to gather), end"""
    pf.slam_update_sharded_begin_dev(d_P.data_ptr(), d_beams.data_ptr(), B)
    m.synchronize()
    pf.gather_buffers()
    pf.slam_update_sharded_end_dev(d_beams.data_ptr(), B, r01, frac, True)


@pytest.mark.parametrize("near", NEAR)
@pytest.mark.parametrize("B", [5, 33])
def test_paired_sharded_and_separate_steps_agree_bit_for_bit_and_with_the_oracle(monkeypatch, near, B):
    """the pose folded in LDS by the ray workgroups themselves (slam_update_dev; the sharded kernel on one rank) against the
    separate calls, where it comes from memory (score, normalise, update_at_dev): same maps, same particles, bit for bit, and the
    oracle's integration at the weighted pose the filter reports.  The last step's cloud holds a NaN: a NaN weighted pose,
    (int)NaN -> 0."""
    import torch
    N = 300
    ms, g = {}, None
    for k in ("paired", "sharded", "separate"):
        ms[k], g = _make(monkeypatch, near)
    log = _new_logs(g)
    rng = np.random.default_rng(B)
    first = _scan(rng, 48, 6.0)
    for m in ms.values():
        m.update(first, POSES[0])
    _expect(g, log, first, POSES[0])
    pfs = {k: ParticleFilter(m, N) for k, m in ms.items()}
    pfs["sharded"].set_shard(0, N)
    for t in range(4):
        Ph = synth.make_particles(POSES[0], N, seed=40 + t, sigma_xy=0.02, sigma_theta_deg=0.5)
        if t == 3:
            Ph[7, 0] = np.nan
        scan = _scan(rng, B, 6.0)
        d_P = torch.from_numpy(Ph).cuda()
        d_beams = torch.from_numpy(scan.view(np.uint8).copy()).cuda()
        r01, frac = 0.3 + 0.1 * t, 0.5
        pfs["paired"].slam_update_dev(d_P.data_ptr(), d_beams.data_ptr(), B, r01, frac, True)
        _sharded_step(pfs["sharded"], ms["sharded"], d_P, d_beams, B, r01, frac)
        sep = pfs["separate"]
        sep.set_poses_dev(d_P.data_ptr()); sep.score_dev(d_beams.data_ptr(), B); sep.normalize(fetch=False)
        ms["separate"].update_at_dev(d_beams.data_ptr(), B, sep)
        wpose = pfs["paired"].last_step()["weighted_pose"]
        assert np.isnan(wpose).any() == (t == 3)
        assert np.array_equal(pfs["sharded"].last_step()["weighted_pose"], wpose, equal_nan=True)
        assert np.array_equal(sep.weighted_pose(), wpose, equal_nan=True)
        _expect(g, log, scan, wpose)
        _check_map(ms["paired"], g, log)
        ref_log, ref_lik = ms["paired"].download_log(), ms["paired"].download_likelihood()
        for k in ("sharded", "separate"):
            assert np.array_equal(ms[k].download_log(), ref_log), k
            assert np.array_equal(ms[k].download_likelihood(), ref_lik), k
        assert np.array_equal(pfs["sharded"].get_poses(), pfs["paired"].get_poses(), equal_nan=True)
        assert np.array_equal(pfs["sharded"].get_weights(), pfs["paired"].get_weights(), equal_nan=True)
    for pf in pfs.values():
        pf.close()
    for m in ms.values():
        m.close()
