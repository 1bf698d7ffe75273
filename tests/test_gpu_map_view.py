"""Map views on the device (include/gridmapslam.h "map views"): gms_map_view[_dev] and gms_slam_view[_dev] against pictures the
test builds itself from the doubles the download calls return (tests/_view_expect.py: the grey chain of the definition, invLogOdds
through the oracle's libm once per distinct log-odds value).  The inputs are first shown to hold no fragile cell -- none whose idx
changes when the value moves by 4 double ulps --, then every comparison is array_equal.  A view must show what a download would
return at that moment and must not change any later result of its handle: twins that never view end bit-identical.

`python tests/test_gpu_map_view.py <resample 0|1>` runs the per-particle scenario in a process of its own (the in-memory field state
needs GMS_SLAM_EAGER_LIK=1 in the environment the handle is created in)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _view_expect as ve
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError

pytestmark = pytest.mark.gpu

RES = 0.05
W, H = 37, 29                                          # neither a multiple of 4 or 8: rows of the rectangle start misaligned
RECTS = [None, (1, 2, 35, 26), (5, 0, 3, 29), (36, 28, 1, 1), (0, 0, 37, 1)]
DS = [1, 2, 3, 8]                                      # ragged last rows and columns; 8 exceeds some rectangles
ODO = (0.02, 0.1)                                      # |dTheta| = 5.7 degrees: every update integrates (SLAM.java:82)


def _check_views(view, log, lik, rects, ds, w, h):
    """view(rect, d, likelihood, packed) -> image, for every combination, against the expectation from the downloaded arrays"""
    idx = {False: ve.idx_map(log, False), True: ve.idx_map(lik, True)}
    for rect in rects:
        for d in ds:
            for likelihood in (False, True):
                for packed in (False, True):
                    want = ve.expect(idx[likelihood], rect or (0, 0, w, h), d, likelihood, packed)
                    got = view(rect, d, likelihood, packed)
                    assert got.dtype == want.dtype and got.shape == want.shape, (rect, d, likelihood, packed)
                    assert np.array_equal(got, want), (rect, d, likelihood, packed)


def _shared_map(n_maps=1):
    m = GridMap(1.83, 1.43, RES, (-0.915, -0.715), n_maps=n_maps, max_beams=32)
    assert (m.W, m.H) == (W, H) and len(m.kernel) == 7
    tr = synth.make_trace(1.8, RES, 24, T=8, seed=17)
    for t in range(3):
        scans = tr.scans[t] if n_maps == 1 else np.stack([tr.scans[(t + k) % 8] for k in range(n_maps)])
        poses = tr.poses[t] if n_maps == 1 else np.stack([tr.poses[(t + k) % 8] for k in range(n_maps)])
        m.update(scans, poses)
    return m


def test_shared_map_host_views():
    m = _shared_map()
    log, lik = m.download_log(), m.download_likelihood()
    assert (log < 0).any() and (log > 0).any() and (log == 0).any(), "free, occupied and unexplored cells must all occur"
    assert len(np.unique(lik)) > 3
    _check_views(lambda r, d, l, p: m.view(r, d, l, p), log, lik, RECTS, DS, W, H)
    m.close()


def test_shared_map_device_views_leave_the_guards_alone():
    import torch
    m = _shared_map()
    log, lik = m.download_log(), m.download_likelihood()

    def view(rect, d, likelihood, packed, shift=0):
        want_shape = ve.expect(np.zeros((H, W), np.int32), rect or (0, 0, W, H), d, likelihood, packed).shape
        nbytes = want_shape[0] * want_shape[1] * (4 if packed else 1)
        buf = torch.full((16 + shift + nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out = buf[16 + shift:16 + shift + nbytes]
        assert m.view(rect, d, likelihood, packed, out=out) is out
        m.synchronize()
        b = buf.cpu().numpy()
        assert (b[:16 + shift] == 0xA5).all() and (b[16 + shift + nbytes:] == 0xA5).all(), "bytes outside the output were written"
        return b[16 + shift:16 + shift + nbytes].copy().view(np.uint32 if packed else np.uint8).reshape(want_shape)

    _check_views(view, log, lik, RECTS, DS, W, H)
    # outputs that start 1, 2, 3 bytes (grey) / 4, 8, 12 bytes (packed) past a 16-byte boundary: short first groups
    for shift in (1, 2, 3):
        _check_views(lambda r, d, l, p: view(r, d, l, p, shift * (4 if p else 1)), log, lik, [None, (1, 2, 35, 26), (36, 28, 1, 1)], [1, 3], W, H)
    m.close()


def test_batched_map_view_of_one_map():
    m = _shared_map(n_maps=3)
    log, lik = m.download_log(), m.download_likelihood()
    assert not np.array_equal(log[2], log[0]) and not np.array_equal(log[2], log[1])
    _check_views(lambda r, d, l, p: m.view(r, d, l, p, mi=2), log[2], lik[2], [None, (1, 2, 35, 26)], [1, 3], W, H)
    with pytest.raises(GmsError) as e:
        m.view(mi=3)
    assert e.value.code == GMS_ERR_INVALID
    m.close()


def test_uploaded_values_and_rectangles_outside_the_map():
    m = GridMap(1.83, 1.43, RES, (-0.915, -0.715))
    log = np.zeros((H, W))
    log[2, 3], log[2, 4], log[2, 5], log[2, 6], log[2, 7] = 40.0, -40.0, 0.0, -0.0, np.nan
    m.upload_log(log)
    img = m.view()
    back = m.download_log()
    assert np.array_equal(ve.idx_map(back, False)[2, 3:8], [0, 255, 127, 127, 0])
    assert np.array_equal(img[2, 3:8], [0, 254, 126, 126, 0]) and np.array_equal(img, ve.expect(ve.idx_map(back, False), (0, 0, W, H), 1, False, False))
    assert np.array_equal(m.view(packed=True)[2, 3:8], [0xFE000000, 0xFEFEFEFE, 0xFE7E7E7E, 0xFE7E7E7E, 0xFE000000])
    # the library's clamp in the likelihood view: values no field holds
    lik = np.zeros((H, W))
    lik[1, :6] = [1.5, -0.25, np.inf, -np.inf, np.nan, 0.5]
    m.upload_likelihood(lik)
    assert np.array_equal(m.view(likelihood=True)[1, :6], [254, 0, 254, 0, 0, 126])
    before = img.copy()
    for rect in [(0, 0, W + 1, 1), (0, 0, 1, H + 1), (W, 0, 1, 1), (1, 0, W, 1), (0, H - 1, 1, 2), (0, 0, 0, 1), (-1, 0, 2, 2)]:
        with pytest.raises(GmsError) as e:
            m.view(rect)
        assert e.value.code == GMS_ERR_INVALID, rect
    with pytest.raises(GmsError):
        m.view(decimate=0)
    assert np.array_equal(m.view(), before)
    # the world rectangle helper: (int)((x - position) / resolution) in float, clamped
    assert m.world_rect((0.0, 0.0), (0.5, 0.5)) == (13, 9, 11, 11)
    assert m.world_rect((-5.0, 0.0), (9.0, 100.0)) == (0, 0, 9, H)
    with pytest.raises(ValueError):
        m.world_rect((5.0, 0.0), (1.0, 1.0))
    m.close()


def test_views_between_fused_steps_show_the_deferred_pass_and_change_nothing():
    """two fused scan steps (gms_slam_update: the scan's `logData +=` pass stays deferred, the field lazily kept): a view after each
    equals the downloads made right after it; a twin that never views ends bit-identical"""
    ext, n, b = 3.2, 64, 32
    tr = synth.make_trace(ext, RES, b, T=8, seed=7)
    out = []
    for viewing in (True, False):
        m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=b)
        assert (m.W, m.H) == (64, 64)
        for t in range(2):
            m.update(tr.scans[t], tr.poses[t])
        pf = ParticleFilter(m, n)
        for t in (2, 3):
            P = synth.make_particles(tr.poses[t], n, seed=t, sigma_xy=0.03, sigma_theta_deg=1.0)
            pf.slam_update(P, tr.scans[t], 0.25, 0.5, True)
            if viewing:
                imgs = {(l, p): m.view(None, 1, l, p) for l in (False, True) for p in (False, True)}
                over = {l: m.view((3, 1, 60, 61), 4, l) for l in (False, True)}
                log, lik = m.download_log(), m.download_likelihood()
                idx = {False: ve.idx_map(log, False), True: ve.idx_map(lik, True)}
                for (l, p), img in imgs.items():
                    assert np.array_equal(img, ve.expect(idx[l], (0, 0, 64, 64), 1, l, p)), (t, l, p)
                for l, img in over.items():
                    assert np.array_equal(img, ve.expect(idx[l], (3, 1, 60, 61), 4, l, False)), (t, l)
        out.append((m.download_log(), m.download_likelihood(), pf.get_poses().copy(), pf.get_weights().copy()))
        pf.close(); m.close()
    for name, a, c in zip(("logData", "likelihoodData", "poses", "weights"), *out):
        assert np.array_equal(a, c), f"{name} differs on the handle that was viewed"


# ---- the per-particle filter ---------------------------------------------------------------------------------------------------
PM_EXT, PM_N, PM_B = 2.0, 16, 24                       # 40 x 40 cells


def _pm_handle(tr):
    s = SLAMParticleMaps(PM_EXT, PM_EXT, RES, (-PM_EXT / 2, -PM_EXT / 2), num_particles=PM_N, max_beams=32)
    assert (s.W, s.H) == (40, 40)
    s.set_poses(synth.make_particles(tr.poses[0], PM_N, seed=3, sigma_xy=0.03, sigma_theta_deg=4.0))
    return s


def _pm_check(a, b, strongest):
    """every particle's view on a (never read) against the expectation from the twin b's downloads; the strongest one's, picked on
    the device"""
    idx = {}
    for i in range(PM_N):
        for l in (False, True):
            idx[i, l] = ve.idx_map(b.map_of(i, likelihood=l), l)
            img, shown = a.view(i, likelihood=l)
            assert shown == i and np.array_equal(img, ve.expect(idx[i, l], (0, 0, 40, 40), 1, l, False)), (i, l)
    for l in (False, True):
        for rect, d, p in ((None, 1, True), ((3, 5, 33, 31), 3, False)):
            img, shown = a.view("strongest", rect, d, l, p)
            assert shown == strongest
            assert np.array_equal(img, ve.expect(idx[shown, l], rect or (0, 0, 40, 40), d, l, p)), (l, rect, d, p)


def _pm_scenario(resample):
    """a: viewed, never downloaded from; b: its twin, downloaded from; c: the twin nobody looks at until the end"""
    tr = synth.make_trace(PM_EXT, RES, PM_B, T=6, seed=31)
    a, b, c = (_pm_handle(tr) for _ in range(3))
    with pytest.raises(GmsError) as e:                 # no update yet: nothing names a strongest particle
        a.view("strongest")
    assert e.value.code == GMS_ERR_STATE
    for s in (a, b, c):
        s.update(tr.scans[0], None)
        s.update(tr.scans[1], ODO, seed=11, sequence=1)
    assert a.strongest == b.strongest == c.strongest
    _pm_check(a, b, a.strongest)
    if resample:
        idx = [s.resample(0.37, want_indices=True)[0] for s in (a, b, c)]
        assert np.array_equal(idx[0], idx[1]) and np.array_equal(idx[0], idx[2])
        assert not np.array_equal(idx[0], np.arange(PM_N)), "the draw must move maps"
        _pm_check(a, b, a.strongest)                   # the statistics the last update left outlive the resample()
    for s in (a, c):
        s.update(tr.scans[2], ODO, seed=11, sequence=2)
    (Pa, wa), (Pc, wc) = a.get_particles(), c.get_particles()
    assert np.array_equal(Pa, Pc) and np.array_equal(wa, wc)
    assert np.array_equal(a.maps(), c.maps()) and np.array_equal(a.maps(likelihood=True), c.maps(likelihood=True))
    a.reset()
    with pytest.raises(GmsError) as e:
        a.view("strongest")
    assert e.value.code == GMS_ERR_STATE
    img, shown = a.view(5)                             # a named particle needs no statistics: a blank map
    assert shown == 5 and (img == 126).all()
    with pytest.raises(GmsError) as e:
        a.view(PM_N)
    assert e.value.code == GMS_ERR_INVALID
    for s in (a, b, c):
        s.close()


@pytest.mark.parametrize("resample", [False, True], ids=["updated", "resampled"])
def test_per_particle_views_fields_in_the_class_planes(resample):
    """the default storage form: the fields are implicit in the class planes (SLAM_FIELD_FROM_PLANES), in either generation"""
    _pm_scenario(resample)


@pytest.mark.parametrize("resample", [False, True], ids=["in_memory", "owed_copy"])
def test_per_particle_views_fields_in_memory(resample):
    """GMS_SLAM_EAGER_LIK=1 in a child process: every update writes every field (SLAM_FIELD_IN_MEMORY), a resample() owes the copies
    (SLAM_FIELD_OWED_COPY)"""
    env = dict(os.environ, GMS_SLAM_EAGER_LIK="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(int(resample))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scenario ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_batched_filter_handle_strongest_of_one_filter():
    """S = 2 filters of n = 8: `which` and `shown` are handle-wide slots f * n + k (gms_slam_download_map's index space); the
    statistics' strongest is filter-local"""
    S, n = 2, 8
    tr = synth.make_trace(PM_EXT, RES, PM_B, T=6, seed=31)
    hs = [SLAMParticleMapsBatch(S, PM_EXT, PM_EXT, RES, (-PM_EXT / 2, -PM_EXT / 2), num_particles=n, max_beams=32) for _ in range(2)]
    P = np.stack([synth.make_particles(tr.poses[f], n, seed=3 + f, sigma_xy=0.03, sigma_theta_deg=4.0) for f in range(S)])
    for s in hs:
        s.set_poses(P)
        s.update([tr.scans[0], tr.scans[1]], None)
        s.update([tr.scans[1], tr.scans[2]], [ODO, (0.01, -0.05)], seeds=[5, 6], sequence=1)
    a, b = hs
    assert np.array_equal(a.strongest, b.strongest)
    for f in range(S):
        k = int(a.strongest[f])
        for l in (False, True):
            img, shown = a.view("strongest", filter=f, likelihood=l)
            assert shown == f * n + k
            assert np.array_equal(img, ve.expect(ve.idx_map(b.map_of(f, k, likelihood=l), l), (0, 0, 40, 40), 1, l, False)), (f, l)
    img, shown = a.view(3, filter=1)
    assert shown == n + 3 and np.array_equal(img, ve.expect(ve.idx_map(b.map_of(1, 3), False), (0, 0, 40, 40), 1, False, False))
    assert not np.array_equal(b.map_of(0, int(a.strongest[0])), b.map_of(1, int(a.strongest[1])))
    with pytest.raises(IndexError):
        a.view("strongest", filter=2)
    for s in hs:
        s.close()


def test_combined_map_through_the_handles_own_map():
    tr = synth.make_trace(PM_EXT, RES, PM_B, T=6, seed=31)
    s = _pm_handle(tr)
    s.update(tr.scans[0], None)
    s.update(tr.scans[1], ODO, seed=11, sequence=1)
    log = s.calculate_combined()
    assert len(np.unique(log)) > 8
    for l, data in ((False, log), (True, s.grid_map.download_likelihood())):
        for rect, d in ((None, 1), ((2, 3, 37, 35), 2)):
            assert np.array_equal(s.grid_map.view(rect, d, l), ve.expect(ve.idx_map(data, l), rect or (0, 0, 40, 40), d, l, False)), (l, rect, d)
    s.close()


if __name__ == "__main__":
    _pm_scenario(bool(int(sys.argv[1])))
    print("scenario ok")
