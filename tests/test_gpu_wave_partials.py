"""The stand-alone single-map scan step reduces its weights one row per WAVEFRONT (k_partials_wave: 64 particles, no barrier, no
LDS) and the folds of the next launch add a block's four rows themselves (k_norm_raycast<false, true>), in the order the block
kernel's LDS combine uses.  The separate entry points keep the block kernel, so "scan step == separate calls, bit for bit" is the
statement that the two forms agree: poses, weights, the five statistics, the weighted pose, the map.

One 64 x 64 map, 24 beams (two segments).  Populations: 64 (one wavefront, a quarter of a block), 192 (a block short of one
wavefront), 256 (one full block), 320 (a block plus one wavefront), 1088 (several blocks plus one wavefront).  Three steps each:
resampling not taken, forced, decided by Neff.  Then three hand-built weight patterns at 576 particles (two blocks and a
wavefront): every weight zero but one in the last wavefront of a block; two exactly equal maxima in two wavefronts of one block;
two exactly equal maxima in two blocks -- the lower index wins.  A particle far outside the map scores exactly 1.0 (every end
point reads the neutral factor) and any particle inside scores less, which is how the equal maxima are built.  Exact zeros cannot
come from 24 factors >= 0.01, so that one pattern scores a hand-built scan of 384 short beams (32 segments), whose products
underflow for every particle inside the map.

Against the oracle (first step, nothing resampled), with bounds from the arithmetic, eps = 2^-53: two association orders of a
product of B factors differ by at most 2 B eps; two orders of a sum of N positive terms by 2 N eps; a quotient adds eps on each
side.  Hence: raw weight 2 B eps; weight sum 2 (B + N) eps; normalised weight 2 (2 B + N + 1) eps; Neff = 1 / sum wn^2 four times
that plus 6 N eps (squares, their sum, the sum of the normalised weights squared); the largest log-weight 2 B eps (1 + |log w|)
absolute; the weighted pose one float32 ulp plus 2 (B + N) eps times the largest coordinate of the cloud (the double quotient
before it is narrowed).  strongest exactly; n_zero is the device's own count of zeros, each of them below 1e-300 in the oracle
(its sequential product can stick at the smallest denormal where the device, with an exact exponent, rounds once to 0: the
convention of test_gpu_parity.py)."""
import functools

import numpy as np
import pytest

from gridmap_slam_robot_amd import BEAM_DTYPE, GridMap, ParticleFilter, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EXT, RES, B = 3.2, 0.05, 24                      # 64 x 64 cells
ORIGIN = (-EXT / 2, -EXT / 2)
WARM = 3
EPS = 2.0 ** -53
FRACTIONS = (0.0, 2.0, 0.5)
OUTSIDE = np.array([[1e5, 1e5, 0.0], [2e5, 1e5, 1.0]], dtype=np.float32)      # every end point beyond the map: weight exactly 1.0


@functools.lru_cache(maxsize=None)
def _trace():
    return synth.make_trace(EXT, RES, B, T=16, seed=7, n_scans=WARM + len(FRACTIONS))


@functools.lru_cache(maxsize=None)
def _short_scan():
    """384 hits 0.1 m from the sensor: from anywhere inside the map every end point is inside it too"""
    a = 2 * np.pi * np.arange(384) / 384
    s = np.zeros(384, dtype=BEAM_DTYPE)
    s["local_x"] = 0.1 * np.cos(a); s["local_y"] = 0.1 * np.sin(a); s["distance"] = 0.1; s["hit"] = 1
    return s


def _new_map():
    tr = _trace()
    m = GridMap(EXT, EXT, RES, ORIGIN, max_beams=384)
    assert (m.W, m.H) == (64, 64)
    for t in range(WARM):
        m.update(tr.scans[t], tr.poses[t])
    return m


def _cloud(n, k):
    return synth.make_particles(_trace().poses[WARM + k], n, seed=40 + k, sigma_xy=0.03, sigma_theta_deg=2.0)


def _check_oracle(m, lik_before, pf, scan, P, n, nb, what):
    g = orc.Grid(EXT, EXT, RES, ORIGIN[0], ORIGIN[1])
    want = g.score(lik_before, scan, P)
    got = pf.get_weights()
    zeros, ok = got == 0, want > 1e-290
    assert np.all(want[zeros] < 1e-300) and np.all(got[~ok] <= 1e-280) and ok.any(), what
    wn = want.copy()
    ws, strongest = orc.normalize(wn)
    st = pf.stats()
    tol_w = 2 * nb * EPS
    tol_s = 2 * (nb + n) * EPS
    tol_n = 2 * (2 * nb + n + 1) * EPS
    print(f"{what}: weight_sum rel {abs(st['weight_sum'] - ws) / ws:.3g} (bound {tol_s:.3g}), weights rel "
          f"{np.max(np.abs(got[ok] - wn[ok]) / wn[ok]):.3g} (bound {tol_n:.3g})")
    assert st["strongest"] == strongest, what
    assert st["n_zero"] == int(zeros.sum()), what
    assert abs(st["weight_sum"] - ws) <= tol_s * ws, what
    assert np.max(np.abs(got[ok] - wn[ok]) / wn[ok]) <= tol_n, what
    ne = orc.neff(wn)
    assert abs(st["neff"] - ne) <= (4 * tol_n + 6 * n * EPS) * ne, what
    lw = g.score_log(lik_before, scan, P).max()
    assert abs(st["max_log_weight"] - lw) <= tol_w * (1 + abs(lw)), what
    wp, wo = pf.last_step()["weighted_pose"], orc.weighted_pose(P, wn)
    reach = np.maximum(np.abs(P.astype(np.float64)).max(axis=0), [0.0, 0.0, np.pi])       # (angleConstrain(theta) lies within pi)
    assert np.all(np.abs(wp.astype(np.float64) - wo) <= np.spacing(np.abs(wo)).astype(np.float64) + tol_s * reach), what


def _step_against_separate(n, cloud, scan_of, nb, check=None):
    """three steps of the paired scan step (handles a) and of the separate entry points (handles b), compared after each"""
    import torch
    dev = torch.device("cuda", 0)
    a, b = _new_map(), _new_map()
    pa, pb = ParticleFilter(a, n), ParticleFilter(b, n)
    rng = np.random.default_rng(n)
    for k, frac in enumerate(FRACTIONS):
        what = f"n={n} B={nb} step {k}"
        scan, Ph = scan_of(k), cloud(k)
        assert Ph.shape == (n, 3) and len(scan) == nb
        beams = torch.from_numpy(scan.view(np.uint8).copy()).to(dev)
        P = torch.from_numpy(Ph).to(dev)
        r01 = float(rng.random())
        lik_before = a.download_likelihood().reshape(-1) if k == 0 else None
        pa.slam_update_dev(P.data_ptr(), beams.data_ptr(), nb, r01, frac, True)
        pb.set_poses_dev(P.data_ptr()); pb.score_dev(beams.data_ptr(), nb)
        raw = pb.get_weights() if check else None
        pb.normalize(fetch=False)
        wp_b = pb.weighted_pose()
        pb.resample_if(r01, frac)
        b.update_at_dev(beams.data_ptr(), nb, pb)
        torch.cuda.synchronize()
        if check:
            check(raw, pa, what)
        sa, sb = pa.stats(), pb.stats()
        assert sa == sb and set(sa) >= {"weight_sum", "neff", "strongest", "n_zero", "max_log_weight"}, (what, sa, sb)
        la, lb = pa.last_step(), pb.last_step()
        assert np.array_equal(la["weighted_pose"], lb["weighted_pose"]) and np.array_equal(la["weighted_pose"], wp_b), what
        assert la["did_resample"] == lb["did_resample"] and (frac != 2.0 or la["did_resample"]) and (frac != 0.0 or not la["did_resample"]), what
        assert np.array_equal(pa.get_poses(), pb.get_poses()), what
        assert np.array_equal(pa.get_weights(), pb.get_weights()), what
        assert np.array_equal(pa.weighted_pose(), pb.weighted_pose()), what      # of the particles as they are now
        assert np.array_equal(a.download_log(), b.download_log()), what
        assert np.array_equal(a.download_likelihood(), b.download_likelihood()), what
        if k == 0:
            _check_oracle(a, lik_before, pa, scan, Ph, n, nb, what)
    for h in (pa, pb, a, b):
        h.close()


@pytest.mark.parametrize("n", [64, 192, 256, 320, 1088])
def test_populations_at_the_wavefront_and_block_edges(n):
    _step_against_separate(n, lambda k: _cloud(n, k), lambda k: _trace().scans[WARM + k], B)


@pytest.mark.parametrize("n", [64, 320, 1088])
@pytest.mark.parametrize("route", ["log-normalising", "two maps"])
def test_block_rows_of_the_scan_step_equal_the_separate_calls(n, route):
    """The two routes of the scan step that keep BLOCK rows, where the tests above take wavefront rows: log-normalisation on
    (k_partials' block-relative rows through the scaled fold) and two maps in one handle under plain normalisation (the batched
    k_partials).  Each against gms_pf_score -> normalize -> stats on a filter of its own, bit for bit: the weights, the
    statistics (weight_sum, strongest, n_zero, max_log_weight) and the weighted pose.  No resampling, and the separate calls go
    first: the weights stay comparable and both filters score against the same map, which the step then updates."""
    M = 2 if route == "two maps" else 1
    tr = _trace()
    m = GridMap(EXT, EXT, RES, ORIGIN, n_maps=M, max_beams=384)
    for t in range(WARM):
        m.update(np.stack([tr.scans[t]] * M) if M > 1 else tr.scans[t], np.stack([tr.poses[t]] * M) if M > 1 else tr.poses[t])
    P = np.stack([synth.make_particles(tr.poses[WARM], n, seed=60 + i, sigma_xy=0.03, sigma_theta_deg=2.0) for i in range(M)])
    scan = np.stack([tr.scans[WARM]] * M) if M > 1 else tr.scans[WARM]
    step, sep = ParticleFilter(m, n), ParticleFilter(m, n)
    for f in (step, sep):
        f.set_log_normalize(route == "log-normalising")
    sep.set_poses(P if M > 1 else P[0]); sep.score(scan)
    st_sep = sep.normalize()
    step.slam_update(P if M > 1 else P[0], scan, np.full(M, 0.4), 0.0, True)
    st_step = step.stats()
    keys = {"weight_sum", "strongest", "n_zero", "max_log_weight"}
    for a, b in zip(st_step if M > 1 else [st_step], st_sep if M > 1 else [st_sep]):
        assert set(a) >= keys and {k: a[k] for k in keys} == {k: b[k] for k in keys} and a["weight_sum"] > 0, (route, n, a, b)
    assert np.array_equal(step.get_weights(), sep.get_weights()), (route, n)
    assert np.array_equal(step.get_log_weights(), sep.get_log_weights()), (route, n)
    assert np.array_equal(step.last_step()["weighted_pose"], sep.last_step()["weighted_pose"]), (route, n)
    assert np.array_equal(np.asarray(step.last_step()["weighted_pose"]).reshape(M, 3), np.asarray(sep.weighted_pose()).reshape(M, 3)), (route, n)
    for h in (step, sep, m):
        h.close()


N_PAT = 576                                      # blocks 0 and 1 full, block 2 one wavefront


def test_every_weight_zero_but_one_in_the_last_wavefront_of_a_block():
    one = 256 + 3 * 64 + 17                      # block 1, wavefront 3
    def cloud(k):
        P = _cloud(N_PAT, k)
        P[one] = OUTSIDE[0]
        return P
    def check(raw, pa, what):
        assert raw[one] == 1.0 and int((raw == 0).sum()) == N_PAT - 1, what
        st = pa.stats()
        assert st["strongest"] == one and st["n_zero"] == N_PAT - 1 and st["weight_sum"] == 1.0, (what, st)
    _step_against_separate(N_PAT, cloud, lambda k: _short_scan(), 384, check)


@pytest.mark.parametrize("first,second", [(64 + 5, 3 * 64 + 9), (256 + 40, 512 + 33)],
                         ids=["two wavefronts of one block", "two blocks"])
def test_of_two_exactly_equal_maxima_the_lower_index_wins(first, second):
    def cloud(k):
        P = _cloud(N_PAT, k)
        P[first], P[second] = OUTSIDE[0], OUTSIDE[1]
        return P
    def check(raw, pa, what):
        assert raw[first] == 1.0 == raw[second] and int((raw >= 1.0).sum()) == 2, what
        assert pa.stats()["strongest"] == first, what
    _step_against_separate(N_PAT, cloud, lambda k: _trace().scans[WARM + k], B, check)
