"""Pose modes on the device (include/gridmapslam.h "pose modes"): gms_pf_modes against tests/_modes_expect.py -- bins from
cells_of_poses and the header's heading rule, a flood fill over a Python set, the sums in the header's order by numpy.  Every comparison
is array_equal, the doubles as uint64 views: there is no tolerance.  The cached trig the sums read is what the handle's pose_trig makes
of the headings (Map.debug_f32; tests/test_gpu_parity.py holds that against the oracle's libm).

The shapes are small: a 64 x 64 map at 0.05 m, and a 70 x 50 one whose last bins are partial under bin_cells 4 and 7; filters of 1,
255, 256, 257 and 1000 particles around the 256 lanes of the sums' rows.  They are the smallest at which the binning, the unions and
the sums can go wrong, not the scans: no table here holds more than 300 modes, and anchors lie in one round of the scan's top level.
tests/test_gpu_scan_levels.py carries the scans past one block of the table, past one round of the bins and through a table that
grows."""
import ctypes as C

import numpy as np
import pytest

import _modes_expect as mx
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, _lib, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GMS_MODE_NONE, MODE_DTYPE, GmsError, GmsModes

pytestmark = pytest.mark.gpu

RES = 0.05
INTS = ("anchor_bx", "anchor_by", "anchor_bt", "count", "bins", "strongest", "min_bx", "min_by", "max_bx", "max_by", "pad")


def _make_map(W, H, pos=(0.0, 0.0), **kw):
    m = GridMap((W - 0.4) * RES, (H - 0.4) * RES, RES, pos, max_beams=360, **kw)
    assert (m.W, m.H) == (W, H)
    return m


def _same_records(got, want, where=""):
    assert got.dtype == want.dtype == MODE_DTYPE and got.shape == want.shape, (where, got.shape, want.shape)
    for name in INTS:
        assert np.array_equal(got[name], want[name]), (where, name, got[name], want[name])
    for name in mx.SUMS:
        g, w = np.ascontiguousarray(got[name]).view(np.uint64), np.ascontiguousarray(want[name]).view(np.uint64)
        assert np.array_equal(g, w), (where, name, got[name][g != w][:3], want[name][g != w][:3])
    assert got.tobytes() == want.tobytes(), where


def _trig(m, theta):
    th = np.ascontiguousarray(theta, dtype=np.float32)
    return np.stack([m.debug_f32(1, th), m.debug_f32(2, th)], axis=-1)


def _expect(pf, m, bin_cells, n_theta, min_count=1, mi=None, cap=None, pos=(0.0, 0.0)):
    poses, w = pf.get_poses(), pf.get_weights()
    if mi is not None:
        poses, w = poses[mi], w[mi]
    return mx.expect(poses, w, _trig(m, poses[:, 2]), pos, RES, m.W, m.H, bin_cells, n_theta, min_count, cap)


def _check(pf, m, bin_cells, n_theta, min_count=1, where="", pos=(0.0, 0.0)):
    """the host form, labels and table, against the expectation; returns (records, labels, n_outside)"""
    want, want_lab, want_out = _expect(pf, m, bin_cells, n_theta, min_count, pos=pos)
    rec, n_found, n_out, lab = pf.modes(bin_cells, n_theta, min_count=min_count, labels=True, cap=max(len(want), 1))
    assert (n_found, n_out) == (len(want), want_out), where
    assert lab.dtype == np.uint32 and np.array_equal(lab, want_lab), where
    _same_records(rec, want, where)
    return rec, lab, n_out


def _pose_in(bx, by, bt, bin_cells, n_theta, turns=0):
    """the pose at the centre of bin (bx, by, bt); turns: whole turns added to the heading"""
    c = (bin_cells * np.array([bx, by], dtype=np.float64) + 0.5 * bin_cells) * RES
    return [c[0], c[1], (bt + 0.5 + turns * n_theta) * (2 * np.pi / n_theta)]


def _filter(m, poses, weights=None):
    p = np.asarray(poses, dtype=np.float32).reshape(-1, 3)
    pf = ParticleFilter(m, len(p))
    pf.set_poses(p)
    if weights is not None:
        pf.set_weights(weights)
    return pf


def _blob(rng, n, centre, theta, sigma=0.08, sigma_th=0.05):
    return np.column_stack([rng.normal(centre[0], sigma, n), rng.normal(centre[1], sigma, n), rng.normal(theta, sigma_th, n)])


def test_blobs_and_a_heading_that_straddles_pi():
    m = _make_map(64, 64)
    rng = np.random.default_rng(3)
    three = [_blob(rng, 150, (0.6, 0.6), 0.4), _blob(rng, 150, (2.5, 0.8), -1.2), _blob(rng, 150, (1.0, 2.6), 2.0)]
    # the fourth: one place, headings on both sides of +-pi (bins 3 and 4 of 8 through the non-negative mod), and of 0 (bins 7 and 0)
    at_pi = np.concatenate([rng.uniform(np.pi - 0.3, np.pi, 60), rng.uniform(-np.pi, -np.pi + 0.3, 60)])
    fourth = np.column_stack([rng.normal(2.6, 0.02, 120), rng.normal(2.6, 0.02, 120), at_pi])
    pf = _filter(m, np.concatenate(three + [fourth]), rng.uniform(0.1, 1.0, 570))
    rec, lab, _ = _check(pf, m, 4, 8, where="three blobs and one across pi")
    assert len(set(lab[450:])) == 1 and len(rec) == 4, "ONE mode across +-pi"
    assert sorted(rec["count"]) == [120, 150, 150, 150]
    # its two halves two heading bins apart: bins 3 and 5 are no neighbours
    apart = fourth.copy()
    apart[:60, 2] = rng.uniform(np.pi - 0.3, np.pi - 0.1, 60)                  # bin 3
    apart[60:, 2] = rng.uniform(-np.pi + 0.85, -np.pi + 1.1, 60)               # bin 5
    poses = np.concatenate(three + [apart]).astype(np.float32)
    pf.set_poses(poses)
    rec, lab, _ = _check(pf, m, 4, 8, where="the fourth split")
    assert len(set(lab[450:510])) == 1 and len(set(lab[510:])) == 1 and lab[450] != lab[510] and len(rec) == 5
    # across heading 0: bins 7 and 0 wrap
    apart[:, 2] = np.concatenate([rng.uniform(-0.3, -0.01, 60), rng.uniform(0.01, 0.3, 60)])
    pf.set_poses(np.concatenate(three[1:] + [three[0], apart]).astype(np.float32))
    rec, lab, _ = _check(pf, m, 4, 8, where="the fourth across 0")
    assert len(set(lab[450:])) == 1 and len(rec) == 4
    pf.close(); m.close()


def test_corner_contact_unites_and_a_gap_does_not():
    m = _make_map(64, 64)
    B, T = 4, 8
    bins = [(2, 2, 0), (3, 3, 1),                         # a corner in (x, y, theta): one mode
            (8, 2, 0), (10, 2, 0),                        # two apart in x: two
            (2, 8, 0), (2, 8, 2),                         # two apart in theta: two
            (12, 12, 7), (13, 11, 0),                     # a corner through the heading wrap: one
            (15, 15, 3), (15, 15, 4), (15, 15, 5)]        # a column in theta: one
    poses = [_pose_in(*b, B, T, turns=k % 3 - 1) for k, b in enumerate(bins)]          # (whole turns: the non-negative mod)
    pf = _filter(m, poses)
    rec, lab, _ = _check(pf, m, B, T, where="contacts")
    assert len(rec) == 7 and lab[0] == lab[1] and lab[2] != lab[3] and lab[4] != lab[5] and lab[6] == lab[7] and lab[8] == lab[9] == lab[10]
    assert lab[6] == (0 * 16 + 11) * 16 + 13, "the anchor of the wrapped pair is its bin in layer 0"
    pf.close(); m.close()


def test_serpentine_chain_with_the_anchor_in_its_middle():
    """two combs joined along row 0: from (0, 20) down the left comb, along row 0, up the right comb to (62, 20) -- several hundred bins
    in one chain whose smallest index (0, 0) is neither end: many-hop unions and root chasing"""
    m = _make_map(64, 64)
    cells = [(x, 0) for x in range(63)]
    for x0, x1 in ((0, 30), (33, 62)):
        for k, y in enumerate(range(2, 21, 2)):
            cells += [(x, y) for x in range(x0, x1 + 1)]
            cells.append((x1 if k % 2 == 0 else x0, y - 1))
    cells += [(40, 40), (63, 63)]                          # and two bins of their own
    assert len(set(cells)) == len(cells) > 600
    rng = np.random.default_rng(5)
    order = rng.permutation(len(cells))
    poses = [_pose_in(cells[i][0], cells[i][1], 0, 1, 1) for i in order] + [_pose_in(5, 4, 0, 1, 1)] * 3
    pf = _filter(m, poses, rng.uniform(0.0, 1.0, len(poses)))
    rec, lab, _ = _check(pf, m, 1, 1, where="serpentine")
    assert len(rec) == 3 and rec["bins"].tolist() == [len(cells) - 2, 1, 1] and rec["count"][0] == len(cells) + 1
    assert (rec["anchor_bx"][0], rec["anchor_by"][0]) == (0, 0) and (rec["max_bx"][0], rec["max_by"][0]) == (62, 20)
    pf.close(); m.close()


@pytest.mark.parametrize("n_theta", [1, 2, 3, 64])
@pytest.mark.parametrize("W,H,bin_cells", [(70, 50, 7), (70, 50, 4), (64, 64, 1)])
def test_random_clouds_over_heading_counts_and_partial_bins(W, H, bin_cells, n_theta):
    m = _make_map(W, H)
    rng = np.random.default_rng(100 * n_theta + bin_cells)
    n = 1000
    poses = np.column_stack([rng.uniform(-0.1, W * RES + 0.1, n), rng.uniform(-0.1, H * RES + 0.1, n), rng.uniform(-7.0, 7.0, n)])
    poses[:300] = _blob(rng, 300, (W * RES - 0.1, H * RES - 0.1), 3.1, sigma=0.1, sigma_th=0.3)           # a blob on the last, partial bins
    pf = _filter(m, poses, rng.uniform(0.0, 1.0, n))
    rec, lab, n_out = _check(pf, m, bin_cells, n_theta, where=f"{W} x {H} / {bin_cells} / {n_theta}")
    assert n_out > 0 and len(rec) >= 1 and rec["count"].sum() == n - n_out
    if bin_cells == 7:
        assert rec["max_bx"].max() == 9 and rec["max_by"].max() == 7, "the partial last column and row of bins are used"
    pf.close(); m.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_filter_sizes_around_the_rows_of_the_sums(n):
    m = _make_map(70, 50)
    rng = np.random.default_rng(n)
    poses = np.concatenate([_blob(rng, n - n // 2, (1.0, 1.0), 0.3), _blob(rng, n // 2, (2.5, 1.5), -2.0)])
    w = 10.0 ** rng.uniform(-300, 0, n)                    # a span of 1e-300 .. 1
    pf = _filter(m, poses, w)
    rec, _, _ = _check(pf, m, 4, 8, where=f"n = {n}")
    assert rec["count"].sum() == n
    pf.close(); m.close()


def test_one_bin_for_all_and_a_mode_per_particle():
    m = _make_map(64, 64)
    rng = np.random.default_rng(8)
    n = 300
    pf = _filter(m, [_pose_in(7, 9, 3, 4, 8)] * n, rng.uniform(0, 1, n))
    rec, lab, _ = _check(pf, m, 4, 8, where="one bin")
    assert len(rec) == 1 and rec["count"][0] == n and rec["bins"][0] == 1 and (lab == (3 * 16 + 9) * 16 + 7).all()
    pf.set_poses(np.array([_pose_in(2 * (i % 32), 2 * (i // 32), 0, 1, 1) for i in range(n)], dtype=np.float32))
    rec, lab, _ = _check(pf, m, 1, 1, where="a mode per particle")
    assert len(rec) == n and (rec["count"] == 1).all() and np.array_equal(rec["strongest"], np.arange(n)) and len(set(lab)) == n
    pf.close(); m.close()


def test_particles_outside_on_every_side_and_non_finite():
    W, H = 70, 50
    m = _make_map(W, H)
    e = 0.4 * RES
    poses = np.array([[1.0, 1.0, 0.5],
                      [-RES - e, 1.0, 0.5], [W * RES + e, 1.0, 0.5], [1.0, -RES - e, 0.5], [1.0, H * RES + e, 0.5],      # off each side
                      [-e, 1.0, 0.5], [1.0, -e, 0.5], [-e, -e, 0.5],                      # in (-1, 0) cells: cell 0, inside
                      [1.0, 1.0, np.nan], [1.0, 1.0, np.inf], [1.0, 1.0, -np.inf], [1.0, 1.0, 3e38],                      # no heading bin
                      [np.nan, 1.0, 0.5], [1.0, np.nan, 0.5],                            # NaN -> cell 0, inside
                      [np.inf, 1.0, 0.5], [1.0, -np.inf, 0.5],                           # saturate: outside
                      [W * RES - e, H * RES - e, 0.5]], dtype=np.float32)
    pf = _filter(m, poses)
    for bin_cells, n_theta in ((1, 8), (7, 3)):
        rec, lab, n_out = _check(pf, m, bin_cells, n_theta, where="outside")
        assert n_out == 10 and np.array_equal(lab == GMS_MODE_NONE, np.isin(np.arange(len(poses)), [1, 2, 3, 4, 8, 9, 10, 11, 14, 15]))
    pf.close(); m.close()


def test_min_count_cap_and_omitted_outputs():
    m = _make_map(64, 64)
    rng = np.random.default_rng(12)
    sizes = (5, 40, 1, 17, 3, 80, 2)
    poses = np.concatenate([_blob(rng, s, (0.4 + 0.4 * k, 0.4 + 0.35 * k), 0.5 * k, sigma=0.01, sigma_th=0.01) for k, s in enumerate(sizes)])
    pf = _filter(m, poses, rng.uniform(0.5, 1.0, len(poses)))
    full, labels, _ = _check(pf, m, 2, 8, where="all seven")
    assert sorted(full["count"]) == sorted(sizes)
    for min_count in (2, 4, 18, 81):
        rec, lab, _ = _check(pf, m, 2, 8, min_count=min_count, where=f"min_count {min_count}")
        _same_records(rec, full[full["count"] >= min_count], "the kept records are the full table's")
        assert np.array_equal(lab, labels), "labels do not depend on min_count"
    rec, n_found, n_out = pf.modes(2, 8, cap=3)
    assert n_found == 7 and n_out == 0
    _same_records(rec, full[:3], "cap below n_found: the first three in anchor order")
    rec, n_found, n_out, lab = pf.modes(2, 8, min_count=4, cap=2, labels=True)
    assert n_found == 4 and np.array_equal(lab, labels)
    _same_records(rec, full[full["count"] >= 4][:2], "cap and min_count")
    rec, n_found, n_out, lab = pf.modes(2, 8, cap=0, labels=True)
    assert len(rec) == 0 and n_found == 7 and np.array_equal(lab, labels), "cap == 0 without records"
    q = GmsModes(2, 8, 1, 0)                               # every optional pointer NULL
    _lib.check(_lib.load().gms_pf_modes(pf._h, 0, C.byref(q), None, None, 0, None, None))
    pf.close(); m.close()


def test_a_batched_handle_and_the_device_form():
    import torch
    m = _make_map(70, 50, n_maps=2)
    rng = np.random.default_rng(21)
    n = 600
    poses = np.stack([np.concatenate([_blob(rng, 300, (0.7, 0.7), 0.0), _blob(rng, 300, (2.0, 1.5), 1.0)]),
                      np.concatenate([_blob(rng, 200, (2.8, 0.6), -3.0), _blob(rng, 400, (1.2, 2.0), 3.0, sigma=0.2)])]).astype(np.float32)
    pf = ParticleFilter(m, n)
    pf.set_poses(poses)
    pf.set_weights(rng.uniform(0, 1, (2, n)))
    for mi in (1, 0):
        want, want_lab, want_out = _expect(pf, m, 4, 8, mi=mi)
        rec, n_found, n_out, lab = pf.modes(4, 8, labels=True, cap=len(want) + 2, mi=mi)
        assert (n_found, n_out) == (len(want), want_out) and np.array_equal(lab, want_lab)
        _same_records(rec, want, f"map {mi}")
        # the device form into torch tensors: the same bytes; an odd record count and an offset label buffer
        d_rec = torch.zeros((len(want) + 2) * 112 // 8, dtype=torch.int64, device="cuda")
        d_lab = torch.full((n + 1,), 7, dtype=torch.int32, device="cuda")
        got = pf.modes(4, 8, mi=mi, records_out=d_rec, labels_out=d_lab[1:])
        assert got == (len(want), want_out)
        _same_records(d_rec.cpu().numpy().view(MODE_DTYPE)[:len(want)], want, f"map {mi}, device form")
        assert np.array_equal(d_lab.cpu().numpy().view(np.uint32)[1:], want_lab) and int(d_lab[0]) == 7
        assert pf.modes(4, 8, mi=mi, labels_out=d_lab[1:]) == (len(want), want_out), "records omitted"
    pf.close(); m.close()


def _room():
    ext, B = 12.8, 180
    tr = synth.make_trace(ext, RES, B, T=16, seed=11)
    m = GridMap(ext, ext, RES, (-ext / 2, -ext / 2), max_beams=B)
    for t in range(3):
        m.update(tr.scans[t], tr.poses[t])
    return m, tr, B, (-ext / 2, -ext / 2)


def test_weights_uniform_scored_and_hand_set():
    m, tr, B, pos = _room()
    n = 700
    pf = ParticleFilter(m, n)
    pf.set_poses(synth.make_particles(tr.poses[3], n, seed=4, sigma_xy=0.3, sigma_theta_deg=20.0))
    _check(pf, m, 4, 12, where="uniform weights of a fresh filter", pos=pos)
    pf.score(tr.scans[3])
    _check(pf, m, 4, 12, where="a scoring pass still pending", pos=pos)
    pf.normalize()
    rec, _, _ = _check(pf, m, 4, 12, where="scored and normalised", pos=pos)
    assert rec["w"].sum() > 0
    w = np.random.default_rng(2).choice([0.0, 0.25, 0.25, 1e-300, 1e-150, 1.0], n)     # zeros, ties, 300 decades
    w[:5] = np.nan
    pf.set_weights(w)
    rec, lab, _ = _check(pf, m, 4, 12, where="hand-set weights", pos=pos)
    big = np.argmax(rec["count"])
    members = np.flatnonzero(lab == lab[rec["strongest"][big]])
    assert rec["strongest"][big] == members[np.flatnonzero(w[members] == 1.0)[0]], "ties: the first in index order"
    pf.set_weights(np.full(n, np.nan))
    rec, _, _ = _check(pf, m, 4, 12, where="NaN weights", pos=pos)
    assert (rec["strongest"] == -1).all()
    pf.close(); m.close()


def test_the_call_changes_nothing_of_its_handle():
    """poses, weights and log-weights bit-equal before and after; a following normalize and resample with a fixed r01 equal those of a
    twin that never called modes -- also across a scoring pass that is still pending"""
    m, tr, B, pos = _room()
    n = 700
    twins = []
    for k in range(2):
        pf = ParticleFilter(m, n)
        pf.set_poses(synth.make_particles(tr.poses[3], n, seed=4, sigma_xy=0.1, sigma_theta_deg=5.0))
        pf.score(tr.scans[3])
        twins.append(pf)
    pf, twin = twins
    pf.modes(4, 12, labels=True)                           # the scoring pass is pending here
    assert pf.normalize() == twin.normalize()
    before = pf.get_poses(), pf.get_weights(), pf.get_log_weights()
    pf.modes(4, 12, labels=True, cap=8)
    pf.modes(1, 64, min_count=3)
    for got, want in zip((pf.get_poses(), pf.get_weights(), pf.get_log_weights()), before):
        assert got.tobytes() == want.tobytes()
    for got, want in zip(before, (twin.get_poses(), twin.get_weights(), twin.get_log_weights())):
        assert got.tobytes() == want.tobytes()
    i0, a0 = pf.resample(0.37, want_indices=True)
    pf.modes(4, 12)
    i1, a1 = twin.resample(0.37, want_indices=True)
    assert np.array_equal(i0, i1) and a0 == a1
    assert pf.get_poses().tobytes() == twin.get_poses().tobytes() and pf.get_weights().tobytes() == twin.get_weights().tobytes()
    pf.score(tr.scans[4]); twin.score(tr.scans[4])
    pf.modes(4, 12)
    assert pf.normalize() == twin.normalize() and pf.get_weights().tobytes() == twin.get_weights().tobytes()
    pf.close(); twin.close(); m.close()


def test_closed_loop_scatter_then_ten_fused_steps():
    """4096 particles scattered over the room's map, then ten fused scan steps: at each, modes equals the expectation (no convergence
    figure is asserted: nobody has measured one).  As run on an MI355X: with bins this coarse the scattered cloud is ONE mode of 4095
    or 4096 for the first four steps; from the fifth fused step on the plain-product weights of 180 beams have underflowed, the step
    leaves every pose OUTSIDE, and what is held is n_outside = 4096, no mode and GMS_MODE_NONE throughout"""
    import torch
    m, tr, B, pos = _room()
    n = 4096
    pf = ParticleFilter(m, n)
    pf.scatter(seed=5, sequence=1 << 40)
    rng = np.random.default_rng(9)
    for t in range(3, 13):
        if t > 3:
            beams = torch.from_numpy(tr.scans[t].view(np.uint8).copy()).to("cuda")
            d = tr.poses[t] - tr.poses[t - 1]
            pf.slam_update_u_dev(float(np.hypot(d[0], d[1])), float(d[2]), 77, t, beams.data_ptr(), B, rng.random(), 0.5, False)
            torch.cuda.synchronize()
        want, want_lab, want_out = _expect(pf, m, 8, 6, min_count=2, cap=16, pos=pos)
        rec, n_found, n_out, lab = pf.modes(8, 6, min_count=2, cap=16, labels=True)
        print(f"step {t}: n_found {n_found}, n_outside {n_out}, the largest counts {sorted(want['count'])[-3:]}")
        assert (n_found, n_out) == (len(want), want_out) and np.array_equal(lab, want_lab), t
        _same_records(rec, want[:16], f"step {t}")
        if t == 3:
            assert n_out == 0 and n_found >= 1 and len(set(lab)) > 1, "a scattered pose lies in a free cell of the map"
    pf.close(); m.close()


def test_refused_calls_leave_the_outputs_alone():
    import torch
    m = _make_map(70, 50)
    pf = _filter(m, [[1.0, 1.0, 0.0]] * 300)
    L = _lib.load()
    lab, rec = np.full(300, 0xABCDEF01, np.uint32), np.zeros(4, MODE_DTYPE)
    rec["count"] = -5
    nf, no = C.c_int32(-7), C.c_int32(-9)

    def call(fn, handle, mi, q, labels, records, cap):
        return fn(handle, mi, C.byref(q), labels, records, cap, C.byref(nf), C.byref(no))

    ok = GmsModes(4, 8, 1, 0)
    host = (L.gms_pf_modes, lab.ctypes.data, rec.ctypes.data)
    for mi, q, cap, records, word in ((1, ok, 4, host[2], b"map index"), (-1, ok, 4, host[2], b"map index"), (0, ok, -1, host[2], b"cap"),
                                      (0, ok, 0, host[2], b"cap"), (0, ok, 4, None, b"cap"), (0, GmsModes(4, 65, 1, 0), 4, host[2], b"n_theta"),
                                      (0, GmsModes(0, 8, 1, 0), 4, host[2], b"bin_cells"), (0, GmsModes(4, 8, 0, 0), 4, host[2], b"min_count")):
        assert call(host[0], pf._h, mi, q, host[1], records, cap) == GMS_ERR_INVALID and word in L.gms_last_error(), (mi, cap, word)
    big = _make_map(300, 300)                              # 300 x 300 x 64 bins exceed 2^22; x 46 do not
    pf_big = _filter(big, [[1.0, 1.0, 0.0]] * 300)
    assert call(host[0], pf_big._h, 0, GmsModes(1, 64, 1, 0), host[1], host[2], 4) == GMS_ERR_INVALID and b"2^22" in L.gms_last_error()
    assert (nf.value, no.value) == (-7, -9)
    want, want_lab, want_out = _expect(pf_big, big, 1, 46)
    assert call(host[0], pf_big._h, 0, GmsModes(1, 46, 1, 0), host[1], host[2], 4) == 0 and (nf.value, no.value) == (len(want), want_out) == (1, 0)
    assert np.array_equal(lab, want_lab), "the accepted field of more than 2^20 bins: every label"
    _same_records(rec[:1], want, "... and its one record")
    lab[:], nf.value, no.value = 0xABCDEF01, -7, -9
    rec[:] = np.zeros((), MODE_DTYPE)
    rec["count"] = -5
    d_lab, d_rec = torch.full((301,), 7, dtype=torch.int32, device="cuda"), torch.full((4 * 14 + 1,), 7, dtype=torch.int64, device="cuda")
    assert call(L.gms_pf_modes_dev, pf._h, 0, ok, d_lab.data_ptr() + 2, d_rec.data_ptr(), 4) == GMS_ERR_INVALID and b"aligned" in L.gms_last_error()
    assert call(L.gms_pf_modes_dev, pf._h, 0, ok, d_lab.data_ptr(), d_rec.data_ptr() + 4, 4) == GMS_ERR_INVALID and b"aligned" in L.gms_last_error()
    shard = ParticleFilter(m, 256)
    shard.set_shard(0, 512)
    s = SLAMParticleMaps(6.0, 6.0, RES, (-3.0, -3.0), num_particles=16, max_beams=64)
    for handle in (shard._h, s.pf._h):
        assert call(host[0], handle, 0, ok, host[1], host[2], 4) == GMS_ERR_STATE
        assert call(L.gms_pf_modes_dev, handle, 0, ok, d_lab.data_ptr(), d_rec.data_ptr(), 4) == GMS_ERR_STATE
    with pytest.raises(GmsError) as e:
        s.pf.modes(4, 8)
    assert e.value.code == GMS_ERR_STATE
    torch.cuda.synchronize()
    assert (lab == 0xABCDEF01).all() and (rec["count"] == -5).all() and (nf.value, no.value) == (-7, -9)
    assert bool((d_lab == 7).all()) and bool((d_rec == 7).all())
    for x in (s, shard, pf, pf_big, big, m):
        x.close()
