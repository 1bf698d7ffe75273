"""What the cases of tests/_slam_align_edge_cases.py must contain, asserted with the oracle and the restatement alone (no device): a
case that does not reach the code its name claims would let tests/test_gpu_slam_align_edges.py pass on an empty comparison."""
import numpy as np
import pytest

import _align_expect as ax
import _slam_align_edge_cases as ec
from test_gpu_slam_align import _expect


def _used_and_moved(case, call=0, moves=True):
    """at least half of the particles use a beam at the start pose; at least one pose moves"""
    poses, rec = case.want[call]
    assert 2 * int((rec["n_used0"] > 0).sum()) >= case.N, (case.name, rec["n_used0"])
    if moves:
        assert (ax.bits(poses) != ax.bits(case.calls[call].P)).any(), f"{case.name}: no pose moves"


def test_the_visitor_changes_no_value():
    c = ec.tap_case("fifteen_taps")
    call = c.calls[0]
    off = _expect(c.g, call.z, call.P, call.prm, logs=c.logs)
    ax.same((c.want[0][0], c.want[0][1]), off, "visitor on against off")
    assert len(c.visits[0]) >= sum(int(n) for n in off[1]["n_used0"])


# ---- blur widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.TAP_CASES)
def test_tap_cases(name):
    c = ec.tap_case(name)
    assert (c.g.W, c.g.H) == (80, 80) and c.ntaps == ec.TAP_WIDTHS[name] == len(ec.TAPS[name])
    assert c.plain == (not ec.is_literal(name)), f"{name}: the kernel selects the {'plain' if c.plain else 'literal'} form"
    assert c.form(72) == "planes" and c.form(72, forced_memory=True) == "memory"
    if ec.is_literal(name):
        assert any(0.0 < abs(t) < 2.0 ** -900 for t in c.kernel) or any(t < 0.0 for t in c.kernel)
    if name == "fifteen_taps_zero_ends":
        assert c.kernel[0] == 0.0 and c.kernel[-1] == 0.0 and not np.signbit(c.kernel[0]) and not np.signbit(c.kernel[-1])
    _used_and_moved(c, moves=name not in ec.CONSTANT_FIELD)
    if name in ec.CONSTANT_FIELD:                   # said aloud: this case compares a field that is 0.0 everywhere, and a step of 0.0
        assert all((f == 0.0).all() for f in c.fields()) and (c.want[0][1]["status"] == 1).all()
    else:
        assert any(np.unique(f).size > 2 for f in c.fields())
    w = ec.windows(c)
    phases = set((w[:, 0] & 15).tolist())
    assert phases == set(range(16)), f"{name}: phases {sorted(phases)}"
    assert (0, 0) in map(tuple, ec.end_cells(c)) and (78, 78) in map(tuple, ec.end_cells(c)), "the corner beams are used"
    words = ec.words_read(c)
    assert ec.last_word(80 * 80) == 400 and 400 in words, f"{name}: no window reaches the spare word"
    if c.plain and c.kh > 0:                       # (one tap: a window is its own cell, c0 >= 0; the literal form starts at column 0)
        assert (w[:, 0] < 0).any() and -1 in words, f"{name}: no window starts in front of the plane"
    if not c.plain:
        assert (w[:, 0] >= 0).all()
    if c.ntaps == 15:                               # 30 bits of the 34 that a shift by 30 leaves
        assert ((w[:, 0] & 15) == 15).any()
        rows = w[:, 2] - (w[:, 5] - c.kh)           # the lane r of a group that forms the row's sums: all sixteen
        assert set(rows.tolist()) == set(range(16))


# ---- narrower and lower than the blur ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kernel", ec.NARROW_CASES)
def test_narrow_cases(shape, kernel):
    c = ec.narrow_case(shape, kernel)
    assert c.ntaps == 15 and c.kh == 7 and c.plain == (not ec.is_literal(kernel)) and c.form(48) == "planes"
    _used_and_moved(c)
    w = ec.windows(c)
    W, H = c.g.W, c.g.H
    both_columns = (w[:, 3] > 0) & (w[:, 4] < 2 * c.kh)
    j0 = ec.end_cells(c)[:, 1]
    both_rows = (j0 - c.kh < 0) & (j0 + c.kh + 1 > H - 1)
    if W < 15:
        assert both_columns.any(), f"{c.name}: no window is clipped on both sides"
    if H < 16:
        assert both_rows.any(), f"{c.name}: no end point has rows outside the map above and below"
    assert both_columns.any() or both_rows.any()
    if shape == "9x9":
        assert both_columns.any() and both_rows.any()


def test_the_narrow_shapes_cover_both_clips():
    assert {s for s, _ in ec.NARROW_CASES} >= {"9x33", "33x9"}
    assert {k for _, k in ec.NARROW_CASES} == {"fifteen_taps", "fifteen_taps_literal_tiny"}


# ---- uploads -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,stage", ec.UPLOAD_CASES)
def test_upload_cases(shape, stage):
    c = ec.upload_case(shape, stage)
    W, H = c.g.W, c.g.H
    cells = W * H
    assert (cells % 16 != 0) == (shape == "51x67") and c.plain and c.form(72) == "planes" and c.form(72, eager=True) == "memory"
    up = c.steps[0][1]
    for log in up:
        b = np.asarray(log).reshape(-1).view(np.uint64)
        for v in ec.SPECIALS:
            n = int(np.isnan(np.asarray(log)).sum()) if v != v else int((b == np.float64(v).view(np.uint64)).sum())
            assert n == ec.N_SPECIAL, (c.name, v, n)
        frac = [float((np.asarray(log) == ec.L_OCC).mean()), float((np.asarray(log) == ec.L_FREE).mean())]
        assert 0.03 < frac[0] < 0.07 and 0.38 < frac[1] < 0.50, frac
    assert any(not np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)) for a, b in zip(up, up[1:])), "every particle its own logData"
    _used_and_moved(c, 0, moves=stage != "reset")      # (after reset() the field is constant where the scan ends: the one beam below moves)
    assert (ax.bits(c.want[1][0]) != ax.bits(c.calls[1].P)).any(), f"{c.name}: no one-beam pose moves"
    # the one-beam call: some poses use their beam, some do not; the corner cells and with them word -1 and the spare word
    n0 = c.want[1][1]["n_used0"]
    assert 0 < int((n0 == 1).sum()) < c.N and (c.want[1][1]["status"][n0 == 0] == 2).all()
    corners = set(map(tuple, ec.end_cells(c, 1)))
    assert {(0, 0), (W - 2, 0), (0, H - 2), (W - 2, H - 2)} <= corners, corners
    words = ec.words_read(c, 1)
    assert -1 in words and ec.last_word(cells) in words, words
    if stage == "uploaded":
        for i in range(c.N):
            assert all(n > 0 for n in ec.special_cells_in_reach(c, i)), (c.name, i, ec.special_cells_in_reach(c, i))
    if stage == "resampled":
        idx = c.steps[2][2]
        assert len(set(idx.tolist())) < c.N and (idx != np.arange(c.N)).any(), "the draw copies some particle twice"
        for i in range(c.N):
            assert np.array_equal(np.asarray(c.logs[i]).view(np.uint64), np.asarray(up[idx[i]]).view(np.uint64))
    if stage == "reset":
        inner = np.zeros((H, W), bool)
        inner[c.kh:H - c.kh, c.kh:W - c.kh] = True
        f = c.fields()[0].reshape(H, W)
        assert (f[inner] == f[H // 2, W // 2]).all() and (f[~inner] < f[H // 2, W // 2]).all()


# ---- stopping rules --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.STOP_CASES)
def test_stop_cases(name):
    c = ec.stop_case(name)
    poses, rec = c.want[0]
    prm = c.calls[0].prm
    assert c.N == 24 and (rec["n_used0"] > 0).all()
    status, done = rec["status"], rec["iters_done"]
    if name == "converged":
        assert (status == 1).all() and (done == 1).all()
    elif name == "singular_on_reset":
        assert (status == 3).all() and (done == 0).all() and np.array_equal(ax.bits(poses), ax.bits(c.calls[0].P))
    elif name.startswith("det_min"):
        det, _, _ = ec.first_step(c, 0, prm)
        assert (status[0], done[0]) == ((0, 1) if name == "det_min_below" else (3, 0)), (name, det, prm["det_min"])
        assert (abs(det) > prm["det_min"]) == (name == "det_min_below")
        assert set(status.tolist()) == {0, 3}, "particles on both sides of det_min in one launch"
    elif name == "clamps":
        clamped = 0
        for i in range(c.N):
            _, d, _ = ec.first_step(c, i, prm)
            clamped += abs(d[0]) > ec.CLAMP_T or abs(d[1]) > ec.CLAMP_T or abs(d[2]) > ec.CLAMP_R
        assert 2 * clamped >= c.N, f"{clamped} of {c.N} first steps are clamped"
    elif name == "iters_64":
        assert prm["iters"] == 64 and (done == 64).any() and (status[done == 64] == 0).all()
    elif name == "mixed_stops":
        assert len(set(done.tolist())) >= 3, sorted(set(done.tolist()))
        assert {0, 1} <= set(status.tolist())
    if name != "singular_on_reset":
        _used_and_moved(c, moves=not name.startswith("det_min_a"))


def test_chain_case():
    c = ec.chain_case()
    rec = c.want[0][1]
    stopped = rec["status"] != 0
    assert c.calls[0].prm["iters"] == ec.CHAIN_K and stopped.any() and not stopped.all()


# ---- beams ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", ec.BEAM_COUNTS)
def test_beam_count_cases(B):
    c = ec.beam_count_case(B)
    assert len(c.calls[0].z) == B
    _used_and_moved(c)
    if B == 17:                                    # the second pass of the field's values serves one beam: it is used somewhere
        assert any(a[2] == 16 for a in c.visits[0])


def test_non_finite_case():
    c, clean = ec.non_finite_case(), ec.clean_case()
    z, zc = c.calls[0].z, clean.calls[0].z
    bad = ec.bad_beam_indices(zc)
    assert len(bad) == 8 == len(set(bad.tolist())) and (z["hit"][bad] == 1).all()
    assert (~(np.isfinite(z["local_x"][bad]) & np.isfinite(z["local_y"][bad]))).all()
    for kind in (np.isnan, np.isposinf, np.isneginf):
        assert kind(z["local_x"][bad]).any() and kind(z["local_y"][bad]).any()
    rest = np.setdiff1d(np.arange(len(z)), bad)
    assert z[rest].tobytes() == zc[rest].tobytes()
    _used_and_moved(c)
    lost = np.array([sum(1 for a in clean.visits[0] if a[0] == i and a[1] == 0 and a[2] in bad) for i in range(c.N)])
    assert (lost > 0).all() and np.array_equal(c.want[0][1]["n_used0"], clean.want[0][1]["n_used0"] - lost)
    assert not any(a[2] in bad for a in c.visits[0]) and np.isfinite(c.want[0][0]).all()


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------
def test_gate_cases():
    c = ec.gate_case()
    assert 4 * ec.code_words(314 * 313) == 24576 and 4 * ec.code_words(314 * 314) == 24656
    assert ec.planes_kept(314, 313, c.ntaps) and not ec.planes_kept(314, 314, c.ntaps)
    assert [len(k.z) for k in c.calls] == list(ec.GATE_ORDER) and max(ec.GATE_ORDER) <= c.max_beams
    assert tuple(c.form(B) for B in ec.GATE_ORDER) == ec.GATE_WANT
    # 2816 beams sit exactly on the gate, one more beam pads to 2824 and falls behind it; without the 4 KiB both would pass
    assert 48 * 2816 + 24576 + 4096 == ec.LDS_PER_CU and 48 * 2824 + 24576 <= ec.LDS_PER_CU < 48 * 2824 + 24576 + 4096
    for k in range(len(c.calls)):
        _used_and_moved(c, k)
    n = ec.no_planes_case()
    assert n.form(72) == "memory" and (n.g.W, n.g.H) == (314, 314)
    _used_and_moved(n)


# ---- far origins -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.FAR_ORIGINS))
def test_far_cases(name):
    c = ec.far_case(name)
    assert (c.g.W, c.g.H) == (80, 80) and tuple(np.float32(c.origin)) == tuple(np.float32(c.g.pos))
    assert min(abs(v) for v in c.origin) >= 1000.0
    _used_and_moved(c)
    assert (np.abs(c.calls[0].P[:, :2] - np.float32(c.origin)) < 4.0).all(), "the start poses moved with the map"
    cells = set(map(tuple, ec.end_cells(c)))
    assert (0, 0) in cells and (78, 78) in cells
    words = ec.words_read(c)
    assert -1 in words and 400 in words
