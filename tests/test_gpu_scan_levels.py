"""The shared exclusive scan past one block, one round and one map: gms_launch_scan (k_scan_blocks, k_scan_top in gms_query.hip) and its
look-up scan_prefix (gms_regions.h) number the roots of frontier regions and pose modes, the kept records of both tables and the
eligible cells of particle seeding.  A wrong block offset or carry faults nothing: it renumbers regions, misplaces records or draws
from other cells.  So the three units run here on inputs that cross every level -- GMS_SCAN items per block, GMS_SCAN blocks per
round of the top level, several blocks per entry of the batched form -- against their plain expectations (tests/_frontier_expect.py,
_modes_expect.py, _scatter_expect.py).  Every comparison is array_equal on integers, floats and doubles as unsigned views.

The inputs come from tests/_scan_level_cases.py; tests/test_scan_level_inputs.py holds, without a device, that each of them reaches
the edge it is named for.  A failure names the first differing record, label or slot and the scan block of its prefix."""
import ctypes as C
import functools

import numpy as np
import pytest

import _frontier_expect as fx
import _scan_level_cases as sc
from _scan_level_cases import RES, SCAN
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, MODE_DTYPE, GmsModes

pytestmark = pytest.mark.gpu

FAR = 0xFFFF
MODE_INTS = ("anchor_bx", "anchor_by", "anchor_bt", "count", "bins", "strongest", "min_bx", "min_by", "max_bx", "max_by", "pad")


def _map(W, H, **kw):
    m = GridMap(*sc.size_of(W, H), RES, (0.0, 0.0), max_beams=64, **kw)
    assert (m.W, m.H) == (W, H)
    return m


# ---- 1: frontier regions across scan blocks ---------------------------------------------------------------------------------------------
def _same_regions(got, want, W, where):
    """(records, n_found, labels) against the expectation's; the first difference with the scan block of its anchor's plane word"""
    assert got[1] == want[1], f"{where}: n_found {got[1]} != {want[1]}"
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape, (where, got[0].shape, want[0].shape)
    if not np.array_equal(got[0], want[0]):
        bad = np.flatnonzero(got[0] != want[0])
        k = int(bad[0])
        raise AssertionError(f"{where}: {len(bad)} of {len(want[0])} records differ, first {k} (table block {k // SCAN}, anchor in scan block "
                             f"{int(sc.front_blocks(want[0][k:k + 1], W)[0])}): {got[0][k]} != {want[0][k]}")
    if len(got) > 2:
        assert got[2].dtype == np.uint32 and got[2].shape == want[2].shape, where
        if not np.array_equal(got[2], want[2]):
            bad = np.argwhere(got[2] != want[2])
            y, x = (int(v) for v in bad[0])
            raise AssertionError(f"{where}: {len(bad)} of {want[2].size} labels differ, first at (y, x) = ({y}, {x}) in scan block "
                                 f"{int(sc.block_of(x, y, W))}: {got[2][y, x]} != {want[2][y, x]}")


@pytest.mark.parametrize("shape", sc.FRONT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frontier_regions_across_scan_blocks(shape):
    W, H = shape
    m = _map(W, H)
    # a: one region per cell through every block, more of them than the table holds at first
    want = sc.front_want(shape, "a")
    m.upload_log(sc.front_log(shape, "a"))
    for table in ("the table as created: it grows once", "the grown table"):
        _same_regions(m.frontiers(labels=True, cap=want[1] + 1), want, W, f"{shape}, log a, {table}")
    _same_regions(m.frontiers(min_size=2, labels=True, cap=1), sc.front_min_size(want, 2), W, f"{shape}, log a, min_size 2: no flag kept")
    if sc.words_of(W, H) > SCAN:
        cut = sc.front_cut(shape)
        rec, n = m.frontiers(cap=cut)
        _same_regions((rec, n), (want[0][:cut], want[1]), W, f"{shape}, log a, cap {cut} inside block 1's regions")
    # b: a random log; c: the only roots behind every block offset; d: one region with cells in both blocks
    for name in sc.FRONT_LOGS[shape][1:]:
        m.upload_log(sc.front_log(shape, name))
        for inflate in (0, 1) if name == "b" else (0,):
            want = sc.front_want(shape, name, inflate)
            for min_size in (1, 2):
                small = sc.front_min_size(want, min_size)
                _same_regions(m.frontiers(min_size=min_size, inflate=inflate, labels=True, cap=small[1] + 1), small, W,
                              f"{shape}, log {name}, inflate {inflate}, min_size {min_size}")
        if name == "b":                                    # the goal keys go through the same region indices
            cost = m.reach([(0, 0)])
            want = fx.expect(sc.front_log(shape, "b"), cost=cost)
            assert (want[0]["goal_cost"] != FAR).sum() > want[1] // 2, "the seed at (0, 0) reaches most regions"
            _same_regions(m.frontiers(cost=cost, labels=True, cap=want[1] + 1), want, W, f"{shape}, log b, a cost field")
    m.close()


def test_frontier_regions_of_a_particles_own_map():
    """front_run is shared with the per-particle filter: one particle, its logData uploaded, the random log of 65 x 513"""
    shape = sc.FRONT_SHAPES[2]
    W, H = shape
    s = SLAMParticleMaps(*sc.size_of(W, H), RES, (0.0, 0.0), num_particles=1, max_beams=64)
    assert (s.W, s.H) == (W, H)
    s.set_map(0, log=sc.front_log(shape, "b"))
    want = sc.front_want(shape, "b")
    *got, shown = s.frontiers(0, labels=True, cap=want[1] + 1)
    assert shown == 0
    _same_regions(got, want, W, f"{shape}, log b, the particle's own map")
    s.close()


# ---- 2: pose modes -----------------------------------------------------------------------------------------------------------------------
def _same_modes(got, want, where, blocks_of=None):
    """records against the expectation's, the doubles as uint64 views; blocks_of(record) -> a text that places its anchor"""
    assert got.dtype == want.dtype == MODE_DTYPE and got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.zeros(len(want), dtype=bool)
    for name in MODE_INTS:
        bad |= (got[name] != want[name]).reshape(len(want), -1).any(axis=1)
    for name in sc.mx.SUMS:
        bad |= np.ascontiguousarray(got[name]).view(np.uint64) != np.ascontiguousarray(want[name]).view(np.uint64)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        place = f", {blocks_of(want[k:k + 1])}" if blocks_of else ""
        raise AssertionError(f"{where}: {int(bad.sum())} of {len(want)} records differ, first {k} (table block {k // SCAN}{place}): {got[k]} != {want[k]}")
    assert got.tobytes() == want.tobytes(), where


def _same_labels(got, want, where):
    assert got.dtype == np.uint32 and got.shape == want.shape, where
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{where}: {len(bad)} of {len(want)} labels differ, first slot {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _trig(m, theta):
    th = np.ascontiguousarray(theta, dtype=np.float32)
    return np.stack([m.debug_f32(1, th), m.debug_f32(2, th)], axis=-1)


def _filter(m, poses, weights):
    pf = ParticleFilter(m, len(poses))
    pf.set_poses(poses)
    pf.set_weights(weights)
    return pf


def _mode_want(pf, m, bin_cells, n_theta):
    poses = pf.get_poses()
    return sc.mode_want(poses, pf.get_weights(), _trig(m, poses[:, 2]), m.W, m.H, bin_cells, n_theta)


@pytest.mark.parametrize("W,H", sc.MODE_FIELDS)
def test_pose_modes_through_the_rounds_of_the_top_level(W, H):
    """bin fields of 1024 blocks with the last ragged, of exactly one round, of a second round of 8 blocks and of four full rounds
    (the limit; one column more is refused): anchors in every round, a mode whose bins lie in the last round under an anchor of layer 0"""
    poses, weights, _ = sc.mode_cloud(W, H)
    m = _map(W, H)
    pf = _filter(m, poses, weights)
    full, want_lab, want_out = _mode_want(pf, m, 1, sc.N_THETA)
    place = lambda r: f"anchor in block {int(sc.mode_anchor_index(r, W, H)[0]) // SCAN}, round {int(sc.mode_anchor_index(r, W, H)[0]) // sc.ROUND}"
    for min_count in (1, 6):                               # (6: the kept flags have gaps)
        want = full[full["count"] >= min_count]
        where = f"{W} x {H} x {sc.N_THETA} bins, min_count {min_count}"
        rec, n_found, n_out, lab = pf.modes(1, sc.N_THETA, min_count=min_count, labels=True, cap=len(full))
        assert (n_found, n_out) == (len(want), want_out), (where, n_found, n_out, len(want), want_out)
        _same_labels(lab, want_lab, where)
        _same_modes(rec, want, where, place)
    pf.close(); m.close()
    if W * H * sc.N_THETA == sc.MOD_MAX_BINS:
        _one_column_more_is_refused_untouched()


def _one_column_more_is_refused_untouched():
    W, H = sc.MODE_REFUSED
    m = _map(W, H)
    pf = _filter(m, np.tile(np.array(sc.pose_in(3, 3, 0, 1, sc.N_THETA), dtype=np.float32), (8, 1)), np.full(8, 0.125))
    lab, rec = np.full(8, 0xABCDEF01, np.uint32), np.zeros(4, MODE_DTYPE)
    rec["count"] = -5
    nf, no = C.c_int32(-7), C.c_int32(-9)
    L = _lib.load()
    q = GmsModes(1, sc.N_THETA, 1, 0)
    assert L.gms_pf_modes(pf._h, 0, C.byref(q), lab.ctypes.data, rec.ctypes.data, 4, C.byref(nf), C.byref(no)) == GMS_ERR_INVALID
    assert b"2^22" in L.gms_last_error()
    assert (lab == 0xABCDEF01).all() and (rec["count"] == -5).all() and (nf.value, no.value) == (-7, -9)
    pf.close(); m.close()


def _table_filter():
    m = _map(*sc.TABLE_MAP)
    return m, _filter(m, *sc.table_cloud())


@functools.lru_cache(maxsize=None)
def _table_want():
    """the expectation of the table cloud under bin_cells 1 and one heading bin, every record's sums: made once, left unchanged (the
    cached trig it reads depends on the headings alone)"""
    m, pf = _table_filter()
    want = _mode_want(pf, m, 1, 1)
    for a in want[:2]:
        a.flags.writeable = False
    pf.close(); m.close()
    return want


def _table_place(r):
    return f"anchor bin {int(sc.mode_anchor_index(r, *sc.TABLE_MAP)[0])}"


def test_a_mode_table_past_one_scan_block():
    """2100 modes in three blocks of the table: the second scan (the kept flags, its length from device memory), the look-up of
    k_modes_emit and caps on both sides of a block edge.  strongest is a slot, not a rank: the slots are shuffled"""
    import torch
    full, want_lab, want_out = _table_want()
    m, pf = _table_filter()
    assert len(full) > 2 * SCAN
    for min_count in (1, 2):
        want = full[full["count"] >= min_count]
        for cap in (len(full), SCAN, SCAN + 1, 3):
            where = f"{len(full)} modes, min_count {min_count}, cap {cap}"
            rec, n_found, n_out, lab = pf.modes(1, 1, min_count=min_count, labels=True, cap=cap)
            assert (n_found, n_out) == (len(want), want_out), (where, n_found, n_out)
            _same_labels(lab, want_lab, where)
            _same_modes(rec, want[:cap], where, _table_place)
    cap = SCAN + 1
    d_rec = torch.zeros(cap * MODE_DTYPE.itemsize // 8, dtype=torch.int64, device="cuda")
    d_lab = torch.full((pf.n,), 7, dtype=torch.int32, device="cuda")
    assert pf.modes(1, 1, records_out=d_rec, labels_out=d_lab) == (len(full), want_out)
    _same_modes(d_rec.cpu().numpy().view(MODE_DTYPE), full[:cap], f"the device form, cap {cap}", _table_place)
    _same_labels(d_lab.cpu().numpy().view(np.uint32), want_lab, "the device form")
    pf.close(); m.close()


def test_the_mode_table_grows_between_requests_on_one_filter():
    """4 rows, then 2600 (the table grows from one block to three), 4 again, then twice the bins (the bins grow, the table does not)"""
    table_want = _table_want()
    m, pf = _table_filter()                                # a filter of its own: its buffers start empty
    results = []
    for bin_cells, n_theta in ((64, 1), (1, 1), (64, 1), (1, 2)):
        want, want_lab, want_out = table_want if (bin_cells, n_theta) == (1, 1) else _mode_want(pf, m, bin_cells, n_theta)
        where = f"bin_cells {bin_cells}, n_theta {n_theta}"
        rec, n_found, n_out, lab = pf.modes(bin_cells, n_theta, labels=True, cap=len(want))
        assert (n_found, n_out) == (len(want), want_out), (where, n_found, n_out, len(want), want_out)
        _same_labels(lab, want_lab, where)
        _same_modes(rec, want, where)
        results.append((rec.tobytes(), lab.tobytes(), len(want)))
    assert results[0][2] == 1 and results[1][2] > 2 * SCAN and results[3][2] > 2 * SCAN
    assert results[2][:2] == results[0][:2], "the small request after the large one: byte for byte the first"
    pf.close(); m.close()


# ---- 3: particle seeding ---------------------------------------------------------------------------------------------------------------
def _same_poses(got, want, cells, W, where):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, where
    bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=1))
    if len(bad):
        k = int(bad[0])
        word = int(cells[k, 1]) * sc.wpr64_of(W) + int(cells[k, 0]) // 64
        raise AssertionError(f"{where}: {len(bad)} of {len(want)} slots differ, first {k} (its cell {cells[k].tolist()} in word {word}, scan block "
                             f"{word // SCAN}): {got[k]} != {want[k]}")


def test_batched_scatter_with_two_scan_blocks_per_map():
    W, H = sc.BATCH_SHAPE
    logs = sc.batch_logs()
    m = _map(W, H, n_maps=len(logs))
    m.upload_log(logs)
    pf = ParticleFilter(m, sc.BATCH_N)
    for rect in (None, sc.BATCH_RECT):                     # the rectangle: another table of the same shapes on the same handle
        M = pf.scatter(rect=rect, seed=sc.SEED, sequence=sc.BATCH_SEQ, want_count=True)
        got = pf.get_poses()
        for mi in range(len(logs)):
            want, cells, want_M = sc.batch_want(mi, rect)
            assert M[mi] == want_M, f"map {mi}, rect {rect}: M {M[mi]} != {want_M}"
            _same_poses(got[mi], want, cells, W, f"map {mi}, rect {rect}")
    w = pf.get_weights()
    assert np.array_equal(w.view(np.uint64), np.full(w.shape, 1.0 / sc.BATCH_N).view(np.uint64))
    pf.close(); m.close()


def test_scatter_with_a_last_bracket_of_one_word(monkeypatch):
    """64 x 1025: 33 staged entries, the last bracket word 1024 alone (hi - lo == 1: no search in memory); 64 x 1024: 32 full brackets.
    GMS_SCATTER_SHIFT=9 stages every 512th word: three entries, the last bracket again one word.  One test: log i (every prefix before
    its one word is 0) and the one-block map cannot tell a wrong block offset by themselves, log ii on 64 x 1025 does"""
    for name, shift in (("i", None), ("ii", None), ("ii", "9"), ("full", None)):
        W, H = sc.FULL_SHAPE if name == "full" else sc.BRACKET_SHAPE
        monkeypatch.delenv("GMS_SCATTER_SHIFT", raising=False)
        if shift:
            monkeypatch.setenv("GMS_SCATTER_SHIFT", shift)                     # read when the handle is created
        m = _map(W, H)
        monkeypatch.delenv("GMS_SCATTER_SHIFT", raising=False)
        m.upload_log(sc.bracket_log(name))
        want, cells, want_M = sc.bracket_want(name)
        pf = ParticleFilter(m, sc.BRACKET_N)
        assert pf.scatter(seed=sc.SEED, sequence=sc.SEQ, want_count=True) == want_M, (name, shift)
        _same_poses(pf.get_poses(), want, cells, W, f"{W} x {H}, log {name}, GMS_SCATTER_SHIFT={shift}")
        pf.close(); m.close()
