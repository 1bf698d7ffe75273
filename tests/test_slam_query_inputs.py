"""What the cases of tests/_slam_query_cases.py must contain for tests/test_gpu_slam_query_shapes.py to mean something: conditions on the
builders and the oracle alone, no device.  Where a condition cannot hold on a shape by construction, the reason stands beside it."""
import numpy as np
import pytest

import _slam_query_cases as sq
from _slam_query_cases import N, RAGGED, SHAPES, SLOT_LOGS, expect_of, poses_of, same_bytes
import test_gpu_query_shapes as qs
from test_gpu_query_shapes import RES, _small_cap, log_of

BIG = [s for s in SHAPES if s[0] * s[1] >= 64]
ids = lambda s: f"{s[0]}x{s[1]}"


def _answers(shape, k):
    e, pose = expect_of(shape, SLOT_LOGS[k]), poses_of(shape)[k]
    return {(q, p): e.answer(q, p, pose, sq.warp_dst_log(shape)) for q, p in sq.requests(shape)}


def test_the_shapes_reach_the_code_word_edges():
    assert SHAPES[:13] == qs.SHAPES and len(qs.SHAPES) == 13
    assert RAGGED == [s for s in SHAPES if s[0] * s[1] % 16 != 0]
    assert set(RAGGED) >= {(63, 65), (129, 65), (31, 3), (33, 2), (1, 70), (1, 1)}
    assert len({W % 16 for W, _ in SHAPES}) >= 5, "a row starts at five code offsets or more"
    for group in (sq.EAGER_SHAPES, sq.WALK_MEM_SHAPES, sq.GEN1_SHAPES, [sq.BATCH_SHAPE]):
        assert set(group) <= set(SHAPES)
    assert len(set(SLOT_LOGS)) == N == 5 and len(sq.requests((63, 65))) == len(set(sq.requests((63, 65))))
    assert {q for q, _ in sq.requests((63, 65))} == set(sq.QUERIES)


def test_the_plane_limit_shapes():
    """slam_code_words (gms_slam_kernels.hip): ceil(cells / 16) words and one spare, rounded up to four; kept up to 24 KiB"""
    words = lambda s: ((s[0] * s[1] + 15) // 16 + 1 + 3) & ~3
    assert [4 * words(s) for s in sq.LIMIT_SHAPES] == [24576, 24592, 24656]
    assert sq.LIMIT_SHAPES[0][0] * sq.LIMIT_SHAPES[0][1] % 16 != 0 and sq.LIMIT_SHAPES[0][0] % 16 != 0
    for shape in sq.LIMIT_SHAPES:
        x0, y0, w, h = sq.limit_rect(shape)
        assert (x0 + w, y0 + h) == shape and (w, h) == (70, 40)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_poses(shape):
    W, H = shape
    p = poses_of(shape).astype(np.float64)
    cell = np.floor(p[:, :2] / np.float64(np.float32(RES))).astype(int)
    assert cell[0].tolist() == [0, 0] and cell[4].tolist() == [W - 1, H - 1], "corner cells"
    assert np.allclose(p[0, :2] / RES, [0.5, 0.5]) and np.allclose(p[4, :2] / RES, [W - 0.5, H - 0.5]), "... at their centres"
    assert p[1, 0] < 0 and -2 * RES < p[1, 0], "one just off the map"
    assert len({tuple(q) for q in p.tolist()}) == N or W * H == 1
    for k in (2, 3):                                                           # (the walks start in floor(pose / RES + 0.5))
        x, y = np.floor(p[k, :2] / np.float64(np.float32(RES)) + 0.5).astype(int)
        assert log_of(shape, SLOT_LOGS[k])[y, x] < 0, "the random slots' poses stand in a free cell of their own log"


@pytest.mark.parametrize("shape", BIG, ids=ids)
def test_the_slots_answer_differently(shape):
    """a stray read across a slot boundary shows: per query the expectations of slots 2, 3 and 4 differ pairwise (every query in at
    least one of its parameter sets; the unpacked whole-map view, the cast, the whole-map clearance fields and the uncapped reach
    fields one by one), and slot 0 differs from slot 1 wherever not_free is set"""
    ans = [_answers(shape, k) for k in range(N)]
    for a, b in ((2, 3), (2, 4), (3, 4)):
        for q in sq.QUERIES:
            keys = [key for key in ans[a] if key[0] == q]
            assert any(not same_bytes(ans[a][key], ans[b][key]) for key in keys), (shape, q, a, b)
        for key in (("view", (None, 1, False)), ("cast", ()), ("clearance", (None, 255, False)), ("clearance", (None, 255, True)),
                    ("reach", (0, True, 0xFFFE)), ("reach", (0, False, 0xFFFE)), ("frontiers", (1,)), ("gain", (255,))):
            assert not same_bytes(ans[a][key], ans[b][key]), (shape, key, a, b)
    for (q, p), got in ans[0].items():
        if q in sq.USES_NOT_FREE and sq.USES_NOT_FREE[q](p):
            assert not same_bytes(got, ans[1][(q, p)]), (shape, q, p, "free against unknown")


@pytest.mark.parametrize("shape", BIG, ids=ids)
def test_the_random_slots_contain_every_case(shape):
    W, H = shape
    for k in (2, 3):
        ans = _answers(shape, k)
        step = ans[("cast", ())][0]["step"]
        assert (step >= 0).any() and (step < 0).any(), (shape, k, "a probe that hits and one that misses")
        assert ans[("frontiers", (1,))][1][0] >= 1, (shape, k, "a frontier region")
        assert any(int(ans[("locate", p)][0]["score"].max()) > 0 for p in ((0, False), (1, True))), (shape, k, "a locate record")
        if W >= 3 and H >= 3:
            # (on a thin map the seed set holds the first cell of every run of free cells: no cost exceeds five times the longest run,
            # and no run of these logs is as long as the cap -- tests/test_gpu_query_shapes.py asserts its cap on the same shapes)
            cuts = [((ans[("reach", (i, nf, _small_cap(shape)))][0] == 0xFFFF) & (ans[("reach", (i, nf, 0xFFFE))][0] != 0xFFFF)).any()
                    for i in (0, 2) for nf in (True, False)]
            assert any(cuts), (shape, k, "a cell the small cap cuts")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] % 16 != 0 and s[0] * s[1] >= 64 and s[1] > 1], ids=ids)
def test_walks_and_obstacles_in_code_words_that_two_rows_share(shape):
    """(a map of one row has no second row to share a word with)"""
    shared = sq.shared_word_cells(shape)
    assert shared.any()
    assert any((sq.cast_walk_cells(shape, k) & shared).any() for k in (2, 3)), (shape, "a cast walk")
    assert any(((log_of(shape, SLOT_LOGS[k]) > 0) & shared).any() for k in (2, 3)), (shape, "a clearance obstacle")


@pytest.mark.parametrize("shape", [s for s in RAGGED if s[0] * s[1] > 8], ids=ids)
def test_an_occupied_cell_in_the_ragged_last_code_word(shape):
    """(the one cell of 1 x 1 is the seed cell, free in every random log)"""
    last = sq.last_word_cells(shape)
    assert 0 < last.sum() < 16
    assert any(((log_of(shape, name) > 0) & last).any() for name in SLOT_LOGS), shape


@pytest.mark.parametrize("shape", sq.GEN1_SHAPES, ids=ids)
def test_the_resampling_draw_moves_maps(shape):
    r01, idx, logs = sq.resampling_draw(shape)
    assert not np.array_equal(idx, np.arange(N)), "not the identity"
    moved = [k for k in range(N) if idx[k] != k and logs[k].tobytes() != logs[idx[k]].tobytes()]
    assert moved, "a slot receives a map that differs from its own"
    w = sq.oracle_after_update(shape).weights
    assert len(np.unique(w)) > 1, "the update made the weights differ"
    assert any(logs[k].tobytes() != np.ascontiguousarray(log_of(shape, SLOT_LOGS[k])).tobytes() for k in range(N)), "the update wrote a map"


def test_the_batched_slots_differ_and_one_filter_draws():
    for i in range(sq.BATCH_N):
        assert sq.BATCH_LOGS[0][i] != sq.BATCH_LOGS[1][i], "slot f * 3 + i against slot i"
    assert sq.batch_poses().shape == (2, 3, 3)
    neff, frac = sq.batch_draw()
    # (the device's Neff agrees with the oracle's to 1e-11, tests/test_gpu_slam_particle_maps.py: a gap of 1e-6 cannot close)
    assert abs(neff[0] - neff[1]) > 1e-6 * neff.max(), "the filters' Neff differ"
    assert int((neff < frac * sq.BATCH_N).sum()) == 1, "exactly one filter meets the fraction"


def test_nobody_writes_to_what_a_builder_returns():
    shape = (31, 3)
    arrays = [poses_of(shape), sq.batch_poses(), sq.FAN, sq.OFFSETS, sq.SCAN, sq.SCAN2, sq.arcs_of(shape), log_of(shape, "second"), sq.batch_draw()[0]]
    arrays += list(sq.resampling_draw(shape)[1:])
    for k in range(N):
        for res in _answers(shape, k).values():
            arrays += list(res)
    assert not any(a.flags.writeable for a in arrays)
