"""What the inputs of tests/test_gpu_scan_levels.py must contain for its comparisons to reach the scan's levels: conditions on the
cases of tests/_scan_level_cases.py and their plain expectations alone, none on the device.  A random case that misses a condition
gets another seed through the recorded turns of the cases module; no condition is loosened."""
import numpy as np
import pytest

import _scan_level_cases as sc
from _scan_level_cases import ROUND, SCAN
from gridmap_slam_robot_amd._lib import GMS_MODE_NONE

NONE = 0xFFFFFFFF


# ---- 1: frontier regions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.FRONT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frontier_logs_reach_their_blocks(shape):
    W, H = shape
    blocks = -(-sc.words_of(W, H) // SCAN)
    a = sc.front_want(shape, "a")
    assert a[1] > sc.FRT_CAP0 and a[1] == len(a[0]) and (a[0]["count"] == 1).all(), "log a: more regions than the table holds at first, one per cell"
    assert sc.front_min_size(a, 2)[1] == 0
    for name, inflate in (("a", 0), ("b", 0), ("b", 1)):
        want = sc.front_want(shape, name, inflate)
        per_block = np.bincount(sc.front_blocks(want[0], W), minlength=blocks)
        assert len(per_block) == blocks and (per_block >= (3 if name == "a" else 1)).all(), (name, inflate, per_block, "anchors in every scan block")
        if name == "b":
            small = sc.front_min_size(want, 2)
            assert 0 < small[1] < want[1], "min_size 2 leaves gaps among the kept flags"
            assert sc.front_log(shape, "b")[0, 0] < 0, "the cost field's seed cell is free"
    if blocks > 1:
        assert sc.front_cut(shape) > (sc.front_blocks(a[0], W) == 0).sum() and sc.front_cut(shape) < a[1], "the cap cuts inside block 1's regions"
    if "c" in sc.FRONT_LOGS[shape]:
        c = sc.front_want(shape, "c")
        assert c[1] == 1 and c[0]["count"][0] == 3 and (c[0]["max_x"][0], c[0]["max_y"][0]) == (W - 1, H - 1)
        assert (sc.front_blocks(c[0], W) >= 1).all(), "log c: every anchor behind block 0"
    if "d" in sc.FRONT_LOGS[shape]:
        d = sc.front_want(shape, "d")
        ys, xs = np.nonzero(d[2] != NONE)
        assert d[1] == 1 and d[0]["count"][0] == len(ys) == (sc.front_log(shape, "d") < 0).sum(), "log d: one region, every corridor cell a member"
        assert set(sc.block_of(xs, ys, W).tolist()) == {0, 1}, "its cells lie in words of both blocks"
        assert sc.front_blocks(d[0], W)[0] == 0 and (ys == H - 1).sum() > 1, "it starts in the last row, its anchor lies in block 0"


# ---- 2: pose modes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sc.MODE_FIELDS)
def test_mode_clouds_reach_every_round(W, H):
    poses, weights, wrap_anchor = sc.mode_cloud(W, H)
    n, NB, rounds = len(poses), W * H * sc.N_THETA, sc.rounds_of(W, H)
    assert 1400 <= n <= 1700 and NB <= sc.MOD_MAX_BINS
    full, labels, n_out = sc.mode_want(poses, weights, np.zeros((n, 2)), W, H, 1, sc.N_THETA)
    anchors = sc.mode_anchor_index(full, W, H)
    assert 0 < n_out <= 8 and (labels == GMS_MODE_NONE).sum() == n_out
    assert set((anchors // ROUND).tolist()) == set(range(rounds)), "anchors in every round of the top level"
    assert (anchors < SCAN).sum() >= 3 and (anchors >= NB - SCAN).sum() >= 3, "anchors in the first and the last block"
    for k in range(1, rounds):
        if k * ROUND < NB:
            assert ((anchors >= k * ROUND - SCAN) & (anchors < k * ROUND)).any() and ((anchors >= k * ROUND) & (anchors < k * ROUND + SCAN)).any(), k
    kept = full["count"] >= 6
    assert kept.sum() >= 30 and (~kept).sum() >= 30
    level = ROUND if rounds > 1 else SCAN                                      # (a field of one round has later blocks, no later round)
    first_dropped = anchors[~kept].min()
    assert (anchors[kept] // level > first_dropped // level).any(), "min_count 6: a dropped mode sorts before kept modes of a later round"
    at = np.flatnonzero(anchors == wrap_anchor)
    assert len(at) == 1 and full["anchor_bt"][at[0]] == 0 and full["bins"][at[0]] >= 8 and full["count"][at[0]] >= 24, "the wrapping mode is one mode of layer 0"
    member_bins = sc.mx.bins_of(poses[labels == wrap_anchor], (0.0, 0.0), sc.RES, W, H, 1, sc.N_THETA)
    assert (member_bins >= (sc.N_THETA - 1) * W * H).sum() >= 12, "half its particles lie in the last heading layer: the last round"


def test_the_refused_field_is_the_first_beyond_the_limit():
    W, H = sc.MODE_REFUSED
    assert W * H * sc.N_THETA > sc.MOD_MAX_BINS and sc.MODE_FIELDS[-1][0] * sc.MODE_FIELDS[-1][1] * sc.N_THETA == sc.MOD_MAX_BINS


def test_table_cloud_fills_three_blocks():
    W, H = sc.TABLE_MAP
    poses, weights = sc.table_cloud()
    full, labels, n_out = sc.mode_want(poses, weights, np.zeros((len(poses), 2)), W, H, 1, 1, cap=0)
    assert len(poses) == sc.TABLE_N and n_out == sc.TABLE_OUTSIDE
    assert len(full) == sc.TABLE_BINS > 2 * SCAN and -(-len(full) // SCAN) == 3, "n_found > 2 * GMS_SCAN: a table of three blocks"
    assert (full["bins"] == 1).all() and sorted(np.unique(full["count"]).tolist()) == [1, 2]
    twice = np.flatnonzero(full["count"] == 2)
    assert len(twice) == sc.TABLE_TWICE and set((twice // SCAN).tolist()) == {0, 1, 2}, "min_count 2: kept modes in all three blocks of the table"
    anchors = sc.mode_anchor_index(full, W, H)
    occupied = np.unique(sc.mx.bins_of(poses, (0.0, 0.0), sc.RES, W, H, 1, 1))
    occupied = occupied[occupied >= 0]
    assert np.array_equal(anchors, occupied) and anchors[SCAN] == occupied[SCAN], "the 1025th record's anchor is the 1025th occupied bin"
    once = full["count"] == 1
    assert np.array_equal(labels[full["strongest"][once]], anchors[once].astype(np.uint32)), "count 1: the strongest member is the particle itself"
    assert (full["strongest"][once] != np.flatnonzero(once)).mean() > 0.99, "... whose slot is not the mode's rank"
    # the requests of the growth test: 4 bins and 4 rows, 16384 bins and 2600 rows, 32768 bins and 2600 rows
    assert (W // 64) * (H // 64) == 4 and W * H > SCAN and 2 * W * H > -(-W * H // SCAN) * SCAN


# ---- 3: particle seeding ----------------------------------------------------------------------------------------------------------------
def test_batched_scatter_logs_reach_both_blocks():
    W, H = sc.BATCH_SHAPE
    (_, cells0, M0), (_, cells1, M1), (_, cells2, M2) = (sc.batch_want(mi) for mi in range(3))
    assert set(sc.block_of(cells0[:, 0], cells0[:, 1], W).tolist()) == {0, 1}, "map 0: draws from both blocks"
    assert (sc.block_of(cells1[:, 0], cells1[:, 1], W) == 1).all() and M1 > 20, "map 1: every draw from block 1"
    assert (cells1[:, 0] == W - 1).any() and (cells1[:, 0] < 64).any(), "... from both of its words, the ragged one too"
    assert M2 == 2 and {tuple(c) for c in cells2.tolist()} == {(0, H - 1), (W - 1, H - 1)}, "map 2: two cells, both drawn"
    assert len({M0, M1, M2}) == 3, "a total read from another map's entry shows"
    for mi, M in ((0, None), (1, M1 - int(sc.batch_logs()[1][H - 1, 0] < 0)), (2, 1)):        # (the rectangle leaves column 0 out)
        _, cells, got_M = sc.batch_want(mi, sc.BATCH_RECT)
        assert (M is None or got_M == M) and (cells[:, 0] >= 1).all() and (cells[:, 1] >= sc.BATCH_RECT[1]).all()
    assert sc.batch_want(0, sc.BATCH_RECT)[2] < M0


def test_bracket_logs_end_in_the_one_word_bracket():
    W, H = sc.BRACKET_SHAPE
    last = sc.words_of(W, H) - 1
    assert last == SCAN and last % (1 << sc.SCT_SHIFT_MIN) == 0, "word 1024 opens a staged bracket and is all of it"
    _, cells, M = sc.bracket_want("i")
    assert M == W // 2 and (cells[:, 1] == H - 1).all() and len(np.unique(cells[:, 0])) == M, "log i: every draw ends in the one-word bracket"
    _, cells, M = sc.bracket_want("ii")
    words = cells[:, 1] * sc.wpr64_of(W) + cells[:, 0] // 64
    assert set((words // SCAN).tolist()) == {0, 1} and (words == last - 1).any() and (words == last).any(), "log ii: both blocks, words 1023 and 1024"
    assert len(np.unique(words >> sc.SCT_SHIFT_MIN)) == 33, "every staged bracket is drawn from"
    _, cells, M = sc.bracket_want("full")
    words = cells[:, 1] + 0 * cells[:, 0]
    assert sc.wpr64_of(sc.FULL_SHAPE[0]) == 1 and len(np.unique(words >> sc.SCT_SHIFT_MIN)) == 32 and words.max() == SCAN - 1, "32 full brackets, the last word drawn"
