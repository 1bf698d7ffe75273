"""The maps of the map-warp chain test (tests/_warp_cases.py), checked without a device: B is the window of A it is meant to be, and
the exhaustive search of A for B's occupied cells has a single best candidate -- the true pose -- far ahead of the second."""
import numpy as np

import _warp_cases as wc
import _warp_expect as wx
from gridmap_slam_robot_amd import locate_offsets, map_as_scan


def test_the_window_is_found_by_one_candidate_only():
    a = wc.chain_a()
    b = wc.chain_b(a)
    x0, y0 = wc.B_AT
    assert np.array_equal(wx.bits(b), wx.bits(a[y0:y0 + wc.H_B, x0:x0 + wc.W_B])), "a whole-cell shift is a slice"
    scan = map_as_scan(b, wc.POS_B, wc.RES_D)
    offsets = locate_offsets(scan, wc.N_THETA, wc.RES_D)
    i = np.flatnonzero(b.reshape(-1) > 0)
    assert np.array_equal(offsets[0], np.column_stack([i % wc.W_B - wc.B_ORIGIN[0], i // wc.W_B - wc.B_ORIGIN[1]])), "the beams are B's cells about its origin"
    score = wc.exhaustive_locate(a, offsets)
    k, y, x = np.unravel_index(np.argmax(score), score.shape)
    assert (k, x, y) == (0, x0 + wc.B_ORIGIN[0], y0 + wc.B_ORIGIN[1]) and score[k, y, x] == len(scan) and a[y, x] < 0
    assert np.sort(score.reshape(-1))[-2] < 3 * len(scan) // 4, "no other candidate reaches the test's min_score"
    tx, ty, _ = wc.chain_true_pose()
    ga, _ = wc.chain_geometry()
    assert abs(tx - (ga.px + (x + 0.5) * ga.res)) < 1e-12 and abs(ty - (ga.py + (y + 0.5) * ga.res)) < 1e-12
