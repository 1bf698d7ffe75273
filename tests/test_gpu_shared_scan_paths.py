"""The paths of what frontier regions, pose modes and particle seeding share on the device -- the two-level exclusive scan of uint32
counts (1024 items per workgroup, the workgroups' totals walked with a carry), its form that runs to a count held on the device, its
batched form, and the "one atomic per distinct key of the wavefront" loop -- at the places the feature tests do not reach.  Everything
goes through the public calls and is compared with array_equal against the expectations the feature tests use (_frontier_expect,
_modes_expect, _scatter_expect); nothing here knows how the library scans.

Pinned elsewhere and not repeated:
  * a frontier request with more regions than the table holds at first (4096), so that the table grows and the pass over it runs twice:
    test_gpu_frontiers.py::test_many_regions_cap_and_min_size (6800 regions);
  * a wavefront whose 64 lanes share one key, and one whose 64 lanes all differ, in the particles' binning:
    test_gpu_modes.py::test_one_bin_for_all_and_a_mode_per_particle (300 particles in one bin, then in 300 bins);
  * a frontier plane word whose 64 cells are one region: test_gpu_frontiers.py::test_snake_through_all_twelve_tiles;
  * the batched scan on a plane of one block: test_gpu_scatter.py::test_batched_maps_draw_from_their_own_map_without_a_read_back."""
import numpy as np
import pytest

import _frontier_expect as fx
import _modes_expect as mx
import _scatter_expect as sx
import test_gpu_modes as tm
import test_gpu_scatter as ts
from gridmap_slam_robot_amd import GridMap, ParticleFilter

pytestmark = pytest.mark.gpu

RES = 0.05
L_FREE = -0.4054651081081643
SCAN = 1024                                            # items per block of the scan; 256 blocks made one round of the units' own top levels
NONE = 0xFFFFFFFF


# ---- the top level: more blocks than one round of it takes ---------------------------------------------------------------------------
@pytest.mark.parametrize("side,item", [(520, 262144), (1025, 1048576)])
def test_modes_over_more_bins_than_one_round_of_block_totals(side, item):
    """bin_cells = 1, n_theta = 1: a bin per cell.  520 x 520 = 270400 bins are 265 blocks, 1025 x 1025 = 1050625 are 1026: more than 256
    and more than 1024 block totals, so whichever width a round of the top level has, there is a carry.  Bins are occupied below block
    item / 1024, in it and in the last, partial block; modes are anchored on both sides of `item`, and one anchored below it has members
    behind it"""
    m = tm._make_map(side, side)
    NB = side * side
    ty, tx = divmod(item, side)
    first_of_last = (NB - 1) // SCAN * SCAN
    assert NB % SCAN != 0 and ty + 1 < side and first_of_last > item
    bins = [(x, ty) for x in range(max(0, tx - 4), tx + 5)]                   # a run across `item`: anchored below it
    bins += [(tx + 40, ty), (tx + 41, ty + 1)]                                 # anchored behind it
    bins += [(200, y) for y in range(ty - 4, ty + 2)]                          # a column from below into the block of `item`
    bins += [(x, side - 1) for x in range(side - 10, side)]                    # the last bins of the last block
    ly, lx = divmod(first_of_last, side)
    bins += [(lx, ly)] + ([(lx - 1, ly)] if lx > 0 else [])                    # the first item of the last block and the one before it
    for x0, y0 in ((10, 10), (300, 100), (side - 5, 250)):                     # and 3 x 3 blocks far below
        bins += [(x0 + dx, y0 + dy) for dy in range(3) for dx in range(3)]
    rng = np.random.default_rng(side)
    bins += [(int(x), int(y)) for x, y in zip(rng.integers(0, side, 60), rng.integers(0, ty - 10, 60))]
    bins = sorted(set(bins))
    poses = [tm._pose_in(bx, by, 0, 1, 1) for k, (bx, by) in enumerate(bins) for _ in range(20 + k % 7)]
    poses = np.array(poses)[rng.permutation(len(poses))]
    assert 2000 < len(poses) < 5000
    pf = tm._filter(m, poses, rng.uniform(0.0, 1.0, len(poses)))
    b = mx.bins_of(pf.get_poses(), (0.0, 0.0), RES, side, side, 1, 1)
    assert (b >= 0).all() and len(set(b.tolist())) == len(bins)
    blocks = set((b // SCAN).tolist())
    assert min(blocks) < 256 and item // SCAN in blocks and (NB - 1) // SCAN in blocks and b.max() == NB - 1
    rec, lab, n_out = tm._check(pf, m, 1, 1, where=f"{side} x {side} bins")
    anchors = (rec["anchor_by"].astype(np.int64) * side + rec["anchor_bx"])
    assert n_out == 0 and (anchors < item).any() and (anchors >= item).any() and len(rec) > 40
    assert ((lab < item) & (b >= item)).any(), "a mode anchored below the item has members behind it"
    tm._check(pf, m, 1, 1, min_count=24, where=f"{side} x {side} bins, min_count 24")
    pf.close(); m.close()


def _narrow_map(H, W=16):
    m = GridMap((W - 0.4) * RES, (H - 0.4) * RES, RES, (0.0, 0.0), max_beams=16)
    assert (m.W, m.H) == (W, H)
    return m


def _same_frontiers(got, want, where):
    assert got[1] == want[1], f"{where}: n_found {got[1]} != {want[1]}"
    assert got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0]), where
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), where


def test_frontiers_on_a_plane_of_more_than_262144_words():
    """A map 16 cells wide has one plane word per row; 263300 rows are 263300 words in 258 blocks, the last one partial.  Regions in the
    first rows, around word 262144 (one anchored before it with members behind it, one anchored exactly on it) and in the last rows.
    (More than 1024 blocks, a carry in a top level that takes 1024 totals per round, would need a map of 16.8 million cells here: that
    carry is held by the 1025 x 1025 bins above, through the same scan.)"""
    W, H, T = 16, 263300, 262144
    log = np.zeros((H, W))
    cells = [(3, 0), (4, 1), (10, 2)]                                          # a diagonal pair and a single cell
    cells += [(5, y) for y in range(T - 4, T + 7)]                             # a corridor across word T, anchored before it
    cells += [(9, T - 1), (13, T), (1, T + 2), (2, T + 3)]                     # singles on both sides of T, a pair behind it
    cells += [(0, H - 1), (15, H - 1), (7, H - 2), (8, H - 1)]                 # the map's last corners, a pair into the last row
    for x, y in cells:
        log[y, x] = L_FREE
    m = _narrow_map(H, W)
    m.upload_log(log)
    for min_size in (1, 2):
        want = fx.expect(log, min_size=min_size)
        assert want[1] == (9, 4)[min_size - 1]
        _same_frontiers(m.frontiers(min_size=min_size, labels=True), want, f"min_size {min_size}")
    anchors = want[0]["anchor_y"]
    assert (anchors < T).any() and (anchors >= T).any() and want[2][T + 6, 5] == (T - 4) * W + 5 and want[2][T, 13] == T * W + 13
    m.close()


# ---- the form that runs to a count held on the device --------------------------------------------------------------------------------
COUNTS = [1021, 1024, 1025]                            # inside a block and no multiple of four; exactly one block; one item into the second


@pytest.mark.parametrize("n_regions", COUNTS)
def test_frontier_region_counts_around_one_block(n_regions):
    """the scan of the kept flags runs to the number of regions.  Region i is the cell (3 (i % 67), 2 (i / 67)) of a never-observed map, every
    third one and the last with the cell to its right as well: min_size = 2 keeps those, at places only the flags' scan gives"""
    Wm, Hm = 200, 136
    log = np.zeros((Hm, Wm))
    for i in range(n_regions):
        x, y = 3 * (i % 67), 2 * (i // 67)
        log[y, x:x + (2 if i % 3 == 0 or i == n_regions - 1 else 1)] = L_FREE
    m = GridMap(9.98, 6.78, RES, (0.0, 0.0), max_beams=16)
    assert (m.W, m.H) == (Wm, Hm)
    m.upload_log(log)
    for min_size in (1, 2):
        want = fx.expect(log, min_size=min_size)
        assert want[1] == (n_regions if min_size == 1 else (n_regions + 2) // 3 + ((n_regions - 1) % 3 != 0))
        _same_frontiers(m.frontiers(min_size=min_size, labels=True, cap=2048), want, f"{n_regions} regions, min_size {min_size}")
    m.close()


@pytest.mark.parametrize("n_modes", COUNTS)
def test_mode_counts_around_one_block(n_modes):
    """the same through the number of modes: mode i is the bin (2 (i % 50), 2 (i / 50)) of a 100 x 70 map (7000 bins: seven blocks, the last
    one partial), every third one and the last with two particles; min_count = 2 keeps those"""
    m = tm._make_map(100, 70)
    poses = []
    for i in range(n_modes):
        poses += [tm._pose_in(2 * (i % 50), 2 * (i // 50), 0, 1, 1)] * (2 if i % 3 == 0 or i == n_modes - 1 else 1)
    rng = np.random.default_rng(n_modes)
    poses = np.array(poses)[rng.permutation(len(poses))]
    pf = tm._filter(m, poses, rng.uniform(0.1, 1.0, len(poses)))
    rec, n_found, n_out = pf.modes(1, 1, cap=0)
    assert (len(rec), n_found, n_out) == (0, n_modes, 0)
    rec, _, _ = tm._check(pf, m, 1, 1, min_count=2, where=f"{n_modes} modes, min_count 2")
    assert len(rec) == (n_modes + 2) // 3 + ((n_modes - 1) % 3 != 0) and (rec["count"] == 2).all()
    pf.close(); m.close()


# ---- the batched form -----------------------------------------------------------------------------------------------------------------
def test_scatter_on_three_maps_of_more_than_one_block():
    """130 x 400 cells are 400 rows of 3 words: 1200 words, two blocks per map.  Three maps with different eligible counts, the middle
    one none at all: the values' and the totals' strides and the per-map totals at once"""
    W, H, n = 130, 400, 257
    sparse = np.zeros((H, W))
    sparse[H - 50:, 64:] = L_FREE                                              # eligible cells in the second block only
    logs = np.stack([ts._random_log(W, H), np.zeros((H, W)), sparse])
    assert H * ((W + 63) // 64) > SCAN and (H - 50) * 3 > SCAN
    m = ts._make_map(W, H, n_maps=3)
    m.upload_log(logs)
    pf = ParticleFilter(m, n)
    before = pf.get_poses()
    M = pf.scatter(seed=ts.SEED, sequence=ts.SEQ, want_count=True)
    got = pf.get_poses()
    for mi in (0, 2):
        want, cells, want_M = sx.expect(logs[mi], (0.0, 0.0), RES, 0, n, ts.SEED, ts.SEQ, mi=mi)
        assert M[mi] == want_M > 0
        ts._same(got[mi], want, f"map {mi}")
    assert M[1] == 0 and M[0] != M[2] and M[2] == 50 * 66
    ts._same(got[1], before[1], "a map without a free cell: its filter untouched")
    pf.close(); m.close()


# ---- the group loop at its edges --------------------------------------------------------------------------------------------------------
def test_a_wavefront_whose_only_keyed_lane_is_the_last():
    """64 particles, the first 63 off the map and the last one on it: the only key of the wavefront sits in lane 63.  Then the same for
    the table's pass, which takes 64 bins per wavefront on a map 64 bins wide: a row of 64 occupied bins (every lane one mode), a row of
    32 bins with gaps between them (as many modes as neighbouring bins allow) and a row whose only occupied bin is the last"""
    m = tm._make_map(64, 64)
    poses = [[-1.0, 1.0, 0.0]] * 63 + [tm._pose_in(9, 7, 0, 1, 1)]
    pf = tm._filter(m, poses)
    rec, lab, n_out = tm._check(pf, m, 1, 1, where="lane 63 alone")
    assert n_out == 63 and len(rec) == 1 and (lab[:63] == NONE).all() and lab[63] == 7 * 64 + 9
    pf.close()
    bins = [(x, 3) for x in range(64)] + [(x, 6) for x in range(0, 64, 2)] + [(63, 9)]
    rng = np.random.default_rng(63)
    poses = [tm._pose_in(bx, by, 0, 1, 1) for k, (bx, by) in enumerate(bins) for _ in range(1 + k % 3)]
    pf = tm._filter(m, poses, rng.uniform(0.1, 1.0, len(poses)))
    rec, _, _ = tm._check(pf, m, 1, 1, where="rows of 64 bins")
    assert rec["bins"].tolist() == [64] + [1] * 33 and (rec["min_bx"][0], rec["max_bx"][0]) == (0, 63)
    pf.close(); m.close()
