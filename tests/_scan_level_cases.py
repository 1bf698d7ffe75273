"""The inputs of tests/test_scan_level_inputs.py (no device) and tests/test_gpu_scan_levels.py: logs, poses, weights and shapes that carry
the shared exclusive scan (gms_launch_scan in gms_query.hip, scan_prefix in gms_regions.h) past one block of GMS_SCAN items, past one
round of k_scan_top and past one map of its batched form.  Pure numpy; the expectations stay tests/_frontier_expect.py,
_modes_expect.py and _scatter_expect.py.  Every shape is derived from the units' constants with asserts: a changed constant fails the
derivation here and does not quietly leave a case inside one block."""
import functools
import os
import re

import numpy as np

import _frontier_expect as fx
import _modes_expect as mx
import _scatter_expect as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643


def unit_constant(name, unit, pattern=r"(\d+)"):
    """#define `name` of a unit of csrc: the first group of `pattern`, as an int"""
    src = open(os.path.join(ROOT, "gridmap_slam_robot_amd", "csrc", unit)).read()
    return int(re.search(r"#define %s %s" % (name, pattern), src).group(1))


SCAN = unit_constant("GMS_SCAN", "gms_internal.h")
FRT_CAP0 = unit_constant("FRT_CAP0", "gms_frontier.hip")
SCT_SHIFT_MIN = unit_constant("SCT_SHIFT_MIN", "gms_scatter.hip")
MOD_MAX_BINS = 1 << unit_constant("MOD_MAX_BINS", "gms_modes.hip", r"\(\(int64_t\)1 << (\d+)\)")
ROUND = SCAN * SCAN                                        # the items one round of k_scan_top covers
assert SCAN % 64 == 0 and (SCAN + 2) % 2 == 0 and (SCAN + 2) % 3 == 0, "the shapes below are made of whole rows"


def size_of(W, H):
    """GridMap's extent in metres for W x H cells at RES, as the other tests size their maps"""
    return (W - 0.4) * RES, (H - 0.4) * RES


def wpr64_of(W):
    return (W + 63) // 64


def words_of(W, H):
    return H * wpr64_of(W)


def block_of(x, y, W):
    """the scan block of the plane word that holds cell (x, y)"""
    return (np.asarray(y, dtype=np.int64) * wpr64_of(W) + np.asarray(x, dtype=np.int64) // 64) // SCAN


# ---- 1: frontier regions ----------------------------------------------------------------------------------------------------------------
# exactly one block; one word in block 1; two words per row, the block edge inside the map; three words per row, the edge inside the last row
FRONT_SHAPES = ((64, SCAN), (64, SCAN + 1), (65, (SCAN + 2) // 2), (130, (SCAN + 2) // 3))
assert [words_of(*s) for s in FRONT_SHAPES] == [SCAN, SCAN + 1, SCAN + 2, SCAN + 2]
assert all(W * H < 2 ** 17 for W, H in FRONT_SHAPES), "the flood fills of the expectation stay quick"
# the logs of front_log per shape: c needs a block 1 to put its only roots in, d a block edge inside the map
FRONT_LOGS = {FRONT_SHAPES[0]: "ab", FRONT_SHAPES[1]: "abc", FRONT_SHAPES[2]: "abcd", FRONT_SHAPES[3]: "abcd"}
# the seed of log b is W * 1000 + H + 1000000 * turn; a turn is recorded here when a condition of test_scan_level_inputs.py asks for it
FRONT_SEED_TURN = {(64, SCAN + 1): 1, (65, (SCAN + 2) // 2): 2}           # (turn 0 leaves no region anchored in the last row, which is block 1)


def serpentine_points(W, H):
    """from the middle of the last row to its last column but one (the map's corner cell has no never-observed neighbour inside the map),
    then up in three bends: the anchor, the corridor's other end, lies twelve rows up"""
    return [(W // 2, H - 1), (W - 2, H - 1), (W - 2, H - 4), (0, H - 4), (0, H - 8), (W - 1, H - 8), (W - 1, H - 12), (5, H - 12)]


@functools.lru_cache(maxsize=None)
def front_log(shape, name):
    """a: isolated free cells in never-observed space, every second column of every second row, the last row among them (so that the
          last row, all there is of block 1 on 130 x 342, holds regions): one region per cell
       b: 12 % occupied, 10 % never observed from {0.0, -0.0, NaN}, the rest free, cell (0, 0) free (the mix of test_gpu_query_shapes.py)
       c: never observed but for a free corridor of three cells that ends in the last cell of the map
       d: a one-cell-wide serpentine corridor from the last row up into block 0"""
    W, H = shape
    assert name in FRONT_LOGS[shape]
    log = np.zeros((H, W))
    if name == "a":
        log[(H - 1) % 2::2, 0::2] = L_FREE
    elif name == "b":
        rng = np.random.default_rng(W * 1000 + H + 1000000 * FRONT_SEED_TURN.get(shape, 0))
        u = rng.random((H, W))
        log = np.where(u < 0.12, L_OCC, np.where(u < 0.22, rng.choice([0.0, -0.0, np.nan], size=(H, W)), L_FREE))
        log[0, 0] = L_FREE
    elif name == "c":
        log[H - 1, W - 3:] = L_FREE
    else:
        pts = serpentine_points(W, H)
        for (xa, ya), (xb, yb) in zip(pts, pts[1:]):
            assert xa == xb or ya == yb
            log[min(ya, yb):max(ya, yb) + 1, min(xa, xb):max(xa, xb) + 1] = L_FREE
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def front_want(shape, name, inflate=0):
    """fx.expect of the log with min_size 1 and no cost field, computed once"""
    want = fx.expect(front_log(shape, name), inflate=inflate)
    for a in (want[0], want[2]):
        a.flags.writeable = False
    return want


def front_min_size(want, min_size):
    """the result for a larger min_size from the one for 1: the records with count >= min_size, their number, the same labels"""
    rec = want[0][want[0]["count"] >= min_size]
    return rec, len(rec), want[2]


def front_blocks(rec, W):
    """the scan block of every record's anchor"""
    return block_of(rec["anchor_x"], rec["anchor_y"], W)


def front_cut(shape):
    """a cap that cuts two regions into block 1 of log a"""
    a = front_want(shape, "a")
    return int((front_blocks(a[0], shape[0]) == 0).sum()) + 2


# ---- 2: pose modes ------------------------------------------------------------------------------------------------------------------------
N_THETA = 64
# (W, H) at bin_cells 1 and N_THETA headings: 1024 blocks with the last ragged; one full round; a second round of 8 blocks; MOD_MAX_BINS
MODE_FIELDS = ((129, 127), (128, 128), (129, 128), (256, 256))
MODE_REFUSED = (257, 256)
_nb = [W * H * N_THETA for W, H in MODE_FIELDS]
assert _nb[0] < ROUND and -(-_nb[0] // SCAN) == SCAN and _nb[0] % SCAN != 0
assert _nb[1] == ROUND
assert -(-_nb[2] // SCAN) == SCAN + 8
assert _nb[3] == MOD_MAX_BINS == 4 * ROUND
assert MODE_REFUSED[0] * MODE_REFUSED[1] * N_THETA > MOD_MAX_BINS == (MODE_REFUSED[0] - 1) * MODE_REFUSED[1] * N_THETA


def pose_in(bx, by, bt, bin_cells, n_theta, turns=0):
    """the pose at the centre of bin (bx, by, bt); turns: whole turns added to the heading"""
    c = (bin_cells * np.array([bx, by], dtype=np.float64) + 0.5 * bin_cells) * RES
    return [c[0], c[1], (bt + 0.5 + turns * n_theta) * (2 * np.pi / n_theta)]


def rounds_of(W, H, n_theta=N_THETA):
    return -(-W * H * n_theta // ROUND)


@functools.lru_cache(maxsize=None)
def mode_cloud(W, H):
    """(poses float32 [n][3], weights [n], the wrapping mode's anchor index) on a W x H map, bin_cells 1, N_THETA headings: forty compact
    blobs of 5 .. 60 particles in one bin or a 2 x 2 x 2 block of bins -- three anchored in the first SCAN bins, three in the last, one
    on each side of every multiple of ROUND inside the field, the others anywhere --, one mode in the heading layers N_THETA - 1 and 0,
    and the rest of about 1500 particles anywhere, five of them off the map"""
    BW, BH, T = W, H, N_THETA
    NB = BW * BH * T
    rng = np.random.default_rng(W * 1000 + H)
    split = lambda i: (i % BW, (i // BW) % BH, i // (BW * BH))
    single = [5, 300, 700, NB - 6, NB - 300, NB - 700]
    for k in range(1, rounds_of(W, H)):
        if k * ROUND < NB:
            single += [k * ROUND - 3, k * ROUND + 3]
    blobs = [(split(i), False) for i in single]
    while len(blobs) < 40:
        blobs.append(((int(rng.integers(0, BW - 1)), int(rng.integers(0, BH - 1)), int(rng.integers(0, T - 1))), bool(rng.random() < 0.7)))
    poses = []
    for k, ((bx, by, bt), wide) in enumerate(blobs):
        n = 5 if k % 8 == 0 else int(rng.integers(5, 61))                      # (fives: dropped under min_count 6)
        for j in range(n):
            d = (0, 0, 0) if j == 0 or not wide else tuple(int(v) for v in rng.integers(0, 2, 3))
            poses.append(pose_in(bx + d[0], by + d[1], bt + d[2], 1, T, turns=j % 3 - 1))
    wx, wy = BW // 2, BH // 2
    for j in range(24):                                                        # the wrapping mode: 2 x 2 bins in layers T - 1 and 0
        poses.append(pose_in(wx + (j & 1), wy + ((j >> 1) & 1), T - 1 if j & 4 else 0, 1, T))
    n_rest = max(120, 1500 - len(poses))                                       # about 1500 in all
    rest = np.column_stack([rng.uniform(0.0, W * RES, n_rest), rng.uniform(0.0, H * RES, n_rest), rng.uniform(-7.0, 7.0, n_rest)])
    rest[:5, 0] = [-0.2, W * RES + 0.2, 1.0, 1.0, np.inf]
    rest[2:4, 1] = [-0.2, H * RES + 0.2]
    rest[4, 1] = 1.0
    poses = np.concatenate([np.array(poses), rest]).astype(np.float32)
    poses = poses[rng.permutation(len(poses))]
    weights = rng.uniform(0.0, 1.0, len(poses))
    poses.flags.writeable = False
    weights.flags.writeable = False
    return poses, weights, wy * BW + wx


def mode_want(poses, weights, trig, W, H, bin_cells, n_theta, min_count=1, cap=None):
    """mx.expect on a map at (0, 0); trig [n][2]: the filter's cached cos and sin -- zeros where only the integers matter"""
    return mx.expect(poses, weights, trig, (0.0, 0.0), RES, W, H, bin_cells, n_theta, min_count, cap)


def mode_anchor_index(rec, W, H, bin_cells=1):
    """the linear bin index of every record's anchor"""
    BW, BH, _ = mx.geometry(W, H, bin_cells, 1)
    return (rec["anchor_bt"].astype(np.int64) * BH + rec["anchor_by"]) * BW + rec["anchor_bx"]


# the table past one block: a 128 x 128 map, bin_cells 1, one heading bin
TABLE_MAP = (128, 128)
TABLE_N, TABLE_BINS, TABLE_TWICE = 2600, 2 * SCAN + 52, 250
TABLE_OUTSIDE = TABLE_N - TABLE_BINS - TABLE_TWICE
assert TABLE_BINS > 2 * SCAN and TABLE_BINS <= (TABLE_MAP[0] // 2) * (TABLE_MAP[1] // 2) and TABLE_OUTSIDE >= 0 and TABLE_N > TABLE_BINS + TABLE_TWICE - 1
assert -(-TABLE_N // SCAN) == 3 and TABLE_N > SCAN, "a table of three blocks, grown from the one block a request of four bins leaves"


@functools.lru_cache(maxsize=None)
def table_cloud():
    """(poses float32 [2600][3], weights): TABLE_BINS of the (even, even) bins in random order with one particle each -- so that no two
    modes touch and a mode's rank says nothing about its particle's slot --, TABLE_TWICE of those bins with a second particle, and the
    remaining particles off the map; the slots shuffled"""
    W, H = TABLE_MAP
    rng = np.random.default_rng(2600)
    even = rng.permutation((W // 2) * (H // 2))[:TABLE_BINS]
    twice = even[rng.permutation(TABLE_BINS)[:TABLE_TWICE]]
    poses = [pose_in(2 * (b % (W // 2)), 2 * (b // (W // 2)), 0, 1, 1) for b in np.concatenate([even, twice])]
    poses = np.array(poses + [[-0.3, 1.0, 0.0]] * TABLE_OUTSIDE)
    poses[:, 2] = rng.uniform(-3.0, 3.0, len(poses))
    poses = poses[rng.permutation(len(poses))].astype(np.float32)
    weights = rng.uniform(0.0, 1.0, len(poses))
    assert len(poses) == TABLE_N
    poses.flags.writeable = False
    weights.flags.writeable = False
    return poses, weights


# ---- 3: particle seeding ----------------------------------------------------------------------------------------------------------------
SEED, SEQ = 0x123456789ABCDEF, 0xFEDCBA9876543210      # both halves of key and counter carry bits
BATCH_SHAPE = FRONT_SHAPES[2]                          # 65 x 513: two words per row, two scan blocks per map
BATCH_N = 257
BATCH_RECT = (1, 400, 64, 113)
# A draw's rank is a fixed fraction of M whatever the log is, and block 1 of map 0 -- its last row -- holds the last 0.2 % of the ranks:
# the sequence is turned until one of the 257 fractions lies that high (a recorded turn, as the seeds' are)
BATCH_SEQ_TURN = 5
BATCH_SEQ = SEQ + BATCH_SEQ_TURN
BRACKET_SHAPE, FULL_SHAPE = FRONT_SHAPES[1], FRONT_SHAPES[0]
BRACKET_N = 4096                                       # four draws per word on average: words SCAN - 1 and SCAN are both hit
assert words_of(*BATCH_SHAPE) == SCAN + 2 and wpr64_of(BATCH_SHAPE[0]) == 2
assert BATCH_RECT[0] + BATCH_RECT[2] == BATCH_SHAPE[0] and BATCH_RECT[1] + BATCH_RECT[3] == BATCH_SHAPE[1]
assert words_of(*BRACKET_SHAPE) % (1 << SCT_SHIFT_MIN) == 1 and -(-words_of(*BRACKET_SHAPE) >> SCT_SHIFT_MIN) == 33, "the last bracket is one word"
assert words_of(*FULL_SHAPE) % (1 << SCT_SHIFT_MIN) == 0 and words_of(*FULL_SHAPE) >> SCT_SHIFT_MIN == 32
# the seed of a random scatter log is 1000 * W + H + seed + 1000000 * turn (see FRONT_SEED_TURN)
SCATTER_SEED_TURN = {}


def scatter_random_log(W, H, seed=0):
    """free 60 %, occupied 15 %, the rest never observed as 0, -0.0 and NaN (the mix of test_gpu_scatter.py)"""
    rng = np.random.default_rng(1000 * W + H + seed + 1000000 * SCATTER_SEED_TURN.get((W, H, seed), 0))
    u = rng.random((H, W))
    log = np.where(u < 0.6, L_FREE, np.where(u < 0.75, L_OCC, 0.0))
    log[(u >= 0.75) & (u < 0.83)] = -0.0
    log[(u >= 0.83) & (u < 0.91)] = np.nan
    return log


@functools.lru_cache(maxsize=None)
def batch_logs():
    """[3][H][W]: a random log; one never observed in every row of block 0 (all rows but the last), its last cell -- the ragged second
    word's -- free; one never observed but for the first and the last cell of the last row"""
    W, H = BATCH_SHAPE
    logs = np.stack([scatter_random_log(W, H, seed) for seed in range(3)])
    rows0 = SCAN // wpr64_of(W)
    assert rows0 == H - 1
    logs[1, :rows0] = 0.0
    logs[1, H - 1, W - 1] = L_FREE
    logs[2] = 0.0
    logs[2, H - 1, 0] = logs[2, H - 1, W - 1] = L_FREE
    logs.flags.writeable = False
    return logs


@functools.lru_cache(maxsize=None)
def batch_want(mi, rect=None):
    """(poses, cells, M) of map mi's filter"""
    return sx.expect(batch_logs()[mi], (0.0, 0.0), RES, 0, BATCH_N, SEED, BATCH_SEQ, rect=rect, mi=mi)


@functools.lru_cache(maxsize=None)
def bracket_log(name):
    """i: 64 x 1025, free cells only in the last row, every second one; ii: 64 x 1025, random; full: 64 x 1024, random"""
    W, H = FULL_SHAPE if name == "full" else BRACKET_SHAPE
    if name == "i":
        log = np.zeros((H, W))
        log[H - 1, 0::2] = L_FREE
    else:
        log = scatter_random_log(W, H)
    log.flags.writeable = False
    return log


@functools.lru_cache(maxsize=None)
def bracket_want(name):
    return sx.expect(bracket_log(name), (0.0, 0.0), RES, 0, BRACKET_N, SEED, SEQ)
