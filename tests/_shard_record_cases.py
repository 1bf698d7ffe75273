"""The inputs of tests/test_gpu_slam_shard_records.py: the RECORDS a sharded gms_slam moves in resample() -- a particle's logData
(`cells` doubles) followed by its two class planes (`code_words` doubles) -- at the edges of the two kernels that move them
(k_slam_export_records, k_slam_shard_gather: 256 lanes, chunks of 2048 doubles, the `e < cells` split inside a chunk) and of the plans
that drive them.  Builders only, numpy, no device code; what they must contain is asserted in tests/test_shard_record_inputs.py, so that
a green device test cannot hide an empty comparison.  Nobody writes to what a builder returns."""
import functools

import numpy as np

from _slam_align_edge_cases import code_words

RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
N = 256                                                    # GMS_BLOCK: the smallest block gms_slam_create_shard takes
CHUNK = 2048                                               # doubles of a record per workgroup of both kernels (256 lanes x 8)
SPECIALS = (float("nan"), -0.0, 5e-324)

# (W, H): cells, code_words, record doubles -- and the edge each shape is there for
SHAPES = {
    (40, 5): (200, 16, 216),                               # a record under one 256-lane pass
    (41, 41): (1681, 108, 1789),                           # odd cell count (the planes start at an odd double); rows straddle code words; one partial chunk
    (52, 37): (1924, 124, 2048),                           # exactly one chunk
    (55, 35): (1925, 124, 2049),                           # one chunk and one double; odd cells
    (120, 120): (14400, 904, 15304),                       # the shape tests/test_gpu_slam_sharded.py uses; the last chunk partial
    (390, 252): (98280, 6144, 104424),                     # the plane limit: 24 576 bytes exactly
}
OVER_THE_LIMIT = (384, 256)                                # 24 592 bytes a plane: not kept, a shard of it is refused (tests/test_gpu_slam_no_planes.py)
MASKS = ("none", "all", "third", "self")


def size_of(shape):
    """metres that give exactly W x H cells at RES (as tests/test_gpu_query_shapes.py builds its sizes)"""
    return (shape[0] - 0.4) * RES, (shape[1] - 0.4) * RES


def record_doubles(shape):
    cells = shape[0] * shape[1]
    return cells + code_words(cells)


# ---- logs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def logs_of(shape, n=N):
    """float64 [n][cells]: a seeded field of free, occupied and unknown cells with NaN, -0.0 and 5e-324 among them, made different for
    every particle in a way that names the particle: cell i % cells holds float(i + 1), and the map's LAST cell -- in the ragged last
    code word where cells % 16 != 0 -- is occupied for odd i and free for even i"""
    W, H = shape
    cells = W * H
    rng = np.random.default_rng(7000 * W + H)
    u = rng.random(cells)
    base = np.where(u < 0.12, L_OCC, np.where(u < 0.22, rng.choice([0.0, -0.0, np.nan, 5e-324], size=cells), L_FREE))
    base[cells // 2: cells // 2 + 3] = SPECIALS            # (present whatever the choice drew)
    logs = np.tile(base, (n, 1))
    i = np.arange(n)
    logs[i, i % cells] = (i + 1).astype(np.float64)
    logs[i, cells - 1] = np.where(i % 2 == 1, L_OCC, L_FREE)
    logs.flags.writeable = False
    return logs


@functools.lru_cache(maxsize=None)
def poses_of(shape, n=N):
    """float32 [n][3]: every particle at a pose of its own inside the middle half of the map, so that the weights differ"""
    W, H = shape
    i = np.arange(n)
    p = np.stack([(0.25 + 0.5 * ((i * 37) % n) / n) * W * RES, (0.25 + 0.5 * ((i * 101) % n) / n) * H * RES, -3.0 + 6.0 * i / n], axis=1).astype(np.float32)
    p.flags.writeable = False
    return p


def pack_planes(log):
    """uint32 [..., code_words]: the class plane of logData [..., cells] restated -- two bits a cell, sixteen cells a word, cell c in bits
    2 (c % 16) of word c // 16: 0 where logData == 0 or NaN, 1 where < 0, 2 where > 0; the words behind the last cell are zero"""
    log = np.asarray(log, dtype=np.float64)
    cells = log.shape[-1]
    cw = code_words(cells)
    with np.errstate(invalid="ignore"):
        cls = np.where(log > 0.0, 2, np.where(log < 0.0, 1, 0)).astype(np.uint32)
    pad = np.zeros(log.shape[:-1] + (16 * cw,), dtype=np.uint32)
    pad[..., :cells] = cls
    pad = pad.reshape(log.shape[:-1] + (cw, 16))
    return np.bitwise_or.reduce(pad << (2 * np.arange(16, dtype=np.uint32)), axis=-1).astype(np.uint32)


# ---- plans --------------------------------------------------------------------------------------------------------------------------------
def mask_of(name, src):
    """bool [n]: the slots whose source travels as a record -- none; all; every third slot plus slot 0 and slot n - 1; exactly the
    slots whose source is themselves"""
    src = np.asarray(src)
    n = len(src)
    if name == "none":
        return np.zeros(n, dtype=bool)
    if name == "all":
        return np.ones(n, dtype=bool)
    if name == "third":
        m = np.arange(n) % 3 == 0
        m[0] = m[n - 1] = True
        return m
    assert name == "self"
    return src == np.arange(n)


def plan_of(src, remote):
    """(export_list, src_local, recv_pos) int32: export_list the sorted unique sources of the masked slots; on a masked slot src_local =
    -1 and recv_pos the index of its source in export_list; elsewhere src_local = src (recv_pos -1: not read)"""
    src = np.asarray(src, dtype=np.int32)
    remote = np.asarray(remote, dtype=bool)
    export_list = np.unique(src[remote]).astype(np.int32)
    src_local = np.where(remote, -1, src).astype(np.int32)
    recv_pos = np.full(len(src), -1, dtype=np.int32)
    recv_pos[remote] = np.searchsorted(export_list, src[remote]).astype(np.int32)
    return export_list, src_local, recv_pos


def reversed_plan(plan):
    """the same copies from a receive buffer in another order and with a record twice: export_list reversed, its first entry then
    repeated in front, recv_pos adjusted -- the slots that want the repeated record read its two copies in turn.  The order and the
    multiplicity of the buffer are the plan's business, not the kernel's"""
    export_list, src_local, recv_pos = plan
    L = len(export_list)
    if L == 0:
        return plan
    rev = export_list[::-1]
    new_list = np.concatenate([rev[:1], rev]).astype(np.int32)
    new_pos = np.where(recv_pos >= 0, 1 + (L - 1 - recv_pos), -1).astype(np.int32)
    twice = np.nonzero(new_pos == 1)[0]                    # the slots of the repeated record: every other one reads the copy in front
    new_pos[twice[::2]] = 0
    return new_list, src_local.copy(), new_pos


def replay(plan, n):
    """int [n]: the particle every slot ends up holding under the plan, the received buffer being the records of export_list in order"""
    export_list, src_local, recv_pos = plan
    assert len(src_local) == n and len(recv_pos) == n
    out = np.array(src_local, dtype=np.int64)
    far = out < 0
    assert (recv_pos[far] >= 0).all() and (recv_pos[far] < len(export_list)).all()
    out[far] = export_list[recv_pos[far]]
    return out


def rounds_of(shape):
    """[(mask, reversed buffer)]: the draws of one handle in tests/test_gpu_slam_shard_records.py, an update between them -- every mask
    with both buffers, eight generation flips.  (The same for every shape: at the plane limit a round downloads and compares 1.6 GB of
    maps, and the eight of them take two to three seconds.)"""
    return [(m, r) for m in MASKS for r in (False, True)]
