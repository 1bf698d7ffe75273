"""What tests/test_gpu_slam_shard_records.py feeds the record movers of a sharded gms_slam, checked without a device: the shapes sit on
the edges they are named for, every particle's log differs from every other's, the plans resolve every slot to its source whatever the
order and multiplicity of the receive buffer -- and the 41 x 41 drive of tests/test_gpu_slam_sharded.py meets both sides of the
resampling rule in the oracle's own filter."""
import numpy as np
import pytest

import _shard_record_cases as sc
from _slam_align_edge_cases import MAX_PLANE_BYTES, code_words, planes_kept
from oracle import oracle as orc

shapes = pytest.mark.parametrize("shape", list(sc.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")


@shapes
def test_the_table(shape):
    cells, cw, rec = sc.SHAPES[shape]
    g = orc.Grid(*sc.size_of(shape), sc.RES, 0.0, 0.0)
    assert (g.W, g.H) == shape
    assert (shape[0] * shape[1], code_words(cells), sc.record_doubles(shape)) == (cells, cw, rec)
    assert planes_kept(shape[0], shape[1], len(g.kernel))


def test_the_edges_the_shapes_are_named_for():
    rec = {s: v[2] for s, v in sc.SHAPES.items()}
    assert rec[(40, 5)] < 256                                                          # under one pass of a workgroup's 256 lanes
    assert rec[(41, 41)] < sc.CHUNK and sc.SHAPES[(41, 41)][0] % 2 == 1 and 41 % 16 != 0
    assert rec[(52, 37)] == sc.CHUNK and rec[(55, 35)] == sc.CHUNK + 1 and sc.SHAPES[(55, 35)][0] % 2 == 1
    assert rec[(120, 120)] > sc.CHUNK and rec[(120, 120)] % sc.CHUNK != 0
    assert 4 * sc.SHAPES[(390, 252)][1] == MAX_PLANE_BYTES
    # the `e < cells` split falls inside a chunk, not on its edge, wherever there is more than one chunk
    assert all(v[0] % sc.CHUNK != 0 for v in sc.SHAPES.values())
    # the last code word is ragged somewhere, full somewhere
    assert any(v[0] % 16 for v in sc.SHAPES.values()) and any(v[0] % 16 == 0 for v in sc.SHAPES.values())
    W, H = sc.OVER_THE_LIMIT
    g = orc.Grid(*sc.size_of((W, H)), sc.RES, 0.0, 0.0)
    assert (g.W, g.H) == (W, H) and not planes_kept(W, H, len(g.kernel)) and 4 * code_words(W * H) == MAX_PLANE_BYTES + 16


@shapes
def test_every_particle_has_a_log_of_its_own(shape):
    logs = sc.logs_of(shape)
    cells = shape[0] * shape[1]
    assert logs.shape == (sc.N, cells) and logs.dtype == np.float64
    assert len({row.tobytes() for row in logs}) == sc.N                                # no two particles' logs have equal bytes
    bits = logs.view(np.uint64)
    for v in sc.SPECIALS:
        assert (bits == np.array(v).view(np.uint64)).any(), v
    assert (logs < 0).any() and (logs > 0).any() and (logs == 0).any()
    i = np.arange(sc.N)
    named = i % cells != cells - 1                                                     # (where the two marks fall on one cell the last cell's wins)
    assert (logs[i, i % cells][named] == (i + 1)[named]).all()
    assert (logs[1::2, -1] == sc.L_OCC).all() and (logs[0::2, -1] == sc.L_FREE).all()
    # the planes the marks give differ too: in the last cell's word by parity
    planes = sc.pack_planes(logs[:4])
    last = (cells - 1) // 16
    assert planes.shape == (4, code_words(cells)) and planes[0, last] != planes[1, last]
    assert (planes[:, (cells + 15) // 16:] == 0).all()


def test_the_plane_restatement_on_a_hand_made_log():
    log = np.zeros(19)
    log[[0, 1, 2, 3, 4, 15, 16, 18]] = [1.0, -1.0, np.nan, -0.0, 5e-324, -5e-324, np.inf, -np.inf]
    p = sc.pack_planes(log)
    assert p.shape == (code_words(19),) and p.dtype == np.uint32
    assert p[0] == (2 | 1 << 2 | 2 << 8 | 1 << 30) and p[1] == (2 | 1 << 4) and (p[2:] == 0).all()


def _sources(n, seed, fixed):
    """a non-decreasing draw, as systematic resampling gives, with at least `fixed` slots that drew themselves"""
    rng = np.random.default_rng(seed)
    src = np.sort(rng.integers(0, n, n)).astype(np.int32)
    if fixed:
        assert (src == np.arange(n)).sum() >= fixed
    return src


@pytest.mark.parametrize("mask", sc.MASKS)
@pytest.mark.parametrize("seed", [1, 4])
def test_every_plan_resolves_every_slot_to_its_source(mask, seed):
    n = sc.N
    src = _sources(n, seed, fixed=1)
    remote = sc.mask_of(mask, src)
    assert remote.sum() == {"none": 0, "all": n, "third": len(set(range(0, n, 3)) | {0, n - 1}), "self": (src == np.arange(n)).sum()}[mask]
    plan = sc.plan_of(src, remote)
    export_list, src_local, recv_pos = plan
    assert np.array_equal(export_list, np.unique(src[remote])) and export_list.dtype == src_local.dtype == recv_pos.dtype == np.int32
    assert (src_local[remote] == -1).all() and np.array_equal(src_local[~remote], src[~remote])
    assert np.array_equal(export_list[recv_pos[remote]], src[remote])
    assert np.array_equal(sc.replay(plan, n), src)
    rev = sc.reversed_plan(plan)
    assert np.array_equal(sc.replay(rev, n), src)
    if len(export_list):
        assert len(rev[0]) == len(export_list) + 1 and rev[0][0] == rev[0][1] == export_list[-1]
        assert np.array_equal(rev[0][1:], export_list[::-1])
        wants = remote & (src == export_list[-1])
        assert set(rev[2][wants]) == ({0, 1} if wants.sum() > 1 else {0})              # both copies of the repeated record are read
        if len(export_list) > 1:
            assert (np.diff(rev[0][1:]) < 0).all()                                     # not ascending
    else:
        assert rev is plan


def test_the_rounds():
    for shape in sc.SHAPES:
        rounds = sc.rounds_of(shape)
        assert len(rounds) >= 3                                                        # the generation flips back at least once
        assert set(rounds) == {(m, r) for m in sc.MASKS for r in (False, True)} and len(rounds) == 8


def test_the_41_x_41_drive_draws_and_skips_in_the_oracle():
    """tests/test_gpu_slam_sharded.py's (world 2, 2.05 m) case needs both sides of `neff < fraction * N`: the oracle's own filter of 512
    particles over the same six frames draws at least once and skips at least once (a fraction of a second on the CPU)"""
    import test_gpu_slam_sharded as sh
    world, refine, ext, N, T = next(c for c in sh.CASES if c[2] == 2.05)
    scans, start = sh._scans(ext, 90, T)
    g = orc.Grid(ext, ext, 0.05, -ext / 2, -ext / 2)
    assert (g.W, g.H) == (41, 41)
    s = orc.Slam(g, N)
    s.set_poses(np.tile(np.asarray(start, np.float32), (N, 1)))
    r01s = np.random.default_rng(9).random(T)
    fractions = sh._fractions(T)
    did = []
    for k, (z, u) in enumerate(scans):
        neff = s.update(z, u, seed=5, sequence=k)
        did.append(neff < fractions[k] * N)
        if did[-1]:
            s.resample(float(r01s[k]))
    assert any(did) and not all(did)
