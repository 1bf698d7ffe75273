"""k_score_c<1, true>: a scoring workgroup's lanes take its particles in the order of the segment's end-point lines (a counting sort
in LDS keyed by the row and 16-cell group of the middle hit beam's end point, folded to 256 buckets: ((row & 63) << 2) | (group & 3)).  Which lane forms a particle's product does not enter
the arithmetic, so everything here is array_equal between a filter created under GMS_SCORE_ORDER=0 (the caller's order) and filters
created with the order on: GMS_SCORE_SEGORDER=1 (every workgroup shape of more than one wavefront) and the launcher's default at
1024-lane workgroups (GMS_SCORE_THREADS=1024).  The switches are read when a filter is created, so the filters share one process;
gms_pf_segment_order_launches says which kernel a filter's launches took, and every comparison asserts it.

A 128 x 136 map (the key folds rows to 64 and the eight 16-cell groups to 4: rows and groups alias) built from three fixture scans; the weights of two cases
also go to the oracle at the tolerance test_gpu_parity.py / test_gpu_step_argument_order.py hold the scoring kernel to."""
import functools
import os

import numpy as np
import pytest

from gridmap_slam_robot_amd import BEAM_DTYPE, GridMap, ParticleFilter, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 1e-11                                   # test_gpu_step_argument_order.py's bound on the normalised weights
EXT_X, EXT_Y, RES = 6.4, 6.8, 0.05              # 128 x 136 cells
ORIGIN = (-EXT_X / 2, -EXT_Y / 2)
N_MAP_SCANS = 3
OFF = {"GMS_SCORE_ORDER": "0"}
ON = {"GMS_SCORE_SEGORDER": "1"}
ON_1024 = {"GMS_SCORE_THREADS": "1024"}
SWITCHES = ("GMS_SCORE_ORDER", "GMS_SCORE_SEGORDER", "GMS_SCORE_THREADS")


@functools.lru_cache(maxsize=None)
def _fixture(seed=1):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"scan64_seed{seed}.npz"))
    poses = np.asarray(d["poses"], dtype=np.float32)
    return d["scans"].view(BEAM_DTYPE).reshape(len(poses), -1), poses


@functools.lru_cache(maxsize=None)
def _oracle_field():
    scans, poses = _fixture()
    g = orc.Grid(EXT_X, EXT_Y, RES, ORIGIN[0], ORIGIN[1])
    assert (g.W, g.H) == (128, 136)
    log = g.new_log()
    for t in range(N_MAP_SCANS):
        g.integrate(log, scans[t], poses[t])
    return g, g.build_likelihood(log)


def _new_map():
    m = GridMap(EXT_X, EXT_Y, RES, ORIGIN)
    assert (m.W, m.H) == (128, 136)
    scans, poses = _fixture()
    for t in range(N_MAP_SCANS):
        m.update(scans[t], poses[t])
    return m


@pytest.fixture(scope="module")
def shared_map():
    m = _new_map()
    yield m
    m.close()


def _scan(B, k=N_MAP_SCANS):
    scans, _ = _fixture()
    s = np.concatenate([scans[(k + i) % len(scans)] for i in range(len(scans))])[:B].copy()
    assert len(s) == B
    return s


def _cloud(n, k=0):
    _, poses = _fixture()
    return synth.make_particles(poses[N_MAP_SCANS], n, seed=20 + k, sigma_xy=0.08, sigma_theta_deg=4.0)


def _filter(monkeypatch, m, n, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pf = ParticleFilter(m, n)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return pf


def _scored(monkeypatch, m, env, P, scan):
    pf = _filter(monkeypatch, m, len(P), env)
    pf.set_poses(P)
    pf.score(scan)
    out = pf.get_weights().copy(), pf.get_log_weights().copy()
    # which kernel ran: the caller's order never takes the segment order; forced on, every shape of more than one wavefront does
    # (a population of 64 or fewer is one wavefront); the default takes it at 1024-lane workgroups, whatever the population
    took = pf.segment_order_launches()
    assert took == (0 if env is OFF or (env is ON and len(P) <= 64) else 1), (env, len(P), took)
    pf.close()
    return out


def _same_bits(monkeypatch, m, P, scan, what):
    w0, l0 = _scored(monkeypatch, m, OFF, P, scan)
    for name, env in (("every shape", ON), ("1024 lanes", ON_1024)):
        w, l = _scored(monkeypatch, m, env, P, scan)
        assert np.array_equal(w, w0, equal_nan=True) and np.array_equal(l, l0, equal_nan=True), (what, name)
    return w0


def _check_oracle(w, scan, P, what):
    g, lik = _oracle_field()
    want = g.score(lik, scan, P)
    ok = want > 1e-290
    assert ok.any() and w.sum() > 0, what
    assert np.max(np.abs(w[ok] / w.sum() - want[ok] / want.sum()) / (want[ok] / want.sum())) <= TIGHT, what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_populations_at_the_wavefront_block_and_workgroup_edges(monkeypatch, shared_map, n):
    scan = _scan(90)
    P = _cloud(n)
    w = _same_bits(monkeypatch, shared_map, P, scan, f"n={n}")
    assert (w > 0).any()
    if n == 1025:
        _check_oracle(w, scan, P, f"n={n}")


@pytest.mark.parametrize("B", [1, 12, 45, 46, 90, 384, 385])
def test_scans_on_the_one_segment_path_and_under_both_segment_rules(monkeypatch, shared_map, B):
    scan = _scan(B)
    P = _cloud(1025, 1)
    w = _same_bits(monkeypatch, shared_map, P, scan, f"B={B}")
    if B == 12:                                  # one segment: w / logw stored by the scoring launch itself
        _check_oracle(w, scan, P, f"B={B}")


@pytest.mark.parametrize("hits", ["middle segment without a hit", "only a segment's last beam hits", "one hit in the whole scan"])
def test_segments_without_hits_and_with_one(monkeypatch, shared_map, hits):
    scan = _scan(36)                             # three segments of 12
    if hits == "middle segment without a hit":
        scan["hit"][12:24] = 0
    elif hits == "only a segment's last beam hits":
        scan["hit"][12:23] = 0
        scan["hit"][23] = 1
    else:
        scan["hit"][:] = 0
        scan["hit"][35] = 1
    w = _same_bits(monkeypatch, shared_map, _cloud(1300, 2), scan, hits)
    assert (w > 0).any() and len(np.unique(w)) > 1


def _end_cells(P, lx, ly):
    """the middle beam's end-point cell at heading 0 (c = 1, s = 0) in float64, as the kernel forms it"""
    qx = ((lx * 1.0 - ly * 0.0 + P[:, 0].astype(np.float64)) - ORIGIN[0]) * (1.0 / RES)
    qy = ((lx * 0.0 + ly * 1.0 + P[:, 1].astype(np.float64)) - ORIGIN[1]) * (1.0 / RES)
    return qx, qy


@pytest.mark.parametrize("state", ["one pose", "every bucket", "half outside", "non-finite", "guard"])
def test_particle_states(monkeypatch, shared_map, state):
    scan = _scan(24)                             # two segments of 12; every beam of the fixture's scan 3 hits (asserted)
    n = 1024
    P = _cloud(n, 3)
    if state == "one pose":
        P[:] = P[1]
    elif state == "every bucket":
        # heading 0, one particle per (row < 128, 16-cell group) of segment 0's middle hit beam: every one of the key's 256 buckets
        # holds exactly four of the workgroup's 1024 particles
        assert (scan["hit"][:12] != 0).all()
        lx, ly = float(scan["local_x"][6]), float(scan["local_y"][6])
        r, c = np.divmod(np.arange(n), 8)
        P[:, 0] = ORIGIN[0] + (16 * c + 8.5) * RES - lx
        P[:, 1] = ORIGIN[1] + (r + 0.5) * RES - ly
        P[:, 2] = 0.0
        P = P[np.random.default_rng(5).permutation(n)]
        qx, qy = _end_cells(P, lx, ly)
        keys = ((np.trunc(qy).astype(np.int64) & 63) << 2) | ((np.trunc(qx).astype(np.int64) >> 4) & 3)
        assert np.array_equal(np.bincount(keys, minlength=256), np.full(256, 4))
    elif state == "half outside":
        P[::2, 0] += 100.0
        P[1::4, 1] -= 7.0
    elif state == "non-finite":
        for i, v in enumerate([np.nan, np.inf, -np.inf]):
            for d in range(3):
                P[40 + 100 * i + 7 * d, d] = v
    else:
        # poses on cell corners at heading 0 and beams whose coordinates are whole cells: every quotient lies within 2^-19 of an
        # integer, beam_cell_fast's guard fires for the key's beam and in the loop (the exact-quotient tests' construction)
        k = np.random.default_rng(6).integers(40, 90, size=(n, 2))
        P[:, 0] = (k[:, 0] * np.float32(RES)).astype(np.float32) + np.float32(ORIGIN[0])
        P[:, 1] = (k[:, 1] * np.float32(RES)).astype(np.float32) + np.float32(ORIGIN[1])
        P[:, 2] = 0.0
        P[::3] = _cloud(n, 4)[::3]               # a third of the cloud stays ordinary
        j = np.arange(24)
        LX, LY = (j % 7 - 3) * 4 * RES, (j % 5 - 2) * 4 * RES
        scan = orc.make_beams(LX, LY, np.hypot(LX, LY), np.ones(24))
        qx, qy = _end_cells(P, LX[6], LY[6])
        tripped = (np.abs(qx - np.rint(qx)) <= 2.0 ** -19) | (np.abs(qy - np.rint(qy)) <= 2.0 ** -19)
        assert tripped.sum() >= n // 2
    w = _same_bits(monkeypatch, shared_map, P, scan, state)
    if state != "non-finite":
        assert np.isfinite(w).all()


def _step_state(pf, m):
    return pf.stats(), pf.get_poses(), pf.get_weights(), m.download_log(), m.download_likelihood()


def _assert_same_state(a, b, what):
    assert a[0] == b[0], what
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("entry", ["moved", "launch"])
def test_scan_steps_with_the_order_on_and_off(monkeypatch, entry):
    """the full scan step at 2048 particles over 3 scans -- poses entering through the scoring launch, and the motion-model sample
    taken inside it (the Philox draw is keyed by particle, not by lane): poses, weights, stats, map log-odds and likelihood"""
    import torch
    dev = torch.device("cuda", 0)
    n, B = 2048, 90
    maps = [_new_map() for _ in range(3)]
    pfs = [_filter(monkeypatch, m, n, env) for m, env in zip(maps, (OFF, ON, ON_1024))]
    P0 = _cloud(n, 5)
    for pf in pfs:
        pf.set_poses(P0)
    rng = np.random.default_rng(8)
    for k, frac in enumerate((0.0, 2.0, 0.5)):
        beams = torch.from_numpy(_scan(B, N_MAP_SCANS + k).view(np.uint8).copy()).to(dev)
        P = torch.from_numpy(_cloud(n, 6 + k)).to(dev)
        r01 = float(rng.random())
        for pf in pfs:
            if entry == "moved":
                pf.slam_update_u_dev(0.03, 0.02, 77, k, beams.data_ptr(), B, r01, frac, True)
            else:
                pf.slam_update_dev(P.data_ptr(), beams.data_ptr(), B, r01, frac, True)
        torch.cuda.synchronize()
        states = [_step_state(pf, m) for pf, m in zip(pfs, maps)]
        if entry == "moved" and k == 0:
            assert not np.array_equal(states[0][1], P0)
        for s in states[1:]:
            _assert_same_state(states[0], s, f"{entry} step {k}")
    assert [pf.segment_order_launches() for pf in pfs] == [0, 3, 3]
    for h in pfs + maps:
        h.close()


def test_shard_at_a_non_zero_offset_with_the_order_on_equals_the_stand_alone_filter_without(monkeypatch):
    """HipShardOps at offsets 0 and 1024 of 2048 particles, created with the order on for every shape (the second shard is the one
    whose offset is not zero; its gather slots are filled from the first shard's buffers, the copy an all-gather would make),
    against a stand-alone filter in the caller's order, with the motion-free scan step"""
    import torch
    from gridmap_slam_robot_amd.distributed import HipShardOps
    dev = torch.device("cuda", 0)
    n, world, B = 1024, 2, 90
    N = n * world
    ref_map = _new_map()
    maps = [_new_map() for _ in range(world)]
    ref = _filter(monkeypatch, ref_map, N, OFF)
    monkeypatch.setenv("GMS_SCORE_SEGORDER", "1")
    ops = [HipShardOps(m, n, r * n, N) for r, m in enumerate(maps)]
    monkeypatch.delenv("GMS_SCORE_SEGORDER")
    assert ops[1].pf.offset == n
    rng = np.random.default_rng(9)
    for k, frac in enumerate((0.0, 2.0)):
        beams = torch.from_numpy(_scan(B, N_MAP_SCANS + k).view(np.uint8).copy()).to(dev)
        P = torch.from_numpy(_cloud(N, 9 + k)).to(dev)
        r01 = float(rng.random())
        ref.slam_update_dev(P.data_ptr(), beams.data_ptr(), B, r01, frac, True)
        torch.cuda.synchronize()
        for r, o in enumerate(ops):
            o.exchange_begin((P[r * n:(r + 1) * n].data_ptr(), beams.data_ptr(), B, True))
        torch.cuda.synchronize()
        views = [o.gather_views() for o in ops]
        for r in range(world):
            for q in range(world):
                if q != r:
                    pg, _, tg, _ = views[r]
                    _, pl, _, tl = views[q]
                    pg[q * pl.numel():(q + 1) * pl.numel()].copy_(pl)
                    tg[q * tl.numel():(q + 1) * tl.numel()].copy_(tl)
        torch.cuda.synchronize()
        for o in ops:
            o.exchange_end((0, beams.data_ptr(), B, True), r01, frac)
        torch.cuda.synchronize()
        st, poses, weights = ref.stats(), ref.get_poses(), ref.get_weights()
        for r, (o, m) in enumerate(zip(ops, maps)):
            what = f"shard {r} step {k}"
            assert o.pf.stats() == st, what
            assert np.array_equal(o.pf.get_poses(), poses[r * n:(r + 1) * n]), what
            assert np.array_equal(o.pf.get_weights(), weights[r * n:(r + 1) * n]), what
            assert np.array_equal(m.download_log(), ref_map.download_log()), what
            assert np.array_equal(m.download_likelihood(), ref_map.download_likelihood()), what
    assert ref.segment_order_launches() == 0 and [o.pf.segment_order_launches() for o in ops] == [2, 2]
    for o in ops:
        o.pf.close()
    ref.close()
    for m in maps + [ref_map]:
        m.close()
