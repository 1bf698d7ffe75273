"""The scan step's kernels take their arguments in an order chosen for kernel-argument preload (k_score_c, k_partials,
k_norm_raycast, k_lik_resample: what the first loads and branches read leads, the grid descriptor comes last).  A reorder goes wrong
by swapping two pointers of one type or two int32 values, and such a swap survives exactly where the two happen to be equal or
unused.  So every case here makes the neighbours differ: W != H (128 x 96), n != B, more than one block with lanes beyond the
population (n = 300) and exactly one block (n = 256), one segment (B = 12: the w / logw store path), four segments (B = 48), a
long scan with a run of misses (B = 400: beam_stride != hits), poses entering through the launch, moved in the launch and already
resident, the locality order (ord / perm), a batched handle with a scan per map (the map strides), a shard at a non-zero offset,
resampling taken and not taken, the map update on and off.

Paired step == the same step through the separate entry points, bit for bit (poses, weights, statistics, map and field); the
weights of the first step against the oracle at the tolerance test_gpu_parity.py holds the scoring kernel to; the cells and classes
every beam of the step's scan visits (trace_scan: k_raycast's tracing form) after the paired step, after the separate calls and
from the oracle, exactly."""
import functools
import os

import numpy as np
import pytest

from gridmap_slam_robot_amd import BEAM_DTYPE, GridMap, ParticleFilter, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = 1e-11                                   # test_gpu_parity.py's bound on the weights (tree vs sequential rounding)
EXT_X, EXT_Y, RES = 6.4, 4.8, 0.05              # 128 x 96 cells
ORIGIN = (-EXT_X / 2, -EXT_Y / 2)
N_MAP_SCANS = 5


@functools.lru_cache(maxsize=None)
def _fixture(seed):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"scan64_seed{seed}.npz"))
    poses = np.asarray(d["poses"], dtype=np.float32)
    scans = d["scans"].view(BEAM_DTYPE).reshape(len(poses), -1)
    return scans, poses


@functools.lru_cache(maxsize=None)
def _oracle_field(seed):
    """the oracle's field after the fixture's first scans (computed once and shared; nothing writes to it)"""
    scans, poses = _fixture(seed)
    g = orc.Grid(EXT_X, EXT_Y, RES, ORIGIN[0], ORIGIN[1])
    assert (g.W, g.H) == (128, 96)
    log = g.new_log()
    for t in range(N_MAP_SCANS):
        g.integrate(log, scans[t], poses[t])
    return g, g.build_likelihood(log)


def _new_map(seed, n_maps=1, seeds=None):
    m = GridMap(EXT_X, EXT_Y, RES, ORIGIN, n_maps=n_maps)
    assert (m.W, m.H) == (128, 96)
    fx = [_fixture(s) for s in (seeds or [seed])]
    for t in range(N_MAP_SCANS):
        if n_maps > 1:
            m.update(np.stack([f[0][t] for f in fx]), np.stack([f[1][t] for f in fx]))
        else:
            m.update(fx[0][0][t], fx[0][1][t])
    return m


def _scan(seed, B, k):
    """B beams out of the fixture's scans from scan k on (72 beams each, end to end); the long scan gets a run of misses"""
    scans, _ = _fixture(seed)
    order = [(k + i) % len(scans) for i in range(len(scans))]
    s = np.concatenate([scans[i] for i in order])[:B].copy()
    assert len(s) == B
    if B >= 400:
        s["hit"][100:181] = 0
        assert 0 < int((s["hit"] != 0).sum()) < B
    return s


def _particles(seed, n, k):
    _, poses = _fixture(seed)
    return synth.make_particles(poses[N_MAP_SCANS], n, seed=10 * seed + k, sigma_xy=0.04, sigma_theta_deg=2.0)


def _same(pa, pb, a, b, what):
    assert pa.stats() == pb.stats(), what
    assert np.array_equal(pa.get_poses(), pb.get_poses()), what
    assert np.array_equal(pa.get_weights(), pb.get_weights()), what
    assert np.array_equal(a.download_log(), b.download_log()), what
    assert np.array_equal(a.download_likelihood(), b.download_likelihood()), what


TRACE_CAP = 256                                 # cells per beam: a ray of a 128 x 96 grid visits at most W + H + 1 = 225


@functools.lru_cache(maxsize=None)
def _oracle_cells(seed, B, k):
    """the oracle's cells and classes, beam by beam, of _scan(seed, B, k) from the fixture's pose k (computed once and shared)"""
    g, _ = _oracle_field(seed)
    rays = g.scan_rays(_scan(seed, B, k), _trace_pose(seed, k))
    return [g.apply_measurement(None, *rays[b, :5], bool(rays[b, 5]), cap=4096) for b in range(B)]


def _trace_pose(seed, k):
    _, poses = _fixture(seed)
    return poses[k % len(poses)]


def _same_cells(seed, B, k, handles, what):
    """trace_scan of every handle: the same cell lists from each of them, and the oracle's.  (The lists depend on the grid's
    geometry, the scan and the pose alone; the traced scan's beam stride is the map's max_beams, not B.)"""
    scan, pose = _scan(seed, B, k), _trace_pose(seed, k)
    want = _oracle_cells(seed, B, k)
    got = [h.trace_scan(scan, pose, cap=TRACE_CAP) for h in handles]
    cells0, cls0, counts0 = got[0]
    assert counts0.max() <= TRACE_CAP and counts0.max() > 0, what
    live = np.arange(cells0.shape[1])[None, :] < counts0[:, None]
    for cells, cls, counts in got[1:]:
        assert np.array_equal(counts, counts0), what
        assert np.array_equal(cells[live], cells0[live]) and np.array_equal(cls[live], cls0[live]), what
    assert counts0.tolist() == [len(oc) for oc, _ in want], what
    for b, (oc, ok) in enumerate(want):
        assert np.array_equal(cells0[b, :counts0[b]], oc) and np.array_equal(cls0[b, :counts0[b]], ok), (what, b)


def _check_oracle(seed, pf, scan, what):
    """normalised weights of a step that did not resample, at the poses the filter holds, against the oracle's"""
    g, lik = _oracle_field(seed)
    P = pf.get_poses()
    want = g.score(lik, scan, P)
    ok = want > 1e-290
    wn = want.copy()
    ws, strongest = orc.normalize(wn)
    got = pf.get_weights()
    assert ok.any() and np.max(np.abs(got[ok] - wn[ok]) / wn[ok]) <= TIGHT, what
    assert pf.stats()["strongest"] == strongest, what


# resampling not taken (the first step: its weights go to the oracle), forced, decided by Neff
FRACTIONS = (0.0, 2.0, 0.5)


@pytest.mark.parametrize("entry,B,n,order,integrate", [
    ("launch", 12, 300, None, True), ("launch", 48, 300, None, True), ("launch", 400, 300, None, True), ("launch", 48, 256, None, False),
    ("moved", 12, 256, None, True), ("moved", 48, 300, None, False), ("moved", 400, 300, None, True),
    ("resident", 12, 300, None, False), ("resident", 48, 256, None, True), ("resident", 400, 300, None, True),
    ("launch", 48, 300, "1", True), ("moved", 400, 300, "1", True), ("resident", 12, 256, "1", False)])
def test_paired_step_equals_the_separate_calls(monkeypatch, entry, B, n, order, integrate):
    import torch
    dev = torch.device("cuda", 0)
    seed = 1
    if order is not None:
        monkeypatch.setenv("GMS_SCORE_ORDER", order)            # read when the filter is created
    a, b = _new_map(seed), _new_map(seed)
    pa, pb = ParticleFilter(a, n), ParticleFilter(b, n)
    P0 = _particles(seed, n, 0)
    pa.set_poses(P0); pb.set_poses(P0)
    rng = np.random.default_rng(4)
    for k, frac in enumerate(FRACTIONS):
        scan = _scan(seed, B, N_MAP_SCANS + k)
        beams = torch.from_numpy(scan.view(np.uint8).copy()).to(dev)
        P = torch.from_numpy(_particles(seed, n, 1 + k)).to(dev)
        r01 = float(rng.random())
        what = f"{entry} B={B} n={n} order={order} integrate={integrate} step {k}"
        if entry == "launch":                                    # the poses enter the filter through the scoring launch
            pa.slam_update_dev(P.data_ptr(), beams.data_ptr(), B, r01, frac, integrate)
            pb.set_poses_dev(P.data_ptr())
        elif entry == "moved":                                   # the motion-model sample is taken inside the scoring launch
            pa.slam_update_u_dev(0.03, 0.02, 77, k, beams.data_ptr(), B, r01, frac, integrate)
            pb.sample_motion(0.03, 0.02, 77, k)
        else:                                                    # the poses the filter already holds
            pa.set_poses_dev(P.data_ptr())
            pa.slam_update_dev(0, beams.data_ptr(), B, r01, frac, integrate)
            pb.set_poses_dev(P.data_ptr())
        pb.score_dev(beams.data_ptr(), B); pb.normalize(fetch=False); pb.resample_if(r01, frac)
        if integrate:
            b.update_at_dev(beams.data_ptr(), B, pb)
        torch.cuda.synchronize()
        _same(pa, pb, a, b, what)
        _same_cells(seed, B, N_MAP_SCANS + k, (a, b), what)
        if k == 0:
            if entry == "moved":
                assert not np.array_equal(pa.get_poses(), P0), what
            _check_oracle(seed, pa, scan, what)
        elif k == 1:
            assert len(np.unique(pa.last_resample_indices())) < n, what          # the forced resampling was taken
    for h in (pa, pb, a, b):
        h.close()


@pytest.mark.parametrize("order", [None, "1"])
def test_batched_paired_step_with_a_scan_per_map(monkeypatch, order):
    """two maps built from different fixtures, a scan and a cloud per map: the map strides (and, ordered, k_score_c<3>)"""
    import torch
    dev = torch.device("cuda", 0)
    if order is not None:
        monkeypatch.setenv("GMS_SCORE_ORDER", order)
    seeds, n, B = [1, 2], 300, 48
    a, b = _new_map(0, 2, seeds), _new_map(0, 2, seeds)
    pa, pb = ParticleFilter(a, n), ParticleFilter(b, n)
    rng = np.random.default_rng(6)
    for k, frac in enumerate(FRACTIONS):
        scans = np.stack([_scan(s, B, N_MAP_SCANS + k) for s in seeds])
        assert not np.array_equal(scans[0], scans[1])
        sd = torch.from_numpy(scans.view(np.uint8).copy()).to(dev)
        Ph = np.stack([_particles(s, n, 1 + k) for s in seeds])
        Pd = torch.from_numpy(Ph).to(dev)
        r01 = rng.random(2)
        pa.slam_update_dev(Pd.data_ptr(), sd.data_ptr(), B, r01, frac, True)
        pb.set_poses_dev(Pd.data_ptr()); pb.score_dev(sd.data_ptr(), B); pb.normalize(fetch=False); pb.resample_if(r01, frac)
        b.update_at_dev(sd.data_ptr(), B, pb)
        torch.cuda.synchronize()
        _same(pa, pb, a, b, f"batched order={order} step {k}")
        _same_cells(seeds[0], B, N_MAP_SCANS + k, (a, b), f"batched order={order} step {k}")
        if k == 0:
            got = pa.get_weights()
            for i, s in enumerate(seeds):
                g, lik = _oracle_field(s)
                want = g.score(lik, scans[i], Ph[i])
                ok = want > 1e-290
                orc.normalize(want)
                assert ok.any() and np.max(np.abs(got[i][ok] - want[ok]) / want[ok]) <= TIGHT, (order, i)
    for h in (pa, pb, a, b):
        h.close()


@pytest.mark.parametrize("integrate", [True, False])
def test_shard_at_a_non_zero_offset_equals_the_stand_alone_filter(integrate):
    """HipShardOps at offsets 0 and 256 of a population of 512 (the second is the shard whose offset is not zero; its gather slots
    are filled from the first shard's buffers, the copy an all-gather would make): particles, weights, statistics and the map
    replica of the shard at the offset equal the stand-alone filter's"""
    import torch
    from gridmap_slam_robot_amd.distributed import HipShardOps
    dev = torch.device("cuda", 0)
    seed, n, world, B = 3, 256, 2, 48
    N = n * world
    ref_map = _new_map(seed)
    maps = [_new_map(seed) for _ in range(world)]
    ref = ParticleFilter(ref_map, N)
    ops = [HipShardOps(m, n, r * n, N) for r, m in enumerate(maps)]
    assert ops[1].pf.offset == n
    rng = np.random.default_rng(9)
    for k, frac in enumerate(FRACTIONS):
        scan = _scan(seed, B, N_MAP_SCANS + k)
        beams = torch.from_numpy(scan.view(np.uint8).copy()).to(dev)
        P = torch.from_numpy(_particles(seed, N, 1 + k)).to(dev)
        r01 = float(rng.random())
        ref.slam_update_dev(P.data_ptr(), beams.data_ptr(), B, r01, frac, integrate)
        torch.cuda.synchronize()
        for r, o in enumerate(ops):
            o.exchange_begin((P[r * n:(r + 1) * n].data_ptr(), beams.data_ptr(), B, integrate))
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
            o.exchange_end((0, beams.data_ptr(), B, integrate), r01, frac)
        torch.cuda.synchronize()
        st, poses, weights = ref.stats(), ref.get_poses(), ref.get_weights()
        for r, (o, m) in enumerate(zip(ops, maps)):
            what = f"shard {r} integrate={integrate} step {k}"
            assert o.pf.stats() == st, what
            assert np.array_equal(o.pf.get_poses(), poses[r * n:(r + 1) * n]), what
            assert np.array_equal(o.pf.get_weights(), weights[r * n:(r + 1) * n]), what
            assert np.array_equal(m.download_log(), ref_map.download_log()), what
            assert np.array_equal(m.download_likelihood(), ref_map.download_likelihood()), what
        _same_cells(seed, B, N_MAP_SCANS + k, (ref_map, maps[0], maps[1]), f"shards integrate={integrate} step {k}")
        if k == 0:
            _check_oracle(seed, ref, scan, "stand-alone filter beside the shards")
    for o in ops:
        o.pf.close()
    ref.close()
