"""Everything that moves the shared map's logData, and every map query that answers from something derived from logData, as data: no
device is touched here.  tests/test_mover_inputs.py holds the two lists against each other on the host (a mover that a query's fixed
request cannot see would let a stale answer pass), tests/test_gpu_query_movers.py runs every pair on the device.

A mover is the quadruple tests/test_gpu_cast_edges.py already uses -- (logData before, logData the oracle predicts, prepare, move) of a
grid --; its eleven are imported, not copied.  A consumer is ask(m, pf) -> a tuple of numpy arrays and expect(log) -> the same tuple from
the suite's own expectation modules; two answers are equal when every array's bytes are."""
import collections
import functools
import math

import numpy as np

import _align_expect as ax
import _beams_expect as bx
import _cast_expect as ce
import _clearance_expect as xe
import _frontier_expect as fx
import _gain_expect as gx
import _locate_expect as lx
import _reach_expect as rx
import _rollout_expect as ro
import _scatter_expect as sx
import _view_expect as ve
import _warp_expect as wx
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, beam_model_factors
from gridmap_slam_robot_amd._lib import GMS_CLEAR_NOT_FREE, GMS_CLEAR_OCCUPIED
from oracle import oracle as orc
from test_gpu_cast_edges import BACK, FRONT, LEFT, MOVERS as CAST_MOVERS, POSE5, RIGHT, _fan, _scanned

RES = 0.05
SHAPES = {"64x64": (64, 64), "65x33": (65, 33)}        # 65 x 33: one cell in the second 64-bit word, an odd count of rows
N_PF = 257                                             # the consumers' filter: one slot more than a workgroup of the draw
SEED, SEQ = 0x123456789ABCDEF, 0xFEDCBA9876543210
MARGIN = 4                                             # cells, records or poses a mover must change for a pair to count as seen


def grid_of(shape):
    W, H = SHAPES[shape]
    g = orc.Grid((W - 0.4) * RES, (H - 0.4) * RES, RES, 0.0, 0.0)
    assert (g.W, g.H) == (W, H)
    return g


def map_of(g, **kw):
    """a GridMap of the grid's geometry (64 x 64: test_gpu_cast_edges._map5's)"""
    m = GridMap((g.W - 0.4) * RES, (g.H - 0.4) * RES, RES, (0.0, 0.0), max_beams=64, **kw)
    assert (m.W, m.H) == (g.W, g.H)
    return m


def as_grid(g, log):
    return np.asarray(log, dtype=np.float64).reshape(g.H, g.W)


# ---- the movers ----------------------------------------------------------------------------------------------------------------------
Mover = collections.namedtuple("Mover", "case moves exact repacks env ragged slam fresh field")
# case(g) -> (before, predicted, prepare, move); moves: logData changes; exact: the pose the scan is integrated at is POSE5 to the bit
# (a weighted mean of equal poses is not); repacks: the planes are marked stale although nothing moved; env: set while the map is
# created; ragged: runs on 65 x 33 too; slam: the map is the shared map of a SLAMParticleMaps that prepare(None) creates; fresh: prepare
# makes `before` itself, by updates of a fresh map (nothing is uploaded); field: what the mover does to likelihoodData -- None: it leaves
# the field as it is (the consumers of the field take it for a non-mover), "exact": it rebuilds or replaces it with the field the oracle
# builds from the predicted logData, "rounded": with the field of logData that equals the prediction up to rounding only


def _on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def _warp(op, shift, wall_scans, before_scans):
    """warp_from a second map that holds the wall, under a shift of `shift` cells along x (0: the identity)"""
    def case(g):
        gd = wx.Geometry.make(g.W, g.H, RES, 0.0, 0.0)
        wall, before = _scanned(g, *wall_scans), _scanned(g, *before_scans)
        pose = (shift * RES, 0.0, 1.0, 0.0)
        predicted, _ = wx.expect(as_grid(g, before), gd, as_grid(g, wall), gd, pose, op)
        def prepare(m):
            other = map_of(g)
            other.upload_log(wall)
            return other
        return before, predicted, prepare, lambda m, other: m.warp_from(other, pose[:2], c=pose[2], s=pose[3], op=op, stats=False)
    return case


def _mv_copy_with_field(g):
    """copy_from a map whose field has been built: logData and likelihoodData both arrive"""
    wall = _scanned(g, FRONT)
    def prepare(m):
        other = map_of(g)
        other.upload_log(wall)
        other.compute_likelihood_map()
        return other
    return g.new_log(), wall, prepare, lambda m, other: m.copy_from(other)


def _mv_upload_likelihood(g):
    wall = _scanned(g, LEFT)
    return wall, wall, lambda m: None, lambda m, c: m.upload_likelihood(m.download_likelihood())


def _mv_slam_combined(g):
    """gms_slam_combined: calculateCombined over the particles' maps, written into the handle's shared map"""
    wall = _scanned(g, FRONT)
    def prepare(_):
        s = SLAMParticleMaps((g.W - 0.4) * RES, (g.H - 0.4) * RES, RES, (0.0, 0.0), num_particles=2, max_beams=64)
        assert (s.W, s.H) == (g.W, g.H)
        lik = g.build_likelihood(wall.reshape(-1)).reshape(g.H, g.W)
        for k in range(2):
            s.set_map(k, as_grid(g, wall), lik)
        return s
    return g.new_log(), orc.combine_maps(np.stack([wall.reshape(-1)] * 2)), prepare, lambda m, s: s.calculate_combined()


FRACTION = 0.9                                         # Neff < 0.9 n resamples: the steps pair their tail with it and leave the apply pass owed


def _after_two_updates(g, prepare):
    """(before, predicted, prepare) of two fused steps on a map in its steady state: two updates behind the pose have built the field,
    so the first step pairs its launches already, the second one's ray cast carries the first one's apply pass, and the second one's
    is owed when the next query comes"""
    behind = _scanned(g, BACK, BACK)
    def prepared(m):
        m.update(BACK, POSE5); m.update(BACK, POSE5)
        return prepare(m)
    return behind, _scanned(g, LEFT, RIGHT, log=behind), prepared


def _device_steps(step):
    """two fused steps that integrate LEFT and RIGHT at sixteen particles on POSE5, from device-resident inputs, nothing read back
    in between; step(pf, poses, beams, B, r01)"""
    def move(m, pf):
        import torch
        P = _on_device(np.tile(POSE5, (16, 1)))
        scans = [_on_device(z) for z in (LEFT, RIGHT)]
        torch.cuda.synchronize()
        for d, z, r01 in zip(scans, (LEFT, RIGHT), (0.3, 0.6)):
            step(pf, P.data_ptr(), d.data_ptr(), len(z), r01)
        m.synchronize()                                # (the inputs live until the steps have read them)
    return move


def _mv_slam_update_dev_twice(g):
    move = _device_steps(lambda pf, P, d, B, r01: pf.slam_update_dev(P, d, B, r01, FRACTION, True))
    return _after_two_updates(g, lambda m: ParticleFilter(m, 16)) + (move,)


def _mv_sharded_twice(g):
    """one shard of one: the all-gather between the two halves has nothing to copy"""
    def prepare(m):
        pf = ParticleFilter(m, 16)
        pf.set_shard(0, 16)
        return pf
    def step(pf, P, d, B, r01):
        pf.slam_update_sharded_begin_dev(P, d, B)
        assert pf.gather_buffers()[1] > 0
        pf.slam_update_sharded_end_dev(d, B, r01, FRACTION, True)
    return _after_two_updates(g, prepare) + (_device_steps(step),)


def _mover(case, moves=True, exact=True, repacks=False, env=None, ragged=False, slam=False, fresh=False, field=None):
    return Mover(case, moves, exact, repacks, env, ragged, slam, fresh, field)


CAST_FIELDS = {"update, first call": "exact", "update, deferred": "exact", "update_at": "exact", "slam_update twice": "rounded"}
MOVERS = {name: _mover(case, exact=name != "slam_update twice", ragged=name in ("upload_log", "update, deferred"), field=CAST_FIELDS.get(name))
          for name, case in CAST_MOVERS.items()}
MOVERS.update({
    "warp_from, replace": _mover(_warp("replace", 0, (FRONT,), ())),
    "warp_from, replace, shifted a cell": _mover(_warp("replace", 1, (FRONT,), ())),
    "warp_from, add": _mover(_warp("add", 0, (FRONT,), (BACK,)), ragged=True),
    "warp_from, add, shifted a cell": _mover(_warp("add", 1, (FRONT,), (BACK,))),
    "the gms_slam write": _mover(_mv_slam_combined, slam=True, field="rounded"),
    "copy_from, with its field": _mover(_mv_copy_with_field, field="exact"),
    "sharded step twice, one shard of one": _mover(_mv_sharded_twice, exact=False, fresh=True, field="rounded"),
    "slam_update_dev twice": _mover(_mv_slam_update_dev_twice, exact=False, fresh=True, field="rounded"),
    "slam_update_dev twice, GMS_PAIR_LAUNCHES=0": _mover(_mv_slam_update_dev_twice, exact=False, env={"GMS_PAIR_LAUNCHES": "0"}, fresh=True,
                                                         field="rounded"),
    "warp_from, compare only": _mover(_warp("compare", 1, (FRONT,), (LEFT,)), moves=False),
    "upload_likelihood": _mover(_mv_upload_likelihood, moves=False, repacks=True),
})
assert len(CAST_MOVERS) == 11 and len(MOVERS) == 22 and sum(mv.field is not None for mv in MOVERS.values()) >= 9


def mover_names(shape):
    return [n for n, mv in MOVERS.items() if shape == "64x64" or mv.ragged]


# ---- the consumers -------------------------------------------------------------------------------------------------------------------
Consumer = collections.namedtuple("Consumer", "ask expect occupied not_free table field", defaults=(None,))
# occupied / not_free: a request of it reads that plane; table: it reads the seeding table; field: None, or -- a consumer that answers
# from likelihoodData, not from logData -- the expectation as a function of the field; expect(log) is then that of the field the oracle
# builds from log, which holds behind the movers that rebuild the field (Mover.field) and behind no other

CELL5 = (32, 32)                                       # POSE5's cell
NEAR5 = np.array([[1.6, 1.6, 0.0], [1.45, 1.6, 1.5], [1.75, 1.6, 3.0], [1.6, 1.45, -1.5], [1.6, 1.75, 0.7], [1.5, 1.5, 2.2]], dtype=np.float32)
RING = _fan(-math.pi, math.pi * 15 / 16, 32, 0.9)      # all round a pose, 18 cells long
POSES16 = np.concatenate([np.tile(POSE5, (11, 1)), NEAR5[1:]]).astype(np.float32)      # eleven particles on POSE5, five beside it
BEHIND, AHEAD = 3, 2
FACTORS = beam_model_factors(RES, BEHIND, AHEAD, 0.05)
ALL_ROUND = np.concatenate([FRONT[::2], BACK[::2]])    # the fan the filter is scored with: 64 beams ahead of and behind the pose
LOCATE_RECT, N_THETA = (27, 27, 11, 11), 4


def _straight_arcs(K=8, T=16):
    """K straight runs of T steps of one cell, their headings all round the start pose"""
    a = np.arange(K) * (2.0 * math.pi / K)
    d = RES * np.arange(1, T + 1)
    return ro.steps(np.cos(a)[:, None] * d[None, :], np.sin(a)[:, None] * d[None, :], np.cos(a)[:, None] + 0 * d[None, :], np.sin(a)[:, None] + 0 * d[None, :])


ARCS = _straight_arcs()
ROLL_POSES = NEAR5[:2]


def _cells(a):
    return tuple(np.ascontiguousarray(x) for x in a)


def consumers(shape):
    """name -> Consumer for maps of this shape (the expectations need the grid)"""
    g = grid_of(shape)
    W, H = g.W, g.H
    geo = ro.Geometry(W, H, RES, 0.0, 0.0)
    rect = (20, 4, 30, H - 8)                          # cuts words on both sides at either shape
    offsets = lx.offsets_of(FRONT["local_x"], FRONT["local_y"], FRONT["hit"], N_THETA, RES)
    loc_rect = (LOCATE_RECT[0], min(LOCATE_RECT[1], H - 11), 11, 11)
    walks = gx.walks_of(g, RING, NEAR5)
    out = {}

    def cached(fn):
        memo = {}
        def expect(log):
            log = as_grid(g, log)
            key = log.tobytes()
            if key not in memo:
                memo[key] = _cells(fn(log))
            return memo[key]
        return expect

    # clearance: both modes, the whole map and under poses
    out["clearance"] = Consumer(lambda m, pf: _cells(m.clearance(None, 8, nf) for nf in (False, True)),
                                cached(lambda log: [xe.expect(log, 8, nf) for nf in (False, True)]), True, True, False)
    fan_poses = np.concatenate([NEAR5, np.stack([POSE5[0] + np.float32(0.5) * np.cos(np.linspace(-3, 3, 26)), POSE5[1] + np.float32(0.5) * np.sin(np.linspace(-3, 3, 26)),
                                                 np.zeros(26)], axis=1).astype(np.float32)])
    out["clearance_poses"] = Consumer(lambda m, pf: _cells(m.clearance_poses(fan_poses, 8, nf) for nf in (False, True)),
                                      cached(lambda log: [xe.expect_poses(xe.expect(log, 8, nf), fan_poses, 0.0, 0.0, RES) for nf in (False, True)]),
                                      True, True, False)
    # reach: seeded at the pose's cell
    reach_modes = [(i, nf) for i in (0, 2) for nf in (False, True)]
    out["reach"] = Consumer(lambda m, pf: _cells(m.reach([CELL5], inflate=i, not_free=nf) for i, nf in reach_modes),
                            cached(lambda log: [rx.expect(log, [CELL5], inflate=i, not_free=nf) for i, nf in reach_modes]), True, True, False)
    # frontiers: records, their count and the label field
    def ask_frontiers(m, pf):
        rec, n, lab = m.frontiers(min_size=1, labels=True)
        return _cells([rec, np.array([n]), lab])
    def want_frontiers(log):
        rec, n, lab = fx.expect(log, min_size=1)
        return [rec, np.array([n]), lab]
    out["frontiers"] = Consumer(ask_frontiers, cached(want_frontiers), True, True, False)
    out["gain"] = Consumer(lambda m, pf: _cells([m.gain(NEAR5, RING, 16)]), cached(lambda log: [gx.expect_walks(walks, log, 16)]), True, True, False)
    # the beam model: sixteen distinct particles repeated over the filter
    tiled = np.tile(POSES16, (N_PF // 16 + 1, 1))[:N_PF]
    def ask_beams(m, pf):
        pf.set_poses(tiled)
        idx = pf.score_beams(ALL_ROUND, FACTORS, BEHIND, AHEAD, residuals=True)
        return _cells([idx, pf.get_weights(), pf.get_log_weights()])
    def want_beams(log):
        w, lw, idx = bx.expect(g, log, ALL_ROUND, POSES16, FACTORS, BEHIND, AHEAD)
        rep = lambda a: np.concatenate([a] * (N_PF // 16 + 1))[:N_PF]
        return [rep(idx), rep(w), rep(lw)]
    out["score_beams"] = Consumer(ask_beams, cached(want_beams), True, False, False)
    roll_modes = [(i, nf) for i in (0, 1) for nf in (True, False)]
    out["rollout"] = Consumer(lambda m, pf: _cells(m.rollout(ROLL_POSES, ARCS, None, 255, i, nf) for i, nf in roll_modes),
                              cached(lambda log: [ro.expect(geo, log, ROLL_POSES, ARCS, np.zeros((0, 2), np.float32), 255, i, nf) for i, nf in roll_modes]),
                              True, True, False)
    loc_modes = [(fo, nf) for fo in (True, False) for nf in (False, True)]
    def ask_locate(m, pf):
        got = []
        for fo, nf in loc_modes:
            rec, n = m.locate(offsets, loc_rect, tol=1, not_free=nf, min_score=1, cap=64, free_only=fo, full=True)
            got += [rec, np.array([n])]
        return _cells(got)
    def want_locate(log):
        want = []
        for fo, nf in loc_modes:
            rec, n, _ = lx.expect(log, offsets, loc_rect, 1, nf, 1, 64, fo)
            want += [rec, np.array([n])]
        return want
    out["locate"] = Consumer(ask_locate, cached(want_locate), True, True, False)
    # scatter: one request each (a second request rebuilds the table on an unchanged map as well)
    def scatter(name, r, inflate, nf):
        def ask(m, pf):
            pf.set_poses(np.zeros((N_PF, 3), np.float32))
            M = pf.scatter(rect=r, inflate=inflate, mode=GMS_CLEAR_NOT_FREE if nf else GMS_CLEAR_OCCUPIED, seed=SEED, sequence=SEQ, want_count=True)
            return _cells([pf.get_poses(), np.array([M])])
        def want(log):
            poses, _, M = sx.expect(log, (0.0, 0.0), RES, 0, N_PF, SEED, SEQ, rect=r, inflate=inflate, not_free=nf)
            return [np.zeros((N_PF, 3), np.float32) if M == 0 else poses, np.array([M])]           # nothing eligible: the poses stay
        out[name] = Consumer(ask, cached(want), inflate > 0 and not nf, True, True)
    scatter("scatter, whole map", None, 0, True)
    scatter("scatter, rectangle, inflate 1, NOT_FREE", rect, 1, True)
    scatter("scatter, whole map, inflate 1, OCCUPIED", None, 1, False)
    # cast_at: from the strongest pose of a filter that sits on POSE5
    probes = np.concatenate([_fan(-math.pi, math.pi * 23 / 24, 48, 1.2), _fan(-0.03, 0.03, 8, 1.2)])     # (eight of them along apply_ray's line)
    def ask_cast_at(m, pf):
        pf.set_poses(np.tile(POSE5, (N_PF, 1)))
        pf.score(FRONT)
        pf.normalize()
        assert np.array_equal(pf.last_step()["strongest_pose"], POSE5)
        return _cells([m.cast_at(probes, pf, strongest=True)])
    out["cast_at"] = Consumer(ask_cast_at, cached(lambda log: [ce.expect(g, log, probes, POSE5)]), True, False, False)
    out["view"] = Consumer(lambda m, pf: _cells([m.view(), m.view((3, 1, W - 5, H - 3), 2)]),
                           cached(lambda log: [ve.expect(ve.idx_map(log, False), (0, 0, W, H), 1, False, False),
                                               ve.expect(ve.idx_map(log, False), (3, 1, W - 5, H - 3), 2, False, False)]), False, False, False)
    # align: six poses beside POSE5 against the likelihood field as it stands
    prm = ax.default_params()
    def want_align(lik):
        poses, rec = ax.align(lik, W, H, RES, 0.0, 0.0, FRONT, NEAR5, prm)
        return [poses, np.stack([rec[k] for k in ax.RECORD_INTS], axis=1),
                np.concatenate([rec["score0"][:, None], rec["score"][:, None], rec["H"]], axis=1) + 0.0]       # (+ 0.0: one zero)
    def ask_align(m, pf):
        poses, rec = m.align(FRONT, NEAR5, records=True)
        return _cells([poses, np.stack([rec[k] for k in ax.RECORD_INTS], axis=1),
                       np.concatenate([rec["score0"][:, None], rec["score"][:, None], rec["H"]], axis=1) + 0.0])
    of_field = cached(want_align)
    out["align"] = Consumer(ask_align, lambda log: of_field(g.build_likelihood(np.ascontiguousarray(log, dtype=np.float64).reshape(-1))), False, False, False,
                            of_field)
    return out


@functools.lru_cache(maxsize=None)
def consumers_of(shape):
    return consumers(shape)


CONSUMERS = tuple(consumers_of("64x64"))


def same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


def differing(a, b):
    """cells, records or poses in which two answers differ (an array of another length differs in all of them)"""
    n = 0
    for x, y in zip(a, b):
        if x.shape != y.shape:
            n += max(len(x), len(y))
        elif x.ndim == 2 and x.dtype.names is None and x.dtype != np.float32:      # a field: cells
            n += int((x != y).sum())
        else:                                                                      # records or poses: rows
            if x.dtype.names is not None:
                x, y = x.reshape(-1), y.reshape(-1)
            xb, yb = (np.ascontiguousarray(v).view(np.uint8).reshape(len(v), -1) if len(v) else np.zeros((0, 1), np.uint8) for v in (x, y))
            n += int((xb != yb).any(axis=1).sum())
    return n


@functools.lru_cache(maxsize=None)
def case_of(shape, mover):
    """(before, predicted, prepare, move) of the mover on this shape, the two logs as [H][W] arrays that are not written again"""
    g = grid_of(shape)
    before, predicted, prepare, move = MOVERS[mover].case(g)
    before, predicted = as_grid(g, before).copy(), as_grid(g, predicted).copy()
    before.flags.writeable = predicted.flags.writeable = False
    return before, predicted, prepare, move


# the pairs no request of the consumer can see, whatever it asks: they are not run on the device and not counted as seen
BLIND = frozenset({
    # calculateCombined leaves no cell unknown -- no frontier before (nothing is free) or after -- and, from these walls, no free cell
    # that has not an obstacle of either mode beside it
    ("combine_from", "frontiers"), ("the gms_slam write", "frontiers"),
    ("combine_from", "scatter, rectangle, inflate 1, NOT_FREE"), ("combine_from", "scatter, whole map, inflate 1, OCCUPIED"),
    # one ray frees a line one cell wide: every cell of it has a neighbour that is not free
    ("apply_ray", "scatter, rectangle, inflate 1, NOT_FREE"),
})


def sees(mover, consumer):
    """the consumer's expected answer moves with this mover: a consumer of the field sees the movers that rebuild it, the others every
    true mover but the BLIND pairs"""
    mv, c = MOVERS[mover], consumers_of("64x64")[consumer]
    if not mv.moves or (mover, consumer) in BLIND:
        return False
    return mv.field is not None if c.field else True


def pairs(shape):
    """the (mover, consumer) pairs the device runs: every one but the BLIND"""
    return [(mv, c) for mv in mover_names(shape) for c in CONSUMERS if (mv, c) not in BLIND]
