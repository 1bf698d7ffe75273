"""Every map query behind everything that moves the shared map's logData.  The map keeps three things derived from logData until it
moves -- the OCCUPIED bit plane, the NOT_FREE bit plane and the seeding table --, and one transition (map_planes_stale) invalidates all
three; a path that writes logData and misses it answers from the map as it was, with any tolerance and without a fault.
tests/test_gpu_cast_edges.py holds that for gms_map_cast; here every consumer of tests/_mover_cases.py is asked before and after every
mover.  Expectations are the suite's own modules on constructed or downloaded logData, every comparison is on bytes; that a stale answer
would differ is held on the host by tests/test_mover_inputs.py.  The NOT_FREE plane has no build counter: there the answers alone decide."""
import numpy as np
import pytest

import _beams_expect as bx
import _clearance_expect as xe
import _frontier_expect as fx
import _gain_expect as gx
import _mover_cases as mc
import _reach_expect as rx
import _rollout_expect as ro
import _scatter_expect as sx
from gridmap_slam_robot_amd import ParticleFilter
from test_gpu_cast_edges import BACK, FRONT, LEFT, POSE5, RIGHT, _scanned

pytestmark = pytest.mark.gpu


class _Case:
    """the map of a mover's case with logData `before` in it, the mover prepared, and the consumers' filter"""

    def __init__(self, shape, mover, monkeypatch, n_pf=mc.N_PF):
        self.mv, self.g = mc.MOVERS[mover], mc.grid_of(shape)
        self.before, self.predicted, prepare, self._move = mc.case_of(shape, mover)
        for k, v in (self.mv.env or {}).items():
            monkeypatch.setenv(k, v)                   # read when a map is created
        if self.mv.slam:
            self.ctx = prepare(None)
            self.m = self.ctx.grid_map
        else:
            self.m = mc.map_of(self.g)
        for k in self.mv.env or {}:
            monkeypatch.delenv(k)
        if prepare == "two updates first":
            self.m.update(BACK, POSE5); self.m.update(BACK, POSE5)
            self.ctx = None
        elif not self.mv.slam:
            if (self.before != 0).any() and not self.mv.fresh:            # (fresh: prepare makes `before` by updates of its own)
                self.m.upload_log(self.before)
            self.ctx = prepare(self.m)
        self.pf = ParticleFilter(self.m, n_pf)

    def move(self):
        self._move(self.m, self.ctx)

    def builds(self):
        return self.m.cast_plane_builds(), self.m.scatter_table_builds()

    def close(self):
        self.pf.close()
        if self.ctx is not None:
            self.ctx.close()
        if not self.mv.slam:
            self.m.close()


def _same(got, want, where):
    assert mc.same(got, want), f"{where}: {mc.differing(got, want)} cells, records or poses differ"


def _field_consumer_after_a_mover(k, c, mover):
    """a consumer of likelihoodData: behind a mover that rebuilds or replaces the field it answers from the new field -- the lazy
    field a deferred step leaves is brought up to date by the request itself --, behind every other mover its answer stays"""
    first = c.ask(k.m, k.pf)
    _same(first, c.field(k.m.download_likelihood()), f"before {mover}: against the expectation on the downloaded field")
    built = k.builds()
    k.move()
    second = c.ask(k.m, k.pf)                          # (before anything is downloaded: the request has to bring the field up to date)
    log, lik = k.m.download_log(), k.m.download_likelihood()
    _same(second, c.field(lik), f"after {mover}: against the expectation on the downloaded field")
    if k.mv.field is None:
        _same(second, first, f"{mover} leaves the field as it is")
    else:
        assert mc.differing(second, first) >= mc.MARGIN, "the answers of the field as it was are others"
        assert np.array_equal(lik.reshape(-1), k.g.build_likelihood(log.reshape(-1))), "the field is the field of the moved logData"
        if k.mv.field == "exact" and k.mv.exact:
            _same(second, c.expect(k.predicted), f"after {mover}: against the expectation on the field of the predicted logData")
    _same(c.ask(k.m, k.pf), second, "the same request again")
    assert k.builds() == built, "a consumer of the field packs no plane and builds no table"


@pytest.mark.parametrize("shape, mover, consumer", [(s, mv, c) for s in mc.SHAPES for mv, c in mc.pairs(s)])
def test_a_query_after_a_mover_answers_from_the_moved_map(shape, mover, consumer, monkeypatch):
    c = mc.consumers_of(shape)[consumer]
    k = _Case(shape, mover, monkeypatch)
    if c.field:
        _field_consumer_after_a_mover(k, c, mover)
        k.close()
        return
    first = c.ask(k.m, k.pf)                           # builds the plane or the table
    _same(first, c.expect(k.before), f"before {mover}")
    built = k.builds()
    k.move()
    assert k.builds() == built, "a mover packs no plane and builds no table"
    second = c.ask(k.m, k.pf)
    log = k.m.download_log()
    _same(second, c.expect(log), f"after {mover}: against the expectation on the downloaded logData")
    if k.mv.exact:                                     # (a weighted mean of sixteen equal poses is equal up to rounding only)
        _same(second, c.expect(k.predicted), f"after {mover}: against the expectation on the logData the oracle predicted")
    third = c.ask(k.m, k.pf)
    _same(third, second, "the same request again")
    stale = k.mv.moves or k.mv.repacks
    planes, tables = k.builds()
    assert planes - built[0] == (1 if stale and c.occupied else 0), "the OCCUPIED plane of the moved map is packed once, for the second answer"
    assert tables - built[1] == (1 if stale and c.table else 0), "the table of the moved map is built once, for the second answer"
    k.close()


# ---- both planes at once ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mover", ["upload_log", "update, deferred", "slam_update_dev twice"])
def test_neither_plane_is_served_from_the_other_ones_stale_state(mover, monkeypatch):
    k = _Case("64x64", mover, monkeypatch)
    occ = lambda: (k.m.clearance(None, 8, False), k.m.reach([mc.CELL5], inflate=2, not_free=False))
    nf = lambda: (k.m.clearance(None, 8, True), k.m.reach([mc.CELL5], inflate=2, not_free=True))
    want = lambda log, mode: (xe.expect(log, 8, mode), rx.expect(log, [mc.CELL5], inflate=2, not_free=mode))
    for mode in (False, True):
        assert mc.differing(want(k.before, mode), want(k.predicted, mode)) >= mc.MARGIN
    a, b = occ(), nf()
    _same(a, want(k.before, False), "OCCUPIED before"); _same(b, want(k.before, True), "NOT_FREE before")
    k.move()
    b, a = nf(), occ()                                 # the other order
    log = k.m.download_log().reshape(k.g.H, k.g.W)
    _same(b, want(log, True), f"NOT_FREE first after {mover}"); _same(a, want(log, False), f"OCCUPIED second after {mover}")
    k.move()                                           # and once more, the OCCUPIED plane first
    a, b = occ(), nf()
    log = k.m.download_log().reshape(k.g.H, k.g.W)
    _same(a, want(log, False), "OCCUPIED first"); _same(b, want(log, True), "NOT_FREE second")
    k.close()


# ---- a batched handle ------------------------------------------------------------------------------------------------------------------
N_B = 64
POSES3 = np.stack([POSE5, mc.NEAR5[1], mc.NEAR5[3]])
SCANS3 = np.stack([FRONT, BACK, FRONT])


def _ask_batched(m, pf, n_maps):
    pf.set_poses(np.zeros((n_maps, N_B, 3), np.float32) if n_maps > 1 else np.zeros((N_B, 3), np.float32))
    M = np.atleast_1d(pf.scatter(inflate=1, seed=mc.SEED, sequence=mc.SEQ, want_count=True))
    drawn = pf.get_poses().reshape(n_maps, N_B, 3)
    out = []
    for mi in range(n_maps):
        rec, n, lab = m.frontiers(min_size=1, labels=True, mi=mi)
        out.append(mc._cells([m.clearance(None, 8, False, mi=mi), m.clearance(None, 8, True, mi=mi), m.reach([mc.CELL5], inflate=2, not_free=True, mi=mi),
                              rec, np.array([n]), lab, m.gain(mc.NEAR5, mc.RING, 16, mi=mi), m.rollout(mc.ROLL_POSES, mc.ARCS, None, 255, 1, True, mi=mi),
                              m.clearance_poses(mc.NEAR5, 8, True, mi=mi), drawn[mi], M[mi:mi + 1]]))
    return out


def _want_batched(g, log, mi):
    log = mc.as_grid(g, log)
    rec, n, lab = fx.expect(log, min_size=1)
    poses, _, M = sx.expect(log, (0.0, 0.0), mc.RES, 0, N_B, mc.SEED, mc.SEQ, inflate=1, not_free=True, mi=mi)
    return mc._cells([xe.expect(log, 8, False), xe.expect(log, 8, True), rx.expect(log, [mc.CELL5], inflate=2, not_free=True), rec, np.array([n]), lab,
                      gx.expect_poses(g, log, mc.RING, mc.NEAR5, 16),
                      ro.expect(ro.Geometry(g.W, g.H, mc.RES, 0.0, 0.0), log, mc.ROLL_POSES, mc.ARCS, np.zeros((0, 2), np.float32), 255, 1, True),
                      xe.expect_poses(xe.expect(log, 8, True), mc.NEAR5, 0.0, 0.0, mc.RES), np.zeros((N_B, 3), np.float32) if M == 0 else poses,
                      np.array([M])])


BEFORE3 = np.stack([BACK, np.concatenate([RIGHT, RIGHT]), np.concatenate([LEFT, LEFT])])      # what the three maps hold before: 64 beams each


def _fused3(pf16, scans, r01):
    """a batched fused step that resamples below 0.9 n: its tail is paired with the resample and its apply pass stays owed"""
    pf16.slam_update(np.stack([np.tile(p, (16, 1)) for p in POSES3]), scans, r01, mc.FRACTION, True)


def _batched_movers(g):
    walls = np.stack([_scanned(g, FRONT), _scanned(g, LEFT), _scanned(g, RIGHT)])
    def fused(m, pf16):                                # the second step's launches carry the first one's apply pass; its own is owed
        _fused3(pf16, SCANS3, [0.3, 0.5, 0.7])
        _fused3(pf16, SCANS3[::-1].copy(), [0.6, 0.2, 0.4])
    return {"upload_log of all three": lambda m, pf16: m.upload_log(walls), "batched update": lambda m, pf16: m.update(SCANS3, POSES3),
            "two batched fused steps": fused}


@pytest.mark.parametrize("mover", ["upload_log of all three", "batched update", "two batched fused steps"])
def test_every_map_of_a_batched_handle_answers_from_its_own_moved_map(mover):
    g = mc.grid_of("64x64")
    m = mc.map_of(g, n_maps=3)
    m.update(BEFORE3, np.tile(POSE5, (3, 1))); m.update(BEFORE3, np.tile(POSE5, (3, 1)))           # the steady state: a field exists, steps pair
    before = m.download_log()
    assert all(np.array_equal(np.sign(before[mi].reshape(-1)), np.sign(_scanned(g, BEFORE3[mi], BEFORE3[mi]))) for mi in range(3))
    pf, pf16 = ParticleFilter(m, N_B), ParticleFilter(m, 16)
    first = _ask_batched(m, pf, 3)
    for mi in range(3):
        _same(first[mi], _want_batched(g, before[mi], mi), f"map {mi} before")
    built = m.cast_plane_builds(), m.scatter_table_builds()
    _batched_movers(g)[mover](m, pf16)
    assert (m.cast_plane_builds(), m.scatter_table_builds()) == built
    second = _ask_batched(m, pf, 3)
    assert (m.cast_plane_builds(), m.scatter_table_builds()) == (built[0] + 1, built[1] + 1), "one pre-pass and one table hold every map's part"
    logs = m.download_log()
    for mi in range(3):
        want = _want_batched(g, logs[mi], mi)
        changed = mc.differing(want, _want_batched(g, before[mi], mi))
        print(f"{mover}, map {mi}: {changed} cells, records or poses change")
        assert changed >= mc.MARGIN and mc.differing(want[-2:], _want_batched(g, before[mi], mi)[-2:]) >= mc.MARGIN, "the mover changes this map's answers and its draw"
        _same(second[mi], want, f"map {mi} after {mover}")
    assert all(mc.differing(second[i][-2:], second[j][-2:]) >= mc.MARGIN for i, j in ((0, 1), (0, 2), (1, 2))), "every map's draw is its own"
    pf.close(); pf16.close(); m.close()


def test_a_single_map_combined_from_a_moved_batch():
    g = mc.grid_of("64x64")
    batch, single = mc.map_of(g, n_maps=3), mc.map_of(g)
    pf = ParticleFilter(single, N_B)
    pf16 = ParticleFilter(batch, 16)
    batch.update(BEFORE3, np.tile(POSE5, (3, 1))); batch.update(BEFORE3, np.tile(POSE5, (3, 1)))
    single.combine_from(batch)
    first = _ask_batched(single, pf, 1)[0]
    _same(first, _want_batched(g, single.download_log(), 0), "combined once")
    built = single.cast_plane_builds(), single.scatter_table_builds()
    _fused3(pf16, SCANS3, [0.3, 0.5, 0.7])             # the batch moves: the step's apply pass is owed when the combination reads it
    single.combine_from(batch)
    assert (single.cast_plane_builds(), single.scatter_table_builds()) == built
    second = _ask_batched(single, pf, 1)[0]
    log = single.download_log()
    want = _want_batched(g, log, 0)
    assert mc.differing(want, first) >= mc.MARGIN
    _same(second, want, "combined from the moved batch")
    pf.close(); pf16.close(); single.close(); batch.close()


# ---- what moves nothing ----------------------------------------------------------------------------------------------------------------
def test_what_moves_nothing_changes_no_answer_and_builds_nothing():
    g = mc.grid_of("64x64")
    cons = mc.consumers_of("64x64")
    wall = mc.as_grid(g, _scanned(g, LEFT))
    m, other = mc.map_of(g), mc.map_of(g)
    m.upload_log(wall); other.upload_log(_scanned(g, FRONT))
    m.compute_likelihood_map()                         # the field of the wall: what the consumer of likelihoodData answers from
    pf, scored = ParticleFilter(m, mc.N_PF), ParticleFilter(m, 16)
    scored.set_poses(np.tile(POSE5, (16, 1)))
    table = "scatter, whole map"
    kept = [c for c in mc.CONSUMERS if not cons[c].table] + [table]            # (another scatter request would rebuild the table by itself)
    assert sum(cons[c].not_free for c in kept) >= 7
    for c in [c for c in mc.CONSUMERS if c not in kept] + kept:
        _same(cons[c].ask(m, pf), cons[c].expect(wall), f"settled: {c}")
    built = m.cast_plane_builds(), m.scatter_table_builds()
    def score():
        scored.score(FRONT); scored.normalize()
    ops = (("download_log", m.download_log), ("download_likelihood", m.download_likelihood), ("view", m.view), ("score + normalize", score),
           ("trace_ray", lambda: m.trace_ray(32.5, 32.5, 50.5, 32.5)), ("a compare-only warp", lambda: m.warp_from(other, (mc.RES, 0.0), c=1.0, s=0.0, op="compare")),
           ("a compare-only warp without counts", lambda: m.warp_from(other, (0.0, 0.0), c=1.0, s=0.0, op="compare", stats=False)),
           ("the same requests again", lambda: None))
    for name, op in ops:
        op()
        for c in [table] + kept[:-1]:
            _same(cons[c].ask(m, pf), cons[c].expect(wall), f"after {name}: {c}")
            assert (m.cast_plane_builds(), m.scatter_table_builds()) == built, f"{name} moved no logData: {c} packs and builds nothing"
    assert np.array_equal(m.download_log().view(np.uint64), wall.view(np.uint64))
    pf.close(); scored.close(); other.close(); m.close()


# ---- a filter's pending state across a mover --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mover", ["upload_log", "update, deferred", "slam_update_dev twice"])
def test_a_pending_score_across_a_mover(mover, monkeypatch):
    """score() leaves its weights pending; the map moves; score_beams and a scatter of some slots follow.  "A twin that never saw the
    mover" is read as: a twin filter on a twin map that was moved the same way before that filter did anything -- its state crossed no
    mover -- and the two are equal.  Independently of the twin, the slots the scatter left alone carry the weights _beams_expect gives
    for the moved map, which are not those of the map as it was."""
    n, first, count = 256, 100, 50
    a, b = _Case("64x64", mover, monkeypatch, n_pf=n), _Case("64x64", mover, monkeypatch, n_pf=n)
    poses = np.tile(mc.POSES16, (n // 16, 1))
    a.pf.set_poses(poses)
    a.pf.score(FRONT)                                  # pending: not normalised
    a.move()
    b.move()
    b.pf.set_poses(poses)
    got = []
    for k in (a, b):
        k.pf.score_beams(mc.ALL_ROUND, mc.FACTORS, mc.BEHIND, mc.AHEAD)
        assert k.pf.scatter(first=first, count=count, seed=mc.SEED, sequence=mc.SEQ, want_count=True) > 0
        got.append((k.pf.get_poses(), k.pf.get_weights(), k.pf.get_log_weights()))
    _same(got[0], got[1], "the filter with a pending score against its twin")
    log = a.m.download_log()
    assert np.array_equal(log.view(np.uint64), b.m.download_log().view(np.uint64))
    w, lw, _ = bx.expect(a.g, log, mc.ALL_ROUND, mc.POSES16, mc.FACTORS, mc.BEHIND, mc.AHEAD)
    stale, _, _ = bx.expect(a.g, a.before, mc.ALL_ROUND, mc.POSES16, mc.FACTORS, mc.BEHIND, mc.AHEAD)
    assert (w != stale).sum() >= mc.MARGIN, "the weights of the map as it was are others"
    keep = np.r_[0:first, first + count:n]
    assert bx.same_bits(got[0][1][keep], np.tile(w, n // 16)[keep]) and bx.same_bits(got[0][2][keep], np.tile(lw, n // 16)[keep]), "the untouched slots' weights"
    assert bx.same_bits(got[0][1][first:first + count], np.full(count, 1.0 / n)), "the scattered slots' weights"
    want, _, _ = sx.expect(log, (0.0, 0.0), mc.RES, first, count, mc.SEED, mc.SEQ)
    assert np.array_equal(got[0][0][first:first + count].view(np.uint32), want.view(np.uint32)) and np.array_equal(got[0][0][keep], poses[keep])
    a.close(); b.close()
