"""The map queries with ONE PARTICLE'S MAP of a gms_slam handle as their source, at the code-word, plane-word and tile edges: view,
cast, clearance, reach, frontiers, gain, rollout, locate and warp_into on the shapes of tests/test_gpu_query_shapes.py (and 40 x 5:
tests/_slam_query_cases.py), five slots per handle with a log and a pose each (free, unknown, random, second, last column; NaN and
-0.0 among the unknown cells), every result against the plain expectation of that slot's log.  Every comparison is byte for byte.
When a comparison fails, the same request is sent to a shared GridMap holding the same log, and the message says which side of the
source the fault lies on.  What the cases contain is asserted without a device in tests/test_slam_query_inputs.py.

Which device code each handle form reaches (the source-side kernels; the feature units behind them are the shared maps'):
  planes kept (default)      k_slam_plane<true> (clearance, reach, frontiers, gain, rollout, locate), k_cast_slam<true>, k_slam_view,
                             k_slam_codes_from_log behind set_map, k_warp's per-particle source
  GMS_SLAM_EAGER_LIK=1       k_slam_plane<false>, k_cast_slam<false>, k_slam_view from logData alone
  GMS_CAST_WALK=mem          k_cast_slam<false> beside k_slam_plane<true> (cast only)
  generation 1               all of the first row with epoch = 1: the update (k_slam_particle) writes the planes, resample()
                             (k_slam_gather_*) moves logData and planes; asked before any download
  batched                    the first row with slot f * 3 + i and filter f's own epoch words
  the plane limit            k_cast_slam<true> with its largest dynamic LDS (24 576 bytes), k_slam_plane and k_slam_view on rows of
                             390 cells; the <false> forms one step beyond
  likelihood view            k_slam_likelihood_shown (plane 1 at + code_words, stride 2 * code_words) and k_slam_view

The plane limit: a plane is ceil(cells / 16) words and one spare word, rounded up to four (slam_code_words), and is kept up to
24 576 bytes.  390 x 252 cells make 24 576 bytes exactly -- with a ragged last word and rows that start at every even code offset --
and keep their planes; 384 x 256 cells are 24 576 bytes of codes, 24 592 with the spare word, and keep none, as 385 x 256.  All three
run.  No shape is refused by gms_slam_create.  On the batched handle the filters are put into different generations by one
resample_if with a fraction midway between their Neff / n, which the oracle gives and the device's Neff must meet: exactly one draws."""
import numpy as np
import pytest

import _slam_query_cases as sq
import _view_expect as ve
import test_gpu_query_shapes as qs
from _slam_query_cases import N, SHAPES, SLOT_LOGS, Expect, expect_of, poses_of
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch
from test_gpu_query_shapes import RES, _size, log_of
from test_gpu_slam_no_planes import _planes_kept

pytestmark = pytest.mark.gpu

ids = lambda s: f"{s[0]}x{s[1]}"
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- one request, on a particle's map and on a shared map ---------------------------------------------------------------------------------
def _ask(h, which, e, query, params, dst, f):
    """(the canonical result, shown) of one request on particle `which` of handle h; e: the expectation of the map it reads (its seeds
    and cost field are arguments); f: {} or {"filter": f}"""
    shape = e.shape
    if query == "view":
        rect, d, packed = params
        img, shown = h.view(which, rect=rect, decimate=d, packed=packed, **f)
        return (img,), shown
    if query == "cast":
        rec, shown = h.cast(sq.FAN, which=which, **f)
        return (rec,), shown
    if query == "clearance":
        rect, R, not_free = params
        field, shown = h.clearance(which, rect=rect, max_radius=R, not_free=not_free, **f)
        return (field,), shown
    if query == "reach":
        inflate, not_free, max_cost = params
        field, shown = h.reach(which, seeds=e.seeds(not_free), max_cost=max_cost, inflate=inflate, not_free=not_free, **f)
        return (field,), shown
    if query == "frontiers":
        cost = e.answer("reach", sq.REACH_FOR_FRONTIERS, None)[0]
        rec, n, lab, shown = h.frontiers(which, min_size=params[0], cost=cost, labels=True, cap=qs.CAP, **f)
        return (rec, np.array([n], dtype=np.int64), lab), shown
    if query == "gain":
        rec, shown = h.gain(qs.gain_poses_of(shape), qs.PROBES, params[0], which=which, **f)
        return (rec,), shown
    if query == "rollout":
        rec, shown = h.rollout(sq.arcs_of(shape), sq.POINTS, which=which, max_range=255, inflate=params[0], not_free=params[1], **f)
        return (rec,), shown
    if query == "locate":
        (rec, n), shown = h.locate(sq.OFFSETS, which=which, tol=params[0], not_free=False, min_score=1, cap=sq.LOCATE_CAP, free_only=params[1],
                                   full=True, **f)
        return (rec, np.array([n], dtype=np.int64)), shown
    tx, ty, c, s = sq.WARP_POSES[params[0]]
    st, shown = h.warp_into(dst, which, pose=(tx, ty), c=c, s=s, op="compare", **f)
    return (np.asarray(st["pair"]).astype(np.int64).reshape(3, 3), np.array([int(st["n_outside"])], dtype=np.int64)), shown


def _ask_shared(e, pose, query, params, dst):
    """the same request on a shared GridMap that holds e's log: the diagnostic of a failed comparison"""
    m = qs._map(e.shape, max_beams=sq.MAX_BEAMS)
    m.upload_log(e.log)
    try:
        if query == "view":
            return (m.view(params[0], params[1], False, params[2]),)
        if query == "cast":
            return (m.cast(np.asarray(pose, np.float32).reshape(1, 3), sq.FAN)[0],)
        if query == "clearance":
            return (m.clearance(rect=params[0], max_radius=params[1], not_free=params[2]),)
        if query == "reach":
            return (m.reach(e.seeds(params[1]), max_cost=params[2], inflate=params[0], not_free=params[1]),)
        if query == "frontiers":
            rec, n, lab = m.frontiers(min_size=params[0], cost=e.answer("reach", sq.REACH_FOR_FRONTIERS, None)[0], labels=True, cap=qs.CAP)
            return (rec, np.array([n], dtype=np.int64), lab)
        if query == "gain":
            return (m.gain(qs.gain_poses_of(e.shape), qs.PROBES, params[0]),)
        if query == "rollout":
            return (m.rollout(np.asarray(pose, np.float32).reshape(1, 3), sq.arcs_of(e.shape), sq.POINTS, 255, params[0], params[1]),)
        if query == "locate":
            rec, n = m.locate(sq.OFFSETS, tol=params[0], not_free=False, min_score=1, cap=sq.LOCATE_CAP, free_only=params[1], full=True)
            return (rec, np.array([n], dtype=np.int64))
        tx, ty, c, s = sq.WARP_POSES[params[0]]
        st = dst.warp_from(m, (tx, ty), c=c, s=s, op="compare")
        return (np.asarray(st["pair"]).astype(np.int64).reshape(3, 3), np.array([int(st["n_outside"])], dtype=np.int64))
    finally:
        m.close()


def _differ(got, want):
    """None, or where two canonical results differ"""
    if len(got) != len(want):
        return f"{len(got)} arrays for {len(want)}"
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
            return f"array {i}: {a.dtype} {a.shape} for {b.dtype} {b.shape}"
        if a.tobytes() != b.tobytes():
            ra, rb = a.reshape(-1), b.reshape(-1)
            bad = np.flatnonzero((ra.view(np.uint8).reshape(ra.size, -1) != rb.view(np.uint8).reshape(rb.size, -1)).any(axis=1))
            return f"array {i}: {len(bad)} of {ra.size} differ, first at {np.unravel_index(bad[0], a.shape)}: {ra[bad[0]]} != {rb[bad[0]]}"
    return None


def _judge(got, shown, slot, e, pose, query, params, dst, where):
    """one answer of a handle against e's expectation, and the slot it showed; where they differ, the shared map says on which side"""
    at = f"{where}, {query} {params}"
    assert shown == slot, f"{at}: shown {shown}, not {slot}"
    want = e.answer(query, params, pose, sq.warp_dst_log(e.shape) if dst is not None else None)
    bad = _differ(got, want)
    if bad is not None:
        other = _differ(_ask_shared(e, pose, query, params, dst), want)
        side = ("the shared map holding the same log agrees with the expectation: the fault is on the per-particle side" if other is None
                else f"the shared map disagrees with the expectation as well ({other})")
        raise AssertionError(f"{at}: {bad}; {side}")


def _check(h, which, slot, e, pose, dst, where, f=None, reqs=None):
    """every request of one slot against e's expectation; `which` may be "strongest", slot is the handle-wide slot it must show"""
    for query, params in (sq.requests(e.shape) if reqs is None else reqs):
        got, shown = _ask(h, which, e, query, params, dst, f or {})
        _judge(got, shown, slot, e, pose, query, params, dst, f"{where}, which = {which}")


# ---- handles ------------------------------------------------------------------------------------------------------------------------------
def _handle(shape, names=SLOT_LOGS, poses=None):
    """a handle whose slot k holds log_of(shape, names[k]) and stands at poses[k] (the environment is read when it is created).  The
    uploads read back bit for bit, NaN and -0.0 included"""
    s = SLAMParticleMaps(*_size(shape), RES, (0.0, 0.0), num_particles=len(names), max_beams=sq.MAX_BEAMS)
    assert (s.W, s.H) == shape
    for k, name in enumerate(names):
        s.set_map(k, log=log_of(shape, name))
    s.set_poses(poses_of(shape) if poses is None else poses)
    for k, name in enumerate(names):
        assert np.array_equal(bits(s.map_of(k)), bits(log_of(shape, name))), f"{shape}: slot {k} reads back what was uploaded"
    return s


def _all_particles_cast(s, shape, names, poses, where):
    """GMS_CAST_ALL: row k is the single request's result, which is the expectation"""
    rec, shown = s.cast(sq.FAN, which="all")
    assert shown is None and rec.shape == (len(names), len(sq.FAN))
    for k, name in enumerate(names):
        one, sh = s.cast(sq.FAN, which=k)
        assert sh == k and rec[k].tobytes() == one.tobytes(), f"{where}: row {k} of the all-particles cast"
        bad = _differ((one,), expect_of(shape, name).answer("cast", (), poses[k]))
        assert bad is None, f"{where}, slot {k}, cast: {bad}"


def _every_slot(shape, reqs=None, where=""):
    s = _handle(shape)
    dst = qs._map(shape)
    dst.upload_log(sq.warp_dst_log(shape))
    try:
        for k, name in enumerate(SLOT_LOGS):
            _check(s, k, k, expect_of(shape, name), poses_of(shape)[k], dst, f"{shape}{where}, slot {k} ({name})", reqs=reqs)
        _all_particles_cast(s, shape, SLOT_LOGS, poses_of(shape), f"{shape}{where}")
        for k, name in enumerate(SLOT_LOGS):
            assert np.array_equal(bits(s.map_of(k)), bits(log_of(shape, name))), "a request changes no map"
    finally:
        s.close(); dst.close()


# ---- the forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_class_planes_kept(shape):
    assert _planes_kept(*_size(shape), RES, max_beams=sq.MAX_BEAMS)
    _every_slot(shape)


@pytest.mark.parametrize("shape", sq.EAGER_SHAPES, ids=ids)
def test_no_class_planes(shape, monkeypatch):
    monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")
    assert not _planes_kept(*_size(shape), RES, max_beams=sq.MAX_BEAMS)
    _every_slot(shape, where=", GMS_SLAM_EAGER_LIK=1")


@pytest.mark.parametrize("shape", sq.WALK_MEM_SHAPES, ids=ids)
def test_cast_walks_memory_beside_the_planes(shape, monkeypatch):
    monkeypatch.setenv("GMS_CAST_WALK", "mem")
    assert _planes_kept(*_size(shape), RES, max_beams=sq.MAX_BEAMS)
    _every_slot(shape, reqs=[("cast", ())], where=", GMS_CAST_WALK=mem")


def _strongest(s, shape, exps, poses, dst, where, f=None, base=0):
    """the strongest particle, picked on the device: it shows the slot view() shows, and answers as that slot"""
    shown = s.view("strongest", **(f or {}))[1]
    assert base <= shown < base + len(exps)
    _check(s, "strongest", shown, exps[shown - base], poses[shown - base], dst, where, f=f)
    return shown


@pytest.mark.parametrize("shape", sq.GEN1_SHAPES, ids=ids)
def test_generation_one(shape):
    """one update (the weights differ, the maps are written), a resampling that moves maps, then every request of every slot before
    anything is downloaded: the answers are those of the maps downloaded afterwards, which are the maps in front of the draw, moved"""
    r01, want_idx, _ = sq.resampling_draw(shape)
    s = _handle(shape)
    dst = qs._map(shape)
    dst.upload_log(sq.warp_dst_log(shape))
    try:
        s.update(sq.SCAN, None)
        before = [s.map_of(k) for k in range(N)]
        idx, _ = s.resample(r01, want_indices=True)
        assert np.array_equal(idx, want_idx), f"{shape}: the draw {r01} gives {idx.tolist()}, the oracle {want_idx.tolist()}"
        poses = poses_of(shape)[idx]                                           # (a particle moves with its pose)
        src = {int(j): Expect(shape, before[j]) for j in set(idx.tolist())}     # (the expectation of a map is made once, however many slots hold it)
        got = {}
        for k in range(N):
            got[k] = [_ask(s, k, src[int(idx[k])], q, p, dst, {}) for q, p in sq.requests(shape)]
        all_rec = s.cast(sq.FAN, which="all")[0]
        strongest = _ask(s, "strongest", src[int(idx[0])], "view", (None, 1, False), dst, {})
        assert np.array_equal(s.pf.get_poses(), poses)
        after = [s.map_of(k) for k in range(N)]
        for k in range(N):
            assert np.array_equal(bits(after[k]), bits(before[idx[k]])), f"{shape}: slot {k} holds the map of particle {idx[k]}"
        assert any(not np.array_equal(bits(after[k]), bits(before[k])) for k in range(N)), "a slot's map changed"
        exps = [src[int(idx[k])] for k in range(N)]                           # (bit-equal to the maps downloaded afterwards: just asserted)
        for k in range(N):
            for (q, p), (res, shown) in zip(sq.requests(shape), got[k]):
                _judge(res, shown, k, exps[k], poses[k], q, p, dst, f"{shape}, generation 1, slot {k} (from {idx[k]})")
            assert all_rec[k].tobytes() == got[k][[q for q, _ in sq.requests(shape)].index("cast")][0][0].tobytes(), f"{shape}: row {k} of the all-particles cast"
        sh = strongest[1]
        assert 0 <= sh < N and _differ(strongest[0], exps[sh].answer("view", (None, 1, False), None)) is None, f"{shape}: the strongest particle's view"
        _strongest(s, shape, exps, poses, dst, f"{shape}, generation 1")
    finally:
        s.close(); dst.close()


def test_batched_handle():
    shape, S, n = sq.BATCH_SHAPE, sq.BATCH_FILTERS, sq.BATCH_N
    bat = SLAMParticleMapsBatch(S, *_size(shape), RES, (0.0, 0.0), num_particles=n, max_beams=sq.MAX_BEAMS)
    dst = qs._map(shape)
    dst.upload_log(sq.warp_dst_log(shape))
    try:
        assert (bat.W, bat.H) == shape
        for f in range(S):
            for i in range(n):
                bat.set_map(f, i, log=log_of(shape, sq.BATCH_LOGS[f][i]))
        bat.set_poses(sq.batch_poses())
        for f in range(S):
            for i in range(n):
                assert np.array_equal(bits(bat.map_of(f, i)), bits(log_of(shape, sq.BATCH_LOGS[f][i])))
                _check(bat, i, f * n + i, expect_of(shape, sq.BATCH_LOGS[f][i]), sq.batch_poses()[f, i], dst, f"batched, filter {f}, particle {i}",
                       f={"filter": f})
        # one update, then one resample_if that only the filter with the smaller Neff meets (the builder's fraction, from the oracle):
        # the filters sit in different generations
        want_neff, frac = sq.batch_draw()
        neff = bat.update([sq.SCAN, sq.SCAN], None)
        assert (np.abs(neff - want_neff) <= 1e-11 * want_neff).all(), (neff, want_neff)
        before = bat.maps()
        bat.resample_if([0.35, 0.65], frac)
        did = bat.did_resample()
        assert did.sum() == 1 and np.array_equal(did, want_neff < frac * n), (neff, frac, did)
        idx = bat.last_resample_indices()
        poses = np.stack([sq.batch_poses()[f][idx[f]] if did[f] else sq.batch_poses()[f] for f in range(S)])
        origin = lambda f, i: int(idx[f, i]) if did[f] else i
        src = {(f, j): Expect(shape, before[f, j]) for f in range(S) for j in {origin(f, i) for i in range(n)}}
        got = {(f, i): [_ask(bat, i, src[f, origin(f, i)], q, p, dst, {"filter": f}) for q, p in sq.requests(shape)] for f in range(S) for i in range(n)}
        after = bat.maps()
        for f in range(S):
            exps = [src[f, origin(f, i)] for i in range(n)]
            for i in range(n):
                assert np.array_equal(bits(after[f, i]), bits(before[f, origin(f, i)])), (f, i)
                for (q, p), (res, shown) in zip(sq.requests(shape), got[f, i]):
                    _judge(res, shown, f * n + i, exps[i], poses[f, i], q, p, dst, f"batched, filter {f} ({'drew' if did[f] else 'did not draw'}), particle {i}")
            _strongest(bat, shape, exps, poses[f], dst, f"batched, filter {f}", f={"filter": f}, base=f * n)
    finally:
        bat.close(); dst.close()


@pytest.mark.parametrize("shape, kept", list(zip(sq.LIMIT_SHAPES, (True, False, False))), ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_the_plane_limit(shape, kept):
    assert _planes_kept(*_size(shape), RES, max_beams=sq.MAX_BEAMS) == kept
    poses = sq.limit_poses(shape)
    s = _handle(shape, names=sq.LIMIT_LOGS, poses=poses)
    try:
        _all_particles_cast(s, shape, sq.LIMIT_LOGS, poses, f"{shape}")
        for k, name in enumerate(sq.LIMIT_LOGS):
            _check(s, k, k, expect_of(shape, name), poses[k], None, f"{shape}, slot {k} ({name})", reqs=[r for r in sq.limit_requests(shape) if r[0] != "cast"])
    finally:
        s.close()


@pytest.mark.parametrize("shape", sq.GEN1_SHAPES, ids=ids)
def test_likelihood_view_from_plane_one(shape):
    """after one update and before any download -- slots 2 and 4 (the last particle), grey and packed, and the strongest particle, all
    taken first --: the likelihood view is the render of the field a download returns then,
    that field is the oracle's, and a twin that never asked ends with the same bytes.  The reference makes the field in front of the
    integration (SLAM.java:93 runs before :105): it is the field of the logData the update started from -- the uploaded log, read
    back bit for bit by _handle -- and the oracle's filter (orc.Slam) behind the same update holds it; likelihoodData compares
    for equality, as in tests/test_gpu_slam_particle_maps.py"""
    g, o = qs._grid(shape), sq.oracle_after_update(shape)
    a, b = _handle(shape), _handle(shape)
    try:
        for s in (a, b):
            s.update(sq.SCAN, None)
        # every view first: the first download of a field writes every particle's (the handle's fields are then in memory, and a
        # view reads the array instead of plane 1)
        views = {(k, packed): a.view(k, likelihood=True, packed=packed) for k in (2, 4) for packed in (False, True)}
        first = a.view("strongest", likelihood=True)
        assert first[1] == a.last_stats["strongest"]
        for k in (2, 4):
            lik, log = a.map_of(k, likelihood=True), a.map_of(k)
            for packed, (img, shown) in ((packed, views[k, packed]) for packed in (False, True)):
                want = ve.expect(ve.idx_map(lik, True), (0, 0) + shape, 1, True, packed)
                assert shown == k and img.dtype == want.dtype and np.array_equal(img, want), f"{shape}: slot {k}, likelihood view, packed = {packed}"
            assert np.array_equal(lik.reshape(-1), o.lik(k)), f"{shape}: slot {k}, likelihoodData: {int((lik.reshape(-1) != o.lik(k)).sum())} cells differ"
            assert np.array_equal(o.lik(k), g.build_likelihood(np.array(log_of(shape, SLOT_LOGS[k])).reshape(-1))), "... the field of the uploaded log"
            assert np.array_equal(log != 0, o.log(k).reshape(log.shape) != 0), f"{shape}: slot {k}: the update touched the oracle's cells"
            assert len(np.unique(lik)) > 1 or not (log > 0).any()
        want = ve.expect(ve.idx_map(a.map_of(first[1], likelihood=True), True), (0, 0) + shape, 1, True, False)
        assert np.array_equal(first[0], want), f"{shape}: the strongest particle's likelihood view, in front of any download"
        img, shown = a.view("strongest", likelihood=True)                       # ... and a later one, from the array
        assert shown == first[1] and np.array_equal(img, want)
        for s in (a, b):
            s.update(sq.SCAN2, None)
        (Pa, wa), (Pb, wb) = a.get_particles(), b.get_particles()
        assert np.array_equal(Pa, Pb) and np.array_equal(bits(wa), bits(wb))
        assert np.array_equal(bits(a.maps()), bits(b.maps())) and np.array_equal(bits(a.maps(likelihood=True)), bits(b.maps(likelihood=True)))
    finally:
        a.close(); b.close()
