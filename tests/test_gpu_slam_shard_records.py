"""The record movers of a sharded gms_slam -- gms_slam_shard_draw / gms_slam_shard_export (k_slam_export_records) / gms_slam_shard_gather
(k_slam_shard_gather) -- driven directly, one rank, single thread, at the edges tests/_shard_record_cases.py lists: records under one
workgroup pass, of exactly one chunk and of one chunk plus one double, odd cell counts, the plane limit; export lists that are empty,
whole, reversed and repeating; gather plans with every slot remote, every slot local and no buffer, and a receive buffer out of order
with a record twice; draw after draw, so that the "previous" generation is either buffer in turn; a draw that does not draw.

Every comparison is bit for bit, doubles as uint64.  What a record must hold is said three ways: logData by the download before the
draw; the planes by a plain restatement of the class plane (pack_planes) AND by a second handle that reaches the same planes through
another kernel; the gathered maps by the downloads before the draw and by a stand-alone gms_slam of the same 256 particles, fed the
same maps, poses, scans, seeds and r01."""
import ctypes as C

import numpy as np
import pytest
import torch

import _shard_record_cases as sc
from gridmap_slam_robot_amd import SLAMParticleMaps, _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GMS_OK, GmsError
from gridmap_slam_robot_amd.distributed import ShardedParticleFilter, ShardedSlamParticleMaps, SlamShardOps
from oracle import oracle as orc

from _thread_collectives import ThreadWorld

pytestmark = pytest.mark.gpu

N = sc.N
MAX_BEAMS = 32
GUARD = 64                                                 # doubles in front of and behind an export's destination
SENTINEL = float(np.array(0x7FF8DEADBEEF0001, dtype=np.uint64).view(np.float64))     # a NaN no kernel here writes
U = (0.01, 0.005)                                          # odometry of every update: the motion draw runs, keyed by the global index
SMALL = (41, 41)

shapes = pytest.mark.parametrize("shape", list(sc.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")


def _scan(k):
    """two hand-made scans of twelve beams, 0.15 .. 1.3 m, hits and misses, taken in turn"""
    ang = np.arange(12) * (2 * np.pi / 12) + 0.1 + 0.37 * (k % 2)
    dist = 0.15 + 1.15 * ((np.arange(12) * 5 + 3 * (k % 2)) % 12) / 11
    hit = (np.arange(12) % 4 != 2).astype(np.uint8)
    return orc.make_beams(dist * np.cos(ang), dist * np.sin(ang), dist, hit)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(got, want, where):
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape)
    g, w = _u64(got), _u64(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{where}: {len(bad)} of {w.size} differ, first at {bad[0].tolist()}")


def _shard(shape):
    torch.cuda.set_device(0)
    ops = SlamShardOps(*sc.size_of(shape), sc.RES, (0.0, 0.0), N, 0, N, max_beams=MAX_BEAMS)
    assert (ops.slam.W, ops.slam.H) == shape and ops.record_doubles == sc.SHAPES[shape][2]
    return ops


def _put_maps(handle, logs):
    for i in range(N):
        handle.set_map(i, log=logs[i])                     # gms_slam_upload_map: logData, and plane 0 behind it by k_slam_codes_from_log


def _epoch(ops):
    """draws that drew so far: every one copies N maps (gms_slam_copies)"""
    c = ops.slam.maps_copied()
    assert c % N == 0
    return c // N


def _maps(handle, lik=True):
    """(logData [N][cells], likelihoodData [N][cells]) of the current generation"""
    return handle.maps().reshape(N, -1), (handle.maps(likelihood=True).reshape(N, -1) if lik else None)


def _export(ops, idx, dst_records=None):
    """gms_slam_shard_export into a tensor with GUARD doubles of SENTINEL on either side: (rc, records [count][rec] as numpy, guards intact)"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    rec = ops.record_doubles
    count = idx.size if dst_records is None else dst_records
    buf = torch.full((2 * GUARD + count * rec,), SENTINEL, dtype=torch.float64, device=ops.device)
    torch.cuda.synchronize()
    rc = _lib.load().gms_slam_shard_export(ops.slam._h, _lib.ptr(idx) if idx.size else None, int(idx.size), C.c_void_p(buf.data_ptr() + 8 * GUARD))
    ops.synchronize()
    host = buf.cpu().numpy()
    guard = np.full(GUARD, SENTINEL).view(np.uint64)
    intact = np.array_equal(host[:GUARD].view(np.uint64), guard) and np.array_equal(host[GUARD + count * rec:].view(np.uint64), guard)
    return rc, host[GUARD:GUARD + count * rec].reshape(count, rec), intact


def _untouched(records):
    return bool((records.view(np.uint64) == np.array(SENTINEL).view(np.uint64)).all())


def _gather_rc(ops, src_local, recv_pos, recv):
    a, b = np.ascontiguousarray(src_local, dtype=np.int32), np.ascontiguousarray(recv_pos, dtype=np.int32)
    rc = _lib.load().gms_slam_shard_gather(ops.slam._h, _lib.ptr(a), _lib.ptr(b), C.c_void_p(recv.data_ptr()) if recv is not None else None)
    ops.synchronize()
    return rc


class Pair:
    """a shard that is the whole population (SlamShardOps, updated and normalised through ShardedSlamParticleMaps over a world of one)
    beside a stand-alone SLAMParticleMaps: the same maps, the same poses"""

    def __init__(self, shape, stand_alone=True):
        self.shape, self.k = shape, 0
        self.ops = _shard(shape)
        self.f = ShardedSlamParticleMaps(N, self.ops, coll=ThreadWorld(1).comm(0))
        self.ref = SLAMParticleMaps(*sc.size_of(shape), sc.RES, (0.0, 0.0), num_particles=N, max_beams=MAX_BEAMS) if stand_alone else None
        for h in (self.ops.slam, self.ref):
            if h is not None:
                _put_maps(h, sc.logs_of(shape))
                h.set_poses(sc.poses_of(shape))

    def update(self):
        """one update on both; everything the two hold must be equal afterwards.  Returns the shard's (logData, likelihoodData)"""
        z, k = _scan(self.k), self.k
        self.k += 1
        neff = self.f.update(z, U, seed=5, sequence=k)
        log, lik = _maps(self.ops.slam)
        if self.ref is not None:
            assert self.ref.update(z, U, seed=5, sequence=k) == neff, k
            assert self.f.stats()["strongest"] == self.ref.strongest and np.array_equal(self.f.weighted_pose(), self.ref.get_weighted_pose()), k
            self.same_particles(f"update {k}")
            rlog, rlik = _maps(self.ref)
            _same(log, rlog, f"update {k}: logData, shard against stand-alone")
            _same(lik, rlik, f"update {k}: likelihoodData, shard against stand-alone")
        return log, lik

    def same_particles(self, where):
        (P, w), (Pr, wr) = self.ops.slam.get_particles(), self.ref.get_particles()
        _same(P, Pr, where + ": poses")
        _same(w, wr, where + ": weights")

    def close(self):
        self.ops.slam.close()
        if self.ref is not None:
            self.ref.close()


# ---- export ---------------------------------------------------------------------------------------------------------------------------------
@shapes
def test_export_writes_the_records_of_the_generation_the_draw_left_behind(shape):
    """Handle A: maps uploaded, ONE update, a draw.  Its records' planes were reached by the update: plane 1 is the copy k_slam_particle
    stores of the plane it staged (the logData the update started from), plane 0 what its apply pass wrote back where a cell changed
    class.  Handle B holds the same logs by upload alone: its plane 0 comes from k_slam_codes_from_log -- once for the logs A started
    from, once for the logs A's update left.  Both must equal the plain restatement (pack_planes) as well."""
    cells, cw, rec = sc.SHAPES[shape]
    logs0 = sc.logs_of(shape)
    a = Pair(shape, stand_alone=False)
    try:
        assert a.ops.record_doubles == rec
        pre_log, _ = a.update()
        assert _u64(pre_log).tobytes() != _u64(logs0).tobytes()                           # the update wrote the maps
        e0 = _epoch(a.ops)
        did, _src = a.ops.draw(0.37, None)
        assert did and _epoch(a.ops) == e0 + 1
        whole = np.arange(N, dtype=np.int32)
        back = np.concatenate([whole[::-1][:40], [N - 1, 7, 7]]).astype(np.int32)        # not ascending, N - 1 and 7 twice
        by_particle = None
        for name, idx in (("ascending, all", whole), ("reversed with repeats", back), ("one", np.array([N - 2], np.int32))):
            rc, r, intact = _export(a.ops, idx)
            assert rc == GMS_OK and intact, name
            _same(r[:, :cells], pre_log[idx], f"{name}: logData of the records")
            if by_particle is None:
                by_particle = r
            _same(r, by_particle[idx], f"{name}: a particle's record is the same wherever and however often it is listed")
        planes = np.ascontiguousarray(by_particle[:, cells:]).view(np.uint32).reshape(N, 2, cw)
        _same(planes[:, 0], sc.pack_planes(pre_log), "plane 0 against the restatement of logData as the update left it")
        _same(planes[:, 1], sc.pack_planes(logs0), "plane 1 against the restatement of logData as the update found it")
        # count == 0 behind a draw: OK, nothing written
        rc, r, intact = _export(a.ops, np.zeros(0, np.int32), dst_records=1)
        assert rc == GMS_OK and intact and _untouched(r)
    finally:
        a.close()
    b = _shard(shape)
    try:
        weights = ShardedParticleFilter(N, b, coll=ThreadWorld(1).comm(0))              # no update on B: the flat weights of reset(), normalised
        for want_log, plane_of_a, what in ((logs0, 1, "plane 1 of A (stored by the update) against plane 0 of B (k_slam_codes_from_log)"),
                                           (pre_log, 0, "plane 0 of A (the apply pass) against plane 0 of B (k_slam_codes_from_log)")):
            _put_maps(b.slam, want_log)
            weights.normalize()                                                          # (the draw's source: the gathered population)
            did, src = b.draw(0.5, None)
            assert did and (np.abs(src - whole) <= 1).all()                              # flat weights: every slot draws itself, give or take a rounding
            rc, r, intact = _export(b, whole)
            assert rc == GMS_OK and intact
            _same(r[:, :cells], want_log, what + ": logData")
            _same(np.ascontiguousarray(r[:, cells:]).view(np.uint32).reshape(N, 2, cw)[:, 0], planes[:, plane_of_a], what)
            b.gather(src, np.full(N, -1, np.int32), None)                                # the draw's copies, every one local
            b.synchronize()
            _same(b.slam.maps().reshape(N, -1), want_log[src], what + ": logData behind the gather")
    finally:
        b.slam.close()


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
@shapes
def test_gather_fills_every_slot_under_every_plan(shape):
    """update, draw, export the plan's list, gather -- a fresh draw for every (mask, buffer order), the update between them: every slot holds
    its source's maps as they stood before the draw and as the stand-alone resample() leaves them, and the next update, which reads the
    moved planes, leaves both handles equal.  The generation flips with every draw: "previous" is either buffer in turn."""
    p = Pair(shape)
    r01s = np.random.default_rng(31).random(16)
    try:
        parities, used = [], set()
        for k, (mask, backwards) in enumerate(sc.rounds_of(shape)):
            pre_log, pre_lik = p.update()
            e0 = _epoch(p.ops)
            did, src = p.ops.draw(float(r01s[k]), None)
            assert did and _epoch(p.ops) == e0 + 1
            parities.append((e0 + 1) & 1)
            idx, _amb = p.ref.resample(float(r01s[k]), want_indices=True)
            assert np.array_equal(src, idx), (mask, backwards)
            assert len(np.unique(src)) < N                                               # some map moved
            remote = sc.mask_of(mask, src)
            plan = sc.plan_of(src, remote)
            if backwards:
                plan = sc.reversed_plan(plan)
            assert np.array_equal(sc.replay(plan, N), src)
            export_list, src_local, recv_pos = plan
            used.add((mask, int(remote.sum()) > 0, int((~remote).sum()) > 0))
            buf = p.ops.export(export_list) if export_list.size else None              # "none": no receive buffer at all
            assert (buf is None) == (mask == "none" or not remote.any())
            p.ops.gather(src_local, recv_pos, buf)
            p.ops.synchronize()
            where = f"round {k} ({mask}{', reversed buffer' if backwards else ''})"
            log, lik = _maps(p.ops.slam)
            _same(log, pre_log[src], where + ": logData against the sources' before the draw")
            _same(lik, pre_lik[src], where + ": likelihoodData against the sources' before the draw")
            rlog, rlik = _maps(p.ref)
            _same(log, rlog, where + ": logData against the stand-alone resample()")
            _same(lik, rlik, where + ": likelihoodData against the stand-alone resample()")
            p.same_particles(where)
        assert ("all", True, False) in used and ("none", False, True) in used and ("third", True, True) in used
        assert all(a != b for a, b in zip(parities, parities[1:])) and len(parities) >= 3
        p.update()                                                                       # reads the planes the last gather moved
    finally:
        p.close()


# ---- the order of the three calls --------------------------------------------------------------------------------------------------------------
def _refused(ops, code, what):
    """export and gather both return `code` and touch nothing: the export's destination keeps its sentinels"""
    whole = np.arange(N, dtype=np.int32)
    rc, r, intact = _export(ops, whole[:3])
    assert rc == code and intact and _untouched(r), what
    assert code == GMS_ERR_STATE and b"no draw to move maps for" in _lib.load().gms_last_error()
    recv = torch.full((2 * ops.record_doubles,), 1.0, dtype=torch.float64, device=ops.device)
    for src_local, buf in ((whole[::-1], None), (np.full(N, -1, np.int32), recv)):
        assert _gather_rc(ops, src_local, np.zeros(N, np.int32), buf) == code, what
    with pytest.raises(GmsError) as e:
        ops.gather(whole, np.zeros(N, np.int32), None)
    assert e.value.code == code and "gms_slam_shard_gather" in str(e.value)


def test_without_a_draw_that_drew_export_and_gather_are_refused():
    """GMS_ERR_STATE before the first draw, after a draw whose rule said no (the generation pair did not advance: the kernels would read a
    stale generation as the "previous" one and the gather would overwrite the live maps from it), after the gather, and after a reset --
    and the maps, the fields, the particles and the generation stay as they were, bit for bit.  A draw that draws opens both again."""
    p = Pair(SMALL)
    try:
        ops = p.ops
        _refused(ops, GMS_ERR_STATE, "before any draw")
        pre_log, pre_lik = p.update()
        # first a draw that DRAWS and its gather, so that the other generation holds maps of its own (older ones) for a stale read to find
        did, src = ops.draw(0.61, None)
        assert did
        p.ref.resample(0.61)
        ops.gather(src, np.full(N, -1, np.int32), None)
        ops.synchronize()
        _refused(ops, GMS_ERR_STATE, "a second gather on one draw")
        pre_log, pre_lik = p.update()
        e0, (P0, w0) = _epoch(ops), ops.slam.get_particles()
        did, src = ops.draw(0.37, 1e-9)                                                  # Neff < 1e-9 * N: never
        assert not did and _epoch(ops) == e0
        assert src.shape == (N,) and (src >= 0).all() and (src < N).all()                # (the sources are returned all the same)
        for when in ("behind the draw that did not draw", "behind the refused calls"):
            log, lik = _maps(ops.slam)
            _same(log, pre_log, f"logData {when}")
            _same(lik, pre_lik, f"likelihoodData {when}")
            P, w = ops.slam.get_particles()
            _same(P, P0, f"poses {when}"); _same(w, w0, f"weights {when}")
            assert _epoch(ops) == e0
            _refused(ops, GMS_ERR_STATE, "the last draw did not draw")
        # the next update and a draw that draws: both work again, on both generations' true contents
        pre_log, pre_lik = p.update()
        did, src = ops.draw(0.83, None)
        idx, _ = p.ref.resample(0.83, want_indices=True)
        assert did and np.array_equal(src, idx) and _epoch(ops) == e0 + 1
        plan = sc.reversed_plan(sc.plan_of(src, sc.mask_of("third", src)))
        ops.gather(plan[1], plan[2], ops.export(plan[0]))
        ops.synchronize()
        log, lik = _maps(ops.slam)
        _same(log, pre_log[src], "logData behind the draw that drew")
        _same(lik, pre_lik[src], "likelihoodData behind the draw that drew")
        p.update()
        # a reset forgets an open draw
        did, _src = ops.draw(0.5, None)
        assert did
        ops.slam.reset()
        _refused(ops, GMS_ERR_STATE, "behind a reset")
    finally:
        p.close()


def test_refused_arguments_leave_an_open_draw_as_it_was():
    """the refusals the calls had before: a local source >= n, a remote slot with no buffer, a negative position on a remote slot, an
    export index out of range, more records than particles -- each GMS_ERR_INVALID, nothing written, and the draw still open: the export and the gather that follow give what they would have given.  And the stand-alone resample() on a block of a larger population: GMS_ERR_STATE"""
    p = Pair(SMALL)
    try:
        ops = p.ops
        pre_log, pre_lik = p.update()
        did, src = ops.draw(0.29, None)
        idx, _ = p.ref.resample(0.29, want_indices=True)
        assert did and np.array_equal(src, idx)
        plan = sc.plan_of(src, sc.mask_of("third", src))
        export_list, src_local, recv_pos = plan
        buf = ops.export(export_list)
        ops.synchronize()
        cur0 = ops.slam.maps().reshape(N, -1)                                            # the generation the gather will fill, whatever it holds now
        far = int(np.nonzero(src_local < 0)[0][0])
        bad = []
        a = src_local.copy(); a[5 if far != 5 else 6] = N
        bad.append((a, recv_pos, buf))                                                   # a local source out of range
        bad.append((src_local, recv_pos, None))                                          # a remote slot, no buffer
        b = recv_pos.copy(); b[far] = -1
        bad.append((src_local, b, buf))                                                  # a remote slot, no position
        for k, (sl, rp, rb) in enumerate(bad):
            assert _gather_rc(ops, sl, rp, rb) == GMS_ERR_INVALID, k
        for k, wrong in enumerate((np.array([0, N], np.int32), np.array([-1], np.int32), np.zeros(N + 1, np.int32))):
            rc, r, intact = _export(ops, wrong)
            assert rc == GMS_ERR_INVALID and intact and _untouched(r), k                 # index out of range (twice); count > n
        _same(ops.slam.maps().reshape(N, -1), cur0, "the generation to be filled, behind the refusals")
        rc, r, intact = _export(ops, export_list)
        assert rc == GMS_OK and intact
        _same(r, buf.cpu().numpy(), "the export behind the refusals")
        ops.gather(src_local, recv_pos, buf)
        ops.synchronize()
        log, lik = _maps(ops.slam)
        _same(log, pre_log[src], "logData behind the refusals and the gather")
        _same(lik, pre_lik[src], "likelihoodData behind the refusals and the gather")
        p.same_particles("behind the refusals and the gather")
        p.update()
    finally:
        p.close()
    # (a shard that is the whole population is one rank's view of a one-rank group AND a stand-alone filter: the refusal of the
    # stand-alone resample() needs a block that is not everything)
    half = SlamShardOps(*sc.size_of(SMALL), sc.RES, (0.0, 0.0), N, N, 2 * N, max_beams=MAX_BEAMS)
    try:
        _put_maps(half.slam, sc.logs_of(SMALL))
        with pytest.raises(GmsError) as e:
            half.slam.resample(0.5)
        assert e.value.code == GMS_ERR_STATE and _epoch(half) == 0
        _same(half.slam.maps().reshape(N, -1), sc.logs_of(SMALL), "logData behind the refused stand-alone resample()")
    finally:
        half.slam.close()
