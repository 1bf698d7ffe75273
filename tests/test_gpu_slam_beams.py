"""The per-particle beam sensor model on the device (include/gridmapslam.h "per-particle beam sensor model": gms_slam_score_beams,
gms_slam_set_beam_model; k_slam_beam_score, k_slam_weight_combine) against tests/_beams_expect.py, imported unchanged and called once
per particle with that particle's own logData.  Every comparison is array_equal on bits (same_bits).

The shapes are the smallest that can go wrong: a 40 x 36 map (neither a multiple of 32), 24 particles with 24 different maps, scans of
1, 7 and 300 beams (300: some lanes own two beams), tables of 2, 10 and 512 entries per row; a 1024 x 1024 map for the window that
does not fit the LDS; 32 particles on 48 x 48 cells and 40 beams for the updates."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import _beams_expect as bx
from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, beam_model_factors, synth
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_STATE, GmsError, load, ptr
from oracle import oracle as orc

from test_gpu_slam_batch import _compare as _compare_batch

pytestmark = pytest.mark.gpu

RES = 0.05
W0, H0, N0 = 40, 36, 24
SIZE0 = ((W0 - 0.4) * RES, (H0 - 0.4) * RES)
LDS_WORDS = 64 * 1024 // 4
STATS = ("weight_sum", "neff", "strongest", "n_zero", "max_log_weight")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _with_walk(mem, make):
    old = os.environ.pop("GMS_CAST_WALK", None)
    if mem:
        os.environ["GMS_CAST_WALK"] = "mem"                                # read when the handle is created
    try:
        return make()
    finally:
        os.environ.pop("GMS_CAST_WALK", None)
        if old is not None:
            os.environ["GMS_CAST_WALK"] = old


def _beams(x, y, hit):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    b = np.zeros(x.shape, dtype=BEAM_DTYPE)
    b["local_x"], b["local_y"] = x, y
    b["distance"] = np.sqrt(x * x + y * y)
    b["hit"] = hit
    return b


def _handle(size=SIZE0, cells=(W0, H0), n=N0, max_beams=320, mem=False, cls=SLAMParticleMaps, **kw):
    s = _with_walk(mem, lambda: cls(size[0], size[1], RES, (0.0, 0.0), num_particles=n, max_beams=max_beams, **kw))
    assert (s.W, s.H) == cells
    return s


def _grid(size=SIZE0, cells=(W0, H0)):
    g = orc.Grid(size[0], size[1], RES, 0.0, 0.0)
    assert (g.W, g.H) == cells
    return g


def _put(s, logs, poses):
    for i, lg in enumerate(logs):
        s.set_map(i, log=lg)
    s.set_poses(poses)


# ---- 1, 2: the stand-alone call against the definition, all three sources of the bits ---------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case():
    """(logData [24][H0][W0], poses [24][3], beams [300]): every particle's map different, 6 % occupied, with cells of 0, -0.0, NaN,
    5e-324 (occupied) and negative values; poses whose beams leave the map, one pose outside, one NaN pose; both hit values"""
    g = _grid()
    rng = np.random.default_rng(20261020)
    u = rng.random((N0, H0, W0))
    logs = np.where(u < 0.06, g.l_occ, np.where(u < 0.6, g.l_free, 0.0))
    for i in range(N0):
        for v in (0.0, -0.0, np.nan, 5e-324, -3.25):
            logs[i, rng.integers(0, H0, 25), rng.integers(0, W0, 25)] = v
    logs[:, 0, 0] = g.l_occ                                                # where a NaN coordinate lands (NaN -> cell 0)
    poses = np.column_stack([rng.uniform(0.15, SIZE0[0] - 0.15, N0), rng.uniform(0.15, SIZE0[1] - 0.15, N0), rng.uniform(-math.pi, math.pi, N0)])
    poses[2] = (-0.6, 0.9, 0.1)                                            # outside, looking in: no walk starts
    poses[6] = (np.nan, 0.7, 0.0)
    ang = rng.uniform(-math.pi, math.pi, 300)
    dist = np.where(rng.random(300) < 0.7, rng.uniform(0.05, 1.2, 300), rng.uniform(2.5, 5.0, 300))       # three in ten leave the map
    beams = _beams(dist * np.cos(ang), dist * np.sin(ang), rng.random(300) < 0.7)
    beams["hit"][0] = 1
    logs.flags.writeable = False
    return logs, poses.astype(np.float32), beams


@functools.lru_cache(maxsize=None)
def small_rem(ahead):
    """n_rem [24][300] of small_case, particle i through ITS map (once per ahead; B < 300 is its first columns)"""
    logs, poses, beams = small_case()
    g = _grid()
    r = np.stack([bx.remaining(g, logs[i], beams, poses[i], ahead) for i in range(N0)])
    r.flags.writeable = False
    return r


def _check_call(s, beams, factors, behind, ahead, rem, where):
    idx = bx.indices_from(rem, behind, ahead)
    w, lw = bx.weights_of(idx, beams["hit"] != 0, factors)
    res = s.score_beams(beams, factors, behind, ahead, residuals=True)
    assert res.dtype == np.uint16 and res.shape == idx.shape, (where, res.shape)
    bad = np.argwhere(res != idx)
    assert np.array_equal(res, idx), f"{where}: {len(bad)} of {idx.size} indices differ, first at {bad[:1].tolist()}"
    assert bx.same_bits(s.pf.get_weights(), w), (where, "weights")
    assert bx.same_bits(s.pf.get_log_weights(), lw), (where, "log-weights")
    return w, lw


@pytest.mark.parametrize("source", ["lds", "mem"])
@pytest.mark.parametrize("behind,ahead", [(0, 0), (3, 5), (255, 255)])
def test_stand_alone_call_equals_the_definition(behind, ahead, source):
    logs, poses, beams = small_case()
    rem = small_rem(ahead)
    idx = bx.indices_from(rem, behind, ahead)
    T = behind + ahead + 2
    # what the expectation must contain for the comparison to mean something
    assert (idx == T - 1).any() and (idx < T - 1).mean() > 0.2, "walls found and walks that find none"
    assert (rem[2] == 0).all(), "a pose outside the map starts no walk"
    assert len({idx[i].tobytes() for i in range(N0)}) >= N0 - 2, "the particles' maps answer differently"
    assert set(np.unique(beams["hit"])) == {0, 1}
    if source == "lds":
        assert 0 < max(bx.window_words(_grid(), beams, p, ahead) for p in poses) <= LDS_WORDS
    s = _handle(mem=source == "mem")
    _put(s, logs, poses)
    before = (s.pf.get_poses(), s.maps(), s.maps(likelihood=True))
    rng = np.random.default_rng(behind + 11)
    for B in (1, 7, 300):
        factors = rng.uniform(0.7, 1.3, (2, T))
        _check_call(s, beams[:B], factors, behind, ahead, rem[:, :B], f"{source} ({behind}, {ahead}) B {B}")
    # without the residuals nothing else changes
    w, lw = bx.weights_of(idx, beams["hit"] != 0, factors)
    s.pf.set_weights(np.ones(N0))
    assert s.score_beams(beams, factors, behind, ahead) is None
    assert bx.same_bits(s.pf.get_weights(), w) and bx.same_bits(s.pf.get_log_weights(), lw)
    after = (s.pf.get_poses(), s.maps(), s.maps(likelihood=True))
    for a, b, what in zip(before, after, ("poses", "logData", "likelihoodData")):
        assert _same(a, b), f"{source}: the call changed {what}"
    s.close()


def test_device_form_and_refusals():
    torch = pytest.importorskip("torch")
    logs, poses, beams = small_case()
    behind, ahead, B = 3, 5, 300
    rem = small_rem(ahead)
    idx = bx.indices_from(rem, behind, ahead)
    factors = np.random.default_rng(5).uniform(0.7, 1.3, (2, behind + ahead + 2))
    w, lw = bx.weights_of(idx, beams["hit"] != 0, factors)
    s = _handle()
    _put(s, logs, poses)
    db = torch.from_numpy(beams.view(np.uint8).copy()).cuda()
    out = torch.zeros(N0 * B + 1, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()                                               # (the handle runs on a stream of its own)
    s.score_beams_dev(db.data_ptr(), B, factors, behind, ahead, residuals_out=out[:N0 * B])
    s.grid_map.synchronize()
    assert np.array_equal(out[:N0 * B].cpu().numpy().view(np.uint16).reshape(N0, B), idx) and int(out[-1]) == 0
    assert bx.same_bits(s.pf.get_weights(), w) and bx.same_bits(s.pf.get_log_weights(), lw)
    # refused with nothing touched: B out of range, a misaligned residual buffer
    L = load()
    s.pf.set_weights(np.full(N0, 0.25))
    for Bbad in (0, 321, -1):
        assert L.gms_slam_score_beams(s._h, ptr(beams), Bbad, behind, ahead, ptr(factors), None) != 0 and b"max_beams" in L.gms_last_error()
    assert L.gms_slam_score_beams_dev(s._h, C.c_void_p(db.data_ptr()), B, behind, ahead, ptr(factors), C.c_void_p(out.data_ptr() + 1)) != 0
    assert b"aligned" in L.gms_last_error()
    assert (s.pf.get_weights() == 0.25).all()
    s.close()


def test_window_larger_than_the_lds_walks_memory():
    """two particles on 1024 x 1024 cells under one scan of 20 m beams: particle 0 in the middle -- its window does not fit 64 KiB and
    every bit comes from logData in memory --, particle 1 in a corner, where the clipped window fits: both in one launch"""
    cells, size = (1024, 1024), ((1024 - 0.4) * RES, (1024 - 0.4) * RES)
    g = _grid(size, cells)
    rng = np.random.default_rng(1024)
    logs = np.where(rng.random((2, 1024, 1024)) < 0.0015, g.l_occ, g.l_free)
    logs[:, 0, 0] = g.l_occ
    poses = np.array([(25.6, 25.6, 0.3), (4.0, 3.0, -2.0)], np.float32)
    ang = np.linspace(-math.pi, math.pi, 48, endpoint=False) + 0.01
    dist = rng.uniform(18.0, 22.0, 48)
    beams = _beams(dist * np.cos(ang), dist * np.sin(ang), rng.random(48) < 0.7)
    behind, ahead = 6, 4
    words = [bx.window_words(g, beams, p, ahead) for p in poses]
    assert words[0] > LDS_WORDS >= words[1] > 0, words
    rem = np.stack([bx.remaining(g, logs[i], beams, poses[i], ahead) for i in range(2)])
    idx = bx.indices_from(rem, behind, ahead)
    assert ((idx < behind + ahead + 1).mean(axis=1) > 0.2).all() and (idx == behind + ahead + 1).any()
    s = _handle(size, cells, n=2, max_beams=64)
    _put(s, logs, poses)
    factors = rng.uniform(0.7, 1.3, (2, behind + ahead + 2))
    _check_call(s, beams, factors, behind, ahead, rem, "1024 x 1024")
    s.close()


# ---- 3: the state the call leaves -----------------------------------------------------------------------------------------------------
def test_normalize_and_resample_follow_the_call():
    logs, poses, beams = small_case()
    behind, ahead = 3, 5
    factors = beam_model_factors(RES, behind, ahead, 0.05)
    s = _handle()
    _put(s, logs, poses)
    s.score_beams(beams[:40], factors, behind, ahead)
    raw = s.pf.get_weights()
    st = s.pf.normalize()
    with np.errstate(under="ignore"):
        assert st["weight_sum"] == pytest.approx(raw.sum(), rel=1e-12) and st["strongest"] == int(np.argmax(raw))
    wn = s.pf.get_weights()
    assert wn.sum() == pytest.approx(1.0, rel=1e-12) and st["neff"] < N0
    s.resample_if(0.37, fraction=1.0)                                      # Neff < n: it draws
    src = s.pf.last_resample_indices()
    assert len(np.unique(src)) < N0 and (src >= 0).all() and (src < N0).all()
    assert _same(s.maps(), np.asarray(logs)[src]), "the maps that follow the drawn indices are the sources' maps"
    assert _same(s.pf.get_poses(), poses[src])
    s.close()


# ---- 4, 7: what the model must not change ---------------------------------------------------------------------------------------------
EXT4, N4, B4 = 2.4, 32, 40


@functools.lru_cache(maxsize=None)
def _trace4():
    return synth.make_trace(EXT4, RES, B4, T=12, seed=77)


def _handle4(config="plain", n=N4, cls=SLAMParticleMaps, **kw):
    s = cls(EXT4, EXT4, RES, (-EXT4 / 2, -EXT4 / 2), num_particles=n, max_beams=64, **kw)
    assert (s.W, s.H) == (48, 48)
    if config == "refine":
        s.set_refine(True)
    if config == "align":
        s.set_align(True)
    return s


def _same_handles(a, b, where, maps=True):
    assert _same(a.pf.get_poses(), b.pf.get_poses()), f"{where}: poses"
    assert _same(a.pf.get_weights(), b.pf.get_weights()), f"{where}: weights"
    for k in STATS:
        x, y = a.last_stats[k], b.last_stats[k]
        assert x == y or (x != x and y != y), f"{where}: {k} {x} != {y}"
    if maps:
        assert _same(a.maps(), b.maps()), f"{where}: logData"


def _drive(s, T=6, seed=5, first=0):
    tr = _trace4()
    for k in range(first, first + T):
        s.update(tr.scans[k], (0.03, 0.05 if k % 2 else -0.04), seed=seed, sequence=k)


@pytest.mark.parametrize("config", ["plain", "refine", "align"])
def test_all_ones_table_changes_nothing(config):
    """MULTIPLY by a table of ones: the motion draw moves into the beam launch, the weight is multiplied by 1.0 and the log-weight
    gets + 0.0 -- six updates with sample_motion = 1 equal the same handle without the model, bit for bit"""
    a, b = _handle4(config), _handle4(config)
    b.set_beam_model(np.ones((2, 10)), 3, 5, combine="multiply")
    tr = _trace4()
    for k in range(6):
        for s in (a, b):
            s.update(tr.scans[k], (0.03, 0.05 if k % 2 else -0.04), seed=5, sequence=k)
        _same_handles(a, b, f"{config} update {k}", maps=k == 5)
    assert not _same(a.pf.get_poses(), np.zeros((N4, 3), np.float32)), "the motion sample was drawn"
    a.close(); b.close()


def test_a_model_set_and_cleared_is_gone():
    a, b = _handle4(), _handle4()
    _drive(a, 2); _drive(b, 2)
    b.set_beam_model(beam_model_factors(RES, 3, 5, 0.05), 3, 5, combine="replace")
    b.set_beam_model(None)
    _drive(a, 2, first=2); _drive(b, 2, first=2)
    _same_handles(a, b, "set, then cleared")
    # ... and a model that stays set survives reset()
    b.set_beam_model(beam_model_factors(RES, 3, 5, 0.05), 3, 5, combine="replace")
    a.reset(); b.reset()
    _drive(a, 2); _drive(b, 2)
    assert _same(a.pf.get_poses(), b.pf.get_poses()) and not _same(a.pf.get_weights(), b.pf.get_weights()), "reset() keeps the setting"
    a.close(); b.close()


# ---- 5: the weights inside the update ---------------------------------------------------------------------------------------------------
def _update_local(s, z, odo, seed, sequence):
    """gms_slam_update_local: the update without its normalisation -- the weights stay raw"""
    b = np.ascontiguousarray(z, dtype=BEAM_DTYPE)
    rc = load().gms_slam_update_local(s._h, ptr(b), len(b), 1, float(odo[0]), float(odo[1]), int(seed), int(sequence))
    assert rc == 0, load().gms_last_error()


@pytest.mark.parametrize("config", ["plain", "align"])
def test_weights_inside_the_update(config):
    behind, ahead = 3, 5
    factors = beam_model_factors(RES, behind, ahead, 0.05)
    tr = _trace4()
    g = orc.Grid(EXT4, EXT4, RES, -EXT4 / 2, -EXT4 / 2)
    z, odo = tr.scans[4], (0.04, 0.06)
    hs = {k: _handle4(config) for k in ("replace", "multiply", "plain", "plain_raw", "multiply_raw")}
    for s in hs.values():
        _drive(s, 4)                                                       # four plain updates: every particle has a map of its own
    logs0, P0 = hs["plain"].maps(), hs["plain"].pf.get_poses()
    assert len({logs0[i].tobytes() for i in range(N4)}) > N4 // 2
    hs["replace"].set_beam_model(factors, behind, ahead, combine="replace")
    hs["multiply"].set_beam_model(factors, behind, ahead, combine="multiply")
    hs["multiply_raw"].set_beam_model(factors, behind, ahead, combine="multiply")
    for k in ("replace", "multiply", "plain"):
        hs[k].update(z, odo, seed=9, sequence=40)
    for k in ("plain_raw", "multiply_raw"):
        _update_local(hs[k], z, odo, 9, 40)
    A = hs["replace"]
    P1 = A.pf.get_poses()
    assert not _same(P1, P0), "the poses moved: the walk is taken at the pose the particle is weighted at"
    for k in hs:
        assert _same(hs[k].pf.get_poses(), P1), f"{k}: poses"
        assert _same(hs[k].maps(), hs["plain"].maps()), f"{k}: the model changes weights only"
    # a second handle holding the pre-update maps and A's poses: the raw beam weights, themselves the definition's
    Bh = _handle4()
    _put(Bh, logs0, P1)
    Bh.score_beams(z, factors, behind, ahead)
    wb, lwb = Bh.pf.get_weights(), Bh.pf.get_log_weights()
    want = [bx.expect(g, logs0[i], z, P1[i:i + 1], factors, behind, ahead) for i in range(N4)]
    assert bx.same_bits(wb, np.concatenate([w[0] for w in want])) and bx.same_bits(lwb, np.concatenate([w[1] for w in want]))
    assert len(np.unique(wb)) > N4 // 2
    # REPLACE: a third handle on which those raw weights were set and normalised
    Ch = _handle4()
    Ch.pf.set_weights(wb)
    Ch.pf.normalize()
    assert bx.same_bits(A.pf.get_weights(), Ch.pf.get_weights()), "REPLACE: the normalised weights are the beam weights'"
    # MULTIPLY: the raw product, one double multiply; the log-weight the sum
    we, lwe = hs["plain_raw"].pf.get_weights(), hs["plain_raw"].pf.get_log_weights()
    with np.errstate(under="ignore"):
        assert bx.same_bits(hs["multiply_raw"].pf.get_weights(), we * wb), "MULTIPLY: raw weight = probabilityOf * beam weight"
    assert bx.same_bits(hs["multiply_raw"].pf.get_log_weights(), lwe + lwb), "MULTIPLY: raw log-weight = the sum"
    Ch.pf.set_weights(we * wb)
    Ch.pf.normalize()
    assert bx.same_bits(hs["multiply"].pf.get_weights(), Ch.pf.get_weights())
    assert not _same(hs["multiply"].pf.get_weights(), hs["plain"].pf.get_weights())
    for s in list(hs.values()) + [Bh, Ch]:
        s.close()


# ---- 6: batched and sharded handles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["multiply", "replace"])
def test_batched_handle_equals_stand_alone_handles(combine):
    S, n, counts = 3, 16, (40, 0, 17)                                      # ragged, one filter without a beam: its raw weight stays the update's
    factors = beam_model_factors(RES, 3, 5, 0.05)
    bat = _handle4(n=n, cls=functools.partial(SLAMParticleMapsBatch, S))
    alone = [_handle4(n=n) for _ in range(S)]
    for s in [bat] + alone:
        s.set_beam_model(factors, 3, 5, combine=combine)
    scans = [synth.make_trace(EXT4, RES, B, T=4, seed=31 + 17 * f).scans if B else [np.zeros(0, dtype=BEAM_DTYPE)] * 4 for f, B in enumerate(counts)]
    odo = [(0.03, 0.05), (0.02, -0.03), (0.05, 0.01)]
    for k in range(4):
        bat.update([scans[f][k] for f in range(S)], odo, seeds=[3, 4, 5], sequence=k)
        for f in range(S):
            alone[f].update(scans[f][k], odo[f], seed=3 + f, sequence=k)
        _compare_batch(bat, alone, f"{combine} update {k}", maps=k == 3, indices=False)
    W = bat.get_particles()[1]
    assert (W[1] == 1.0 / n).all() and len(np.unique(W[0])) > 1, "no beam: the empty product, normalised"
    # the stand-alone call is for one filter: GMS_ERR_STATE, the weights untouched
    L = load()
    z = np.ascontiguousarray(scans[0][0])
    assert L.gms_slam_score_beams(bat._h, ptr(z), len(z), 3, 5, ptr(factors), None) == GMS_ERR_STATE and b"filters" in L.gms_last_error()
    assert _same(bat.get_particles()[1], W)
    for s in [bat] + alone:
        s.close()


def test_shard_scores_its_own_block():
    """two blocks of 256 of a filter of 512: the stand-alone call on each, and a local update with the model whose motion sample is
    keyed by the global index, equal the stand-alone filter's slices"""
    n, nl = 512, 256
    rng = np.random.default_rng(512)
    g = _grid()
    logs = np.where(rng.random((n, H0, W0)) < 0.06, g.l_occ, g.l_free)
    poses = np.column_stack([rng.uniform(0.3, SIZE0[0] - 0.3, n), rng.uniform(0.3, SIZE0[1] - 0.3, n), rng.uniform(-3, 3, n)]).astype(np.float32)
    beams = small_case()[2][:40]
    factors = beam_model_factors(RES, 3, 5, 0.05)
    whole = _handle(n=n)
    _put(whole, logs, poses)
    res = whole.score_beams(beams, factors, 3, 5, residuals=True)
    w, lw = whole.pf.get_weights(), whole.pf.get_log_weights()
    assert bx.same_bits(w[:3], np.concatenate([bx.expect(g, logs[i], beams, poses[i:i + 1], factors, 3, 5)[0] for i in range(3)]))
    whole.set_beam_model(factors, 3, 5, combine="multiply")
    _update_local(whole, beams, (0.03, 0.02), 7, 1)
    for r in range(2):
        sh = SLAMParticleMaps.__new__(SLAMParticleMaps)
        sh._init_shard(SIZE0[0], SIZE0[1], RES, (0.0, 0.0), nl, r * nl, n, max_beams=320)
        blk = slice(r * nl, (r + 1) * nl)
        _put(sh, logs[blk], poses[blk])
        assert np.array_equal(sh.score_beams(beams, factors, 3, 5, residuals=True), res[blk]), f"rank {r}: residuals"
        assert bx.same_bits(sh.pf.get_weights(), w[blk]) and bx.same_bits(sh.pf.get_log_weights(), lw[blk]), f"rank {r}"
        sh.set_beam_model(factors, 3, 5, combine="multiply")
        _update_local(sh, beams, (0.03, 0.02), 7, 1)
        assert _same(sh.pf.get_poses(), whole.pf.get_poses()[blk]) and _same(sh.pf.get_weights(), whole.pf.get_weights()[blk]), f"rank {r}: the local update"
        assert _same(sh.maps(), whole.maps()[blk]), f"rank {r}: the maps"
        sh.close()
    whole.close()
