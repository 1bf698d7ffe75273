"""Global scan matching at the ends of its documented domain (include/gridmapslam.h "global scan matching"): pyramid levels 5, 6 and 7,
coordinates beyond 2^16, 1024 headings, up to 4096 beams (the threshold search's chunks), the 2^24 work-list limit and the _dev forms'
precondition.  The helpers are tests/test_gpu_locate.py's and the expectations tests/_locate_expect.py's; every comparison is
array_equal on the whole record array, fillers and guard records included, and on n_out.  Each case's expectation is made once, by a
function that needs no device and that asserts what the case relies on (which records the expectation holds), and shared among the
handles created with GMS_LOCATE_LEVELS forced or unset."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import _locate_expect as lx
from gridmap_slam_robot_amd import LOCATE_DTYPE
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_NOMEM, GmsError, load
from gridmap_slam_robot_amd.gridmap import _locate_args, _locate_table
from test_gpu_locate import GUARD, L_FREE, L_OCC, SKIP, _map, _quarter_turn_offsets, _random_log, _random_offsets, _raw, _room_log, _same

pytestmark = pytest.mark.gpu

DEEP = ("5", "6", "7", None)


def _open(shape, levels, log, **kw):
    maps = [_map(shape, lv, **kw) for lv in levels]
    for m in maps:
        m.upload_log(log)
    return maps


def _all_same(maps, levels, log, off, where, want, **kw):
    for lv, m in zip(levels, maps):
        _same(m, log, off, f"{where}, levels {lv}", want=want, **kw)


# ---- 1. deep levels ------------------------------------------------------------------------------------------------------------------
#            shape, the unaligned rectangle, the log's seed, the offsets' seed
DEEP_MAPS = [((70, 67), (7, 3, 59, 61), 7067_5, 11),        # two words a row: the level-7 top level is ONE block per heading
             ((129, 65), (11, 2, 113, 60), 12965_5, 12),    # three words, one bit in the last
             ((200, 130), (37, 5, 150, 120), 200130, 13)]   # four words; the rectangle: two level-7 blocks in x, children dropped at x1 and y1 on every level


@functools.lru_cache(maxsize=None)
def _deep_case(i):
    """(log, off, [(where, kw, want)]): whole map and the unaligned rectangle x free_only x tol 0 / 2 x cap 1 / 300"""
    shape, rect, seed, oseed = DEEP_MAPS[i]
    log = _random_log(shape, seed)
    off = _random_offsets(3, 24, 12, oseed)
    cases = []
    for tol in (0, 2):
        hit = lx.hit_cells(log, tol)
        for r in (None, rect):
            for fo in (False, True):
                for cap in (1, 300):
                    kw = dict(rect=r, tol=tol, min_score=3, cap=cap, free_only=fo)
                    want = lx.expect(log, off, hit=hit, **kw)
                    assert want[2] > 300, "more candidates than either cap"
                    cases.append((f"{shape}, {kw}", kw, want))
    return log, off, cases


@pytest.mark.parametrize("i", range(len(DEEP_MAPS)), ids=lambda i: "%dx%d" % DEEP_MAPS[i][0])
def test_levels_5_6_7_on_random_maps(i):
    log, off, cases = _deep_case(i)
    maps = _open(DEEP_MAPS[i][0], DEEP, log)
    for where, kw, want in cases:
        _all_same(maps, DEEP, log, off, where, want, **kw)
    for lv, m in zip(DEEP, maps):
        assert m.locate_stats()["levels"] == (int(lv) if lv else {0: 3, 1: 4, 2: 5}[i]), "the unaligned rectangle was the last request"
        m.close()


@functools.lru_cache(maxsize=None)
def _handover_case(down):
    """The hand-over to the NEXT word (down: to the row block 64 rows on) on 200 x 130: free but for single occupied cells at x = 64,
    127, 128 and 191 (down: y = 64, 127 and 128) in rows (columns) 30 apart.  One beam per heading, 64 .. 127 cells to the right (up),
    so a pose in [0, 64) hits only in the next word and a pose in [64, 128) only two words on.  The other component of each beam keeps
    every other occupied cell out of the beam's level-6 and level-7 windows: the bound of the block that holds such a pose is 1 only
    through the word (rows) a whole word (64 rows) beyond the beam's end.
    k = 0: (64, 50) from (64, 20) ends in (128, 70), from (127, 50) in (191, 100): upper-half poses of the level-7 block at 0;
    k = 1: (96, 50) from (32, 20) ends in (128, 70): the upper half of the level-6 block at 0, the end at bit 32 of word 1;
    k = 2: (64, -20) and k = 3: (127, 10): from (0, 30) they end in (64, 10) and (127, 40)."""
    log = np.full((130, 200), L_FREE)
    cells = [(64, 10), (127, 40), (128, 70), (191, 100)]
    off = np.array([[[64, 50]], [[96, 50]], [[64, -20]], [[127, 10]]], dtype=np.int16)
    first, whole = [(0, 30)], [(0, 64, 20), (1, 32, 20), (0, 127, 50), (1, 95, 50)]
    if down:
        cells = [(y, x) for x, y in cells[:3]]
        off = off[:, :, ::-1].copy()
        whole = [(k, y, x) for k, x, y in whole[:2]]
        first = [(30, 0)]
    for x, y in cells:
        log[y, x] = L_OCC
    ax = 1 if down else 0                                                      # the component under test: y when down, else x
    name = "y" if down else "x"
    assert ((off[:, 0, ax] >= 64) & (off[:, 0, ax] <= 127)).all()
    near = (0, 0, 200, 64) if down else (0, 0, 64, 130)
    cases = []
    for fo in (False, True):
        kw = dict(rect=near, tol=0, min_score=1, cap=16, free_only=fo)
        want = lx.expect(log, off, **kw)
        rec = want[0][:want[1]]
        assert want[1] >= 3 and (rec[name] < 64).all() and (rec[name] + off[rec["k"], 0, ax] >= 64).all(), "poses in [0, 64), every end in the next word"
        assert {(2,) + first[0], (3,) + first[0]} <= {(r["k"], r["x"], r["y"]) for r in rec}
        cases.append((f"down {down}, {kw}", kw, want))
        kw = dict(rect=None, tol=0, min_score=1, cap=16, free_only=fo)
        want = lx.expect(log, off, **kw)
        rec = want[0][:want[1]]
        assert set(whole) <= {(r["k"], r["x"], r["y"]) for r in rec}, "the poses whose only hit lies a whole word beyond the beam's end from the block's origin"
        cases.append((f"down {down}, {kw}", kw, want))
    return log, off, cases


@pytest.mark.parametrize("down", [False, True], ids=["next_word", "next_row_block"])
def test_the_pyramids_hand_over_across_a_whole_word(down):
    log, off, cases = _handover_case(down)
    maps = _open((200, 130), DEEP, log)
    for where, kw, want in cases:
        _all_same(maps, DEEP, log, off, where, want, **kw)
    for m in maps:
        m.close()


THIN = [((260, 3), 6), ((3, 260), 6), ((520, 3), 7), ((3, 520), 7)]


@functools.lru_cache(maxsize=None)
def _thin_case(i):
    shape, _ = THIN[i]
    log = _random_log(shape, 26_000 + i)
    off = _random_offsets(4, 24, 12, 260 + i)
    cases = []
    for kw in (dict(tol=0, min_score=1, cap=300, free_only=False), dict(tol=2, min_score=2, cap=16, free_only=True)):
        want = lx.expect(log, off, **kw)
        print(f"{shape}, {kw}: N = {want[2]}")
        assert want[2] > 16
        cases.append((f"{shape}, {kw}", kw, want))
    return log, off, cases


@pytest.mark.parametrize("i", range(len(THIN)), ids=lambda i: "%dx%d" % THIN[i][0])
def test_unset_levels_reach_6_and_7_on_thin_maps(i):
    """almost every child is dropped in one direction"""
    shape, L = THIN[i]
    log, off, cases = _thin_case(i)
    m, = _open(shape, (None,), log)
    for where, kw, want in cases:
        _same(m, log, off, where, want=want, **kw)
        st = m.locate_stats()
        assert st["levels"] == L and st["evaluated"][L] == 4 * -(-max(shape) // 2 ** L), f"2^({L} + 2) <= {max(shape)} < 2^({L} + 3)"
    m.close()


# ---- 2. wide fields ------------------------------------------------------------------------------------------------------------------
FAR = 70001


@functools.lru_cache(maxsize=None)
def _far_case(tall):
    """a 70001 x 3 (tall: 3 x 70001) map, 2 % of it occupied: rectangles of 40 x 3 at the far end, across 65536 and at the origin"""
    rng = np.random.default_rng(70002)                                         # (a seed with occupied cells beside all three rectangles)
    strip = np.where(rng.random((3, FAR)) < 0.02, L_OCC, L_FREE)
    log = np.ascontiguousarray(strip.T) if tall else strip
    off = _random_offsets(4, 128, 12, 7000 + tall)                            # (of 128 beams a dozen end inside the three rows)
    cut = log[:300] if tall else log[:, :300]
    assert np.array_equal(lx.hit_cells(cut, 0), cut > 0), "tol 0: the hit cells are the occupied cells"
    name = "y" if tall else "x"
    cases = []
    for start in (FAR - 40, 65516, 0):
        rect = (0, start, 3, 40) if tall else (start, 0, 40, 3)
        for cap in (16, 300):
            kw = dict(rect=rect, tol=0, min_score=1, cap=cap, free_only=False)
            want = lx.expect(log, off, **kw)
            rec = want[0][:want[1]]
            assert want[2] > 16
            if start == FAR - 40:
                assert (rec[name] >= 65536).all(), "every coordinate needs 17 bits"
            if start == 65516:
                assert (rec[name] >= 65536).any() and (rec[name] < 65536).any(), "records on both sides of 2^16"
            cases.append((f"tall {tall}, {kw}", kw, want))
    return log, off, cases


@pytest.mark.parametrize("tall", [False, True], ids=["70001x3", "3x70001"])
def test_coordinates_above_65536(tall):
    log, off, cases = _far_case(tall)
    levels = (None, "0")
    maps = _open((3, FAR) if tall else (FAR, 3), levels, log)
    for where, kw, want in cases:
        _all_same(maps, levels, log, off, where, want, **kw)
    for m in maps:
        m.close()


@functools.lru_cache(maxsize=None)
def _headings_case():
    shape = (70, 67)
    log = _random_log(shape, 1024)
    off = np.concatenate([_random_offsets(1, 24, 12, 5000 + k) for k in range(1024)])          # every heading's row is its own
    assert off.shape == (1024, 24, 2) and len({r.tobytes() for r in off}) == 1024
    kw = dict(rect=(30, 29, 9, 9), tol=0, min_score=1, cap=4096, free_only=False)
    want = lx.expect(log, off, **kw)
    ks = want[0]["k"]
    assert want[1] == 4096 and want[2] > 4096, "more survivors than the selection sorts at once: the radix path"
    assert ((ks > 255) & (ks < 512)).any() and (ks > 511).any() and ks.max() > 1000, "heading indices that need all ten bits"
    return log, off, kw, want


def test_1024_headings():
    log, off, kw, want = _headings_case()
    levels = (None, "0", "3")
    maps = _open((70, 67), levels, log)
    _all_same(maps, levels, log, off, "1024 headings", want, **kw)
    for m in maps:
        m.close()


BEAMS = (255, 256, 257, 1000, 4096)            # B + 1 counters in chunks of 1, 2 (257: the last lane's chunk is cut short), 4 and 17


@functools.lru_cache(maxsize=None)
def _beams_case(B):
    """the room in a corner of 70 x 67 (far from its walls every bound is 0: pruning is certain) under the quarter-turn beams and random
    ones up to B, a tenth of them SKIP"""
    log = np.full((67, 70), L_FREE)
    log[:41, :41] = _room_log()
    q = _quarter_turn_offsets()[:2]
    off = np.concatenate([q, _random_offsets(2, B - q.shape[1], 12, 9000 + B)], axis=1)
    assert off.shape == (2, B, 2) and 0.05 < (off[:, :, 0] == SKIP).mean() < 0.15
    wants = {cap: lx.expect(log, off, tol=0, min_score=1, cap=cap, free_only=False) for cap in (1, 16)}
    assert wants[16][2] > 4096
    return log, off, wants


@pytest.mark.parametrize("B", BEAMS)
def test_many_beams_the_thresholds_chunks(B):
    log, off, wants = _beams_case(B)
    levels = (None, "3")
    maps = _open((70, 67), levels, log, max_beams=4096)
    for cap, want in wants.items():
        _all_same(maps, levels, log, off, f"B {B}, cap {cap}", want, tol=0, min_score=1, cap=cap, free_only=False)
        st = maps[0].locate_stats()
        print(f"B {B}, cap {cap}: {st}")
        assert st["levels"] == 4, "unset: 2^(4 + 2) <= 70 < 2^(5 + 2), a level above the forced handle's"
        assert 0 < st["evaluated"][0] < 2 * 70 * 67, "the histogram's threshold pruned"
    for m in maps:
        m.close()


# ---- 3. the list limit ---------------------------------------------------------------------------------------------------------------
def _first_of_all_ones(w, cap):
    """every candidate scores 1: the order is k, y, x, so the first cap records (cap <= w * h) are k = 0 row by row"""
    i = np.arange(cap)
    rec = np.empty(cap, dtype=LOCATE_DTYPE)
    rec["score"], rec["k"], rec["x"], rec["y"] = 1, 0, i % w, i // w
    return rec


def _refused(m, off, **kw):
    """a host-form request that is to be refused: (code, message, the buffer with its guard records, n_out)"""
    t = _locate_table(off)
    lc = _locate_args(m.W, m.H, kw.pop("rect", None), t.shape, 0, False, kw.pop("min_score", 1), kw["cap"], False)
    buf = np.array([GUARD] * (kw["cap"] + 2), dtype=LOCATE_DTYPE)
    n = C.c_int32(-7)
    rc = load().gms_map_locate(m._h, 0, C.byref(lc), t.ctypes.data, t.shape[1], buf.ctypes.data, C.byref(n))
    return rc, load().gms_last_error().decode(), buf, n.value


@pytest.mark.parametrize("lv", ["0", None], ids=["exhaustive", "unset"])
def test_the_work_lists_limit(lv):
    """129 x 128 occupied cells under 1024 headings of one beam (0, 0): every candidate scores 1 and none can be pruned.  128 columns
    are exactly 2^24 candidates, the largest list there is; 129 are one column too many: the documented GMS_ERR_NOMEM, nothing written,
    and the handle answers as before afterwards (the level's append guard keeps every entry below the list's capacity and the host
    returns before anything reads a list whose counter went past it)."""
    import torch
    small = np.full((4, 5), L_OCC)
    want = lx.expect(small, np.zeros((3, 1, 2), np.int16), cap=16, free_only=False)
    assert want[1:] == (16, 60) and np.array_equal(want[0], _first_of_all_ones(5, 16)), "the analytic records against the expectation"
    shape, cap = (129, 128), 4096
    log = np.full((128, 129), L_OCC)
    off = np.zeros((1024, 1, 2), np.int16)
    full = (_first_of_all_ones(128, cap), cap)
    little_kw = dict(rect=(3, 5, 20, 11), tol=0, min_score=1, cap=16, free_only=False)
    little = lx.expect(log, off, **little_kw)
    m = _map(shape, lv)
    m.upload_log(log)

    def exactly_2_24(where):
        t0 = time.perf_counter()
        _same(m, log, off, where, want=full, rect=(0, 0, 128, 128), tol=0, min_score=1, cap=cap, free_only=False)
        print(f"levels {lv}, {where}: {time.perf_counter() - t0:.3f} s for the request of 2^24 survivors")
    exactly_2_24("exactly 2^24, lists allocated")
    exactly_2_24("exactly 2^24 again")
    for _ in range(1):
        rc, msg, buf, n = _refused(m, off, cap=cap)
        assert rc == GMS_ERR_NOMEM and "2^24" in msg, (rc, msg)
        assert buf.tolist() == [GUARD] * (cap + 2) and n == -7, "a refused request writes nothing"
        # the device form on the caller's stream
        stream = torch.cuda.Stream()
        m.set_stream(stream.cuda_stream)
        d_off = torch.from_numpy(off.reshape(-1).copy()).to("cuda")
        out = torch.full((16 * cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(GmsError) as e:
            m.locate_dev(d_off.data_ptr(), 1024, 1, out, n_out, tol=0, min_score=1, cap=cap, free_only=False)
        assert e.value.code == GMS_ERR_NOMEM and "2^24" in str(e.value)
        m.synchronize(); stream.synchronize(); torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all() and n_out.cpu().tolist() == [-7] * 4, "a refused request writes nothing"
        m.set_stream(None)
        # the handle afterwards: the counters the refused request left above the capacity are cleared
        _same(m, log, off, f"levels {lv}, after the refusal", want=little, **little_kw)
    exactly_2_24("exactly 2^24 after the refusals")
    m.close()


def test_more_than_int_max_candidates_are_refused():
    m = _map((2049, 1024))
    off = np.zeros((1024, 1, 2), np.int16)
    rc, msg, buf, n = _refused(m, off, cap=4)
    assert rc == GMS_ERR_INVALID and "2^31 - 1" in msg, (rc, msg)
    assert buf.tolist() == [GUARD] * 6 and n == -7
    rc, msg, buf, n = _refused(m, off, cap=4, rect=(1, 0, 2048, 1024))      # 2^31 itself
    assert rc == GMS_ERR_INVALID and "2^31 - 1" in msg and buf.tolist() == [GUARD] * 6 and n == -7
    got, n = _raw(m, off[:3], rect=(2040, 1020, 9, 4), cap=4)                 # the handle serves what is in range: an empty map has no hit
    assert n == 0 and got.tolist() == [lx.FILLER] * 4
    m.close()


# ---- 4. the device forms' precondition -----------------------------------------------------------------------------------------------
BEYOND = [(4096, 0), (0, -4096), (SKIP, 5), (5, SKIP), (-32768, -32767), (32767, 32767), (-4096, 4095)]


def _ranked(sc, free, min_score, cap, free_only):
    """the records of a score array [n_theta][H][W] (the whole map), by numpy's lexsort"""
    ok = sc >= min_score
    if free_only:
        ok &= free[None]
    k, y, x = np.nonzero(ok)
    s = sc[k, y, x]
    order = np.lexsort((x, y, k, -s))[:cap]
    rec = np.array([lx.FILLER] * cap, dtype=LOCATE_DTYPE)
    rec["score"][:len(order)], rec["k"][:len(order)], rec["x"][:len(order)], rec["y"][:len(order)] = s[order], k[order], x[order], y[order]
    return rec


@functools.lru_cache(maxsize=None)
def _beyond_case():
    """test_device_form_on_the_callers_stream's table with twelve pairs beyond the precondition; walls on the map's edges, so that a
    device that clamped such a pair's cell into the map, or kept 13 bits of each component, would count hits the expectation has not"""
    shape = (129, 65)
    log = _random_log(shape, 12965)
    log[:, 0] = log[:, 128] = log[0, :] = log[64, :] = L_OCC
    off = _random_offsets(8, 65, 12, 77)
    off[0, 0] = [4095, 4095]
    rng = np.random.default_rng(4096)
    where = [(int(k), int(b)) for k, b in zip(rng.integers(0, 8, 12), rng.choice(np.arange(1, 65), 12, replace=False))]
    bad = off.copy()
    as_skip = off.copy()
    for i, (k, b) in enumerate(where):
        bad[k, b] = BEYOND[i % len(BEYOND)]
        as_skip[k, b] = SKIP
    kw = dict(tol=2, min_score=6, cap=40, free_only=True)
    want = lx.expect(log, as_skip, **kw)
    assert want[1] == 40
    # what other treatments of those pairs would return
    hit = lx.hit_cells(log, 2)
    sc = lx.scores(log, as_skip, tol=2, hit=hit)
    with np.errstate(invalid="ignore"):
        free = log < 0
    assert np.array_equal(_ranked(sc, free, 6, 40, True), want[0]), "the ranking used below against the expectation's"
    ys, xs = np.mgrid[0:65, 0:129]
    clamped, wrapped = sc.copy(), sc.copy()
    for i, (k, b) in enumerate(where):
        dx, dy = BEYOND[i % len(BEYOND)]
        clamped[k] += hit[np.clip(ys + dy, 0, 64), np.clip(xs + dx, 0, 128)]
        wx, wy = ((dx + 4096) & 8191) - 4096, ((dy + 4096) & 8191) - 4096
        px, py = xs + wx, ys + wy
        wrapped[k] += hit[np.clip(py, 0, 64), np.clip(px, 0, 128)] & (px >= 0) & (px < 129) & (py >= 0) & (py < 65)
    assert not np.array_equal(_ranked(clamped, free, 6, 40, True), want[0]), "clamped into the map, the pairs would change the records"
    assert not np.array_equal(_ranked(wrapped, free, 6, 40, True), want[0]), "cut to 13 bits, the pairs would change the records"
    return log, bad, kw, want


def test_device_form_pairs_beyond_the_precondition_are_skipped():
    import torch
    log, bad, kw, want = _beyond_case()
    cap = kw["cap"]
    for lv in (None, "0"):
        m = _map((129, 65), lv)
        m.upload_log(log)
        with pytest.raises(GmsError) as e:
            _raw(m, bad, **kw)
        assert e.value.code == GMS_ERR_INVALID, "the host form refuses the table"
        stream = torch.cuda.Stream()
        m.set_stream(stream.cuda_stream)
        d_off = torch.from_numpy(bad.reshape(-1).copy()).to("cuda")
        out = torch.full((16 * cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.locate_dev(d_off.data_ptr(), 8, 65, out, n_out, **kw)
        stream.synchronize()
        raw = out.cpu().numpy()
        assert np.array_equal(raw[:16 * cap].view(LOCATE_DTYPE), want[0]), f"levels {lv}"
        assert (raw[16 * cap:] == 0xA5).all() and n_out.cpu().tolist() == [want[1], -7, -7, -7]
        m.set_stream(None)
        m.close()
