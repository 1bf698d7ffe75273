"""The inputs of tests/test_gpu_slam_align_edges.py and their expectations: the per-particle scan alignment (k_slam_align) at the edges
of its own code -- the widest and narrowest blur kernels, maps narrower and lower than the blur, class planes written from uploaded
logData, the stopping rules of its workgroup-uniform loop, scans of one pass of sixteen beams more or less, non-finite beams, the
gate between its two forms, an origin far from zero.  Builders only, CPU only: the oracle brings the maps there, the restatement
(tests/_align_expect.py through test_gpu_slam_align._expect) says what the device must return.  What every case must contain is
asserted in tests/test_slam_align_edge_inputs.py, so that a green device test cannot hide an empty comparison.

A Case holds what brings a fresh handle to the oracle's state (`steps`), the logData the expectation is computed from (`logs`) and
the calls to make (`calls`).  Nobody writes to what a builder returns."""
import functools
import math
from collections import namedtuple

import numpy as np

import _align_expect as ax
from gridmap_slam_robot_amd import synth
from gridmap_slam_robot_amd._lib import BEAM_DTYPE
from oracle import oracle as orc

from test_gpu_slam_align import GEO80, THREADS, _expect, _particles, _prm, _scene
from test_gpu_slam_no_planes import TAPS_15 as _GAUSS_15

RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
SPECIALS = (-0.0, float("nan"), 5e-324, -5e-324, float("inf"), float("-inf"))
N_SPECIAL = 60

Call = namedtuple("Call", "label z P prm")


# ---- what the launcher and the kernel do with a map and a kernel, restated -------------------------------------------------------------
LDS_PER_CU = 163840                      # gms_internal.h: 160 KiB per compute unit on this part
MAX_PLANE_BYTES = 24 * 1024              # gms_slam_create keeps a plane up to this size ...
MAX_PLANE_KHALF = 7                      # ... for kernels of up to fifteen taps


def code_words(cells):
    """32-bit words per class plane: sixteen cells a word, one spare word, a multiple of four"""
    return ((cells + 15) // 16 + 1 + 3) & ~3


def last_word(cells):
    """the index of the word behind the last one that holds a cell: the spare word a window may run into"""
    return (cells + 15) // 16


def planes_kept(W, H, ntaps, eager=False):
    return not eager and (ntaps - 1) // 2 <= MAX_PLANE_KHALF and 4 * code_words(W * H) <= MAX_PLANE_BYTES


def takes_planes(W, H, ntaps, B, eager=False, forced_memory=False):
    """gms_slam_align_from_planes: the planes are kept, nothing forces the memory form, and 48 bytes per padded beam, the plane and
    4 KiB fit a compute unit's LDS"""
    if forced_memory or not planes_kept(W, H, ntaps, eager):
        return False
    Bpad = 8 if B < 8 else (B + 7) & ~7
    return 48 * Bpad + 4 * code_words(W * H) + 4096 <= LDS_PER_CU


def taps_plain(taps):
    """gms_map::taps_plain: every tap is +0.0 or lies in [2^-900, 2^900]; a negative tap, a -0.0 or a tap outside clears it and the
    on-demand sums take the literal form"""
    return all(not math.copysign(1.0, a) < 0 and (a == 0.0 or 2.0 ** -900 <= a <= 2.0 ** 900) for a in taps)


# ---- a case ----------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; size (metres), origin, N, taps (None: the map's default), max_beams: the handle; g: the oracle's grid; steps: what brings
    a fresh handle to the state -- ("update", poses, scan), ("upload", logs), ("weights", w), ("resample", r01, indices),
    ("reset",) --; logs [N]: every particle's logData in that state; calls: the alignments to compare"""

    def __init__(self, name, size, origin, N, taps, g, steps, logs, calls, max_beams=128):
        self.name, self.size, self.origin, self.N, self.taps, self.g = name, size, origin, N, taps, g
        self.steps, self.logs, self.calls, self.max_beams = steps, logs, calls, max_beams
        self.kernel = tuple(float(t) for t in g.kernel)
        self.ntaps, self.kh, self.plain = len(self.kernel), (len(self.kernel) - 1) // 2, taps_plain(self.kernel)
        for a in list(logs) + [c.z for c in calls] + [c.P for c in calls]:
            a.setflags(write=False)

    @functools.cached_property
    def _ran(self):
        out = []
        for c in self.calls:
            seen = []
            out.append((_expect(self.g, c.z, c.P, c.prm, logs=self.logs, visit=lambda *a: seen.append(a)), seen))
        return out

    @property
    def want(self):
        """per call: (poses float32 [N][3], records as a dict of arrays)"""
        return [w for w, _ in self._ran]

    @property
    def visits(self):
        """per call: [(particle, evaluation, beam, i0, j0)] of every used beam"""
        return [v for _, v in self._ran]

    def form(self, B, eager=False, forced_memory=False):
        return "planes" if takes_planes(self.g.W, self.g.H, self.ntaps, B, eager, forced_memory) else "memory"

    def fields(self):
        """every particle's field, float64 [N][H * W]"""
        return [self.g.build_likelihood(np.asarray(l, np.float64).reshape(-1)) for l in self.logs]


def end_cells(case, call=0):
    """int64 [n][2]: the distinct first cells (i0, j0) of the call's used beams, over every particle and evaluation"""
    v = case.visits[call]
    return np.unique(np.array([(a[3], a[4]) for a in v], np.int64).reshape(-1, 2), axis=0)


def windows(case, call=0):
    """what sa_hsum / sa_hsum_plain are asked for over the call's used beams: per (end cell, column gx in {i0, i0 + 1}, row y of
    j0 - kh .. j0 + kh + 1 inside the map) the window's first cell c0 -- y W + gx - kh in the plain form, y W + gx + max(-kh, -gx) in
    the literal one --, and the clips of the columns tlo = max(0, kh - gx), thi = min(2 kh, W - 1 - gx + kh).
    Returns int64 [n][6]: c0, gx, y, tlo, thi, j0"""
    W, H, kh = case.g.W, case.g.H, case.kh
    rows = []
    for i0, j0 in end_cells(case, call):
        for gx in (i0, i0 + 1):
            for y in range(j0 - kh, j0 + kh + 2):
                if 0 <= y < H:
                    c0 = y * W + gx - kh if case.plain else y * W + gx + max(-kh, -gx)
                    rows.append((c0, gx, y, max(0, kh - gx), min(2 * kh, W - 1 - gx + kh), j0))
    return np.array(rows, np.int64).reshape(-1, 6)


def words_read(case, call=0):
    """the plane's words the call's windows are taken from: (c0 >> 4) and the one behind it (an arithmetic shift: word -1 for c0 < 0)"""
    c0 = windows(case, call)[:, 0]
    return np.unique(np.concatenate([c0 >> 4, (c0 >> 4) + 1]))


def beam_to(g, pose, i0, j0, fx=0.5, fy=0.5):
    """(local_x, local_y) of a beam that, seen from `pose`, ends fx, fy into the interpolation cell (i0, j0)"""
    res, px, py = (float(np.float32(v)) for v in (g.resolution, g.pos[0], g.pos[1]))
    c, s = (float(v) for v in orc.pose_trig(np.float32(pose[2])))
    X, Y = px + (i0 + 0.5 + fx) * res - float(pose[0]), py + (j0 + 0.5 + fy) * res - float(pose[1])
    return X * c + Y * s, -X * s + Y * c


def pose_for(g, lx, ly, theta, i0, j0, fx, fy):
    """the pose with heading theta from which the beam (lx, ly) ends fx, fy into cell (i0, j0): as
    test_end_points_at_the_maps_edges_and_poses_that_use_no_beam builds them"""
    res, px, py = (float(np.float32(v)) for v in (g.resolution, g.pos[0], g.pos[1]))
    c, s = orc.pose_trig(np.float32(theta))
    return (px + (i0 + fx + 0.5) * res - (lx * c - ly * s), py + (j0 + fy + 0.5) * res - (lx * s + ly * c), theta)


def with_corner_beams(g, z, pose):
    """the scan with its first two beams replaced by hits that `pose` sees in the cells (0, 0) and (W - 2, H - 2): the windows that
    begin in front of the plane and the ones that end in the spare word behind it"""
    z = z.copy()
    for b, (i0, j0) in enumerate(((0, 0), (g.W - 2, g.H - 2))):
        lx, ly = beam_to(g, pose, i0, j0)
        z["local_x"][b], z["local_y"][b], z["distance"][b], z["hit"][b] = lx, ly, math.hypot(lx, ly), 1
    return z


def _shifted(P, shift):
    return (np.asarray(P, np.float64) + np.array([shift[0], shift[1], 0.0])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene_at(W, H, res, N, B, T, origin, seed=61):
    """test_gpu_slam_align._scene with the map's corner at `origin` instead of (-W / 2, -H / 2): the room, the particles and the true
    poses move with it.  (grid, oracle filter, trace, shift)"""
    shift = (origin[0] + W / 2, origin[1] + H / 2)
    tr = synth.make_trace(min(W, H, 6.4), res, B, T=T + 5, seed=seed)
    g = orc.Grid(W, H, res, origin[0], origin[1])
    o = orc.Slam(g, N)
    for k in range(T):
        o.set_poses(_shifted(_particles(tr, k, N), shift))
        o.update(tr.scans[k], None, threads=THREADS)
    return g, o, tr, shift


def _from_scene(name, W, H, N, B, T, taps, prm, corners=False, origin=None, z=None):
    """a case whose maps come from T updates at perturbed particles and whose call is the scan behind them"""
    if origin is None:
        g, o, tr = _scene(W, H, RES, N, B, T, taps)
        shift, origin = (0.0, 0.0), (-W / 2, -H / 2)
    else:
        g, o, tr, shift = scene_at(W, H, RES, N, B, T, origin)
    steps = [("update", _shifted(_particles(tr, k, N), shift), tr.scans[k]) for k in range(T)]
    P = _shifted(_particles(tr, T, N), shift)
    z = tr.scans[T] if z is None else z(tr.scans[T])
    if corners:
        z = with_corner_beams(g, z, P[0])
    return Case(name, (W, H), origin, N, taps, g, steps, [o.log(i).copy() for i in range(N)], [Call("scan", z, P, prm)])


# ---- blur widths -------------------------------------------------------------------------------------------------------------------------
TAPS_15 = tuple(float(t) for t in _GAUSS_15)
_G13 = tuple(float(t) for t in orc.gaussian_kernel(1.8, 6))
TAPS = {
    "one_tap": (1.0,),
    "three_taps": (0.25, 0.5, 0.25),
    "thirteen_taps": _G13,
    "fifteen_taps": TAPS_15,
    "fifteen_taps_zero_ends": (0.0,) + _G13 + (0.0,),
    # the literal form: a tap below 2^-900 in each; asymmetric where the width allows, so that a tap taken from the wrong end shows
    "one_tap_literal_tiny": (1e-300,),
    "three_taps_literal_tiny": (1e-300, 0.6, 0.4),
    "thirteen_taps_literal_tiny": (1e-300,) + _G13[1:],
    "fifteen_taps_literal_tiny": TAPS_15[:-1] + (1e-300,),
    "fifteen_taps_literal_negative": (-0.01,) + TAPS_15[1:-1] + (-0.01,),
    # (beyond the list: one tap of 1e-300 gives a field of 0.0 everywhere -- the products underflow --, so one tap in the literal form
    # gets a second case whose field is not constant)
    "one_tap_literal_negative": (-1.0,),
}
TAP_WIDTHS = {"one_tap": 1, "three_taps": 3, "thirteen_taps": 13, "fifteen_taps": 15, "fifteen_taps_zero_ends": 15, "one_tap_literal_tiny": 1,
              "three_taps_literal_tiny": 3, "thirteen_taps_literal_tiny": 13, "fifteen_taps_literal_tiny": 15, "fifteen_taps_literal_negative": 15,
              "one_tap_literal_negative": 1}
TAP_CASES = tuple(TAPS)
CONSTANT_FIELD = ("one_tap_literal_tiny",)           # no pose can move on it: every value is 0.0


def is_literal(name):
    return "literal" in name


@functools.lru_cache(maxsize=None)
def tap_case(name):
    """80 x 80 cells, 8 particles, 72 beams, three warm-up updates, the scan with the two corner beams"""
    return _from_scene(name, 4.0, 4.0, 8, 72, 3, TAPS[name], _prm(iters=4), corners=True)


# ---- narrower and lower than the blur ----------------------------------------------------------------------------------------------------
NARROW_SHAPES = {"9x33": (0.45, 1.65), "33x9": (1.65, 0.45), "9x9": (0.45, 0.45)}      # (9 x 9, beyond the list: every clip at once)
NARROW_CASES = tuple((s, k) for s in NARROW_SHAPES for k in ("fifteen_taps", "fifteen_taps_literal_tiny"))


@functools.lru_cache(maxsize=None)
def narrow_case(shape, kernel):
    W, H = NARROW_SHAPES[shape]
    c = _from_scene(f"{shape} {kernel}", W, H, 8, 48, 3, TAPS[kernel], _prm(iters=4))
    assert f"{c.g.W}x{c.g.H}" == shape
    return c


# ---- planes written from uploaded logData ------------------------------------------------------------------------------------------------
UPLOAD_SHAPES = {"51x67": (2.55, 3.35), "80x80": (4.0, 4.0)}
UPLOAD_STAGES = ("uploaded", "resampled", "reset")
UPLOAD_CASES = tuple((s, t) for s in UPLOAD_SHAPES for t in UPLOAD_STAGES)
UPLOAD_R01 = 0.37


@functools.lru_cache(maxsize=None)
def upload_logs(shape, N=8):
    """[N] of float64 [H][W]: 5 % occupied, 45 % free, the rest 0.0; sixty cells each of -0.0, NaN, the two smallest subnormals and the
    infinities"""
    W, H = (int(v) for v in shape.split("x"))
    rng = np.random.default_rng(W * 1000 + H)
    logs = []
    for _ in range(N):
        u = rng.random(W * H)
        log = np.where(u < 0.05, L_OCC, np.where(u < 0.5, L_FREE, 0.0))
        at = rng.choice(W * H, len(SPECIALS) * N_SPECIAL, replace=False)
        for k, v in enumerate(SPECIALS):
            log[at[k * N_SPECIAL:(k + 1) * N_SPECIAL]] = v
        log = log.reshape(H, W)
        log.setflags(write=False)
        logs.append(log)
    return logs


def upload_weights(N=8):
    w = np.random.default_rng(8).random(N) ** 3
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def upload_case(shape, stage):
    """a synthetic scan seen from perturbed poses, and one beam seen from eight poses: its end point in the four corner cells
    (0 | W - 2, 0 | H - 2) -- the windows that start in word -1 and end in the spare word -- and just outside the map on each side.
    uploaded: as set_map left it.  resampled: one draw behind the uploads (the planes of the other generation).  reset: behind that,
    reset() -- every class 0, the field 0.5 wherever the blur's reach stays inside the map"""
    W, H = UPLOAD_SHAPES[shape]
    N = 8
    g = orc.Grid(W, H, RES, -W / 2, -H / 2)
    assert f"{g.W}x{g.H}" == shape
    up = upload_logs(shape, N)
    steps, logs = [("upload", up)], up
    if stage != "uploaded":
        w = upload_weights(N)
        idx, clamped = orc.resample_indices(w, UPLOAD_R01)
        assert clamped == 0
        steps += [("weights", w), ("resample", UPLOAD_R01, np.asarray(idx, np.int64))]
        logs = [up[j] for j in idx]
    if stage == "reset":
        steps.append(("reset",))
        logs = [np.zeros((g.H, g.W)) for _ in range(N)]
    tr = synth.make_trace(min(W, H), RES, 72, T=6, seed=71)
    lx, ly = 0.30, -0.20
    z1 = np.zeros(1, BEAM_DTYPE)
    z1["local_x"], z1["local_y"], z1["hit"], z1["distance"] = lx, ly, 1, math.hypot(lx, ly)
    inside = [(0, 0.25, 0, 0.25), (g.W - 2, 0.75, 0, 0.25), (0, 0.25, g.H - 2, 0.75), (g.W - 2, 0.75, g.H - 2, 0.75)]
    outside = [(-1, 0.75, 0, 0.25), (g.W - 1, 0.25, g.H - 2, 0.75), (0, 0.25, -1, 0.75), (g.W - 2, 0.75, g.H - 1, 0.25)]
    P1 = np.array([pose_for(g, lx, ly, (0.7, -2.4)[k & 1], i0, j0, fx, fy) for k, (i0, fx, j0, fy) in enumerate(inside + outside)], np.float32)
    calls = [Call("scan", tr.scans[0].copy(), _particles(tr, 0, N), _prm(iters=4)), Call("one beam", z1, P1, _prm(iters=3))]
    return Case(f"{shape} {stage}", (W, H), (-W / 2, -H / 2), N, None, g, steps, [np.array(l) for l in logs], calls)


def special_cells_in_reach(case, i, call=0):
    """per special value: how many of particle i's cells that hold it lie within the blur's reach of one of its used end points' four
    cells (columns i0 - kh .. i0 + 1 + kh, rows j0 - kh .. j0 + 1 + kh)"""
    H, W, kh = case.g.H, case.g.W, case.kh
    reach = np.zeros((H, W), bool)
    for a in case.visits[call]:
        if a[0] == i:
            reach[max(0, a[4] - kh):a[4] + kh + 2, max(0, a[3] - kh):a[3] + kh + 2] = True
    log = np.asarray(case.logs[i]).reshape(H, W)
    bits = log.view(np.uint64)
    return [int((reach & (bits == np.float64(v).view(np.uint64))).sum()) if v == v else int((reach & np.isnan(log)).sum()) for v in SPECIALS]


# ---- the stopping rules of the workgroup-uniform loop --------------------------------------------------------------------------------------
STOP_CASES = ("converged", "singular_on_reset", "det_min_above", "det_min_equal", "det_min_below", "clamps", "iters_64", "mixed_stops")
CHAIN_PRM = dict(eps_t=0.05, eps_r=1e-3)             # tests/test_gpu_align.py::test_k_iterations_equal_k_chained_single_steps
CHAIN_K = 5
CLAMP_T, CLAMP_R = 0.05, 0.002


def first_step(case, i, prm, call=0):
    """(det, [delta before the clamp]) of particle i's first step, from the restatement's own functions"""
    g, c = case.g, case.calls[call]
    res, px, py = (float(np.float32(v)) for v in (g.resolution, g.pos[0], g.pos[1]))
    L = g.build_likelihood(np.asarray(case.logs[i], np.float64).reshape(-1))
    Hm, gv, _, n = ax.evaluate(L, g.W, g.H, res, px, py, c.z, c.P[i])
    det, num = ax.solve(Hm, gv, prm["damp_t"], prm["damp_r"])
    return det, ([v / det for v in num] if det != 0.0 else None), n


@functools.lru_cache(maxsize=None)
def stop_case(name):
    """the 80 x 80 scene of tests/test_gpu_slam_align.py with 24 particles, under the parameter sets of tests/test_gpu_align.py"""
    W, H, _, N, B, T = GEO80
    if name == "singular_on_reset":                  # a map never observed: the field is constant where the beams end, H = 0, no damping
        g, _, tr = _scene(*GEO80)
        logs = [np.zeros((g.H, g.W)) for _ in range(N)]
        return Case(name, (W, H), (-W / 2, -H / 2), N, None, g, [("reset",)], logs,
                    [Call("scan", tr.scans[T].copy(), _particles(tr, T, N), _prm(damp_t=0.0, damp_r=0.0))])
    if name.startswith("det_min"):
        base = _from_scene("det", W, H, N, B, T, None, _prm())
        det, _, n = first_step(base, 0, _prm())
        assert n > 0 and det > 1.0
        det_min = {"det_min_above": np.nextafter(det, np.inf), "det_min_equal": det, "det_min_below": np.nextafter(det, 0.0)}[name]
        prm = _prm(iters=1, eps_t=0.0, eps_r=0.0, det_min=float(det_min))
    else:
        prm = {"converged": _prm(eps_t=10.0, eps_r=10.0), "clamps": _prm(iters=4, max_t=CLAMP_T, max_r=CLAMP_R),
               "iters_64": _prm(iters=64, eps_t=0.0, eps_r=0.0), "mixed_stops": _prm(iters=8, **CHAIN_PRM)}[name]
    return _from_scene(name, W, H, N, B, T, None, prm)


@functools.lru_cache(maxsize=None)
def chain_case():
    """iters = 5 in one call; the device test sets it against five calls of iters = 1"""
    W, H, _, N, B, T = GEO80
    return _from_scene("chain", W, H, N, B, T, None, _prm(iters=CHAIN_K, **CHAIN_PRM))


# ---- beams -------------------------------------------------------------------------------------------------------------------------------
BEAM_COUNTS = (15, 16, 17)                           # one pass of the field's values takes sixteen beams
BAD_BEAMS = ((float("nan"), None), (None, float("nan")), (float("inf"), None), (None, float("inf")), (float("-inf"), None),
             (None, float("-inf")), (float("nan"), float("nan")), (float("inf"), float("-inf")))


@functools.lru_cache(maxsize=None)
def beam_count_case(B):
    return _from_scene(f"B = {B}", 4.0, 4.0, 8, B, 2, None, _prm(iters=3))


def bad_beam_indices(z):
    """eight beams that hit, spread over the scan"""
    hits = np.flatnonzero(z["hit"])
    return hits[np.linspace(0, len(hits) - 1, len(BAD_BEAMS)).astype(int)]


def _spoil(z):
    z = z.copy()
    for b, (x, y) in zip(bad_beam_indices(z), BAD_BEAMS):
        if x is not None:
            z["local_x"][b] = x
        if y is not None:
            z["local_y"][b] = y
    return z


@functools.lru_cache(maxsize=None)
def non_finite_case():
    """72 beams, eight of them with hit = 1 and a NaN or an infinity in local_x or local_y"""
    return _from_scene("non-finite beams", 4.0, 4.0, 8, 72, 3, None, _prm(iters=4), z=_spoil)


@functools.lru_cache(maxsize=None)
def clean_case():
    """non_finite_case with the scan as the trace made it"""
    return _from_scene("clean beams", 4.0, 4.0, 8, 72, 3, None, _prm(iters=4))


# ---- the gate between the forms ------------------------------------------------------------------------------------------------------------
GATE_SIZE, GATE_CELLS = (15.68, 15.62), (314, 313)   # the largest plane that is kept: exactly 24 576 bytes
GATE_ORDER = (72, 2816, 72, 2817)                    # the second call needs more LDS than the first was granted; the fourth none
GATE_WANT = ("planes", "planes", "planes", "memory")
NO_PLANES_SIZE, NO_PLANES_CELLS = (15.68, 15.68), (314, 314)


def _gate(name, size, cells, order, max_beams):
    W, H = size
    N, seed = 2, 67
    g = orc.Grid(W, H, RES, -W / 2, -H / 2)
    assert (g.W, g.H) == cells
    traces = {B: synth.make_trace(6.4, RES, B, T=3, seed=seed) for B in set(order) | {72}}
    o = orc.Slam(g, N)
    P0 = _particles(traces[72], 0, N)
    o.set_poses(P0)
    o.update(traces[72].scans[0], None, threads=THREADS)
    prm = _prm(iters=2)
    calls = [Call(f"B = {B}", traces[B].scans[1].copy(), _particles(traces[B], 1, N), prm) for B in order]
    return Case(name, size, (-W / 2, -H / 2), N, None, g, [("update", P0, traces[72].scans[0].copy())], [o.log(i).copy() for i in range(N)], calls,
                max_beams=max_beams)


@functools.lru_cache(maxsize=None)
def gate_case():
    return _gate("314x313", GATE_SIZE, GATE_CELLS, GATE_ORDER, 2880)


@functools.lru_cache(maxsize=None)
def no_planes_case():
    return _gate("314x314", NO_PLANES_SIZE, NO_PLANES_CELLS, (72,), 128)


# ---- an origin far from zero -------------------------------------------------------------------------------------------------------------
FAR_ORIGINS = {"1000_-2000": (1000.0, -2000.0), "-4096_4096": (-4096.0, 4096.0)}


@functools.lru_cache(maxsize=None)
def far_case(name):
    return _from_scene(f"origin {name}", 4.0, 4.0, 8, 72, 3, None, _prm(iters=4), corners=True, origin=FAR_ORIGINS[name])
