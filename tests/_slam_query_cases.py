"""The inputs of tests/test_gpu_slam_query_shapes.py and their expectations: the map queries (view, cast, clearance, reach, frontiers,
gain, rollout, locate, warp) with ONE PARTICLE'S MAP of a gms_slam handle as the source, on the thirteen shapes of
tests/test_gpu_query_shapes.py and 40 x 5.  Builders only, numpy, the oracle and the tests' plain expectations (_*_expect.py), no device code;
what the cases must contain is asserted in tests/test_slam_query_inputs.py.  Nobody writes to what a builder returns.

A handle has five slots, each with a log of its own (SLOT_LOGS: test_gpu_query_shapes.log_of) and a pose of its own (poses_of), so
that a read across a slot boundary, from the other generation or through a wrong row base lands in a map with another answer.
requests() lists the parameter sets of every query; Expect answers one of them for one (shape, log) in the canonical form the device
test compares: a tuple of arrays, every one compared byte for byte."""
import functools

import numpy as np

import _cast_expect as cx
import _clearance_expect as xe
import _frontier_expect as fx
import _gain_expect as gx
import _locate_expect as lx
import _reach_expect as rx
import _rollout_expect as ro
import _view_expect as ve
import _warp_expect as wx
import test_gpu_query_shapes as qs
from oracle import oracle as orc
from test_gpu_query_shapes import RANGES, RES, _odd_rect, _small_cap, log_of

# the thirteen shapes of tests/test_gpu_query_shapes.py and one more: their widths leave W % 16 in {0, 1, 6, 15} only, and 40 x 5 adds a
# row that starts in the middle of a code word (offset 8) on a plane with a ragged last word
SHAPES = list(qs.SHAPES) + [(40, 5)]
SLOT_LOGS = ("free", "unknown", "random", "second", "last column")
N = len(SLOT_LOGS)
MAX_BEAMS = 96                                             # the gain's probe fan
RAGGED = [s for s in SHAPES if s[0] * s[1] % 16 != 0]      # the last code word of a particle's plane is not full
EAGER_SHAPES = [(63, 65), (129, 65), (33, 2), (1, 70)]
WALK_MEM_SHAPES = [(63, 65), (65, 64)]
GEN1_SHAPES = [(63, 65), (129, 65), (31, 3)]
BATCH_SHAPE, BATCH_FILTERS, BATCH_N = (63, 65), 2, 3
BATCH_LOGS = (("random", "second", "last column"), ("second", "free", "random"))     # [filter][particle]: slot f * 3 + i differs from slot i
LIMIT_SHAPES = [(390, 252), (384, 256), (385, 256)]        # planes kept (24 576 bytes exactly), not kept (24 592), not kept
LIMIT_LOGS = ("random", "second")
LIMIT_RECT = (70, 40)
LOCATE_CAP = 32
ROLL_T = 40


# ---- slots ------------------------------------------------------------------------------------------------------------------------------
def _free_cell_near(shape, name, cx_, cy_):
    """the cell of log_of(shape, name) known free that lies nearest to (cx_, cy_): a cast from an occupied cell hits at step 0"""
    ys, xs = np.nonzero(log_of(shape, name) < 0)
    k = np.argmin((xs - cx_) ** 2 + (ys - cy_) ** 2)
    return int(xs[k]), int(ys[k])


@functools.lru_cache(maxsize=None)
def poses_of(shape):
    """float32 [5][3], slot k's pose: 0 the centre of corner cell (0, 0); 1 just off the map (the unknown map answers nothing
    anyway); 2 in the free cell of its log nearest to the middle; 3 in the free cell of its log nearest to the corner (W - 1, 0); 4
    the centre of corner cell (W - 1, H - 1), in the unobserved last column"""
    W, H = shape
    p = np.array([[0.5 * RES, 0.5 * RES, 0.3],
                  [-0.06, H * RES / 2, 0.0],
                  qs._cell_pose(*_free_cell_near(shape, SLOT_LOGS[2], W // 2, H // 2), 0.7),
                  qs._cell_pose(*_free_cell_near(shape, SLOT_LOGS[3], W - 1, 0), 2.0),
                  [(W - 0.5) * RES, (H - 0.5) * RES, -2.5]], dtype=np.float32)
    p.flags.writeable = False
    return p


@functools.lru_cache(maxsize=None)
def batch_poses():
    """float32 [2][3][3]: the batched handle's poses, three of poses_of per filter"""
    p = poses_of(BATCH_SHAPE)
    out = np.stack([p[[2, 3, 4]], p[[0, 2, 3]]])
    out.flags.writeable = False
    return out


def limit_poses(shape):
    W, H = shape
    p = np.array([qs._cell_pose(W - 30, H - 20, 0.7), qs._cell_pose(W - 1, H - 1, -2.5)], dtype=np.float32)
    p.flags.writeable = False
    return p


def limit_rect(shape):
    """70 x 40 cells that end at the last column and row"""
    return (shape[0] - LIMIT_RECT[0], shape[1] - LIMIT_RECT[1]) + LIMIT_RECT


# ---- the requests' constants ------------------------------------------------------------------------------------------------------------
def _cast_fan():
    """24 probes over the full circle, 0.3 m, 2 m and 12 m long in turn (12 m leaves the widest map, 9.6 m, on every side from any
    pose inside), probe 5 of length zero"""
    f = qs._fan(24, [0.3, 2.0, 12.0])
    f["local_x"][5] = f["local_y"][5] = f["distance"][5] = 0.0
    f.flags.writeable = False
    return f


FAN = _cast_fan()
POINTS = np.array([[0.06, 0.04], [-0.06, -0.04]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def arcs_of(shape):
    """six straight lines of ROLL_T steps from the start pose, 60 degrees apart, each 1.2 times the map's longer side long: from any
    pose inside some cross the last column and some the last row"""
    step = 1.2 * max(shape) * RES / ROLL_T
    ang = np.arange(6) * (np.pi / 3)
    d = step * np.arange(1, ROLL_T + 1)
    a = ro.steps(np.cos(ang)[:, None] * d[None, :], np.sin(ang)[:, None] * d[None, :], 1.0, 0.0)
    a.flags.writeable = False
    return a


def _offsets():
    """a twelve-beam offset table of two headings: end cells within six cells of the pose's, one beam skipped"""
    rng = np.random.default_rng(12)
    t = rng.integers(-6, 7, size=(2, 12, 2)).astype(np.int16)
    t[1, 7] = lx.SKIP
    t.flags.writeable = False
    return t


OFFSETS = _offsets()
WARP_POSES = ((0.0, 0.0, 1.0, 0.0), (2 * RES + 0.013, -RES, 1.0, 0.0))       # (tx, ty, c, s): the identity, and a shift


def requests(shape):
    """[(query, params)]: every request the device test sends for one slot, in order.  frontiers takes the cost field of the reach
    request REACH_FOR_FRONTIERS"""
    rects = (None, _odd_rect(shape))
    out = [("view", (rect, d, packed)) for rect in rects for d in (1, 3) for packed in (False, True)]
    out += [("cast", ())]
    out += [("clearance", (rect, R, not_free)) for not_free in (False, True) for R in (9, 255) for rect in rects]
    out += [("reach", (inflate, not_free, max_cost)) for inflate in (0, 2) for not_free in (True, False) for max_cost in (0xFFFE, _small_cap(shape))]
    out += [("frontiers", (min_size,)) for min_size in (1, 2)]
    out += [("gain", (R,)) for R in RANGES]
    out += [("rollout", (inflate, not_free)) for inflate, not_free in ((0, True), (1, False))]
    out += [("locate", (tol, free_only)) for tol in (0, 1) for free_only in (False, True)]
    out += [("warp", (k,)) for k in range(len(WARP_POSES))]
    return out


QUERIES = ("view", "cast", "clearance", "reach", "frontiers", "gain", "rollout", "locate", "warp")
REACH_FOR_FRONTIERS = (0, True, 0xFFFE)
USES_NOT_FREE = {"clearance": lambda p: p[2], "reach": lambda p: p[1], "rollout": lambda p: p[1]}


def limit_requests(shape):
    rect = limit_rect(shape)
    return [("cast", ()), ("clearance", (rect, 9, False)), ("clearance", (rect, 9, True)), ("view", (rect, 1, False)), ("view", (rect, 3, True))]


# ---- expectations -------------------------------------------------------------------------------------------------------------------------
def seeds_for(shape, log, not_free):
    """the seed set "both" of test_gpu_query_shapes.seeds_of for any log: (0, 0) -- on a thin map the first cell of every run of free
    cells -- and (W - 1, H - 1)"""
    W, H = shape
    first = ((0, 0),)
    if qs._thin(shape):
        first = tuple(qs._run_starts(~rx.blocked(log, 0, not_free))) or first
    return first + ((W - 1, H - 1),)


def _frozen(arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


class Expect:
    """the plain expectation of every request on one map: shape and its logData [H][W]; name: the log is log_of(shape, name), and the
    cached fields of tests/test_gpu_query_shapes.py serve"""

    def __init__(self, shape, log, name=None):
        self.shape, self.name, self.memo = shape, name, {}
        self.log = np.ascontiguousarray(log, dtype=np.float64).reshape(shape[1], shape[0])
        self.grid = qs._grid(shape)
        self.geo = ro.Geometry(shape[0], shape[1], RES, 0.0, 0.0)
        self.wgeo = wx.Geometry.make(shape[0], shape[1], RES, 0.0, 0.0)

    def _once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def seeds(self, not_free):
        if self.name is not None:
            return qs.seeds_of(self.shape, self.name, not_free, "both")
        return self._once(("seeds", not_free), lambda: seeds_for(self.shape, self.log, not_free))

    def cost(self, inflate, not_free):
        if self.name is not None:
            return qs.cost_of(self.shape, self.name, not_free, inflate, "both")
        return self._once(("cost", inflate, not_free), lambda: rx.costs(rx.blocked(self.log, inflate, not_free), self.seeds(not_free)))

    def field(self, R, not_free):
        if self.name is not None:
            return qs.clearance_of(self.shape, self.name, R, not_free)
        return self._once(("clear", R, not_free), lambda: xe.expect(self.log, R, not_free))

    def idx(self):
        return self._once("idx", lambda: ve.idx_map(self.log, False))

    def walks(self):
        return qs.walks_of(self.shape)

    def answer(self, query, params, pose, dst_log=None):
        """the canonical result of one request: a tuple of arrays.  pose: the slot's own (cast, rollout); dst_log: the destination
        of the warp"""
        key = (query, params) + ((tuple(np.asarray(pose, np.float32).tolist()),) if query in ("cast", "rollout") else ())
        return self._once(key, lambda: _frozen(self._answer(query, params, pose, dst_log)))

    def _answer(self, query, params, pose, dst_log):
        W, H = self.shape
        if query == "view":
            rect, d, packed = params
            return (ve.expect(self.idx(), rect or (0, 0, W, H), d, False, packed),)
        if query == "cast":
            return (cx.expect(self.grid, self.log, FAN, pose),)
        if query == "clearance":
            rect, R, not_free = params
            x0, y0, w, h = rect or (0, 0, W, H)
            if self.name is None and rect is not None and W * H > 20000:
                return (xe.expect(self.log, R, not_free, rect=rect),)
            return (np.ascontiguousarray(self.field(R, not_free)[y0:y0 + h, x0:x0 + w]),)
        if query == "reach":
            inflate, not_free, max_cost = params
            return (rx.cap(self.cost(inflate, not_free), max_cost),)
        if query == "frontiers":
            cost = self.answer("reach", REACH_FOR_FRONTIERS, None)[0]
            rec, n, lab = fx.expect(self.log, min_size=params[0], inflate=0, cost=cost)
            return (rec, np.array([n], dtype=np.int64), lab)
        if query == "gain":
            return (gx.expect_walks(self.walks(), self.log, params[0]),)
        if query == "rollout":
            inflate, not_free = params
            return (ro.expect(self.geo, self.log, np.asarray(pose, np.float32).reshape(1, 3), arcs_of(self.shape), POINTS, 255, inflate, not_free),)
        if query == "locate":
            tol, free_only = params
            rec, n_out, _ = lx.expect(self.log, OFFSETS, tol=tol, not_free=False, min_score=1, cap=LOCATE_CAP, free_only=free_only)
            return (rec, np.array([n_out], dtype=np.int64))
        assert query == "warp"
        _, st = wx.expect(dst_log, self.wgeo, self.log, self.wgeo, WARP_POSES[params[0]], "compare")
        return (np.ascontiguousarray(st["pair"]).astype(np.int64).reshape(3, 3), np.array([int(st["n_outside"])], dtype=np.int64))


@functools.lru_cache(maxsize=None)
def expect_of(shape, name):
    return Expect(shape, log_of(shape, name), name)


def warp_dst_log(shape):
    """what the destination of the warps holds: the shape's random log"""
    return log_of(shape, "random")


def same_bytes(a, b):
    """two canonical results, byte for byte (doubles with their NaN and -0.0 bits)"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- code words ---------------------------------------------------------------------------------------------------------------------------
def shared_word_cells(shape):
    """bool [H][W]: the cells whose code word (sixteen 2-bit codes, word (x + y * W) >> 4) also holds cells of another row"""
    W, H = shape
    c = np.arange(W * H, dtype=np.int64)
    lo, hi = (c >> 4) * 16, np.minimum((c >> 4) * 16 + 15, W * H - 1)
    return (lo // W != hi // W).reshape(H, W)


def last_word_cells(shape):
    """bool [H][W]: the cells of the plane's last code word"""
    W, H = shape
    c = np.arange(W * H, dtype=np.int64)
    return ((c >> 4) == ((W * H - 1) >> 4)).reshape(H, W)


def cast_walk_cells(shape, k):
    """bool [H][W]: the cells slot k's fan walks over, hit or not (the planned walks, cut at the map's edge)"""
    W, H = shape
    on = np.zeros((H, W), dtype=bool)
    for _, cells in cx.walks(qs._grid(shape), FAN, poses_of(shape)[k]):
        c = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        c = c[(c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H)]
        on[c[:, 1], c[:, 0]] = True
    return on


# ---- generation 1: one update, then a resampling that moves maps -------------------------------------------------------------------------------
def _scan():
    """a hand-made scan of eight short beams, hits and misses"""
    ang = np.array([0.0, 0.8, 1.6, 2.4, 3.1, -2.3, -1.5, -0.7])
    dist = np.array([0.22, 0.4, 0.31, 0.55, 0.18, 0.47, 0.36, 0.6])
    z = orc.make_beams(dist * np.cos(ang), dist * np.sin(ang), dist, np.array([1, 1, 0, 1, 1, 0, 1, 1]))
    z.flags.writeable = False
    return z


SCAN = _scan()
SCAN2 = orc.make_beams(*(np.array(v) for v in ([0.3, -0.2, 0.1], [0.1, 0.25, -0.35], [0.31622776601683794, 0.32015621187164245, 0.36400549446402586], [1, 1, 0])))
SCAN2.flags.writeable = False


def oracle_after_update(shape, names=SLOT_LOGS, poses=None):
    """the oracle's filter (orc.Slam) holding the slots' logs and poses behind ONE update with SCAN and no odometry"""
    poses = poses_of(shape) if poses is None else poses
    o = orc.Slam(qs._grid(shape), len(names))
    for k, name in enumerate(names):
        o.set_log(k, log_of(shape, name))
    o.set_poses(poses)
    o.update(np.array(SCAN), None)
    return o


@functools.lru_cache(maxsize=None)
def resampling_draw(shape):
    """(r01, indices, maps [5][H * W] behind the update): a draw whose indices are not the identity, move at least one map into a
    slot whose own differs, and stay the same for r01 +- 1e-6 (so that the device's last-bit differences in the weights cannot
    change them), searched over r01 = 0.05, 0.15, ... with the oracle alone"""
    o = oracle_after_update(shape)
    w, logs = o.weights, o.logs()
    for r01 in np.arange(0.05, 1.0, 0.1):
        idx = orc.resample_indices(w, float(r01))[0]
        if any(not np.array_equal(orc.resample_indices(w, float(r01) + e)[0], idx) for e in (-1e-6, 1e-6)):
            continue
        moved = [k for k in range(N) if idx[k] != k and logs[k].tobytes() != logs[idx[k]].tobytes()]
        if moved:
            want = o.resample(float(r01))[0]
            assert np.array_equal(want, idx)
            return (float(r01),) + _frozen((np.array(idx, dtype=np.int32), logs))
    raise AssertionError(f"{shape}: no draw moves a map")


# ---- the batched handle: one update, then a resample_if that one filter meets -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_draw():
    """(Neff [2] of the oracle's two filters behind ONE update with SCAN, the fraction of resample_if): the fraction lies midway
    between the filters' Neff / n, so that `neff < fraction * n` holds for exactly one of them"""
    neff = np.array([oracle_after_update(BATCH_SHAPE, BATCH_LOGS[f], batch_poses()[f]).neff() for f in range(BATCH_FILTERS)])
    neff.flags.writeable = False
    return neff, float(neff.sum()) / 2 / BATCH_N
