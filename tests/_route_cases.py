"""Hand-built inputs of the routes (include/gridmapslam.h "routes") that isolate one rule each: tests/test_route_inputs.py proves on
the host, with tests/_route_expect.py alone, that every family has the property it exists for; tests/test_gpu_route_edges.py runs
them on the device.  Pure numpy, nothing random.  A Case is a map (W, H), its logData, a uint16 cost field and named start cells; the
families differ in what the field and the plane hold:

  A  descent rules       gadgets a few cells across in a field that is FAR everywhere else, on a free map
  B  the longest descent a boustrophedon of 13107 cells over 200 x 136, on a free map
  C  closed supercover   L paths with one occupied cell in their bounding box; a 4097-cell chain in a map 4100 x 40
  D  pass edges          one-cell-wide corridors in a map that is occupied everywhere else"""
import functools

import numpy as np

import _rollout_expect as rx
import _route_expect as rt

FAR = rt.FAR
RES = 0.05
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
FILL = 60000                     # a cell that is not FAR and that no current cell of any gadget can step to: every current cost is below it
E, N, W_, S, NE, NW, SW, SE = range(8)
NAMES = ("E", "N", "W", "S", "NE", "NW", "SW", "SE")


class Case:
    def __init__(self, name, W, H, field, log, starts=None, meta=None):
        self.name, self.W, self.H = name, W, H
        self.field, self.log = field, log
        self.starts = starts or {}            # name -> (x, y)
        self.meta = meta or {}
        for a in (self.field, self.log):
            a.flags.writeable = False

    @functools.cached_property
    def blocked(self):
        b = rx.blocked_plane(self.log, 0, True)
        b.flags.writeable = False
        return b

    def size_m(self):
        return (self.W - 0.4) * RES, (self.H - 0.4) * RES

    def cells_of(self, names):
        return np.array([self.starts[n] for n in names], np.int32).reshape(-1, 2)


def _put(field, cells, at=(0, 0)):
    for (x, y), v in cells.items():
        assert field[at[1] + y, at[0] + x] == FAR, "gadgets overlap"
        field[at[1] + y, at[0] + x] = v


# ---- family A ------------------------------------------------------------------------------------------------------------------
A_W, A_H = 340, 330
A_CENTRE = 35                    # 35 - 5 = 30 falls to 0 along an axis, 35 - 7 = 28 along a diagonal: every neighbour has an arm of its own


def _gadget_subset(mask):
    """3 x 3 block whose centre costs 35; neighbour k of `mask` is admissible (axis 30, diagonal 28) and leads along its own straight
    arm to its own seed; the other neighbours hold FILL, so every diagonal's sides are not FAR"""
    g = {(0, 0): A_CENTRE}
    for k, (dx, dy) in enumerate(rt.ORDER):
        if not mask >> k & 1:
            g[(dx, dy)] = FILL
            continue
        step = rt.DIAG if dx and dy else rt.AXIS
        for r in range(1, A_CENTRE // step + 1):
            g[(r * dx, r * dy)] = A_CENTRE - step * r
            if dx and dy and r < A_CENTRE // step:                             # the sides of the arm's next diagonal step
                g.setdefault(((r + 1) * dx, r * dy), FILL)
                g.setdefault((r * dx, (r + 1) * dy), FILL)
    return g


def _gadget_single(k):
    """neighbour k alone is admissible, and is a seed; everything else FAR but a diagonal's two sides"""
    dx, dy = rt.ORDER[k]
    g = {(0, 0): rt.DIAG if dx and dy else rt.AXIS, (dx, dy): 0}
    if dx and dy:
        g[(dx, 0)] = g[(0, dy)] = FILL
    return g


def _gadget_squeeze(k, far_a, far_b, later):
    """diagonal k holds cur - 7 with side (dx, 0) FAR (far_a), side (0, dy) FAR (far_b) or both; `later`: a diagonal later in the
    order, with sides of its own, holds cur - 7 as well"""
    dx, dy = rt.ORDER[k]
    g = {(0, 0): 7, (dx, dy): 0}
    if not far_a:
        g[(dx, 0)] = FILL
    if not far_b:
        g[(0, dy)] = FILL
    if later is not None:
        lx, ly = rt.ORDER[later]
        g[(lx, ly)] = 0
        g.setdefault((lx, 0), FILL)
        g.setdefault((0, ly), FILL)
    return g


def _squeezes():
    """(name, gadget, expected next direction or None) -- a later diagonal is offered wherever one exists whose sides stay clear"""
    out = []
    for k in (NE, NW, SW, SE):
        for far_a, far_b in ((True, False), (False, True), (True, True)):
            tag = f"{NAMES[k]}-{'a' if far_a else ''}{'b' if far_b else ''}"
            out.append((f"squeeze {tag} alone", _gadget_squeeze(k, far_a, far_b, None), None))
            dx, dy = rt.ORDER[k]
            for later in range(k + 1, 8):
                lx, ly = rt.ORDER[later]
                if (far_a and lx == dx) or (far_b and ly == dy):               # it would lose a side to the same FAR cell
                    continue
                out.append((f"squeeze {tag} then {NAMES[later]}", _gadget_squeeze(k, far_a, far_b, later), later))
                break
    return out


def _gadget_sum(cur):
    """a neighbour that qualifies only if cur - step wraps: W holds cur - 5 + 65536, NE cur - 7 + 65536 between sides that are not FAR"""
    g = {(0, 0): cur, (1, 0): FILL, (0, 1): FILL}
    if cur < rt.AXIS:
        g[(-1, 0)] = cur - rt.AXIS + 65536
    if cur < rt.DIAG:
        g[(1, 1)] = cur - rt.DIAG + 65536
    return g


def _chain(n, last, more):
    """n cells running east, 5 apart, the last one costing `last`; `more`: one further cell behind them"""
    g = {(k, 0): last + rt.AXIS * (n - 1 - k) for k in range(n)}
    if more:
        assert last >= rt.AXIS
        g[(n, 0)] = last - rt.AXIS
    return g


EXIT_N = (1, 64, 65)


def _border_gadgets(W, H):
    """current cells on the four edges and four corners, cost 20.  Every neighbour off the map whose row-major index would still land
    in the field gets an admissible-looking value THERE (15 for an axis neighbour, 13 for a diagonal one); the true axis neighbours
    hold FILL.  Variant "one": the last true neighbour in the order is admissible as well."""
    spots = {"west": (0, 40), "east": (W - 1, 90), "south": (60, 0), "north": (130, H - 1), "sw": (0, 0), "se": (W - 1, 0), "nw": (0, H - 1), "ne": (W - 1, H - 1)}
    shift = {"west": (0, 25), "east": (0, 25), "south": (40, 0), "north": (40, 0)}
    cells, wrapped, starts, want = {}, {}, {}, {}
    for variant in ("none", "one"):
        for name, (x, y) in spots.items():
            if variant == "one":
                if name not in shift:
                    continue                                                   # the corners come once
                x, y = x + shift[name][0], y + shift[name][1]
            g = {(x, y): 20}
            true = []
            for k, (dx, dy) in enumerate(rt.ORDER):
                nx, ny = x + dx, y + dy
                if 0 <= nx < W and 0 <= ny < H:
                    true.append(k)
                    if not (dx and dy):
                        g[(nx, ny)] = FILL
                    continue
                idx = ny * W + nx
                if 0 <= idx < W * H:
                    wrapped[(idx % W, idx // W)] = 20 - (rt.DIAG if dx and dy else rt.AXIS)
            nxt = None
            if variant == "one":
                dx, dy = rt.ORDER[true[-1]]
                g[(x + dx, y + dy)] = 20 - rt.DIAG                             # (the last true neighbour of an edge cell is a diagonal)
                nxt = (x + dx, y + dy)
            for c, v in g.items():
                assert cells.setdefault(c, v) == v, (name, variant, c)
            starts[f"border {name} {variant}"] = (x, y)
            want[f"border {name} {variant}"] = nxt
    for c, v in wrapped.items():                                               # (where two corners meet, a gadget's own cell stays)
        cells.setdefault(c, v)
    return cells, starts, want


@functools.lru_cache(maxsize=None)
def family_a():
    field = np.full((A_H, A_W), FAR, np.uint16)
    gadgets = [(f"single {NAMES[k]}", _gadget_single(k), k) for k in range(8)]
    gadgets += [(f"subset {m:02x}", _gadget_subset(m), min(k for k in range(8) if m >> k & 1)) for m in range(1, 256)]
    gadgets += _squeezes()
    gadgets += [(f"sum {cur}", _gadget_sum(cur), None) for cur in (0, 1, 2, 3, 4, 6)]
    gadgets += [("sum fffe", {(0, 0): 0xFFFE, (1, 0): 0xFFF9}, E)]
    for n in EXIT_N:
        gadgets += [(f"exit {n} broken", _chain(n, 3, False), None), (f"exit {n} seed", _chain(n, 0, False), None), (f"exit {n} next", _chain(n, 5, True), None)]
    starts, nxt = {}, {}
    x0, y0, row_h = 4, 4, 0                                                    # shelves, one FAR cell between the bounding boxes, clear of the border
    for name, g, k in gadgets:
        xs, ys = [c[0] for c in g], [c[1] for c in g]
        w, h = max(xs) - min(xs) + 1, max(ys) - min(ys) + 1
        if x0 + w > A_W - 4:
            x0, y0, row_h = 4, y0 + row_h + 1, 0
        at = (x0 - min(xs), y0 - min(ys))
        _put(field, g, at)
        starts[name] = at
        nxt[name] = None if k is None else (at[0] + rt.ORDER[k][0], at[1] + rt.ORDER[k][1])
        x0, row_h = x0 + w + 1, max(row_h, h)
    assert y0 + row_h <= A_H - 4, (y0, row_h)
    cells, bstarts, bnext = _border_gadgets(A_W, A_H)
    _put(field, cells)
    starts.update(bstarts)
    nxt.update(bnext)
    return Case("A", A_W, A_H, field, np.full((A_H, A_W), L_FREE), starts, {"next": nxt})


@functools.lru_cache(maxsize=None)
def family_a_corners():
    """family A's map with the second variant at the corners, which a field holds once: each corner's last true neighbour -- the
    diagonal into the map -- admissible"""
    a = family_a()
    field = a.field.copy()
    starts, nxt = {}, {}
    for name in ("sw", "se", "nw", "ne"):
        x, y = a.starts[f"border {name} none"]
        dx, dy = (1 if x == 0 else -1), (1 if y == 0 else -1)
        assert field[y + dy, x + dx] == FAR
        field[y + dy, x + dx] = 20 - rt.DIAG
        starts[name] = (x, y)
        nxt[name] = (x + dx, y + dy)
    return Case("A corners", a.W, a.H, field, a.log.copy(), starts, {"next": nxt})


# ---- family B ------------------------------------------------------------------------------------------------------------------
B_W, B_H, B_N = 200, 136, 13107


def _snake(two_diagonals):
    """the chain's cells, index 0 first: rows 0, 2, 4, ... alternately east and west, joined at their ends through the odd rows; with
    two_diagonals the first joint is two diagonal steps, (199, 0) -> (198, 1) -> (197, 2), and FILL on their sides"""
    cells, sides = [], []
    for r in range(B_H // 2):
        y = 2 * r
        xs = list(range(B_W)) if r % 2 == 0 else list(range(B_W - 1, -1, -1))
        if two_diagonals and r == 1:
            xs = xs[2:]
        cells += [(x, y) for x in xs]
        if two_diagonals and r == 0:
            cells.append((B_W - 2, 1))
            sides += [(B_W - 1, 1), (B_W - 3, 1), (B_W - 2, 2)]
        else:
            cells.append((xs[-1], y + 1))
    return cells[:B_N], sides


@functools.lru_cache(maxsize=None)
def family_b(two_diagonals=False):
    chain, sides = _snake(two_diagonals)
    assert len(chain) == B_N and len(set(chain)) == B_N
    field = np.full((B_H, B_W), FAR, np.uint16)
    cost = 0
    for k in range(B_N - 1, -1, -1):                                           # the seed last in the chain
        field[chain[k][1], chain[k][0]] = cost
        if k:
            cost += rt.DIAG if chain[k][0] != chain[k - 1][0] and chain[k][1] != chain[k - 1][1] else rt.AXIS
    for x, y in sides:
        field[y, x] = FILL
    assert cost == (0xFFFE if two_diagonals else 65530)
    starts = {f"n={n}": chain[B_N - n] for n in (1, 63, 64, 65, 4096, 4097, B_N)}
    return Case("B2" if two_diagonals else "B1", B_W, B_H, field, np.full((B_H, B_W), L_FREE), starts, {"chain": chain})


B_CLEAR = ([(f"unique at {i}", {i: 100}) for i in (0, 63, 64, 127, 128, 8191, 8192, 13106)] +
           [(f"equal at {i} and {j}", {i: 100, j: 100}) for i, j in ((63, 64), (8191, 13106), (0, 13106))] +
           [("minimum 0", {8191: 0}), ("minimum fffe", {8192: 0xFFFE}), ("ffff everywhere", {})])


def clear_b(name):
    """(clearance field, min_d2, min_d2_at of the whole chain): a varying ground above the minima, 0xFFFF off the chain"""
    minima = dict(B_CLEAR)[name]
    chain = family_b().meta["chain"]
    clear = np.full((B_H, B_W), 0xFFFF, np.uint16)
    if name not in ("minimum fffe", "ffff everywhere"):
        for k, (x, y) in enumerate(chain):
            clear[y, x] = 20000 + (k * 7919) % 30011
    for k, v in minima.items():
        clear[chain[k][1], chain[k][0]] = v
    return clear, (min(minima.values()) if minima else 0xFFFF), (min(minima) if minima else 0)


# ---- family C, short segments -----------------------------------------------------------------------------------------------------
C_MAX = 8                        # (the issue asks for 6: 360 tie cells block there, 400 are asked for; 8 holds every gadget of 6 and 648 of them)
C_W, C_H = 820, 820


def l_path(dx, dy, x_first):
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    if x_first:
        return [(sx * k, 0) for k in range(abs(dx) + 1)] + [(dx, sy * k) for k in range(1, abs(dy) + 1)]
    return [(0, sy * k) for k in range(abs(dy) + 1)] + [(sx * k, dy) for k in range(1, abs(dx) + 1)]


def band_excess(dx, dy, c):
    """2 |cross| - (|dx| + |dy|) of the cell c relative to a: <= 0 inside the closed band, 0 on its edge"""
    return 2 * abs(c[0] * dy - c[1] * dx) - (abs(dx) + abs(dy))


@functools.lru_cache(maxsize=None)
def family_c():
    """per gadget (a, b, the occupied cell or None, x_first); start names are the gadgets' indices"""
    field = np.full((C_H, C_W), FAR, np.uint16)
    log = np.full((C_H, C_W), L_FREE)
    gadgets, starts = [], {}
    x0, y0, row_h = 1, 1, 0
    for dy in range(-C_MAX, C_MAX + 1):
        for dx in range(-C_MAX, C_MAX + 1):
            if not dx and not dy:
                continue
            w, h = abs(dx) + 1, abs(dy) + 1
            for x_first in (True, False):
                path = l_path(dx, dy, x_first)
                box = [(min(0, dx) + i, min(0, dy) + j) for j in range(h) for i in range(w)]
                for c in [None] + [c for c in box if c not in path]:
                    if x0 + w > C_W - 1:
                        x0, y0, row_h = 1, y0 + row_h + 1, 0
                    at = (x0 - min(0, dx), y0 - min(0, dy))
                    _put(field, {p: rt.AXIS * (len(path) - 1 - k) for k, p in enumerate(path)}, at)
                    if c is not None:
                        log[at[1] + c[1], at[0] + c[0]] = L_OCC
                    starts[len(gadgets)] = at
                    gadgets.append((at, (at[0] + dx, at[1] + dy), c, x_first))
                    x0, row_h = x0 + w + 1, max(row_h, h)
    assert y0 + row_h <= C_H - 1, (y0, row_h)
    return Case("C", C_W, C_H, field, log, starts, {"gadgets": gadgets})


# ---- family C, long segments ------------------------------------------------------------------------------------------------------
CL_W, CL_H, CL_N, CL_DY = 4100, 40, 4097, 30


def long_chain(reverse=False, mirror=False, transpose=False):
    """the monotone chain (0, 0) .. (4096, 30), its 30 diagonal steps spread evenly, as cells in the order the descent takes them"""
    chain = [(x, x * CL_DY // (CL_N - 1)) for x in range(CL_N)]
    if mirror:
        chain = [(x, CL_H - 1 - y) for x, y in chain]
    if reverse:
        chain = chain[::-1]
    if transpose:
        chain = [(y, x) for x, y in chain]
    return chain


def segment_columns(a, b, t):
    """the cells of column t (counted along the major axis from a) of the segment a -> b with their band_excess, minor offsets -1 .. an + 1"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    xmajor = abs(dx) >= abs(dy)
    out = []
    for v in range(-1, min(abs(dx), abs(dy)) + 2):
        c = (sx * t, sy * v) if xmajor else (sx * v, sy * t)
        out.append(((a[0] + c[0], a[1] + c[1]), band_excess(dx, dy, c)))
    return out


CL_DEEP, CL_RIM = 4000, 50        # of |dx| + |dy| = 4126: an excess below -4000 is deep inside the band, one within 50 of 0 at its edge
CL_WINDOW = 140                  # columns: one period of 4096 / 30 = 136.5, so a window holds every margin the segment has


def long_blockers(a, b, t, W, H, chain):
    """around major offset t, among the cells that are neither on the path nor an end point: (the nearest band cell deep inside the band, the
    nearest band cell at the band's edge, the nearest cell just outside it), each with its excess.  Within a few columns of either end the
    band of this segment holds the path's own cells alone (its first other cell is in column 69), hence a window of one period."""
    am = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
    cols = [cc for u in range(max(t - CL_WINDOW, 1), min(t + CL_WINDOW, am - 1) + 1) for cc in segment_columns(a, b, u)]
    path = set(chain)
    ok = [cc for cc in cols if 0 <= cc[0][0] < W and 0 <= cc[0][1] < H and cc[0] not in path]
    major = 0 if abs(b[0] - a[0]) == am else 1
    nearest = lambda cs: min(cs, key=lambda cc: (abs(abs(cc[0][major] - a[major]) - t), cc[1]))
    return (nearest([cc for cc in ok if cc[1] < -CL_DEEP]), nearest([cc for cc in ok if -CL_RIM < cc[1] <= 0]),
            nearest([cc for cc in ok if 0 < cc[1] < CL_RIM]))


def long_end_cells(a, b, W, H, chain):
    """in the columns next to either end, where the band is one cell wide: the cells beside the band, off the path -- they hide nothing"""
    am = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
    path = set(chain)
    out = []
    for t in (1, am - 1):
        beside = [(ex, c) for c, ex in segment_columns(a, b, t) if ex > 0 and 0 <= c[0] < W and 0 <= c[1] < H and c not in path]
        out.append(min(beside)[1])
    return out


@functools.lru_cache(maxsize=None)
def family_c_long(reverse=False, mirror=False, transpose=False, blocker=None):
    W, H = (CL_H, CL_W) if transpose else (CL_W, CL_H)
    chain = long_chain(reverse, mirror, transpose)
    field = np.full((H, W), FAR, np.uint16)
    cost = 0
    for k in range(CL_N - 1, -1, -1):
        field[chain[k][1], chain[k][0]] = cost
        if k:
            (x, y), (px, py) = chain[k], chain[k - 1]
            diag = x != px and y != py
            cost += rt.DIAG if diag else rt.AXIS
            if diag:
                field[py, x] = field[y, px] = FILL
    assert cost == 20540
    log = np.full((H, W), L_FREE)
    if blocker is not None:
        log[blocker[1], blocker[0]] = L_OCC
    return Case("C long", W, H, field, log, {0: chain[0], 1: chain[1], 2: chain[2]}, {"chain": chain})


# ---- family D ----------------------------------------------------------------------------------------------------------------------
D_W, D_H = 84, 720
D_LEGS = (65, 64, 63, 2, 1)                    # outermost first
D_EXTRA = (0, 1, 63, 64, 65, 127, 128, 129, 640)


def _corridor_case(name, W, H, corridors, occupied=(), more_starts=None):
    field = np.full((H, W), FAR, np.uint16)
    log = np.full((H, W), L_OCC)
    starts = {}
    for key, cells in corridors.items():
        _put(field, {c: rt.AXIS * (len(cells) - 1 - k) for k, c in enumerate(cells)})
        for x, y in cells:
            log[y, x] = L_FREE
        starts[key] = cells[0]
    for x, y in occupied:
        log[y, x] = L_OCC
    starts.update(more_starts or {})
    return Case(name, W, H, field, log, starts, {"corridors": corridors})


@functools.lru_cache(maxsize=None)
def family_d():
    """corridor d: d cells east of its first cell, the corner, then north to the map's last row but one; two blocked cells between
    neighbouring corridors"""
    corridors = {}
    for k, d in enumerate(D_LEGS):
        cx, y = 80 - 3 * k, 2 + 3 * k
        cells = [(cx - d + i, y) for i in range(d + 1)] + [(cx, yy) for yy in range(y + 1, D_H - 1)]
        assert len(cells) - d - 1 >= 700
        corridors[d] = cells
    return _corridor_case("D", D_W, D_H, corridors)


S_N, S_W = 700, 356


def staircase_cells():
    return [(2 + (k + 1) // 2, 2 + k // 2) for k in range(S_N)]               # E, N, E, N, ...


@functools.lru_cache(maxsize=None)
def family_d_stairs(occupied=None):
    cells = staircase_cells()
    return _corridor_case("D stairs", S_W, S_W, {0: cells}, () if occupied is None else (cells[occupied],), {"late": cells[S_N - 80]})


M_N, M_W, M_H, M_RUN = 700, 290, 8, 4


def meander_cells():
    """runs of four cells north and south by turns, one wall column between them, joined by one cell at their ends"""
    cells, x, up = [], 2, True
    while len(cells) < M_N:
        ys = range(2, 2 + M_RUN) if up else range(1 + M_RUN, 1, -1)
        cells += [(x, y) for y in ys]
        cells.append((x + 1, cells[-1][1]))
        x, up = x + 2, not up
    return cells[:M_N]


@functools.lru_cache(maxsize=None)
def family_d_meander(occupied=None):
    cells = meander_cells()
    return _corridor_case("D meander", M_W, M_H, {0: cells}, () if occupied is None else (cells[occupied],), {"late": cells[M_N - 80]})


def memo_see(cache):
    """rt.visible_box, each (a, b) of one plane computed once: requests that differ only in their limits share the look-ups"""
    def see(blocked, a, b):
        key = (id(blocked), a, b)
        if key not in cache:
            cache[key] = rt.visible_box(blocked, a, b)
        return cache[key]
    return see


MEANDER_SEEN = {}


def expect_meander(case, names, look, max_cells, max_waypoints):
    return rt.expect(case.field, case.blocked, case.cells_of(names), look, max_cells, max_waypoints, see=memo_see(MEANDER_SEEN))


# ---- family E ----------------------------------------------------------------------------------------------------------------------
OFF_MAP = [(-1, 40), (A_W, 90), (60, -1), (130, A_H), (-1, -1), (A_W, A_H), (-2 ** 31, 5), (2 ** 31 - 1, 2 ** 31 - 1)]


def launch_starts(P):
    """P starts drawn cyclically from family A's gadgets and cells off the map"""
    pool = [tuple(s) for s in family_a().starts.values()] + OFF_MAP
    return np.array([pool[(7 * p) % len(pool)] for p in range(P)], np.int64)


@functools.lru_cache(maxsize=None)
def _expect_one(case_key, start, look, max_cells, max_waypoints):
    c = {"A": family_a}[case_key]()
    return rt.expect(c.field, c.blocked, [start], look, max_cells, max_waypoints)


def expect_memo(case_key, starts, look, max_cells, max_waypoints):
    """rt.expect of many starts that repeat: the reference once per distinct start"""
    rec = np.zeros(len(starts), dtype=rt.ROUTE_DTYPE)
    ways, paths = [], []
    for p, s in enumerate(starts):
        r, w, c = _expect_one(case_key, (int(s[0]), int(s[1])), look, max_cells, max_waypoints)
        rec[p] = r[0]
        ways.append(w[0])
        paths.append(c[0])
    return rec, ways, paths
