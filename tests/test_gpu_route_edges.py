"""Routes on the device on hand-built fields (tests/_route_cases.py; tests/test_route_inputs.py shows what each family isolates): every
comparison is array_equal on whole arrays -- records, waypoints, cells -- against tests/_route_expect.py.  The blocked plane always
comes from an uploaded logData, in the planner's mode at inflate = 0."""
import numpy as np
import pytest

import _route_cases as rc
import _route_expect as rt
from gridmap_slam_robot_amd import ROUTE_DTYPE, GridMap, SLAMParticleMaps, SLAMParticleMapsBatch
from test_gpu_route import GUARD, _arrays, _guarded, _same, _slam_route_dev

pytestmark = pytest.mark.gpu


def _new_map(case):
    m = GridMap(*case.size_m(), rc.RES, (0.0, 0.0), max_beams=360)
    assert (m.W, m.H) == (case.W, case.H)
    m.upload_log(case.log)
    return m


@pytest.fixture(scope="module")
def maps():
    """one handle per case for the tests that only read it, closed when the module is done"""
    held = {}

    def of(case):
        if case.name not in held:
            held[case.name] = _new_map(case)
        return held[case.name]
    yield of
    for m in held.values():
        m.close()


def _check(case, starts, look, max_cells, max_wp, clear=None, where="", m=None, want=None):
    """the host form with cells and without against the definition; returns the expected (records, waypoint lists, cell lists)"""
    rec, ways, paths = want or rt.expect(case.field, case.blocked, starts, look, max_cells, max_wp, clear)
    full = (rec,) + _arrays(rec, ways, paths, max_wp, max_cells)
    kw = dict(look=look, inflate=0, not_free=True, max_cells=max_cells, max_waypoints=max_wp, clear=clear)
    _same(m.route(case.field, starts, cells=True, **kw), full, f"{case.name} {where}")
    _same(m.route(case.field, starts, **kw), full, f"{case.name} {where}, the path in the handle's scratch")
    return rec, ways, paths


# ---- A ----
@pytest.mark.parametrize("look", [1, 64])
def test_a_descent_gadgets(look, maps):
    a = rc.family_a()
    names = list(a.starts)
    rec, _, paths = _check(a, a.cells_of(names), look, 128, 128, where=f"look = {look}", m=maps(a))
    nxt = a.meta["next"]
    for p, n in enumerate(names):
        if not n.startswith(("exit", "border")) and n != "sum fffe":
            assert (paths[p][1] if len(paths[p]) > 1 else None) == nxt[n], n


@pytest.mark.parametrize("n", rc.EXIT_N)
def test_a_exits_in_the_definitions_order(n, maps):
    a = rc.family_a()
    rec, _, _ = _check(a, a.cells_of([f"exit {n} {k}" for k in ("broken", "seed", "next")]), 64, n, n, where=f"max_cells = {n}", m=maps(a))
    assert rec["flags"].tolist() == [rt.BROKEN, 0, rt.CELLS_CUT]


def test_a_corners_with_one_true_neighbour(maps):
    c = rc.family_a_corners()                                                  # (family A's logData: the same handle)
    rec, _, paths = _check(c, c.cells_of(list(c.starts)), 64, 16, 16, m=maps(rc.family_a()))
    assert [p[1] for p in paths] == list(c.meta["next"].values())


# ---- B ----
B_STARTS = ["n=13107", "n=1", "n=63", "n=64", "n=65", "n=4096", "n=4097"]


@pytest.mark.parametrize("look", [1, 4096])
@pytest.mark.parametrize("max_cells", [13106, 13107, 16384])
def test_b_the_longest_descent(max_cells, look, maps):
    b = rc.family_b()
    max_wp = max_cells if look == 1 else 8
    rec, ways, paths = _check(b, b.cells_of(B_STARTS), look, max_cells, max_wp, where=f"max_cells = {max_cells}, look = {look}", m=maps(b))
    assert rec["n_cells"].tolist() == [min(13107, max_cells), 1, 63, 64, 65, 4096, 4097]
    assert rec["flags"][0] == (rt.CELLS_CUT if max_cells == 13106 else 0) and (rec["flags"][1:] == 0).all()
    if look == 1:
        assert ways == paths


def test_b_from_fffe_with_two_diagonal_steps(maps):
    b = rc.family_b(True)
    rec, _, _ = _check(b, b.cells_of(["n=13107", "n=4097"]), 4096, 16384, 8, m=maps(b))
    assert (rec["n_cells"][0], rec["start_cost"][0], rec["end_cost"][0], rec["flags"][0]) == (13107, 0xFFFE, 0, 0)


@pytest.mark.parametrize("name", [n for n, _ in rc.B_CLEAR])
def test_b_clearance_key(name, maps):
    b = rc.family_b()
    clear, d2, at = rc.clear_b(name)
    rec, _, _ = _check(b, b.cells_of(["n=13107", "n=4097", "n=65", "n=64", "n=1"]), 4096, 13107, 8, clear=clear, where=name, m=maps(b))
    assert (rec["min_d2"][0], rec["min_d2_at"][0]) == (d2, at)


# ---- C ----
def test_c_every_cell_of_the_closed_band_blocks_and_no_other(maps):
    c = rc.family_c()
    g = c.meta["gadgets"]
    rec, ways, _ = _check(c, c.cells_of(range(len(g))), 64, 32, 8, m=maps(c))
    for i, (a, b, occ, _) in enumerate(g):
        inside = occ is not None and rc.band_excess(b[0] - a[0], b[1] - a[1], occ) <= 0
        assert (ways[i] != [a, b]) == inside, (a, b, occ)


LONG = [dict(), dict(reverse=True), dict(mirror=True), dict(transpose=True), dict(reverse=True, mirror=True, transpose=True)]


@pytest.mark.parametrize("kw", LONG, ids=lambda kw: "+".join(kw) or "plain")
def test_c_a_line_of_sight_of_4096_cells(kw):
    free = rc.family_c_long(**kw)
    chain = free.meta["chain"]
    a, b = chain[0], chain[-1]
    m = _new_map(free)
    rec, ways, _ = _check(free, free.cells_of([0, 1, 2]), 4096, 4100, 4, m=m, where="free")
    assert ways[0] == [a, b] and ways[1] == [chain[1], b]
    rec, ways, _ = _check(free, free.cells_of([0]), 4095, 4100, 4, m=m, where="look = 4095")
    assert ways[0] == [a, chain[4095], b]
    for t in (1, 2048, 4095) if not kw else (2048, 4095):
        inner, edge, out = rc.long_blockers(a, b, t, free.W, free.H, chain)
        ends = [(e, False) for e in rc.long_end_cells(a, b, free.W, free.H, chain)] if t == 2048 else []
        for cell, hides in [(inner[0], True), (edge[0], True), (out[0], False)] + ends:
            case = rc.family_c_long(blocker=cell, **kw)
            m.upload_log(case.log)
            rec, ways, _ = _check(case, case.cells_of([0]), 4096, 4100, 2, m=m, where=f"occupied {cell}")
            assert (ways[0][1] != b) == hides, (t, cell)
    m.close()


# ---- D ----
@pytest.mark.parametrize("leg", rc.D_LEGS)
def test_d_the_corner_on_every_lane_of_a_pass(leg, maps):
    d = rc.family_d()
    for look in [leg + h for h in rc.D_EXTRA] + [4096]:
        rec, ways, _ = _check(d, d.cells_of([leg]), look, 1024, 16, where=f"leg {leg}, look = {look}", m=maps(d))
        assert ways[0][1] == d.meta["corridors"][leg][leg]
    _check(d, d.cells_of(rc.D_LEGS), 4096, 1024, 16, where="all corridors", m=maps(d))


def test_d_the_staircase(maps):
    s = rc.family_d_stairs()
    rec, ways, _ = _check(s, s.cells_of([0, "late"]), 4096, 1024, 700, m=maps(s))
    assert rec["n_waypoints"].tolist() == [2, 2]
    o = rc.family_d_stairs(occupied=41)
    m = _new_map(o)
    rec, ways, _ = _check(o, o.cells_of([0]), 4096, 1024, 700, m=m, where="cell 41 occupied")
    assert rec["flags"][0] == rt.MISMATCH
    rec, _, _ = _check(o, o.cells_of([0]), 4096, 1024, len(ways[0]) - 1, m=m, where="one waypoint short")
    assert rec["flags"][0] & rt.WAYPOINTS_CUT
    m.close()


def test_d_the_meander_hundreds_of_waypoints_each_after_many_passes(maps):
    m = rc.family_d_meander()
    want = rc.expect_meander(m, [0, "late"], 4096, 1024, 700)
    rec, ways, _ = _check(m, m.cells_of([0, "late"]), 4096, 1024, 700, m=maps(m), want=want)
    assert rec["n_waypoints"][0] >= 250 and (rec["flags"] == 0).all()
    short = len(ways[0]) - 1
    rec, _, _ = _check(m, m.cells_of([0]), 4096, 1024, short, m=maps(m), want=rc.expect_meander(m, [0], 4096, 1024, short), where="one waypoint short")
    assert rec["flags"][0] == rt.WAYPOINTS_CUT
    rec, _, _ = _check(m, m.cells_of([0, "late"]), 129, 1024, 700, m=maps(m), want=rc.expect_meander(m, [0, "late"], 129, 1024, 700), where="look = 129")
    assert rec["n_waypoints"][0] == len(ways[0])
    o = rc.family_d_meander(occupied=650)
    mo = _new_map(o)
    rec, _, _ = _check(o, o.cells_of(["late"]), 4096, 1024, 700, m=mo, where="cell 650 occupied")
    assert rec["flags"][0] == rt.MISMATCH
    mo.close()


# ---- E ----
@pytest.mark.parametrize("P", [4, 5, 8, 65536])
def test_e_launch_shapes(P, maps):
    a = rc.family_a()
    starts = rc.launch_starts(P)
    cap = 1 if P == 65536 else 64
    rec, _, _ = _check(a, starts, 64, cap, cap, want=rc.expect_memo("A", starts, 64, cap, cap), where=f"P = {P}", m=maps(a))
    assert P < 100 or (rec["flags"] == rt.NO_PATH).sum() > 1000


# the handle's path scratch holds P * max_cells cells and is sized in steps of 65536: (1, 16) allocates 65536, (65, 512) = 33280 fits,
# (65, 4096) = 266240 has it freed and allocated anew (262144 < 266240 <= 327680), (3, 13107) and (1, 16) then run in the larger one
SCRATCH = [(1, 16), (65, 512), (65, 4096), (3, 13107), (1, 16)]
assert SCRATCH[0][0] * SCRATCH[0][1] <= 65536 < SCRATCH[2][0] * SCRATCH[2][1] and SCRATCH[1][0] * SCRATCH[1][1] <= 65536


def _scratch_starts(P):
    return rc.family_b().cells_of((["n=13107", "n=4097", "n=65"] * 22)[:P])


def test_e_scratch_grows_twice_and_is_reused():
    b = rc.family_b()
    m = _new_map(b)
    for P, max_cells in SCRATCH:
        _check(b, _scratch_starts(P), 4096, max_cells, 8, m=m, where=f"P = {P}, max_cells = {max_cells}")
    m.close()


def test_e_scratch_through_the_device_form():
    import torch
    b = rc.family_b()
    m = _new_map(b)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to("cuda")
    d_cost = dev(b.field).view(torch.int16)
    word = np.uint32(GUARD * 0x01010101).view(np.int32)
    for P, max_cells in SCRATCH:
        starts = _scratch_starts(P)
        rec, ways, paths = rt.expect(b.field, b.blocked, starts, 4096, max_cells, 8)
        d_starts = dev(starts).view(torch.int32)
        d_rec = torch.full((32 * P + 64,), GUARD, dtype=torch.uint8, device="cuda")
        d_ways = torch.full((8 * P * 8 + 64,), GUARD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.route_dev(d_cost, d_starts, d_rec, d_ways.view(torch.int32), look=4096, inflate=0, not_free=True, max_cells=max_cells, max_waypoints=8)
        m.synchronize(); torch.cuda.synchronize()
        raw = [t.cpu().numpy() for t in (d_rec, d_ways)]
        got = (raw[0][:32 * P].view(ROUTE_DTYPE), raw[1][:64 * P].view(np.int32).reshape(P, 8, 2))
        _same(got, (rec, _arrays(rec, ways, paths, 8, max_cells, fill=word)[0], None), f"device form, P = {P}, max_cells = {max_cells}")
        assert (raw[0][32 * P:] == GUARD).all() and (raw[1][64 * P:] == GUARD).all(), "bytes past the outputs"
    m.close()


def _particle_cases():
    a, d = rc.family_a(), rc.family_d()
    return [(a, a.cells_of(list(a.starts)), 64, 128, 16), (d, d.cells_of(rc.D_LEGS), 65 + 64, 1024, 16)]


@pytest.mark.parametrize("which_case", [0, 1], ids=["A", "D"])
def test_e_a_particles_map_installed_by_hand(which_case):
    case, starts, look, max_cells, max_wp = _particle_cases()[which_case]
    n, k = 3, 1
    s = SLAMParticleMaps(*case.size_m(), rc.RES, (0.0, 0.0), num_particles=n, max_beams=64)
    assert (s.W, s.H) == (case.W, case.H)
    s.set_map(k, log=case.log)
    rec, ways, paths = rt.expect(case.field, case.blocked, starts, look, max_cells, max_wp)
    full = (rec,) + _arrays(rec, ways, paths, max_wp, max_cells)
    kw = dict(which=k, look=look, inflate=0, not_free=True)
    host = s.route(case.field, starts, max_cells=max_cells, max_waypoints=max_wp, cells=True, **kw)
    assert host[3] == k
    _same(host[:3], full, f"{case.name} in particle {k}'s map")
    got = _slam_route_dev(s, case.field, starts, max_cells, max_wp, **kw)
    _same(got[:3], _guarded(host, max_wp, max_cells), f"{case.name}, the device form")
    assert got[3] == [k, -7, -7, -7]
    s.close()


@pytest.mark.parametrize("which_case", [0, 1], ids=["A", "D"])
def test_e_a_batched_filters_map_installed_by_hand(which_case):
    case, starts, look, max_cells, max_wp = _particle_cases()[which_case]
    S, n, f, k = 2, 2, 1, 1
    bat = SLAMParticleMapsBatch(S, *case.size_m(), rc.RES, (0.0, 0.0), num_particles=n, max_beams=64)
    assert (bat.W, bat.H) == (case.W, case.H)
    bat.set_map(f, k, log=case.log)
    rec, ways, paths = rt.expect(case.field, case.blocked, starts, look, max_cells, max_wp)
    full = (rec,) + _arrays(rec, ways, paths, max_wp, max_cells)
    kw = dict(which=k, filter=f, look=look, inflate=0, not_free=True)
    host = bat.route(case.field, starts, max_cells=max_cells, max_waypoints=max_wp, cells=True, **kw)
    assert host[3] == f * n + k
    _same(host[:3], full, f"{case.name} in filter {f}, particle {k}")
    got = _slam_route_dev(bat, case.field, starts, max_cells, max_wp, **kw)
    _same(got[:3], _guarded(host, max_wp, max_cells), f"{case.name}, the device form")
    assert got[3] == [f * n + k, -7, -7, -7]
    bat.close()
