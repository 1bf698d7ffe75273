"""GridMap.findBestPose for a filter on a SHARED map (J/slam/GridMap.java:319-346; gms_pf_refine_poses / gms_pf_set_refine ->
k_compact_beams + k_refine: 1210 lattice poses per particle, one lane per pose, a butterfly argmax and a four-wave merge) against
the oracle's literal loop (orc_find_best_pose), at the places where the kernel can be wrong: equal products in different lanes
and waves (the first maximum wins), products that are all 0 (the start pose is kept), batched handles, scans without a hit or
without a beam, more than 2048 hit beams (the kernel's beam table is dynamic LDS above 32 KB), quotients on cell boundaries (the
exact division behind beam_cell_fast's guard), lattices outside the map or across its edge, ragged / 2 cm / non-square maps, the
fused step's field after a deferred map update, and the weights scored at the refined poses.

In every test the refined pose of EVERY particle equals the oracle's argmax, the oracle has evaluated 1210 poses, and -- where the
field is not blank -- some pose has moved.  The lattice is q = 110 ix + 10 iy + it (theta fastest, GridMap.java:328-330): poses that
differ only in ix sit 110 slots apart, poses that differ only in iy 10 slots apart; lane = q mod 256, wave = lane / 64."""
import numpy as np
import pytest

from gridmap_slam_robot_amd import GridMap, ParticleFilter, synth
from oracle import oracle as orc

from test_gpu_parity import REL, TIGHT, rel_err

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the lattice, as the reference walks it
def _lattice_steps():
    """the float loop counters of GridMap.java:324-330: 11 x 11 x 10 offsets"""
    f = np.float32
    x_span = y_span = f(0.20)
    theta_span = f(15 * (np.pi / 180.0))
    trans_step, theta_step = f(0.04), f(theta_span / f(5))

    def run(span, step):
        out, d = [], f(-span)
        while d < span:
            out.append(d)
            d = f(d + step)
        return np.array(out, dtype=np.float32)
    return run(x_span, trans_step), run(y_span, trans_step), run(theta_span, theta_step)


S_DX, S_DY, S_DT = _lattice_steps()
assert (S_DX.size, S_DY.size, S_DT.size) == (11, 11, 10)


def _lattice(start):
    """[1210][3] float32: start + offset in the reference's loop order (:328-332)"""
    s = np.asarray(start, dtype=np.float32)
    out = np.empty((11, 11, 10, 3), dtype=np.float32)
    out[..., 0] = (s[0] + S_DX)[:, None, None]
    out[..., 1] = (s[1] + S_DY)[None, :, None]
    out[..., 2] = (s[2] + S_DT)[None, None, :]
    return out.reshape(-1, 3)


def _first_pose(P):
    P = np.asarray(P, dtype=np.float32)
    return P + np.array([S_DX[0], S_DY[0], S_DT[0]], dtype=np.float32)


def _oracle_refine(g, lik, z, P):
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    best = np.empty_like(P)
    for i in range(len(P)):
        best[i], _, n_eval = g.find_best_pose(lik, z, P[i])
        assert n_eval == 1210
    return best


def _assert_refined(got, want, label=""):
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=-1) if got.shape == want.shape else None
    assert np.array_equal(got, want), f"{label}: {int(bad.sum())} of {bad.size} refined poses differ from the oracle's argmax, first at {np.argwhere(bad)[0]}"


def _ring_scan(B, r_lo, r_hi, seed, hit=1):
    """B beams at evenly spread bearings with ranges in [r_lo, r_hi)"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * (np.arange(B) + rng.random(B)) / max(B, 1)
    r = rng.uniform(r_lo, r_hi, B)
    return orc.make_beams(r * np.cos(a), r * np.sin(a), r, np.full(B, hit))


def _scanned_map(W, H, res, B, seed, n_scans=4, **kw):
    """(trace, oracle grid, device map, oracle field): n_scans of the synthetic drive in both; the device's field EQUALS the oracle's"""
    tr = synth.make_trace(min(W, H), res, B, T=16, seed=seed, n_scans=n_scans + 3)
    g = orc.Grid(W, H, res, -W / 2, -H / 2)
    m = GridMap(W, H, res, (-W / 2, -H / 2), **kw)
    assert (m.W, m.H) == (g.W, g.H)
    log = g.new_log()
    for t in range(n_scans):
        m.update(tr.scans[t], tr.poses[t])
        g.integrate(log, tr.scans[t], tr.poses[t])
    lik = g.build_likelihood(log)
    assert np.array_equal(m.download_likelihood().reshape(-1), lik)
    return tr, g, m, lik, log


def _uploaded_map(W, H, res, log2d, pos=None, **kw):
    pos = (-W / 2, -H / 2) if pos is None else pos
    g = orc.Grid(W, H, res, pos[0], pos[1])
    m = GridMap(W, H, res, pos, **kw)
    assert (m.W, m.H) == (g.W, g.H)
    log = np.ascontiguousarray(log2d(g.H, g.W), dtype=np.float64).reshape(-1)
    m.upload_log(log)
    m.compute_likelihood_map()
    lik = g.build_likelihood(log)
    assert np.array_equal(m.download_likelihood().reshape(-1), lik)
    return g, m, lik


def _compare_weights(pf, g, lik, z, best, label):
    """score + normalise at the refined poses against Grid.score at the ORACLE's refined poses: tolerance and underflow mask of
    test_gpu_parity.py::test_score_normalize_neff_pose"""
    pf.score(z)
    w = pf.get_weights()
    want = g.score(lik, z, best)
    ok = want > 1e-290
    assert rel_err(w[ok], want[ok]) <= TIGHT < REL, label
    assert np.all(w[~ok] <= 1e-280), label
    assert np.max(np.abs(pf.get_log_weights() - g.score_log(lik, z, best))) <= 1e-9, label
    st = pf.normalize()
    wn = want.copy()
    ws, strongest = orc.normalize(wn)
    assert st["strongest"] == strongest, label
    assert abs(st["weight_sum"] - ws) <= TIGHT * ws, label
    assert rel_err(pf.get_weights()[ok], wn[ok]) <= TIGHT < REL, label
    return int(ok.sum())


# ------------------------------------------------------------------ 1. shapes, poses and weights
@pytest.mark.parametrize("W,H,res,B,N", [(3.2, 3.2, 0.05, 90, 300), (10.24, 10.24, 0.02, 720, 65), (3.3, 3.3, 0.07, 60, 1),
                                         (4.13, 2.55, 0.05, 64, 63)])
def test_refined_poses_and_their_weights(W, H, res, B, N):
    """64 x 64 cells with more particles than a launch has lanes; a 2 cm map of 512 x 512 with 720 beams and a particle count that is
    no multiple of anything; a grid of 48 x 48 cells of 7 cm with ONE particle; a ragged non-square map (83 x 51).  Four scans
    are integrated first; every particle is a perturbed pose (none is the trace's own).  Then the weights scored from the trig
    cache that k_refine rewrites."""
    tr, g, m, lik, _ = _scanned_map(W, H, res, B, seed=31)
    z = tr.scans[4]
    P = synth.make_particles(tr.poses[4], N + 1, seed=7, sigma_xy=0.05, sigma_theta_deg=3.0)[1:]
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    best = _oracle_refine(g, lik, z, P)
    _assert_refined(got, best, f"{g.W}x{g.H}")
    assert (got != P).any()
    n_ok = _compare_weights(pf, g, lik, z, best, f"{g.W}x{g.H}")
    assert n_ok > 0, "every weight lies under the mask: the comparison would be empty"


# ------------------------------------------------------------------ 2. batched handle
def test_batched_handle_refines_every_map_against_its_own_field_and_scan():
    """three maps with three histories in one handle, one call: map 0's scan has a hit in every beam, map 1's in two of three, map
    2's in none -- nhit[mi], the hit-beam rows at stride max_beams (2048) with B = 120, fac + mi * fac_stride, gi = mi * n + p.  An
    earlier call with full scans has left other beams in every row, so a count read from the wrong map multiplies stale beams."""
    M, B, N = 3, 120, 40
    ext, res = 6.4, 0.05
    traces = [synth.make_trace(ext, res, B, T=8, seed=40 + i) for i in range(M)]
    mb = GridMap(ext, ext, res, (-ext / 2, -ext / 2), n_maps=M)
    g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
    logs = [g.new_log() for _ in range(M)]
    for t in range(4):
        mb.update(np.stack([tr.scans[t] for tr in traces]), np.stack([tr.poses[t] for tr in traces]))
        for i in range(M):
            g.integrate(logs[i], traces[i].scans[t], traces[i].poses[t])
    liks = [g.build_likelihood(l) for l in logs]
    kb = mb.download_likelihood()
    for i in range(M):
        assert np.array_equal(kb[i].reshape(-1), liks[i])
    pfb = ParticleFilter(mb, N)
    P = np.stack([synth.make_particles(traces[i].poses[4], N + 1, seed=i, sigma_xy=0.05, sigma_theta_deg=3.0)[1:] for i in range(M)])
    pfb.set_poses(P)
    pfb.refine_poses(np.stack([tr.scans[5] for tr in traces]))         # (leaves 120 other beams in every map's row)
    zs = []
    for i in range(M):
        s = traces[i].scans[4]
        z = np.resize(s[s["hit"] != 0], B).copy()                      # every beam a hit
        if i == 1:
            z["hit"][::3] = 0
        if i == 2:
            z["hit"] = 0
        zs.append(z)
    nhit = [int((z["hit"] != 0).sum()) for z in zs]
    assert nhit[0] == B > nhit[1] > 0 == nhit[2]
    pfb.set_poses(P)
    pfb.refine_poses(np.stack(zs))
    got = pfb.get_poses()
    for i in range(M):
        _assert_refined(got[i], _oracle_refine(g, liks[i], zs[i], P[i]), f"map {i}")
    assert (got[0] != P[0]).any() and (got[1] != P[1]).any()
    assert np.array_equal(got[2], _first_pose(P[2]))


# ------------------------------------------------------------------ 3. the argmax rule
def _central_particles(N, seed, spread=0.25):
    rng = np.random.default_rng(seed)
    P = np.empty((N, 3), dtype=np.float32)
    P[:, :2] = rng.uniform(-spread, spread, (N, 2))
    P[:, 2] = rng.uniform(-np.pi, np.pi, N)
    return P


def test_all_products_equal_the_first_lattice_pose_wins():
    """(a) a blank 128 x 128 map and 64 hits that end at least 1 m inside it from every lattice pose: 1210 equal products in every
    lane of every wave, and the pose is start + (s_dx[0], s_dy[0], s_dt[0]) in the reference's float arithmetic."""
    g, m, lik = _uploaded_map(6.4, 6.4, 0.05, lambda H, W: np.zeros((H, W)))
    z = _ring_scan(64, 0.5, 1.7, seed=1)
    N = 33
    P = _central_particles(N, seed=2)
    for i in (0, N - 1):                                               # the condition on the inputs, on the CPU
        prods = g.score(lik, z, _lattice(P[i]))
        assert prods[0] > 0 and (prods == prods[0]).all()
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), "blank map")
    assert np.array_equal(got, _first_pose(P))


def _band_log(n, seed):
    """n values: bands of 3 cells, each occupied, free or unknown"""
    rng = np.random.default_rng(seed)
    return np.repeat(rng.choice([-2.0, 0.0, 2.0], size=(n + 2) // 3), 3)[:n]


@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_ties_between_lanes_and_waves_go_to_the_smaller_slot(axis):
    """(b) log-odds that depend on the row only: the field's interior columns are equal bit for bit, a beam's row does not depend on
    the pose's x, so lattice poses that differ only in ix -- 110 slots apart: other lanes, other waves -- have bit-equal products (asserted
    on the CPU with the oracle first), and the chosen ix must be 0.  (c) columns only: ties 10 slots apart, iy must be 0.  Particles
    within 0.25 m of the centre of a 6.4 m map, ranges under 1.7 m: no end point comes near the edge, where the blur is clipped."""
    bands = _band_log(128, seed=5)
    g, m, lik = _uploaded_map(6.4, 6.4, 0.05, (lambda H, W: np.tile(bands[:, None], (1, W))) if axis == "rows"
                              else (lambda H, W: np.tile(bands[None, :], (H, 1))))
    z = _ring_scan(48, 0.5, 1.7, seed=3)
    N = 24
    P = _central_particles(N, seed=4)
    for i in range(N):
        prods = g.score(lik, z, _lattice(P[i])).reshape(11, 11, 10)
        tied = prods == (prods[:1] if axis == "rows" else prods[:, :1])
        assert tied.all(), "the inputs must tie along the axis"
        assert np.unique(prods).size > 1
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), axis)
    k = 0 if axis == "rows" else 1
    assert np.array_equal(got[:, k], _first_pose(P)[:, k])
    assert (got != P).any() and not np.array_equal(got, _first_pose(P))


def test_all_products_zero_keep_the_start_pose():
    """(d) as many hits on a blank 12.8 m map as it takes for every lattice product to be exactly 0 (the count is found with the
    oracle: the first multiple of 100 at which all 1210 products of every particle are 0): maxProb stays 0, the start pose is kept
    bit for bit (GridMap.java:320-321, 334), and the weights are 0 / 0 on both sides."""
    g, m, lik = _uploaded_map(12.8, 12.8, 0.05, lambda H, W: np.zeros((H, W)))
    N = 5
    P = _central_particles(N, seed=6)
    for B in range(100, 2001, 100):
        z = _ring_scan(B, 0.5, 3.0, seed=8)
        if all((g.score(lik, z, _lattice(P[i])) == 0).all() for i in range(N)):
            break
    else:
        pytest.fail("no beam count up to 2000 brings every product to 0")
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), f"{B} beams")
    assert np.array_equal(got.view(np.uint32), P.view(np.uint32))
    pf.score(z)
    pf.normalize()
    want = g.score(lik, z, P)
    orc.normalize(want)
    assert np.isnan(want).all() and np.isnan(pf.get_weights()).all()


def test_a_scan_without_a_beam():
    """(e) B = 0: every product is the empty product 1, the first lattice pose wins."""
    tr, g, m, lik, _ = _scanned_map(3.2, 3.2, 0.05, 90, seed=31)
    N = 7
    P = synth.make_particles(tr.poses[4], N, seed=1, sigma_xy=0.05, sigma_theta_deg=3.0)
    z = tr.scans[4][:0].copy()
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), "B = 0")
    assert np.array_equal(got, _first_pose(P))


# ------------------------------------------------------------------ 4. edges
def test_lattices_outside_the_map_across_its_edge_and_in_its_corner():
    """particles far outside the map on every side (every beam is skipped, :276: the first pose wins), particles whose lattice lies
    across an edge, and particles in the four corner cells: negative and saturating cell indices, the neutral border of the factor
    table."""
    W = 3.2
    tr, g, m, lik, _ = _scanned_map(W, W, 0.05, 90, seed=31)
    z = tr.scans[4]
    h = W / 2
    far = [[30.0, 2.0, 0.4], [-500.0, -500.0, 0.0], [1e5, 1e5, 2.0], [0.3, -40.0, -1.0], [-3e9, 3e9, 0.1]]
    edge = [[-h - 0.1, 0.0, 0.0], [h + 0.05, 0.3, 1.0], [0.2, h - 0.1, 2.0], [-0.4, -h + 0.19, -2.0], [h, h, 0.5], [-h, -h, 0.5]]
    corner = [[-h + 0.01, -h + 0.01, 0.3], [h - 0.01, -h + 0.01, 1.3], [-h + 0.01, h - 0.01, -0.3], [h - 0.01, h - 0.01, 3.0]]
    inside = synth.make_particles(tr.poses[4], 4, seed=2, sigma_xy=0.05, sigma_theta_deg=3.0)[1:].tolist()
    P = np.array(far + edge + corner + inside, dtype=np.float32)
    pf = ParticleFilter(m, len(P))
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), "edges")
    assert np.array_equal(got[: len(far)], _first_pose(P[: len(far)]))
    assert (got != P).any() and not np.array_equal(got[len(far):], _first_pose(P[len(far):]))


# ------------------------------------------------------------------ 5. the exact division behind the guard
def _kernel_quotients(g, L, lx, ly):
    """k_refine's own expressions for lattice poses L [n][3] and beams: the fast quotients q = d * RN(1 / res) in x and y, and the
    reference's d / res (j_cell_fast / j_cell_exact), each [n][B], in float64 without contraction"""
    res, posx, posy = float(g.resolution), float(g.pos[0]), float(g.pos[1])
    rinv = 1.0 / res
    ct = L[:, 2].astype(np.float64)
    c = np.cos(ct).astype(np.float32).astype(np.float64)[:, None]
    s = np.sin(ct).astype(np.float32).astype(np.float64)[:, None]
    px, py = L[:, 0].astype(np.float64)[:, None], L[:, 1].astype(np.float64)[:, None]
    dx, dy = (lx * c - ly * s + px) - posx, (lx * s + ly * c + py) - posy
    return dx * rinv, dy * rinv, dx / res, dy / res


def _under_a_cell_boundary(g, v, p0, rng):
    """a local coordinate l for which d = (l + v) - p0 lies one step under a cell boundary n * res, where (int)(d / res) and
    (int)(d * RN(1 / res)) are different cells"""
    res = float(g.resolution)
    rinv = 1.0 / res
    for n in rng.permutation(np.arange(40, 110)):
        d = np.nextafter(n * res, 0.0)
        l = d + p0 - v
        if np.trunc(d / res) != np.trunc(d * rinv) and (l * 1.0 - 0.0 + v) - p0 == d:
            return l
    raise AssertionError("no such coordinate")


def test_quotients_on_cell_boundaries_take_the_exact_division():
    """a 2 cm map of 128 x 128 cells whose origin is 32 cells from 0; 32 start poses on cell corners (x0, y0 = k * res in float,
    k in 8, 16, 24, 32) whose heading is minus a lattice offset, so that one heading of every lattice is exactly 0 (c = 1, s = 0);
    the beam (0, 0), 32 beams on the axes at multiples of 4 res, and 26 beams that end one float64 step under a cell boundary as
    seen from one of the 26 lattice abscissae / ordinates at heading 0 -- there (int)(d * RN(1 / res)) is the cell beyond the
    reference's (int)(d / res).  Counted here in float64 with the kernel's own expression, before the device runs:
    263116 (lattice pose, beam) pairs with |q - rint(q)| <= 2^-19 (required: 1000), 24714 pairs whose fast quotient names another
    cell than the exact one (required: 1000), and 3 particles for which the first maximum over products taken at the fast
    quotients' cells is another lattice pose (required: 3).  The field is salt and pepper: a neighbouring cell has another factor."""
    res32 = np.float32(0.02)
    rng = np.random.default_rng(3)
    g, m, lik = _uploaded_map(2.56, 2.56, 0.02, lambda H, W: np.random.default_rng(14).choice([-2.0, 0.0, 2.0], size=(H, W)),
                              pos=(-0.64, -0.64))
    posx, posy = float(g.pos[0]), float(g.pos[1])
    X0 = [np.float32(np.float32(k) * res32) for k in (8, 16, 24, 32)]
    P = np.array([[x, y, -S_DT[it]] for x in X0 for y in X0 for it in (5, 2)], dtype=np.float32)
    coords = sorted({float(np.float32(x + d)) for x in X0 for d in S_DX})          # (S_DX == S_DY)
    lx = np.array([_under_a_cell_boundary(g, v, posx, rng) for v in coords])
    ly = np.array([_under_a_cell_boundary(g, v, posy, rng) for v in coords])
    rng.shuffle(ly)
    ax = np.arange(1, 9) * 4 * float(g.resolution)
    o = np.zeros_like(ax)
    LX, LY = np.concatenate([[0.0], ax, -ax, o, o, lx]), np.concatenate([[0.0], o, o, ax, -ax, ly])
    z = orc.make_beams(LX, LY, np.hypot(LX, LY), np.ones(LX.size))
    fac = np.where(lik == 0.5, 1.0 / g.g.max_range, g.g.z_hit * lik + g.g.z_random * 1.0 / g.g.max_range)      # GridMap.java:285-288

    def first_maximum(qx, qy):
        gx, gy = np.trunc(qx).astype(np.int64), np.trunc(qy).astype(np.int64)
        inside = (gx >= 0) & (gy >= 0) & (gx < g.W) & (gy < g.H)
        f = np.where(inside, fac[np.clip(gy, 0, g.H - 1) * g.W + np.clip(gx, 0, g.W - 1)], 1.0)
        prod = np.ones(len(f))
        for j in range(f.shape[1]):
            prod = prod * f[:, j]
        return int(np.argmax(prod))
    tripped = other_cell = other_pose = 0
    for p in P:
        qx, qy, ex, ey = _kernel_quotients(g, _lattice(p), LX, LY)
        tripped += int(((np.abs(qx - np.rint(qx)) <= 2.0 ** -19) | (np.abs(qy - np.rint(qy)) <= 2.0 ** -19)).sum())
        other_cell += int(((np.trunc(qx) != np.trunc(ex)) | (np.trunc(qy) != np.trunc(ey))).sum())
        other_pose += int(first_maximum(qx, qy) != first_maximum(ex, ey))
    print(f"guard pairs {tripped}, pairs whose fast quotient names another cell {other_cell}, particles whose argmax depends on it {other_pose}")
    assert tripped >= 1000 and other_cell >= 1000 and other_pose >= 3
    pf = ParticleFilter(m, len(P))
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), "cell boundaries")
    assert (got != P).any()


# ------------------------------------------------------------------ 6. long scans
@pytest.mark.parametrize("field,B", [("mostly_occupied", 2049), ("mostly_occupied", 4096), ("blank", 4096)])
def test_more_hit_beams_than_the_static_beam_table_holds(field, B):
    """GMS_MAX_BEAMS = 4096 allows it: above 2048 hit beams the beam table is dynamic LDS beyond 32 KB (64 KB at 4096).  On a
    scanned map 2049 factors underflow at every pose, so the field is one that is occupied except for one cell in twelve, where the
    products of 2049 and of 4096 factors stay positive (asserted) and differ from pose to pose; and 4096 hits on a blank map,
    where every product is 0 and the start pose is kept."""
    rng = np.random.default_rng(12)
    g, m, lik = _uploaded_map(6.4, 6.4, 0.05, (lambda H, W: np.zeros((H, W))) if field == "blank"
                              else (lambda H, W: np.where(rng.random((H, W)) < 1 / 12, -2.0, 2.0)), max_beams=4096)
    z = _ring_scan(B, 0.3, 2.4, seed=13)
    N = 4
    P = _central_particles(N, seed=14)
    prods = g.score(lik, z, _lattice(P[0]))
    if field == "blank":
        assert (prods == 0).all()
    else:
        assert (prods > 0).all() and np.unique(prods).size > 1000
    pf = ParticleFilter(m, N)
    pf.set_poses(P)
    pf.refine_poses(z)
    got = pf.get_poses()
    _assert_refined(got, _oracle_refine(g, lik, z, P), f"{field} {B}")
    if field == "blank":
        assert np.array_equal(got.view(np.uint32), P.view(np.uint32))
    else:
        assert (got != P).any()


# ------------------------------------------------------------------ 7. the fused step, three times
def test_three_fused_steps_with_refinement_see_the_field_of_the_step_before():
    """slam_update(..., fraction = -1, integrate = True) with set_refine(True), default deferred apply pass and lazy likelihood,
    nothing read back between the steps: the refinement of step k + 1 reads the factor table after step k's map update.  The oracle
    loop per step: findBestPose on the field of its own log, score, normalise, integrate at the weighted pose."""
    W, res, B, N = 6.4, 0.05, 120, 96
    tr, g, m, lik, log = _scanned_map(W, W, res, B, seed=52, n_scans=2)
    pf = ParticleFilter(m, N)
    pf.set_refine(True)
    steps = (2, 3, 4)
    Ps = [synth.make_particles(tr.poses[t], N + 1, seed=20 + t, sigma_xy=0.05, sigma_theta_deg=3.0)[1:] for t in steps]
    for t, P in zip(steps, Ps):
        pf.slam_update(P, tr.scans[t], 0.5, -1.0, True)
    for t, P in zip(steps, Ps):
        lik = g.build_likelihood(log)
        best = _oracle_refine(g, lik, tr.scans[t], P)
        assert (best != P).any()
        want = g.score(lik, tr.scans[t], best)
        wn = want.copy()
        ws, strongest = orc.normalize(wn)
        wp = orc.weighted_pose(best, wn)
        g.integrate(log, tr.scans[t], wp)
    _assert_refined(pf.get_poses(), best, "third step")
    ok = wn > 1e-290
    w = pf.get_weights()
    assert ok.any() and rel_err(w[ok], wn[ok]) <= TIGHT < REL
    assert np.all(w[~ok] <= 1e-280)
    st = pf.stats()
    assert st["strongest"] == strongest and abs(st["weight_sum"] - ws) <= TIGHT * ws
    assert np.array_equal(pf.last_step()["weighted_pose"], wp), "the map updates ran at another pose than the oracle's: pick another seed"
    assert np.array_equal(m.download_likelihood().reshape(-1), g.build_likelihood(log))
    got_log = m.download_log().reshape(-1)
    assert np.array_equal(got_log != 0, log != 0) and np.max(np.abs(got_log - log)) <= 1e-10
