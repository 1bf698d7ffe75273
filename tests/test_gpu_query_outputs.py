"""What the Python layer accepts and refuses as a device output of a map query, over every device form: a caller's torch tensor must
be on the device, contiguous and large enough (shown_out / n_out: an int32 word on the device, contiguity not asked; device seeds:
contiguous int32 pairs; the trajectory's out: contiguous, 4-byte elements, 3 * kept of them), a refusal is a ValueError raised before
the library is entered -- nothing is written --, and a tensor of exactly the needed size receives the bytes the host form returns.
The shown particle is one rule for the eight per-particle queries, and the batch class checks filter and particle the same way on
every one of them.

Host-path facts, so the shapes are tiny (those of test_gpu_query_selection.py): a 48 x 40 cell map (a partial 64-cell plane word, a
single tile), a shared map with a filter of 8, a SLAMParticleMaps of 4, a SLAMParticleMapsBatch of 2 x 4, 8 probes, a history of 4,
one update each."""
import numpy as np
import pytest

from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps, SLAMParticleMapsBatch, _lib, beam_model_factors, locate_offsets
from gridmap_slam_robot_amd._lib import BEAM_DTYPE

pytestmark = pytest.mark.gpu

GEOM = (2.4, 2.0, 0.05, (-1.2, -1.0))           # 48 x 40 cells
W, H, N_PF, N_PER, N_FILTERS, HIST = 48, 40, 8, 4, 2, 4
RECT, RW, RH = (3, 2, 41, 35), 41, 35           # odd on every side
L_OCC, L_FREE = 0.8472978603872037, -0.4054651081081643
FILL = 0xA5
LOCATE = dict(tol=1, min_score=1, cap=5)
BEHIND, AHEAD = 3, 2
QUERIES = ("view", "cast", "clearance", "reach", "frontiers", "gain", "locate", "trajectory")


def _scan(n, seed):
    """a short synthetic scan: n beams fanned around the robot, every one a hit between 0.3 and 0.8 m"""
    rng = np.random.default_rng(seed)
    a = np.linspace(-np.pi, np.pi, n, endpoint=False)
    d = rng.uniform(0.3, 0.8, n)
    b = np.zeros(n, dtype=BEAM_DTYPE)
    b["local_x"], b["local_y"], b["distance"], b["hit"] = d * np.cos(a), d * np.sin(a), d, 1
    return b


PROBES, SCAN = _scan(8, 1), _scan(16, 2)
POSES = np.array([[0.0, 0.0, 0.3], [0.31, -0.22, 2.0], [-0.4, 0.35, -1.0]], dtype=np.float32)
SEEDS = np.array([[24, 20], [5, 5]], dtype=np.int32)


def _log():
    """12 % occupied, 10 % never observed, the rest free; the seeds' cells free"""
    u = np.random.default_rng(4840).random((H, W))
    log = np.where(u < 0.12, L_OCC, np.where(u < 0.22, 0.0, L_FREE))
    for x, y in SEEDS:
        log[y, x] = L_FREE
    return log


# ---- the tensors ------------------------------------------------------------------------------------------------------------------------
# kinds of output: "bytes" (need = bytes), "word" (shown_out, n_out), "traj" (need = float32 elements), "records" (need = one record's
# bytes: there is no minimum, the tensor's size is the cap)
def _good(kind, need):
    import torch
    if kind == "word":
        return torch.full((1,), -7, dtype=torch.int32, device="cuda")
    if kind == "traj":
        return torch.full((need,), -7.0, dtype=torch.float32, device="cuda")
    return torch.full((2 * need if kind == "records" else need,), FILL, dtype=torch.uint8, device="cuda")


def _bad(kind, need):
    """(what is wrong, the tensor to pass, the tensor to watch) of every refused form of an output of this kind"""
    import torch
    if kind == "word":
        out = [("on the host", torch.full((1,), -7, dtype=torch.int32)), ("int64", torch.full((1,), -7, dtype=torch.int64, device="cuda")),
               ("empty", torch.full((0,), -7, dtype=torch.int32, device="cuda"))]
        return [(why, t, t) for why, t in out]
    if kind == "traj":
        twice = torch.full((2 * need,), -7.0, dtype=torch.float32, device="cuda")
        short = torch.full((need - 1,), -7.0, dtype=torch.float32, device="cuda")
        return [("on the host", _good(kind, need).cpu(), None), ("one element short", short, short), ("not contiguous", twice[::2], twice)]
    size = 2 * need if kind == "records" else need
    twice = torch.full((2 * size,), FILL, dtype=torch.uint8, device="cuda")
    out = [("on the host", _good(kind, need).cpu(), None), ("not contiguous", twice[::2], twice)]
    if kind == "bytes":
        short = torch.full((need - 1,), FILL, dtype=torch.uint8, device="cuda")
        out.append(("one byte short", short, short))
    return out


def _raw(t) -> bytes:
    return t.cpu().numpy().tobytes()


class Case:
    """one device form: outs = [(argument, kind, need)]; dev(t) calls it with the tensors t[argument] (and seeds, where it takes device
    seeds); host() = {argument: what the host form returns for the same request -- bytes, the word's value, or the records --,
    "return": what the device form returns, where that is not the tensors}; sync() waits for the handle's stream"""

    def __init__(self, outs, dev, host, sync, seeds=False):
        self.outs, self.dev, self.host, self.sync, self.seeds = outs, dev, host, sync, seeds

    def tensors(self):
        return {arg: _good(kind, need) for arg, kind, need in self.outs}


def _map_cases(m, pf, d):
    n_rect, P, B = RW * RH, len(POSES), len(PROBES)
    factors = beam_model_factors(GEOM[2], BEHIND, AHEAD, 0.05)

    def sync():
        import torch
        m.synchronize(); torch.cuda.synchronize()

    def locate_host():
        rec, n = m.locate(d["off_host"], rect=RECT, full=True, **LOCATE)
        return {"out": rec.tobytes(), "n_out": n}

    def frontiers_host():
        rec, n, lab = m.frontiers(rect=RECT, labels=True)
        assert n >= 2, "the log has several frontier regions"
        return {"records": rec, "labels": lab.tobytes(), "return": n}

    def modes_host():
        rec, nf, no, lab = pf.modes(2, 8, labels=True, cap=N_PF)
        assert nf >= 1 and no == 0
        return {"records_out": rec, "labels_out": lab.tobytes(), "return": (nf, no)}

    return {
        "map.view": Case([("out", "bytes", n_rect)], lambda t: m.view(rect=RECT, out=t["out"]), lambda: {"out": m.view(rect=RECT).tobytes()}, sync),
        "map.clearance": Case([("out", "bytes", 2 * n_rect)], lambda t: m.clearance(rect=RECT, max_radius=5, out=t["out"]),
                              lambda: {"out": m.clearance(rect=RECT, max_radius=5).tobytes()}, sync),
        "map.reach": Case([("out", "bytes", 2 * n_rect)], lambda t, seeds=None: m.reach(d["seeds"] if seeds is None else seeds, max_cost=200, rect=RECT, out=t["out"]),
                          lambda: {"out": m.reach(SEEDS, max_cost=200, rect=RECT).tobytes()}, sync, seeds=True),
        "map.cast_dev": Case([("out", "bytes", 16 * P * B)], lambda t: m.cast_dev(d["poses"].data_ptr(), P, d["probes"].data_ptr(), B, t["out"]),
                             lambda: {"out": m.cast(POSES, PROBES).tobytes()}, sync),
        "map.cast_at_dev": Case([("out", "bytes", 16 * B)], lambda t: m.cast_at_dev(d["probes"].data_ptr(), B, pf, t["out"]),
                                lambda: {"out": m.cast_at(PROBES, pf).tobytes()}, sync),
        "map.gain_dev": Case([("out", "bytes", 32 * P)], lambda t: m.gain_dev(d["poses"].data_ptr(), P, d["probes"].data_ptr(), B, t["out"], 20),
                             lambda: {"out": m.gain(POSES, PROBES, 20).tobytes()}, sync),
        "map.locate_dev": Case([("out", "bytes", 16 * LOCATE["cap"]), ("n_out", "word", 1)],
                               lambda t: m.locate_dev(d["off"].data_ptr(), d["n_theta"], B, t["out"], t["n_out"], rect=RECT, **LOCATE), locate_host, sync),
        "map.frontiers_dev": Case([("records", "records", _lib.FRONTIER_DTYPE.itemsize), ("labels", "bytes", 4 * n_rect)],
                                  lambda t: m.frontiers_dev(records=t["records"], labels=t["labels"], rect=RECT), frontiers_host, sync),
        "map.clearance_poses_dev": Case([("out", "bytes", 2 * P)], lambda t: m.clearance_poses_dev(d["poses"].data_ptr(), P, t["out"], max_radius=5),
                                        lambda: {"out": m.clearance_poses(POSES, 5).tobytes()}, sync),
        "pf.modes": Case([("records_out", "records", _lib.MODE_DTYPE.itemsize), ("labels_out", "bytes", 4 * N_PF)],
                         lambda t: pf.modes(2, 8, records_out=t["records_out"], labels_out=t["labels_out"]), modes_host, sync),
        "pf.score_beams_dev": Case([("residuals_out", "bytes", 2 * N_PF * len(SCAN))],
                                   lambda t: pf.score_beams_dev(d["scan"].data_ptr(), len(SCAN), factors, BEHIND, AHEAD, residuals_out=t["residuals_out"]),
                                   lambda: {"residuals_out": pf.score_beams(SCAN, factors, BEHIND, AHEAD, residuals=True).tobytes()}, sync),
    }


def _slam_cases(s, d, **kw):
    """the per-particle queries of a SLAMParticleMaps (kw empty) or of filter kw["filter"] of a SLAMParticleMapsBatch, of the strongest
    particle"""
    n_rect, P, B, st = RW * RH, len(POSES), len(PROBES), "strongest"

    def sync():
        import torch
        s.grid_map.synchronize(); torch.cuda.synchronize()

    def pair(got):
        return {"out": got[0].tobytes(), "shown_out": got[1]}

    def locate_host():
        (rec, n), shown = s.locate(d["off_host"], st, rect=RECT, full=True, **LOCATE, **kw)
        return {"out": rec.tobytes(), "n_out": n, "shown_out": shown}

    def frontiers_host():
        rec, n, lab, shown = s.frontiers(st, rect=RECT, labels=True, **kw)
        assert n >= 1, "an update leaves a frontier"
        return {"records_out": rec, "labels_out": lab.tobytes(), "shown_out": shown, "return": n}

    shown = ("shown_out", "word", 1)
    return {
        "view": Case([("out", "bytes", n_rect), shown], lambda t: s.view(st, rect=RECT, **t, **kw), lambda: pair(s.view(st, rect=RECT, **kw)), sync),
        "cast": Case([("out", "bytes", 16 * B), shown], lambda t: s.cast((d["probes"].data_ptr(), B), st, **t, **kw), lambda: pair(s.cast(PROBES, st, **kw)), sync),
        "clearance": Case([("out", "bytes", 2 * n_rect), shown], lambda t: s.clearance(st, rect=RECT, max_radius=5, **t, **kw),
                          lambda: pair(s.clearance(st, rect=RECT, max_radius=5, **kw)), sync),
        "reach": Case([("out", "bytes", 2 * n_rect), shown], lambda t, seeds=None: s.reach(st, seeds=seeds, max_cost=200, rect=RECT, **t, **kw),
                      lambda: pair(s.reach(st, max_cost=200, rect=RECT, **kw)), sync, seeds=True),
        "frontiers": Case([("records_out", "records", _lib.FRONTIER_DTYPE.itemsize), ("labels_out", "bytes", 4 * n_rect), shown], lambda t: s.frontiers(st, rect=RECT, **t, **kw),
                          frontiers_host, sync),
        "gain": Case([("out", "bytes", 32 * P), shown], lambda t: s.gain((d["poses"].data_ptr(), P), (d["probes"].data_ptr(), B), 20, st, **t, **kw),
                     lambda: pair(s.gain(POSES, PROBES, 20, st, **kw)), sync),
        "locate": Case([("out", "bytes", 16 * LOCATE["cap"]), ("n_out", "word", 1), shown],
                       lambda t: s.locate((d["off"].data_ptr(), d["n_theta"], B), st, rect=RECT, **LOCATE, **t, **kw), locate_host, sync),
        "trajectory": Case([("out", "traj", 3 * s.history_len()[1]), shown], lambda t: s.trajectory(st, **t, **kw), lambda: pair(s.trajectory(st, **kw)), sync),
    }


@pytest.fixture(scope="module")
def world():
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    off = locate_offsets(PROBES, 4, GEOM[2])
    d = {"probes": dev(PROBES), "poses": dev(POSES), "scan": dev(SCAN), "off": dev(off), "off_host": off, "n_theta": len(off),
         "seeds": torch.from_numpy(SEEDS.copy()).to("cuda")}
    m = GridMap(*GEOM, max_beams=16)
    assert (m.W, m.H) == (W, H)
    m.upload_log(_log())
    m.compute_likelihood_map()
    m.update(SCAN, POSES[0])
    pf = ParticleFilter(m, N_PF)
    rng = np.random.default_rng(8)
    pf.set_poses(np.column_stack([rng.uniform(-0.5, 0.5, (N_PF, 2)), rng.uniform(-3.0, 3.0, N_PF)]).astype(np.float32))
    pf.score(SCAN)
    pf.normalize()
    s = SLAMParticleMaps(*GEOM, num_particles=N_PER, max_beams=16)
    bat = SLAMParticleMapsBatch(N_FILTERS, *GEOM, num_particles=N_PER, max_beams=16)
    s.set_history(HIST); bat.set_history(HIST)
    s.update(SCAN, seed=5)
    bat.update([SCAN, _scan(11, 3)], seeds=5)
    cases = _map_cases(m, pf, d)
    cases.update({"slam." + q: c for q, c in _slam_cases(s, d).items()})
    cases.update({"batch." + q: c for q, c in _slam_cases(bat, d, filter=1).items()})
    yield {"cases": cases, "slam": s, "batch": bat, "d": d}
    pf.close(); m.close(); s.close(); bat.close()


MAP_FORMS = ("map.view", "map.clearance", "map.reach", "map.cast_dev", "map.cast_at_dev", "map.gain_dev", "map.locate_dev", "map.frontiers_dev",
             "map.clearance_poses_dev", "pf.modes", "pf.score_beams_dev")
FORMS = MAP_FORMS + tuple(f"{c}.{q}" for c in ("slam", "batch") for q in QUERIES)
forms = pytest.mark.parametrize("form", FORMS)


def test_the_table_covers_every_device_form(world):
    assert set(world["cases"]) == set(FORMS)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(case, t, watch, where, **kw):
    import torch
    before = [w.cpu().clone() for w in watch]
    torch.cuda.synchronize()                                   # (the handle has a stream of its own)
    with pytest.raises(ValueError):
        case.dev(t, **kw)
        pytest.fail(f"{where}: accepted")
    case.sync()
    for w, b in zip(watch, before):
        assert torch.equal(w.cpu(), b), f"{where}: a refused call wrote to an output"


@forms
def test_a_wrong_output_tensor_is_refused_and_nothing_is_written(world, form):
    case = world["cases"][form]
    for arg, kind, need in case.outs:
        for why, bad, base in _bad(kind, need):
            t = case.tensors()
            t[arg] = bad
            watch = [v for k, v in t.items() if k != arg] + ([base] if base is not None else [bad])
            _refused(case, t, watch, f"{form}, {arg} {why}")


@pytest.mark.parametrize("form", [f for f in FORMS if f.endswith("reach")])
def test_wrong_device_seeds_are_refused(world, form):
    import torch
    case = world["cases"][form]
    assert case.seeds
    for why, seeds in (("an odd element count", torch.zeros(3, dtype=torch.int32, device="cuda")),
                       ("int64", torch.zeros((1, 2), dtype=torch.int64, device="cuda")), ("on the host", torch.zeros((1, 2), dtype=torch.int32))):
        t = case.tensors()
        _refused(case, t, list(t.values()), f"{form}, seeds {why}", seeds=seeds)


# ---- what is accepted ---------------------------------------------------------------------------------------------------------------------
@forms
def test_the_exact_size_is_accepted_and_receives_the_host_forms_bytes(world, form):
    """every output of exactly the needed size (records: exactly the regions found); shown_out and n_out as a NON-contiguous int32 view,
    which receives its word in the first element"""
    import torch
    case = world["cases"][form]
    want = case.host()
    t, words = {}, {}
    for arg, kind, need in case.outs:
        if kind == "word":
            words[arg] = torch.full((4,), -7, dtype=torch.int32, device="cuda")
            t[arg] = words[arg][::2]
            assert not t[arg].is_contiguous()
        elif kind == "records":
            t[arg] = torch.full((need * len(want[arg]),), FILL, dtype=torch.uint8, device="cuda")
        else:
            t[arg] = _good(kind, need)
    torch.cuda.synchronize()
    got = case.dev(t)
    case.sync()
    if "return" in want:
        assert got == want["return"], form
    for arg, kind, need in case.outs:
        if kind == "word":
            assert words[arg].cpu().tolist() == [want[arg], -7, -7, -7], (form, arg)
        else:
            assert _raw(t[arg]) == (want[arg].tobytes() if kind == "records" else want[arg]), (form, arg)


@pytest.mark.parametrize("form", [f for f in FORMS if f.endswith("frontiers") or f.endswith("frontiers_dev") or f == "pf.modes"])
def test_a_shorter_record_tensor_lowers_the_cap(world, form):
    """room for one record and a half: the counts are those of the host form, one record is written, the half stays"""
    import torch
    case = world["cases"][form]
    want = case.host()
    (arg, need), = [(a, n) for a, k, n in case.outs if k == "records"]
    t = case.tensors()
    t[arg] = torch.full((need + need // 2,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert case.dev(t) == want["return"], form
    case.sync()
    raw, k = t[arg].cpu().numpy(), min(1, len(want[arg]))
    assert raw[:need * k].tobytes() == want[arg][:k].tobytes() and (raw[need * k:] == FILL).all(), form


# ---- which particle, which filter -----------------------------------------------------------------------------------------------------------
def _ask(s, d, q, which, **kw):
    """the host form of query q through the public method"""
    if q == "view":
        return s.view(which, **kw)
    if q == "cast":
        return s.cast(PROBES, which, **kw)
    if q == "clearance":
        return s.clearance(which, max_radius=5, **kw)
    if q == "reach":
        return s.reach(which, max_cost=200, **kw)
    if q == "frontiers":
        return s.frontiers(which, cap=16, **kw)
    if q == "gain":
        return s.gain(POSES, PROBES, 20, which, **kw)
    if q == "locate":
        return s.locate(d["off_host"], which, **LOCATE, **kw)
    return s.trajectory(which, **kw)


@pytest.mark.parametrize("q", QUERIES)
def test_which_is_one_rule(world, q):
    d = world["d"]
    for s in (world["slam"], world["batch"]):
        with pytest.raises(ValueError):
            _ask(s, d, q, "weakest")
        if q != "cast":
            with pytest.raises(ValueError):
                _ask(s, d, q, "all")
    assert _ask(world["slam"], d, "cast", "all")[0].shape == (N_PER, len(PROBES))
    assert _ask(world["batch"], d, "cast", "all")[0].shape == (N_FILTERS * N_PER, len(PROBES))


@pytest.mark.parametrize("q", QUERIES)
def test_the_batch_checks_filter_and_particle(world, q):
    bat, d = world["batch"], world["d"]
    with pytest.raises(IndexError):
        _ask(bat, d, q, N_PER, filter=0)
    for which in (0, "strongest"):
        with pytest.raises(IndexError):
            _ask(bat, d, q, which, filter=N_FILTERS)
    assert _ask(bat, d, q, N_PER - 1, filter=1)[-1] == 2 * N_PER - 1


def test_the_batch_checks_the_filter_of_trajectories_and_calculate_combined(world):
    bat = world["batch"]
    with pytest.raises(IndexError):
        bat.trajectories(N_FILTERS)
    with pytest.raises(IndexError):
        bat.calculate_combined(N_FILTERS)
    assert bat.trajectories(1).shape == (1, N_PER, 3) and bat.calculate_combined(1).shape == (H, W)
