"""The per-particle map queries share ONE rule for which particle is shown and ONE staging path for their host forms: view, cast,
clearance, reach, frontiers and trajectory refuse the same requests with the same codes, show the same particle for the same request,
host form and device form alike, and a host form's staging grows and is reused without changing a byte of the result.

Host-path facts, so the shapes are tiny: 2 filters x 4 particles on a 48 x 40 cell map (a partial 64-cell plane word, a single tile),
scans of at most 16 beams, a history of 4 updates."""
import ctypes as C

import numpy as np
import pytest

from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, _lib
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_INVALID, GMS_ERR_STATE, GMS_OK, GmsError

pytestmark = pytest.mark.gpu

QUERIES = ("view", "cast", "clearance", "reach", "frontiers", "trajectory")
GEOM = (2.4, 2.0, 0.05, (-1.2, -1.0))           # 48 x 40 cells
W, H, N_FILTERS, N_PER, HIST = 48, 40, 2, 4, 4
STRONGEST = "strongest"


def _scan(n, seed):
    """a short synthetic scan: n beams fanned around the robot, every one a hit between 0.3 and 0.8 m"""
    rng = np.random.default_rng(seed)
    a = np.linspace(-np.pi, np.pi, n, endpoint=False)
    d = rng.uniform(0.3, 0.8, n)
    b = np.zeros(n, dtype=BEAM_DTYPE)
    b["local_x"], b["local_y"], b["distance"], b["hit"] = d * np.cos(a), d * np.sin(a), d, 1
    return b


PROBES = _scan(8, 1)


def _trajectory(s, which, filter, dev=None):
    """gms_slam_trajectory[_dev] through the C ABI (the Python wrapper asks gms_slam_history_len first, which a shard refuses)"""
    L = _lib.load()
    which = _lib.GMS_VIEW_STRONGEST if which == STRONGEST else int(which)
    if dev is not None:
        out, sh = dev
        rc = L.gms_slam_trajectory_dev(s._h, which, int(filter), C.c_void_p(int(out.data_ptr())), HIST, C.c_void_p(int(sh.data_ptr())))
    else:
        xy, count, shown = np.empty((HIST, 3), np.float32), C.c_int32(0), C.c_int32(-1)
        rc = L.gms_slam_trajectory(s._h, which, int(filter), xy.ctypes.data, HIST, C.byref(count), C.byref(shown))
    if rc != GMS_OK:
        raise GmsError(rc, L.gms_last_error().decode("utf-8", "replace"))
    return None if dev is not None else int(shown.value)


def _host(s, q, which, filter=0):
    """the host form of query q; the shown index it reports"""
    if q == "view":
        return s._view(which, filter, None, 1, False, False, None, None)[1]
    if q == "cast":
        return s._cast(which, filter, PROBES, None, None)[1]
    if q == "clearance":
        return s._clearance(which, filter, None, 5, False, None, None)[1]
    if q == "reach":
        return s._reach(which, filter, None, 200, 0, True, None, None, None)[1]
    if q == "frontiers":
        return s._frontiers(which, filter, 1, 0, None, None, False, 16, None, None, None)[-1]
    return _trajectory(s, which, filter)


def _dev(s, q, which, filter=0):
    """the device form of query q; the shown index it leaves on the device"""
    import torch
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    out = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")          # (room for every query's output here)
    if q == "view":
        s._view(which, filter, None, 1, False, False, out, sh)
    elif q == "cast":
        d_probes = torch.from_numpy(PROBES.view(np.uint8).reshape(-1).copy()).to("cuda")
        s._cast(which, filter, (d_probes.data_ptr(), len(PROBES)), out, sh)
    elif q == "clearance":
        s._clearance(which, filter, None, 5, False, out, sh)
    elif q == "reach":
        s._reach(which, filter, None, 200, 0, True, None, out, sh)
    elif q == "frontiers":
        s._frontiers(which, filter, 1, 0, None, None, False, 16, out, None, sh)
    else:
        _trajectory(s, which, filter, dev=(out.view(torch.float32), sh))
    s.grid_map.synchronize(); torch.cuda.synchronize()
    got = sh.cpu().numpy()
    assert (got[1:] == -7).all(), "one int32 is written"
    return int(got[0])


def _refused(code, text, fn, *args):
    with pytest.raises(GmsError) as e:
        fn(*args)
    assert e.value.code == code and text in str(e.value), (code, text, str(e.value))


@pytest.fixture(scope="module")
def handles():
    bat = SLAMParticleMapsBatch(N_FILTERS, *GEOM, num_particles=N_PER, max_beams=16)
    shard = SLAMParticleMaps.__new__(SLAMParticleMaps)
    shard._init_shard(*GEOM, 256, 0, 512, max_beams=16)
    assert (bat.W, bat.H, shard.W, shard.H) == (W, H, W, H)
    bat.set_history(HIST)
    fresh = {}
    for q in QUERIES:                                       # (1), while nothing has updated: asked once, before the module's one update
        try:
            _host(bat, q, STRONGEST, 1)
            fresh[q] = None
        except GmsError as e:
            fresh[q] = (e.code, str(e))
    st = bat.update([_scan(16, 2), _scan(11, 3)], seeds=5)
    assert st is not None
    yield bat, shard, fresh
    bat.close(); shard.close()


@pytest.mark.parametrize("q", QUERIES)
def test_one_selection_rule(handles, q):
    bat, shard, fresh = handles
    # (1) before any update there is no strongest particle
    assert fresh[q] is not None and fresh[q][0] == GMS_ERR_STATE and "no strongest particle yet" in fresh[q][1], fresh[q]
    # (2) the strongest of a filter that does not exist; a particle that does not exist; a named particle ignores the filter
    for f in (-1, N_FILTERS):
        _refused(GMS_ERR_INVALID, "out of range", _host, bat, q, STRONGEST, f)
        _refused(GMS_ERR_INVALID, "out of range", _dev, bat, q, STRONGEST, f)
    for which in (N_FILTERS * N_PER, -3):
        _refused(GMS_ERR_INVALID, "out of range", _host, bat, q, which, 0)
    assert _host(bat, q, 5, 7) == 5 and _dev(bat, q, 5, 7) == 5
    # (3) the strongest particle of filter 1, host form and device form: filter 1's statistics, handle-wide
    want = N_PER + int(bat.strongest[1])
    assert _host(bat, q, STRONGEST, 1) == want and _dev(bat, q, STRONGEST, 1) == want
    # (4) a shard cannot know its filter's strongest particle; a named one is served -- but it keeps no history
    _refused(GMS_ERR_STATE, "shard" if q != "trajectory" else "history", _host, shard, q, STRONGEST, 0)
    if q == "trajectory":
        _refused(GMS_ERR_STATE, "history", _host, shard, q, 3, 0)
    else:
        assert _host(shard, q, 3, 0) == 3


def test_the_staging_is_reused_across_sizes(handles):
    """(5) a host form with a large output directly followed by one with a small output, and the reverse: each matches its device
    form byte for byte, whatever the staging held before"""
    import torch
    bat = handles[0]

    def host(rect):
        field, shown = bat._clearance(6, 0, rect, 5, False, None, None)
        assert shown == 6
        return field

    def same_as_device(field, rect):
        out = torch.full((field.size,), 0x5A5A, dtype=torch.int16, device="cuda")
        bat._clearance(6, 0, rect, 5, False, out, None)
        bat.grid_map.synchronize(); torch.cuda.synchronize()
        assert field.tobytes() == out.cpu().numpy().tobytes(), rect

    all_, cell = (0, 0, W, H), (17, 9, 1, 1)
    whole, one = host(all_), host(cell)
    one2, whole2 = host(cell), host(all_)
    for field, rect in ((whole, all_), (one, cell), (one2, cell), (whole2, all_)):
        same_as_device(field, rect)
    assert one.shape == (1, 1) and one[0, 0] == whole[9, 17]
