"""Global scan matching of the per-particle filter (include/gridmapslam.h "global scan matching"): gms_slam_locate[_dev] -- one scan
against the shown particle's own map -- against the brute force of tests/_locate_expect.py on that particle's downloaded logData.
Every comparison is array_equal, the filler records included.  8 particles x 120 x 120 cells, 90 beams, a few updates of the synthetic
room with a resampling in between (the maps' generation flips, so it has to be picked from the epoch counters).  Every case runs on
handles created with GMS_LOCATE_LEVELS = 0, 1, 3 and unset."""
import numpy as np
import pytest

import _locate_expect as lx
from gridmap_slam_robot_amd import LOCATE_DTYPE, SLAMParticleMaps, SLAMParticleMapsBatch, locate_offsets, synth
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_ERR_STATE, GmsError
from test_gpu_locate import LEVELS, _with_levels

pytestmark = pytest.mark.gpu

RES, B, N, EXT = 0.05, 90, 8, 6.0
ODO = (0.02, 0.1)
RECT = (30, 34, 61, 53)                                 # sides that are no multiples of 8; every particle's pose lies inside
KW = dict(rect=RECT, tol=1, min_score=20, cap=24, free_only=True)


def _same(got, want, where):
    rec, n = got
    assert rec.dtype == LOCATE_DTYPE and n == want[1], f"{where}: n_out {n} != {want[1]}"
    bad = np.flatnonzero(rec != want[0])
    assert np.array_equal(rec, want[0]), f"{where}: {len(bad)} records differ, first at {bad[:1].tolist()}: {rec[bad[:1]]} != {want[0][bad[:1]]}"


def _handle(lv, n=N):
    s = _with_levels(lv, lambda: SLAMParticleMaps(EXT, EXT, RES, (-EXT / 2, -EXT / 2), num_particles=n, max_beams=128))
    tr = synth.make_trace(EXT, RES, B, T=8, seed=23)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    return s, tr


def _offsets(tr):
    return locate_offsets(tr.scans[2], 6, RES, theta0=float(tr.poses[2][2]) - 0.3, dtheta=0.15)


@pytest.mark.parametrize("lv", LEVELS, ids=lambda v: f"levels-{v}")
def test_every_particle_the_strongest_and_an_owed_copy(lv):
    s, tr = _handle(lv)
    assert (s.W, s.H) == (120, 120)
    off = _offsets(tr)
    with pytest.raises(GmsError) as e:
        s.locate(off, **KW)
    assert e.value.code == GMS_ERR_STATE, "no strongest particle before the first update"
    (rec, n), shown = s.locate(off, which=3, full=True, **KW)
    assert shown == 3 and n == 0 and rec.tolist() == [lx.FILLER] * 24, "a fresh map has no walls"
    s.update(tr.scans[0], ODO, seed=5, sequence=0)
    s.update(tr.scans[1], ODO, seed=5, sequence=1)
    s.resample(0.37)                                                           # the copies are owed when the request comes
    got3 = s.locate(off, which=3, full=True, **KW)
    _same(got3[0], lx.expect(s.map_of(3), off, **KW), "particle 3 behind a resampling")
    s.update(tr.scans[2], ODO, seed=5, sequence=2)
    logs = [s.map_of(k) for k in range(N)]
    wants = [lx.expect(logs[k], off, **KW) for k in range(N)]
    assert all(w[2] > 0 for w in wants) and any(not np.array_equal(wants[0][0], w[0]) for w in wants[1:]), "results, and maps that differ in them"
    for k in range(N):
        got, shown = s.locate(off, which=k, full=True, **KW)
        assert shown == k
        _same(got, wants[k], f"particle {k}")
    got, shown = s.locate(off, full=True, **KW)
    assert shown == s.view("strongest")[1] == s.last_stats["strongest"]
    _same(got, wants[shown], "strongest")
    for mode_kw in (dict(not_free=True, tol=0, free_only=True), dict(not_free=False, tol=0, free_only=False), dict(not_free=True, tol=3, free_only=False)):
        kw = dict(KW, **mode_kw)
        _same(s.locate(off, which=5, full=True, **kw)[0], lx.expect(logs[5], off, **kw), f"particle 5, {mode_kw}")
    assert s.grid_map.locate_stats()["levels"] == (3 if lv is None else int(lv)), "2^(3 + 2) <= 61 < 2^(4 + 2)"
    for bad in (-2, N):
        with pytest.raises(GmsError) as e:
            s.locate(off, which=bad, **KW)
        assert e.value.code == GMS_ERR_INVALID
    with pytest.raises(GmsError) as e:
        s.locate(off, which=0, **dict(KW, rect=(60, 60, 61, 53)))
    assert e.value.code == GMS_ERR_INVALID, "a rectangle off the map"
    again = [s.map_of(k) for k in range(N)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(logs, again)), "a request changes no map"
    s.reset()
    with pytest.raises(GmsError) as e:
        s.locate(off, **KW)
    assert e.value.code == GMS_ERR_STATE, "... and none after a reset"
    s.close()


@pytest.mark.parametrize("lv", (None, "0"), ids=lambda v: f"levels-{v}")
def test_batched_handle_and_the_device_form(lv):
    import torch
    S, n = 3, 4
    tr = synth.make_trace(EXT, RES, B, T=12, seed=23)
    bat = _with_levels(lv, lambda: SLAMParticleMapsBatch(S, EXT, EXT, RES, (-EXT / 2, -EXT / 2), num_particles=n, max_beams=128))
    bat.set_poses(np.stack([np.tile(tr.poses[3 * f], (n, 1)) for f in range(S)]))
    off = locate_offsets(tr.scans[5], 6, RES, theta0=float(tr.poses[5][2]) - 0.3, dtheta=0.15)
    kw = dict(KW, rect=None, cap=20)
    with pytest.raises(GmsError) as e:
        bat.locate(off, filter=1, **kw)
    assert e.value.code == GMS_ERR_STATE
    for k in range(3):
        bat.update([tr.scans[3 * f + k] for f in range(S)], [ODO] * S, seeds=[11, 12, 13], sequence=k)
        if k == 1:
            bat.resample([0.37, 0.52, 0.81])
    got, shown = bat.locate(off, filter=1, full=True, **kw)
    assert shown == bat.view("strongest", filter=1)[1] and n <= shown < 2 * n, "a slot of filter 1"
    want1 = lx.expect(bat.map_of(1, shown - n), off, **kw)
    assert want1[2] > 0
    _same(got, want1, "filter 1, strongest")
    for f, k in ((0, 3), (2, 1)):
        got, sh = bat.locate(off, which=k, filter=f, full=True, **kw)
        assert sh == f * n + k
        _same(got, lx.expect(bat.map_of(f, k), off, **kw), f"filter {f}, particle {k}")
    with pytest.raises(IndexError):
        bat.locate(off, filter=S, **kw)
    # the device form: records, their number, the shown slot, nothing past any of them
    d_off = torch.from_numpy(off.reshape(-1).copy()).to("cuda")
    out = torch.full((16 * 20 + 48,), 0xA5, dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    sh = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(GmsError) as e:
        bat.locate((d_off.data_ptr(), 6, B), filter=1, out=out[8:], n_out=n_out, shown_out=sh, **kw)
    assert e.value.code == GMS_ERR_INVALID
    bat.locate((d_off.data_ptr(), 6, B), filter=1, out=out, n_out=n_out, shown_out=sh, **kw)
    bat.grid_map.synchronize(); torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.array_equal(raw[:16 * 20].view(LOCATE_DTYPE), want1[0]), "the device form"
    assert (raw[16 * 20:] == 0xA5).all() and n_out.cpu().tolist() == [want1[1], -7, -7, -7] and sh.cpu().tolist() == [shown, -7, -7, -7]
    bat.close()
