"""Map warps out of a batched per-particle handle and out of a shard (include/gridmapslam.h "map warps"): the slot
`filter * n + strongest` and the generation `epoch[2 * (slot / n)]` that k_warp picks on the device.  Three filters of 8 particles
on 120 x 120 cells, driven as tests/test_gpu_slam_batch.py drives them beside three stand-alone handles, until ONE resample_if has
drawn in some filters and not in others: the filters then sit on different generations, and a wrong stride or counter reads another
filter's maps or the stale generation of the right one.  Every comparison is array_equal on bits against the restatement
(tests/_warp_expect.py) on the downloaded map of the particle, and against what the stand-alone handle gives."""
import numpy as np
import pytest

import _warp_cases as wc
import _warp_expect as wx
from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, SLAMParticleMapsBatch, synth
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_BLOCK, GMS_ERR_INVALID, GMS_ERR_STATE, GmsError, load, ptr

from test_gpu_slam_batch import _compare, _odometry, _scans

pytestmark = pytest.mark.gpu

EXT, RES, S, N = 6.0, 0.05, 3, 8
BEAMS = (72, 40, 65)
SEEDS = np.array([11, 12345, 7], dtype=np.uint64)
T = 8
NAMED = ((1, 6), (0, 7), (3, 5))                            # two filter-local particles per filter
OPS = ("replace", "add", "fill", "compare")
CLAMP = 1.5


def _destination(n_maps=1):
    d = GridMap(wc.metres(wc.W_D, wc.RES_D), wc.metres(wc.H_D, wc.RES_D), wc.RES_D, wc.POS_D, n_maps=n_maps)
    assert (d.W, d.H) == (wc.W_D, wc.H_D)
    return d


def _state(h):
    poses, weights = h.get_particles()
    return wx.bits(poses.astype(np.float64)), wx.bits(weights), wx.bits(h.maps())


def _refused(code, call, *args, **kw):
    with pytest.raises(GmsError) as e:
        call(*args, **kw)
    assert e.value.code == code


@pytest.mark.parametrize("form", ["planes", "eager"])
def test_every_filter_of_a_batch_on_its_own_generation(form, monkeypatch):
    import torch
    if form == "eager":
        monkeypatch.setenv("GMS_SLAM_EAGER_LIK", "1")                            # the handle without class planes
    scans = _scans(EXT, RES, BEAMS, T, seed0=300)
    u = _odometry(S, T, seed=5)
    rng = np.random.default_rng(9)
    corner = (-EXT / 2, -EXT / 2)
    bat = SLAMParticleMapsBatch(S, EXT, EXT, RES, corner, num_particles=N, max_beams=max(BEAMS) + 8)
    alone = [SLAMParticleMaps(EXT, EXT, RES, corner, num_particles=N, max_beams=max(BEAMS) + 8) for _ in range(S)]
    dst, other, pair = _destination(), _destination(), _destination(n_maps=2)
    d_log = wc.dst_log()
    gd, gs = wx.Geometry.of(dst), wx.Geometry.of(bat.grid_map)
    assert (bat.W, bat.H) == (120, 120)
    pose = wc.turned(0.3, (0.2, -0.1), (gd.px + 5.0, gd.py + 3.4))                # the filters' world about its middle, turned, in the middle of dst
    kw = dict(c=pose[2], s=pose[3])

    def update(k):
        zs = [scans[f][k] for f in range(S)]
        neff = bat.update(zs, [tuple(u[k, f]) for f in range(S)], seeds=SEEDS, sequence=k)
        for f in range(S):
            alone[f].update(zs[f], tuple(u[k, f]), seed=int(SEEDS[f]), sequence=k)
        return neff
    try:
        P0 = synth.make_particles(np.zeros(3), N * S, seed=3, sigma_xy=0.02, sigma_theta_deg=1.0).reshape(S, N, 3)
        bat.set_poses(P0)
        for f in range(S):
            alone[f].set_poses(P0[f])
        dst.upload_log(d_log)
        _refused(GMS_ERR_STATE, bat.warp_into, dst, "strongest", 1, pose[:2], **kw)            # no strongest particle before the first update
        # 1. frames until one resample_if splits the filters
        did, k = np.zeros(S, bool), 0
        while not (did.any() and not did.all()):
            assert k < T - 1, "no frame on which some filters resampled and others did not"
            ratio = np.sort(update(k) / N)
            k += 1
            if ratio[0] == ratio[-1]:
                continue
            before_draw = bat.maps()
            r01 = rng.random(S)
            frac = float(ratio[0] + ratio[-1]) / 2
            bat.resample_if(r01, frac)
            for f in range(S):
                alone[f].resample_if(float(r01[f]), frac)
            did = bat.did_resample()
            assert np.array_equal(did, [a.pf.did_resample() for a in alone])
        assert did.any() and not did.all(), "the filters sit on different generations"
        update(k)
        k += 1
        _compare(bat, alone, f"{form}: before the warps")
        # 3. a wrong slot or generation cannot give the expected bits
        logs = bat.maps()
        strongest = [int(bat.last_stats[f]["strongest"]) for f in range(S)]
        asked = [(f, i) for f in range(S) for i in (*NAMED[f], strongest[f])]
        for f, i in asked:
            for g in range(S):
                assert g == f or not np.array_equal(wx.bits(logs[f, i]), wx.bits(logs[g, i])), f"particle {i} of filters {f} and {g}"
            if did[f]:
                assert not np.array_equal(wx.bits(logs[f, i]), wx.bits(before_draw[f, i])), f"filter {f} drew: slot {i} is not the stale one"
        before = _state(bat), [_state(a) for a in alone]
        # 2. every filter: its strongest particle and two named ones, the four ops spread over the calls
        call = 0
        for f in range(S):
            for which in ("strongest", *NAMED[f]):
                op = OPS[call % 4]
                call += 1
                i = strongest[f] if which == "strongest" else which
                dst.upload_log(d_log); other.upload_log(d_log)
                st, shown = bat.warp_into(dst, which, f, pose[:2], op=op, clamp=CLAMP, **kw)
                assert shown == f * N + i, (f, which)
                want_log, want_st = wx.expect(d_log, gd, logs[f, i], gs, pose, op, clamp=CLAMP)
                got = dst.download_log()
                assert np.array_equal(wx.bits(got), wx.bits(want_log)), (f, which, op)
                assert np.array_equal(st["pair"], want_st["pair"]) and st["n_outside"] == want_st["n_outside"], (f, which, op)
                assert want_st["pair"][:, 1:].sum() > 100, "the particle's map shows in the destination"
                st1, shown1 = alone[f].warp_into(other, which, pose[:2], op=op, clamp=CLAMP, **kw)
                assert shown1 == i and st1 == st and np.array_equal(wx.bits(other.download_log()), wx.bits(got)), f"the stand-alone handle {f}"
        # 4. the device form, filter 2: the counts, the shown slot, nothing past either
        dst.upload_log(d_log)
        out = torch.full((12,), -7, dtype=torch.int64, device="cuda")
        shw = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert bat.warp_into_dev(dst, out[1:11], "strongest", 2, pose[:2], op="add", clamp=CLAMP, shown_out=shw[1:2], **kw) is not None
        got = dst.download_log()                                                 # (synchronises the destination's stream)
        torch.cuda.synchronize()
        want_log, want_st = wx.expect(d_log, gd, logs[2, strongest[2]], gs, pose, "add", clamp=CLAMP)
        raw = out.cpu().numpy()
        assert np.array_equal(wx.bits(got), wx.bits(want_log)) and shw.cpu().tolist() == [-7, 2 * N + strongest[2], -7, -7]
        assert raw[0] == -7 and raw[11] == -7 and np.array_equal(raw[1:10].reshape(3, 3), want_st["pair"]) and raw[10] == want_st["n_outside"]
        shw.fill_(-7)
        torch.cuda.synchronize()
        bat.warp_into_dev(dst, None, NAMED[1][1], 1, pose[:2], op="replace", shown_out=shw[2:3], **kw)
        got = dst.download_log()
        torch.cuda.synchronize()
        assert np.array_equal(wx.bits(got), wx.bits(wx.expect(want_log, gd, logs[1, NAMED[1][1]], gs, pose, "replace")[0]))
        assert shw.cpu().tolist() == [-7, -7, N + NAMED[1][1], -7]
        # 5. a named particle into a rectangle of map 1 of a two-map destination, over a guard pattern
        guard = np.full((2, wc.H_D, wc.W_D), wc.GUARD)
        rect = (63, 60, 66, 5)
        for op in ("replace", "add", "fill"):
            pair.upload_log(guard)
            st, shown = bat.warp_into(pair, NAMED[2][0], 2, pose[:2], op=op, rect=rect, mi=1, **kw)
            want_log, want_st = wx.expect(guard[1], gd, logs[2, NAMED[2][0]], gs, pose, op, rect=rect)
            got = pair.download_log()
            assert shown == 2 * N + NAMED[2][0] and np.array_equal(wx.bits(got[1]), wx.bits(want_log)) and st == want_st, op
            assert (got[0] == wc.GUARD).all(), "map 0 keeps the guard"
            keeps = np.ones((wc.H_D, wc.W_D), bool)
            keeps[60:65, 63:129] = False
            assert (got[1][keeps] == wc.GUARD).all() and want_st["pair"].sum() + want_st["n_outside"] == 66 * 5
            assert op == "fill" or (got[1][~keeps] != wc.GUARD).any(), "the rectangle was written"
        # 6. refusals, nothing touched
        dst.upload_log(d_log)
        for bad in (-1, S):
            for which in ("strongest", 0):
                with pytest.raises(IndexError):
                    bat.warp_into(dst, which, bad, pose[:2], op="replace", **kw)
                with pytest.raises(IndexError):
                    bat.warp_into_dev(dst, None, which, bad, pose[:2], op="replace", **kw)
            _refused(GMS_ERR_INVALID, bat._warp, "strongest", bad, dst, pose[:2], pose[2], pose[3], "replace", None, 0.0, 0, True, None, None, False)
        with pytest.raises(IndexError):
            bat.warp_into(dst, N, 1, pose[:2], op="replace", **kw)
        for slot in (-2, S * N):                                                 # (the library's own bound is the handle's S * n slots)
            _refused(GMS_ERR_INVALID, bat._warp, slot, 0, dst, pose[:2], pose[2], pose[3], "replace", None, 0.0, 0, True, None, None, False)
        _refused(GMS_ERR_INVALID, bat.warp_into, bat.grid_map, 0, 1, pose[:2], op="replace", **kw)
        assert np.array_equal(wx.bits(dst.download_log()), wx.bits(d_log))
        # 7. the filters were only read
        assert all(np.array_equal(a, b) for a, b in zip(_state(bat), before[0])), "poses, weights and maps are bit-identical"
        for f in range(S):
            assert all(np.array_equal(a, b) for a, b in zip(_state(alone[f]), before[1][f]))
        update(k)
        _compare(bat, alone, f"{form}: the update behind the warps")
        bat.reset()
        _refused(GMS_ERR_STATE, bat.warp_into, dst, "strongest", 0, pose[:2], **kw)            # ... and none after a reset
        assert np.array_equal(wx.bits(dst.download_log()), wx.bits(d_log))
    finally:
        bat.close()
        for h in (*alone, dst, other, pair):
            h.close()


def test_named_particle_of_a_shard_is_the_whole_filters_block():
    """two shard handles (offsets 0 and GMS_BLOCK of 2 GMS_BLOCK: gms_slam_create_shard takes no smaller block) updated with
    gms_slam_update_local beside a whole filter: shard r's local particle i warps to the bits of the whole filter's particle
    GMS_BLOCK r + i, shown is the local index, and "strongest" is refused"""
    ext, NL, NG = 3.2, GMS_BLOCK, 2 * GMS_BLOCK
    tr = synth.make_trace(ext, RES, 64, T=4, seed=23)
    scans = [(np.ascontiguousarray(z, dtype=BEAM_DTYPE), (0.02, 0.1)) for z in tr.scans[:4]]
    start = np.tile(np.asarray(tr.poses[0], np.float32), (NG, 1))
    whole = SLAMParticleMaps(ext, ext, RES, (-ext / 2, -ext / 2), num_particles=NG, max_beams=64)
    whole.set_poses(start)
    shards = []
    for r in range(2):
        s = SLAMParticleMaps.__new__(SLAMParticleMaps)
        s._init_shard(ext, ext, RES, (-ext / 2, -ext / 2), NL, r * NL, NG, max_beams=64)
        s.set_poses(start[:NL])
        shards.append(s)
    dst, other = _destination(), _destination()
    d_log = wc.dst_log()
    gd, gs = wx.Geometry.of(dst), wx.Geometry.of(whole.grid_map)
    pose = wc.turned(-0.7, (0.1, 0.2), (gd.px + 4.0, gd.py + 3.0))
    kw = dict(c=pose[2], s=pose[3])
    L = load()
    try:
        for k, (z, u) in enumerate(scans):
            zb = np.ascontiguousarray(z)
            whole.update(z, u, seed=21, sequence=k)
            for s in shards:
                assert L.gms_slam_update_local(s._h, ptr(zb), len(zb), 1, float(u[0]), float(u[1]), 21, k) == 0
        logs = whole.maps()
        for r, s in enumerate(shards):
            assert np.array_equal(wx.bits(s.maps()), wx.bits(logs[r * NL:(r + 1) * NL])), f"shard {r}: logData"
        for i in (0, 137, NL - 1):
            assert not np.array_equal(wx.bits(logs[i]), wx.bits(logs[NL + i])), "the blocks differ: a wrong offset shows"
        for r, s in enumerate(shards):
            for i, op in ((0, "replace"), (NL - 1, "add"), (137, "fill")):
                dst.upload_log(d_log); other.upload_log(d_log)
                st, shown = s.warp_into(dst, i, pose[:2], op=op, clamp=CLAMP, **kw)
                assert shown == i, "the local index is the slab index"
                want_log, want_st = wx.expect(d_log, gd, logs[r * NL + i], gs, pose, op, clamp=CLAMP)
                got = dst.download_log()
                assert np.array_equal(wx.bits(got), wx.bits(want_log)) and st == want_st, (r, i, op)
                assert want_st["pair"][:, 1:].sum() > 100, "the particle's map shows in the destination"
                st1, shown1 = whole.warp_into(other, r * NL + i, pose[:2], op=op, clamp=CLAMP, **kw)
                assert shown1 == r * NL + i and st1 == st and np.array_equal(wx.bits(other.download_log()), wx.bits(got))
            dst.upload_log(d_log)
            _refused(GMS_ERR_STATE, s.warp_into, dst, "strongest", pose[:2], op="replace", **kw)
            _refused(GMS_ERR_INVALID, s.warp_into, dst, NL, pose[:2], op="replace", **kw)
            assert np.array_equal(wx.bits(dst.download_log()), wx.bits(d_log))
    finally:
        whole.close()
        for h in (*shards, dst, other):
            h.close()
