"""The two forms of the beam sensor model give the same bits when every particle's map IS the shared map: ParticleFilter.score_beams
(k_beam_score: the window staged from the map's packed plane) and SLAMParticleMaps.score_beams (k_slam_beam_score: the window packed
from a particle's logData) run one workgroup body (gms_beams_device.h) over two sources of occupancy bits, and this is the property
that body exists to keep.  Residuals, weights and log-weights of the two are compared bit for bit with each other and with
tests/_beams_expect.py, every index and every weight.

The cases: a 48 x 40 map (a row is one whole plane word plus half of the next) with the LDS window and with GMS_CAST_WALK=mem, a
300 x 300 map, and a 736 x 720 map.  A window is at most the map's whole plane -- 3000 words at 300 x 300, under the cap of 16384
words -- so it is the 736 x 720 map (23 words x 720 rows = 16560) on which the window exceeds the cap and every bit comes from
memory; the case asserts that.  logData holds occupied, free and unknown cells and 0.0, -0.0, NaN and 5e-324; 5 particles, one pose
outside the map; 257 beams (lane 0 owns two, the tree sees 255 neutral partials), hits and misses, one of zero length; tables
(behind, ahead) = (3, 2) of random factors in [0.7, 1.3]."""
import functools
import math
import os

import numpy as np
import pytest

import _beams_expect as bx
from gridmap_slam_robot_amd import GridMap, ParticleFilter, SLAMParticleMaps
from gridmap_slam_robot_amd._lib import BEAM_DTYPE
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

RES = 0.05
N, B, BEHIND, AHEAD = 5, 257, 3, 2
LDS_WORDS = 64 * 1024 // 4


def _with_walk(mem, make):
    old = os.environ.pop("GMS_CAST_WALK", None)
    if mem:
        os.environ["GMS_CAST_WALK"] = "mem"                                # read when a handle is created
    try:
        return make()
    finally:
        os.environ.pop("GMS_CAST_WALK", None)
        if old is not None:
            os.environ["GMS_CAST_WALK"] = old


@functools.lru_cache(maxsize=None)
def _case(W, H):
    """(size, logData [H][W], poses [5][3], beams [257], factors [2][7], the expectation (w, logw, idx)) of a W x H map"""
    size = ((W - 0.4) * RES, (H - 0.4) * RES)
    g = orc.Grid(size[0], size[1], RES, 0.0, 0.0)
    assert (g.W, g.H) == (W, H)
    rng = np.random.default_rng(W * 1000 + H)
    u = rng.random((H, W))
    log = np.where(u < 0.02, g.l_occ, np.where(u < 0.6, g.l_free, 0.0))
    for v in (0.0, -0.0, np.nan, 5e-324):
        log[rng.integers(0, H, 40), rng.integers(0, W, 40)] = v
    poses = np.column_stack([rng.uniform(0.2, size[0] - 0.2, N), rng.uniform(0.2, size[1] - 0.2, N), rng.uniform(-math.pi, math.pi, N)])
    poses[0] = (size[0] / 2, size[1] / 2, 0.3)
    poses[3] = (-0.6, size[1] / 2, 0.1)                                    # outside the map
    ang = np.linspace(-math.pi, math.pi, B, endpoint=False) + 0.01
    short = rng.random(B) < 0.7                                            # three in ten leave the map, in every direction
    dist = np.where(short, rng.uniform(0.05, 0.45 * min(size), B), rng.uniform(1.0, 1.5, B) * max(size))
    beams = np.zeros(B, dtype=BEAM_DTYPE)
    beams["local_x"], beams["local_y"], beams["distance"] = dist * np.cos(ang), dist * np.sin(ang), dist
    beams["hit"] = rng.random(B) < 0.7
    beams["local_x"][5] = beams["local_y"][5] = beams["distance"][5] = 0.0   # zero length
    factors = rng.uniform(0.7, 1.3, (2, BEHIND + AHEAD + 2))
    poses = poses.astype(np.float32)
    want = bx.expect(g, log, beams, poses, factors, BEHIND, AHEAD)
    for a in (log, poses, beams, factors) + want:
        a.flags.writeable = False
    return size, log, poses, beams, factors, want, g


@pytest.mark.parametrize("W,H,source", [(48, 40, "lds"), (48, 40, "mem"), (300, 300, "lds"), (736, 720, "cap")])
def test_shared_map_and_per_particle_forms_give_the_same_bits(W, H, source):
    size, log, poses, beams, factors, (w, lw, idx), g = _case(W, H)
    top = BEHIND + AHEAD + 1
    # what the case must contain for the comparison to mean something
    assert set(np.unique(beams["hit"])) == {0, 1} and (idx == top).any() and (idx < top).mean() > 0.2, "walls found and walks that find none"
    assert (idx[3] == top).all(), "a pose outside the map starts no walk"
    assert (np.isnan(log).any() and (log == 5e-324).any() and np.signbit(log[log == 0.0]).any() and (log > 1e-300).any() and (log < 0).any())
    words = [bx.window_words(g, beams, p, AHEAD) for p in poses]
    if source == "cap":
        assert min(words[:3]) > LDS_WORDS, words
    else:
        assert 0 < max(words) <= LDS_WORDS, words

    def make():
        m = GridMap(size[0], size[1], RES, (0.0, 0.0), max_beams=320)
        s = SLAMParticleMaps(size[0], size[1], RES, (0.0, 0.0), num_particles=N, max_beams=320)
        return m, s
    m, s = _with_walk(source == "mem", make)
    assert (m.W, m.H, s.W, s.H) == (W, H, W, H)
    m.upload_log(log)
    pf = ParticleFilter(m, N)
    pf.set_poses(poses)
    for i in range(N):
        s.set_map(i, log=log)
    s.set_poses(poses)
    res_shared = pf.score_beams(beams, factors, BEHIND, AHEAD, residuals=True)
    res_own = s.score_beams(beams, factors, BEHIND, AHEAD, residuals=True)
    got = {"shared map": (res_shared, pf.get_weights(), pf.get_log_weights()), "own maps": (res_own, s.pf.get_weights(), s.pf.get_log_weights())}
    for k, (r, gw, glw) in got.items():
        print(f"{W} x {H} {source} {k}: {int((r != idx).sum())} of {idx.size} indices differ, weights {gw.tolist()}, log-weights {glw.tolist()}")
    for k, (r, gw, glw) in got.items():
        assert r.dtype == np.uint16 and np.array_equal(r, idx), f"{k}: {int((r != idx).sum())} of {idx.size} indices differ from the expectation"
        assert bx.same_bits(gw, w), f"{k}: weights"
        assert bx.same_bits(glw, lw), f"{k}: log-weights"
    assert np.array_equal(res_shared, res_own)
    assert bx.same_bits(got["shared map"][1], got["own maps"][1]) and bx.same_bits(got["shared map"][2], got["own maps"][2])
    s.close()
