"""The beam sensor model (include/gridmapslam.h "beam sensor model") without a device: the exported symbols, every refusal of
gms_beam_model_check and of both entry points on a fake handle, beam_model_factors against entries computed by hand, and the
expectation module (tests/_beams_expect.py) -- the index rule and the order of product and sum -- on a 5-beam and a 300-beam example
worked out by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _beams_expect as bx
from gridmap_slam_robot_amd import _lib, beam_model_factors
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_INVALID, GMS_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_beam_model_check", "gms_pf_score_beams", "gms_pf_score_beams_dev"]


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None
    assert "gms_pf_score_beams(" in mirror and "gms_pf_score_beams_dev(" in mirror
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                           os.path.join(ROOT, "include", "gridmapslam.hpp")])


def _table(behind, ahead, **put):
    f = np.full((2, behind + ahead + 2), 0.5)
    for k, v in put.items():
        f.reshape(-1)[int(k[1:])] = v
    return f


# (behind, ahead, entries to overwrite, the word the message must hold)
BAD = [(-1, 2, {}, b"behind"), (256, 2, {}, b"behind"), (3, -1, {}, b"ahead"), (3, 256, {}, b"ahead"),
       (3, 2, dict(e0=0.0), b"factors[0][0]"), (3, 2, dict(e6=-0.0), b"factors[0][6]"), (3, 2, dict(e7=-1.0), b"factors[1][0]"),
       (3, 2, dict(e13=math.nan), b"factors[1][6]"), (3, 2, dict(e9=math.inf), b"factors[1][2]"), (0, 0, dict(e3=-math.inf), b"factors[1][1]")]


def test_beam_model_check_ranges():
    L = _lib.load()
    assert L.gms_beam_model_check(3, 2, None) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    for behind, ahead, put, word in BAD:
        f = _table(max(behind, 0) % 256, max(ahead, 0) % 256, **put)
        assert L.gms_beam_model_check(behind, ahead, f.ctypes.data) == GMS_ERR_INVALID, (behind, ahead, put)
        assert word in L.gms_last_error(), (behind, ahead, put, L.gms_last_error())
    for behind, ahead, put in ((0, 0, {}), (255, 255, {}), (3, 2, dict(e0=5e-324, e13=1.7976931348623157e308)), (0, 255, {}), (255, 0, {})):
        f = _table(behind, ahead, **put)
        assert L.gms_beam_model_check(behind, ahead, f.ctypes.data) == GMS_OK, (behind, ahead, put)


def test_entry_points_refuse_bad_arguments_on_a_fake_handle():
    """checked before anything is touched: the fake filter is a block of zero bytes whose first field, the map, points at a block
    whose every int32 is 7 -- a handle of max_beams = 7 --, so B = 8 is one too many; neither block is written"""
    L = _lib.load()
    fake_map = np.full(1 << 14, 7, np.int32)               # (kept alive: the handles are this memory)
    fake_pf = np.zeros(1 << 11, np.uint64)
    fake_pf[0] = fake_map.ctypes.data
    pf = fake_pf.ctypes.data
    beams = np.zeros(8, dtype=BEAM_DTYPE)
    res = np.full(64, 0xABCD, np.uint16)
    good = _table(3, 2)
    for fn in (L.gms_pf_score_beams, L.gms_pf_score_beams_dev):
        for args in ((None, beams.ctypes.data, 4, 3, 2, good.ctypes.data), (pf, None, 4, 3, 2, good.ctypes.data), (pf, beams.ctypes.data, 4, 3, 2, None)):
            assert fn(*args, res.ctypes.data) == GMS_ERR_INVALID and b"null" in L.gms_last_error(), args
        for behind, ahead, put, word in BAD:
            f = _table(max(behind, 0) % 256, max(ahead, 0) % 256, **put)
            assert fn(pf, beams.ctypes.data, 4, behind, ahead, f.ctypes.data, res.ctypes.data) == GMS_ERR_INVALID, (behind, ahead, put)
            assert word in L.gms_last_error(), (behind, ahead, put, L.gms_last_error())
        for B in (0, 8, -3):
            assert fn(pf, beams.ctypes.data, B, 3, 2, good.ctypes.data, res.ctypes.data) == GMS_ERR_INVALID, B
            assert b"max_beams" in L.gms_last_error(), L.gms_last_error()
    assert L.gms_pf_score_beams_dev(pf, beams.ctypes.data, 4, 3, 2, good.ctypes.data, res.ctypes.data + 1) == GMS_ERR_INVALID
    assert b"aligned" in L.gms_last_error()
    assert (res == 0xABCD).all() and (fake_map == 7).all() and fake_pf[0] == fake_map.ctypes.data and not fake_pf[1:].any(), "a refused call writes nothing"


def test_beam_model_factors_by_hand():
    # sigma = one step: r / sigma = d = -2, -1, 0, 1; every weight a binary fraction
    f = beam_model_factors(0.05, 2, 1, 0.05, z_hit=0.5, z_short=0.25, z_rand=0.125, z_miss=0.75)
    assert f.shape == (2, 5) and f.dtype == np.float64
    assert f[0].tolist() == [0.125, 0.125, 0.125, 0.125, 0.875], "a miss: the floor under every wall, z_miss + z_rand under none"
    assert f[1, 2] == 0.625 and f[1, 4] == 0.375, "d = 0: z_hit + z_rand; none: z_short + z_rand"
    # (numpy's exp and libm's may differ in the last place: 4 ulp)
    assert f[1, 0] == pytest.approx(0.5 * math.exp(-2.0) + 0.125, rel=1e-15) and f[1, 1] == pytest.approx(0.5 * math.exp(-0.5) + 0.125, rel=1e-15)
    assert f[1, 3] == pytest.approx(0.5 * math.exp(-0.5) + 0.375, rel=1e-15), "d = 1: the short-reading term on top"
    assert f[1, 3] - f[1, 1] == pytest.approx(0.25, abs=1e-15)
    # a wide sigma: the Gaussian of d * resolution, not of d
    g = beam_model_factors(0.02, 0, 3, 0.04, z_hit=1.0, z_short=0.0, z_rand=0.5, z_miss=0.0)
    assert g.shape == (2, 5) and g[1, 0] == 1.5 and g[1, 2] == pytest.approx(math.exp(-0.5) + 0.5, rel=1e-15) and g[0].tolist() == [0.5] * 5
    assert beam_model_factors(0.05, 0, 0, 0.1).shape == (2, 2) and beam_model_factors(0.05, 255, 255, 0.1).shape == (2, 512)
    L = _lib.load()
    assert L.gms_beam_model_check(255, 255, beam_model_factors(0.05, 255, 255, 0.01).ctypes.data) == GMS_OK, "the far tail stays > 0 through z_rand"
    for kw in (dict(behind=-1), dict(ahead=256), dict(sigma=0.0), dict(z_rand=0.0), dict(resolution=0.0), dict(z_hit=-1.0)):
        args = dict(resolution=0.05, behind=2, ahead=2, sigma=0.05)
        args.update(kw)
        with pytest.raises(ValueError):
            beam_model_factors(**args)
    assert "sqrt(2)" in beam_model_factors.__doc__


def test_init_count_with_javas_casts():
    # finite: 1 + extra + |dfloor x| + |dfloor y|
    assert bx.n0_of(10.5, 10.5, 15.5, 10.5, 2) == 8 and bx.n0_of(10.5, 10.5, 7.2, 12.9, 0) == 1 + 3 + 2
    assert bx.n0_of(3.5, 3.5, 3.5, 3.5, 5) == 6, "no length: 1 + extra"
    # NaN end: dx is NaN (not 0), x1 > x0 is false: n += x - (int)floor(NaN) = x - 0
    assert bx.n0_of(4.5, 6.5, math.nan, math.nan, 1) == 2 + 4 + 6
    # +Inf end: n += (int)(Inf - x) saturates, and the add wraps
    assert bx.n0_of(4.5, 6.5, math.inf, 6.5, 1) == bx._wrap(2 + 2147483647)
    assert bx.n0_of(4.5, 6.5, -math.inf, 6.5, 0) == bx._wrap(1 + bx._wrap(4 + 2147483648))
    # NaN start: cell 0; the end decides nothing (x1 > NaN is false): n += 0 - floor(x1)
    assert bx.n0_of(math.nan, math.nan, 3.5, 2.5, 0) == 1 - 3 - 2


def test_index_rule_and_order_on_five_beams_by_hand():
    behind, ahead = 3, 2                                   # T = 7, top = 6; d = ahead + 1 - n_rem
    n_rem = [1, 3, 6, 7, None, 40]                         # d = 2, 0, -3, -4 (held at -3), none, -37 (held)
    idx = [bx.index_of(n, behind, ahead) for n in n_rem]
    assert idx == [5, 3, 0, 0, 6, 0]
    assert [bx.index_of(n, 0, 0) for n in (1, 2, None)] == [0, 0, 1], "behind = ahead = 0: the end cell, anything in front, none"
    assert [bx.index_of(n, 255, 255) for n in (1, 256, 511, 512, None)] == [510, 255, 0, 0, 511]
    # powers of two: the product is exact whatever the order; row 0 for the beams that missed
    f = np.array([[2.0 ** -(k + 1) for k in range(7)], [2.0 ** (k + 1) for k in range(7)]])
    hit = np.array([1, 0, 1, 1, 0], dtype=bool)
    w, lw = bx.weights_of(np.array(idx[:5]), hit, f)
    assert w == 2.0 ** 6 * 2.0 ** -4 * 2.0 * 2.0 * 2.0 ** -7 == 0.125
    # the sum: five partials of one beam; the tree adds +0.0 down to s = 8, then p0 += p4, p0 += p2 and p1 += p3, p0 += p1
    l = [math.log(2.0 ** 6), math.log(2.0 ** -4), math.log(2.0), math.log(2.0), math.log(2.0 ** -7)]
    assert lw == ((l[0] + l[4]) + l[2]) + (l[1] + l[3])
    # one beam, none: the table's last entry, alone
    w, lw = bx.weights_of(np.array([6]), np.array([False]), f)
    assert w == 2.0 ** -7 and lw == math.log(2.0 ** -7)


def test_order_on_three_hundred_beams_by_hand():
    # the tree itself: 1 in lane 0, 2^-53 behind it in the same lane (lost against 1), two more in lane 1 (2^-52 together: kept)
    v = np.zeros(300)
    v[0], v[256], v[1], v[257] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    assert bx.tree(v, 0.0, np.add) == 1.0 + 2.0 ** -52
    assert np.cumsum(v)[-1] == 1.0, "(one chain in index order loses all three)"
    assert bx.tree(np.zeros(0), 1.0, np.multiply) == 1.0 and bx.tree(np.zeros(0), 0.0, np.add).tobytes() == np.float64(0.0).tobytes()
    # 300 beams under a table whose products round: lanes 0 .. 43 hold two beams, the tree restated in plain Python
    rng = np.random.default_rng(300)
    behind, ahead = 4, 3
    T = behind + ahead + 2
    f = rng.uniform(0.05, 1.5, (2, T))
    idx = rng.integers(0, T, 300)
    hit = rng.random(300) < 0.7
    p, s = [1.0] * 256, [0.0] * 256
    for b in range(300):
        p[b % 256] = p[b % 256] * float(f[int(hit[b]), idx[b]])
        s[b % 256] = s[b % 256] + math.log(float(f[int(hit[b]), idx[b]]))
    h = 128
    while h >= 1:
        for k in range(h):
            p[k], s[k] = p[k] * p[k + h], s[k] + s[k + h]
        h //= 2
    w, lw = bx.weights_of(idx, hit, f)
    assert bx.same_bits(w, p[0]) and bx.same_bits(lw, s[0])
    chain = 1.0
    for b in range(300):
        chain *= float(f[int(hit[b]), idx[b]])
    assert abs(chain / p[0] - 1.0) < 1e-13, "the same product up to rounding"
    # 300 decades: the product underflows to 0, the sum of logarithms stays finite
    f2 = np.array([[1e-300, 1.0], [1e-300, 1.0]])
    w, lw = bx.weights_of(np.zeros(300, dtype=np.int64), np.ones(300, dtype=bool), f2)
    assert w == 0.0 and math.isfinite(float(lw)) and abs(float(lw) - 300 * math.log(1e-300)) < 1e-6
