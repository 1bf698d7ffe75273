"""Continuous scan alignment (include/gridmapslam.h "continuous scan alignment") without a device: the structs' layout in header, mirror,
dtype and a compiled offsetof program, the exported symbols, gms_align_check on every field, the defaults, the entry points' refusals on
a fake handle, align_covariance on hand-made records, and the restatement (tests/_align_expect.py) on the synthetic room: the
definition's own sanity, which guards e.g. the sign of g."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _align_expect as ax
from gridmap_slam_robot_amd import AlignParams, _lib, align_covariance
from gridmap_slam_robot_amd._lib import ALIGN_DTYPE, GMS_ERR_INVALID, GMS_OK, GmsAlignParams, GmsAlignRecord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_align_params_default", "gms_align_check", "gms_map_align", "gms_map_align_dev", "gms_pf_align", "gms_pf_align_dev"]
PARAM_OFFSETS = dict(iters=0, pad=4, damp_t=8, damp_r=16, max_t=24, max_r=32, eps_t=40, eps_r=48, det_min=56)
RECORD_OFFSETS = dict(status=0, iters_done=4, n_used=8, n_used0=12, score0=16, score=24, H=32)


def test_structs_in_header_mirror_dtype_and_compiled_offsets(tmp_path):
    assert C.sizeof(GmsAlignParams) == 64 and C.sizeof(GmsAlignRecord) == 80 and ALIGN_DTYPE.itemsize == 80
    for name, off in PARAM_OFFSETS.items():
        assert getattr(GmsAlignParams, name).offset == off, name
    for name, off in RECORD_OFFSETS.items():
        assert getattr(GmsAlignRecord, name).offset == off and ALIGN_DTYPE.fields[name][1] == off, name
    assert ALIGN_DTYPE.fields["H"][0].shape == (6,) and list(ALIGN_DTYPE.names) == list(RECORD_OFFSETS)
    src = tmp_path / "size.c"
    terms = (["sizeof(gms_align_params)", "sizeof(gms_align_record)"] + [f"offsetof(gms_align_params, {n})" for n in PARAM_OFFSETS]
             + [f"offsetof(gms_align_record, {n})" for n in RECORD_OFFSETS])
    fmt = " ".join(["%zu"] * len(terms))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\n'
                   f'int main(void) {{ printf("{fmt}", {", ".join(terms)}); return 0; }}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == [64, 80] + list(PARAM_OFFSETS.values()) + list(RECORD_OFFSETS.values())


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None


def test_defaults_are_deterministic_accepted_and_what_the_restatement_holds():
    L = _lib.load()
    assert L.gms_align_params_default(None) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    a, b = GmsAlignParams(), GmsAlignParams()
    C.memset(C.byref(a), 0xA5, 64)
    C.memset(C.byref(b), 0x00, 64)
    assert L.gms_align_params_default(C.byref(a)) == GMS_OK and L.gms_align_params_default(C.byref(b)) == GMS_OK
    assert bytes(a) == bytes(b)                                 # every byte, the padding included
    assert L.gms_align_check(C.byref(a)) == GMS_OK
    assert {n: getattr(a, n) for n in ax.default_params()} == ax.default_params()
    p = AlignParams(iters=3, max_t=0.25)
    assert (p.iters, p.max_t, p.damp_t, p.max_r) == (3, 0.25, a.damp_t, a.max_r) and p.check() is p
    with pytest.raises(TypeError):
        AlignParams(bogus=1)
    with pytest.raises(_lib.GmsError):
        AlignParams(iters=0).check()


NAN, INF = math.nan, math.inf
BAD = ([("iters", v) for v in (0, -1, 65, 2**31 - 1)]
       + [(f, v) for f in ("damp_t", "damp_r", "eps_t", "eps_r", "det_min") for v in (-1e-300, -1.0, NAN, INF, -INF)]
       + [(f, v) for f in ("max_t", "max_r") for v in (0.0, -0.0, -1.0, NAN, -INF)])
GOOD = ([("iters", v) for v in (1, 64)] + [(f, v) for f in ("damp_t", "damp_r", "eps_t", "eps_r", "det_min") for v in (0.0, 5e-324, 1e300)]
        + [(f, v) for f in ("max_t", "max_r") for v in (5e-324, INF)] + [("pad", 77)])


def test_align_check_refuses_each_field_out_of_range_or_non_finite():
    L = _lib.load()
    assert L.gms_align_check(None) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    for field, v in BAD:
        p = AlignParams()
        setattr(p, field, v)
        assert L.gms_align_check(C.byref(p)) == GMS_ERR_INVALID, (field, v)
        assert field.encode() in L.gms_last_error(), (field, v, L.gms_last_error())
    for field, v in GOOD:
        p = AlignParams()
        setattr(p, field, v)
        assert L.gms_align_check(C.byref(p)) == GMS_OK, (field, v)


def test_entry_points_refuse_null_pointers_and_bad_requests_untouched():
    """checked before anything is touched: the fake handles are blocks of zero bytes (max_beams 0: every B is out of range behind the
    parameters' own checks); the outputs keep their marks"""
    L = _lib.load()
    zeros = np.zeros(1 << 16, np.uint8)                # (kept alive: the handle is this memory)
    fake = zeros.ctypes.data
    beams = np.zeros(4, _lib.BEAM_DTYPE)
    poses = np.full((2, 3), 7.0, np.float32)
    out = np.full((2, 3), -3.0, np.float32)
    rec = np.full(2 * 80, 0xEE, np.uint8)
    good, bad = AlignParams(), AlignParams()
    bad.iters = 0
    bp, pp, op, rp = beams.ctypes.data, poses.ctypes.data, out.ctypes.data, rec.ctypes.data
    for fn in (L.gms_map_align, L.gms_map_align_dev):
        for args in ((None, 0, bp, 4, pp, 2, C.byref(good), op, rp), (fake, 0, None, 4, pp, 2, C.byref(good), op, rp),
                     (fake, 0, bp, 4, None, 2, C.byref(good), op, rp), (fake, 0, bp, 4, pp, 2, C.byref(good), None, rp),
                     (fake, 0, bp, 4, pp, 2, None, op, rp), (fake, 0, bp, 4, pp, 2, C.byref(bad), op, rp), (fake, 0, bp, 4, pp, 2, C.byref(good), op, rp)):
            assert fn(*args) == GMS_ERR_INVALID, args
    for fn in (L.gms_pf_align, L.gms_pf_align_dev):
        for args in ((None, bp, 4, C.byref(good), rp), (fake, None, 4, C.byref(good), rp), (fake, bp, 4, None, rp), (fake, bp, 4, C.byref(bad), rp)):
            assert fn(*args) == GMS_ERR_INVALID, args
    assert (out == -3.0).all() and (rec == 0xEE).all() and (poses == 7.0).all()


def test_align_covariance_inverts_a_hand_made_information_matrix():
    rec = np.zeros(4, ALIGN_DTYPE)
    rec["H"][0] = [4.0, 0.0, 0.0, 16.0, 0.0, 25.0]              # diag(4, 16, 25)
    rec["H"][1] = [2.0, 1.0, 0.0, 2.0, 0.0, 1.0]                # [[2, 1, 0], [1, 2, 0], [0, 0, 1]]: inverse [[2, -1, 0], [-1, 2, 0], [0, 0, 3]] / 3
    rec["H"][2] = [1.0, 1.0, 0.0, 1.0, 0.0, 1.0]                # singular
    rec["H"][3] = [1.0, 0.0, 0.0, NAN, 0.0, 1.0]
    cov = align_covariance(rec, 0.5)
    assert cov.shape == (4, 3, 3)
    assert np.array_equal(cov[0], np.diag([0.25 * 0.25, 0.25 / 16.0, 1.0 / 25.0]))
    want = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 3.0]]) / 3.0 * np.outer([0.5, 0.5, 1.0], [0.5, 0.5, 1.0])
    assert np.allclose(cov[1], want, rtol=1e-14, atol=0.0)
    assert np.isnan(cov[2]).all() and np.isnan(cov[3]).all()


# ---- the restatement's own sanity on the synthetic room (ax.room: shared with tests/test_gpu_align.py) --------------------------------
EXT, RES, SCAN = ax.EXT, ax.RES, ax.SCAN


def test_restatement_pulls_perturbed_poses_towards_the_true_one():
    """8 iterations with the default parameters: the median translation error and the median heading error both fall below their
    starting medians (DESIGN.md section 4n has the figures: 1.17 -> 0.29 cells, 1.84 -> 0.10 degrees)"""
    g, _, lik, tr = ax.room()
    true = tr.poses[SCAN].astype(np.float64)
    start = ax.perturbed(true, 24)
    out, rec = ax.align(lik, g.W, g.H, RES, -EXT / 2, -EXT / 2, tr.scans[SCAN], start, ax.default_params())
    t0, t1 = np.hypot(*(start[:, :2] - true[:2]).T), np.hypot(*(out[:, :2] - true[:2]).T)
    r0, r1 = np.abs(start[:, 2] - true[2]), np.abs(out[:, 2] - true[2])
    print(f"median translation error {np.median(t0) / RES:.3f} -> {np.median(t1) / RES:.3f} cells, "
          f"median heading error {np.degrees(np.median(r0)):.3f} -> {np.degrees(np.median(r1)):.3f} degrees")
    assert np.median(t1) < np.median(t0) and np.median(r1) < np.median(r0)
    assert np.median(rec["score"]) > np.median(rec["score0"]) and (rec["n_used"] > 0).all() and np.isin(rec["status"], (0, 1)).all()
