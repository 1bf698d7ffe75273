"""Per-particle scan alignment (include/gridmapslam.h "per-particle scan alignment") without a device: the exports and their ctypes
signatures, the header's text, the argument checks that come before a handle is looked at -- NULL handles, and a fake handle (a
block of zero bytes) with missing beams or parameters and with every bad parameter field: GMS_ERR_INVALID, the outputs untouched --
and the Python wrappers."""
import ctypes as C
import os

import numpy as np

from gridmap_slam_robot_amd import AlignParams, SLAMParticleMaps, SLAMParticleMapsBatch
from gridmap_slam_robot_amd._lib import ALIGN_DTYPE, BEAM_DTYPE, GMS_ERR_INVALID, GmsAlignParams, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("gms_slam_align", "gms_slam_align_dev", "gms_slam_set_align", "gms_slam_last_align")

BAD_FIELDS = (("iters", 0), ("iters", 65), ("damp_t", -1.0), ("damp_t", float("nan")), ("damp_t", float("inf")), ("damp_r", -1.0),
              ("damp_r", float("nan")), ("max_t", 0.0), ("max_t", float("nan")), ("max_r", 0.0), ("max_r", -0.1), ("eps_t", -1.0),
              ("eps_t", float("inf")), ("eps_r", float("nan")), ("det_min", -1.0), ("det_min", float("inf")))


def test_exports_and_signatures():
    L = load()
    ap = C.POINTER(GmsAlignParams)
    for name in EXPORTS:
        assert getattr(L, name).restype is C.c_int, name
    assert L.gms_slam_align.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, ap, C.c_void_p]
    assert L.gms_slam_align_dev.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, ap, C.c_void_p]
    assert L.gms_slam_set_align.argtypes == [C.c_void_p, ap]
    assert L.gms_slam_last_align.argtypes == [C.c_void_p, C.c_void_p]
    assert L.gms_slam_align_form.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]


def test_the_header_names_them():
    text = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    for name in EXPORTS + ("gms_slam_align_form", "GMS_SLAM_ALIGN_PLANES", "GMS_SLAM_ALIGN_MEMORY", "GMS_SLAM_ALIGN_FIELD"):
        assert name in text, name
    assert "int gms_slam_align(gms_slam *s, const gms_beam *beams, int32_t B, const gms_align_params *params, gms_align_record *records);" in text
    assert "int gms_slam_set_align(gms_slam *s, const gms_align_params *params);" in text
    assert "int gms_slam_last_align(gms_slam *s, gms_align_record *records);" in text


def test_argument_checks_come_before_the_handle():
    """the fake handle is a block of zero bytes: a call that got past its argument checks would follow its null map"""
    L = load()
    zeros = np.zeros(8192, np.uint8)
    fake = zeros.ctypes.data
    beams = np.zeros(4, BEAM_DTYPE)
    rec = np.full(4, 7, np.uint8).repeat(ALIGN_DTYPE.itemsize).view(ALIGN_DTYPE)
    rec0 = rec.copy()
    bp, rp = beams.ctypes.data, rec.ctypes.data
    good = AlignParams()
    for fn in (L.gms_slam_align, L.gms_slam_align_dev):
        for args in ((None, bp, 4, C.byref(good), rp), (fake, None, 4, C.byref(good), rp), (fake, bp, 4, None, rp)):
            assert fn(*args) == GMS_ERR_INVALID, args
        assert fn(fake, bp, 4, C.byref(good), rp) == GMS_ERR_INVALID                  # (no map behind it: not a handle)
        for k, v in BAD_FIELDS:
            bad = AlignParams()
            setattr(bad, k, v)
            assert fn(fake, bp, 4, C.byref(bad), rp) == GMS_ERR_INVALID, (k, v)
            assert k in L.gms_last_error().decode(), (k, v)
    assert L.gms_slam_set_align(None, C.byref(good)) == GMS_ERR_INVALID and L.gms_slam_set_align(None, None) == GMS_ERR_INVALID
    for k, v in BAD_FIELDS:
        bad = AlignParams()
        setattr(bad, k, v)
        assert L.gms_slam_set_align(fake, C.byref(bad)) == GMS_ERR_INVALID, (k, v)
    assert L.gms_slam_set_align(fake, C.byref(good)) == GMS_ERR_INVALID and L.gms_slam_set_align(fake, None) == GMS_ERR_INVALID
    assert L.gms_slam_last_align(None, rp) == GMS_ERR_INVALID and L.gms_slam_last_align(fake, None) == GMS_ERR_INVALID
    assert L.gms_slam_last_align(fake, rp) == GMS_ERR_INVALID
    assert L.gms_slam_align_form(None, C.byref(C.c_int32())) == GMS_ERR_INVALID and L.gms_slam_align_form(fake, None) == GMS_ERR_INVALID
    assert not zeros.any(), "a refused call wrote to the handle"
    assert rec.tobytes() == rec0.tobytes(), "a refused call wrote to the records"


def test_python_wrappers_exist():
    for cls in (SLAMParticleMaps, SLAMParticleMapsBatch):
        for name in ("set_align", "last_align", "align_form"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert callable(SLAMParticleMaps.align) and callable(SLAMParticleMaps.align_dev)
