"""Predicted scans (include/gridmapslam.h "predicted scans") without a device: the record's size, the exported symbols in header
and library, the argument checks of the entry points, and scan_residual on hand-written cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gridmap_slam_robot_amd import _lib, scan_residual
from gridmap_slam_robot_amd import gridmap as gm
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, CAST_DTYPE, GMS_ERR_INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAST_SYMBOLS = ["gms_map_cast", "gms_map_cast_dev", "gms_map_cast_at", "gms_map_cast_at_dev", "gms_slam_cast", "gms_slam_cast_dev"]


def test_record_is_16_bytes_in_header_and_mirror(tmp_path):
    assert CAST_DTYPE.itemsize == 16 and [CAST_DTYPE.fields[n][1] for n in ("step", "x", "y", "range")] == [0, 4, 8, 12]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gridmapslam.h"\nint main(void) { printf("%zu %zu %d %d", sizeof(gms_cast_hit), '
                   'offsetof(gms_cast_hit, range), GMS_CAST_ALL, GMS_VIEW_STRONGEST); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["16", "12", str(_lib.GMS_CAST_ALL), str(_lib.GMS_VIEW_STRONGEST)]


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    L = _lib.load()
    for name in CAST_SYMBOLS + ["gms_map_cast_plane_builds"]:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name) is not None


def test_entry_points_refuse_null_handles_and_bad_counts():
    """checked before anything is touched: the fake handles are blocks of zero bytes (max_beams 0, n_maps 0), so every count is bad"""
    L = _lib.load()
    fake = np.zeros(8192, np.uint8).ctypes.data
    poses = np.zeros((2, 3), np.float32)
    probes = np.zeros(4, BEAM_DTYPE)
    out = np.zeros((2, 4), CAST_DTYPE)
    p, b, o = poses.ctypes.data, probes.ctypes.data, out.ctypes.data
    for fn in (L.gms_map_cast, L.gms_map_cast_dev):
        for args in ((None, 0, p, 2, b, 4, o), (fake, 0, None, 2, b, 4, o), (fake, 0, p, 2, None, 4, o), (fake, 0, p, 2, b, 4, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
        for args in ((fake, 0, p, 2, b, 4, o), (fake, -1, p, 2, b, 4, o), (fake, 0, p, 0, b, 4, o), (fake, 0, p, 2, b, 0, o), (fake, 0, p, 2, b, -1, o),
                     (fake, 0, p, (1 << 20) + 1, b, 4, o)):
            assert fn(*args) == GMS_ERR_INVALID
    for fn in (L.gms_map_cast_at, L.gms_map_cast_at_dev):
        for args in ((None, b, 4, fake, 0, o), (fake, None, 4, fake, 0, o), (fake, b, 4, None, 0, o), (fake, b, 4, fake, 0, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    for fn in (L.gms_slam_cast, L.gms_slam_cast_dev):
        for args in ((None, 0, 0, b, 4, o, None), ):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    assert (out.view(np.uint8) == 0).all(), "a refused cast writes nothing"


def _beams(dist, hit):
    b = np.zeros(len(dist), BEAM_DTYPE)
    b["distance"], b["hit"] = dist, hit
    return b


def _cast(step, rng):
    c = np.zeros(len(step), CAST_DTYPE)
    c["step"], c["range"] = step, rng
    return c


def test_scan_residual_one_case_per_class():
    res, tol = 0.05, 2.0                                   # distances in metres, ranges in cells; the band is +-1 cell
    beams = _beams([1.00, 1.00, 1.00, 1.00, 1.00, 10.0, 10.0], [1, 1, 1, 1, 1, 0, 0])
    cast = _cast([7, 7, 7, 7, -1, -1, 9], [20.0, 21.0, 25.0, 12.0, 20.0, 200.0, 30.0])
    got = scan_residual(beams, cast, res, tol)
    assert got.dtype == np.uint8
    assert got.tolist() == [gm.RESIDUAL_AGREE,              # 20 cells measured, 20 predicted
                            gm.RESIDUAL_AGREE,              # exactly on the band's edge: |20 - 21| <= 1
                            gm.RESIDUAL_MEASURED_SHORTER,   # 20 < 25 - 1: something the map lacks
                            gm.RESIDUAL_MEASURED_LONGER,    # 20 > 12 + 1: the map has a wall the beam passed
                            gm.RESIDUAL_NO_PREDICTION,      # a return, and nothing on the walk
                            gm.RESIDUAL_AGREE,              # a miss, and nothing on the walk
                            gm.RESIDUAL_MEASURED_LONGER]    # a miss through a predicted wall
    nan = scan_residual(_beams([np.nan], [1]), _cast([3], [20.0]), res, tol)
    assert nan.tolist() == [gm.RESIDUAL_NO_PREDICTION]
    with pytest.raises(ValueError):
        scan_residual(beams, cast[:3], res, tol)
