"""The per-particle beam sensor model (include/gridmapslam.h "per-particle beam sensor model") without a device: the three exported
symbols in the header, the C++ mirror and the library, the refusals that come before a handle is looked at -- on a fake handle, a
block of zero bytes, which a call that got past its checks would follow into its null map -- and the Python setters' argument
handling."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, _lib
from gridmap_slam_robot_amd._lib import BEAM_DTYPE, GMS_ERR_INVALID, GMS_SLAM_BEAMS_MULTIPLY, GMS_SLAM_BEAMS_REPLACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gms_slam_score_beams", "gms_slam_score_beams_dev", "gms_slam_set_beam_model"]


def test_symbols_in_header_mirror_and_library():
    header = open(os.path.join(ROOT, "include", "gridmapslam.h")).read()
    mirror = open(os.path.join(ROOT, "include", "gridmapslam.hpp")).read()
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name).restype is C.c_int, name
    vp, i32 = C.c_void_p, C.c_int32
    assert L.gms_slam_score_beams.argtypes == [vp, vp, i32, i32, i32, vp, vp] == L.gms_slam_score_beams_dev.argtypes
    assert L.gms_slam_set_beam_model.argtypes == [vp, i32, i32, vp, i32]
    assert re.search(r"#define GMS_SLAM_BEAMS_MULTIPLY 0\b", header) and re.search(r"#define GMS_SLAM_BEAMS_REPLACE +1\b", header)
    assert (GMS_SLAM_BEAMS_MULTIPLY, GMS_SLAM_BEAMS_REPLACE) == (0, 1)
    assert "per-particle beam sensor model" in header and "gms_slam_reset keeps the setting" in header
    assert "gms_slam_score_beams(" in mirror and "gms_slam_set_beam_model(" in mirror
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


def test_set_beam_model_refuses_bad_arguments_before_the_handle():
    L = _lib.load()
    zeros = np.zeros(8192, np.uint8)
    fake = zeros.ctypes.data
    good = _table(3, 2)
    assert L.gms_slam_set_beam_model(None, 3, 2, good.ctypes.data, 0) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    assert L.gms_slam_set_beam_model(None, 0, 0, None, 0) == GMS_ERR_INVALID
    for behind, ahead, put, word in BAD:
        f = _table(max(behind, 0) % 256, max(ahead, 0) % 256, **put)
        for combine in (GMS_SLAM_BEAMS_MULTIPLY, GMS_SLAM_BEAMS_REPLACE):
            assert L.gms_slam_set_beam_model(fake, behind, ahead, f.ctypes.data, combine) == GMS_ERR_INVALID, (behind, ahead, put)
            assert word in L.gms_last_error() and b"gms_slam_set_beam_model" in L.gms_last_error(), (behind, ahead, put, L.gms_last_error())
    for combine in (-1, 2, 7):
        assert L.gms_slam_set_beam_model(fake, 3, 2, good.ctypes.data, combine) == GMS_ERR_INVALID, combine
        assert b"combine" in L.gms_last_error()
    # good arguments reach the handle, which is none
    assert L.gms_slam_set_beam_model(fake, 3, 2, good.ctypes.data, GMS_SLAM_BEAMS_REPLACE) == GMS_ERR_INVALID and b"handle" in L.gms_last_error()
    assert L.gms_slam_set_beam_model(fake, 0, 0, None, 0) == GMS_ERR_INVALID and b"handle" in L.gms_last_error()
    assert not zeros.any(), "a refused call wrote to the handle"


def test_score_beams_refuses_bad_arguments_before_the_handle():
    L = _lib.load()
    zeros = np.zeros(8192, np.uint8)
    fake = zeros.ctypes.data
    beams = np.zeros(8, dtype=BEAM_DTYPE)
    res = np.full(64, 0xABCD, np.uint16)
    good = _table(3, 2)
    for fn in (L.gms_slam_score_beams, L.gms_slam_score_beams_dev):
        for args in ((None, beams.ctypes.data, 4, 3, 2, good.ctypes.data), (fake, None, 4, 3, 2, good.ctypes.data), (fake, beams.ctypes.data, 4, 3, 2, None)):
            assert fn(*args, res.ctypes.data) == GMS_ERR_INVALID and b"null" in L.gms_last_error(), args
        for behind, ahead, put, word in BAD:
            f = _table(max(behind, 0) % 256, max(ahead, 0) % 256, **put)
            assert fn(fake, beams.ctypes.data, 4, behind, ahead, f.ctypes.data, res.ctypes.data) == GMS_ERR_INVALID, (behind, ahead, put)
            assert word in L.gms_last_error(), (behind, ahead, put, L.gms_last_error())
        assert fn(fake, beams.ctypes.data, 4, 3, 2, good.ctypes.data, res.ctypes.data) == GMS_ERR_INVALID and b"handle" in L.gms_last_error()
    assert (res == 0xABCD).all() and not zeros.any(), "a refused call writes nothing"


class _Recorder:
    """stands in for the library: records what a setter passes down"""

    def __init__(self):
        self.calls = []

    def gms_slam_set_beam_model(self, h, behind, ahead, factors, combine):
        self.calls.append((behind, ahead, factors, combine))
        return 0


@pytest.mark.parametrize("cls", [SLAMParticleMaps, SLAMParticleMapsBatch])
def test_python_setter_argument_handling(cls, monkeypatch):
    from gridmap_slam_robot_amd import gridmap
    rec = _Recorder()
    monkeypatch.setattr(gridmap, "load", lambda: rec)
    s = cls.__new__(cls)
    s._h = C.c_void_p(0)                                      # (close() then has nothing to destroy)
    f = np.full((2, 7), 0.5)
    s.set_beam_model(f, 3, 2)
    s.set_beam_model(f.tolist(), behind=3, ahead=2, combine="replace")
    s.set_beam_model(None)
    s.set_beam_model(None, 9, 9, combine="whatever")          # off is off
    assert [(c[0], c[1], c[3]) for c in rec.calls] == [(3, 2, 0), (3, 2, 1), (0, 0, 0), (0, 0, 0)]
    assert rec.calls[0][2] is not None and rec.calls[2][2] is None and rec.calls[3][2] is None
    for args, kw in (((f, 3, 3), {}), ((f[:1], 3, 2), {}), ((np.full(14, 0.5), 3, 2), {}), ((f, 3, 2), dict(combine="add")),
                     ((f, 3, 2), dict(combine=1))):
        with pytest.raises(ValueError):
            s.set_beam_model(*args, **kw)
    assert len(rec.calls) == 4, "a refused call reaches no library"
    assert callable(SLAMParticleMaps.score_beams) and callable(SLAMParticleMaps.score_beams_dev)
    assert not hasattr(SLAMParticleMapsBatch, "score_beams"), "a batched handle has the setter only (GMS_ERR_STATE in the library)"
