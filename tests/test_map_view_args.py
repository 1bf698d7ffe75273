"""Map views (include/gridmapslam.h "map views") without a device: gms_view_size, the argument checks of the view entry points, the
exported symbols, and the grey chain of the definition as pure numpy against hand-derived values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _view_expect as ve
from gridmap_slam_robot_amd import _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID, GMS_VIEW_GREY8, GMS_VIEW_LIKELIHOOD, GMS_VIEW_LOG, GMS_VIEW_PACKED32, GmsView

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_SYMBOLS = ["gms_view_size", "gms_map_view", "gms_map_view_dev", "gms_slam_view", "gms_slam_view_dev"]


def _size(v):
    ow, oh, nb = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1)
    rc = _lib.load().gms_view_size(C.byref(v), C.byref(ow), C.byref(oh), C.byref(nb))
    return rc, ow.value, oh.value, nb.value


@pytest.mark.parametrize("d", [1, 2, 3, 7])
@pytest.mark.parametrize("fmt,bpp", [(GMS_VIEW_GREY8, 1), (GMS_VIEW_PACKED32, 4)])
def test_view_size_exact_and_ragged(d, fmt, bpp):
    for (w, h) in [(42, 84), (37, 29), (1, 1), (7, 6), (2048, 2048)]:          # 42 x 84: exact for 1, 2, 3, 7; the others ragged somewhere
        ow, oh = -(-w // d), -(-h // d)
        assert _size(GmsView(3, 5, w, h, d, GMS_VIEW_LOG, fmt, 0)) == (0, ow, oh, ow * oh * bpp)
    assert (42 % d, 84 % d) == (0, 0) and _size(GmsView(0, 0, 42, 84, d, GMS_VIEW_LIKELIHOOD, fmt, 0))[1:3] == (42 // d, 84 // d)
    # any of the three outputs may be NULL
    assert _lib.load().gms_view_size(C.byref(GmsView(0, 0, 5, 5, d, 0, fmt, 0)), None, None, None) == 0


def test_bad_views_are_reported_not_crashed():
    L = _lib.load()
    assert L.gms_view_size(None, None, None, None) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    good = dict(x0=0, y0=0, w=4, h=4, decimate=1, source=GMS_VIEW_LOG, format=GMS_VIEW_GREY8, filter=0)
    for bad in (dict(w=0), dict(h=0), dict(w=-3), dict(x0=-1), dict(y0=-1), dict(decimate=0), dict(decimate=-2), dict(source=2),
                dict(source=-1), dict(format=2), dict(format=-1)):
        rc, ow, oh, nb = _size(GmsView(**{**good, **bad}))
        assert rc == GMS_ERR_INVALID, bad
        assert (ow, oh, nb) == (-1, -1, -1), "a refused view writes nothing"
    assert _size(GmsView(**good))[0] == 0


def test_view_entry_points_refuse_null_arguments():
    """the handle, the view and the output are checked before anything is touched (the handle of the NULL-view / NULL-output cases is
    a block of zero bytes that is never read)"""
    L = _lib.load()
    v = GmsView(0, 0, 4, 4, 1, GMS_VIEW_LOG, GMS_VIEW_GREY8, 0)
    out = np.zeros(64, np.uint8)
    fake = np.zeros(4096, np.uint8).ctypes.data
    for fn in (L.gms_map_view, L.gms_map_view_dev):
        for args in ((None, 0, C.byref(v), out.ctypes.data), (fake, 0, None, out.ctypes.data), (fake, 0, C.byref(v), None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    for fn in (L.gms_slam_view, L.gms_slam_view_dev):
        for args in ((None, 0, C.byref(v), out.ctypes.data, None), (fake, 0, None, out.ctypes.data, None), (fake, 0, C.byref(v), None, None)):
            assert fn(*args) == GMS_ERR_INVALID and b"null" in L.gms_last_error()
    assert not out.any()


def test_view_symbols_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gridmapslam.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gms_[a-z0-9_]+)\s*\(", src))
    assert set(VIEW_SYMBOLS) <= declared
    assert "typedef struct gms_view" in src and "GMS_VIEW_STRONGEST" in src
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(VIEW_SYMBOLS) <= exported
    L = _lib.load()
    for n in VIEW_SYMBOLS:
        assert getattr(L, n).argtypes is not None, f"{n} has no signature in _lib.py"
    assert C.sizeof(GmsView) == 32


def test_grey_chain_hand_derived():
    """l = 0: invLogOdds = 0.5, value 0.5, 0.5f * 255 = 127.5 -> idx 127, g = (int)(255 * 127 / 256) = (int)126.5 = 126.
    value 1.0: idx 255, g = (int)(255 * 255 / 256) = (int)254.004 = 254 (white is 254).  value 0 and NaN: 0."""
    v = ve.log_values(np.array([0.0, -0.0]))
    assert np.array_equal(v, [0.5, 0.5])
    assert np.array_equal(ve.idx_of_value(v), [127, 127]) and np.array_equal(ve.grey_of_idx(ve.idx_of_value(v)), [126, 126])
    assert ve.idx_of_value(1.0) == 255 and ve.grey_of_idx(np.array(255)) == 254
    assert ve.idx_of_value(0.0) == 0 and ve.grey_of_idx(np.array(0)) == 0
    assert ve.idx_of_value(np.nan) == 0
    assert ve.packed_of_grey(np.array(126)) == 0xFE7E7E7E and ve.packed_of_grey(np.array(0)) == 0xFE000000
    # the library's clamp: Java would throw on these
    assert np.array_equal(ve.idx_of_value([1.5, -0.25, np.inf, -np.inf, 1e300]), [255, 0, 255, 0, 255])
    # saturated log-odds: exp(-40) vanishes beside 1 (value 1.0), 1 / (1 + exp(40)) beside 1 (value 0.0); NaN stays NaN
    assert np.array_equal(ve.idx_of_value(ve.log_values(np.array([40.0, -40.0, np.nan]))), [0, 255, 0])
    # truncation, not rounding: 254.99 / 255 stays 254
    assert ve.idx_of_value(np.float64(np.float32(254.99) / np.float32(255))) == 254
    assert not ve.fragile(np.array([0.5, 1.0, 0.0, np.nan, 128.0 / 255.0])).any()
    # fragile: a double half way between the two neighbouring floats on either side of an idx step (its float rounding decides idx)
    f = np.float32(128) / np.float32(255)
    while ve.idx_of_value(np.float64(f)) >= 128:
        f = np.nextafter(f, np.float32(0))
    g = np.nextafter(f, np.float32(1))
    assert (ve.idx_of_value(np.float64(f)), ve.idx_of_value(np.float64(g))) == (127, 128)
    assert ve.fragile(np.array([(np.float64(f) + np.float64(g)) / 2])).all()


def test_expected_image_decimation():
    """a one-cell wall survives an overview: min idx in the log view, max idx in the likelihood view; ragged last row and column"""
    idx = np.full((5, 7), 127, np.int32)
    idx[3, 6] = 0                                      # one occupied cell (dark in the log view)
    img = ve.expect(idx, (0, 0, 7, 5), 3, False, False)
    assert img.shape == (2, 3) and img[1, 2] == 0 and (np.delete(img.reshape(-1), 5) == 126).all()
    lik = np.zeros((5, 7), np.int32)
    lik[4, 0] = 255
    img = ve.expect(lik, (0, 0, 7, 5), 3, True, True)
    assert img.dtype == np.uint32 and img[1, 0] == 0xFEFEFEFE and (np.delete(img.reshape(-1), 3) == 0xFE000000).all()
    assert np.array_equal(ve.expect(idx, (6, 3, 1, 1), 8, False, False), [[0]])
