"""The batched entry points of the reference-shape filter (gms_slam_update_batch[_dev], gms_slam_resample_maps[_if]_batch) refuse a
NULL handle or a NULL required argument before they touch a device: no GPU needed."""
import ctypes as C

import numpy as np

from gridmap_slam_robot_amd import _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID


def test_null_handle_and_arguments_are_refused():
    L = _lib.load()
    beams = np.zeros((2, 4), dtype=_lib.BEAM_DTYPE)
    odo, seeds, sm = np.zeros((2, 2)), np.zeros(2, np.uint64), np.ones(2, np.int32)
    r01 = np.full(2, 0.5)
    for fn in (L.gms_slam_update_batch, L.gms_slam_update_batch_dev):
        assert fn(None, beams.ctypes.data, 4, None, odo.ctypes.data, seeds.ctypes.data, sm.ctypes.data, 0, None) == GMS_ERR_INVALID
        assert b"null" in L.gms_last_error()
    assert L.gms_slam_resample_maps_batch(None, r01.ctypes.data, None, None) == GMS_ERR_INVALID
    assert L.gms_slam_resample_maps_if_batch(None, r01.ctypes.data, 0.5) == GMS_ERR_INVALID
    assert b"null" in L.gms_last_error()


def test_create_refuses_filter_counts_out_of_range():
    L = _lib.load()
    p = _lib.GmsParams()
    _lib.check(L.gms_params_default(C.byref(p), 3.2, 3.2, 0.05, -1.6, -1.6))
    h = C.c_void_p()
    for n_maps, n in ((0, 8), (1025, 8), (2, 40000)):
        p.n_maps = n_maps
        assert L.gms_slam_create(C.byref(p), n, C.byref(h)) == GMS_ERR_INVALID
        assert not h.value
    p.n_maps = 2
    assert L.gms_slam_create_shard(C.byref(p), 256, 0, 512, C.byref(h)) == GMS_ERR_INVALID
    assert b"n_maps" in L.gms_last_error()
