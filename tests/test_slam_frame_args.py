"""The frame entry points of the reference-shape filter (gms_slam_frame_per_particle, gms_slam_frame_batch) refuse a NULL handle or
a NULL required array before they touch a device or the handle: no GPU needed.  (The handle of the NULL-array cases is a block of zero
bytes that is never read: the arrays are checked first.)"""
import numpy as np

from gridmap_slam_robot_amd import _lib
from gridmap_slam_robot_amd._lib import GMS_ERR_INVALID


def _refused(L, rc):
    assert rc == GMS_ERR_INVALID
    assert b"null" in L.gms_last_error()


def test_scalar_frame_refuses_null_handle_and_arrays():
    L = _lib.load()
    a, d, h = np.zeros(4), np.ones(4), np.ones(4, np.uint8)
    fake = np.zeros(4096, np.uint8).ctypes.data
    _refused(L, L.gms_slam_frame_per_particle(None, a.ctypes.data, d.ctypes.data, h.ctypes.data, 4, 0.01, 0.0, 1, 0, 0.5, 0.5, None))
    for k in range(3):
        args = [a.ctypes.data, d.ctypes.data, h.ctypes.data]
        args[k] = None
        _refused(L, L.gms_slam_frame_per_particle(fake, *args, 4, 0.01, 0.0, 1, 0, 0.5, 0.5, None))


def test_batch_frame_refuses_null_handle_and_arrays():
    L = _lib.load()
    a, d, h = np.zeros((2, 4)), np.ones((2, 4)), np.ones((2, 4), np.uint8)
    odo, seeds, r01 = np.zeros((2, 2)), np.zeros(2, np.uint64), np.full(2, 0.5)
    fake = np.zeros(4096, np.uint8).ctypes.data
    req = [a.ctypes.data, d.ctypes.data, h.ctypes.data, odo.ctypes.data, seeds.ctypes.data, r01.ctypes.data]

    def call(handle, p):
        return L.gms_slam_frame_batch(handle, p[0], p[1], p[2], 4, None, p[3], p[4], 0, p[5], 0.5, None)

    _refused(L, call(None, req))
    for k in range(len(req)):
        p = list(req)
        p[k] = None
        _refused(L, call(fake, p))


def test_last_beams_refuses_null_arguments():
    L = _lib.load()
    _refused(L, L.gms_slam_last_beams(None, 0, None, 0, None))
