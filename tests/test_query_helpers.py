"""The binding's shared request helpers, as far as they work without a device or a handle: the one tensor check refuses a tensor on
the host, the one shown-particle rule resolves `which`, the one rectangle default covers the whole map."""
import pytest

from gridmap_slam_robot_amd import _lib
from gridmap_slam_robot_amd.gridmap import _device_ptr, _locate_args, _obstacles, _rect, _shown_ptr, _which


def test_a_host_tensor_is_refused_and_an_omitted_output_passes():
    import torch
    t = torch.zeros(8, dtype=torch.int32)
    for kw in ({}, {"nbytes": 4}, {"itemsize": 4, "contiguous": False}, {"itemsize": 4, "multiple": 2}, {"optional": True}):
        with pytest.raises(ValueError, match="view: out"):
            _device_ptr("view", "out", t, **kw)
    with pytest.raises(ValueError, match="reach: shown_out"):
        _shown_ptr("reach", t)
    with pytest.raises(ValueError):
        _device_ptr("view", "out", None)
    with pytest.raises(ValueError):
        _device_ptr("view", "out", [0] * 8)
    assert _device_ptr("view", "out", None, optional=True) is None and _shown_ptr("view", None) is None


def test_which_is_resolved_in_one_place():
    assert _which("view", 5) == 5 and _which("view", -3) == -3
    assert _which("gain", "strongest") == _lib.GMS_VIEW_STRONGEST == _which("cast", "strongest", allow_all=True)
    assert _which("cast", "all", allow_all=True) == _lib.GMS_CAST_ALL
    for who, which, kw in (("view", "all", {}), ("view", "weakest", {}), ("cast", "weakest", {"allow_all": True}), ("trajectory", "", {})):
        with pytest.raises(ValueError, match=who + ": which"):
            _which(who, which, **kw)


def test_the_rectangle_default_and_the_obstacle_word():
    assert _rect(48, 40, None) == (0, 0, 48, 40) and _rect(48, 40, [3.0, 2, 41, 35]) == (3, 2, 41, 35)
    assert (_obstacles(True), _obstacles(False)) == (_lib.GMS_CLEAR_NOT_FREE, _lib.GMS_CLEAR_OCCUPIED)
    lc = _locate_args(48, 40, None, (4, 8), 1, True, 2, 5, True, filter=1)
    assert [getattr(lc, n) for n, _ in lc._fields_][:7] == [0, 0, 48, 40, 4, 1, _lib.GMS_CLEAR_NOT_FREE]
