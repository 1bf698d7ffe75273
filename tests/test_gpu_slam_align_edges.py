"""Per-particle scan alignment (k_slam_align, gms_slam_align.hip) at the edges of its own code, against the restatement applied per
particle to the oracle's field of that particle's logData (tests/test_gpu_slam_align.py::_expect): poses as float bit patterns, record
integers and doubles with array_equal -- the device is only ever compared for equality.  The cases and what each of them reaches come
from tests/_slam_align_edge_cases.py and are held to their claims, without a device, in tests/test_slam_align_edge_inputs.py.

Every stand-alone call is also checked to leave the weights, logData and likelihoodData as they were, and to have taken the form of the
field (planes / memory) that the launcher's gate, restated in the case builders, says."""
import numpy as np
import pytest

import _align_expect as ax
import _slam_align_edge_cases as ec
from gridmap_slam_robot_amd import SLAMParticleMaps
from gridmap_slam_robot_amd._lib import GMS_SLAM_ALIGN_MEMORY, GMS_SLAM_ALIGN_PLANES

from test_gpu_slam_align import FORM_ENV, _same_handles, _state

pytestmark = pytest.mark.gpu
FORM_CODE = {"planes": GMS_SLAM_ALIGN_PLANES, "memory": GMS_SLAM_ALIGN_MEMORY}
FORM_NAME = {v: k for k, v in FORM_CODE.items()}
TWO_FORMS = ("planes", "memory")


def _bring(case, form, monkeypatch):
    """a fresh handle taken through the case's steps"""
    for k, v in FORM_ENV[form].items():
        monkeypatch.setenv(k, v)
    W, H = case.size
    dev = SLAMParticleMaps(W, H, ec.RES, case.origin, num_particles=case.N, max_beams=case.max_beams,
                           kernel=None if case.taps is None else list(case.taps))
    assert (dev.W, dev.H) == (case.g.W, case.g.H)
    for s in case.steps:
        if s[0] == "update":
            dev.set_poses(s[1])
            dev.update(s[2], None)
        elif s[0] == "upload":
            for i, log in enumerate(s[1]):
                dev.set_map(i, log=log)
        elif s[0] == "weights":
            dev.pf.set_weights(s[1])
        elif s[0] == "resample":
            idx, _ = dev.resample(s[1], want_indices=True)
            assert np.array_equal(idx, s[2]), f"{case.name}: the draw {s[1]} sits on a rounding boundary; pick another"
        elif s[0] == "reset":
            dev.reset()
        else:
            raise AssertionError(s[0])
    return dev


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _call(dev, case, k, form):
    """call k of the case on the handle: the form taken, the result against the restatement, and nothing else changed.  Returns the
    records"""
    c = case.calls[k]
    where = f"{case.name}: {c.label} ({form})"
    dev.set_poses(c.P)
    _, w0, log0, lik0 = _state(dev)
    rec = dev.align(c.z, c.prm, records=True)
    expected = case.form(len(c.z), eager=form == "no_planes", forced_memory=form == "memory")
    reported = FORM_NAME.get(dev.align_form(), dev.align_form())
    assert reported == expected, f"{where}: B = {len(c.z)}: the gate says {expected}, the launch reports {reported}"
    Pd, w1, log1, lik1 = _state(dev)
    ax.same((Pd, rec), case.want[k], where)
    assert _same_bytes(w0, w1) and _same_bytes(log0, log1) and _same_bytes(lik0, lik1), f"{where}: no weight and no map may change"
    return rec


def _run(case, form, monkeypatch):
    dev = _bring(case, form, monkeypatch)
    for k in range(len(case.calls)):
        _call(dev, case, k, form)
    dev.close()


def _inside_update(case, form, monkeypatch):
    """a.set_align(p); a.update(z) == b.align(z, p); b.update(z), and last_align() == the stand-alone records == the restatement's"""
    a, b = _bring(case, form, monkeypatch), _bring(case, form, monkeypatch)
    c = case.calls[0]
    a.set_align(c.prm)
    a.set_poses(c.P); b.set_poses(c.P)
    a.update(c.z, None)
    rec = b.align(c.z, c.prm, records=True)
    Pb = b.get_particles()[0]
    b.update(c.z, None)
    _same_handles(a, b, f"{case.name} ({form}): the aligned update")
    got = a.last_align()
    assert got.tobytes() == rec.tobytes(), f"{case.name} ({form}): last_align"
    ax.same((Pb, got), case.want[0], f"{case.name} ({form}): the aligned update's records")
    assert np.array_equal(ax.bits(a.get_particles()[0]), ax.bits(case.want[0][0]))
    a.close(); b.close()


# ---- blur widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("name", ec.TAP_CASES)
def test_blur_widths(name, form, monkeypatch):
    """1, 3, 13 and 15 taps in the plain and in the literal form of the on-demand sums (fifteen taps: all sixteen lanes of a group, the
    shuffle source grp + 15, a window of 30 bits behind a shift by 30); corner beams whose windows start in word -1 and end in the
    spare word"""
    _run(ec.tap_case(name), form, monkeypatch)


@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("name", ["fifteen_taps", "fifteen_taps_literal_tiny"])
def test_blur_widths_inside_update(name, form, monkeypatch):
    _inside_update(ec.tap_case(name), form, monkeypatch)


# ---- narrower and lower than the blur ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("shape,kernel", ec.NARROW_CASES)
def test_maps_narrower_and_lower_than_fifteen_taps(shape, kernel, form, monkeypatch):
    """9 x 33: both column clips bind in one window; 33 x 9: rows outside the map above and below one end point; 9 x 9: all of it"""
    _run(ec.narrow_case(shape, kernel), form, monkeypatch)


# ---- planes written from uploaded logData ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["planes", "memory", "no_planes"])
@pytest.mark.parametrize("shape,stage", ec.UPLOAD_CASES)
def test_uploaded_maps(shape, stage, form, monkeypatch):
    """k_slam_codes_from_log's planes: 0.0, -0.0, NaN, the smallest subnormals of either sign and the infinities in logData, a partly
    filled tail word (51 x 67) and a full one with the spare word directly behind (80 x 80); behind a resample() draw; behind reset()"""
    _run(ec.upload_case(shape, stage), form, monkeypatch)


@pytest.mark.parametrize("form", ["planes", "memory", "no_planes"])
@pytest.mark.parametrize("shape", list(ec.UPLOAD_SHAPES))
def test_uploaded_maps_inside_update(shape, form, monkeypatch):
    _inside_update(ec.upload_case(shape, "uploaded"), form, monkeypatch)


# ---- the stopping rules of the workgroup-uniform loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("name", ec.STOP_CASES)
def test_stopping_rules(name, form, monkeypatch):
    """status 1 after one step; status 3 on a map never observed and on either side of a computed determinant; clamps that bind; 64
    iterations; particles of one launch that stop at different evaluations"""
    _run(ec.stop_case(name), form, monkeypatch)


@pytest.mark.parametrize("form", TWO_FORMS)
def test_k_iterations_equal_k_chained_calls(form, monkeypatch):
    case = ec.chain_case()
    c = case.calls[0]
    dev = _bring(case, form, monkeypatch)
    whole = _call(dev, case, 0, form)
    whole_p = dev.get_particles()[0]
    one = dict(c.prm, iters=1)
    cur, done, stopped, final = c.P.copy(), np.zeros(case.N, np.int32), np.zeros(case.N, bool), c.P.copy()
    for _ in range(ec.CHAIN_K):
        dev.set_poses(cur)
        rec = dev.align(c.z, one, records=True)
        nxt = dev.get_particles()[0]
        live = ~stopped
        final[live] = nxt[live]
        done[live] += rec["iters_done"][live]
        stopped |= rec["status"] != 0
        cur = nxt
    assert np.array_equal(ax.bits(whole_p), ax.bits(final)) and np.array_equal(whole["iters_done"], done)
    assert np.array_equal(whole["status"] != 0, stopped) and stopped.any() and not stopped.all()
    dev.close()


# ---- beams -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("B", ec.BEAM_COUNTS)
def test_scans_of_one_pass_of_sixteen_beams_more_or_less(B, form, monkeypatch):
    _run(ec.beam_count_case(B), form, monkeypatch)


@pytest.mark.parametrize("form", TWO_FORMS)
def test_non_finite_beams_that_hit_take_no_part(form, monkeypatch):
    _run(ec.non_finite_case(), form, monkeypatch)


# ---- the gate between the forms and the opt-in to dynamic LDS ------------------------------------------------------------------------------
def test_lds_gate_and_the_later_opt_in():
    """314 x 313 cells, the largest plane that is kept.  One handle: 72 beams (a small grant of dynamic LDS), 2816 beams (the planes
    form at 159 744 bytes: the launcher opts in again), 72 beams, 2817 beams (padded to 2824: behind the gate, the memory form)"""
    case = ec.gate_case()
    dev = _bring(case, "planes", None)
    for k in range(len(case.calls)):
        _call(dev, case, k, "planes")
    dev.close()


def test_a_plane_too_large_to_keep_takes_the_memory_form():
    case = ec.no_planes_case()
    dev = _bring(case, "planes", None)
    _call(dev, case, 0, "planes")
    dev.close()


# ---- an origin far from zero ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", TWO_FORMS)
@pytest.mark.parametrize("name", list(ec.FAR_ORIGINS))
def test_far_origins(name, form, monkeypatch):
    _run(ec.far_case(name), form, monkeypatch)
