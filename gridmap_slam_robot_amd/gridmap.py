"""Host-side mirror of the reference's GridMap / ParticleFilter / SLAM class surface, over the C-ABI.

Method names and argument meaning follow the Java classes (J/ = java/GridMapGL/src/main/java/com/
fmsz/gridmapgl/ in the reference tree):

  GridMap          J/slam/GridMap.java:47-432   (geometry + GridMapData; one handle holds both)
  Observation      J/slam/Observation.java:29-106
  ParticleFilter   J/slam/ParticleFilter.java:19-84  (resample semantics of SLAM.resample)
  SLAM             J/slam/SLAM.java:26-204

Everything that computes runs in libgridmapslam.so on the GPU; this file only marshals.
snake_case names are primary, the Java camelCase names are kept as aliases.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import BEAM_DTYPE, CAST_DTYPE, GmsParams, GmsPfStats, check, load, ptr

__all__ = ["GridMap", "Observation", "ParticleFilter", "SLAM", "Pose", "scan_residual", "clearance_metres", "reach_metres", "frontier_centroids",
           "cells_of_poses", "descend", "route_points", "mode_estimate", "strongest_mode", "AlignParams", "align_covariance", "warp_agreement", "map_as_scan",
           "census_entropy", "census_outliers", "site_cells", "site_vectors", "skeleton_cells"]


def Pose(x: float, y: float, theta: float) -> np.ndarray:
    """Pose{float x, y, theta} (J/slam/Pose.java:21-35)."""
    return np.array([x, y, theta], dtype=np.float32)


class Observation:
    """One LIDAR revolution (J/slam/Observation.java)."""

    def __init__(self, beams: Optional[np.ndarray] = None):
        self.beams = np.zeros(0, dtype=BEAM_DTYPE) if beams is None else np.ascontiguousarray(beams, dtype=BEAM_DTYPE)

    @staticmethod
    def from_polar(angles, distances, hits) -> "Observation":
        """Measurement(angle, distance, wasHit): localX = distance * cos(angle) (Observation.java:44-51)."""
        angles = np.asarray(angles, dtype=np.float64)
        distances = np.asarray(distances, dtype=np.float64)
        b = np.zeros(angles.shape, dtype=BEAM_DTYPE)
        # math.cos per element: the same libm the oracle uses (numpy's SIMD cos may differ by an ulp)
        b["local_x"] = distances * np.array([math.cos(a) for a in angles.ravel()]).reshape(angles.shape)
        b["local_y"] = distances * np.array([math.sin(a) for a in angles.ravel()]).reshape(angles.shape)
        b["distance"] = distances
        b["hit"] = np.asarray(hits).astype(np.uint8)
        return Observation(b)

    @staticmethod
    def from_local(x, y, hits) -> "Observation":
        """Measurement(x, y, wasHit, dummy) (Observation.java:69-76)."""
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        b = np.zeros(x.shape, dtype=BEAM_DTYPE)
        b["local_x"] = x
        b["local_y"] = y
        b["distance"] = np.sqrt(x * x + y * y)
        b["hit"] = np.asarray(hits).astype(np.uint8)
        return Observation(b)

    def getNumberOfMeasurements(self) -> int:
        return int(self.beams.shape[-1])

    def __len__(self) -> int:
        return self.getNumberOfMeasurements()


def _device_ptr(who: str, what: str, t, nbytes: int = 0, itemsize: Optional[int] = None, multiple: int = 1, contiguous: bool = True,
                optional: bool = False):
    """The device address (a c_void_p) of a caller's torch tensor t, argument `what` of the query `who`: on the device, contiguous
    unless contiguous=False, of at least nbytes bytes, its elements of itemsize bytes (None: any) and their number a multiple of
    `multiple`.  optional: None stands for an omitted output and passes through.  ValueError otherwise: the one check of them all."""
    if t is None and optional:
        return None
    if not getattr(t, "is_cuda", False) or (contiguous and not t.is_contiguous()):
        raise ValueError(f"{who}: {what} must be a {'contiguous ' if contiguous else ''}torch tensor on the device")
    if (itemsize is not None and t.element_size() != itemsize) or t.numel() % multiple:
        raise ValueError(f"{who}: {what} must hold {itemsize or t.element_size()}-byte elements, a multiple of {multiple} of them")
    if t.numel() * t.element_size() < nbytes:
        raise ValueError(f"{who}: {what} holds {t.numel() * t.element_size()} bytes, {nbytes} are needed")
    return C.c_void_p(int(t.data_ptr()))


def _shown_ptr(who: str, shown_out):
    """the device address of the int32 word that receives the index of the particle shown (None: not wanted)"""
    return _device_ptr(who, "shown_out", shown_out, 4, itemsize=4, contiguous=False, optional=True)


def _which(who: str, which, allow_all: bool = False) -> int:
    """the particle a per-particle query shows: an index passes through, "strongest" is GMS_VIEW_STRONGEST (picked on the device) and,
    where the query allows it, "all" GMS_CAST_ALL"""
    if not isinstance(which, str):
        return int(which)
    if which == "strongest":
        return _lib.GMS_VIEW_STRONGEST
    if allow_all and which == "all":
        return _lib.GMS_CAST_ALL
    raise ValueError(f'{who}: which must be a particle index or "strongest"' + (' or "all"' if allow_all else ""))


def _rect(W: int, H: int, rect):
    """rect = (x0, y0, w, h) in cells of a W x H map; None: the whole map"""
    return (0, 0, W, H) if rect is None else tuple(int(c) for c in rect)


def _obstacles(not_free: bool) -> int:
    """the obstacle-mode word: every cell that is not known free, or the occupied ones alone"""
    return _lib.GMS_CLEAR_NOT_FREE if not_free else _lib.GMS_CLEAR_OCCUPIED


def _sized(size_fn, request):
    """(request, output shape (oh, ow), bytes) of a field request, as the library's gms_*_size sizes it"""
    ow, oh, nbytes = C.c_int32(), C.c_int32(), C.c_int64()
    check(size_fn(C.byref(request), C.byref(ow), C.byref(oh), C.byref(nbytes)))
    return request, (oh.value, ow.value), nbytes.value


def world_rect_to_cells(grid_map, center, size):
    """The cell rectangle (x0, y0, w, h) a world rectangle -- centre and size in metres -- covers on grid_map, clamped to the map.
    A world coordinate becomes a cell as the reference's lookups do it (J/slam/GridMap.java:273-276): (int)((x - position) /
    resolution) in float arithmetic, truncated toward zero.  ValueError where the rectangle misses the map."""
    f = np.float32
    res = f(grid_map.params.resolution)
    out = []
    for c, sz, pos, n in ((center[0], size[0], grid_map.params.pos_x, grid_map.W), (center[1], size[1], grid_map.params.pos_y, grid_map.H)):
        half = f(sz) / f(2)
        lo_w, hi_w = (f(c) - half - f(pos)) / res, (f(c) + half - f(pos)) / res
        if not (hi_w >= 0 and lo_w < n):                # (also refuses NaN)
            raise ValueError("world_rect_to_cells: the rectangle lies outside the map")
        lo, hi = max(int(lo_w), 0), min(int(min(hi_w, f(n))), n - 1)
        out.append((lo, hi - lo + 1))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _beams_of(obs) -> np.ndarray:
    b = obs.beams if isinstance(obs, Observation) else obs
    return np.ascontiguousarray(b, dtype=BEAM_DTYPE)


RESIDUAL_AGREE, RESIDUAL_MEASURED_SHORTER, RESIDUAL_MEASURED_LONGER, RESIDUAL_NO_PREDICTION = 0, 1, 2, 3


def scan_residual(measured_beams, cast, resolution: float, hit_tolerance: float) -> np.ndarray:
    """Holds a measured scan against the scan predicted for the same beams (cast = the gms_cast_hit records of GridMap.cast /
    SLAMParticleMaps.cast of measured_beams as probes): one uint8 class per beam.  Pure numpy, float32 like the sensor model.

    With m = float32(distance) / float32(resolution), the beam's measuredDistance in grid units (GridMap.java:188), r = cast.range and
    t = float32(hit_tolerance) / 2, the band inverseSensorModel puts around a measurement (SensorModel.java:35-40):

      RESIDUAL_NO_PREDICTION (3)     cast.step < 0 and the beam hit: the map has no occupied cell on the beam's walk, there is nothing to
                                     hold the return against (an unmapped or free stretch)
      RESIDUAL_AGREE (0)             both hit and |m - r| <= t; or the beam missed and the walk found nothing either
      RESIDUAL_MEASURED_SHORTER (1)  the beam hit and m < r - t: something is there that the map lacks
      RESIDUAL_MEASURED_LONGER (2)   m > r + t, or the beam missed although the walk found a wall: the map has a wall the beam passed

    A hit beam whose distance is NaN satisfies none of the three comparisons and stays RESIDUAL_NO_PREDICTION."""
    b = _beams_of(measured_beams)
    c = np.asarray(cast)
    if b.shape != c.shape:
        raise ValueError(f"scan_residual: {b.shape} beams against {c.shape} predictions")
    f = np.float32
    m = b["distance"].astype(f) / f(resolution)
    r = c["range"].astype(f)
    t = f(hit_tolerance) / f(2)
    hit, pred = b["hit"] != 0, c["step"] >= 0
    out = np.full(b.shape, RESIDUAL_NO_PREDICTION, dtype=np.uint8)
    both = hit & pred
    out[both & (np.abs(m - r) <= t)] = RESIDUAL_AGREE
    out[both & (m < r - t)] = RESIDUAL_MEASURED_SHORTER
    out[both & (m > r + t)] = RESIDUAL_MEASURED_LONGER
    out[~hit & ~pred] = RESIDUAL_AGREE
    out[~hit & pred] = RESIDUAL_MEASURED_LONGER
    return out


def probe_fan(n: int, range_m: float, fov: float = 2 * math.pi) -> np.ndarray:
    """n probes of length range_m (metres), evenly spaced fov / n apart and centred on the heading -- probe i at the angle
    (i - (n - 1) / 2) * fov / n in the robot's frame -- as BEAM_DTYPE [n] (hit = 0): what cast() and gain() take.  The default
    fov is the full circle."""
    if n < 1:
        raise ValueError("probe_fan: n must be at least 1")
    a = (np.arange(n, dtype=np.float64) - (n - 1) / 2) * (float(fov) / n)
    b = np.zeros(n, dtype=BEAM_DTYPE)
    b["local_x"] = float(range_m) * np.cos(a)
    b["local_y"] = float(range_m) * np.sin(a)
    b["distance"] = float(range_m)
    return b


def locate_offsets(scan, n_theta: int, resolution: float, theta0: float = 0.0, dtheta: Optional[float] = None) -> np.ndarray:
    """The offset table of a scan for locate() (gridmapslam.h "global scan matching", gms_locate_offsets; no device needed): int16
    [n_theta][B][2], entry (k, b) the end cell (dx, dy) of beam b relative to the pose's cell under the heading theta0 + k * dtheta
    -- dtheta defaults to a full turn over n_theta --, the pose at the centre of its cell.  Beams that missed, non-finite ones and
    those beyond 4095 cells become the pair (GMS_LOCATE_SKIP, GMS_LOCATE_SKIP) and do not count."""
    b = _beams_of(scan).reshape(-1)
    n_theta = int(n_theta)
    if dtheta is None:
        dtheta = 2.0 * math.pi / max(n_theta, 1)
    out = np.empty((max(n_theta, 0), len(b), 2), dtype=np.int16)
    check(load().gms_locate_offsets(ptr(b), len(b), float(theta0), float(dtheta), n_theta, float(resolution), ptr(out)))
    return out


def locate_poses(records, position, resolution: float, theta0: float = 0.0, dtheta: Optional[float] = None, n_theta: Optional[int] = None) -> np.ndarray:
    """locate()'s records as poses, float64 [n][3]: x = position.x + (record.x + 0.5) * resolution, y likewise -- the centre of the
    cell --, theta = theta0 + k * dtheta (dtheta, or a full turn over n_theta: what locate_offsets was given)."""
    r = np.asarray(records)
    if dtheta is None:
        if n_theta is None:
            raise ValueError("locate_poses: dtheta or n_theta is required")
        dtheta = 2.0 * math.pi / int(n_theta)
    out = np.empty((len(r), 3), dtype=np.float64)
    out[:, 0] = float(position[0]) + (r["x"].astype(np.float64) + 0.5) * float(resolution)
    out[:, 1] = float(position[1]) + (r["y"].astype(np.float64) + 0.5) * float(resolution)
    out[:, 2] = float(theta0) + r["k"].astype(np.float64) * float(dtheta)
    return out


def locate_peaks(records, radius: int, k_radius: Optional[int] = None, n_theta: Optional[int] = None) -> np.ndarray:
    """Greedy non-maximum suppression over locate()'s records (host code): the best `cap` records cluster around each peak, so walk
    them in their order -- best first -- and keep a record unless a kept one lies within `radius` cells of it along both axes (and,
    with k_radius, within k_radius heading indices; n_theta: the headings wrap around a full turn).  Returns the kept records."""
    r = np.asarray(records)
    keep = []
    for i in range(len(r)):
        x, y, k = int(r["x"][i]), int(r["y"][i]), int(r["k"][i])
        for j in keep:
            if abs(int(r["x"][j]) - x) > radius or abs(int(r["y"][j]) - y) > radius:
                continue
            if k_radius is not None:
                dk = abs(int(r["k"][j]) - k)
                if n_theta is not None:
                    dk = min(dk, int(n_theta) - dk)
                if dk > k_radius:
                    continue
            break
        else:
            keep.append(i)
    return r[keep]


def _locate_args(W: int, H: int, rect, offsets_shape, tol: int, not_free: bool, min_score: int, cap: int, free_only: bool, filter: int = 0):
    """the gms_locate of a request on a W x H map; rect = (x0, y0, w, h) in cells, None: the whole map; offsets_shape = (n_theta, B)"""
    return _lib.GmsLocate(*_rect(W, H, rect), int(offsets_shape[0]), int(tol), _obstacles(not_free), int(min_score), int(cap), int(bool(free_only)),
                          int(filter), 0)


def _locate_table(offsets) -> np.ndarray:
    """offsets as the int16 [n_theta][B][2] table the library takes"""
    a = np.ascontiguousarray(offsets, dtype=np.int16)
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError(f"locate: offsets must be [n_theta][B][2] (dx, dy) cells, not {a.shape}")
    return a


def scatter_slots(n: int, fraction: float):
    """(first, count) of the slots a recovery step replaces by fresh uniform samples after a resample: the LAST round(fraction * n)
    slots of a filter of n -- after resample() a slot's index says nothing about its particle, so any block serves --, at least one
    while fraction > 0, never all n while fraction < 1.  (n, 0) for fraction <= 0: nothing to scatter.  What
    ParticleFilter.scatter(first=..., count=...) takes."""
    if n < 1:
        raise ValueError("scatter_slots: n must be at least 1")
    if not fraction > 0:
        return n, 0
    count = n if fraction >= 1 else min(max(int(round(fraction * n)), 1), max(n - 1, 1))
    return n - count, count


def beam_model_factors(resolution: float, behind: int, ahead: int, sigma: float, z_hit: float = 0.8, z_short: float = 0.1, z_rand: float = 0.05,
                       z_miss: float = 0.9) -> np.ndarray:
    """factors [2][T], T = behind + ahead + 2, for ParticleFilter.score_beams: the usual mixture of a ray-cast beam model, pure numpy
    float64.  Entry k < T - 1 belongs to the residual d = k - behind in walk steps (the map's first wall d steps behind the measured
    end point; negative: in front of it; d = -behind also stands for every wall further in front), entry T - 1 to "the walk found no
    wall".  With r = d * resolution:

      row 1 (beams that hit)     z_hit * exp(-0.5 * (r / sigma)^2)  +  z_short where d > 0  +  z_rand;      none: z_short + z_rand
      row 0 (beams that missed)  z_rand for every d (the map has a wall where the beam saw none);           none: z_miss + z_rand

    i.e. a Gaussian around agreement, a constant short-reading term where the beam ended in front of the map's wall (d > 0) or of
    anything the walk could reach (none), a uniform floor everywhere, and a high value where a beam that saw nothing meets a map
    that holds nothing.  The entries are weights, not densities: only their ratios matter once the filter normalises.
    A walk step is one cell along x or y, so it is between resolution / sqrt(2) (a diagonal ray) and resolution (an axis-parallel
    one) of range: sigma and the reach of behind / ahead in metres are direction dependent by that factor.  z_rand must be > 0 (every
    entry must be, or gms_pf_score_beams refuses the table)."""
    behind, ahead = int(behind), int(ahead)
    if not (0 <= behind <= 255 and 0 <= ahead <= 255):
        raise ValueError("beam_model_factors: 0 <= behind, ahead <= 255")
    if not (sigma > 0 and resolution > 0 and z_rand > 0 and z_hit >= 0 and z_short >= 0 and z_miss >= 0):
        raise ValueError("beam_model_factors: sigma, resolution and z_rand must be > 0, the other terms >= 0")
    T = behind + ahead + 2
    d = np.arange(-behind, ahead + 1, dtype=np.float64)
    r = d * float(resolution)
    f = np.empty((2, T), dtype=np.float64)
    f[1, :T - 1] = float(z_hit) * np.exp(-0.5 * (r / float(sigma)) ** 2) + np.where(d > 0, float(z_short), 0.0) + float(z_rand)
    f[1, T - 1] = float(z_short) + float(z_rand)
    f[0, :T - 1] = float(z_rand)
    f[0, T - 1] = float(z_miss) + float(z_rand)
    return f


class AlignParams(_lib.GmsAlignParams):
    """The parameters of align() (gridmapslam.h "continuous scan alignment", gms_align_params): the library's defaults
    (gms_align_params_default: iters 8, damp_t 10, damp_r 1e4, max_t 2 cells, max_r 0.1 rad, eps_t 0.01 cells, eps_r 1e-4 rad, det_min
    1e-6) with the keyword arguments written over them.  check() is gms_align_check: GmsError on a value out of range."""

    def __init__(self, **fields):
        super().__init__()
        check(load().gms_align_params_default(C.byref(self)))
        names = {n for n, _ in self._fields_}
        for k, v in fields.items():
            if k not in names or k == "pad":
                raise TypeError(f"AlignParams: no field {k!r}")
            setattr(self, k, int(v) if k == "iters" else float(v))

    def check(self) -> "AlignParams":
        check(load().gms_align_check(C.byref(self)))
        return self


def _align_params(params) -> _lib.GmsAlignParams:
    if params is None:
        return AlignParams()
    return params if isinstance(params, _lib.GmsAlignParams) else AlignParams(**dict(params))


def align_covariance(records, resolution: float) -> np.ndarray:
    """The covariance of align()'s poses from their records' H, host numpy: float64 [n][3][3] in (metres, metres, radians), the inverse
    of the information matrix H (cells, cells, radians) scaled by the resolution, up to the residuals' variance, which the caller
    knows; NaN where H is singular or not finite."""
    Hs = np.asarray(np.asarray(records)["H"], dtype=np.float64).reshape(-1, 6)
    out = np.full((len(Hs), 3, 3), np.nan)
    scale = np.array([float(resolution), float(resolution), 1.0])
    for i, h in enumerate(Hs):
        A = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])
        if not np.isfinite(A).all():
            continue
        with np.errstate(all="ignore"):
            try:
                inv = np.linalg.inv(A)
            except np.linalg.LinAlgError:
                continue
        if np.isfinite(inv).all() and np.linalg.matrix_rank(A) == 3:
            out[i] = inv * np.outer(scale, scale)
    return out


def clearance_metres(d2, resolution: float) -> np.ndarray:
    """Clearance values (GridMap.clearance / clearance_poses: squared cell distances as uint16) as metres, float64: sqrt(d2) *
    resolution; GMS_CLEAR_FAR (beyond the radius, or no obstacle at all) becomes inf, GMS_CLEAR_OUTSIDE (a pose off the map) nan."""
    a = np.asarray(d2)
    out = np.sqrt(a.astype(np.float64)) * float(resolution)
    out[a == _lib.GMS_CLEAR_FAR] = np.inf
    out[a == _lib.GMS_CLEAR_OUTSIDE] = np.nan
    return out


def site_cells(site, W: int) -> tuple:
    """Sites (GridMap.skeleton's site field or nearest_poses' "site": uint32 oy * W + ox) as cells: (ox, oy, valid), int64, int64 and
    bool arrays of the input's shape.  valid is False, and ox = oy = -1, where the site is GMS_SITE_NONE (no obstacle within the
    radius) or GMS_SITE_OUTSIDE (a pose off the map)."""
    s = np.asarray(site).astype(np.int64)
    valid = (s != _lib.GMS_SITE_NONE) & (s != _lib.GMS_SITE_OUTSIDE)
    return np.where(valid, s % int(W), -1), np.where(valid, s // int(W), -1), valid


def site_vectors(site, x0: int, y0: int, W: int, resolution: float) -> np.ndarray:
    """The metric vector from the centre of every cell of a site field [h][w] of the rectangle at (x0, y0) to the centre of its site,
    float64 [h][w][2] = (dx, dy) in metres: (ox - x, oy - y) * resolution, the map's float resolution widened.  NaN where the cell
    has no site.  The direction away from the nearest wall is its negative."""
    s = np.asarray(site)
    ox, oy, valid = site_cells(s, W)
    ys, xs = np.mgrid[int(y0):int(y0) + s.shape[0], int(x0):int(x0) + s.shape[1]]
    res = np.float64(np.float32(resolution))
    v = np.stack([(ox - xs) * res, (oy - ys) * res], axis=-1)
    v[~valid] = np.nan
    return v


def skeleton_cells(skel) -> tuple:
    """The skeleton cells of a skeleton field (GridMap.skeleton's skel [h][w]: d2 on the skeleton, else 0): (ys, xs, d2), the cells in
    row-major order within the rectangle and their squared clearance in cells; doorways are the local minima of d2 along it."""
    k = np.asarray(skel)
    ys, xs = np.nonzero(k)
    return ys, xs, k[ys, xs]


def _reach_seeds(seeds, who: str = "reach", what: str = "seeds") -> np.ndarray:
    """seeds (route: starts) as the int32 [K][2] (x, y) array the library takes"""
    a = np.ascontiguousarray(seeds, dtype=np.int32)
    if a.ndim == 1 and a.size == 2:
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{who}: {what} must be [K][2] (x, y) cells, not {a.shape}")
    return a


def reach_metres(field, resolution: float) -> np.ndarray:
    """Cost-to-go values (GridMap.reach: uint16, 5 per axis step, 7 per diagonal one) as metres, float64: cost / 5 * resolution;
    GMS_REACH_FAR (blocked, unreachable, or beyond the cap) becomes inf."""
    a = np.asarray(field)
    out = a.astype(np.float64) / _lib.GMS_REACH_AXIS * float(resolution)
    out[a == _lib.GMS_REACH_FAR] = np.inf
    return out


def _rollout_table(arcs) -> np.ndarray:
    """arcs as the ROLLOUT_STEP_DTYPE [K][T] table the library takes: such records, or floats [K][T][4] = (dx, dy, c, s)"""
    a = np.asarray(arcs)
    if a.dtype != _lib.ROLLOUT_STEP_DTYPE:
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError(f"rollout: arcs must be [K][T] steps (dx, dy, c, s), not {a.shape}")
        a = a.view(_lib.ROLLOUT_STEP_DTYPE).reshape(a.shape[:2])
    if a.ndim != 2:
        raise ValueError(f"rollout: arcs must be [K][T] steps, not {a.shape}")
    return np.ascontiguousarray(a)


def rollout_arcs(v, omega, dt: float, T: int) -> np.ndarray:
    """The arc table of K unicycle commands (gms_rollout_arcs, the library's C helper, so that every host gets the same table):
    ROLLOUT_STEP_DTYPE [K][T], step j of command k the pose after (j + 1) * dt seconds at speed v[k] (m/s) and turn rate omega[k]
    (rad/s) in the frame of the start pose; the straight line where |omega| < 1e-9.  What rollout() and rollout_risk() take."""
    vv, ww = np.ascontiguousarray(v, dtype=np.float64).reshape(-1), np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
    if len(vv) != len(ww):
        raise ValueError(f"rollout_arcs: {len(vv)} speeds and {len(ww)} turn rates")
    out = np.empty((len(vv), max(int(T), 0)), dtype=_lib.ROLLOUT_STEP_DTYPE)
    check(load().gms_rollout_arcs(ptr(vv), ptr(ww), len(vv), float(dt), int(T), ptr(out)))
    return out


def footprint_box(length: float, width: float, spacing: float) -> np.ndarray:
    """Outline points of a rectangular robot centred on its origin, length along x and width along y (metres), float32 [F][2]: each
    side divided into ceil(side / spacing) equal parts, the corners once each, counter-clockwise from (-length / 2, -width / 2).  The
    centre is not listed: rollouts always test it.  spacing at most the map's resolution leaves no cell of the outline untested.
    ValueError where that takes more than GMS_ROLLOUT_MAX_F points."""
    if not (length > 0 and width > 0 and spacing > 0):
        raise ValueError("footprint_box: length, width and spacing must be > 0")
    nx, ny = max(int(math.ceil(length / spacing)), 1), max(int(math.ceil(width / spacing)), 1)
    hx, hy = length / 2.0, width / 2.0
    xs, ys = [-hx + length * i / nx for i in range(nx)], [-hy + width * i / ny for i in range(ny)]
    pts = [(x, -hy) for x in xs] + [(hx, y) for y in ys] + [(-x, hy) for x in xs] + [(-hx, -y) for y in ys]
    if len(pts) > _lib.GMS_ROLLOUT_MAX_F:
        raise ValueError(f"footprint_box: {len(pts)} points, at most {_lib.GMS_ROLLOUT_MAX_F} are taken: use a coarser spacing")
    return np.asarray(pts, dtype=np.float32)


def rollout_pick(records, T: Optional[int] = None, min_d2: int = 0, w_cost: float = 1.0, w_clear: float = 0.0) -> int:
    """The index of the best candidate among ONE start pose's rollout records [K], plain numpy, or -1 where none is admissible.
    Admissible: the arc is collision-free over all its steps (first_hit == T; T None: the largest first_hit of the records), the
    footprint does not collide at the start pose, and min_d2 along it is at least `min_d2` (squared cells; GMS_CLEAR_FAR passes).
    The objective, larger is better: -w_cost * best_cost + w_clear * sqrt(min_d2), GMS_REACH_FAR and GMS_CLEAR_FAR taken as their
    values 65535; argmax, ties to the smallest index."""
    r = np.asarray(records).reshape(-1)
    if not len(r):
        return -1
    full = int(r["first_hit"].max()) if T is None else int(T)
    ok = (r["first_hit"] == full) & ((r["flags"] & _lib.GMS_ROLLOUT_START_BLOCKED) == 0) & (r["min_d2"] >= int(min_d2))
    if not ok.any():
        return -1
    score = -float(w_cost) * r["best_cost"].astype(np.float64) + float(w_clear) * np.sqrt(r["min_d2"].astype(np.float64))
    return int(np.argmax(np.where(ok, score, -np.inf)))


_WARP_OPS = {"compare": _lib.GMS_WARP_COMPARE, "replace": _lib.GMS_WARP_REPLACE, "add": _lib.GMS_WARP_ADD, "fill": _lib.GMS_WARP_FILL}


def _warp_request(W: int, H: int, pose, c, s, op, rect, clamp: float) -> _lib.GmsWarp:
    """gms_warp for a destination of W x H cells: pose = (x, y, theta) of the SOURCE map's world frame in the destination's world
    (gms_warp_pose: the host's libm), or -- c and s given -- (x, y) beside that cosine and sine, taken as they are (exact quarter
    turns: c=0, s=1); None: the origin.  op: "compare", "replace", "add", "fill" or a GMS_WARP_* value; checked by gms_warp_check."""
    w = _lib.GmsWarp()
    w.x0, w.y0, w.w, w.h = _rect(W, H, rect)
    w.op = _WARP_OPS[op] if isinstance(op, str) else int(op)
    w.clamp = float(clamp)
    p = (0.0, 0.0, 0.0) if pose is None else tuple(float(v) for v in pose)
    if (c is None) != (s is None):
        raise ValueError("warp: c and s are given together")
    if c is None:
        if len(p) != 3:
            raise ValueError("warp: pose is (x, y, theta)")
        check(load().gms_warp_pose(C.byref(w), p[0], p[1], p[2]))
    else:
        w.tx, w.ty, w.c, w.s = p[0], p[1], float(c), float(s)
    check(load().gms_warp_check(C.byref(w)))
    return w


def _query_warp(src: _Source, dst: "GridMap", mi: int, w: _lib.GmsWarp, stats, stats_out, shown_out, dev: bool) -> tuple:
    """gms_<kind>_warp[_dev]: a particle's source takes (which, filter) in front of the destination, a map's follows it.  Returns
    (stats,) and then what the source appends; stats: a WARP_STATS_DTYPE record, None where not wanted, or -- dev -- stats_out"""
    lead = (*src.lead, src.filter, dst._h, int(mi)) if src.shows else (dst._h, int(mi), *src.lead)
    if dev:
        sp = _device_ptr("warp", "stats_out", stats_out, _lib.WARP_STATS_DTYPE.itemsize, optional=True)
        tail = (_shown_ptr("warp", shown_out),) if src.shows else ()
        check(getattr(load(), f"gms_{src.kind}_warp_dev")(*lead, C.byref(w), sp, *tail))
        return (stats_out, shown_out) if src.shows else (stats_out,)
    rec = np.zeros((), dtype=_lib.WARP_STATS_DTYPE) if stats else None
    shown = C.c_int32(-1)
    tail = (C.byref(shown),) if src.shows else ()
    check(getattr(load(), f"gms_{src.kind}_warp")(*lead, C.byref(w), None if rec is None else ptr(rec), *tail))
    return (rec, int(shown.value)) if src.shows else (rec,)


def warp_agreement(stats) -> dict:
    """What the class-pair counts of a warp (WARP_STATS_DTYPE: pair[destination class][source class], classes 0 unknown, 1 free,
    2 occupied) say about the pose, plain numpy: overlap -- both known --, agree -- free/free plus occupied/occupied --, conflict --
    free/occupied plus occupied/free --, gained -- destination unknown, source known --, outside.  Compare first (op="compare"),
    merge only where conflict is small beside agree: a false merge cannot be taken back."""
    pair = np.asarray(stats["pair"], dtype=np.int64).reshape(3, 3)
    return {"overlap": int(pair[1:, 1:].sum()), "agree": int(pair[1, 1] + pair[2, 2]), "conflict": int(pair[1, 2] + pair[2, 1]),
            "gained": int(pair[0, 1] + pair[0, 2]), "outside": int(np.asarray(stats["n_outside"]).sum())}


def census_entropy(counts, n: int) -> np.ndarray:
    """The per-cell Shannon entropy in bits of the three-way split of a filter's n particles that a census counted (counts [H][W][2]
    = {fr, oc}): H(fr / n, oc / n, (n - fr - oc) / n), 0 where all particles agree, log2(3) where they split evenly.  Plain numpy on
    the host."""
    c = np.asarray(counts).astype(np.float64)
    if c.shape[-1] != 2:
        raise ValueError("census_entropy: counts must be [...][2] = {fr, oc}")
    n = int(n)
    p = np.stack([c[..., 0], c[..., 1], n - c[..., 0] - c[..., 1]], axis=-1) / n
    if n < 1 or (p < 0).any():
        raise ValueError("census_entropy: n must be positive and at least fr + oc in every cell")
    terms = np.zeros_like(p)
    np.log2(p, out=terms, where=p > 0)
    return 0.0 - (p * terms).sum(axis=-1)


def census_outliers(agree) -> np.ndarray:
    """Per particle the cells where it contradicts the consensus of a census (CENSUS_AGREE_DTYPE records: pair[the particle's
    class][the consensus class]): pair[1][2] + pair[2][1], free against occupied plus occupied against free."""
    pair = np.asarray(agree["pair"], dtype=np.int64)
    return pair[..., 1, 2] + pair[..., 2, 1]


def map_as_scan(log, position, resolution: float, max_beams: int = 4096) -> np.ndarray:
    """The occupied cells (logData > 0) of a host logData array [H][W] as gms_beam records: local_x / local_y the cell's centre in
    that map's OWN world -- position + (index + 0.5) * resolution in double, position and resolution as floats, what the warp's
    arithmetic widens --, distance their hypot, hit 1.  More than max_beams cells: every ceil(n / max_beams)-th in index order
    (x + y * W).  The idiom: the pose that other.locate(locate_offsets(scan, ...)) -> locate_poses() -> other.align(scan, poses)
    return for these beams in ANOTHER map is the pose of this map's world frame in that map's world -- it IS the pose of
    other.warp_from(this, pose)."""
    a = np.asarray(log, dtype=np.float64)
    if a.ndim != 2 or max_beams < 1:
        raise ValueError("map_as_scan: log is one map [H][W] and max_beams >= 1")
    idx = np.flatnonzero(a.reshape(-1) > 0)
    if len(idx) > max_beams:
        idx = idx[::-(-len(idx) // int(max_beams))]
    res, px, py = (np.float64(np.float32(v)) for v in (resolution, position[0], position[1]))
    b = np.zeros(len(idx), dtype=BEAM_DTYPE)
    b["local_x"] = px + ((idx % a.shape[1]).astype(np.float64) + 0.5) * res
    b["local_y"] = py + ((idx // a.shape[1]).astype(np.float64) + 0.5) * res
    b["distance"] = np.hypot(b["local_x"], b["local_y"])
    b["hit"] = 1
    return b


def _frontier_cost(cost, W: int, H: int, who: str = "frontiers", what: str = "cost", kind: str = "cost-to-go"):
    """a whole-map field (what reach() or clearance() returns for the full rectangle) as the contiguous uint16 [H][W] the library takes"""
    if cost is None:
        return None
    a = np.asarray(cost)
    if a.shape != (H, W) or a.dtype != np.uint16:
        raise ValueError(f"{who}: {what} must be the whole map's uint16 [{H}][{W}] {kind} field, not {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def frontier_centroids(records) -> np.ndarray:
    """The centroids of frontier regions (GridMap.frontiers' records) in cells, float64 [n][2] = (x, y): sum / count"""
    r = np.asarray(records)
    n = r["count"].astype(np.float64)
    return np.stack([r["sum_x"] / n, r["sum_y"] / n], axis=-1)


def room_centroids(records) -> np.ndarray:
    """The centroids of rooms (GridMap.rooms' room records) in cells, float64 [n][2] = (x, y): sum / count"""
    r = np.asarray(records)
    n = r["count"].astype(np.float64)
    return np.stack([r["sum_x"] / n, r["sum_y"] / n], axis=-1)


def door_points(doors, position, resolution: float) -> np.ndarray:
    """The mean opening position of every door record (GridMap.rooms' doors) in world coordinates, float64 [n][2]: the mean of the
    contact pairs' cell centres, position + (sum / (2 count) + 0.5) * resolution"""
    d = np.asarray(doors)
    n = 2.0 * d["count"].astype(np.float64)
    res = np.float64(np.float32(resolution))
    return np.stack([np.float64(np.float32(position[0])) + (d["sum_x2"] / n + 0.5) * res, np.float64(np.float32(position[1])) + (d["sum_y2"] / n + 0.5) * res], axis=-1)


def rooms_of_cells(labels, cells, x0: int = 0, y0: int = 0) -> np.ndarray:
    """Which room each of cells [n][2] = (x, y) lies in -- a frontier goal, a particle's cell (cells_of_poses) --, from the label field
    GridMap.rooms returns for the rectangle at (x0, y0): uint32 [n], the room's anchor index, GMS_ROOM_NONE for a cell without a room
    or outside the rectangle"""
    lab = np.asarray(labels)
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    x, y = c[:, 0] - int(x0), c[:, 1] - int(y0)
    inside = (x >= 0) & (y >= 0) & (x < lab.shape[1]) & (y < lab.shape[0])
    out = np.full(len(c), _lib.GMS_ROOM_NONE, dtype=np.uint32)
    out[inside] = lab[y[inside], x[inside]]
    return out


def room_graph(rooms, doors, W: Optional[int] = None) -> dict:
    """The rooms' adjacency: {anchor index: {neighbour's anchor index: the door's contact count}}, the labels' values as keys.  With
    W, the map's width in cells, every room of `rooms` is a key (anchor_y * W + anchor_x), a room without a door with an empty
    dict; without it only the rooms that a door names appear."""
    d = np.asarray(doors)
    g = {}
    if W is not None:
        r = np.asarray(rooms)
        g = {int(k): {} for k in (r["anchor_y"].astype(np.int64) * int(W) + r["anchor_x"]).tolist()}
    for a, b, n in zip(d["a"].tolist(), d["b"].tolist(), d["count"].tolist()):
        g.setdefault(a, {})[b] = n
        g.setdefault(b, {})[a] = n
    return g


def _query_rooms(src: "_Source", core: int, inflate: int, not_free: bool, min_core: int, max_cost: int, rect, want, caps, dev=None):
    """want = (labels, depth): which fields the host form returns; caps = (cap_rooms, cap_doors).  dev = (labels, depth, rooms, doors,
    shown_out), torch device tensors or None each: the device form, which returns (n_rooms, n_doors)"""
    q = _lib.GmsRooms(*_rect(src.W, src.H, rect), int(core), int(inflate), _obstacles(not_free), int(min_core), int(max_cost), src.filter)
    ow, oh, lb, db = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    check(load().gms_rooms_size(C.byref(q), C.byref(ow), C.byref(oh), C.byref(lb), C.byref(db)))
    nr, nd = C.c_int32(0), C.c_int32(0)
    if dev is not None:
        labels, depth, rooms, doors, shown_out = dev
        cap_r = 0 if rooms is None else rooms.numel() * rooms.element_size() // _lib.ROOM_DTYPE.itemsize
        cap_d = 0 if doors is None else doors.numel() * doors.element_size() // _lib.DOOR_DTYPE.itemsize
        src.dev("rooms", C.byref(q), _device_ptr("rooms", "labels", labels, lb.value, optional=True), _device_ptr("rooms", "depth", depth, db.value, optional=True),
                _device_ptr("rooms", "rooms", rooms, optional=True), int(cap_r), C.byref(nr), _device_ptr("rooms", "doors", doors, optional=True), int(cap_d),
                C.byref(nd), shown_out=shown_out)
        return int(nr.value), int(nd.value)
    shape = (oh.value, ow.value)
    cap_r, cap_d = int(caps[0]), int(caps[1])
    lab = np.empty(shape, dtype=np.uint32) if want[0] else None
    dep = np.empty(shape, dtype=np.uint16) if want[1] else None
    rooms = np.zeros(cap_r, dtype=_lib.ROOM_DTYPE)
    doors = np.zeros(cap_d, dtype=_lib.DOOR_DTYPE)
    tail = src.host("rooms", C.byref(q), None if lab is None else ptr(lab), None if dep is None else ptr(dep), ptr(rooms) if cap_r else None, cap_r, C.byref(nr),
                    ptr(doors) if cap_d else None, cap_d, C.byref(nd))
    out = {"rooms": rooms[:min(nr.value, cap_r)], "doors": doors[:min(nd.value, cap_d)], "n_rooms": int(nr.value), "n_doors": int(nd.value), "labels": lab,
           "depth": dep}
    if tail:
        out["shown"] = tail[0]
    return out


def cells_of_poses(poses, position, resolution: float):
    """probabilityOf's cell of every pose of poses [P][3] (GridMap.java:273-274): (int)((x - position.x) / resolution) in double -- the
    pose's floats and the map's float position and resolution widened -- with Java's cast: toward zero (a coordinate in (-1, 0) cells
    lands in cell 0), NaN -> 0, saturating.  (gx, gy), int64 [P] each; a cell off the map is the caller's to test for."""
    p = np.asarray(poses, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    out = []
    for col in (0, 1):
        with np.errstate(invalid="ignore", over="ignore"):
            q = (p[:, col] - np.float64(np.float32(position[col]))) / np.float64(np.float32(resolution))
        q = np.where(np.isnan(q), 0.0, np.clip(np.trunc(q), -2147483648.0, 2147483647.0))
        out.append(q.astype(np.int64))
    return out[0], out[1]


def mode_estimate(records) -> dict:
    """Pose estimates of pose modes (ParticleFilter.modes' records), host numpy, float64 arrays over the records: "mean" [n][3] =
    (wx / w, wy / w, atan2(ws, wc)); "cov" [n][2][2], the position covariance [[wxx / w - mx^2, wxy / w - mx * my], [., wyy / w -
    my^2]]; "circular_variance" [n] = 1 - hypot(wc, ws) / w; "share" [n] = w / sum of w over the listed modes.  A mode of zero weight
    gives NaN."""
    r = np.asarray(records)
    w = r["w"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mx, my = r["wx"] / w, r["wy"] / w
        cxy = r["wxy"] / w - mx * my
        cov = np.stack([np.stack([r["wxx"] / w - mx * mx, cxy], axis=-1), np.stack([cxy, r["wyy"] / w - my * my], axis=-1)], axis=-2)
        return dict(mean=np.stack([mx, my, np.arctan2(r["ws"], r["wc"])], axis=-1), cov=cov,
                    circular_variance=1.0 - np.hypot(r["wc"], r["ws"]) / w, share=w / w.sum())


def strongest_mode(records) -> int:
    """The index of the record of the largest w among pose modes (ParticleFilter.modes' records), ties to the first; -1 for none"""
    w = np.asarray(records)["w"]
    return int(np.argmax(w)) if len(w) else -1


_DESCEND_ORDER = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))       # E, N, W, S, NE, NW, SW, SE; north is y + 1


def descend(field, start) -> list:
    """The cells of one cheapest path from start = (x, y) down to a seed over a WHOLE-MAP cost-to-go field, in order, start first: from
    the current cell the first neighbour n, in the order E, N, W, S, NE, NW, SW, SE (north = y + 1), with field[n] + step ==
    field[current].  A diagonal is admitted only if both cells it squeezes between are not FAR -- sound, because the side cells of a
    legal diagonal predecessor cost at most predecessor + 5 < current.  A FAR start (or one off the map) returns an empty list."""
    f = np.asarray(field)
    H, W = f.shape
    x, y = int(start[0]), int(start[1])
    far = _lib.GMS_REACH_FAR
    if not (0 <= x < W and 0 <= y < H) or f[y, x] == far:
        return []
    path = [(x, y)]
    while f[y, x] != 0:
        cur = int(f[y, x])
        for dx, dy in _DESCEND_ORDER:
            nx, ny = x + dx, y + dy
            if not (0 <= nx < W and 0 <= ny < H) or f[ny, nx] == far:
                continue
            if dx and dy:
                if f[y, nx] == far or f[ny, x] == far or int(f[ny, nx]) + _lib.GMS_REACH_DIAG != cur:
                    continue
            elif int(f[ny, nx]) + _lib.GMS_REACH_AXIS != cur:
                continue
            x, y = nx, ny
            break
        else:
            raise ValueError(f"descend: no predecessor at ({x}, {y}): not a whole-map cost-to-go field")
        path.append((x, y))
    return path


def route_points(waypoints, n: int, position, resolution: float) -> np.ndarray:
    """The world coordinates of ONE route's waypoints (GridMap.route's waypoints [max_waypoints][2] of one start and its record's
    n_waypoints; a cell list and n_cells do as well): the cell centres, position + (cell + 0.5) * resolution in double with the map's
    float position and resolution widened, float64 [n][2] = (x, y)."""
    w = np.asarray(waypoints).reshape(-1, 2)[:int(n)].astype(np.float64)
    res = np.float64(np.float32(resolution))
    return np.stack([np.float64(np.float32(position[0])) + (w[:, 0] + 0.5) * res, np.float64(np.float32(position[1])) + (w[:, 1] + 0.5) * res], axis=-1)


class _Source:
    """Where a map query reads its map, the Python counterpart of the library's QuerySource: map `index` of a gms_map handle
    (kind "map": the entry points gms_map_*) or a particle of a gms_slam handle (kind "slam": gms_slam_*, `index` a handle-wide
    slot or GMS_VIEW_STRONGEST of `filter`).  The entry points of a query take the same arguments on both; a particle's are followed
    by the shown word, the index of the particle that was read."""

    def __init__(self, kind: str, handle, index: int, W: int, H: int, filter: int = 0):
        self.kind, self.lead, self.W, self.H, self.filter, self.shows = kind, (handle, int(index)), W, H, int(filter), kind == "slam"

    def host(self, query: str, *args) -> tuple:
        """gms_<kind>_<query>(handle, index, args...); returns what the source appends to the result: (shown,) or ()"""
        fn = getattr(load(), f"gms_{self.kind}_{query}")
        if not self.shows:
            check(fn(*self.lead, *args))
            return ()
        shown = C.c_int32(-1)
        check(fn(*self.lead, *args, C.byref(shown)))
        return (int(shown.value),)

    def dev(self, query: str, *args, shown_out=None) -> tuple:
        """gms_<kind>_<query>_dev(handle, index, args...), shown_out the device word of a particle's; returns (shown_out,) or ()"""
        tail = (_shown_ptr(query, shown_out),) if self.shows else ()
        check(getattr(load(), f"gms_{self.kind}_{query}_dev")(*self.lead, *args, *tail))
        return (shown_out,) if self.shows else ()


# One body per query for a shared map and a particle's own: each returns a tuple, the query's values and then what the source appends.
# out (frontiers: dev) given: the device form, into the caller's torch tensors on the handle's stream.
def _query_view(src: _Source, rect, decimate: int, likelihood: bool, packed: bool, out, shown_out) -> tuple:
    v = _lib.GmsView(*_rect(src.W, src.H, rect), int(decimate), _lib.GMS_VIEW_LIKELIHOOD if likelihood else _lib.GMS_VIEW_LOG,
                     _lib.GMS_VIEW_PACKED32 if packed else _lib.GMS_VIEW_GREY8, src.filter)
    v, shape, nbytes = _sized(load().gms_view_size, v)
    if out is not None:
        return (out,) + src.dev("view", C.byref(v), _device_ptr("view", "out", out, nbytes), shown_out=shown_out)
    img = np.empty(shape, dtype=np.uint32 if packed else np.uint8)
    return (img,) + src.host("view", C.byref(v), ptr(img))


def _query_clearance(src: _Source, rect, max_radius: int, not_free: bool, out, shown_out) -> tuple:
    c, shape, nbytes = _sized(load().gms_clearance_size, _lib.GmsClearance(*_rect(src.W, src.H, rect), int(max_radius), _obstacles(not_free), src.filter))
    if out is not None:
        return (out,) + src.dev("clearance", C.byref(c), _device_ptr("clearance", "out", out, nbytes), shown_out=shown_out)
    field = np.empty(shape, dtype=np.uint16)
    return (field,) + src.host("clearance", C.byref(c), ptr(field))


def _query_skeleton(src: _Source, rect, max_radius: int, not_free: bool, min_clear: int, min_gap: int, want, dev, shown_out) -> tuple:
    """want: which of (site, skel, totals) the host form returns, None for the others; dev: the device form's (site, skel, totals)
    torch tensors, None for an output that is not wanted"""
    q = _lib.GmsSkeleton(*_rect(src.W, src.H, rect), int(max_radius), _obstacles(not_free), int(min_clear), int(min_gap), src.filter)
    ow, oh, sb, kb = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    check(load().gms_skeleton_size(C.byref(q), C.byref(ow), C.byref(oh), C.byref(sb), C.byref(kb)))
    if dev is not None:
        site, skel, totals = dev
        ptrs = (_device_ptr("skeleton", "site", site, sb.value, optional=True), _device_ptr("skeleton", "skel", skel, kb.value, optional=True),
                _device_ptr("skeleton", "totals", totals, _lib.SKELETON_TOTALS_DTYPE.itemsize, optional=True))
        return (site, skel, totals) + src.dev("skeleton", C.byref(q), *ptrs, shown_out=shown_out)
    shape = (oh.value, ow.value)
    site = np.empty(shape, dtype=np.uint32) if want[0] else None
    skel = np.empty(shape, dtype=np.uint16) if want[1] else None
    totals = np.zeros(1, dtype=_lib.SKELETON_TOTALS_DTYPE) if want[2] else None
    tail = src.host("skeleton", C.byref(q), *(None if a is None else ptr(a) for a in (site, skel, totals)))
    return (site, skel, None if totals is None else totals[0]) + tail


def _query_reach(src: _Source, seeds, max_cost: int, inflate: int, not_free: bool, rect, out, shown_out) -> tuple:
    """seeds None (a particle's map alone): the shown particle's own cell"""
    r = _lib.GmsReach(*_rect(src.W, src.H, rect), int(max_cost), int(inflate), _obstacles(not_free), src.filter)
    r, shape, nbytes = _sized(load().gms_reach_size, r)
    if out is not None:
        sp = _device_ptr("reach", "seeds", seeds, itemsize=4, multiple=2, optional=src.shows)
        return (out,) + src.dev("reach", C.byref(r), sp, 0 if sp is None else seeds.numel() // 2, _device_ptr("reach", "out", out, nbytes),
                                shown_out=shown_out)
    sd = None if seeds is None and src.shows else _reach_seeds(seeds)
    field = np.empty(shape, dtype=np.uint16)
    return (field,) + src.host("reach", C.byref(r), None if sd is None else ptr(sd), 0 if sd is None else len(sd), ptr(field))


def _query_gain(src: _Source, poses, probes, max_range: int, out, shown_out) -> tuple:
    g = _lib.GmsGain(int(max_range), src.filter)
    if out is not None:                                  # poses: (device address, P), probes: (device address, B)
        (dev_poses, P), (dev_probes, B) = poses, probes
        return (out,) + src.dev("gain", C.byref(g), C.c_void_p(dev_poses), int(P), C.c_void_p(dev_probes), int(B),
                                _device_ptr("gain", "out", out, _lib.GAIN_DTYPE.itemsize * int(P)), shown_out=shown_out)
    p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
    b = _beams_of(probes).reshape(-1)
    rec = np.empty(len(p), dtype=_lib.GAIN_DTYPE)
    return (rec,) + src.host("gain", C.byref(g), ptr(p), len(p), ptr(b), len(b), ptr(rec))


def _query_rollout(src: _Source, poses, arcs, points, max_range: int, inflate: int, not_free: bool, clear, cost, out, shown_out) -> tuple:
    """poses None (a particle's map alone): the shown particle's own pose.  out given: the device form -- poses = (device address, P)
    or None, arcs = (device address, K, T), points = (device address, F) or None, clear / cost torch device tensors or None"""
    r = _lib.GmsRollout(int(max_range), int(inflate), _obstacles(not_free), src.filter)
    if out is not None:
        (dev_poses, P), (dev_arcs, K, T), (dev_points, F) = poses or (None, 0), arcs, points or (None, 0)
        fields = [_device_ptr("rollout", n, f, 2 * src.W * src.H, itemsize=2, optional=True) for n, f in (("clear", clear), ("cost", cost))]
        return (out,) + src.dev("rollout", C.byref(r), C.c_void_p(dev_poses), int(P), C.c_void_p(dev_arcs), int(K), int(T), C.c_void_p(dev_points), int(F),
                                *fields, _device_ptr("rollout", "out", out, _lib.ROLLOUT_DTYPE.itemsize * max(int(P), 1) * int(K)), shown_out=shown_out)
    p = None if poses is None and src.shows else np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
    a = _rollout_table(arcs)
    f = np.zeros((0, 2), dtype=np.float32) if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    cl, co = _frontier_cost(clear, src.W, src.H), _frontier_cost(cost, src.W, src.H)
    rec = np.empty((1 if p is None else len(p), a.shape[0]), dtype=_lib.ROLLOUT_DTYPE)
    return (rec,) + src.host("rollout", C.byref(r), None if p is None else ptr(p), 0 if p is None else len(p), ptr(a), a.shape[0], a.shape[1],
                             ptr(f) if len(f) else None, len(f), None if cl is None else ptr(cl), None if co is None else ptr(co), ptr(rec))


def _query_route(src: _Source, field, starts, look: int, inflate: int, not_free: bool, max_cells: int, max_waypoints: int, clear, cells, dev=None) -> tuple:
    """starts None (a particle's map alone): the shown particle's own cell.  dev = (out, waypoints, shown_out), torch device tensors
    (shown_out or None): the device form -- field, starts, clear and cells (or None) then torch device tensors too"""
    r = _lib.GmsRoute(int(max_cells), int(max_waypoints), int(look), int(inflate), _obstacles(not_free), src.filter)
    check(load().gms_route_check(C.byref(r)))
    if dev is not None:
        out, waypoints, shown_out = dev
        sp = _device_ptr("route", "starts", starts, itemsize=4, multiple=2, optional=src.shows)
        P = 0 if sp is None else starts.numel() // 2
        n = max(P, 1)
        src.dev("route", C.byref(r), sp, P, _device_ptr("route", "field", field, 2 * src.W * src.H, itemsize=2),
                _device_ptr("route", "clear", clear, 2 * src.W * src.H, itemsize=2, optional=True),
                _device_ptr("route", "out", out, _lib.ROUTE_DTYPE.itemsize * n), _device_ptr("route", "waypoints", waypoints, 8 * n * r.max_waypoints, itemsize=4),
                _device_ptr("route", "cells", cells, 8 * n * r.max_cells, itemsize=4, optional=True), shown_out=shown_out)
        return (out, waypoints) + ((cells,) if cells is not None else ()) + ((shown_out,) if src.shows else ())
    if starts is None and not src.shows:
        raise ValueError("route: starts are required (a particle's map alone has a cell of its own)")
    sd = None if starts is None else _reach_seeds(starts, "route", "starts")
    n = 1 if sd is None else len(sd)
    if field is None:
        raise ValueError("route: field, the whole map's cost-to-go field, is required")
    co, cl = _frontier_cost(field, src.W, src.H, "route", "field"), _frontier_cost(clear, src.W, src.H, "route", "clear", "clearance")
    rec = np.zeros(n, dtype=_lib.ROUTE_DTYPE)
    wps = np.zeros((n, r.max_waypoints, 2), dtype=np.int32)
    cel = np.zeros((n, r.max_cells, 2), dtype=np.int32) if cells else None
    tail = src.host("route", C.byref(r), None if sd is None else ptr(sd), 0 if sd is None else n, ptr(co), None if cl is None else ptr(cl), ptr(rec), ptr(wps),
                    None if cel is None else ptr(cel))
    return (rec, wps) + ((cel,) if cells else ()) + tail


def _query_locate(src: _Source, offsets, rect, tol: int, not_free: bool, min_score: int, cap: int, free_only: bool, full: bool, out, n_out,
                  shown_out) -> tuple:
    t = _locate_table(offsets) if out is None else None      # with out, offsets: (device address, n_theta, B)
    n_theta, B = t.shape[:2] if out is None else offsets[1:]
    lc = _locate_args(src.W, src.H, rect, (n_theta, B), tol, not_free, min_score, cap, free_only, src.filter)
    if out is not None:
        return (out, n_out) + src.dev("locate", C.byref(lc), C.c_void_p(offsets[0]), int(B),
                                      _device_ptr("locate", "out", out, _lib.LOCATE_DTYPE.itemsize * int(cap)),
                                      _device_ptr("locate", "n_out", n_out, 4, itemsize=4, contiguous=False), shown_out=shown_out)
    rec = np.empty(max(int(cap), 0), dtype=_lib.LOCATE_DTYPE)
    n = C.c_int32(0)
    tail = src.host("locate", C.byref(lc), ptr(t), B, ptr(rec), C.byref(n))
    return ((rec, int(n.value)) if full else rec[:n.value],) + tail


def _query_align(src: _Source, scan, poses, params, records, out=None) -> tuple:
    """out given: the device form -- scan = (device address, B), poses = (device address, P), records a torch device tensor or None"""
    prm = _align_params(params)
    if out is not None:
        (dev_beams, B), (dev_poses, P) = scan, poses
        return (out, records) + src.dev("align", C.c_void_p(dev_beams), int(B), C.c_void_p(dev_poses), int(P), C.byref(prm),
                                        _device_ptr("align", "out", out, 12 * int(P), itemsize=4),
                                        _device_ptr("align", "records_out", records, _lib.ALIGN_DTYPE.itemsize * int(P), optional=True))
    p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
    b = _beams_of(scan).reshape(-1)
    res = np.empty_like(p)
    rec = np.empty(len(p), dtype=_lib.ALIGN_DTYPE) if records else None
    tail = src.host("align", ptr(b), len(b), ptr(p), len(p), C.byref(prm), ptr(res), None if rec is None else ptr(rec))
    return ((res, rec) if records else (res,)) + tail


def _query_frontiers(src: _Source, min_size: int, inflate: int, cost, rect, labels, cap: int, dev=None):
    """dev = (records, labels, shown_out), torch device tensors or None each, cost then one too: the device form, which returns
    n_found alone"""
    f, shape, nbytes = _sized(load().gms_frontiers_size, _lib.GmsFrontiers(*_rect(src.W, src.H, rect), int(min_size), int(inflate), src.filter, 0))
    n = C.c_int32(0)
    if dev is not None:
        records, labels, shown_out = dev
        sfx = "_out" if src.shows else ""
        cap = 0 if records is None else records.numel() * records.element_size() // _lib.FRONTIER_DTYPE.itemsize
        src.dev("frontiers", C.byref(f), _device_ptr("frontiers", "cost", cost, src.W * src.H * 2, optional=True),
                _device_ptr("frontiers", "labels" + sfx, labels, nbytes, optional=True),
                _device_ptr("frontiers", "records" + sfx, records, optional=True), int(cap), C.byref(n), shown_out=shown_out)
        return int(n.value)
    cst = _frontier_cost(cost, src.W, src.H)
    rec = np.zeros(int(cap), dtype=_lib.FRONTIER_DTYPE)
    lab = np.empty(shape, dtype=np.uint32) if labels else None
    tail = src.host("frontiers", C.byref(f), None if cst is None else ptr(cst), None if lab is None else ptr(lab), ptr(rec) if cap else None,
                    int(cap), C.byref(n))
    out = (rec[:min(n.value, int(cap))], int(n.value))
    return (out + (lab,) if labels else out) + tail


class GridMap:
    """GridMap(width, height, resolution, position) + its GridMapData (GridMap.java:80-132)."""

    def __init__(self, width: float, height: float, resolution: float, position: Sequence[float],
                 n_maps: int = 1, device: int = 0, max_beams: int = 0, kernel=None,
                 l_free: Optional[float] = None, l_occ: Optional[float] = None):
        L = load()
        p = GmsParams()
        check(L.gms_params_default(C.byref(p), width, height, resolution, position[0], position[1]))
        p.n_maps = n_maps
        p.device = device
        p.max_beams = max_beams
        if kernel is not None:
            k = np.asarray(kernel, dtype=np.float64)
            if k.size % 2 != 1 or k.size > _lib.GMS_MAX_TAPS:
                raise ValueError("kernel must have an odd number of taps <= GMS_MAX_TAPS")
            p.ktaps = k.size
            for i, t in enumerate(k):
                p.kernel[i] = float(t)
        if l_free is not None:
            p.l_free = l_free
        if l_occ is not None:
            p.l_occ = l_occ
        self.params = p
        self._h = C.c_void_p()
        check(L.gms_map_create(C.byref(p), C.byref(self._h)))
        W, H, M = C.c_int32(), C.c_int32(), C.c_int32()
        check(L.gms_map_get_size(self._h, C.byref(W), C.byref(H), C.byref(M)))
        self.W, self.H, self.n_maps = W.value, H.value, M.value
        self._filters = weakref.WeakSet()         # ParticleFilters bound to this map: they are closed before it

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            for pf in list(getattr(self, "_filters", ())):      # gms_map_destroy refuses while filters are alive
                pf.close()
            check(load().gms_map_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- geometry (GridMap.java:422-432) ---------------------------------------------------------
    @property
    def resolution(self) -> float:
        return float(self.params.resolution)

    @property
    def position(self):
        return (float(self.params.pos_x), float(self.params.pos_y))

    @property
    def kernel(self) -> np.ndarray:
        return np.array(self.params.kernel[: self.params.ktaps], dtype=np.float64)

    def getResolution(self): return self.resolution
    def getPosition(self): return self.position
    def getWorldSize(self):
        # gridSize * resolution in float (GridMap.java:88)
        return (float(np.float32(self.W) * np.float32(self.resolution)), float(np.float32(self.H) * np.float32(self.resolution)))

    def point_in_map(self, point) -> bool:
        """pointInMap (GridMap.java:164-170): float arithmetic."""
        tx = (np.float32(point[0]) - np.float32(self.params.pos_x)) / np.float32(self.params.resolution)
        ty = (np.float32(point[1]) - np.float32(self.params.pos_y)) / np.float32(self.params.resolution)
        return not (tx < 0 or ty < 0 or tx >= self.W or ty >= self.H)

    # -- stream / sync ---------------------------------------------------------------------------
    def set_stream(self, hip_stream: Optional[int]):
        """Run on an existing HIP stream (e.g. torch.cuda.Stream().cuda_stream).  None / 0 = the handle's own stream --
        note that torch's DEFAULT stream has handle 0, so passing it does not put the library on torch's stream."""
        check(load().gms_map_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def synchronize(self):
        check(load().gms_map_synchronize(self._h))

    # -- GridMapData ------------------------------------------------------------------------------
    def _shape(self):
        return (self.H, self.W) if self.n_maps == 1 else (self.n_maps, self.H, self.W)

    def _src(self, mi: int) -> _Source:
        """map mi as the source of a query"""
        return _Source("map", self._h, mi, self.W, self.H)

    def reset(self):
        check(load().gms_map_reset(self._h))

    def upload_log(self, log):
        a = np.ascontiguousarray(log, dtype=np.float64)
        assert a.size == self.n_maps * self.W * self.H
        check(load().gms_map_upload_log(self._h, ptr(a)))

    def download_log(self) -> np.ndarray:
        out = np.empty(self._shape(), dtype=np.float64)
        check(load().gms_map_download_log(self._h, ptr(out)))
        return out

    def upload_likelihood(self, lik):
        a = np.ascontiguousarray(lik, dtype=np.float64)
        assert a.size == self.n_maps * self.W * self.H
        check(load().gms_map_upload_likelihood(self._h, ptr(a)))

    def download_likelihood(self) -> np.ndarray:
        out = np.empty(self._shape(), dtype=np.float64)
        check(load().gms_map_download_likelihood(self._h, ptr(out)))
        return out

    def view(self, rect=None, decimate: int = 1, likelihood: bool = False, packed: bool = False, mi: int = 0, out=None):
        """GridMap.render's grey levels (GridMap.java:371-388) of map mi, made on the device: rect = (x0, y0, w, h) in cells (None: the
        whole map), decimate cells per pixel and axis, likelihood: likelihoodData instead of logData, packed: 0xFE000000 | g << 16 |
        g << 8 | g words instead of bytes.  Returns a numpy uint8 / uint32 array [ceil(h / d)][ceil(w / d)] (synchronises); with out -- a
        contiguous torch device tensor of that many bytes -- the picture is written there on the handle's stream, nothing is
        synchronised, and out is returned."""
        return _query_view(self._src(mi), rect, decimate, likelihood, packed, out, None)[0]

    def world_rect(self, center, size):
        """(x0, y0, w, h): the cells under a world rectangle (centre, size in metres), clamped to the map (world_rect_to_cells)"""
        return world_rect_to_cells(self, center, size)

    def cast(self, poses, probes, mi: int = 0) -> np.ndarray:
        """The predicted scan (gridmapslam.h "predicted scans"): from each of poses [P][3], the first occupied cell (logData > 0) on the
        walk integrateObservation would make for each probe -- a beam of which local_x, local_y and distance are read -- in map mi.
        Returns gms_cast_hit records [P][B] (step, x, y, range; step -1: nothing on the walk, range = the probe's own distance in grid
        units).  The walk includes the extra_steps cells past a probe's end point: a wall that close behind it is still reported."""
        p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        b = _beams_of(probes).reshape(-1)
        out = np.empty((len(p), len(b)), dtype=CAST_DTYPE)
        check(load().gms_map_cast(self._h, int(mi), ptr(p), len(p), ptr(b), len(b), ptr(out)))
        return out

    def cast_dev(self, dev_poses: int, P: int, dev_probes: int, B: int, out, mi: int = 0):
        """cast() with device pointers; out: a contiguous torch device tensor of P * B * 16 bytes, written on the handle's stream"""
        check(load().gms_map_cast_dev(self._h, int(mi), C.c_void_p(dev_poses), int(P), C.c_void_p(dev_probes), int(B),
                                      _device_ptr("cast_dev", "out", out, 16 * P * B)))
        return out

    def cast_at(self, probes, pf: "ParticleFilter", strongest: bool = False) -> np.ndarray:
        """cast() from the filter's device-resident weighted (or strongest particle's) pose, as integrate_at takes it: records [B]
        ([n_maps][B] on a batched handle, map i from its own filter pose)"""
        b = _beams_of(probes).reshape(-1)
        out = np.empty((self.n_maps, len(b)), dtype=CAST_DTYPE)
        check(load().gms_map_cast_at(self._h, ptr(b), len(b), pf._h, 1 if strongest else 0, ptr(out)))
        return out[0] if self.n_maps == 1 else out

    def cast_at_dev(self, dev_probes: int, B: int, pf: "ParticleFilter", out, strongest: bool = False):
        check(load().gms_map_cast_at_dev(self._h, C.c_void_p(dev_probes), int(B), pf._h, 1 if strongest else 0,
                                         _device_ptr("cast_at_dev", "out", out, 16 * self.n_maps * B)))
        return out

    def gain(self, poses, probes, max_range: int, mi: int = 0) -> np.ndarray:
        """The view gain (gridmapslam.h "view gain") of each of poses [P][3] in map mi: the DISTINCT cells the probes' walks see from
        there -- each walk as cast() makes it without the extra_steps cells, cut at max_range cells (1 .. 255, Chebyshev) from the
        start cell and ended by (and including) its first occupied cell -- counted by class.  Returns gms_gain_rec records [P]
        (GAIN_DTYPE: unknown, free_cells, occupied, hits, walked, start_x, start_y, pad).  Probes: probe_fan()."""
        return _query_gain(self._src(mi), poses, probes, max_range, None, None)[0]

    def gain_dev(self, dev_poses: int, P: int, dev_probes: int, B: int, out, max_range: int, mi: int = 0):
        """gain() with device pointers; out: a contiguous torch device tensor of P * 32 bytes, written on the handle's stream"""
        return _query_gain(self._src(mi), (dev_poses, P), (dev_probes, B), max_range, out, None)[0]

    def rollout(self, poses, arcs, points=None, max_range: int = 255, inflate: int = 0, not_free: bool = True, clear=None, cost=None,
                mi: int = 0) -> np.ndarray:
        """Trajectory rollouts (gridmapslam.h "trajectory rollouts") from each of the start poses [P][3] in map mi: arcs [K][T]
        (rollout_arcs()) are the candidates' poses in the start pose's frame, points [F][2] the footprint (footprint_box(); the
        centre is always tested as well).  A point collides off the map, farther than max_range cells from the start cell, or on a
        cell that reach() would block for inflate / not_free.  clear / cost: whole-map fields of clearance() / reach(), or None.
        Returns gms_rollout_rec records [P][K] (ROLLOUT_DTYPE: first_hit, hit_point, min_d2, best_step, best_cost, end_cost, flags,
        pad, last_x, last_y, start_x, start_y); rollout_pick() chooses among one pose's."""
        return _query_rollout(self._src(mi), poses, arcs, points, max_range, inflate, not_free, clear, cost, None, None)[0]

    def rollout_dev(self, dev_poses: int, P: int, dev_arcs: int, K: int, T: int, dev_points: int, F: int, out, max_range: int = 255, inflate: int = 0,
                    not_free: bool = True, clear=None, cost=None, mi: int = 0):
        """rollout() with device pointers (arcs 16-byte aligned); clear / cost: torch device uint16-sized tensors [H][W] or None; out: a
        contiguous torch device tensor of P * K * 32 bytes, written on the handle's stream"""
        return _query_rollout(self._src(mi), (dev_poses, P), (dev_arcs, K, T), (dev_points, F), max_range, inflate, not_free, clear, cost, out, None)[0]

    def route(self, field, starts, *, look: int = 64, inflate: int = 0, not_free: bool = True, max_cells: int = 4096, max_waypoints: int = 64, clear=None,
              cells: bool = False, mi: int = 0):
        """Routes (gridmapslam.h "routes") from each of the start cells [P][2] over field, a whole-map cost-to-go field of reach() for the
        same inflate / not_free: the cheapest 8-connected path down to a seed -- descend()'s cells -- pulled taut by line of sight over
        at most `look` path cells through what reach() blocks.  clear: a whole-map field of clearance(), or None.  Returns (records
        [P] of ROUTE_DTYPE: n_cells, n_waypoints, start_cost, end_cost, min_d2, flags, min_d2_at, end_x, end_y, pad; waypoints int32
        [P][max_waypoints][2], zero behind n_waypoints) and with cells=True the cell lists int32 [P][max_cells][2] as well;
        route_points() turns one route into world coordinates."""
        return _query_route(self._src(mi), field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells)

    def route_dev(self, field, starts, out, waypoints, *, look: int = 64, inflate: int = 0, not_free: bool = True, max_cells: int = 4096,
                  max_waypoints: int = 64, clear=None, cells=None, mi: int = 0):
        """route() on torch device tensors, on the handle's stream: field / clear uint16-sized [H][W], starts int32 [P][2], out P * 32
        bytes, waypoints int32 [P][max_waypoints][2], cells int32 [P][max_cells][2] or None; entries behind the counts are not written"""
        return _query_route(self._src(mi), field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells, (out, waypoints, None))

    def locate(self, offsets, rect=None, tol: int = 1, not_free: bool = False, min_score: int = 1, cap: int = 64, free_only: bool = True,
               mi: int = 0, full: bool = False):
        """Global scan matching (gridmapslam.h "global scan matching") in map mi: the candidates (k, x, y) -- a heading index of
        offsets [n_theta][B][2] (locate_offsets()) and a cell of rect = (x0, y0, w, h) (None: the whole map), with free_only only
        the known-free cells -- whose SCORE, the beams that end within tol cells of an obstacle (logData > 0, or with not_free every
        cell not known free), is at least min_score: the best cap of them (<= 4096) as gms_locate_rec records (LOCATE_DTYPE: score, k,
        x, y), score descending, then k, y, x ascending.  The result of the exhaustive search, found by a pruned multi-resolution
        one.  full=True: (all cap records, n_out), the filler records {0, -1, -1, -1} behind the first n_out included.
        Poses: locate_poses(); peaks: locate_peaks()."""
        return _query_locate(self._src(mi), offsets, rect, tol, not_free, min_score, cap, free_only, full, None, None, None)[0]

    def locate_dev(self, dev_offsets: int, n_theta: int, B: int, out, n_out, rect=None, tol: int = 1, not_free: bool = False, min_score: int = 1,
                   cap: int = 64, free_only: bool = True, mi: int = 0):
        """locate() with device memory on the handle's stream: dev_offsets the table's device address (its entries within [-4095,
        4095] or SKIP pairs: a precondition), out a contiguous torch device tensor of cap * 16 bytes (16-byte aligned), n_out an int32
        one.  The call waits on the stream once per level of the search."""
        return _query_locate(self._src(mi), (dev_offsets, n_theta, B), rect, tol, not_free, min_score, cap, free_only, False, out, n_out, None)

    def align(self, obs, poses, params=None, mi: int = 0, records: bool = False):
        """Continuous scan alignment (gridmapslam.h "continuous scan alignment") in map mi: each of poses [P][3] is moved by a damped
        Gauss-Newton scan matcher on the bilinearly interpolated likelihood field until the scan's end points lie on the field's ridges
        -- a sub-cell pose from "about here", at 4 x B field values per iteration.  params: an AlignParams (None: the defaults), or a
        dict of its fields.  Returns the poses, float32 [P][3]; records=True: (poses, records), ALIGN_DTYPE (status 0 ran all iters /
        1 converged / 2 no usable beam / 3 singular, iters_done, n_used, n_used0, score0, score, H [6]: the information matrix at the
        final pose -- align_covariance()).  The idiom after a global match: recs = m.locate(locate_offsets(scan, n_theta, res), ...);
        start = locate_poses(recs, m.position, res, n_theta=n_theta); fine = m.align(scan, start)."""
        r = _query_align(self._src(mi), obs, poses, params, records)
        return r if records else r[0]

    def align_dev(self, dev_beams: int, B: int, dev_poses: int, P: int, out, params=None, mi: int = 0, records_out=None):
        """align() with device memory on the handle's stream: dev_beams [B] gms_beam and dev_poses [P][3] float are device addresses,
        out a contiguous float32 torch device tensor of P * 3 elements (it may be the tensor behind dev_poses), records_out None or a
        contiguous torch device tensor of P * 80 bytes, 8-byte aligned.  Nothing is synchronised.  Returns (out, records_out)."""
        return _query_align(self._src(mi), (dev_beams, B), (dev_poses, P), params, records_out, out)

    def locate_stats(self) -> dict:
        """diagnostics of the last locate() on this handle: {"levels": the top level L of its search, "evaluated": the candidates it
        evaluated at levels 0 .. 7}"""
        levels, ev = C.c_int32(0), (C.c_int64 * 8)()
        check(load().gms_map_locate_stats(self._h, C.byref(levels), ev))
        return {"levels": int(levels.value), "evaluated": [int(v) for v in ev]}

    def scatter_table_builds(self) -> int:
        """diagnostics: seeding tables built so far (ParticleFilter.scatter on an unchanged map with the same request builds none)"""
        n = C.c_int64(0)
        check(load().gms_map_scatter_table_builds(self._h, C.byref(n)))
        return int(n.value)

    def cast_plane_builds(self) -> int:
        """diagnostics: launches of the casts' bit-plane pre-pass so far (casts of an unchanged map add none)"""
        n = C.c_int64(0)
        check(load().gms_map_cast_plane_builds(self._h, C.byref(n)))
        return int(n.value)

    def clearance(self, rect=None, max_radius: int = 25, not_free: bool = False, mi: int = 0, out=None):
        """The clearance field (gridmapslam.h "clearance fields") of map mi: for every cell of rect = (x0, y0, w, h) (None: the whole
        map) the squared distance in cells to the nearest obstacle cell of the whole map -- logData > 0, or with not_free every cell
        that is not known free, !(logData < 0) -- as uint16 [h][w]; GMS_CLEAR_FAR (0xFFFF) beyond max_radius (1 .. 255 cells).
        Returns a numpy array (synchronises); with out -- a contiguous torch device tensor of h * w * 2 bytes -- the field is written
        there on the handle's stream, nothing is synchronised, and out is returned (clearance_dev).  Metres: clearance_metres()."""
        return _query_clearance(self._src(mi), rect, max_radius, not_free, out, None)[0]

    def clearance_dev(self, out, rect=None, max_radius: int = 25, not_free: bool = False, mi: int = 0):
        """clearance() into out, a contiguous torch device tensor of h * w * 2 bytes, on the handle's stream"""
        return self.clearance(rect, max_radius, not_free, mi, out)

    def reach(self, seeds, max_cost: int = 0xFFFE, inflate: int = 0, not_free: bool = True, rect=None, mi: int = 0, out=None):
        """The cost-to-go field (gridmapslam.h "cost-to-go fields") of map mi: for every cell of rect = (x0, y0, w, h) (None: the whole
        map) the cost of the cheapest 8-connected path (5 per axis step, 7 per diagonal one, no corner cutting) from any of seeds
        [K][2] (x, y) cells through the cells that have no obstacle within `inflate` cells -- an obstacle is every cell not known free,
        !(logData < 0), or with not_free=False logData > 0 -- as uint16 [h][w]; GMS_REACH_FAR (0xFFFF) where blocked, unreachable or
        beyond max_cost.  Paths use the whole map.  Returns a numpy array; with out (a contiguous torch device tensor of h * w * 2
        bytes) seeds must be an int32 torch device tensor [K][2], the field is written there on the handle's stream, and out is
        returned (reach_dev).  Metres: reach_metres(); a path: descend()."""
        return _query_reach(self._src(mi), seeds, max_cost, inflate, not_free, rect, out, None)[0]

    def reach_dev(self, out, seeds, max_cost: int = 0xFFFE, inflate: int = 0, not_free: bool = True, rect=None, mi: int = 0):
        """reach() from device seeds into out, on the handle's stream; the call waits on that stream between batches of rounds"""
        return self.reach(seeds, max_cost, inflate, not_free, rect, mi, out)

    def frontiers(self, min_size: int = 1, inflate: int = 0, cost=None, rect=None, labels: bool = False, cap: int = 4096, mi: int = 0):
        """The frontier regions (gridmapslam.h "frontier regions") of map mi: the known-free cells (logData < 0) with a never-observed
        axis neighbour inside the map (0, -0.0, NaN), without those that have an occupied cell within `inflate` cells, grouped into
        maximal 8-connected regions.  Returns (records, n_found): records a structured array (FRONTIER_DTYPE: anchor, count, box,
        coordinate sums, goal) of the regions with count >= min_size in ascending anchor order, at most cap of them; n_found how
        many qualify.  cost: the whole map's cost-to-go field (the array reach() returns) -- a region's goal is then its member of the
        smallest cost, goal_cost that cost; without it goal = (-1, -1).  labels=True appends the label field of rect = (x0, y0, w, h)
        (None: the whole map), uint32 [h][w]: every frontier cell its region's anchor index y * W + x, GMS_FRONTIER_NONE elsewhere.
        Centroids: frontier_centroids()."""
        return _query_frontiers(self._src(mi), min_size, inflate, cost, rect, labels, cap)

    def frontiers_dev(self, records=None, labels=None, cost=None, min_size: int = 1, inflate: int = 0, rect=None, mi: int = 0) -> int:
        """frontiers() with device memory on the handle's stream: records (room for cap = bytes // 56 gms_frontier, 8-byte aligned),
        labels (h * w * 4 bytes, 4-byte aligned) and cost (the whole map's uint16 field) are contiguous torch device tensors, any of
        them None.  Returns n_found; the call waits on the stream once (once more when the handle's region table has to grow), so the
        outputs are complete when it returns."""
        return _query_frontiers(self._src(mi), min_size, inflate, cost, rect, False, 0, dev=(records, labels, None))

    def rooms(self, core: int = 15, inflate: int = 5, not_free: bool = True, min_core: int = 1, max_cost: int = 0xFFFE, rect=None,
              labels: bool = True, depth: bool = False, cap_rooms: int = 1024, cap_doors: int = 4096, mi: int = 0) -> dict:
        """Rooms and doors (gridmapslam.h "rooms and doors") of map mi: the cells not blocked at inflation `core` fall into 4-connected
        cores, the cores of at least min_core cells are the rooms, ranked by their anchors, and every cell not blocked at inflation
        `inflate` goes to the room that minimises (cost-to-go, rank) within max_cost.  Returns a dict: "rooms" (ROOM_DTYPE, rank
        order, at most cap_rooms), "doors" (DOOR_DTYPE: one record per pair of rooms whose cells touch across a cell edge, ascending
        (a, b), at most cap_doors), "n_rooms" / "n_doors" (the true numbers), "labels" (uint32 [h][w] of rect, the room's anchor index
        y * W + x or GMS_ROOM_NONE; None unless asked for) and "depth" (uint16 [h][w], the cost outside the room's core, GMS_REACH_FAR
        without a room; None unless asked for).  Helpers: room_centroids, door_points, rooms_of_cells, room_graph."""
        return _query_rooms(self._src(mi), core, inflate, not_free, min_core, max_cost, rect, (labels, depth), (cap_rooms, cap_doors))

    def rooms_dev(self, labels=None, depth=None, rooms=None, doors=None, core: int = 15, inflate: int = 5, not_free: bool = True, min_core: int = 1,
                  max_cost: int = 0xFFFE, rect=None, mi: int = 0) -> tuple:
        """rooms() with device memory on the handle's stream: labels (h * w * 4 bytes), depth (h * w * 2 bytes), rooms (room for
        bytes // 56 gms_room, 8-byte aligned) and doors (bytes // 48 gms_door, 8-byte aligned) are contiguous torch device tensors, any
        of them None.  Returns (n_rooms, n_doors); the call waits on the stream for the number of rooms, between batches of rounds
        and for the door table, and returns with the last copies into the outputs enqueued."""
        return _query_rooms(self._src(mi), core, inflate, not_free, min_core, max_cost, rect, None, None, dev=(labels, depth, rooms, doors, None))

    def rooms_stats(self) -> dict:
        """diagnostics of the last rooms() on this handle: {"rounds": launches over the tiles, "tile_runs": tile relaxations that
        actually ran, "door_rebuilds": how often the door table was doubled and filled again, "stage_us": the host clock's
        microseconds of the call's parts (planes, cores, rounds, fields and records, doors) where GMS_ROOMS_STAGES is set in the
        environment -- the call then waits on the stream after each --, else zeros}"""
        rounds, runs, rebuilds = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        us = (C.c_double * _lib.GMS_ROOMS_STAGES)()
        check(load().gms_map_rooms_stats(self._h, C.byref(rounds), C.byref(runs), C.byref(rebuilds)))
        check(load().gms_map_rooms_stage_us(self._h, us))
        return {"rounds": int(rounds.value), "tile_runs": int(runs.value), "door_rebuilds": int(rebuilds.value), "stage_us": list(us)}

    def reach_stats(self) -> dict:
        """diagnostics of the last cost-to-go field made on this handle: {"rounds": launches over the tiles, "tile_runs": tile
        relaxations that actually ran}"""
        rounds, runs = C.c_int32(0), C.c_int64(0)
        check(load().gms_map_reach_stats(self._h, C.byref(rounds), C.byref(runs)))
        return {"rounds": int(rounds.value), "tile_runs": int(runs.value)}

    def skeleton(self, rect=None, max_radius: int = 25, not_free: bool = False, min_clear: int = 1, min_gap: int = 2, mi: int = 0,
                 site: bool = True, skel: bool = True, totals: bool = True):
        """Nearest-obstacle sites and the free-space skeleton (gridmapslam.h "sites and skeleton") of map mi over rect = (x0, y0, w, h)
        (None: the whole map): (site uint32 [h][w], skel uint16 [h][w], totals).  site: the nearest obstacle cell oy * W + ox, the
        smaller index at equal distance, GMS_SITE_NONE beyond max_radius (site_cells, site_vectors); skel: d2 on the cells equally
        far from two pieces of wall at least min_gap cells apart and at least min_clear cells away, else 0 (skeleton_cells); totals:
        one SKELETON_TOTALS_DTYPE record.  An output switched off is not computed and comes back as None; one must stay on."""
        return _query_skeleton(self._src(mi), rect, max_radius, not_free, min_clear, min_gap, (site, skel, totals), None, None)[:3]

    def skeleton_dev(self, site=None, skel=None, totals=None, rect=None, max_radius: int = 25, not_free: bool = False, min_clear: int = 1,
                     min_gap: int = 2, mi: int = 0):
        """skeleton() into contiguous torch device tensors on the handle's stream, nothing synchronised: site of h * w * 4 bytes, skel
        of h * w * 2, totals of 32; None: that output is not computed"""
        return _query_skeleton(self._src(mi), rect, max_radius, not_free, min_clear, min_gap, None, (site, skel, totals), None)[:3]

    def nearest_poses(self, poses, max_radius: int = 25, not_free: bool = False, mi: int = 0) -> np.ndarray:
        """The nearest obstacle cell under each of poses [P][3] (x, y, theta; theta is not read) without making a field: NEAREST_DTYPE
        [P] = (site, d2), the site field's value at the pose's cell (clearance_poses' cell) and its squared distance;
        (GMS_SITE_OUTSIDE, GMS_CLEAR_OUTSIDE) off the map, (GMS_SITE_NONE, GMS_CLEAR_FAR) with nothing within max_radius."""
        p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(p), dtype=_lib.NEAREST_DTYPE)
        check(load().gms_map_nearest_poses(self._h, int(mi), ptr(p), len(p), int(max_radius), _obstacles(not_free), ptr(out)))
        return out

    def nearest_poses_dev(self, dev_poses: int, P: int, out, max_radius: int = 25, not_free: bool = False, mi: int = 0):
        """nearest_poses() with a device pointer; out: a contiguous torch device tensor of P * 8 bytes, written on the handle's stream"""
        check(load().gms_map_nearest_poses_dev(self._h, int(mi), C.c_void_p(dev_poses), int(P), int(max_radius), _obstacles(not_free),
                                               _device_ptr("nearest_poses_dev", "out", out, 8 * int(P))))
        return out

    def clearance_poses(self, poses, max_radius: int = 25, not_free: bool = False, mi: int = 0) -> np.ndarray:
        """The clearance under each of poses [P][3] (x, y, theta; theta is not read) without making a field: uint16 [P], the field's
        value at the pose's cell -- (int)((x - position) / resolution) as probabilityOf takes it -- or GMS_CLEAR_OUTSIDE (0xFFFE)
        where that cell is off the map."""
        p = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(p), dtype=np.uint16)
        check(load().gms_map_clearance_poses(self._h, int(mi), ptr(p), len(p), int(max_radius), _obstacles(not_free), ptr(out)))
        return out

    def clearance_poses_dev(self, dev_poses: int, P: int, out, max_radius: int = 25, not_free: bool = False, mi: int = 0):
        """clearance_poses() with a device pointer; out: a contiguous torch device tensor of P * 2 bytes, written on the handle's stream"""
        check(load().gms_map_clearance_poses_dev(self._h, int(mi), C.c_void_p(dev_poses), int(P), int(max_radius), _obstacles(not_free),
                                                 _device_ptr("clearance_poses_dev", "out", out, 2 * int(P))))
        return out

    def copy_from(self, other: "GridMap"):
        """createMapData(other) (GridMap.java:106-124)."""
        check(load().gms_map_copy(self._h, other._h))

    def combine_from(self, batch: "GridMap"):
        """calculateCombined (J/app/GridMapApp.java:439-458): this (single) map := combination of batch's maps."""
        check(load().gms_map_combine(self._h, batch._h))

    def warp_from(self, src: "GridMap", pose=None, *, c=None, s=None, op="compare", rect=None, clamp: float = 0.0, mi: int = 0, src_mi: int = 0,
                  stats: bool = True):
        """Map src_mi of src read through a rigid transform and compared with, copied into, added to or filled into rectangle rect
        (None: all) of map mi (gridmapslam.h "map warps"): src of any size, corner and resolution.  pose = (x, y, theta): the pose of
        src's world frame in this map's world -- or (x, y) with c and s, the cosine and sine as they are --; op "compare" (writes
        nothing), "replace", "add" (log-odds fusion where src is known, clamped to [-clamp, clamp] when clamp > 0) or "fill" (only
        where this map is unknown and src is known).  Returns the class-pair counts, a WARP_STATS_DTYPE record taken from this
        map's values BEFORE the call (warp_agreement() reads it), or None with stats=False; synchronises."""
        w = _warp_request(self.W, self.H, pose, c, s, op, rect, clamp)
        return _query_warp(src._src(src_mi), self, mi, w, stats, None, None, False)[0]

    def warp_from_dev(self, src: "GridMap", stats_out, pose=None, *, c=None, s=None, op="compare", rect=None, clamp: float = 0.0, mi: int = 0,
                      src_mi: int = 0):
        """warp_from() with the counts written to stats_out -- a contiguous torch device tensor of 80 bytes, 8-byte aligned, or None
        -- on this handle's stream; nothing is synchronised"""
        w = _warp_request(self.W, self.H, pose, c, s, op, rect, clamp)
        return _query_warp(src._src(src_mi), self, mi, w, False, stats_out, None, True)[0]

    def deskew(self, angles, distances, hits, d_center: float, d_theta: float) -> "Observation":
        """The de-skew loop of GridMapApp.onHandleData (J/app/GridMapApp.java:143-175), on the device."""
        a = np.ascontiguousarray(angles, dtype=np.float64)
        d = np.ascontiguousarray(distances, dtype=np.float64)
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        out = np.zeros(len(a), dtype=BEAM_DTYPE)
        check(load().gms_map_deskew(self._h, ptr(a), ptr(d), ptr(h), len(a), d_center, d_theta, ptr(out), None))
        return Observation(out)

    def get_raw_at(self, x: int, y: int, mi: int = 0) -> float:
        raw = C.c_double()
        check(load().gms_map_get_raw_at(self._h, mi, x, y, C.byref(raw), None))
        return raw.value

    def get_prob_at(self, x: int, y: int, mi: int = 0) -> float:
        prob = C.c_double()
        check(load().gms_map_get_raw_at(self._h, mi, x, y, None, C.byref(prob)))
        return prob.value

    # -- the hot path -----------------------------------------------------------------------------
    def get_raw_at_point(self, point, mi: int = 0) -> float:
        """getRawAt(map, Vec2 point) (GridMap.java:142-148)."""
        raw = C.c_double()
        check(load().gms_map_get_at_point(self._h, mi, float(point[0]), float(point[1]), C.byref(raw), None))
        return raw.value

    def get_likelihood(self, point, mi: int = 0) -> float:
        """getLikelihood(map, Vec2 point) (GridMap.java:150-156)."""
        lik = C.c_double()
        check(load().gms_map_get_at_point(self._h, mi, float(point[0]), float(point[1]), None, C.byref(lik)))
        return lik.value

    getLikelihood = get_likelihood

    def _beam_args(self, obs):
        b = _beams_of(obs)
        if self.n_maps > 1:
            assert b.ndim == 2 and b.shape[0] == self.n_maps, "beams must be [n_maps][B]"
        B = b.shape[-1]
        return b, B

    def _pose_args(self, pose):
        p = np.ascontiguousarray(pose, dtype=np.float32)
        assert p.size == 3 * self.n_maps
        return p

    def integrate_observation(self, obs, pose):
        """integrateObservation(map, obs, pose) (GridMap.java:173-191)."""
        b, B = self._beam_args(obs)
        p = self._pose_args(pose)
        check(load().gms_map_integrate(self._h, ptr(b), B, ptr(p)))

    def integrate_at(self, obs, pf: "ParticleFilter", strongest: bool = False):
        b, B = self._beam_args(obs)
        check(load().gms_map_integrate_at(self._h, ptr(b), B, pf._h, 1 if strongest else 0))

    def apply_measurement(self, start_x, start_y, end_x, end_y, measured_distance, was_hit):
        """applyMeasurement (GridMap.java:194-228), grid coordinates, map 0."""
        check(load().gms_map_apply_ray(self._h, start_x, start_y, end_x, end_y, measured_distance, int(bool(was_hit))))

    def trace_ray(self, x0, y0, x1, y1, extra=2, cap=4096) -> np.ndarray:
        """RayIterator.init + iteration (J/slam/RayIterator.java:65-130) -> [n][2] cells, in order."""
        cells = np.empty((cap, 2), dtype=np.int32)
        n = C.c_int32()
        check(load().gms_map_trace_ray(self._h, x0, y0, x1, y1, extra, ptr(cells), cap, C.byref(n)))
        if n.value > cap:
            return self.trace_ray(x0, y0, x1, y1, extra, cap=n.value)
        return cells[: n.value].copy()

    def trace_scan(self, obs, pose, cap=2048):
        """Cells and sensor-model classes each beam of integrateObservation visits (map untouched)."""
        b = _beams_of(obs)
        B = b.shape[-1]
        p = np.ascontiguousarray(pose, dtype=np.float32)
        cells = np.empty((B, cap, 2), dtype=np.int32)
        cls = np.empty((B, cap), dtype=np.uint8)
        counts = np.empty(B, dtype=np.int32)
        check(load().gms_map_trace_scan(self._h, ptr(b), B, ptr(p), ptr(cells), ptr(cls), cap, ptr(counts)))
        if counts.max(initial=0) > cap:
            return self.trace_scan(obs, pose, cap=int(counts.max()))
        return cells, cls, counts

    def compute_likelihood_map(self):
        """computeLikelihoodMap(map) (GridMap.java:233-250)."""
        check(load().gms_map_build_likelihood(self._h))

    def update(self, obs, pose):
        """integrateObservation + computeLikelihoodMap restricted to what the scan changed."""
        b, B = self._beam_args(obs)
        p = self._pose_args(pose)
        check(load().gms_map_update(self._h, ptr(b), B, ptr(p)))

    def update_at(self, obs, pf: "ParticleFilter", strongest: bool = False):
        b, B = self._beam_args(obs)
        check(load().gms_map_update_at(self._h, ptr(b), B, pf._h, 1 if strongest else 0))

    def probability_of(self, obs, pose) -> float:
        """probabilityOf(map, obs, pose) (GridMap.java:261-294) for one pose (map 0)."""
        assert self.n_maps == 1
        pf = ParticleFilter(self, 1)
        try:
            pf.set_poses(np.asarray(pose, dtype=np.float32).reshape(1, 3))
            pf.score(obs)
            return float(pf.get_weights()[0])
        finally:
            pf.close()

    def find_best_pose(self, obs, start_pose) -> np.ndarray:
        """findBestPose(map, obs, startPose) (GridMap.java:319-346)."""
        assert self.n_maps == 1
        pf = ParticleFilter(self, 1)
        try:
            pf.set_poses(np.asarray(start_pose, dtype=np.float32).reshape(1, 3))
            pf.refine_poses(obs)
            return pf.get_poses()[0]
        finally:
            pf.close()

    # -- measurement ------------------------------------------------------------------------------
    def profile(self, on=True):
        """on: True/False, or a bitmask of kernel classes (bit k = _lib.K_*)."""
        mask = ((1 << len(_lib.KERNEL_NAMES)) - 1 if on else 0) if isinstance(on, bool) else int(on)
        check(load().gms_profile_enable(self._h, mask))

    def deskew_dev(self, angles, distances, hits, d_center: float, d_theta: float):
        """deskew() without the read-back: the beams stay in the map's device staging buffer; returns (device address, count).
        Nothing is synchronised: the next launches on the handle's stream see them."""
        a = np.ascontiguousarray(angles, dtype=np.float64)
        d = np.ascontiguousarray(distances, dtype=np.float64)
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        dev = C.c_void_p()
        check(load().gms_map_deskew(self._h, ptr(a), ptr(d), ptr(h), len(a), d_center, d_theta, None, C.byref(dev)))
        return dev.value, len(a)

    # -- device-resident inputs (raw device pointers, e.g. torch tensor .data_ptr()) -------------------
    def update_dev(self, dev_beams: int, B: int, dev_poses: int):
        check(load().gms_map_update_dev(self._h, C.c_void_p(dev_beams), B, C.c_void_p(dev_poses)))

    def integrate_dev(self, dev_beams: int, B: int, dev_poses: int):
        check(load().gms_map_integrate_dev(self._h, C.c_void_p(dev_beams), B, C.c_void_p(dev_poses)))

    def update_at_dev(self, dev_beams: int, B: int, pf: "ParticleFilter", strongest: bool = False):
        check(load().gms_map_update_at_dev(self._h, C.c_void_p(dev_beams), B, pf._h, 1 if strongest else 0))

    def integrate_at_dev(self, dev_beams: int, B: int, pf: "ParticleFilter", strongest: bool = False):
        check(load().gms_map_integrate_at_dev(self._h, C.c_void_p(dev_beams), B, pf._h, 1 if strongest else 0))

    def profile_sample(self, stride: int = 1):
        """Bracket only every stride-th launch of the enabled kernel classes."""
        check(load().gms_profile_sample(self._h, stride))

    def profile_calibrate(self, reps: int = 200) -> float:
        """Mean event-bracket time around an empty kernel, in milliseconds (what a bracket costs by itself)."""
        v = C.c_double()
        check(load().gms_profile_calibrate(self._h, reps, C.byref(v)))
        return v.value

    def profile_calibrate2(self, reps: int = 200):
        """(event bracket around an empty kernel, one empty kernel in a back-to-back queue), both in milliseconds; their
        difference is what the two event markers add to a bracketed launch."""
        a, b = C.c_double(), C.c_double()
        check(load().gms_profile_calibrate2(self._h, reps, C.byref(a), C.byref(b)))
        return a.value, b.value

    def profile_reset(self):
        check(load().gms_profile_reset(self._h))

    def profile_get(self) -> dict:
        out = {}
        for k, name in enumerate(_lib.KERNEL_NAMES):
            ms, n = C.c_double(), C.c_int64()
            check(load().gms_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def tile_stats(self, enable: bool = True, fetch: bool = True):
        """Census of the likelihood tiles the rebuilds walked since the last call (gms_map_tile_stats): a dict
        {left_alone, constants_kept, constants_written, blurred}; reads and clears the counters, `enable` keeps counting."""
        out = (C.c_int64 * 4)()
        check(load().gms_map_tile_stats(self._h, 1 if enable else 0, out if fetch else None))
        return dict(zip(("left_alone", "constants_kept", "constants_written", "blurred"), [int(v) for v in out])) if fetch else None

    def debug_f32(self, op: int, a: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float32)
        out = np.empty_like(a)
        check(load().gms_debug_f32(self._h, op, ptr(a), ptr(out), a.size))
        return out

    # Java names
    integrateObservation = integrate_observation
    applyMeasurement = apply_measurement
    computeLikelihoodMap = compute_likelihood_map
    probabilityOf = probability_of
    findBestPose = find_best_pose
    getRawAt = get_raw_at
    getProbAt = get_prob_at
    pointInMap = point_in_map


class ParticleFilter:
    """ParticleFilter(numberOfParticles) (J/slam/ParticleFilter.java:43) bound to a GridMap."""

    def __init__(self, grid_map: GridMap, n: int):
        self.map = grid_map
        self.n = n
        self.n_maps = grid_map.n_maps
        self._h = C.c_void_p()
        check(load().gms_pf_create(grid_map._h, n, C.byref(self._h)))
        self.offset, self.n_global = 0, n
        grid_map._filters.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().gms_pf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pshape(self, last=()):
        return ((self.n,) if self.n_maps == 1 else (self.n_maps, self.n)) + tuple(last)

    def set_shard(self, offset: int, n_global: int):
        check(load().gms_pf_set_shard(self._h, offset, n_global))
        self.offset, self.n_global = offset, n_global

    # -- getParticles() ---------------------------------------------------------------------------
    def set_poses(self, xytheta):
        a = np.ascontiguousarray(xytheta, dtype=np.float32)
        assert a.size == self.n_maps * self.n * 3
        check(load().gms_pf_set_poses(self._h, ptr(a)))

    def get_poses(self) -> np.ndarray:
        out = np.empty(self._pshape((3,)), dtype=np.float32)
        check(load().gms_pf_get_poses(self._h, ptr(out)))
        return out

    def set_weights(self, w):
        a = np.ascontiguousarray(w, dtype=np.float64)
        assert a.size == self.n_maps * self.n
        check(load().gms_pf_set_weights(self._h, ptr(a)))

    def get_weights(self) -> np.ndarray:
        out = np.empty(self._pshape(), dtype=np.float64)
        check(load().gms_pf_get_weights(self._h, ptr(out)))
        return out

    def get_log_weights(self) -> np.ndarray:
        out = np.empty(self._pshape(), dtype=np.float64)
        check(load().gms_pf_get_log_weights(self._h, ptr(out)))
        return out

    def get_particles(self):
        """(poses [n][3], weights [n]) -- the fields of ParticleFilter.Particle (ParticleFilter.java:21-38)."""
        return self.get_poses(), self.get_weights()

    # -- SLAM.update pieces ------------------------------------------------------------------------
    def score(self, obs):
        """weight[i] = probabilityOf(map, obs, pose[i]) (SLAM.java:99)."""
        b, B = self.map._beam_args(obs)
        check(load().gms_pf_score(self._h, ptr(b), B))

    def set_poses_dev(self, dev_xytheta: int):
        check(load().gms_pf_set_poses_dev(self._h, C.c_void_p(dev_xytheta)))

    def score_dev(self, dev_beams: int, B: int):
        check(load().gms_pf_score_dev(self._h, C.c_void_p(dev_beams), B))

    def _r01(self, r01):
        """the draws as a contiguous float64 [n_maps] (an array of that shape passes through untouched: the hot loop's case)"""
        if isinstance(r01, np.ndarray) and r01.dtype == np.float64 and r01.shape == (self.n_maps,) and r01.flags.c_contiguous:
            return r01
        return np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))

    def slam_update_dev(self, dev_xytheta: int, dev_beams: int, B: int, r01, fraction: float = 0.5, integrate: bool = True):
        """SLAM.update + `if (neff < fraction*N) resample()` in one call on device-resident inputs."""
        r = self._r01(r01)
        check(load().gms_slam_update_dev(self._h, C.c_void_p(dev_xytheta or 0), C.c_void_p(dev_beams), B, ptr(r), fraction,
                                         1 if integrate else 0))

    def slam_update_u_dev(self, d_center: float, d_theta: float, seed: int, sequence: int, dev_beams: int, B: int, r01,
                          fraction: float = 0.5, integrate: bool = True):
        """SLAM.update(z, u) with the motion-model sample inside the scoring launch (= sample_motion + slam_update_dev(0, ...))."""
        r = self._r01(r01)
        check(load().gms_slam_update_u_dev(self._h, d_center, d_theta, seed, sequence, C.c_void_p(dev_beams), B, ptr(r), fraction,
                                           1 if integrate else 0))

    def slam_frame(self, angles, distances, hits, d_center: float, d_theta: float, seed: int, sequence: int, r01,
                   fraction: float = 0.5, integrate: bool = True):
        """One recorded revolution (GridMapApp.java:133-192) in one call: de-skew, motion-model sample, scan step."""
        a = np.ascontiguousarray(angles, dtype=np.float64)
        d = np.ascontiguousarray(distances, dtype=np.float64)
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        check(load().gms_slam_frame(self._h, ptr(a), ptr(d), ptr(h), a.size, d_center, d_theta, seed, sequence, ptr(r), fraction,
                                    1 if integrate else 0))

    def slam_update(self, poses, obs, r01, fraction: float = 0.5, integrate: bool = True, fetch: bool = False):
        """SLAM.update + conditional resample with HOST inputs (poses may be None)."""
        b, B = self.map._beam_args(obs)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        p = None if poses is None else np.ascontiguousarray(poses, dtype=np.float32)
        arr = (GmsPfStats * self.n_maps)() if fetch else None
        check(load().gms_slam_update(self._h, None if p is None else ptr(p), ptr(b), B, ptr(r), fraction, 1 if integrate else 0, arr))
        return self._stats(arr) if fetch else None

    def _stats(self, arr):
        out = [dict(weight_sum=s.weight_sum, neff=s.neff, strongest=s.strongest, n_zero=s.n_zero,
                    max_log_weight=s.max_log_weight) for s in arr]
        return out[0] if self.n_maps == 1 else out

    def normalize(self, fetch: bool = True):
        """weightSum / strongest / weight /= weightSum / Neff (SLAM.java:87-129)."""
        if not fetch:
            check(load().gms_pf_normalize(self._h, None))
            return None
        arr = (GmsPfStats * self.n_maps)()
        check(load().gms_pf_normalize(self._h, arr))
        return self._stats(arr)

    def stats(self):
        arr = (GmsPfStats * self.n_maps)()
        check(load().gms_pf_get_stats(self._h, arr))
        return self._stats(arr)

    def weighted_pose(self) -> np.ndarray:
        """getWeightedPose() (SLAM.java:165-178)."""
        out = np.empty((self.n_maps, 3), dtype=np.float32)
        check(load().gms_pf_weighted_pose(self._h, ptr(out)))
        return out[0] if self.n_maps == 1 else out

    def set_log_normalize(self, on: bool = True):
        """Opt-in (not in the reference): normalise from the log-weights, weight = exp(logw - max logw), instead of the plain
        product that underflows at hundreds of beams (gms_pf_set_log_normalize)."""
        check(load().gms_pf_set_log_normalize(self._h, 1 if on else 0))

    def set_reference_order(self, on: bool = True):
        """the audit path (gms_pf_set_reference_order): the scan's product, weightSum and the cumulative weights each as ONE chain in
        the reference's order (tests; slow)"""
        check(load().gms_pf_set_reference_order(self._h, 1 if on else 0))

    def resample(self, r01=None, want_indices: bool = False):
        """resample() (SLAM.java:133-153); r01 stands for Math.random()."""
        if r01 is None:
            r01 = np.random.random(self.n_maps)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        if not want_indices:
            check(load().gms_pf_resample(self._h, ptr(r), None, None))
            return None
        idx = np.empty(self._pshape(), dtype=np.int32)
        amb = np.empty(self.n_maps, dtype=np.int32)
        check(load().gms_pf_resample(self._h, ptr(r), ptr(idx), ptr(amb)))
        return idx, (int(amb[0]) if self.n_maps == 1 else amb)

    def resample_if(self, r01, fraction: float = 0.5):
        """if (neff < fraction * N) resample()  (J/app/GridMapApp.java:185-186), decided on the device."""
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        check(load().gms_pf_resample_if(self._h, ptr(r), fraction))

    def last_resample_indices(self) -> np.ndarray:
        """source slot of every particle after the last resampling step (also the one inside a scan step)."""
        idx = np.empty(self._pshape(), dtype=np.int32)
        check(load().gms_pf_last_resample_indices(self._h, ptr(idx)))
        return idx

    def did_resample(self):
        f = np.empty(self.n_maps, dtype=np.int32)
        check(load().gms_pf_did_resample(self._h, ptr(f)))
        return bool(f[0]) if self.n_maps == 1 else f.astype(bool)

    def segment_order_launches(self) -> int:
        """scoring launches so far whose workgroups took their particles in the segment's end-point order (development, tests)"""
        n = C.c_int64(0)
        check(load().gms_pf_segment_order_launches(self._h, C.byref(n)))
        return int(n.value)

    def last_step(self) -> dict:
        """Device-side record of the last normalise / scan step: the weighted pose of the SCORED population (what a
        fused scan step integrated the scan at), the strongest particle's pose, did_resample, n_ambiguous."""
        wp = np.empty((self.n_maps, 3), dtype=np.float32)
        sp = np.empty((self.n_maps, 3), dtype=np.float32)
        did = np.empty(self.n_maps, dtype=np.int32)
        amb = np.empty(self.n_maps, dtype=np.int32)
        check(load().gms_pf_last_step(self._h, ptr(wp), ptr(sp), ptr(did), ptr(amb)))
        if self.n_maps == 1:
            return dict(weighted_pose=wp[0], strongest_pose=sp[0], did_resample=bool(did[0]), n_ambiguous=int(amb[0]))
        return dict(weighted_pose=wp, strongest_pose=sp, did_resample=did.astype(bool), n_ambiguous=amb)

    def sample_motion(self, d_center: float, d_theta: float, seed: int, sequence: int):
        """pose[i] = sampleMotionModel(pose[i], u) (SLAM.java:155-163 -> Odometry.apply, Odometry.java:77-96)."""
        check(load().gms_pf_sample_motion(self._h, d_center, d_theta, seed, sequence))

    def scatter(self, rect=None, inflate: int = 0, mode: int = _lib.GMS_CLEAR_NOT_FREE, first: int = 0, count: Optional[int] = None, jitter: bool = True,
                seed: int = 0, sequence: int = 0, want_count: bool = False):
        """Seed slots [first, first + count) of every map's filter with poses drawn uniformly over the eligible cells of its map
        (gridmapslam.h "particle seeding"): free, inside rect = (x0, y0, w, h) in cells (None: the whole map), no obstacle of `mode`
        (GMS_CLEAR_NOT_FREE: a cell that is not free; GMS_CLEAR_OCCUPIED: an occupied one) within `inflate` cells.  count=None: to the end of the filter.  The
        headings are uniform over (-pi, pi), the weights 1 / n_global.  The draw is Philox on (seed, the global slot, sequence): give
        it a sequence sample_motion() does not use.  want_count: the eligible cells per map are read back (one synchronise) and
        returned, an int or an int64 array [n_maps]; otherwise nothing is synchronised and None is returned.  Slots for the recovery
        idiom: scatter_slots()."""
        sc = _lib.GmsScatter(*_rect(self.map.W, self.map.H, rect), int(inflate), int(mode), int(first),
                             self.n - int(first) if count is None else int(count), 1 if jitter else 0, 0)
        M = np.zeros(self.n_maps, dtype=np.int64) if want_count else None
        check(load().gms_pf_scatter(self._h, C.byref(sc), int(seed), int(sequence), None if M is None else ptr(M)))
        if M is None:
            return None
        return int(M[0]) if self.n_maps == 1 else M

    def modes(self, bin_cells: int, n_theta: int, min_count: int = 1, labels: bool = False, cap: int = 4096, mi: int = 0, records_out=None,
              labels_out=None):
        """The pose modes of map mi's filter (gridmapslam.h "pose modes"): the particles binned in squares of bin_cells cells and n_theta
        heading bins (1 .. 64), the occupied bins grouped into maximal 26-connected sets, the heading wrapping.  Returns (records,
        n_found, n_outside): records a structured array (MODE_DTYPE: anchor bin, count, bins, strongest member, box, the weighted
        sums w, wx, wy, wc, ws, wxx, wxy, wyy in the header's order) of the modes with count >= min_count in ascending anchor order,
        at most cap of them; n_found how many qualify; n_outside the particles off the map or with a non-finite heading.
        labels=True appends every particle's label, uint32 [n]: its mode's anchor index (bt * BH + by) * BW + bx whatever min_count
        is, GMS_MODE_NONE for a particle outside.  The sums cost one pass over the labels per stored record: keep cap or min_count
        tight on large filters.  Estimates: mode_estimate(), strongest_mode().
        records_out / labels_out: contiguous torch device tensors (room for cap = bytes // 112 gms_mode, 8-byte aligned; n * 4 bytes,
        4-byte aligned), either may be None -- the device form, written on the handle's stream; returns (n_found, n_outside).  Every
        form waits on the stream once."""
        q = _lib.GmsModes(int(bin_cells), int(n_theta), int(min_count), 0)
        nf, no = C.c_int32(0), C.c_int32(0)
        if records_out is not None or labels_out is not None:
            cap = 0 if records_out is None else records_out.numel() * records_out.element_size() // _lib.MODE_DTYPE.itemsize
            check(load().gms_pf_modes_dev(self._h, int(mi), C.byref(q), _device_ptr("modes", "labels_out", labels_out, self.n * 4, optional=True),
                                          _device_ptr("modes", "records_out", records_out, optional=True), int(cap), C.byref(nf), C.byref(no)))
            return int(nf.value), int(no.value)
        rec = np.zeros(int(cap), dtype=_lib.MODE_DTYPE)
        lab = np.empty(self.n, dtype=np.uint32) if labels else None
        check(load().gms_pf_modes(self._h, int(mi), C.byref(q), None if lab is None else ptr(lab), ptr(rec) if cap else None, int(cap),
                                  C.byref(nf), C.byref(no)))
        out = (rec[:min(nf.value, int(cap))], int(nf.value), int(no.value))
        return out + (lab,) if labels else out

    def _beam_factors(self, factors, behind: int, ahead: int) -> np.ndarray:
        f = np.ascontiguousarray(factors, dtype=np.float64)
        if f.shape != (2, int(behind) + int(ahead) + 2):
            raise ValueError(f"score_beams: factors must be [2][behind + ahead + 2] = (2, {int(behind) + int(ahead) + 2}), not {f.shape}")
        return f

    def score_beams(self, obs, factors, behind: int, ahead: int, residuals: bool = False):
        """The beam sensor model (gridmapslam.h "beam sensor model"): every particle is weighted by where the map's first occupied
        cell lies on each beam's walk relative to the measured end point -- what lies BETWEEN sensor and end point counts, unlike
        score().  factors [2][behind + ahead + 2] (row 0: beams with hit == 0, row 1: hit != 0; every entry finite and > 0;
        beam_model_factors() builds the usual mixture): entry k < T - 1 is for the residual d = k - behind walk steps (d < 0: the
        map's wall in front of the end point, held at -behind; d > 0: behind it, up to `ahead`), the last entry for a walk that found
        no wall.  The weight is the product of the beams' entries, the log-weight the sum of their logarithms, both in the header's
        one order.  Afterwards the filter is as score() leaves it: normalize(), resample[_if](), set_log_normalize(), modes() work
        unchanged.  residuals=True returns the table index per particle and beam, uint16 [n][B] ([n_maps][n][B] on a batched
        handle), and waits for the stream; otherwise nothing is returned and nothing synchronised."""
        b, B = self.map._beam_args(obs)
        f = self._beam_factors(factors, behind, ahead)
        res = np.empty(self._pshape((B,)), dtype=np.uint16) if residuals else None
        check(load().gms_pf_score_beams(self._h, ptr(b), B, int(behind), int(ahead), ptr(f), None if res is None else ptr(res)))
        return res

    def score_beams_dev(self, dev_beams: int, B: int, factors, behind: int, ahead: int, residuals_out=None):
        """score_beams() on device-resident beams [n_maps][B]; factors stay a host array.  residuals_out: None, or a contiguous torch
        device tensor of at least n_maps * n * B 16-bit elements that receives the table indices.  Runs on the handle's stream and
        synchronises nothing."""
        f = self._beam_factors(factors, behind, ahead)
        out = _device_ptr("score_beams_dev", "residuals_out", residuals_out, 2 * self.n_maps * self.n * int(B), optional=True)
        check(load().gms_pf_score_beams_dev(self._h, C.c_void_p(dev_beams), int(B), int(behind), int(ahead), ptr(f), out))

    def align(self, obs, params=None, records: bool = False):
        """GridMap.align() of every particle, in place (gridmapslam.h "continuous scan alignment", gms_pf_align): on a batched handle
        map i's particles on map i with obs [n_maps][B].  Afterwards the filter is as set_poses() of the new poses would leave it: the
        weights are untouched, a following score() weighs the aligned poses.  records=True returns the records, ALIGN_DTYPE [n]
        ([n_maps][n]), and waits for the stream; otherwise nothing is returned and nothing synchronised."""
        b, B = self.map._beam_args(obs)
        prm = _align_params(params)
        rec = np.empty(self._pshape(), dtype=_lib.ALIGN_DTYPE) if records else None
        check(load().gms_pf_align(self._h, ptr(b), B, C.byref(prm), None if rec is None else ptr(rec)))
        return rec

    def align_dev(self, dev_beams: int, B: int, params=None, records_out=None):
        """align() on device-resident beams [n_maps][B]; records_out: None, or a contiguous torch device tensor of n_maps * n * 80
        bytes, 8-byte aligned.  Runs on the handle's stream and synchronises nothing."""
        prm = _align_params(params)
        out = _device_ptr("align_dev", "records_out", records_out, _lib.ALIGN_DTYPE.itemsize * self.n_maps * self.n, optional=True)
        check(load().gms_pf_align_dev(self._h, C.c_void_p(dev_beams), int(B), C.byref(prm), out))
        return records_out

    def rollout_risk(self, arcs, points=None, max_range: int = 255, inflate: int = 0, not_free: bool = True) -> np.ndarray:
        """GridMap.rollout() from EVERY particle's pose, read on the device, counted per candidate (gms_pf_rollout): gms_rollout_risk
        records [K] ([n_maps][K] on a batched handle; ROLLOUT_RISK_DTYPE: n_hit, n_start_blocked, min_first_hit, pad, sum_first_hit,
        pad2).  After a resample the weights are equal and n_hit / n is the collision probability of the command.  A shard counts
        its own particles.  The filter is not changed."""
        a = _rollout_table(arcs)
        f = np.zeros((0, 2), dtype=np.float32) if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        r = _lib.GmsRollout(int(max_range), int(inflate), _obstacles(not_free), 0)
        out = np.empty(self._pshape()[:-1] + (a.shape[0],), dtype=_lib.ROLLOUT_RISK_DTYPE)
        check(load().gms_pf_rollout(self._h, C.byref(r), ptr(a), a.shape[0], a.shape[1], ptr(f) if len(f) else None, len(f), ptr(out)))
        return out

    def rollout_risk_dev(self, dev_arcs: int, K: int, T: int, dev_points: int, F: int, out, max_range: int = 255, inflate: int = 0, not_free: bool = True):
        """rollout_risk() with device pointers (arcs 16-byte aligned); out: a contiguous torch device tensor of n_maps * K * 32 bytes.
        Runs on the handle's stream and synchronises nothing."""
        r = _lib.GmsRollout(int(max_range), int(inflate), _obstacles(not_free), 0)
        check(load().gms_pf_rollout_dev(self._h, C.byref(r), C.c_void_p(dev_arcs), int(K), int(T), C.c_void_p(dev_points), int(F),
                                        _device_ptr("rollout_risk_dev", "out", out, _lib.ROLLOUT_RISK_DTYPE.itemsize * self.n_maps * int(K))))
        return out

    def set_refine(self, on: bool = True):
        """scan steps (slam_update*) run findBestPose on every particle before weighting it (SLAM.java:96-97)."""
        check(load().gms_pf_set_refine(self._h, 1 if on else 0))

    def refine_poses(self, obs):
        """pose[i] = findBestPose(map, obs, pose[i]) (GridMap.java:319-346)."""
        b, B = self.map._beam_args(obs)
        check(load().gms_pf_refine_poses(self._h, ptr(b), B))

    # -- multi-GPU plumbing (device pointers; see distributed.py) ----------------------------------
    def partials_len(self) -> int:
        n = C.c_int64()
        check(load().gms_pf_partials_len(self._h, C.byref(n)))
        return n.value

    def local_partials(self, dev_ptr: int):
        check(load().gms_pf_local_partials(self._h, C.c_void_p(dev_ptr)))

    def apply_partials(self, dev_partials: int, dev_packed: int):
        check(load().gms_pf_apply_partials(self._h, C.c_void_p(dev_partials), C.c_void_p(dev_packed)))

    def stats_from_partials(self, dev_partials: int):
        check(load().gms_pf_stats_from_partials(self._h, C.c_void_p(dev_partials)))

    def pack(self, dev_packed: int):
        check(load().gms_pf_pack(self._h, C.c_void_p(dev_packed)))

    def import_global(self, dev_packed_global: int):
        check(load().gms_pf_import_global(self._h, C.c_void_p(dev_packed_global)))

    # -- sharded filter with the exchanges inside the library (RCCL; see distributed.RcclComm) --------
    def normalize_sharded_begin(self, comm):
        check(load().gms_pf_normalize_sharded_begin(self._h, comm._h))

    def normalize_sharded_end(self, comm):
        check(load().gms_pf_normalize_sharded_end(self._h, comm._h))

    def slam_update_sharded_dev(self, comm, dev_xytheta: int, dev_beams: int, B: int, r01, fraction: float = 0.5,
                                integrate: bool = True):
        """slam_update_dev for a sharded filter: both collectives happen inside the call."""
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        check(load().gms_slam_update_sharded_dev(self._h, comm._h, C.c_void_p(dev_xytheta or 0), C.c_void_p(dev_beams), B,
                                                 ptr(r), fraction, 1 if integrate else 0))

    def slam_update_sharded_begin_dev(self, dev_xytheta: int, dev_beams: int, B: int):
        check(load().gms_slam_update_sharded_begin_dev(self._h, C.c_void_p(dev_xytheta or 0), C.c_void_p(dev_beams), B))

    def gather_buffers(self):
        """(packed_global ptr, bytes per rank, partials_global ptr, doubles per rank): both are all-gathered in place."""
        a, b = C.c_void_p(), C.c_void_p()
        na, nb = C.c_int64(), C.c_int64()
        check(load().gms_pf_gather_buffers(self._h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        return a.value, na.value, b.value, nb.value

    def slam_update_sharded_end_dev(self, dev_beams: int, B: int, r01, fraction: float = 0.5, integrate: bool = True):
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(r01, dtype=np.float64), (self.n_maps,)))
        check(load().gms_slam_update_sharded_end_dev(self._h, C.c_void_p(dev_beams), B, ptr(r), fraction, 1 if integrate else 0))

    getParticles = get_particles
    getWeightedPose = weighted_pose


class SLAM:
    """The particle filter the reference actually runs (J/slam/SLAM.java), with ONE shared map and N
    poses scored against it, the pose proposal being an input."""

    def __init__(self, width=6.0, height=6.0, resolution=0.05, position=(-3.0, -3.0), num_particles=500,
                 device: int = 0, max_beams: int = 0):
        self.grid_map = GridMap(width, height, resolution, position, device=device, max_beams=max_beams)   # SLAM.java:57
        self.num_particles = num_particles                                                                  # SLAM.java:50
        self.pf = ParticleFilter(self.grid_map, num_particles)
        self.strongest = 0
        self.neff = float(num_particles)
        self.grid_map.compute_likelihood_map()

    def reset(self):
        """reset() (SLAM.java:65-77)."""
        self.grid_map.reset()
        self.grid_map.compute_likelihood_map()
        self.pf.close()
        self.pf = ParticleFilter(self.grid_map, self.num_particles)

    def update(self, z: Observation, poses=None, d_theta: float = 0.0, refine: bool = False) -> float:
        """update(z, u) (SLAM.java:80-131).  `poses` are the motion-model samples (an input here);
        d_theta is u.dTheta for the skip-update rule (:82)."""
        skip_update = abs(d_theta) > math.radians(30)                   # :82
        if poses is not None:
            self.pf.set_poses(poses)                                    # :90
        if refine:
            self.pf.refine_poses(z)                                     # :96
        self.pf.score(z)                                                # :99
        st = self.pf.normalize()                                        # :100-124
        self.strongest, self.neff = st["strongest"], st["neff"]
        if not skip_update:
            self.grid_map.update_at(z, self.pf, strongest=False)        # :105 + :93 for the next scan
        return self.neff

    def resample(self, r01=None):
        self.pf.resample(r01)                                           # :133-153

    def get_weighted_pose(self):
        return self.pf.weighted_pose()                                  # :165-178

    def calculate_neff(self) -> float:
        return self.pf.stats()["neff"]                                  # :180-190

    def get_particles(self):
        return self.pf.get_particles()

    def get_strongest_particle(self) -> int:
        return self.strongest

    def get_grid_map(self) -> GridMap:
        return self.grid_map

    getWeightedPose = get_weighted_pose
    calculateNeff = calculate_neff
    getParticles = get_particles
    getStrongestParticle = get_strongest_particle
    getGridMap = get_grid_map


class _Borrowed:
    """a handle owned by another object (never destroyed from here)"""

    def close(self):
        self._h = C.c_void_p()


class _BorrowedMap(_Borrowed, GridMap):
    def __init__(self, handle, params):
        self.params = params
        self._h = handle
        W, H, M = C.c_int32(), C.c_int32(), C.c_int32()
        check(load().gms_map_get_size(self._h, C.byref(W), C.byref(H), C.byref(M)))
        self.W, self.H, self.n_maps = W.value, H.value, M.value
        self._filters = weakref.WeakSet()


class _BorrowedFilter(_Borrowed, ParticleFilter):
    def __init__(self, handle, grid_map, n):
        self.map = grid_map
        self.n = n
        self.n_maps = 1
        self._h = handle
        self.offset, self.n_global = 0, n


def _put_kernel(p, kernel):
    """the caller's blur kernel (None: gms_params_default's) into gms_params"""
    if kernel is not None:
        k = np.asarray(kernel, dtype=np.float64)
        p.ktaps = k.size
        for i, t in enumerate(k):
            p.kernel[i] = float(t)


class _SlamHandle:
    """What SLAMParticleMaps and SLAMParticleMapsBatch share: one gms_slam handle with its borrowed map and filter; the particles'
    maps are addressed by handle-wide slot (filter f's particle i: f * num_particles + i)."""

    def _create(self, width, height, resolution, position, num_particles, device, max_beams, kernel, n_maps=1, offset=None, n_global=None):
        """gms_slam_create with n_maps filters of num_particles each, or -- offset, n_global -- gms_slam_create_shard for one block"""
        L = load()
        p = GmsParams()
        check(L.gms_params_default(C.byref(p), width, height, resolution, position[0], position[1]))   # SLAM.java:57
        p.n_maps = int(n_maps)
        p.device = device
        p.max_beams = max_beams
        _put_kernel(p, kernel)
        self.params = p
        self.num_particles = int(num_particles)                                                          # :50
        self._h = C.c_void_p()
        if offset is None:
            check(L.gms_slam_create(C.byref(p), self.num_particles, C.byref(self._h)))
        else:
            check(L.gms_slam_create_shard(C.byref(p), self.num_particles, int(offset), int(n_global), C.byref(self._h)))
        mh, ph = C.c_void_p(), C.c_void_p()
        check(L.gms_slam_handles(self._h, C.byref(mh), C.byref(ph)))
        self.grid_map = _BorrowedMap(mh, p)                     # getGridMap() (:200); map f's GridMapData receives filter f's combined map
        self.pf = _BorrowedFilter(ph, self.grid_map, self.num_particles)
        self.pf.n_maps = int(n_maps)                            # (the filter's arrays are [n_maps][n])
        if offset is not None:
            self.pf.offset, self.pf.n_global = int(offset), int(n_global)
        self.W, self.H = self.grid_map.W, self.grid_map.H
        self.sequence = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.grid_map.close(); self.pf.close()
            check(load().gms_slam_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(load().gms_slam_reset(self._h))                                                            # :65-77

    def set_refine(self, on: bool = True):
        """update() runs GridMap.findBestPose (J/slam/GridMap.java:319-346) for every particle against its own likelihood field
        before weighting it (SLAM.java:96; the reference calls findBestPoseOptim, :97, and keeps this search commented out beside it)"""
        check(load().gms_slam_set_refine(self._h, int(bool(on))))

    def set_align(self, params=True):
        """gms_slam_set_align: every update aligns each particle against its own field (gridmapslam.h "per-particle scan alignment")
        between computeLikelihoodMap and the weighting -- the build's stand-in for findBestPoseOptim (SLAM.java:97).  params: an
        AlignParams or a dict of its fields, True for the library's defaults, None (or False) to switch it off.  With set_refine() on
        as well: the lattice search first, the alignment from its best pose."""
        if params is None or params is False:
            check(load().gms_slam_set_align(self._h, None))
            return
        prm = _align_params(None if params is True else params)
        check(load().gms_slam_set_align(self._h, C.byref(prm)))

    @staticmethod
    def _beam_table(who: str, factors, behind: int, ahead: int) -> np.ndarray:
        f = np.ascontiguousarray(factors, dtype=np.float64)
        if f.shape != (2, int(behind) + int(ahead) + 2):
            raise ValueError(f"{who}: factors must be [2][behind + ahead + 2] = (2, {int(behind) + int(ahead) + 2}), not {f.shape}")
        return f

    def set_beam_model(self, factors, behind: int = 0, ahead: int = 0, combine="multiply"):
        """gms_slam_set_beam_model: every update weighs each particle by the beam sensor model as well (gridmapslam.h "per-particle
        beam sensor model") -- the walk of every beam through the particle's OWN map as it stands before this scan is integrated, at
        the pose the particle is weighted at (after the motion sample, set_refine() and set_align(), where on).  factors [2][behind +
        ahead + 2] as ParticleFilter.score_beams takes them (beam_model_factors() builds the usual mixture); combine: "multiply" -- raw
        weight = probabilityOf * beam weight -- or "replace" -- the beam weight alone.  set_beam_model(None) switches it off (the
        default); reset() keeps the setting."""
        if factors is None or factors is False:
            check(load().gms_slam_set_beam_model(self._h, 0, 0, None, 0))
            return
        modes = {"multiply": _lib.GMS_SLAM_BEAMS_MULTIPLY, "replace": _lib.GMS_SLAM_BEAMS_REPLACE}
        if combine not in modes:
            raise ValueError(f'set_beam_model: combine must be "multiply" or "replace", not {combine!r}')
        f = self._beam_table("set_beam_model", factors, behind, ahead)
        check(load().gms_slam_set_beam_model(self._h, int(behind), int(ahead), ptr(f), modes[combine]))

    def last_align(self) -> np.ndarray:
        """gms_slam_last_align: the records of the last aligned update, ALIGN_DTYPE [n] ([n_maps][n] on a batched handle); GmsError
        (GMS_ERR_STATE) before there is one.  Waits for the stream."""
        S = int(self.params.n_maps)
        rec = np.empty((S, self.num_particles) if S > 1 else (self.num_particles,), dtype=_lib.ALIGN_DTYPE)
        check(load().gms_slam_last_align(self._h, ptr(rec)))
        return rec

    def align_form(self) -> int:
        """diagnostics: the form the handle's last alignment launch took -- GMS_SLAM_ALIGN_PLANES (the field's values computed in LDS
        from the particle's class plane) or GMS_SLAM_ALIGN_MEMORY (the field written first); 0 before the first"""
        form = C.c_int32(0)
        check(load().gms_slam_align_form(self._h, C.byref(form)))
        return int(form.value)

    def maps_copied(self) -> int:
        v = C.c_int64(0)
        check(load().gms_slam_copies(self._h, C.byref(v)))
        return int(v.value)

    def _next_sequence(self, sequence: Optional[int]) -> int:
        """the caller's sequence number, or the handle's own counter"""
        if sequence is None:
            sequence = self.sequence
            self.sequence += 1
        return int(sequence)

    @staticmethod
    def _stats_dict(st) -> dict:
        return {"weight_sum": st.weight_sum, "neff": st.neff, "strongest": st.strongest, "n_zero": st.n_zero,
                "max_log_weight": st.max_log_weight}

    def _map_of(self, slot: int, likelihood: bool) -> np.ndarray:
        out = np.empty((self.H, self.W), dtype=np.float64)
        check(load().gms_slam_download_map(self._h, int(slot), None if likelihood else ptr(out), ptr(out) if likelihood else None))
        return out

    def _set_map(self, slot: int, log, lik):
        lg = None if log is None else np.ascontiguousarray(log, dtype=np.float64)
        lk = None if lik is None else np.ascontiguousarray(lik, dtype=np.float64)
        for name, a in (("log", lg), ("lik", lk)):          # (the library copies W * H doubles from the pointer it is given)
            if a is not None and a.size != self.W * self.H:
                raise ValueError(f"set_map: {name} has {a.size} values, the map has {self.W} x {self.H} cells")
        check(load().gms_slam_upload_map(self._h, int(slot), None if lg is None else ptr(lg), None if lk is None else ptr(lk)))

    def _trace_scan(self, slot: int, z, cap: int):
        b = _beams_of(z)
        cap = int(cap) if cap > 0 else self.W + self.H + 8
        cells = np.zeros((len(b), cap, 2), dtype=np.int32)
        cls = np.zeros((len(b), cap), dtype=np.uint8)
        counts = np.zeros(len(b), dtype=np.int32)
        check(load().gms_slam_trace_scan(self._h, int(slot), ptr(b), len(b), ptr(cells), ptr(cls), cap, ptr(counts)))
        return cells, cls, counts

    def _src(self, query: str, which, filter: int) -> _Source:
        """particle `which` -- a handle-wide slot or "strongest" (of `filter`, picked on the device) -- as the source of a query"""
        return _Source("slam", self._h, _which(query, which), self.W, self.H, filter)

    def _view(self, which, filter: int, rect, decimate: int, likelihood: bool, packed: bool, out, shown_out):
        """gms_slam_view[_dev]: (image, shown)"""
        return _query_view(self._src("view", which, filter), rect, decimate, likelihood, packed, out, shown_out)

    def _cast(self, which, filter: int, probes, out, shown_out):
        """gms_slam_cast[_dev]: which = a handle-wide slot, "strongest" (of `filter`, picked on the device) or "all"; (records, shown)"""
        which = _which("cast", which, allow_all=True)
        every = which == _lib.GMS_CAST_ALL
        n_total = self.num_particles * int(self.params.n_maps)
        if out is not None:                                  # probes: (device address, B)
            dev_probes, B = probes
            check(load().gms_slam_cast_dev(self._h, which, int(filter), C.c_void_p(dev_probes), int(B),
                                           _device_ptr("cast", "out", out, 16 * (n_total if every else 1) * B), _shown_ptr("cast", shown_out)))
            return out, shown_out
        b = _beams_of(probes).reshape(-1)
        rec = np.empty((n_total, len(b)) if every else (len(b),), dtype=CAST_DTYPE)
        shown = C.c_int32(-1)
        check(load().gms_slam_cast(self._h, which, int(filter), ptr(b), len(b), ptr(rec), C.byref(shown)))
        return rec, (None if every else int(shown.value))

    def _gain(self, which, filter: int, poses, probes, max_range: int, out, shown_out):
        """gms_slam_gain[_dev]: (records, shown)"""
        return _query_gain(self._src("gain", which, filter), poses, probes, max_range, out, shown_out)

    def _rollout(self, which, filter: int, poses, arcs, points, max_range: int, inflate: int, not_free: bool, clear, cost, out, shown_out):
        """gms_slam_rollout[_dev]: (records, shown); poses None: the shown particle's own pose"""
        return _query_rollout(self._src("rollout", which, filter), poses, arcs, points, max_range, inflate, not_free, clear, cost, out, shown_out)

    def _route(self, which, filter: int, field, starts, look: int, inflate: int, not_free: bool, max_cells: int, max_waypoints: int, clear, cells, dev):
        """gms_slam_route[_dev]: (records, waypoints[, cells], shown); starts None: the shown particle's own cell"""
        return _query_route(self._src("route", which, filter), field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells, dev)

    def _warp(self, which, filter: int, dst, pose, c, s, op, rect, clamp: float, mi: int, stats, stats_out, shown_out, dev: bool):
        """gms_slam_warp[_dev]: (stats, shown)"""
        w = _warp_request(dst.W, dst.H, pose, c, s, op, rect, clamp)
        return _query_warp(self._src("warp", which, filter), dst, mi, w, stats, stats_out, shown_out, dev)

    def _locate(self, which, filter: int, offsets, rect, tol: int, not_free: bool, min_score: int, cap: int, free_only: bool, full: bool, out, n_out,
                shown_out):
        """gms_slam_locate[_dev]: (records, shown), or (out, n_out, shown_out)"""
        return _query_locate(self._src("locate", which, filter), offsets, rect, tol, not_free, min_score, cap, free_only, full, out, n_out, shown_out)

    def _clearance(self, which, filter: int, rect, max_radius: int, not_free: bool, out, shown_out):
        """gms_slam_clearance[_dev]: (field, shown)"""
        return _query_clearance(self._src("clearance", which, filter), rect, max_radius, not_free, out, shown_out)

    def _skeleton(self, which, filter: int, rect, max_radius: int, not_free: bool, min_clear: int, min_gap: int, want, dev, shown_out):
        """gms_slam_skeleton[_dev]: (site, skel, totals, shown)"""
        return _query_skeleton(self._src("skeleton", which, filter), rect, max_radius, not_free, min_clear, min_gap, want, dev, shown_out)

    def _reach(self, which, filter: int, seeds, max_cost: int, inflate: int, not_free: bool, rect, out, shown_out):
        """gms_slam_reach[_dev]: (field, shown); seeds None: the shown particle's own cell"""
        return _query_reach(self._src("reach", which, filter), seeds, max_cost, inflate, not_free, rect, out, shown_out)

    def _frontiers(self, which, filter: int, min_size: int, inflate: int, cost, rect, labels, cap: int, records_out, labels_out, shown_out):
        """gms_slam_frontiers[_dev]: (records, n_found[, labels], shown); any device tensor among the arguments: the device form"""
        dev = records_out is not None or labels_out is not None or shown_out is not None or getattr(cost, "is_cuda", False)
        return _query_frontiers(self._src("frontiers", which, filter), min_size, inflate, cost, rect, labels, cap,
                                dev=(records_out, labels_out, shown_out) if dev else None)

    def _rooms(self, which, filter: int, core: int, inflate: int, not_free: bool, min_core: int, max_cost: int, rect, want, caps, dev):
        """gms_slam_rooms[_dev]: the host form's dict with "shown", or -- dev = (labels, depth, rooms, doors, shown_out) -- (n_rooms, n_doors)"""
        return _query_rooms(self._src("rooms", which, filter), core, inflate, not_free, min_core, max_cost, rect, want, caps, dev=dev)

    def _census_request(self, min_known: int, filter: int, write_map: bool) -> _lib.GmsCensus:
        c = _lib.GmsCensus(int(min_known), int(filter), _lib.GMS_CENSUS_WRITE_MAP if write_map else 0, 0)
        check(load().gms_census_check(C.byref(c), self.num_particles, int(self.params.n_maps)))
        return c

    def _census(self, filter: int, min_known: int, counts: bool, consensus: bool, agree: bool, totals: bool, write_map: bool) -> dict:
        """gms_slam_census: the outputs asked for, by name"""
        c = self._census_request(min_known, filter, write_map)
        out = {}
        if counts:
            out["counts"] = np.empty((self.H, self.W, 2), dtype=np.uint16)
        if consensus:
            out["consensus"] = np.empty((self.H, self.W), dtype=np.uint8)
        if agree:
            out["agree"] = np.empty(self.num_particles, dtype=_lib.CENSUS_AGREE_DTYPE)
        if totals:
            out["totals"] = np.zeros((), dtype=_lib.CENSUS_TOTALS_DTYPE)
        check(load().gms_slam_census(self._h, C.byref(c), *(ptr(out[k]) if k in out else None for k in ("counts", "consensus", "agree", "totals"))))
        return out

    def _census_dev(self, filter: int, min_known: int, counts, consensus, agree, totals, write_map: bool):
        """gms_slam_census_dev on torch device tensors (None: not wanted)"""
        c = self._census_request(min_known, filter, write_map)
        cells = self.W * self.H
        check(load().gms_slam_census_dev(self._h, C.byref(c), _device_ptr("census_dev", "counts", counts, 4 * cells, optional=True),
                                         _device_ptr("census_dev", "consensus", consensus, cells, itemsize=1, optional=True),
                                         _device_ptr("census_dev", "agree", agree, _lib.CENSUS_AGREE_DTYPE.itemsize * self.num_particles, optional=True),
                                         _device_ptr("census_dev", "totals", totals, _lib.CENSUS_TOTALS_DTYPE.itemsize, optional=True)))
        return counts, consensus, agree, totals

    def set_history(self, capacity: int):
        """gms_slam_set_history: keep every particle's pose and parent slot of the last `capacity` updates on the device, through
        resampling (0: off, the memory freed).  reset() clears the history and keeps it on.  Refused on a shard of a filter."""
        check(load().gms_slam_set_history(self._h, int(capacity)))

    def history_len(self):
        """(steps_total, steps_kept): updates recorded since the history was turned on or cleared, and min(total, capacity)"""
        total, kept = C.c_int64(0), C.c_int32(0)
        check(load().gms_slam_history_len(self._h, C.byref(total), C.byref(kept)))
        return int(total.value), int(kept.value)

    def history_walk_rows(self) -> int:
        """diagnostics: the parent rows per LDS chunk of the back-trace; 0 = it chases through memory"""
        rows = C.c_int32(-1)
        check(load().gms_slam_history_walk_rows(self._h, C.byref(rows)))
        return int(rows.value)

    def _trajectory(self, which, filter: int, out, shown_out):
        """gms_slam_trajectory[_dev]: which = a handle-wide slot or "strongest" (of `filter`); (xytheta [kept][3] oldest first, shown)"""
        which = _which("trajectory", which)
        kept = self.history_len()[1]
        if out is not None:
            check(load().gms_slam_trajectory_dev(self._h, which, int(filter), _device_ptr("trajectory", "out", out, 12 * kept, itemsize=4),
                                                 out.numel() // 3, _shown_ptr("trajectory", shown_out)))
            return out, shown_out
        xy = np.empty((kept, 3), dtype=np.float32)
        count, shown = C.c_int32(0), C.c_int32(-1)
        check(load().gms_slam_trajectory(self._h, which, int(filter), ptr(xy), kept, C.byref(count), C.byref(shown)))
        return xy[:count.value], int(shown.value)

    def _trajectories(self, filter: int, ancestors: bool):
        kept = self.history_len()[1]
        xy = np.empty((kept, self.num_particles, 3), dtype=np.float32)
        anc = np.empty((kept, self.num_particles), dtype=np.int32) if ancestors else None
        count = C.c_int32(0)
        check(load().gms_slam_trajectories(self._h, int(filter), ptr(xy), ptr(anc) if ancestors else None, kept, C.byref(count)))
        return (xy, anc) if ancestors else xy

    def _last_beams(self, f: int) -> np.ndarray:
        out = np.zeros(4096, dtype=BEAM_DTYPE)                          # GMS_MAX_BEAMS
        c = C.c_int32(0)
        check(load().gms_slam_last_beams(self._h, int(f), ptr(out), len(out), C.byref(c)))
        return out[:c.value].copy()


class SLAMParticleMaps(_SlamHandle):
    """SLAM as the reference has it (J/slam/SLAM.java:26-204): num_particles particles, each with its own pose, weight AND
    GridMapData -- update() scores a particle against its own likelihood field and integrates the scan into its own map at its own
    pose (:88-107), resample() deep-copies the surviving particles' maps (:41-45).  (`SLAM` above is the shared-map filter that
    BASELINE's configurations need.)  findBestPoseOptim (:97) is left out; the motion-model draw is Philox(seed; particle, sequence)."""

    def __init__(self, width=6.0, height=6.0, resolution=0.05, position=(-3.0, -3.0), num_particles=500, device: int = 0,
                 max_beams: int = 0, kernel=None):
        self._create(width, height, resolution, position, num_particles, device, max_beams, kernel)
        self.strongest = 0
        self.neff = float(num_particles)

    def _init_shard(self, width, height, resolution, position, n_local, offset, n_global, device=0, max_beams=0, kernel=None):
        """one rank's block of a sharded filter (gms_slam_create_shard): distributed.SlamShardOps"""
        self._create(width, height, resolution, position, n_local, device or 0, max_beams, kernel, offset=offset, n_global=n_global)
        self.strongest, self.neff = 0, float(n_global)

    def update(self, z, odometry=None, seed: int = 0, sequence: Optional[int] = None, fetch: bool = True, sample_motion: bool = True):
        """update(z, u) (:80-131); odometry = (dCenter, dTheta) or None (= (0, 0) and no motion sample: `u == null` in
        sampleMotionModel, :159); sample_motion = False keeps the poses (dTheta still decides skipUpdate, :82); returns Neff"""
        b = _beams_of(z)
        have = odometry is not None and sample_motion
        dc, dt = (odometry if odometry is not None else (0.0, 0.0))
        st = GmsPfStats()
        check(load().gms_slam_update_per_particle(self._h, ptr(b), len(b), int(have), float(dc), float(dt), int(seed),
                                                  self._next_sequence(sequence), C.byref(st) if fetch else None))
        return self._fetched(st) if fetch else None

    def align(self, z, params=None, records: bool = False):
        """gms_slam_align: every particle moved, in place, by the continuous scan alignment of scan z against the field of ITS OWN map
        as logData stands (gridmapslam.h "per-particle scan alignment").  No map and no weight changes; a following
        update(sample_motion=False) weighs and integrates at the aligned poses.  records=True returns the records, ALIGN_DTYPE [n], and
        waits for the stream.  (Inside every update instead: set_align().)"""
        b = _beams_of(z).reshape(-1)
        prm = _align_params(params)
        rec = np.empty(self.num_particles, dtype=_lib.ALIGN_DTYPE) if records else None
        check(load().gms_slam_align(self._h, ptr(b), len(b), C.byref(prm), None if rec is None else ptr(rec)))
        return rec

    def align_dev(self, dev_beams: int, B: int, params=None, records_out=None):
        """align() on device-resident beams [B]; records_out: None, or a contiguous torch device tensor of n * 80 bytes, 8-byte aligned.
        Runs on the handle's stream and synchronises nothing."""
        prm = _align_params(params)
        out = _device_ptr("align_dev", "records_out", records_out, _lib.ALIGN_DTYPE.itemsize * self.num_particles, optional=True)
        check(load().gms_slam_align_dev(self._h, C.c_void_p(dev_beams), int(B), C.byref(prm), out))
        return records_out

    def score_beams(self, z, factors, behind: int, ahead: int, residuals: bool = False):
        """gms_slam_score_beams: the beam sensor model of every particle through ITS OWN map as logData stands (gridmapslam.h
        "per-particle beam sensor model"; the table, the walk and the order of ParticleFilter.score_beams).  No pose and no map
        changes.  Afterwards the filter holds RAW weights and log-weights (pf.get_weights(), pf.get_log_weights()), as a sharded
        update leaves them: pf.normalize() finishes as update() does, and resample[_if]() work after that.  residuals=True returns
        the table index per particle and beam, uint16 [n][B], and waits for the stream.  (Inside every update: set_beam_model().)"""
        b = _beams_of(z).reshape(-1)
        f = self._beam_table("score_beams", factors, behind, ahead)
        res = np.empty((self.num_particles, len(b)), dtype=np.uint16) if residuals else None
        check(load().gms_slam_score_beams(self._h, ptr(b), len(b), int(behind), int(ahead), ptr(f), None if res is None else ptr(res)))
        return res

    def score_beams_dev(self, dev_beams: int, B: int, factors, behind: int, ahead: int, residuals_out=None):
        """score_beams() on device-resident beams [B]; factors stay a host array.  residuals_out: None, or a contiguous torch device
        tensor of at least n * B 16-bit elements.  Runs on the handle's stream and synchronises nothing."""
        f = self._beam_table("score_beams_dev", factors, behind, ahead)
        out = _device_ptr("score_beams_dev", "residuals_out", residuals_out, 2 * self.num_particles * int(B), optional=True)
        check(load().gms_slam_score_beams_dev(self._h, C.c_void_p(dev_beams), int(B), int(behind), int(ahead), ptr(f), out))
        return residuals_out

    def _fetched(self, st) -> float:
        self.strongest, self.neff = st.strongest, st.neff
        self.last_stats = self._stats_dict(st)
        return st.neff

    def update_dev(self, dev_beams: int, B: int, odometry=None, seed: int = 0, sequence: int = 0, sample_motion: bool = True):
        have = odometry is not None and sample_motion
        dc, dt = (odometry if odometry is not None else (0.0, 0.0))
        check(load().gms_slam_update_per_particle_dev(self._h, C.c_void_p(dev_beams), B, int(have), float(dc), float(dt), int(seed),
                                                      int(sequence), None))

    def frame(self, angles, distances, hits, d_center: float, d_theta: float, seed: int = 0, sequence: Optional[int] = None,
              r01: Optional[float] = None, fraction: float = 0.5, fetch: bool = False):
        """One recorded revolution as GridMapApp.onHandleData treats it (J/app/GridMapApp.java:133-192) in one call: the de-skew of the
        raw measurements (:143-175), update(z, u) (:178) and `if (neff < fraction * n) resample()` (:185-186; fraction < 0: no
        resampling).  The same bits as grid_map.deskew -> update_dev -> resample_if.  fetch: returns update()'s Neff (synchronises)."""
        a = np.ascontiguousarray(angles, dtype=np.float64)
        d = np.ascontiguousarray(distances, dtype=np.float64)
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        if not (a.ndim == d.ndim == h.ndim == 1 and a.size == d.size == h.size):
            raise ValueError("frame: angles, distances and hits must be one-dimensional and of one length")
        sequence = self._next_sequence(sequence)
        r = float(np.random.random() if r01 is None else r01)
        st = GmsPfStats()
        check(load().gms_slam_frame_per_particle(self._h, ptr(a), ptr(d), ptr(h), a.size, float(d_center), float(d_theta), int(seed),
                                                 sequence, r, float(fraction), C.byref(st) if fetch else None))
        return self._fetched(st) if fetch else None

    def last_beams(self) -> np.ndarray:
        """the de-skewed revolution of the last frame() call (diagnostics; synchronises)"""
        return self._last_beams(0)

    def resample(self, r01: Optional[float] = None, want_indices: bool = False):
        """resample() (:133-153): r01 stands for Math.random()"""
        r = float(np.random.random() if r01 is None else r01)
        idx = np.empty(self.num_particles, dtype=np.int32) if want_indices else None
        amb = C.c_int32(0)
        check(load().gms_slam_resample_maps(self._h, r, ptr(idx) if want_indices else None, C.byref(amb) if want_indices else None))
        return (idx, amb.value) if want_indices else None

    def resample_if(self, r01: Optional[float] = None, fraction: float = 0.5):
        """`if (neff < fraction * n) resample()` (GridMapApp.java:185-186) decided on the device from the last update's Neff: no host
        round trip (update_dev + resample_if is one revolution); pf.last_resample_indices() tells afterwards what happened"""
        r = float(np.random.random() if r01 is None else r01)
        check(load().gms_slam_resample_maps_if(self._h, r, float(fraction)))

    def get_weighted_pose(self) -> np.ndarray:
        return self.pf.weighted_pose()                                                                   # :165-178

    def calculate_neff(self) -> float:
        return self.pf.stats()["neff"]                                                                   # :180-190

    def get_particles(self):
        """(poses [n][3], weights [n]); the maps: map_of(i) / maps()"""
        return self.pf.get_particles()                                                                   # :192

    def set_poses(self, xytheta):
        self.pf.set_poses(xytheta)

    def map_of(self, i: int, likelihood: bool = False) -> np.ndarray:
        """Particle i's logData (or likelihoodData) as [H][W] (Particle.m, :33)"""
        return self._map_of(i, likelihood)

    def maps(self, likelihood: bool = False) -> np.ndarray:
        out = np.empty((self.num_particles, self.H, self.W), dtype=np.float64)
        check(load().gms_slam_download_maps(self._h, None if likelihood else ptr(out), ptr(out) if likelihood else None))
        return out

    def set_map(self, i: int, log=None, lik=None):
        self._set_map(i, log, lik)

    def view(self, which="strongest", rect=None, decimate: int = 1, likelihood: bool = False, packed: bool = False, out=None, shown_out=None):
        """GridMapApp.render's "strongest" / "chosen particle" cases (J/app/GridMapApp.java:374-393) through GridMap.render
        (GridMap.java:371-388), on the device: (image, shown) -- the grey levels of particle `which`'s map as GridMap.view makes them, and
        the particle that was drawn.  which = "strongest": the strongest particle of the last update (:110-115), picked on the device
        without a read-back (GmsError GMS_ERR_STATE before the first update and after reset()).  out / shown_out: torch device tensors
        for the picture and the int32 index (nothing is synchronised).  The combined map: calculate_combined(), then grid_map.view()."""
        return self._view(which, 0, rect, decimate, likelihood, packed, out, shown_out)

    def cast(self, probes, which="strongest", out=None, shown_out=None):
        """The predicted scan of particles at THEIR OWN pose in THEIR OWN map (gridmapslam.h "predicted scans"; GridMap.cast's records):
        which = a particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update):
        (records [B], shown); which = "all": (records [n][B], None).  out / shown_out: torch device tensors, probes then
        (device address, B); nothing is synchronised."""
        return self._cast(which, 0, probes, out, shown_out)

    def clearance(self, which="strongest", rect=None, max_radius: int = 25, not_free: bool = False, out=None, shown_out=None):
        """The clearance field of particle `which`'s OWN map (GridMap.clearance's values): (field uint16 [h][w], shown).  which = a
        particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  out /
        shown_out: torch device tensors for the field and the int32 index; nothing is synchronised."""
        return self._clearance(which, 0, rect, max_radius, not_free, out, shown_out)

    def skeleton(self, which="strongest", rect=None, max_radius: int = 25, not_free: bool = False, min_clear: int = 1, min_gap: int = 2,
                 site: bool = True, skel: bool = True, totals: bool = True, dev=None, shown_out=None):
        """Sites and skeleton of particle `which`'s OWN map (GridMap.skeleton's values): (site, skel, totals, shown).  which = a
        particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  dev: the
        device form, (site, skel, totals) torch device tensors (None: not computed), and shown_out the int32 index; nothing is
        synchronised."""
        return self._skeleton(which, 0, rect, max_radius, not_free, min_clear, min_gap, (site, skel, totals), dev, shown_out)

    def reach(self, which="strongest", seeds=None, max_cost: int = 0xFFFE, inflate: int = 0, not_free: bool = True, rect=None, out=None,
              shown_out=None):
        """The cost-to-go field of particle `which`'s OWN map (GridMap.reach's values): (field uint16 [h][w], shown).  which = a
        particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  seeds=None:
        the shown particle's own pose cell, picked on the device.  out / shown_out: torch device tensors (seeds then a device int32
        tensor or None).  Diagnostics: grid_map.reach_stats()."""
        return self._reach(which, 0, seeds, max_cost, inflate, not_free, rect, out, shown_out)

    def frontiers(self, which="strongest", min_size: int = 1, inflate: int = 0, cost=None, rect=None, labels: bool = False, cap: int = 4096,
                  records_out=None, labels_out=None, shown_out=None):
        """The frontier regions of particle `which`'s OWN map (GridMap.frontiers' values): (records, n_found[, labels], shown).  which =
        a particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  cost: that
        particle's whole-map field, as reach() returns it.  records_out / labels_out / shown_out (torch device tensors, cost then a
        device tensor or None): the device form, which returns n_found alone."""
        return self._frontiers(which, 0, min_size, inflate, cost, rect, labels, cap, records_out, labels_out, shown_out)

    def rooms(self, which="strongest", core: int = 15, inflate: int = 5, not_free: bool = True, min_core: int = 1, max_cost: int = 0xFFFE, rect=None,
              labels: bool = True, depth: bool = False, cap_rooms: int = 1024, cap_doors: int = 4096) -> dict:
        """Rooms and doors of particle `which`'s OWN map (GridMap.rooms' dict, with "shown": the particle that was read).  which = a
        particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).
        Diagnostics: grid_map.rooms_stats()."""
        return self._rooms(which, 0, core, inflate, not_free, min_core, max_cost, rect, (labels, depth), (cap_rooms, cap_doors), None)

    def rooms_dev(self, which="strongest", labels=None, depth=None, rooms=None, doors=None, shown_out=None, core: int = 15, inflate: int = 5,
                  not_free: bool = True, min_core: int = 1, max_cost: int = 0xFFFE, rect=None) -> tuple:
        """rooms() into torch device tensors (GridMap.rooms_dev's), shown_out the int32 index; returns (n_rooms, n_doors)"""
        return self._rooms(which, 0, core, inflate, not_free, min_core, max_cost, rect, None, None, (labels, depth, rooms, doors, shown_out))

    def gain(self, poses, probes, max_range: int, which="strongest", out=None, shown_out=None):
        """The view gain of the CALLER'S candidate poses [P][3] in particle `which`'s OWN map (GridMap.gain's records): (records [P],
        shown).  which = a particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first
        update).  out / shown_out: torch device tensors, poses and probes then (device address, P) and (device address, B); nothing
        is synchronised."""
        return self._gain(which, 0, poses, probes, max_range, out, shown_out)

    def rollout(self, arcs, points=None, poses=None, which="strongest", max_range: int = 255, inflate: int = 0, not_free: bool = True, clear=None,
                cost=None):
        """Trajectory rollouts in particle `which`'s OWN map (GridMap.rollout's records): (records [P][K], shown).  which = a particle
        index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  poses=None: ONE start
        pose, the shown particle's own, read on the device; records [1][K]."""
        return self._rollout(which, 0, poses, arcs, points, max_range, inflate, not_free, clear, cost, None, None)

    def rollout_dev(self, out, arcs, points=None, poses=None, which="strongest", max_range: int = 255, inflate: int = 0, not_free: bool = True,
                    clear=None, cost=None, shown_out=None):
        """rollout() on the device: arcs = (device address, K, T), points = (device address, F) or None, poses = (device address, P) or
        None, clear / cost / out / shown_out torch device tensors; (out, shown_out), nothing is synchronised"""
        return self._rollout(which, 0, poses, arcs, points, max_range, inflate, not_free, clear, cost, out, shown_out)

    def route(self, field, starts=None, which="strongest", *, look: int = 64, inflate: int = 0, not_free: bool = True, max_cells: int = 4096,
              max_waypoints: int = 64, clear=None, cells: bool = False):
        """Routes through particle `which`'s OWN map over that particle's field (GridMap.route's values): (records, waypoints[, cells],
        shown).  which = a particle index or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first
        update).  starts=None: ONE start, the shown particle's own pose cell, read on the device."""
        return self._route(which, 0, field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells, None)

    def route_dev(self, field, out, waypoints, starts=None, which="strongest", *, look: int = 64, inflate: int = 0, not_free: bool = True,
                  max_cells: int = 4096, max_waypoints: int = 64, clear=None, cells=None, shown_out=None):
        """route() on torch device tensors (GridMap.route_dev's): (out, waypoints[, cells], shown_out), nothing is synchronised"""
        return self._route(which, 0, field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells, (out, waypoints, shown_out))

    def warp_into(self, dst: GridMap, which="strongest", pose=None, *, c=None, s=None, op="compare", rect=None, clamp: float = 0.0, mi: int = 0,
                  stats: bool = True):
        """Particle `which`'s OWN map read through a rigid transform into map mi of dst (GridMap.warp_from's arguments, pose: this
        filter's world frame in dst's world): (stats, shown).  which = a particle index or "strongest" (picked on the device as
        view() picks it, GMS_ERR_STATE before the first update).  The filter is only read; dst may not be its own grid_map."""
        return self._warp(which, 0, dst, pose, c, s, op, rect, clamp, mi, stats, None, None, False)

    def warp_into_dev(self, dst: GridMap, stats_out, which="strongest", pose=None, *, c=None, s=None, op="compare", rect=None, clamp: float = 0.0,
                      mi: int = 0, shown_out=None):
        """warp_into() on dst's stream: stats_out / shown_out torch device tensors (80 bytes, 8-byte aligned; int32) or None;
        (stats_out, shown_out), nothing is synchronised"""
        return self._warp(which, 0, dst, pose, c, s, op, rect, clamp, mi, False, stats_out, shown_out, True)

    def locate(self, offsets, which="strongest", rect=None, tol: int = 1, not_free: bool = False, min_score: int = 1, cap: int = 64,
               free_only: bool = True, full: bool = False, out=None, n_out=None, shown_out=None):
        """Global scan matching in particle `which`'s OWN map (GridMap.locate's records): (records, shown).  which = a particle index
        or "strongest" (picked on the device as view() picks it, GMS_ERR_STATE before the first update).  out / n_out / shown_out:
        torch device tensors, offsets then (device address, n_theta, B); returns (out, n_out, shown_out).  Diagnostics:
        grid_map.locate_stats()."""
        return self._locate(which, 0, offsets, rect, tol, not_free, min_score, cap, free_only, full, out, n_out, shown_out)

    def trajectory(self, which="strongest", out=None, shown_out=None):
        """(xytheta [kept][3], shown): the path particle `which` (a slot, or "strongest" as view() picks it) descends along, oldest
        first over the kept updates of set_history() -- the path its map was built along, whatever resampling did to the slots since.
        out / shown_out: torch device tensors (float32 [>= kept][3], int32); nothing is synchronised."""
        return self._trajectory(which, 0, out, shown_out)

    def trajectories(self, ancestors: bool = False):
        """every particle's path at once: xytheta [kept][n][3]; ancestors: also [kept][n], the slot present particle k occupied at
        each kept update"""
        return self._trajectories(0, ancestors)

    def calculate_combined(self) -> np.ndarray:
        """GridMapApp.calculateCombined (J/app/GridMapApp.java:439-458): the combined logData [H][W]; the likelihood field of it is
        grid_map.download_likelihood()"""
        check(load().gms_slam_combined(self._h))
        return self.grid_map.download_log()

    def census(self, min_known: int = 1, counts: bool = True, consensus: bool = True, agree: bool = False, totals: bool = True,
               write_map: bool = False) -> dict:
        """The census of the particles' maps (gridmapslam.h "census of the particles' maps"): what the ENSEMBLE says, cell by cell.
        A dict of the outputs asked for -- "counts" uint16 [H][W][2] = {particles that hold the cell free, occupied}; "consensus" uint8
        [H][W], 0 unknown where fewer than min_known particles know the cell, else 2 occupied where oc >= fr, else 1 free; "totals" a
        CENSUS_TOTALS_DTYPE record; "agree" CENSUS_AGREE_DTYPE [n], every particle's pair[its class][the consensus class] over all
        cells (census_outliers()).  write_map: the consensus is also written, as +1.0 / -1.0 / +0.0, to grid_map's own logData, where
        every GridMap query then works on it.  The map uncertainty: census_entropy(counts, n).  The filter is only read."""
        return self._census(0, min_known, counts, consensus, agree, totals, write_map)

    def census_dev(self, min_known: int = 1, counts=None, consensus=None, agree=None, totals=None, write_map: bool = False):
        """census() into torch device tensors (None: not wanted) -- counts of W * H * 4 bytes and agree of n * 40 bytes, 4-byte
        aligned; consensus of W * H bytes; totals of 32 bytes, 8-byte aligned -- on the handle's stream: nothing is synchronised."""
        return self._census_dev(0, min_known, counts, consensus, agree, totals, write_map)

    def trace_scan(self, i: int, z, cap: int = 0):
        """(cells [B][cap][2], classes [B][cap], counts [B]): the cell walk of integrateObservation for particle i at its current pose
        as the update kernel walks and classifies it (prior-class visits included), in walk order; nothing is written to a map"""
        return self._trace_scan(i, z, cap)

    def get_strongest_particle(self) -> int:
        return self.strongest                                                                            # :196

    def get_grid_map(self) -> GridMap:
        return self.grid_map                                                                             # :200

    getWeightedPose = get_weighted_pose
    calculateNeff = calculate_neff
    getParticles = get_particles
    getStrongestParticle = get_strongest_particle
    getGridMap = get_grid_map


class SLAMParticleMapsBatch(_SlamHandle):
    """num_filters independent SLAMParticleMaps filters in ONE handle (gms_slam_create with gms_params.n_maps = S): every update and
    resampling step is one launch of each kernel for all of them, and filter f computes, bit for bit, what a stand-alone
    SLAMParticleMaps would from the same scans, odometry and seed.  Filter-local particle indices throughout."""

    def __init__(self, num_filters: int, width=6.0, height=6.0, resolution=0.05, position=(-3.0, -3.0), num_particles=500,
                 device: int = 0, max_beams: int = 0, kernel=None):
        self.num_filters = int(num_filters)
        self._create(width, height, resolution, position, num_particles, device, max_beams, kernel, n_maps=num_filters)
        self.strongest = np.zeros(self.num_filters, dtype=np.int64)
        self.neff = np.full(self.num_filters, float(num_particles))

    def _per_filter(self, v, dtype):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (self.num_filters,)))

    def update(self, scans, odometry=None, seeds=0, sequence: Optional[int] = None, fetch: bool = True, sample_motion=True):
        """update(z, u) of every filter: scans = S scans (each an Observation or a beam array of its own length), odometry = None or S
        entries of (dCenter, dTheta) or None (as SLAMParticleMaps.update), seeds = S seeds (or one for all), sample_motion = S flags (or
        one).  Returns the filters' Neff [S] (fetch)."""
        S = self.num_filters
        if len(scans) != S:
            raise ValueError(f"update: {len(scans)} scans for {S} filters")
        bs = [_beams_of(z) for z in scans]
        counts = np.array([len(b) for b in bs], dtype=np.int32)
        B = int(counts.max()) if S else 0
        block = np.zeros((S, max(B, 1)), dtype=BEAM_DTYPE)
        for f, b in enumerate(bs):
            block[f, :len(b)] = b
        odo = [None] * S if odometry is None else list(odometry)
        if len(odo) != S:
            raise ValueError(f"update: {len(odo)} odometry entries for {S} filters")
        u = np.array([(0.0, 0.0) if o is None else (float(o[0]), float(o[1])) for o in odo], dtype=np.float64).reshape(S, 2)
        sm = self._per_filter(sample_motion, np.int32) != 0
        have = np.array([o is not None for o in odo]) & sm
        have = np.ascontiguousarray(have.astype(np.int32))
        sd = self._per_filter(seeds, np.uint64)
        st = (GmsPfStats * S)()
        check(load().gms_slam_update_batch(self._h, ptr(block), B, ptr(counts), ptr(u), ptr(sd), ptr(have), self._next_sequence(sequence),
                                           st if fetch else None))
        return self._fetched(st) if fetch else None

    def _fetched(self, st) -> np.ndarray:
        self.last_stats = [self._stats_dict(s) for s in st]
        self.strongest = np.array([s.strongest for s in st], dtype=np.int64)       # (filter-local)
        self.neff = np.array([s.neff for s in st], dtype=np.float64)
        return self.neff.copy()

    def update_dev(self, dev_beams: int, B: int, counts=None, odometry=None, seeds=0, sequence: int = 0, sample_motion=True):
        """the same on device beams [S][B] (row pitch B); counts [S] or None (all B); odometry [S][2] or None (no motion)"""
        S = self.num_filters
        c = None if counts is None else self._per_filter(counts, np.int32)
        u = np.zeros((S, 2)) if odometry is None else np.ascontiguousarray(np.asarray(odometry, dtype=np.float64).reshape(S, 2))
        have = self._per_filter(sample_motion, np.int32) * (0 if odometry is None else 1)
        have = np.ascontiguousarray(have.astype(np.int32))
        check(load().gms_slam_update_batch_dev(self._h, C.c_void_p(dev_beams), int(B), None if c is None else ptr(c), ptr(u),
                                               ptr(self._per_filter(seeds, np.uint64)), ptr(have), int(sequence), None))

    def frame(self, angles, distances, hits, odometry, seeds=0, sequence: Optional[int] = None, r01=None, fraction: float = 0.5,
              lengths=None, fetch: bool = False):
        """One recorded revolution per filter (GridMapApp.java:133-192) in one call: angles / distances / hits [S][L], filter f's
        revolution its first lengths[f] measurements (None: all L), de-skewed with its own length and odometry[f] = (dCenter, dTheta),
        then update(z, u) of every filter and the rule `if (neff < fraction * n) resample()` per filter (fraction < 0: no resampling).
        Filter f computes what a stand-alone SLAMParticleMaps.frame does.  fetch: the filters' Neff [S] (synchronises)."""
        S = self.num_filters
        a = np.ascontiguousarray(angles, dtype=np.float64)
        d = np.ascontiguousarray(distances, dtype=np.float64)
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        if not (a.ndim == 2 and a.shape[0] == S and a.shape == d.shape == h.shape):
            raise ValueError(f"frame: angles, distances and hits must be [S][L] arrays of one shape for {S} filters")
        u = np.ascontiguousarray(np.asarray(odometry, dtype=np.float64).reshape(S, 2))
        ln = None if lengths is None else self._per_filter(lengths, np.int32)
        sd = self._per_filter(seeds, np.uint64)
        r = self._per_filter(np.random.random(S) if r01 is None else r01, np.float64)
        st = (GmsPfStats * S)()
        check(load().gms_slam_frame_batch(self._h, ptr(a), ptr(d), ptr(h), a.shape[1], None if ln is None else ptr(ln), ptr(u), ptr(sd),
                                          self._next_sequence(sequence), ptr(r), float(fraction), st if fetch else None))
        return self._fetched(st) if fetch else None

    def last_beams(self, f: int) -> np.ndarray:
        """filter f's de-skewed revolution of the last frame() call (diagnostics; synchronises)"""
        return self._last_beams(f)

    def resample(self, r01=None, want_indices: bool = False):
        """resample() of every filter; r01 [S] (or one for all).  want_indices: (indices [S][n] filter-local, n_ambiguous [S])"""
        r = self._per_filter(np.random.random(self.num_filters) if r01 is None else r01, np.float64)
        if not want_indices:
            check(load().gms_slam_resample_maps_batch(self._h, ptr(r), None, None))
            return None
        idx = np.empty((self.num_filters, self.num_particles), dtype=np.int32)
        amb = np.empty(self.num_filters, dtype=np.int32)
        check(load().gms_slam_resample_maps_batch(self._h, ptr(r), ptr(idx), ptr(amb)))
        return idx, amb

    def resample_if(self, r01=None, fraction: float = 0.5):
        """`if (neff < fraction * n) resample()` per filter, decided on the device; did_resample() / last_resample_indices() tell"""
        r = self._per_filter(np.random.random(self.num_filters) if r01 is None else r01, np.float64)
        check(load().gms_slam_resample_maps_if_batch(self._h, ptr(r), float(fraction)))

    def did_resample(self) -> np.ndarray:
        return np.asarray(self.pf.did_resample(), dtype=bool).reshape(self.num_filters)

    def last_resample_indices(self) -> np.ndarray:
        return self.pf.last_resample_indices().reshape(self.num_filters, self.num_particles)

    def get_weighted_pose(self) -> np.ndarray:
        return np.asarray(self.pf.weighted_pose()).reshape(self.num_filters, 3)

    def calculate_neff(self) -> np.ndarray:
        st = self.pf.stats()
        st = st if isinstance(st, list) else [st]
        return np.array([s["neff"] for s in st], dtype=np.float64)

    def get_particles(self):
        """(poses [S][n][3], weights [S][n])"""
        poses, w = self.pf.get_particles()
        return poses.reshape(self.num_filters, self.num_particles, 3), w.reshape(self.num_filters, self.num_particles)

    def set_poses(self, xytheta):
        self.pf.set_poses(xytheta)

    def _slot(self, f: int, i: int) -> int:
        if not (0 <= f < self.num_filters and 0 <= i < self.num_particles):
            raise IndexError(f"particle {i} of filter {f}: out of range ({self.num_filters} x {self.num_particles})")
        return int(f) * self.num_particles + int(i)

    def _local(self, filter: int, which=None):
        """what a filter-local request passes on as `which`: a FILTER-LOCAL particle index as the handle-wide slot, anything else
        ("strongest", "all", None: the filter as a whole) as it is, its filter range-checked"""
        if which is not None and not isinstance(which, str):
            return self._slot(filter, which)
        if not 0 <= filter < self.num_filters:
            raise IndexError(f"filter {filter} out of range ({self.num_filters})")
        return which

    def map_of(self, f: int, i: int, likelihood: bool = False) -> np.ndarray:
        """filter f's particle i's logData (or likelihoodData) as [H][W]"""
        return self._map_of(self._slot(f, i), likelihood)

    def maps(self, f: Optional[int] = None, likelihood: bool = False) -> np.ndarray:
        """filter f's maps [n][H][W]; f = None: every filter's [S][n][H][W]"""
        out = np.empty((self.num_filters, self.num_particles, self.H, self.W), dtype=np.float64)
        check(load().gms_slam_download_maps(self._h, None if likelihood else ptr(out), ptr(out) if likelihood else None))
        return out if f is None else out[int(f)]

    def set_map(self, f: int, i: int, log=None, lik=None):
        self._set_map(self._slot(f, i), log, lik)

    def view(self, which="strongest", filter: int = 0, rect=None, decimate: int = 1, likelihood: bool = False, packed: bool = False, out=None,
             shown_out=None):
        """SLAMParticleMaps.view for filter `filter`: which = "strongest" (that filter's, picked on the device) or a FILTER-LOCAL particle
        index.  shown is the handle-wide slot filter * num_particles + k that was drawn (the index space of gms_slam_download_map)."""
        return self._view(self._local(filter, which), filter, rect, decimate, likelihood, packed, out, shown_out)

    def cast(self, probes, which="strongest", filter: int = 0, out=None, shown_out=None):
        """SLAMParticleMaps.cast for filter `filter`: which = "strongest" (that filter's), a FILTER-LOCAL particle index, or "all":
        every particle of EVERY filter, records [S * n][B] in handle-wide slot order; shown is the handle-wide slot, as view() reports it"""
        return self._cast(self._local(filter, which), filter, probes, out, shown_out)

    def clearance(self, which="strongest", filter: int = 0, rect=None, max_radius: int = 25, not_free: bool = False, out=None, shown_out=None):
        """SLAMParticleMaps.clearance for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown
        is the handle-wide slot filter * num_particles + k whose field was made, as view() reports it"""
        return self._clearance(self._local(filter, which), filter, rect, max_radius, not_free, out, shown_out)

    def skeleton(self, which="strongest", filter: int = 0, rect=None, max_radius: int = 25, not_free: bool = False, min_clear: int = 1,
                 min_gap: int = 2, site: bool = True, skel: bool = True, totals: bool = True, dev=None, shown_out=None):
        """SLAMParticleMaps.skeleton for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown
        is the handle-wide slot filter * num_particles + k whose map was read, as view() reports it"""
        return self._skeleton(self._local(filter, which), filter, rect, max_radius, not_free, min_clear, min_gap, (site, skel, totals), dev, shown_out)

    def reach(self, which="strongest", filter: int = 0, seeds=None, max_cost: int = 0xFFFE, inflate: int = 0, not_free: bool = True, rect=None,
              out=None, shown_out=None):
        """SLAMParticleMaps.reach for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown is
        the handle-wide slot filter * num_particles + k whose field was made, as view() reports it"""
        return self._reach(self._local(filter, which), filter, seeds, max_cost, inflate, not_free, rect, out, shown_out)

    def frontiers(self, which="strongest", filter: int = 0, min_size: int = 1, inflate: int = 0, cost=None, rect=None, labels: bool = False,
                  cap: int = 4096, records_out=None, labels_out=None, shown_out=None):
        """SLAMParticleMaps.frontiers for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown
        is the handle-wide slot filter * num_particles + k whose regions were made, as view() reports it"""
        return self._frontiers(self._local(filter, which), filter, min_size, inflate, cost, rect, labels, cap, records_out, labels_out, shown_out)

    def rooms(self, which="strongest", filter: int = 0, core: int = 15, inflate: int = 5, not_free: bool = True, min_core: int = 1,
              max_cost: int = 0xFFFE, rect=None, labels: bool = True, depth: bool = False, cap_rooms: int = 1024, cap_doors: int = 4096) -> dict:
        """SLAMParticleMaps.rooms for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; "shown"
        is the handle-wide slot filter * num_particles + k whose map was read, as view() reports it"""
        return self._rooms(self._local(filter, which), filter, core, inflate, not_free, min_core, max_cost, rect, (labels, depth), (cap_rooms, cap_doors), None)

    def rooms_dev(self, which="strongest", filter: int = 0, labels=None, depth=None, rooms=None, doors=None, shown_out=None, core: int = 15,
                  inflate: int = 5, not_free: bool = True, min_core: int = 1, max_cost: int = 0xFFFE, rect=None) -> tuple:
        """SLAMParticleMaps.rooms_dev for filter `filter`"""
        return self._rooms(self._local(filter, which), filter, core, inflate, not_free, min_core, max_cost, rect, None, None,
                           (labels, depth, rooms, doors, shown_out))

    def gain(self, poses, probes, max_range: int, which="strongest", filter: int = 0, out=None, shown_out=None):
        """SLAMParticleMaps.gain for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown is
        the handle-wide slot filter * num_particles + k in whose map the poses were judged, as view() reports it"""
        return self._gain(self._local(filter, which), filter, poses, probes, max_range, out, shown_out)

    def rollout(self, arcs, points=None, poses=None, which="strongest", filter: int = 0, max_range: int = 255, inflate: int = 0, not_free: bool = True,
                clear=None, cost=None):
        """SLAMParticleMaps.rollout for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown is
        the handle-wide slot filter * num_particles + k in whose map the arcs were rolled, as view() reports it"""
        return self._rollout(self._local(filter, which), filter, poses, arcs, points, max_range, inflate, not_free, clear, cost, None, None)

    def rollout_dev(self, out, arcs, points=None, poses=None, which="strongest", filter: int = 0, max_range: int = 255, inflate: int = 0,
                    not_free: bool = True, clear=None, cost=None, shown_out=None):
        """SLAMParticleMaps.rollout_dev for filter `filter`"""
        return self._rollout(self._local(filter, which), filter, poses, arcs, points, max_range, inflate, not_free, clear, cost, out, shown_out)

    def route(self, field, starts=None, which="strongest", filter: int = 0, *, look: int = 64, inflate: int = 0, not_free: bool = True,
              max_cells: int = 4096, max_waypoints: int = 64, clear=None, cells: bool = False):
        """SLAMParticleMaps.route for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown is
        the handle-wide slot filter * num_particles + k through whose map the routes were taken, as view() reports it"""
        return self._route(self._local(filter, which), filter, field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells, None)

    def route_dev(self, field, out, waypoints, starts=None, which="strongest", filter: int = 0, *, look: int = 64, inflate: int = 0,
                  not_free: bool = True, max_cells: int = 4096, max_waypoints: int = 64, clear=None, cells=None, shown_out=None):
        """SLAMParticleMaps.route_dev for filter `filter`"""
        return self._route(self._local(filter, which), filter, field, starts, look, inflate, not_free, max_cells, max_waypoints, clear, cells,
                           (out, waypoints, shown_out))

    def warp_into(self, dst: GridMap, which="strongest", filter: int = 0, pose=None, *, c=None, s=None, op="compare", rect=None, clamp: float = 0.0,
                  mi: int = 0, stats: bool = True):
        """SLAMParticleMaps.warp_into for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown
        is the handle-wide slot filter * num_particles + k whose map was read, as view() reports it"""
        return self._warp(self._local(filter, which), filter, dst, pose, c, s, op, rect, clamp, mi, stats, None, None, False)

    def warp_into_dev(self, dst: GridMap, stats_out, which="strongest", filter: int = 0, pose=None, *, c=None, s=None, op="compare", rect=None,
                      clamp: float = 0.0, mi: int = 0, shown_out=None):
        """SLAMParticleMaps.warp_into_dev for filter `filter`"""
        return self._warp(self._local(filter, which), filter, dst, pose, c, s, op, rect, clamp, mi, False, stats_out, shown_out, True)

    def locate(self, offsets, which="strongest", filter: int = 0, rect=None, tol: int = 1, not_free: bool = False, min_score: int = 1, cap: int = 64,
               free_only: bool = True, full: bool = False, out=None, n_out=None, shown_out=None):
        """SLAMParticleMaps.locate for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown is
        the handle-wide slot filter * num_particles + k in whose map the scan was matched, as view() reports it"""
        return self._locate(self._local(filter, which), filter, offsets, rect, tol, not_free, min_score, cap, free_only, full, out, n_out, shown_out)

    def trajectory(self, which="strongest", filter: int = 0, out=None, shown_out=None):
        """SLAMParticleMaps.trajectory for filter `filter`: which = "strongest" (that filter's) or a FILTER-LOCAL particle index; shown
        is the handle-wide slot that was followed, as view() reports it"""
        return self._trajectory(self._local(filter, which), filter, out, shown_out)

    def trajectories(self, f: int, ancestors: bool = False):
        """filter f's particles' paths: xytheta [kept][n][3] (and, ancestors, the filter-local slots [kept][n])"""
        self._local(f)
        return self._trajectories(f, ancestors)

    def calculate_combined(self, f: int, likelihood: bool = False) -> np.ndarray:
        """GridMapApp.calculateCombined over filter f's particles: its logData [H][W] (likelihood: the field of it)"""
        self._local(f)
        check(load().gms_slam_combined(self._h))
        out = self.grid_map.download_likelihood() if likelihood else self.grid_map.download_log()
        return out.reshape(self.num_filters, self.H, self.W)[int(f)]

    def census(self, filter: int = 0, min_known: int = 1, counts: bool = True, consensus: bool = True, agree: bool = False, totals: bool = True,
               write_map: bool = False) -> dict:
        """SLAMParticleMaps.census over filter `filter`'s particles alone; write_map writes map `filter` of grid_map, the others stay"""
        self._local(filter)
        return self._census(filter, min_known, counts, consensus, agree, totals, write_map)

    def census_dev(self, filter: int = 0, min_known: int = 1, counts=None, consensus=None, agree=None, totals=None, write_map: bool = False):
        """SLAMParticleMaps.census_dev for filter `filter`"""
        self._local(filter)
        return self._census_dev(filter, min_known, counts, consensus, agree, totals, write_map)

    def trace_scan(self, f: int, i: int, z, cap: int = 0):
        return self._trace_scan(self._slot(f, i), z, cap)
