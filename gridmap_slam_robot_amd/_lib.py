"""ctypes binding of libgridmapslam.so -- the C-ABI declared in include/gridmapslam.h.

The library is the product: there is no Python or CPU fallback.  Loading fails loudly when the
shared object has not been built (`python -m gridmap_slam_robot_amd.build`), and every compute call
fails with GMS_ERR_NO_DEVICE when no HIP device is visible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgridmapslam.so")
if os.environ.get("GMS_LIBRARY"):          # experiments only (tools/ab_compare.sh alternates two builds on one box)
    LIB_PATH = os.environ["GMS_LIBRARY"]

GMS_MAX_TAPS = 129
GMS_BLOCK = 256
GMS_PARTIAL_STRIDE = 9
PACKED_BYTES = 24

GMS_OK, GMS_ERR_INVALID, GMS_ERR_NO_DEVICE, GMS_ERR_HIP, GMS_ERR_NOMEM, GMS_ERR_STATE, GMS_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6
K_RAYCAST, K_APPLY, K_LIKELIHOOD, K_SCORE, K_REDUCE, K_RESAMPLE, K_REFINE, K_EXCHANGE, K_ORDER, K_MAPCOPY, K_COUNT = range(11)   # enum of gridmapslam.h (GMS_K_*)
KERNEL_NAMES = ["raycast", "apply", "likelihood", "score", "reduce", "resample", "refine", "exchange", "order", "mapcopy"]
assert len(KERNEL_NAMES) == K_COUNT

BEAM_DTYPE = np.dtype(
    [("local_x", "<f8"), ("local_y", "<f8"), ("distance", "<f8"), ("hit", "u1"), ("pad_", "u1", (7,))]
)
CAST_DTYPE = np.dtype([("step", "<i4"), ("x", "<i4"), ("y", "<i4"), ("range", "<f4")])      # gms_cast_hit, 16 bytes
PACKED_DTYPE = np.dtype([("w", "<f8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("pad", "<u4")])


class GmsParams(C.Structure):
    _fields_ = [
        ("width_m", C.c_float), ("height_m", C.c_float), ("resolution", C.c_float),
        ("pos_x", C.c_float), ("pos_y", C.c_float),
        ("n_maps", C.c_int32), ("device", C.c_int32),
        ("l_free", C.c_double), ("l_occ", C.c_double),
        ("ktaps", C.c_int32),
        ("kernel", C.c_double * GMS_MAX_TAPS),
        ("extra_steps", C.c_int32), ("hit_tolerance", C.c_float),
        ("z_hit", C.c_double), ("z_random", C.c_double),
        ("max_range", C.c_float), ("max_beams", C.c_int32),
    ]


class GmsPfStats(C.Structure):
    _fields_ = [
        ("weight_sum", C.c_double), ("neff", C.c_double),
        ("strongest", C.c_int32), ("n_zero", C.c_int32),
        ("max_log_weight", C.c_double),
    ]


class GmsView(C.Structure):
    """gms_view: a rectangle of a map as grey levels (gridmapslam.h "map views")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("decimate", C.c_int32), ("source", C.c_int32), ("format", C.c_int32), ("filter", C.c_int32),
    ]


class GmsClearance(C.Structure):
    """gms_clearance: a rectangle of a map as squared distances to the nearest obstacle (gridmapslam.h "clearance fields")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("max_radius", C.c_int32), ("mode", C.c_int32), ("filter", C.c_int32),
    ]


class GmsSkeleton(C.Structure):
    """gms_skeleton: a rectangle of a map as nearest-obstacle sites and free-space skeleton (gridmapslam.h "sites and skeleton")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("max_radius", C.c_int32), ("mode", C.c_int32), ("min_clear", C.c_int32), ("min_gap", C.c_int32), ("filter", C.c_int32),
        ("pad", C.c_int32 * 3),
    ]


class GmsReach(C.Structure):
    """gms_reach: a rectangle of a map's cost-to-go field (gridmapslam.h "cost-to-go fields")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("max_cost", C.c_int32), ("inflate", C.c_int32), ("mode", C.c_int32), ("filter", C.c_int32),
    ]


class GmsFrontiers(C.Structure):
    """gms_frontiers: a request for a map's frontier regions (gridmapslam.h "frontier regions")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("min_size", C.c_int32), ("inflate", C.c_int32), ("filter", C.c_int32), ("pad", C.c_int32),
    ]


class GmsFrontier(C.Structure):
    """gms_frontier: one region's record, 56 bytes"""
    _fields_ = [
        ("anchor_x", C.c_int32), ("anchor_y", C.c_int32), ("count", C.c_int32), ("goal_cost", C.c_int32),
        ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32),
        ("goal_x", C.c_int32), ("goal_y", C.c_int32), ("sum_x", C.c_int64), ("sum_y", C.c_int64),
    ]


class GmsRooms(C.Structure):
    """gms_rooms: a request for a map's rooms and doors (gridmapslam.h "rooms and doors")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("core", C.c_int32), ("inflate", C.c_int32), ("mode", C.c_int32), ("min_core", C.c_int32), ("max_cost", C.c_int32),
        ("filter", C.c_int32), ("pad", C.c_int32 * 2),
    ]


class GmsRoom(C.Structure):
    """gms_room: one room's record, 56 bytes"""
    _fields_ = [
        ("anchor_x", C.c_int32), ("anchor_y", C.c_int32), ("core_count", C.c_int32), ("count", C.c_int32),
        ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32),
        ("max_depth", C.c_int32), ("doors", C.c_int32), ("sum_x", C.c_int64), ("sum_y", C.c_int64),
    ]


class GmsDoor(C.Structure):
    """gms_door: one pair of touching rooms, 48 bytes"""
    _fields_ = [
        ("a", C.c_uint32), ("b", C.c_uint32), ("count", C.c_int32),
        ("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32), ("pad", C.c_int32),
        ("sum_x2", C.c_int64), ("sum_y2", C.c_int64),
    ]


class GmsGain(C.Structure):
    """gms_gain: a view-gain request (gridmapslam.h "view gain")"""
    _fields_ = [("max_range", C.c_int32), ("filter", C.c_int32)]


class GmsGainRec(C.Structure):
    """gms_gain_rec: one candidate pose's record, 32 bytes"""
    _fields_ = [
        ("unknown", C.c_int32), ("free_cells", C.c_int32), ("occupied", C.c_int32), ("hits", C.c_int32),
        ("walked", C.c_int32), ("start_x", C.c_int32), ("start_y", C.c_int32), ("pad", C.c_int32),
    ]


class GmsScatter(C.Structure):
    """gms_scatter: a seeding request (gridmapslam.h "particle seeding")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("inflate", C.c_int32), ("mode", C.c_int32), ("first", C.c_int32), ("count", C.c_int32),
        ("jitter", C.c_int32), ("pad", C.c_int32),
    ]


class GmsLocate(C.Structure):
    """gms_locate: a global scan-matching request (gridmapslam.h "global scan matching")"""
    _fields_ = [
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
        ("n_theta", C.c_int32), ("tol", C.c_int32), ("mode", C.c_int32), ("min_score", C.c_int32),
        ("cap", C.c_int32), ("free_only", C.c_int32), ("filter", C.c_int32), ("pad", C.c_int32),
    ]


class GmsLocateRec(C.Structure):
    """gms_locate_rec: one pose's record, 16 bytes"""
    _fields_ = [("score", C.c_int32), ("k", C.c_int32), ("x", C.c_int32), ("y", C.c_int32)]


class GmsModes(C.Structure):
    """gms_modes: a pose-mode request (gridmapslam.h "pose modes")"""
    _fields_ = [("bin_cells", C.c_int32), ("n_theta", C.c_int32), ("min_count", C.c_int32), ("pad", C.c_int32)]


class GmsMode(C.Structure):
    """gms_mode: one mode's record, 112 bytes"""
    _fields_ = [
        ("anchor_bx", C.c_int32), ("anchor_by", C.c_int32), ("anchor_bt", C.c_int32), ("count", C.c_int32),
        ("bins", C.c_int32), ("strongest", C.c_int32), ("min_bx", C.c_int32), ("min_by", C.c_int32),
        ("max_bx", C.c_int32), ("max_by", C.c_int32), ("pad", C.c_int32 * 2),
        ("w", C.c_double), ("wx", C.c_double), ("wy", C.c_double), ("wc", C.c_double), ("ws", C.c_double),
        ("wxx", C.c_double), ("wxy", C.c_double), ("wyy", C.c_double),
    ]


class GmsAlignParams(C.Structure):
    """gms_align_params: the parameters of a scan alignment (gridmapslam.h "continuous scan alignment"), 64 bytes"""
    _fields_ = [
        ("iters", C.c_int32), ("pad", C.c_int32), ("damp_t", C.c_double), ("damp_r", C.c_double), ("max_t", C.c_double), ("max_r", C.c_double),
        ("eps_t", C.c_double), ("eps_r", C.c_double), ("det_min", C.c_double),
    ]


class GmsAlignRecord(C.Structure):
    """gms_align_record: one aligned pose's record, 80 bytes"""
    _fields_ = [
        ("status", C.c_int32), ("iters_done", C.c_int32), ("n_used", C.c_int32), ("n_used0", C.c_int32),
        ("score0", C.c_double), ("score", C.c_double), ("H", C.c_double * 6),
    ]


class GmsRollout(C.Structure):
    """gms_rollout: a trajectory-rollout request (gridmapslam.h "trajectory rollouts")"""
    _fields_ = [("max_range", C.c_int32), ("inflate", C.c_int32), ("mode", C.c_int32), ("filter", C.c_int32)]


class GmsRolloutRec(C.Structure):
    """gms_rollout_rec: one (start pose, candidate) record, 32 bytes"""
    _fields_ = [
        ("first_hit", C.c_uint16), ("hit_point", C.c_uint16), ("min_d2", C.c_uint16), ("best_step", C.c_uint16),
        ("best_cost", C.c_uint16), ("end_cost", C.c_uint16), ("flags", C.c_uint16), ("pad", C.c_uint16),
        ("last_x", C.c_int32), ("last_y", C.c_int32), ("start_x", C.c_int32), ("start_y", C.c_int32),
    ]


class GmsRolloutRisk(C.Structure):
    """gms_rollout_risk: one candidate over a filter's particles, 32 bytes"""
    _fields_ = [
        ("n_hit", C.c_uint32), ("n_start_blocked", C.c_uint32), ("min_first_hit", C.c_uint32), ("pad", C.c_uint32),
        ("sum_first_hit", C.c_uint64), ("pad2", C.c_uint64),
    ]


class GmsRoute(C.Structure):
    """gms_route: a route request (gridmapslam.h "routes"), 24 bytes"""
    _fields_ = [("max_cells", C.c_int32), ("max_waypoints", C.c_int32), ("look", C.c_int32), ("inflate", C.c_int32), ("mode", C.c_int32),
                ("filter", C.c_int32)]


class GmsRouteRec(C.Structure):
    """gms_route_rec: one start's record, 32 bytes"""
    _fields_ = [
        ("n_cells", C.c_uint32), ("n_waypoints", C.c_uint32), ("start_cost", C.c_uint16), ("end_cost", C.c_uint16), ("min_d2", C.c_uint16),
        ("flags", C.c_uint16), ("min_d2_at", C.c_uint32), ("end_x", C.c_int32), ("end_y", C.c_int32), ("pad", C.c_uint32),
    ]


class GmsWarp(C.Structure):
    """gms_warp: a map warp -- the pose of the source map's world frame in the destination's, the destination rectangle and the op
    (gridmapslam.h "map warps"), 64 bytes"""
    _fields_ = [
        ("tx", C.c_double), ("ty", C.c_double), ("c", C.c_double), ("s", C.c_double), ("clamp", C.c_double),
        ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("op", C.c_int32), ("pad", C.c_int32),
    ]


class GmsWarpStats(C.Structure):
    """gms_warp_stats: the class-pair counts of a warp, 80 bytes"""
    _fields_ = [("pair", (C.c_int64 * 3) * 3), ("n_outside", C.c_int64)]


class GmsCensus(C.Structure):
    """gms_census: a census of a gms_slam's particle maps (gridmapslam.h "census of the particles' maps"), 16 bytes"""
    _fields_ = [("min_known", C.c_int32), ("filter", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class GmsCensusTotals(C.Structure):
    """gms_census_totals: cells by consensus class, contested cells and the minority sum, 32 bytes"""
    _fields_ = [("cls", C.c_uint32 * 3), ("contested", C.c_uint32), ("minority", C.c_uint64), ("n", C.c_uint32), ("min_known", C.c_uint32)]


GAIN_DTYPE = np.dtype([(n, "<i4") for n, _ in GmsGainRec._fields_])     # gms_gain_rec
assert GAIN_DTYPE.itemsize == C.sizeof(GmsGainRec) == 32
ROLLOUT_STEP_DTYPE = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("c", "<f4"), ("s", "<f4")])     # gms_rollout_step
ROLLOUT_DTYPE = np.dtype([(n, "<u2" if t is C.c_uint16 else "<i4") for n, t in GmsRolloutRec._fields_])     # gms_rollout_rec
ROLLOUT_RISK_DTYPE = np.dtype([(n, "<u8" if t is C.c_uint64 else "<u4") for n, t in GmsRolloutRisk._fields_])     # gms_rollout_risk
assert ROLLOUT_DTYPE.itemsize == C.sizeof(GmsRolloutRec) == 32 and ROLLOUT_RISK_DTYPE.itemsize == C.sizeof(GmsRolloutRisk) == 32
assert ROLLOUT_STEP_DTYPE.itemsize == 16 and C.sizeof(GmsRollout) == 16
GMS_ROLLOUT_MAX_K, GMS_ROLLOUT_MAX_T, GMS_ROLLOUT_MAX_F = 4096, 256, 64
GMS_ROLLOUT_CANDIDATES = 16      # candidates a rollout workgroup takes (gms_rollout_candidates_per_workgroup() of the library as built)
GMS_ROLLOUT_HIT_OUTSIDE, GMS_ROLLOUT_HIT_RANGE, GMS_ROLLOUT_HIT_BLOCKED, GMS_ROLLOUT_START_BLOCKED = 1, 2, 4, 8      # gms_rollout_rec.flags
ROUTE_DTYPE = np.dtype([(n, {C.c_uint16: "<u2", C.c_uint32: "<u4", C.c_int32: "<i4"}[t]) for n, t in GmsRouteRec._fields_])     # gms_route_rec
assert ROUTE_DTYPE.itemsize == C.sizeof(GmsRouteRec) == 32 and C.sizeof(GmsRoute) == 24
GMS_ROUTE_MAX_P, GMS_ROUTE_MAX_CELLS, GMS_ROUTE_MAX_LOOK = 65536, 16384, 4096
GMS_ROUTE_NO_PATH, GMS_ROUTE_BROKEN, GMS_ROUTE_CELLS_CUT, GMS_ROUTE_WAYPOINTS_CUT, GMS_ROUTE_MISMATCH = 1, 2, 4, 8, 16      # gms_route_rec.flags
WARP_STATS_DTYPE = np.dtype([("pair", "<i8", (3, 3)), ("n_outside", "<i8")])     # gms_warp_stats
assert WARP_STATS_DTYPE.itemsize == C.sizeof(GmsWarpStats) == 80 and C.sizeof(GmsWarp) == 64
GMS_WARP_COMPARE, GMS_WARP_REPLACE, GMS_WARP_ADD, GMS_WARP_FILL = 0, 1, 2, 3                     # gms_warp.op
CENSUS_TOTALS_DTYPE = np.dtype([("cls", "<u4", (3,)), ("contested", "<u4"), ("minority", "<u8"), ("n", "<u4"), ("min_known", "<u4")])     # gms_census_totals
CENSUS_AGREE_DTYPE = np.dtype([("pair", "<u4", (3, 3)), ("zero", "<u4")])     # one particle's record of the agreement
assert CENSUS_TOTALS_DTYPE.itemsize == C.sizeof(GmsCensusTotals) == 32 and CENSUS_AGREE_DTYPE.itemsize == 40 and C.sizeof(GmsCensus) == 16
GMS_CENSUS_WRITE_MAP = 1                                                                         # gms_census.flags
# the cells a workgroup of the counting pass takes, the particles of its chunk, the cells a workgroup of the agreement pass takes
# (gms_census_geometry() of the library as built)
GMS_CENSUS_TILE, GMS_CENSUS_CHUNK, GMS_CENSUS_AGREE = 512, 32, 4096
LOCATE_DTYPE = np.dtype([(n, "<i4") for n, _ in GmsLocateRec._fields_])     # gms_locate_rec
assert LOCATE_DTYPE.itemsize == C.sizeof(GmsLocateRec) == 16 and C.sizeof(GmsLocate) == 48
GMS_LOCATE_SKIP = -32768
FRONTIER_DTYPE = np.dtype([(n, "<i8" if n.startswith("sum_") else "<i4") for n, _ in GmsFrontier._fields_])     # gms_frontier
assert FRONTIER_DTYPE.itemsize == C.sizeof(GmsFrontier) == 56
GMS_FRONTIER_NONE = 0xFFFFFFFF
ROOM_DTYPE = np.dtype([(n, "<i8" if n.startswith("sum_") else "<i4") for n, _ in GmsRoom._fields_])     # gms_room
DOOR_DTYPE = np.dtype([(n, "<i8" if n.startswith("sum_") else "<u4" if n in ("a", "b") else "<i4") for n, _ in GmsDoor._fields_])     # gms_door
assert ROOM_DTYPE.itemsize == C.sizeof(GmsRoom) == 56 and DOOR_DTYPE.itemsize == C.sizeof(GmsDoor) == 48 and C.sizeof(GmsRooms) == 48
GMS_ROOM_NONE, GMS_ROOMS_MAX, GMS_ROOMS_STAGES = 0xFFFFFFFF, 0xFFFF, 5
MODE_DTYPE = np.dtype([(n, "<f8" if t is C.c_double else ("<i4", (2,)) if n == "pad" else "<i4") for n, t in GmsMode._fields_])     # gms_mode
assert MODE_DTYPE.itemsize == C.sizeof(GmsMode) == 112
GMS_MODE_NONE = 0xFFFFFFFF
ALIGN_DTYPE = np.dtype([(n, ("<f8", (6,)) if n == "H" else "<f8" if t is C.c_double else "<i4") for n, t in GmsAlignRecord._fields_])     # gms_align_record
assert ALIGN_DTYPE.itemsize == C.sizeof(GmsAlignRecord) == 80 and C.sizeof(GmsAlignParams) == 64
GMS_ALIGN_ITERS, GMS_ALIGN_CONVERGED, GMS_ALIGN_NO_BEAM, GMS_ALIGN_SINGULAR = 0, 1, 2, 3      # gms_align_record.status
GMS_SLAM_ALIGN_PLANES, GMS_SLAM_ALIGN_MEMORY = 1, 2                                          # gms_slam_align_form
GMS_SLAM_BEAMS_MULTIPLY, GMS_SLAM_BEAMS_REPLACE = 0, 1                                       # gms_slam_set_beam_model's combine
GMS_MAX_PARTICLES = 1 << 20
CLEARANCE = GmsClearance
GMS_REACH_AXIS, GMS_REACH_DIAG, GMS_REACH_FAR, GMS_REACH_MAX_SEEDS = 5, 7, 0xFFFF, 4096
GMS_CLEAR_OCCUPIED, GMS_CLEAR_NOT_FREE = 0, 1
GMS_CLEAR_FAR, GMS_CLEAR_OUTSIDE = 0xFFFF, 0xFFFE
GMS_SITE_NONE, GMS_SITE_OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE
SKELETON_TOTALS_DTYPE = np.dtype([("sited", "<i8"), ("skeleton", "<i8"), ("min_d2", "<i4"), ("max_d2", "<i4"), ("pad", "<i4", (2,))])     # gms_skeleton_totals
NEAREST_DTYPE = np.dtype([("site", "<u4"), ("d2", "<u4")])                                   # gms_nearest
assert C.sizeof(GmsSkeleton) == 48 and SKELETON_TOTALS_DTYPE.itemsize == 32 and NEAREST_DTYPE.itemsize == 8
GMS_VIEW_GREY8, GMS_VIEW_PACKED32 = 0, 1
GMS_VIEW_LOG, GMS_VIEW_LIKELIHOOD = 0, 1
GMS_VIEW_STRONGEST = -1
GMS_CAST_ALL = -2


class GmsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libgridmapslam error {code}: {msg}")
        self.code = code


_lib = None


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (different SONAME from /opt/rocm's
    libamdhip64.so.7).  Two HIP runtimes in one process cannot share streams, and whichever initialises
    second may not see the GPU.  Promote torch's copy to the global symbol scope BEFORE our library is
    loaded, so that its hip* symbols bind to the runtime torch uses: one runtime, torch streams usable
    through gms_map_set_stream, RCCL ordering intact.  Without torch the system runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load() -> C.CDLL:
    """Load the in-tree HIP library; raise if it is missing (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m gridmap_slam_robot_amd.build` "
            "(hipcc, --offload-arch=gfx950). gridmap_slam_robot_amd has no CPU fallback."
        )
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    pp = C.POINTER(GmsParams)
    sp = C.POINTER(GmsPfStats)

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("gms_version", C.c_int)
    sig("gms_build_info", C.c_char_p)
    sig("gms_last_error", C.c_char_p)
    sig("gms_device_count", C.c_int)
    sig("gms_params_default", C.c_int, pp, f32, f32, f32, f32, f32)
    sig("gms_grid_size", C.c_int, pp, vp, vp)
    sig("gms_generate_gaussian_kernel", C.c_int, f64, i32, vp)
    sig("gms_log_odds", f64, f64)
    sig("gms_inv_log_odds", f64, f64)
    sig("gms_map_create", C.c_int, pp, C.POINTER(vp))
    sig("gms_map_destroy", C.c_int, vp)
    sig("gms_map_get_size", C.c_int, vp, vp, vp, vp)
    sig("gms_map_set_stream", C.c_int, vp, vp)
    sig("gms_map_synchronize", C.c_int, vp)
    sig("gms_map_reset", C.c_int, vp)
    sig("gms_map_upload_log", C.c_int, vp, vp)
    sig("gms_map_download_log", C.c_int, vp, vp)
    sig("gms_map_upload_likelihood", C.c_int, vp, vp)
    sig("gms_map_download_likelihood", C.c_int, vp, vp)
    sig("gms_map_copy", C.c_int, vp, vp)
    sig("gms_map_get_raw_at", C.c_int, vp, i32, i32, i32, vp, vp)
    sig("gms_map_get_at_point", C.c_int, vp, i32, C.c_float, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_double))
    sig("gms_map_combine", C.c_int, vp, vp)
    sig("gms_map_deskew", C.c_int, vp, vp, vp, vp, i32, f64, f64, vp, vp)
    sig("gms_map_integrate", C.c_int, vp, vp, i32, vp)
    sig("gms_map_integrate_at", C.c_int, vp, vp, i32, vp, i32)
    sig("gms_map_apply_ray", C.c_int, vp, f32, f32, f32, f32, f32, i32)
    sig("gms_map_trace_ray", C.c_int, vp, f32, f32, f32, f32, i32, vp, i32, vp)
    sig("gms_map_trace_scan", C.c_int, vp, vp, i32, vp, vp, vp, i32, vp)
    sig("gms_map_build_likelihood", C.c_int, vp)
    sig("gms_map_update", C.c_int, vp, vp, i32, vp)
    sig("gms_map_update_at", C.c_int, vp, vp, i32, vp, i32)
    sig("gms_map_integrate_dev", C.c_int, vp, vp, i32, vp)
    sig("gms_map_integrate_at_dev", C.c_int, vp, vp, i32, vp, i32)
    sig("gms_map_update_dev", C.c_int, vp, vp, i32, vp)
    sig("gms_map_update_at_dev", C.c_int, vp, vp, i32, vp, i32)
    sig("gms_pf_set_poses_dev", C.c_int, vp, vp)
    sig("gms_pf_score_dev", C.c_int, vp, vp, i32)
    sig("gms_slam_update_dev", C.c_int, vp, vp, vp, i32, vp, f64, i32)
    sig("gms_slam_update_u_dev", C.c_int, vp, f64, f64, C.c_uint64, C.c_uint64, vp, i32, vp, f64, i32)
    sig("gms_slam_frame", C.c_int, vp, vp, vp, vp, i32, f64, f64, C.c_uint64, C.c_uint64, vp, f64, i32)
    sig("gms_slam_update", C.c_int, vp, vp, vp, i32, vp, f64, i32, sp)
    sig("gms_pf_create", C.c_int, vp, i32, C.POINTER(vp))
    sig("gms_pf_destroy", C.c_int, vp)
    sig("gms_pf_set_shard", C.c_int, vp, i64, i64)
    sig("gms_pf_set_poses", C.c_int, vp, vp)
    sig("gms_pf_get_poses", C.c_int, vp, vp)
    sig("gms_pf_set_weights", C.c_int, vp, vp)
    sig("gms_pf_get_weights", C.c_int, vp, vp)
    sig("gms_pf_get_log_weights", C.c_int, vp, vp)
    sig("gms_pf_score", C.c_int, vp, vp, i32)
    sig("gms_pf_normalize", C.c_int, vp, sp)
    sig("gms_pf_get_stats", C.c_int, vp, sp)
    sig("gms_pf_weighted_pose", C.c_int, vp, vp)
    sig("gms_pf_resample", C.c_int, vp, vp, vp, vp)
    sig("gms_pf_resample_if", C.c_int, vp, vp, f64)
    sig("gms_pf_last_resample_indices", C.c_int, vp, vp)
    sig("gms_pf_count", C.c_int, vp, vp, vp, vp)
    sig("gms_pf_did_resample", C.c_int, vp, vp)
    sig("gms_pf_refine_poses", C.c_int, vp, vp, i32)
    sig("gms_pf_last_step", C.c_int, vp, vp, vp, vp, vp)
    sig("gms_pf_segment_order_launches", C.c_int, vp, C.POINTER(C.c_int64))
    sig("gms_pf_set_refine", C.c_int, vp, i32)
    sig("gms_pf_sample_motion", C.c_int, vp, f64, f64, C.c_uint64, C.c_uint64)
    sig("gms_pf_partials_len", C.c_int, vp, vp)
    sig("gms_pf_local_partials", C.c_int, vp, vp)
    sig("gms_pf_apply_partials", C.c_int, vp, vp, vp)
    sig("gms_pf_pack", C.c_int, vp, vp)
    sig("gms_pf_stats_from_partials", C.c_int, vp, vp)
    sig("gms_pf_import_global", C.c_int, vp, vp)
    sig("gms_comm_load", C.c_int, C.c_char_p)
    sig("gms_comm_unique_id", C.c_int, vp)
    sig("gms_comm_create", C.c_int, C.POINTER(vp), vp, i32, i32, i32)
    sig("gms_comm_destroy", C.c_int, vp)
    sig("gms_comm_rank", C.c_int, vp, C.POINTER(i32), C.POINTER(i32))
    sig("gms_pf_normalize_sharded_begin", C.c_int, vp, vp)
    sig("gms_pf_normalize_sharded_end", C.c_int, vp, vp)
    sig("gms_slam_update_sharded_dev", C.c_int, vp, vp, vp, vp, i32, vp, f64, i32)
    sig("gms_slam_update_sharded", C.c_int, vp, vp, vp, vp, i32, vp, f64, i32, sp)
    sig("gms_slam_update_sharded_begin_dev", C.c_int, vp, vp, vp, i32)
    sig("gms_pf_gather_buffers", C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(vp), C.POINTER(C.c_int64))
    sig("gms_slam_update_sharded_end_dev", C.c_int, vp, vp, i32, vp, f64, i32)
    sig("gms_profile_enable", C.c_int, vp, i32)
    sig("gms_profile_reset", C.c_int, vp)
    sig("gms_profile_get", C.c_int, vp, i32, vp, vp)
    sig("gms_profile_sample", C.c_int, vp, i32)
    sig("gms_profile_calibrate", C.c_int, vp, i32, C.POINTER(C.c_double))
    sig("gms_profile_calibrate2", C.c_int, vp, i32, vp, vp)
    sig("gms_map_tile_stats", C.c_int, vp, i32, vp)
    sig("gms_pf_set_log_normalize", C.c_int, vp, i32)
    sig("gms_pf_set_reference_order", C.c_int, vp, i32)
    sig("gms_debug_f32", C.c_int, vp, i32, vp, vp, i64)
    sig("gms_slam_create", C.c_int, pp, i32, C.POINTER(vp))
    sig("gms_slam_destroy", C.c_int, vp)
    sig("gms_slam_reset", C.c_int, vp)
    sig("gms_slam_count", C.c_int, vp, vp, vp, vp)
    sig("gms_slam_handles", C.c_int, vp, C.POINTER(vp), C.POINTER(vp))
    sig("gms_slam_set_refine", C.c_int, vp, i32)
    sig("gms_slam_update_per_particle", C.c_int, vp, vp, i32, i32, f64, f64, C.c_uint64, C.c_uint64, sp)
    sig("gms_slam_update_per_particle_dev", C.c_int, vp, vp, i32, i32, f64, f64, C.c_uint64, C.c_uint64, sp)
    sig("gms_slam_resample_maps", C.c_int, vp, f64, vp, vp)
    sig("gms_slam_resample_maps_if", C.c_int, vp, f64, f64)
    sig("gms_slam_update_batch", C.c_int, vp, vp, i32, vp, vp, vp, vp, C.c_uint64, sp)
    sig("gms_slam_update_batch_dev", C.c_int, vp, vp, i32, vp, vp, vp, vp, C.c_uint64, sp)
    sig("gms_slam_resample_maps_batch", C.c_int, vp, vp, vp, vp)
    sig("gms_slam_resample_maps_if_batch", C.c_int, vp, vp, f64)
    sig("gms_slam_frame_per_particle", C.c_int, vp, vp, vp, vp, i32, f64, f64, C.c_uint64, C.c_uint64, f64, f64, sp)
    sig("gms_slam_frame_batch", C.c_int, vp, vp, vp, vp, i32, vp, vp, vp, C.c_uint64, vp, f64, sp)
    sig("gms_slam_download_map", C.c_int, vp, i32, vp, vp)
    sig("gms_slam_upload_map", C.c_int, vp, i32, vp, vp)
    sig("gms_slam_download_maps", C.c_int, vp, vp, vp)
    sig("gms_slam_combined", C.c_int, vp)
    sig("gms_slam_copies", C.c_int, vp, C.POINTER(C.c_int64))
    sig("gms_slam_trace_scan", C.c_int, vp, i32, vp, i32, vp, vp, i32, vp)
    sig("gms_slam_last_beams", C.c_int, vp, i32, vp, i32, C.POINTER(C.c_int32))
    sig("gms_slam_create_shard", C.c_int, pp, i32, C.c_int64, C.c_int64, C.POINTER(vp))
    sig("gms_slam_update_local", C.c_int, vp, vp, i32, i32, f64, f64, C.c_uint64, C.c_uint64)
    sig("gms_slam_update_local_dev", C.c_int, vp, vp, i32, i32, f64, f64, C.c_uint64, C.c_uint64)
    sig("gms_slam_shard_draw", C.c_int, vp, f64, f64, C.POINTER(C.c_int32), vp)
    sig("gms_slam_record_doubles", C.c_int, vp, C.POINTER(C.c_int64))
    sig("gms_slam_shard_export", C.c_int, vp, vp, i32, vp)
    sig("gms_slam_shard_gather", C.c_int, vp, vp, vp, vp)
    sig("gms_slam_update_sharded_maps", C.c_int, vp, vp, vp, i32, i32, f64, f64, C.c_uint64, C.c_uint64, sp)
    sig("gms_slam_resample_sharded_maps", C.c_int, vp, vp, f64, f64, C.POINTER(C.c_int32))
    sig("gms_slam_plan_exchange", C.c_int, vp, i32, i32, i32, vp, vp, vp, vp, vp)
    sig("gms_debug_set_stamps", C.c_int, vp, vp)
    vw = C.POINTER(GmsView)
    sig("gms_view_size", C.c_int, vw, vp, vp, vp)
    sig("gms_map_view", C.c_int, vp, i32, vw, vp)
    sig("gms_map_view_dev", C.c_int, vp, i32, vw, vp)
    sig("gms_slam_view", C.c_int, vp, i32, vw, vp, vp)
    sig("gms_slam_view_dev", C.c_int, vp, i32, vw, vp, vp)
    sig("gms_slam_history_bytes", C.c_int, i32, i32, C.POINTER(C.c_int64))
    sig("gms_slam_set_history", C.c_int, vp, i32)
    sig("gms_slam_history_len", C.c_int, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32))
    sig("gms_slam_trajectory", C.c_int, vp, i32, i32, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    sig("gms_slam_trajectory_dev", C.c_int, vp, i32, i32, vp, i32, vp)
    sig("gms_slam_trajectories", C.c_int, vp, i32, vp, vp, i32, C.POINTER(C.c_int32))
    sig("gms_slam_history_walk_rows", C.c_int, vp, C.POINTER(C.c_int32))
    sig("gms_map_cast", C.c_int, vp, i32, vp, i32, vp, i32, vp)
    sig("gms_map_cast_dev", C.c_int, vp, i32, vp, i32, vp, i32, vp)
    sig("gms_map_cast_at", C.c_int, vp, vp, i32, vp, i32, vp)
    sig("gms_map_cast_at_dev", C.c_int, vp, vp, i32, vp, i32, vp)
    sig("gms_slam_cast", C.c_int, vp, i32, i32, vp, i32, vp, vp)
    sig("gms_slam_cast_dev", C.c_int, vp, i32, i32, vp, i32, vp, vp)
    sig("gms_map_cast_plane_builds", C.c_int, vp, C.POINTER(C.c_int64))
    cl = C.POINTER(GmsClearance)
    sig("gms_clearance_size", C.c_int, cl, vp, vp, vp)
    sig("gms_map_clearance", C.c_int, vp, i32, cl, vp)
    sig("gms_map_clearance_dev", C.c_int, vp, i32, cl, vp)
    sig("gms_map_clearance_poses", C.c_int, vp, i32, vp, i32, i32, i32, vp)
    sig("gms_map_clearance_poses_dev", C.c_int, vp, i32, vp, i32, i32, i32, vp)
    sig("gms_slam_clearance", C.c_int, vp, i32, cl, vp, vp)
    sig("gms_slam_clearance_dev", C.c_int, vp, i32, cl, vp, vp)
    sk = C.POINTER(GmsSkeleton)
    sig("gms_skeleton_size", C.c_int, sk, vp, vp, vp, vp)
    sig("gms_map_skeleton", C.c_int, vp, i32, sk, vp, vp, vp)
    sig("gms_map_skeleton_dev", C.c_int, vp, i32, sk, vp, vp, vp)
    sig("gms_map_nearest_poses", C.c_int, vp, i32, vp, i32, i32, i32, vp)
    sig("gms_map_nearest_poses_dev", C.c_int, vp, i32, vp, i32, i32, i32, vp)
    sig("gms_slam_skeleton", C.c_int, vp, i32, sk, vp, vp, vp, vp)
    sig("gms_slam_skeleton_dev", C.c_int, vp, i32, sk, vp, vp, vp, vp)
    rp = C.POINTER(GmsReach)
    sig("gms_reach_size", C.c_int, rp, vp, vp, vp)
    sig("gms_map_reach", C.c_int, vp, i32, rp, vp, i32, vp)
    sig("gms_map_reach_dev", C.c_int, vp, i32, rp, vp, i32, vp)
    sig("gms_slam_reach", C.c_int, vp, i32, rp, vp, i32, vp, vp)
    sig("gms_slam_reach_dev", C.c_int, vp, i32, rp, vp, i32, vp, vp)
    sig("gms_map_reach_stats", C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64))
    gp = C.POINTER(GmsGain)
    sig("gms_map_gain", C.c_int, vp, i32, gp, vp, i32, vp, i32, vp)
    sig("gms_map_gain_dev", C.c_int, vp, i32, gp, vp, i32, vp, i32, vp)
    sig("gms_slam_gain", C.c_int, vp, i32, gp, vp, i32, vp, i32, vp, vp)
    sig("gms_slam_gain_dev", C.c_int, vp, i32, gp, vp, i32, vp, i32, vp, vp)
    scp = C.POINTER(GmsScatter)
    sig("gms_scatter_check", C.c_int, scp)
    sig("gms_pf_scatter", C.c_int, vp, scp, C.c_uint64, C.c_uint64, vp)
    sig("gms_map_scatter_table_builds", C.c_int, vp, C.POINTER(C.c_int64))
    lp = C.POINTER(GmsLocate)
    sig("gms_locate_check", C.c_int, lp)
    sig("gms_locate_offsets", C.c_int, vp, i32, C.c_double, C.c_double, i32, C.c_double, vp)
    sig("gms_map_locate", C.c_int, vp, i32, lp, vp, i32, vp, vp)
    sig("gms_map_locate_dev", C.c_int, vp, i32, lp, vp, i32, vp, vp)
    sig("gms_slam_locate", C.c_int, vp, i32, lp, vp, i32, vp, vp, vp)
    sig("gms_slam_locate_dev", C.c_int, vp, i32, lp, vp, i32, vp, vp, vp)
    sig("gms_map_locate_stats", C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64))
    mp = C.POINTER(GmsModes)
    sig("gms_modes_check", C.c_int, mp)
    sig("gms_pf_modes", C.c_int, vp, i32, mp, vp, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    sig("gms_pf_modes_dev", C.c_int, vp, i32, mp, vp, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
    sig("gms_beam_model_check", C.c_int, i32, i32, vp)
    sig("gms_pf_score_beams", C.c_int, vp, vp, i32, i32, i32, vp, vp)
    sig("gms_pf_score_beams_dev", C.c_int, vp, vp, i32, i32, i32, vp, vp)
    ap = C.POINTER(GmsAlignParams)
    sig("gms_align_params_default", C.c_int, ap)
    sig("gms_align_check", C.c_int, ap)
    sig("gms_map_align", C.c_int, vp, i32, vp, i32, vp, i32, ap, vp, vp)
    sig("gms_map_align_dev", C.c_int, vp, i32, vp, i32, vp, i32, ap, vp, vp)
    sig("gms_pf_align", C.c_int, vp, vp, i32, ap, vp)
    sig("gms_pf_align_dev", C.c_int, vp, vp, i32, ap, vp)
    sig("gms_slam_align", C.c_int, vp, vp, i32, ap, vp)
    sig("gms_slam_align_dev", C.c_int, vp, vp, i32, ap, vp)
    sig("gms_slam_set_align", C.c_int, vp, ap)
    sig("gms_slam_score_beams", C.c_int, vp, vp, i32, i32, i32, vp, vp)
    sig("gms_slam_score_beams_dev", C.c_int, vp, vp, i32, i32, i32, vp, vp)
    sig("gms_slam_set_beam_model", C.c_int, vp, i32, i32, vp, i32)
    sig("gms_slam_last_align", C.c_int, vp, vp)
    sig("gms_slam_align_form", C.c_int, vp, C.POINTER(C.c_int32))
    rop = C.POINTER(GmsRollout)
    sig("gms_rollout_check", C.c_int, rop, i32, i32, i32)
    sig("gms_rollout_arcs", C.c_int, vp, vp, i32, f64, i32, vp)
    sig("gms_rollout_candidates_per_workgroup", C.c_int)
    sig("gms_map_rollout", C.c_int, vp, i32, rop, vp, i32, vp, i32, i32, vp, i32, vp, vp, vp)
    sig("gms_map_rollout_dev", C.c_int, vp, i32, rop, vp, i32, vp, i32, i32, vp, i32, vp, vp, vp)
    sig("gms_slam_rollout", C.c_int, vp, i32, rop, vp, i32, vp, i32, i32, vp, i32, vp, vp, vp, vp)
    sig("gms_slam_rollout_dev", C.c_int, vp, i32, rop, vp, i32, vp, i32, i32, vp, i32, vp, vp, vp, vp)
    sig("gms_pf_rollout", C.c_int, vp, rop, vp, i32, i32, vp, i32, vp)
    sig("gms_pf_rollout_dev", C.c_int, vp, rop, vp, i32, i32, vp, i32, vp)
    rtp = C.POINTER(GmsRoute)
    sig("gms_route_check", C.c_int, rtp)
    sig("gms_map_route", C.c_int, vp, i32, rtp, vp, i32, vp, vp, vp, vp, vp)
    sig("gms_map_route_dev", C.c_int, vp, i32, rtp, vp, i32, vp, vp, vp, vp, vp)
    sig("gms_slam_route", C.c_int, vp, i32, rtp, vp, i32, vp, vp, vp, vp, vp, vp)
    sig("gms_slam_route_dev", C.c_int, vp, i32, rtp, vp, i32, vp, vp, vp, vp, vp, vp)
    wp = C.POINTER(GmsWarp)
    sig("gms_warp_pose", C.c_int, wp, f64, f64, f64)
    sig("gms_warp_check", C.c_int, wp)
    sig("gms_map_warp", C.c_int, vp, i32, vp, i32, wp, vp)
    sig("gms_map_warp_dev", C.c_int, vp, i32, vp, i32, wp, vp)
    sig("gms_slam_warp", C.c_int, vp, i32, i32, vp, i32, wp, vp, vp)
    sig("gms_slam_warp_dev", C.c_int, vp, i32, i32, vp, i32, wp, vp, vp)
    cp = C.POINTER(GmsCensus)
    sig("gms_census_check", C.c_int, cp, i32, i32)
    sig("gms_census_geometry", C.c_int, vp, vp, vp)
    sig("gms_slam_census", C.c_int, vp, cp, vp, vp, vp, vp)
    sig("gms_slam_census_dev", C.c_int, vp, cp, vp, vp, vp, vp)
    fp = C.POINTER(GmsFrontiers)
    sig("gms_frontiers_size", C.c_int, fp, vp, vp, vp)
    sig("gms_map_frontiers", C.c_int, vp, i32, fp, vp, vp, vp, i32, C.POINTER(C.c_int32))
    sig("gms_map_frontiers_dev", C.c_int, vp, i32, fp, vp, vp, vp, i32, C.POINTER(C.c_int32))
    sig("gms_slam_frontiers", C.c_int, vp, i32, fp, vp, vp, vp, i32, C.POINTER(C.c_int32), vp)
    sig("gms_slam_frontiers_dev", C.c_int, vp, i32, fp, vp, vp, vp, i32, C.POINTER(C.c_int32), vp)
    rp, ip = C.POINTER(GmsRooms), C.POINTER(C.c_int32)
    sig("gms_rooms_check", C.c_int, rp)
    sig("gms_rooms_size", C.c_int, rp, vp, vp, vp, vp)
    sig("gms_map_rooms", C.c_int, vp, i32, rp, vp, vp, vp, i32, ip, vp, i32, ip)
    sig("gms_map_rooms_dev", C.c_int, vp, i32, rp, vp, vp, vp, i32, ip, vp, i32, ip)
    sig("gms_slam_rooms", C.c_int, vp, i32, rp, vp, vp, vp, i32, ip, vp, i32, ip, vp)
    sig("gms_slam_rooms_dev", C.c_int, vp, i32, rp, vp, vp, vp, i32, ip, vp, i32, ip, vp)
    sig("gms_map_rooms_stats", C.c_int, vp, ip, C.POINTER(C.c_int64), ip)
    sig("gms_map_rooms_stage_us", C.c_int, vp, C.POINTER(C.c_double))
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != GMS_OK:
        raise GmsError(rc, load().gms_last_error().decode("utf-8", "replace"))


def ptr(a: np.ndarray) -> int:
    return a.ctypes.data
