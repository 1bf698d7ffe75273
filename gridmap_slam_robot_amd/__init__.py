"""gridmap_slam_robot_amd -- MI355X-native occupancy-grid SLAM core.

One hot path of antbern/gridmap-slam-robot (log-odds ray-cast map update, likelihood field,
particle scan matcher) as hand-written HIP kernels for gfx950 behind the C-ABI of
include/gridmapslam.h.  This package is the thin host side: a ctypes binding (_lib), the mirror of
the reference's GridMap / ParticleFilter / SLAM class surface (gridmap), particle sharding over
torch.distributed (distributed) and the synthetic trace generator used by tests and bench (synth).
"""
from .gridmap import AlignParams, GridMap, Observation, ParticleFilter, Pose, SLAM, SLAMParticleMaps, SLAMParticleMapsBatch, align_covariance, beam_model_factors, cells_of_poses, census_entropy, census_outliers, clearance_metres, descend, door_points, footprint_box, frontier_centroids, locate_offsets, locate_peaks, locate_poses, map_as_scan, mode_estimate, probe_fan, reach_metres, rollout_arcs, rollout_pick, room_centroids, room_graph, rooms_of_cells, route_points, scan_residual, scatter_slots, site_cells, site_vectors, skeleton_cells, strongest_mode, warp_agreement  # noqa: F401
from ._lib import ALIGN_DTYPE, BEAM_DTYPE, CENSUS_AGREE_DTYPE, CENSUS_TOTALS_DTYPE, GAIN_DTYPE, DOOR_DTYPE, LOCATE_DTYPE, ROLLOUT_DTYPE, ROLLOUT_RISK_DTYPE, ROLLOUT_STEP_DTYPE, ROOM_DTYPE, ROUTE_DTYPE, WARP_STATS_DTYPE, GmsError, load  # noqa: F401

__version__ = "0.1.0"
