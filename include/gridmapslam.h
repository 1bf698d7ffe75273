/*
 * gridmapslam.h -- C-ABI of the MI355X-native occupancy-grid SLAM core (libgridmapslam.so).
 *
 * Drop-in boundary for ONE hot path of antbern/gridmap-slam-robot's GridMapGL app: the log-odds
 * ray-cast map update, the likelihood-field build and the particle scan matcher (score,
 * normalise / Neff, weighted pose, systematic resample).  The reference has no FFI of its own; each
 * entry point below replaces one public Java method and cites it.  J/ =
 * java/GridMapGL/src/main/java/com/fmsz/gridmapgl/ in the reference tree.  The JNI / cgo-style
 * binding a maintainer would add is shown in INTEGRATION.md; a C++ mirror of the Java classes is in
 * include/gridmapslam.hpp.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, opaque handles, int status (GMS_OK = 0, negative =
 *    error; text via gms_last_error()).  No exception crosses the boundary.
 *  - The caller owns every host buffer; the library owns every device buffer.
 *  - One host thread per handle at a time (the reference calls this path from one thread only:
 *    J/app/DataEventHandler.java:24-26).
 *  - All work runs on the handle's HIP stream (gms_map_set_stream).  Entry points that only take
 *    inputs enqueue and return; entry points that fill a host buffer synchronise that stream
 *    before returning.
 *  - Grids are row-major `x + y*W` doubles exactly like GridMapData.logData / likelihoodData
 *    (J/slam/GridMap.java:72-74,135), so a JNI shim can Get/SetDoubleArrayRegion them as they are.
 *  - A handle with n_maps > 1 is a batch of independent maps (and particle sets): every per-map
 *    argument then carries a leading [n_maps] dimension.
 *  - There is no CPU fallback: without a HIP device gms_map_create fails with GMS_ERR_NO_DEVICE.
 */
#ifndef GRIDMAPSLAM_H
#define GRIDMAPSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define GMS_VERSION_MAJOR 0
#define GMS_VERSION_MINOR 1

#define GMS_MAX_TAPS 129        /* size of gms_params.kernel; gms_map_create refuses a kernel whose halo does not fit the likelihood
                                   pass's LDS tile (MI355X: up to 65 taps) */
#define GMS_BLOCK 256           /* particles per reduction block; shard offsets are multiples of it */
#define GMS_MAX_BEAMS 4096      /* beams per scan (per map): gms_params.max_beams may not exceed it */
#define GMS_MAX_PARTICLES (1 << 20)   /* particles per map of a filter, and the global population of a sharded one: the resampling
                                         kernels keep two levels of the cumulative-weight scan in LDS (133 KiB at this size) */

enum {
    GMS_OK = 0,
    GMS_ERR_INVALID = -1,       /* bad argument */
    GMS_ERR_NO_DEVICE = -2,     /* no usable HIP device (there is no CPU path) */
    GMS_ERR_HIP = -3,           /* a HIP runtime call failed */
    GMS_ERR_NOMEM = -4,
    GMS_ERR_STATE = -5,         /* call order violated (e.g. resample before normalise) */
    GMS_ERR_INTERNAL = -6       /* a bound the library proves for itself was exceeded (gms_map_reach's rounds): a bug, reported instead of looping */
};

/* One LIDAR beam = the fields of Observation.Measurement the path reads
 * (J/slam/Observation.java:37-41).  32 bytes. */
typedef struct gms_beam {
    double local_x;             /* Measurement.localX  (robot frame, metres) */
    double local_y;             /* Measurement.localY */
    double distance;            /* Measurement.distance (metres; SENSOR_MAX_RANGE on a miss) */
    uint8_t hit;                /* Measurement.wasHit */
    uint8_t pad_[7];
} gms_beam;

/* Everything the GridMap constructor and the constants it closes over decide
 * (J/slam/GridMap.java:80-100,210,223,259; J/slam/SensorModel.java:20-25).
 * Fill with gms_params_default() and override fields as needed. */
typedef struct gms_params {
    float width_m, height_m;    /* GridMap(width, height, ...) */
    float resolution;           /* metres per cell */
    float pos_x, pos_y;         /* lower-left corner in the world */
    int32_t n_maps;             /* batch of independent maps (1 = the reference's single map) */
    int32_t device;             /* HIP device ordinal */
    double l_free, l_occ;       /* Util.logOdds(P_FREE), Util.logOdds(P_OCCUPPIED); host-supplied so
                                   that the JVM's Math.log decides them */
    int32_t ktaps;              /* likelihood kernel (Util.generateGaussianKernel); host-supplied so */
    double kernel[GMS_MAX_TAPS];/* that the JVM's Math.exp decides the taps */
    int32_t extra_steps;        /* RayIterator additionalSteps, 2 */
    float hit_tolerance;        /* inverseSensorModel hitTolerance, 2 */
    double z_hit, z_random;     /* 0.9, 1 - 0.9 */
    float max_range;            /* SensorModel.SENSOR_MAX_RANGE, 10 */
    int32_t max_beams;          /* capacity per scan (per map); 0 = 2048; at most GMS_MAX_BEAMS */
} gms_params;

typedef struct gms_map gms_map;      /* GridMap + GridMapData (n_maps of them) */
typedef struct gms_pf gms_pf;        /* ParticleFilter / SLAM particle set bound to a gms_map */
typedef struct gms_comm gms_comm;    /* one rank's RCCL communicator (multi-GPU filters) */

/* Results of gms_pf_normalize, per map (SLAM.update's bookkeeping, J/slam/SLAM.java:87-129). */
typedef struct gms_pf_stats {
    double weight_sum;          /* sum of raw weights (SLAM.java:100) */
    double neff;                /* calculateNeff() (SLAM.java:180-190) */
    int32_t strongest;          /* global index of the first maximum raw weight (SLAM.java:110-115) */
    int32_t n_zero;             /* raw weights that were exactly 0 (underflow census; not in the reference) */
    double max_log_weight;      /* max over particles of sum(log factor); see gms_pf_score */
} gms_pf_stats;

/* ---- library ---------------------------------------------------------------------------------- */
int gms_version(void);                         /* major*1000 + minor */
/* 16 hex digits: sha256 prefix of the sources (the csrc directory, this header) the loaded binary was built from; build() prints the
 * same string ("built <hash>" / "reused <hash>"), so a log shows which binary ran. */
const char *gms_build_info(void);
const char *gms_last_error(void);              /* thread-local message of the last failing call */
int gms_device_count(void);                    /* HIP devices visible; 0 when none (never throws) */

/* ---- host-side helpers (pure; usable without a device) ----------------------------------------- */
/* GridMap ctor arithmetic: fills every field with the reference's values, computing l_free/l_occ
 * with libm log and the kernel with libm exp (J/slam/GridMap.java:80-100). */
int gms_params_default(gms_params *p, float width_m, float height_m, float resolution, float pos_x, float pos_y);
/* gridSize = ceil(width / resolution) in float (J/slam/GridMap.java:85). */
int gms_grid_size(const gms_params *p, int32_t *W, int32_t *H);
/* Util.generateGaussianKernel(sigma, size): out has 2*size+1 taps (J/app/Util.java:428-455). */
int gms_generate_gaussian_kernel(double sigma, int32_t size, double *out);
/* Util.logOdds / Util.invLogOdds (J/app/Util.java:35-37,46-48). */
double gms_log_odds(double p);
double gms_inv_log_odds(double l);

/* ---- GridMap / GridMapData --------------------------------------------------------------------- */
/* new GridMap(width,height,resolution,position) + createMapData(null)  (GridMap.java:80,106). */
int gms_map_create(const gms_params *p, gms_map **out);
/* GMS_ERR_STATE while particle filters created on this map are alive: destroy those first. */
int gms_map_destroy(gms_map *m);
int gms_map_get_size(const gms_map *m, int32_t *W, int32_t *H, int32_t *n_maps);
/* Run this handle's work on an existing hipStream_t (e.g. a torch stream); NULL restores the handle's own stream.
 * NB the legacy default stream's handle IS NULL: a host whose other work runs on the default stream gets the handle's
 * own stream here, unrelated to it -- give both sides one real stream when they exchange device buffers. */
int gms_map_set_stream(gms_map *m, void *hip_stream);
int gms_map_synchronize(gms_map *m);
/* GridMap.reset (GridMap.java:129-132): logData := logOdds(0.5) = 0 (likelihoodData is left alone,
 * as in the reference, until the next gms_map_build_likelihood). */
int gms_map_reset(gms_map *m);
/* GridMapData array access (GridMap.java:72-74; read by the renderer :371-388 and serialiser).
 * n_maps*W*H doubles. */
int gms_map_upload_log(gms_map *m, const double *log_data);
int gms_map_download_log(gms_map *m, double *log_data);
int gms_map_upload_likelihood(gms_map *m, const double *lik);
int gms_map_download_likelihood(gms_map *m, double *lik);
/* createMapData(other): device-to-device copy of both arrays (GridMap.java:106-124). */
int gms_map_copy(gms_map *dst, const gms_map *src);
/* GridMapApp.calculateCombined (J/app/GridMapApp.java:439-458): dst (one map) := logOdds(1 - prod_m (1 - prob_m)) over
 * the n_maps of src, maps in index order; rebuild dst's likelihood field afterwards as the reference does (:457). */
int gms_map_combine(gms_map *dst, gms_map *src);
/* The scan de-skew of GridMapApp.onHandleData (J/app/GridMapApp.java:143-175): `length` raw measurements
 * {angle, distance, wasHit} and the frame's odometry -> beams (Observation.java:69-76), computed on the device
 * into the handle's staging buffer.  beams_out (host, may be NULL) receives a copy; *dev_beams_out (may be
 * NULL) its device address, valid until the next call that stages beams, for the *_dev entry points. */
int gms_map_deskew(gms_map *m, const double *angle, const double *distance, const uint8_t *hit, int32_t length,
                   double d_center, double d_theta, gms_beam *beams_out, const gms_beam **dev_beams_out);
/* getRawAt(map,x,y) / getProbAt (GridMap.java:134-140) for map index mi. */
int gms_map_get_raw_at(gms_map *m, int32_t mi, int32_t x, int32_t y, double *raw, double *prob);
/* getRawAt(map, Vec2 point) / getLikelihood(map, Vec2 point) (GridMap.java:142-156): the world point goes through
 * the reference's float arithmetic, (point - position) / resolution, intValue(), index x + y*W -- only the flat
 * index is range-checked there (ArrayIndexOutOfBounds -> GMS_ERR_INVALID here), so an x beyond the row reads the
 * neighbouring row exactly as the Java does.  raw / likelihood may be NULL. */
int gms_map_get_at_point(gms_map *m, int32_t mi, float point_x, float point_y, double *raw, double *likelihood);

/* GridMap.integrateObservation(map, obs, pose) (GridMap.java:173-191): beams[n_maps][B],
 * poses[n_maps][3] = x,y,theta. */
int gms_map_integrate(gms_map *m, const gms_beam *beams, int32_t B, const float *poses);
/* The same with the pose taken from a particle filter's device-resident weighted pose
 * (SLAM.getWeightedPose) or strongest particle -- no host round trip.  which: 0 weighted, 1 strongest. */
int gms_map_integrate_at(gms_map *m, const gms_beam *beams, int32_t B, gms_pf *pf, int32_t which);
/* GridMap.applyMeasurement(map,startX,startY,endX,endY,measuredDistance,wasHit) on map 0
 * (GridMap.java:194-228). */
int gms_map_apply_ray(gms_map *m, float sx, float sy, float ex, float ey, float measured, int32_t hit);
/* RayIterator(W,H).init(x0,y0,x1,y1,extra) + the hasNext/next loop, run on the device
 * (J/slam/RayIterator.java:65-130): ordered cells x0,y0,x1,y1,...; *n = number visited (may
 * exceed cap; only cap cells are stored). */
int gms_map_trace_ray(gms_map *m, float x0, float y0, float x1, float y1, int32_t extra,
                      int32_t *cells_xy, int32_t cap, int32_t *n);
/* The cell walk of integrateObservation for map 0 without touching the map: for beam b,
 * counts[b] cells; cells_xy/classes hold [B][cap] entries (class 0 free, 1 prior, 2 occupied:
 * J/slam/SensorModel.java:31-41). */
int gms_map_trace_scan(gms_map *m, const gms_beam *beams, int32_t B, const float pose[3],
                       int32_t *cells_xy, uint8_t *classes, int32_t cap, int32_t *counts);
/* GridMap.computeLikelihoodMap(map) (GridMap.java:233-250 + Util.java:378-426). */
int gms_map_build_likelihood(gms_map *m);
/* integrate + rebuild only the part of the likelihood field the scan can have changed (bit-identical
 * to gms_map_integrate followed by gms_map_build_likelihood when the field was current before). */
int gms_map_update(gms_map *m, const gms_beam *beams, int32_t B, const float *poses);
/* gms_map_update with the pose taken from the filter on the device (see gms_map_integrate_at). */
int gms_map_update_at(gms_map *m, const gms_beam *beams, int32_t B, gms_pf *pf, int32_t which);

/* ---- ParticleFilter / SLAM particle set -------------------------------------------------------- */
/* new ParticleFilter(n) (J/slam/ParticleFilter.java:43): n particles per map, weights 1/n_global,
 * poses 0 (SLAM.reset, J/slam/SLAM.java:65-77). */
int gms_pf_create(gms_map *m, int32_t n_particles, gms_pf **out);
int gms_pf_destroy(gms_pf *pf);
/* This handle holds particles [offset, offset+n) of a filter of n_global particles sharded over
 * several GPUs (offset % GMS_BLOCK == 0).  Default: offset 0, n_global = n. */
int gms_pf_set_shard(gms_pf *pf, int64_t offset, int64_t n_global);
/* getParticles() pose access (ParticleFilter.java:50): [n_maps][n][3] floats x,y,theta. */
int gms_pf_set_poses(gms_pf *pf, const float *xytheta);
int gms_pf_get_poses(gms_pf *pf, float *xytheta);
int gms_pf_set_weights(gms_pf *pf, const double *w);
int gms_pf_get_weights(gms_pf *pf, double *w);
int gms_pf_get_log_weights(gms_pf *pf, double *lw);
/* weight[i] = GridMap.probabilityOf(map, obs, pose[i]) for every particle (GridMap.java:261-294,
 * SLAM.java:99).  Also stores sum(log factor) per particle (underflow-free companion, not in the
 * reference).  beams[n_maps][B]. */
int gms_pf_score(gms_pf *pf, const gms_beam *beams, int32_t B);
/* SLAM.update's bookkeeping: weightSum, strongest, weight /= weightSum, calculateNeff
 * (SLAM.java:87-129,180-190) and getWeightedPose's sums (SLAM.java:165-178).  stats may be NULL
 * (no host synchronisation then); stats[n_maps]. */
int gms_pf_normalize(gms_pf *pf, gms_pf_stats *stats);
int gms_pf_get_stats(gms_pf *pf, gms_pf_stats *stats);
/* SLAM.getWeightedPose() (SLAM.java:165-178): out[n_maps][3]. */
int gms_pf_weighted_pose(gms_pf *pf, float *out);
/* SLAM.resample() (SLAM.java:133-153; class surface ParticleFilter.resample
 * J/slam/ParticleFilter.java:59-82) with Math.random() passed in as r01[n_maps].
 * Particles are replaced by copies (pose and weight).  indices (may be NULL): [n_maps][n] source
 * index per slot; n_ambiguous (may be NULL): slots whose boundary lies within rounding distance of
 * a cumulative weight, i.e. where a sequential and a blocked scan may legitimately disagree. */
int gms_pf_resample(gms_pf *pf, const double *r01, int32_t *indices, int32_t *n_ambiguous);
/* if (neff < fraction * n) resample()   (J/app/GridMapApp.java:185-186), decided on the device. */
int gms_pf_resample_if(gms_pf *pf, const double *r01, double fraction);
/* indices [n_maps][n]: the source slot of every particle after the last resampling step on this handle -- gms_pf_resample,
 * gms_pf_resample_if or the resample inside a scan step (SLAM.java:140-149; slot m itself where the conditional resample
 * did not run).  Synchronises the stream. */
int gms_pf_last_resample_indices(gms_pf *pf, int32_t *indices);
/* Particles held by this handle per map (ParticleFilter.java:43: `new Particle[n]`), maps, and the global population
 * of a sharded filter; any pointer may be NULL. */
int gms_pf_count(const gms_pf *pf, int32_t *n, int32_t *n_maps, int64_t *n_global);
/* flags[n_maps]: whether the last gms_pf_resample / gms_pf_resample_if replaced the particles. */
int gms_pf_did_resample(gms_pf *pf, int32_t *flags);
/* What the last normalise / scan step left on the device, per map (any pointer may be NULL): the weighted pose
 * (SLAM.getWeightedPose of the SCORED population, i.e. before a resample replaced it: the pose a fused scan step
 * integrated the scan at), the strongest particle's pose (SLAM.getStrongestParticle), whether the conditional
 * resample ran, and how many of its slots were ambiguous (see gms_pf_resample).  Synchronises the stream. */
int gms_pf_last_step(gms_pf *pf, float *weighted_pose, float *strongest_pose, int32_t *did_resample, int32_t *n_ambiguous);
/* SLAM.sampleMotionModel -> Odometry.apply(pose) for every particle (J/slam/SLAM.java:155-163,
 * J/slam/Odometry.java:60-96): Gaussian step and heading change with the reference's standard deviations
 * ((0.01 + 0.05|dCenter|)/2 and 5 deg + 0.1|dTheta|).  The reference's random stream is unseeded and
 * cannot be reproduced; variates come from Philox4x32-10(seed; global particle index, sequence), so a
 * sharded filter draws the same numbers as a stand-alone one. */
int gms_pf_sample_motion(gms_pf *pf, double d_center, double d_theta, uint64_t seed, uint64_t sequence);
/* GridMap.findBestPose(map, obs, startPose) lattice search around every particle
 * (GridMap.java:319-346): poses are replaced by the argmax pose. */
int gms_pf_refine_poses(gms_pf *pf, const gms_beam *beams, int32_t B);

/* SLAM.update refines every particle's pose before weighting it (J/slam/SLAM.java:96-97; the reference calls
 * findBestPoseOptim there, whose objective is broken -- SURVEY.md section 3.1 -- and keeps the lattice search
 * findBestPose commented out beside it).  on != 0: gms_slam_update / gms_slam_update_dev / the sharded scan steps run
 * gms_pf_refine_poses' lattice search (GridMap.java:319-346) on the motion-model samples before scoring them.
 * Default off (the search is 1210 probabilityOf evaluations per particle). */
int gms_pf_set_refine(gms_pf *pf, int32_t on);

/* Opt-in robust normalisation (not in the reference).  The reference's weight is the plain product of up
 * to 720 factors in [0.01, 0.91] (GridMap.java:262-288), which underflows for all but a handful of particles of a wide cloud: the
 * filter then runs on one survivor.  on != 0: the normalise step of this filter (gms_pf_normalize, the scan steps) takes
 * weight[i] = exp(logw[i] - max_j logw[j]) from the log-weights gms_pf_score keeps beside the products, and everything after it
 * -- weight sum, strongest, weighted pose, Neff, resampling -- runs on those weights as before (same blocked reductions; one more
 * launch in front of the block partials).  gms_pf_stats.weight_sum is then the sum of the rescaled weights (the largest is 1),
 * max_log_weight the scale.  Default off: the parity outputs are the reference's arithmetic.  Stand-alone filters only
 * (GMS_ERR_STATE on a shard); gms_pf_set_shard turns it off. */
int gms_pf_set_log_normalize(gms_pf *pf, int32_t on);

/* Reference-order audit (tests; slow on purpose).  The default kernels re-associate three chains of the reference's arithmetic: the
 * product of a scan's factors (GridMap.java:262-288: segment products, combined), weightSum (SLAM.java:100: blocked sums) and the
 * cumulative weights of resample() (SLAM.java:137-144: a three-level scan).  on != 0: gms_pf_score, gms_pf_normalize, gms_pf_resample[_if],
 * gms_pf_weighted_pose and the scan steps of this filter (which then take the separate launches) run each of them as ONE chain in
 * the reference's own order -- one register per particle for the product, one lane for the sums -- so that raw weights (zeros and
 * denormals included), the weight sum, Neff, the weighted pose and the resampling indices can be compared with the oracle for
 * EQUALITY, and the default path with this one: what differs between the two is association and nothing else.  Stand-alone filters. */
int gms_pf_set_reference_order(gms_pf *pf, int32_t on);

/* ---- SLAM as the reference has it: one GridMapData per particle --------------------------------------------------------------
 * J/slam/SLAM.java keeps a map in every Particle (:30-47): update() scores a particle against ITS OWN likelihood field and
 * integrates the scan into ITS OWN map at ITS OWN pose (:88-107), resample() deep-copies both arrays of the surviving particle's
 * map (:41-45 -> GridMap.createMapData(other), J/slam/GridMap.java:106-124).  The gms_pf entry points above score N poses against
 * ONE shared map (what BASELINE's configurations need); this handle is the reference's filter literally, at its own operating
 * point (500 particles x 120 x 120 cells, SLAM.java:50,57) and beyond.  Not the reference's: findBestPoseOptim (:97; BOBYQA on an
 * objective that is 0 / NaN) is left out, and the motion-model draw (:90) comes from Philox keyed by the particle's
 * slot index (see gms_pf_sample_motion). */
typedef struct gms_slam gms_slam;
/* new SLAM() (SLAM.java:56-62) + reset() (:65-77): n_particles particles at Pose(0, 0, 0) with weight 1 / n and a blank map each
 * (createMapData(null)).  p as for gms_map_create (the GridMap whose GridMapData every particle instantiates).
 * p->n_maps = S > 1 (at most 1024, S * n_particles at most 65535): S independent filters of n_particles particles in one handle -- a
 * batched handle.  Filter f's particle k is particle f * n_particles + k of every entry point that takes a particle index
 * (download_map / upload_map / trace_scan) and of the handle's gms_pf ([S][n] poses, weights, indices; its gms_pf_stats are per filter,
 * `strongest` filter-local); download_maps, reset and combined cover every filter (combined: filter f into map f of the handle's own
 * map).  Only the batch forms update and resample it (gms_slam_update_batch[_dev], gms_slam_resample_maps[_if]_batch); the calls that
 * take one scan, one odometry or one draw return GMS_ERR_STATE on it.  Every filter computes, bit for bit, what a stand-alone handle of
 * the same parameters computes from the same inputs and seed. */
int gms_slam_create(const gms_params *p, int32_t n_particles, gms_slam **out);
int gms_slam_destroy(gms_slam *s);
int gms_slam_reset(gms_slam *s);                                    /* SLAM.reset() (SLAM.java:65-77): every filter */
int gms_slam_count(const gms_slam *s, int32_t *n_particles, int32_t *W, int32_t *H);   /* n_particles: per filter */
/* The handles behind it, owned by the gms_slam (do not destroy them; the filter refuses gms_pf_resample[_if], gms_pf_set_shard and the
 * shared-map scan steps with GMS_ERR_STATE: they would move its particles without their maps): *map = SLAM.getGridMap() (:200) -- geometry, constants, the
 * stream every call of this handle runs on, and a GridMapData of its own that receives gms_slam_combined; *pf = getParticles()
 * (:192) without the maps: poses, weights and statistics through gms_pf_get_poses / gms_pf_set_poses / gms_pf_get_weights /
 * gms_pf_set_weights / gms_pf_get_stats / gms_pf_weighted_pose (getWeightedPose, :165-178) / gms_pf_last_step (strongest particle). */
int gms_slam_handles(gms_slam *s, gms_map **map, gms_pf **pf);
/* SLAM.update(z, u) (SLAM.java:80-131) for all particles: sampleMotionModel (:90; sample_motion == 0 is its `u == null` branch,
 * :159: the particles keep their poses, e.g. because the caller has set the samples with gms_pf_set_poses),
 * computeLikelihoodMap(p.m) (:93), p.weight = probabilityOf(p.m, z, p.pose) (:99; the product taken in beam order by one lane: the
 * reference's bits, underflow included), integrateObservation(p.m, z, p.pose) unless |dTheta| > 30 degrees (:82,102-107), weightSum,
 * strongest, weight /= weightSum (:100,110-121), calculateNeff (:124).  beams[B]; stats (may be NULL; when given the call
 * synchronises) receives update()'s return value as stats->neff, the weight sum and the strongest particle's index. */
int gms_slam_update_per_particle(gms_slam *s, const gms_beam *beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                                 uint64_t seed, uint64_t sequence, gms_pf_stats *stats);
int gms_slam_update_per_particle_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                                     uint64_t seed, uint64_t sequence, gms_pf_stats *stats);
/* SLAM.update(z, u) of every filter of a handle (any S, 1 included), one launch of each update kernel for all of them.  beams [S][B]:
 * filter f's scan is beams[f][0 .. counts[f]) (counts [S] may be NULL: all B; padding a scan is not neutral -- a beam that hits nothing
 * is still ray-cast), odometry [S][2] {dCenter, dTheta}, seeds [S], sample_motion [S] (0: keep the poses, as sample_motion of the scalar
 * call), one sequence: filter f's motion-model variates are Philox(seeds[f]; filter-local particle index, sequence), what a stand-alone
 * handle with seed seeds[f] draws.  skipUpdate (|dTheta| > 30 degrees, SLAM.java:82) is decided per filter.  stats [S] (may be NULL;
 * when given the call synchronises).  The host form stages the beams and the filters' table in one copy; _dev reads the caller's
 * device beams (row pitch B) and stages the table alone.  S = 1 runs exactly the scalar call. */
int gms_slam_update_batch(gms_slam *s, const gms_beam *beams, int32_t B, const int32_t *counts, const double *odometry, const uint64_t *seeds,
                          const int32_t *sample_motion, uint64_t sequence, gms_pf_stats *stats);
int gms_slam_update_batch_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, const int32_t *counts, const double *odometry,
                              const uint64_t *seeds, const int32_t *sample_motion, uint64_t sequence, gms_pf_stats *stats);
/* SLAM.update's pose refinement (SLAM.java:96-97): on != 0, every update runs GridMap.findBestPose (J/slam/GridMap.java:319-346: the
 * lattice of 11 x 11 x 10 poses around the motion-model sample, float loop counters, strict `>` against maxProb = 0 so that the first
 * maximum wins) for every particle against ITS OWN likelihood field, between computeLikelihoodMap(p.m) (:93) and the weighting (:99);
 * the particle is then weighted, and its map updated, at the refined pose.  The reference calls findBestPoseOptim (:97: BOBYQA from
 * commons-math on an objective that is 0 / NaN) and keeps this search commented out beside it (:96).  One workgroup per
 * particle; where the particle's field fits the CU's LDS as probabilityOf's factors (120 x 120 cells: 115 KB of 160) it is COMPUTED there
 * from the particle's class plane (no launch writes it first; blur kernels of 7 or 11 plain taps) or staged there from memory
 * (GMS_SLAM_REFINE_LDS=2 forces that form), and read from memory otherwise (GMS_SLAM_REFINE_LDS=0 forces that one).  Default off. */
int gms_slam_set_refine(gms_slam *s, int32_t on);
/* SLAM.resample() (SLAM.java:133-153) with Math.random() = r01: the systematic draw over the particles' weights, then every slot's
 * deep copy -- pose, weight (:42-43) and both arrays of the map (:44, GridMap.java:118-121): map[m] <- map[idx[m]], double-buffered,
 * a pure HBM stream.  logData moves at once (16 bytes per cell); likelihoodData's copy is made when something reads it -- a download,
 * an upload into a slot, another resample -- because the next update's computeLikelihoodMap overwrites every cell of it before
 * anything on the path does (what a caller can see is the deep copy either way; GMS_SLAM_LAZY_LIK_COPY=0 moves both at once).
 * indices [n] / n_ambiguous as gms_pf_resample (either may be NULL). */
int gms_slam_resample_maps(gms_slam *s, double r01, int32_t *indices, int32_t *n_ambiguous);
/* `if (neff < fraction * n) resample()` -- the rule of SLAM.update's caller (J/app/GridMapApp.java:185-186) -- decided ON THE DEVICE from the
 * Neff of the last update: nothing is read back, so update + this is one revolution without a host round trip.  Where the rule says no,
 * nothing is drawn and NOTHING IS COPIED, as in the reference: which of the two generations of the maps is current is itself a device-side
 * fact (a counter of the draws that ran, kept by the resampling kernel; every kernel of the handle picks the generation from its
 * parity), and the copy kernels return at once.  gms_pf_last_resample_indices (on the filter of gms_slam_handles) tells afterwards what
 * happened.  The threshold is fraction * n in doubles; the reference's `numParticles / 2` is an integer division, so for an odd
 * particle count its threshold is half a particle lower than fraction = 0.5's. */
int gms_slam_resample_maps_if(gms_slam *s, double r01, double fraction);
/* The same for every filter of a handle (any S): r01 [S], indices [S][n] FILTER-LOCAL source indices and n_ambiguous [S] (either may be
 * NULL); _if: each filter's rule decided on the device from its own Neff -- some filters may draw and others not, each keeps its own
 * generation of the maps. */
int gms_slam_resample_maps_batch(gms_slam *s, const double *r01, int32_t *indices, int32_t *n_ambiguous);
int gms_slam_resample_maps_if_batch(gms_slam *s, const double *r01, double fraction);
/* One recorded revolution as GridMapApp.onHandleData treats it (J/app/GridMapApp.java:133-192), for this filter, in one call: the raw
 * polar measurements are de-skewed with the frame's odometry (:143-175), then SLAM.update(z, u) (:178; skipUpdate decided from d_theta,
 * the pose refinement if gms_slam_set_refine is on) and `if (neff < resample_fraction * n) resample()` (:185-186; resample_fraction < 0
 * skips it).  Bit-identical to gms_map_deskew on the handle's map, gms_slam_update_per_particle_dev with sample_motion = 1 and
 * gms_slam_resample_maps_if, in that order; one small de-skew launch in front of the update's.  angle / distance / hit [length] are
 * host arrays and may be reused on return.  stats (may be NULL: nothing is read back, no synchronise; when given the call synchronises)
 * receives SLAM.update's return values, i.e. the Neff BEFORE the resampling.  One filter, not a shard. */
int gms_slam_frame_per_particle(gms_slam *s, const double *angle, const double *distance, const uint8_t *hit, int32_t length, double d_center,
                                double d_theta, uint64_t seed, uint64_t sequence, double r01, double resample_fraction, gms_pf_stats *stats);
/* The same for every filter of a handle (any S; S = 1 runs the scalar call): angle / distance / hit [S][L], row pitch L; filter f's
 * revolution is its first lengths[f] measurements (1 .. L; lengths may be NULL: all L) and is de-skewed with ITS OWN length (the d_i of
 * GridMapApp.java:150 divides by it) and odometry [f][2] {dCenter, dTheta} -- all S revolutions in one launch -- then
 * gms_slam_update_batch_dev with every filter drawing its motion sample (seeds [S], one sequence) and gms_slam_resample_maps_if_batch
 * (r01 [S]).  Every filter ends up bit-identical to a stand-alone handle of the same parameters and seed given
 * gms_slam_frame_per_particle.  The raw revolutions and the filters' table travel as one staging copy.  stats [S] (may be NULL). */
int gms_slam_frame_batch(gms_slam *s, const double *angle, const double *distance, const uint8_t *hit, int32_t L, const int32_t *lengths,
                         const double *odometry, const uint64_t *seeds, uint64_t sequence, const double *r01, double resample_fraction,
                         gms_pf_stats *stats);
/* ---- the reference-shape filter over several GPUs: particles WITH their maps, no replica ------------------------------------------
 * Rank r holds the contiguous block [r * n_local, (r + 1) * n_local) of the n_global particles (n_local a multiple of GMS_BLOCK) and
 * nothing else.  update(): gms_slam_update_local[_dev] (the per-particle body of SLAM.java:88-107 for this block; the motion model's
 * variates are keyed by the GLOBAL particle index), then the weight exchange of a sharded gms_pf on the filter of gms_slam_handles --
 * gms_pf_local_partials -> all-reduce(SUM) -> gms_pf_apply_partials -> all-gather -> gms_pf_import_global -- which gives every rank
 * weightSum, strongest, Neff and the weighted pose (SLAM.java:100-124,165-190) bit-identical to the one-GPU filter.  resample():
 * gms_slam_shard_draw on every rank with the same r01 (this rank's slots drawn from the gathered population; systematic resampling is
 * order-preserving, so a slot's source lives on this rank or a neighbouring one unless the weights have collapsed); the ranks
 * all-gather their `sources`, each sends the records (gms_slam_shard_export: logData + class planes, gms_slam_record_doubles doubles
 * per particle) of its particles that other ranks drew, and gms_slam_shard_gather makes the copies from the rank's own previous
 * generation and the received records.  The collectives stay with the caller (gridmap_slam_robot_amd/distributed.py:
 * ShardedSlamParticleMaps over torch.distributed = RCCL).  Poses, weights and every map equal the one-GPU gms_slam's for any number of
 * ranks.  A sharded handle needs the class planes (see gms_slam_create_shard's error text); its likelihoodData is produced on demand. */
int gms_slam_create_shard(const gms_params *p, int32_t n_local, int64_t offset, int64_t n_global, gms_slam **out);   /* p->n_maps == 1 */
int gms_slam_update_local(gms_slam *s, const gms_beam *beams, int32_t B, int32_t sample_motion, double d_center, double d_theta, uint64_t seed,
                          uint64_t sequence);
int gms_slam_update_local_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                              uint64_t seed, uint64_t sequence);
/* fraction < 0: unconditional; else `if (neff < fraction * n_global) resample()`.  *did: it drew; sources [n_local]: global source indices.
 * Synchronises.
 * The order of the three calls is kept by the handle.  A draw that drew (*did != 0) advances the maps' generation and opens export and
 * gather: gms_slam_shard_export may run any number of times, each reading the generation the draw left behind, and ONE
 * gms_slam_shard_gather makes the copies and closes both again -- a second gather would copy over maps that an update may have written
 * since.  Before the first draw, after a draw whose rule said no (*did == 0: no generation changed, there is nothing to move and the
 * "previous" generation is a stale one), after the gather and after gms_slam_reset both return GMS_ERR_STATE and touch nothing.  A
 * gather refused for its plan (a source out of range, a remote slot without a record) leaves the draw open.  recv_pos is not checked
 * against the length of dev_recv, which the call does not carry: that bound is the caller's. */
int gms_slam_shard_draw(gms_slam *s, double r01, double fraction, int32_t *did, int32_t *sources);
int gms_slam_record_doubles(const gms_slam *s, int64_t *doubles);
int gms_slam_shard_export(gms_slam *s, const int32_t *local_indices, int32_t count, double *dev_dst);
int gms_slam_shard_gather(gms_slam *s, const int32_t *src_local, const int32_t *recv_pos, const double *dev_recv);
/* The same with the exchanges inside the library (RCCL; gms_comm_* below): SLAM.update(z, u) and SLAM.resample() of one rank's block as
 * ONE call each -- what a Java host with one JVM per GPU calls through the shim.  update: gms_slam_update_local, then the all-reduce of
 * the block partials and the all-gather of the packed particles (gms_pf_normalize_sharded_begin / _end); stats (may be NULL): identical
 * on every rank.  resample: the draw, an all-gather of the sources, the plan (gms_slam_plan_exchange: a pure host function), the
 * records that cross a rank boundary as one grouped launch of ncclSend / ncclRecv, the copies; *did (may be NULL).  With more than one
 * rank these have never executed (one GPU per box where they were written); the torch.distributed route above is the tested one. */
int gms_slam_update_sharded_maps(gms_slam *s, gms_comm *c, const gms_beam *beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                                 uint64_t seed, uint64_t sequence, gms_pf_stats *stats);
int gms_slam_resample_sharded_maps(gms_slam *s, gms_comm *c, double r01, double fraction, int32_t *did);
int gms_slam_plan_exchange(const int32_t *all_sources, int32_t world, int32_t rank, int32_t n_local, int32_t *send_counts, int32_t *send_lists,
                           int32_t *recv_counts, int32_t *src_local, int32_t *recv_pos);
/* Particle i's GridMapData (SLAM.java:33; GridMap.java:72-74): W * H doubles each, either pointer may be NULL.  A batched handle: i over
 * [S * n], filter f's particle k = f * n + k; download_maps gives [S][n][H][W]. */
int gms_slam_download_map(gms_slam *s, int32_t i, double *log_data, double *lik);
int gms_slam_upload_map(gms_slam *s, int32_t i, const double *log_data, const double *lik);
int gms_slam_download_maps(gms_slam *s, double *log_all, double *lik_all);        /* all particles: [n][H][W] */
/* GridMapApp.calculateCombined (J/app/GridMapApp.java:439-458) over the particles' maps, likelihood field included (:457), into the
 * GridMapData of the handle's own map (gms_slam_handles -> gms_map_download_log / gms_map_download_likelihood); a batched handle: filter
 * f's into map f of it. */
int gms_slam_combined(gms_slam *s);
/* Diagnostics: the cell walk of integrateObservation(p.m, z, p.pose) (SLAM.java:105 -> GridMap.java:173-228) for particle i at its
 * current pose, exactly as the per-particle update kernel walks and classifies it, written out instead of counted: for beam b,
 * counts[b] cells in walk order (RayIterator.java:107-130), cells_xy / classes [B][cap] entries as gms_map_trace_scan (class 0 free,
 * 1 prior, 2 occupied; either may be NULL).  Touches no map.  Synchronises. */
int gms_slam_trace_scan(gms_slam *s, int32_t i, const gms_beam *beams, int32_t B, int32_t *cells_xy, uint8_t *classes, int32_t cap, int32_t *counts);
/* Diagnostics: filter f's de-skewed revolution as the last gms_slam_frame_per_particle / gms_slam_frame_batch call produced it, out
 * [cap] beams, *count its length (GMS_ERR_STATE before the first frame call; it holds until the next call that stages a scan on this
 * handle).  Synchronises. */
int gms_slam_last_beams(gms_slam *s, int32_t f, gms_beam *out, int32_t cap, int32_t *count);
/* maps copied by resampling steps since creation (measurement: bytes moved = copies * W * H * 32) */
int gms_slam_copies(const gms_slam *s, int64_t *maps_copied);

/* ---- map views: GridMap.render's grey levels, produced on the device ---------------------------------------------------------
 * GridMapApp.render (J/app/GridMapApp.java:374-393) hands one GridMapData -- the strongest particle's, a chosen particle's or the
 * combined map -- to GridMap.render (J/slam/GridMap.java:371-388), which turns every cell into a grey level.  A view is that picture
 * as one byte (or one packed colour word) per pixel: a rectangle of the map, optionally reduced, made by one streaming launch instead
 * of a download of W * H doubles and an exp per cell on the host.
 *
 * The grey level of a cell with log-odds l / likelihood L, bit for bit the Java's:
 *   value (double)  log view:        (double)1.0f - ((double)1.0f - (double)1.0f / (1.0 + exp(l)))
 *                                    (GridMap.java:384 `1.0f - Util.invLogOdds(logData[i])`, Util.java:46-48)
 *                   likelihood view: L                                                                  (GridMap.java:382)
 *   v   = (float)value
 *   idx = (int)(v * 255), a float multiply and Java's (int): NaN -> 0, truncation toward zero (Util.java:106-107).  Java would throw
 *         on an index outside the 256-entry LUT; THE CLAMP TO [0, 255] IS THIS LIBRARY'S, not the reference's.
 *   g   = (int)(255 * (idx / 256.0f)) in float: the LUT's ratio is i / 256f and Color.colorToFloatBits truncates 255 * ratio
 *         (Util.java:92-96, Color.java:62-65).  White is therefore 254, not 255.
 *   GMS_VIEW_GREY8:    the byte g.
 *   GMS_VIEW_PACKED32: 0xFE000000 | g << 16 | g << 8 | g -- the int bits colorToFloatBits(ratio, ratio, ratio, 1.0f) produces after its
 *                      `& 0xfeffffff` mask.
 *
 * The rectangle: cells [x0, x0 + w) x [y0, y0 + h), w, h >= 1, inside [0, W] x [0, H] (GMS_ERR_INVALID otherwise, nothing touched).
 * The output: ceil(w / decimate) x ceil(h / decimate) pixels, row-major, row 0 = y0 (logData's orientation), no row padding.  Pixel
 * (u, v) covers cells x0 + u d .. min(x0 + u d + d, x0 + w) - 1 and likewise in y: the last column and row may be ragged.
 * Decimation (d > 1) IS THIS LIBRARY'S OWN RULE -- the reference has none: a pixel is the cell of its block most likely to be
 * occupied, i.e. the minimum idx of the block in the log view and the maximum idx in the likelihood view, so that a wall one cell
 * wide does not vanish from an overview. */
enum { GMS_VIEW_GREY8 = 0, GMS_VIEW_PACKED32 = 1 };            /* gms_view.format: 1 / 4 bytes per pixel */
enum { GMS_VIEW_LOG = 0, GMS_VIEW_LIKELIHOOD = 1 };            /* gms_view.source: logData / likelihoodData */
#define GMS_VIEW_STRONGEST (-1)                                /* gms_slam_view's `which`: the strongest particle of filter gms_view.filter */
typedef struct gms_view {
    int32_t x0, y0, w, h;       /* the cell rectangle */
    int32_t decimate;           /* d >= 1 cells per pixel and axis */
    int32_t source;             /* GMS_VIEW_LOG / GMS_VIEW_LIKELIHOOD */
    int32_t format;             /* GMS_VIEW_GREY8 / GMS_VIEW_PACKED32 */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_view;
/* The output's size in pixels and bytes (any of the three may be NULL).  Pure host code: checks w, h, decimate >= 1, x0, y0 >= 0,
 * source and format -- not the map's bounds, which it does not know. */
int gms_view_size(const gms_view *v, int32_t *out_w, int32_t *out_h, int64_t *bytes);
/* Map mi of a shared or batched map, exactly as gms_map_download_log / gms_map_download_likelihood would return it at this moment (a
 * scan whose `logData +=` pass is still deferred and a lazily kept likelihood field included; like those downloads it changes no
 * later result of the handle).  out: `bytes` of host memory; the call synchronises.  _dev: out is device memory (4-byte aligned
 * for GMS_VIEW_PACKED32), written on the handle's stream; nothing is synchronised. */
int gms_map_view(gms_map *m, int32_t mi, const gms_view *v, void *out);
int gms_map_view_dev(gms_map *m, int32_t mi, const gms_view *v, void *dev_out);
/* One particle's map of the per-particle filter (GridMapApp.render's mapDrawSelect cases "strongest" and "chosen"; the combined map
 * is the handle's own gms_map: gms_slam_combined, then gms_map_view on the map of gms_slam_handles).  which >= 0: the particle, in
 * the index space of gms_slam_download_map (a batched handle: f * n + k).  which == GMS_VIEW_STRONGEST: the strongest particle of
 * filter v->filter, picked ON THE DEVICE from the statistics the last update left there (SLAM.java:110-115; they outlive a
 * resample(), as strongestParticle does) -- the host reads nothing back in front of the launch; GMS_ERR_STATE before the first
 * update, after gms_slam_reset until the next one, and on a shard of a filter (its strongest particle may live on another rank).
 * *shown (may be NULL) receives the index that was drawn, in `which`'s own index space (a batched handle: f * n + k, NOT the
 * filter-local gms_pf_stats.strongest); the host form reads it back in the image's synchronise, the _dev form takes a device int32_t *.
 * The generation of the maps is picked on the device from the epoch counters, as by every kernel of the handle.  The likelihood view
 * is the particle's likelihoodData as gms_slam_download_map would return it, wherever the handle keeps it: read in place, read from
 * the source of a resampling copy that is still owed, or -- where the fields are implicit in the class planes -- computed for the
 * SHOWN particle alone; no other particle's field is written, and the handle's state and later results do not change. */
int gms_slam_view(gms_slam *s, int32_t which, const gms_view *v, void *out, int32_t *shown);
int gms_slam_view_dev(gms_slam *s, int32_t which, const gms_view *v, void *dev_out, int32_t *dev_shown);

/* ---- trajectories: every particle's path, kept through resampling -------------------------------------------------------------
 * The per-particle filter estimates a path together with the map built along it (SLAM.java:33: a Particle is pose, weight and map).
 * The poses a caller collects frame by frame are NOT the path any returned map was built along: resample() rewrites slot m with the
 * map and pose of slot idx[m] (:41-45), and the next one can hand "strongest" to a particle with another past.  An opt-in history keeps,
 * on the device, what is needed to answer "where was the robot, according to the particle whose map is shown": a ring of the last
 * `capacity` updates, row t holding every slot's pose as it stood when update number t returned (what gms_pf_get_poses would have
 * given then: motion sample and, with gms_slam_set_refine, the refinement included) and the slot of row t - 1 the particle descends
 * from.  Every update of the handle -- gms_slam_update_per_particle[_dev], gms_slam_update_batch[_dev], the frame calls; one whose
 * scan is not integrated (|d_theta| > 30 degrees) or that draws no motion sample is a step like any other -- records one row; every
 * draw -- gms_slam_resample_maps[_if][_batch], the frame calls' -- composes its indices into the lineage, per filter and only where
 * the filter did draw, which the kernel reads on the device.  Nothing is read back, by these or by any other call of the handle.
 * Off (the default) the handle allocates nothing and launches nothing for it; on, an update and a resample each take one small
 * launch more on the handle's stream, and no result of any other call changes.
 *
 * gms_slam_set_history: capacity > 0 keeps the last `capacity` updates from now on (a history already kept is dropped); 0 turns it
 * off and frees its memory.  GMS_ERR_STATE on a shard of a filter (gms_slam_create_shard: ancestors cross ranks), GMS_ERR_INVALID for
 * a negative capacity, GMS_ERR_NOMEM where the device cannot hold it.  gms_slam_reset clears the history (no step kept) and keeps it
 * on at the same capacity; gms_pf_set_poses on the handle's filter, gms_slam_upload_map and gms_slam_combined do not touch it (a pose
 * set by hand shows in the rows recorded after it, never in one already there).
 * gms_slam_history_bytes: what gms_slam_set_history allocates for n_particles_total (= filters x particles) slots, with the same
 * checks and without a device: capacity * n * 16 (4 bytes of parent and 12 of pose per slot and row) + n * 8 (the lineage and the
 * buffer the next draw composes it into) + 16 (the device's step count and its ticket); 0 for capacity 0.  GMS_ERR_INVALID for a
 * particle count < 1, a negative capacity or a size beyond int64.
 * gms_slam_history_len: *steps_total = updates recorded since the history was turned on or cleared, *steps_kept = min(total,
 * capacity) (either may be NULL).  The host counts them itself: nothing is synchronised.  GMS_ERR_STATE while the history is off.
 *
 * gms_slam_trajectory: the path of ONE particle as it stands now -- `which` in the index space of gms_slam_view (>= 0: the slot, a
 * batched handle's f * n + k, `filter` ignored; GMS_VIEW_STRONGEST: the strongest particle of `filter`, picked on the device from
 * the statistics the last update left there, with gms_slam_view's GMS_ERR_STATE conditions) -- into xytheta [cap][3] floats, oldest
 * first: entry j is the pose at update number steps_total - kept + j of the ancestor the particle descends from, *count = kept (may
 * be NULL), *shown (may be NULL) the slot that was followed, as gms_slam_view reports it.  A slot resampled since the last update
 * yields the path of the particle it was copied from: the path its map was built along.  cap < kept: GMS_ERR_INVALID, *count set
 * to what is needed, nothing written.  kept == 0: GMS_OK, *count = 0.  GMS_ERR_STATE while the history is off.  Synchronises.
 * gms_slam_trajectory_dev: the same into device memory ([cap][3] floats and a device int32_t * or NULL), written on the handle's
 * stream; nothing is synchronised, and the count is gms_slam_history_len's.
 * gms_slam_trajectories: every particle of `filter` at once: xytheta [kept][n][3] (cap counts steps), oldest first, and -- ancestors
 * may be NULL -- ancestors [kept][n], the filter-local slot present particle k occupied at each kept step.  Synchronises.
 * None of the three changes the handle's state or any later result.
 *
 * The back-trace (one workgroup) follows the chains inside LDS: it stages the filter's parent rows there, newest first, a chunk of
 * rows at a time, the next chunk's loads in flight while the current one is walked, and gathers only the poses from memory.  Where
 * not one row of a filter fits a chunk buffer (more than 8192 particles per filter), or with GMS_SLAM_HISTORY_WALK=mem in the
 * environment at creation (tests), every look-up is a load.  gms_slam_history_walk_rows (diagnostics): the rows per chunk, 0 = the
 * memory form. */
int gms_slam_history_bytes(int32_t n_particles_total, int32_t capacity, int64_t *bytes);
int gms_slam_set_history(gms_slam *s, int32_t capacity);
int gms_slam_history_len(gms_slam *s, int64_t *steps_total, int32_t *steps_kept);
int gms_slam_trajectory(gms_slam *s, int32_t which, int32_t filter, float *xytheta, int32_t cap, int32_t *count, int32_t *shown);
int gms_slam_trajectory_dev(gms_slam *s, int32_t which, int32_t filter, float *dev_xytheta, int32_t cap, int32_t *dev_shown);
int gms_slam_trajectories(gms_slam *s, int32_t filter, float *xytheta, int32_t *ancestors, int32_t cap, int32_t *count);
int gms_slam_history_walk_rows(gms_slam *s, int32_t *rows);

/* ---- predicted scans: what the LIDAR would see in a map from a pose -----------------------------------------------------------
 * The inverse of integrateObservation, and this library's own definition (the reference has no such method).  A PROBE is a gms_beam
 * of which only local_x, local_y and distance are read (`hit` is ignored).  Casting probe b from pose p in a map walks exactly the
 * cells, in exactly the order, that integrateObservation(map, {b}, p) visits for it -- start and end point as GridMap.java:175-188,
 * rayIterator.init(start + 0.5f, end + 0.5f, extra_steps) as :210, the walk ending where it leaves the map as
 * RayIterator.java:107-130: the list gms_map_trace_scan returns for that beam -- and reports the FIRST cell of that walk whose
 * logData > logOdds(0.5) = 0, the class GridMap.java:239 maps to 1.  A cell at exactly 0, at -0.0 or NaN is not occupied.  A ray that
 * starts outside the map visits no cell (RayIterator.hasNext, :108) and reports none.
 * NB the walk includes the gms_params.extra_steps cells PAST the probe's end point (they are part of integrateObservation's walk), so
 * a wall up to that many steps beyond the end point is still reported; one step further it is not.
 * Every walk is cut after W + H + extra_steps + 2 cells whatever its inputs (non-finite poses and probes included; no defined walk is
 * that long), so a cast always terminates.
 *
 * A cast sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment (a scan whose `logData +=` pass
 * is still deferred is applied first, as by those downloads) and changes no later result of its handle.  Arguments are checked before
 * anything is enqueued (GMS_ERR_INVALID, nothing touched). */
typedef struct gms_cast_hit {
    int32_t step;               /* index of the cell in the walk (0 = the first cell next() returns); -1: no occupied cell on the walk */
    int32_t x, y;               /* that cell; -1, -1 when step < 0 */
    float range;                /* grid units.  step >= 0: applyMeasurement's `distance` of that cell (GridMap.java:215-217): dX = startX -
                                   (x + 0.5f), dY likewise, (float)sqrt(dX * dX + dY * dY) in float, every operation rounded, nothing fused.
                                   step < 0: the probe's own measuredDistance, (float)distance / resolution (:188).  The unit
                                   inverseSensorModel compares in: a predicted and a measured beam can be held against hit_tolerance */
} gms_cast_hit;
#define GMS_CAST_ALL (-2)                                      /* gms_slam_cast's `which`: every particle the handle holds */
/* Map mi of a shared or batched map: P poses (poses [P][3] = x, y, theta; 1 <= P <= GMS_MAX_PARTICLES) cast the same B probes
 * (1 <= B <= the handle's max_beams); out [P][B].  The host form stages its inputs, reads the records back and synchronises; _dev
 * takes device pointers (out 16-byte aligned), runs on the handle's stream and synchronises nothing.
 * The lanes of a workgroup walk neighbouring probes of one pose through a BIT PLANE of the map (logData > 0, one bit per cell), which
 * a pre-pass packs and the handle keeps until logData changes: repeated casts on an unchanged map do not rebuild it.  A workgroup
 * stages the window of the plane its rays can reach in LDS and walks there; where that window exceeds the LDS it asked for (64 KiB),
 * or with GMS_CAST_WALK=mem in the environment at creation (tests), it walks the plane in memory. */
int gms_map_cast(gms_map *m, int32_t mi, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_cast_hit *out);
int gms_map_cast_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B, gms_cast_hit *dev_out);
/* The same from the filter's device-resident weighted (which = 0) or strongest (1) pose, as gms_map_integrate_at takes it -- no host
 * round trip; out [n_maps][B]: map i of a batched handle is cast from ITS filter pose (one map: out [B]). */
int gms_map_cast_at(gms_map *m, const gms_beam *probes, int32_t B, gms_pf *pf, int32_t which, gms_cast_hit *out);
int gms_map_cast_at_dev(gms_map *m, const gms_beam *dev_probes, int32_t B, gms_pf *pf, int32_t which, gms_cast_hit *dev_out);
/* The per-particle filter: particles cast at THEIR OWN pose in THEIR OWN map.  which >= 0: that particle, in the index space of
 * gms_slam_download_map, out [B]; GMS_VIEW_STRONGEST: the strongest particle of `filter`, picked on the device exactly as gms_slam_view
 * picks it, with its GMS_ERR_STATE cases (before the first update, after a reset, on a shard), out [B]; *shown (may be NULL; _dev: a
 * device int32_t *) receives the index that was cast, as there; GMS_CAST_ALL: every particle the handle holds (a shard: its local
 * ones), out [n_total][B], nothing written to shown.  `filter` is read with GMS_VIEW_STRONGEST only (gms_slam_trajectory's rule).
 * Pose, its trig and the maps' generation come from device state (the epoch counters, like every kernel of the handle): nothing is
 * read back in front of the launch.  One workgroup per particle: it stages plane 0 of the particle's class planes (2 bits per cell,
 * 3.6 KB at 120 x 120) in LDS and the lanes walk the codes.  Handles that keep no planes (an eager field, a kernel wider than 15 taps,
 * a plane over 24 KiB), and every handle created with GMS_CAST_WALK=mem in the environment (tests), read logData itself. */
int gms_slam_cast(gms_slam *s, int32_t which, int32_t filter, const gms_beam *probes, int32_t B, gms_cast_hit *out, int32_t *shown);
int gms_slam_cast_dev(gms_slam *s, int32_t which, int32_t filter, const gms_beam *dev_probes, int32_t B, gms_cast_hit *dev_out, int32_t *dev_shown);

/* ---- clearance fields: how far the nearest wall is from a place ------------------------------------------------------------------
 * What collision warning, costmap inflation, path planning and the choice of exploration goals rest on, and this library's own
 * definition (the reference has no such method).  All of it is integer arithmetic.
 *
 * An OBSTACLE cell is chosen by gms_clearance.mode:
 *   GMS_CLEAR_OCCUPIED   logData > logOdds(0.5) = 0: the class GridMap.java:239 maps to 1 and the predicate the casts use.  NaN, 0 and
 *                        -0.0 are not obstacles.
 *   GMS_CLEAR_NOT_FREE   !(logData < 0): occupied or never observed; NaN counts as an obstacle.  What a planner wants that must not
 *                        drive into the unknown.
 * For a cell (x, y), d2 = min((x - ox)^2 + (y - oy)^2) over every obstacle cell (ox, oy) of the WHOLE map, not only of the requested
 * rectangle.  An obstacle cell has d2 = 0.  Cells outside the map are not obstacles (the map's border is none).  The output is one
 * uint16_t per cell: d2 where d2 <= max_radius^2, GMS_CLEAR_FAR otherwise -- farther than the radius, or no obstacle at all.
 * max_radius is in cells, 1 <= max_radius <= 255 (255^2 = 65025 fits).  The clearance in metres is sqrt(d2) * resolution, the caller's
 * to take.
 *
 * The rectangle: cells [x0, x0 + w) x [y0, y0 + h), w, h >= 1, inside [0, W] x [0, H] (GMS_ERR_INVALID otherwise, nothing touched):
 * gms_view's rules.  The output: [h][w], row-major, row 0 = y0 (logData's orientation), no row padding.
 *
 * A field sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment (a scan whose `logData +=` pass
 * is still deferred is applied first, a resampling copy that is owed is looked through, the generation of a per-particle map is picked
 * from the epoch counters) and changes no later result of its handle.  Arguments are checked before anything is enqueued
 * (GMS_ERR_INVALID, nothing touched).  These are the casts' rules. */
enum { GMS_CLEAR_OCCUPIED = 0, GMS_CLEAR_NOT_FREE = 1 };       /* gms_clearance.mode */
#define GMS_CLEAR_FAR 0xFFFF                                   /* farther than max_radius from every obstacle, or no obstacle at all */
#define GMS_CLEAR_OUTSIDE 0xFFFE                               /* gms_map_clearance_poses: the pose's cell is outside the map */
typedef struct gms_clearance {
    int32_t x0, y0, w, h;       /* the cell rectangle */
    int32_t max_radius;         /* cells, 1 .. 255 */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_clearance;
/* The output's size in cells and bytes (any of the three may be NULL).  Pure host code: checks w, h >= 1, x0, y0 >= 0, the radius
 * and the mode -- not the map's bounds, which it does not know. */
int gms_clearance_size(const gms_clearance *c, int32_t *out_w, int32_t *out_h, int64_t *bytes);
/* Map mi of a shared or batched map.  out: [h][w] uint16_t of host memory, staged through the views' buffer; the call synchronises.
 * _dev: out is device memory (2-byte aligned), written on the handle's stream; nothing is synchronised.
 * GMS_CLEAR_OCCUPIED reads the casts' bit plane: a field of a map whose plane is current packs none, and a cast after a field packs
 * none either (gms_map_cast_plane_builds).  GMS_CLEAR_NOT_FREE keeps a second plane of its own predicate beside it, by the same rules.
 * The field is the exact separable transform capped at max_radius: a workgroup stages the horizontal distances of its rows and of
 * max_radius rows above and below in LDS (at most 64 KiB) and every lane takes the minimum down its column. */
int gms_map_clearance(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *out);
int gms_map_clearance_dev(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *dev_out);
/* The clearance under P points (poses [P][3] = x, y, theta, of which theta is not read; 1 <= P <= GMS_MAX_PARTICLES) without making a
 * field; out [P].  The cell of a pose is probabilityOf's: gx = (int)((x - position.x) / resolution), gy likewise, in double with
 * Java's cast (GridMap.java:273-274: truncation toward zero, so a coordinate in (-1, 0) cells lands in cell 0; NaN -> 0).  A pose whose
 * cell is outside the map (:276) yields GMS_CLEAR_OUTSIDE; every other value is the field's at that cell. */
int gms_map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out);
int gms_map_clearance_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *dev_out);
/* One particle's map of the per-particle filter.  The rectangle's rules, the index space of `which` (>= 0: the particle, a batched
 * handle's f * n + k; GMS_VIEW_STRONGEST: the strongest particle of filter c->filter, picked on the device), *shown (may be NULL; _dev:
 * a device int32_t *) and the GMS_ERR_STATE cases of "strongest" (before the first update, after a reset, on a shard) are
 * gms_slam_view's.  Particle and generation come from device state: nothing is read back in front of the launches.  A pre-pass packs
 * the shown particle's obstacle bits -- from plane 0 of its class planes (code 2 occupied, code 1 free), or from logData itself on a
 * handle that keeps no planes -- into a scratch plane of the handle, and the shared maps' field kernel runs on that. */
int gms_slam_clearance(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *out, int32_t *shown);
int gms_slam_clearance_dev(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *dev_out, int32_t *dev_shown);

/* ---- sites and skeleton: which obstacle is the nearest one, and where free space is equally far from two walls --------------------
 * The site of a cell is what a reactive controller, a potential field, an ESDF gradient and a "push this waypoint off the wall" step
 * are made of; the skeleton is the generalised Voronoi diagram of the grid, the maximum-clearance roadmap: corridor centre lines,
 * doorways as local minima of the clearance along it, junctions as places to decide.  This library's own definition (the reference has
 * no such method).  All of it is integer arithmetic, and both results are unique.
 *
 * OBSTACLE.  gms_clearance's definition for `mode`: GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE.  Cells outside the map are no obstacles.
 *
 * SITE.  The site of a map cell c = (x, y) is the obstacle cell o = (ox, oy) of the WHOLE map that minimises the pair
 * (d2, oy * W + ox) lexicographically.
 *   - d2 = (x - ox)^2 + (y - oy)^2.
 *   - Only obstacles with d2 <= max_radius^2 count, and 1 <= max_radius <= 255.
 *   - Encoded as uint32_t oy * W + ox.
 *   - GMS_SITE_NONE = 0xFFFFFFFF where no obstacle lies within the radius.
 *   - An obstacle cell is its own site.
 *   - d2(c) is the site's distance.  By construction it equals what gms_map_clearance returns for the same mode and radius.
 *
 * SKELETON.  Parameters:
 *   - min_clear >= 1, in cells;
 *   - min_gap >= 2, in cells;
 *   - min_clear <= max_radius;
 *   - min_gap <= 2 * max_radius.
 * A map cell c is a skeleton cell iff all of these hold:
 *   1. c is no obstacle, site(c) != NONE, and d2(c) >= min_clear^2.
 *   2. c has an axis neighbour n (of the four, inside the map) that is no obstacle and has site(n) != NONE.  The squared distance
 *      between the two site cells must be >= min_gap^2.
 *   3. For that n: d2(c) > d2(n), or d2(c) == d2(n) and c's linear index is below n's.  So of a pair that straddles the ridge, the cell
 *      farther from the walls is marked.  A tie goes to the smaller index.
 * The neighbour n may lie outside the requested rectangle.  The definition is over the whole map.
 * Cells farther than max_radius from every obstacle carry no skeleton.  A caller who wants one in a large hall raises the radius.
 *
 * The outputs for the rectangle x0, y0, w, h (gms_view's rules; [h][w], row-major, row 0 = y0, no row padding).  Each may be NULL, but
 * not all of them:
 *   site    uint32_t [h][w]: as defined above.
 *   skel    uint16_t [h][w]: d2(c) where c is a skeleton cell, else 0 (min_clear >= 1 makes 0 unambiguous).  The non-zero values are
 *           the clearance along the skeleton, so doorways are its local minima.
 *   totals  one gms_skeleton_totals over the rectangle.
 * Tracing the skeleton into a graph of junctions and edges and pruning spurs are the caller's, from skel on the host.
 *
 * A call sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment, changes no later result of its
 * handle, checks its arguments before anything is enqueued (GMS_ERR_INVALID, nothing touched, the reason in gms_last_error) and reuses
 * a current plane without repacking (gms_map_cast_plane_builds): the clearance fields' rules.  A map of 2^32 - 2 cells or more is
 * refused. */
#define GMS_SITE_NONE 0xFFFFFFFFu                              /* no obstacle within max_radius */
#define GMS_SITE_OUTSIDE 0xFFFFFFFEu                           /* gms_map_nearest_poses: the pose's cell is outside the map */
typedef struct gms_skeleton {
    int32_t x0, y0, w, h;       /* the cell rectangle */
    int32_t max_radius;         /* cells, 1 .. 255 */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t min_clear;          /* cells, 1 .. max_radius: skeleton cells are at least this far from their site */
    int32_t min_gap;            /* cells, 2 .. 2 * max_radius: ... and separate sites at least this far apart */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
    int32_t pad[3];
} gms_skeleton;
typedef struct gms_skeleton_totals {
    int64_t sited;              /* cells of the rectangle with a site */
    int64_t skeleton;           /* skeleton cells of the rectangle */
    int32_t min_d2, max_d2;     /* over the skeleton cells; both 0 when there are none */
    int32_t pad[2];             /* zero */
} gms_skeleton_totals;
typedef struct gms_nearest {
    uint32_t site;              /* the site of the pose's cell, GMS_SITE_NONE or GMS_SITE_OUTSIDE */
    uint32_t d2;                /* its squared distance in cells, GMS_CLEAR_FAR or GMS_CLEAR_OUTSIDE */
} gms_nearest;
/* The outputs' size in cells and bytes (any of the four may be NULL).  Pure host code: checks w, h >= 1, x0, y0 >= 0, the radius, the
 * mode, min_clear and min_gap -- not the map's bounds, which it does not know.  This library's own definition. */
int gms_skeleton_size(const gms_skeleton *q, int32_t *out_w, int32_t *out_h, int64_t *site_bytes, int64_t *skel_bytes);
/* Map mi of a shared or batched map; this library's own definition, no reference method stands behind it.  site, skel, totals: host
 * memory, staged through the views' buffer; the call synchronises.  _dev: device memory (site 4-byte, skel 2-byte, totals 8-byte
 * aligned), written on the handle's stream; nothing is synchronised.  The sites are the clearance fields' separable transform with the
 * arg-min kept, into the caller's array where nothing else is asked for; skel and totals come from a second launch over a site field of
 * the rectangle and one cell around it, kept on the handle (it grows and never shrinks: no allocation per call once warm). */
int gms_map_skeleton(gms_map *m, int32_t mi, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals);
int gms_map_skeleton_dev(gms_map *m, int32_t mi, const gms_skeleton *q, uint32_t *dev_site, uint16_t *dev_skel, gms_skeleton_totals *dev_totals);
/* The site and its squared distance under P points without making a field; out [P]; this library's own definition.  The pose's cell
 * is gms_map_clearance_poses' (Java's cast, NaN -> 0).  {GMS_SITE_OUTSIDE, GMS_CLEAR_OUTSIDE} where that cell is off the map,
 * {GMS_SITE_NONE, GMS_CLEAR_FAR} where nothing lies within the radius; every other record is the field's at that cell.  _dev: out is
 * device memory, 4-byte aligned. */
int gms_map_nearest_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *out);
int gms_map_nearest_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *dev_out);
/* One particle's map of the per-particle filter; this library's own definition.  `which`, GMS_VIEW_STRONGEST, q->filter, *shown and
 * the GMS_ERR_STATE cases are gms_slam_view's.  gms_slam_clearance's pre-pass packs the shown particle's plane into the handle's
 * scratch plane, and the shared maps' kernels run on that. */
int gms_slam_skeleton(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals, int32_t *shown);
int gms_slam_skeleton_dev(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *dev_site, uint16_t *dev_skel, gms_skeleton_totals *dev_totals,
                          int32_t *dev_shown);

/* ---- cost-to-go fields: how far it is to drive from a set of places to everywhere else -------------------------------------------
 * What grid planners, the choice of exploration goals and every "can I get there at all" check start from, and this library's own
 * definition (the reference has no such method).  All of it is integer arithmetic, and the field is unique.
 *
 * BLOCKED: a cell is blocked if an obstacle cell under gms_reach.mode -- GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE, exactly the
 * clearance fields' predicates, NaN, 0 and -0.0 as there -- lies within `inflate` cells of it: d2 <= inflate^2, 0 <= inflate <= 255;
 * inflate = 0 blocks the obstacles alone.  Cells outside the map do not exist: they are neither obstacles nor traversable.  Every
 * other cell of the map is traversable.
 * MOVES are 8-connected: an axis step costs GMS_REACH_AXIS, a diagonal step GMS_REACH_DIAG, and a diagonal step is allowed only when
 * both cells it squeezes between -- the two axis neighbours that share the corner -- are traversable (no corner cutting).
 * SEEDS: seeds [K][2] int32_t (x, y) cells, 1 <= K <= GMS_REACH_MAX_SEEDS.  A seed that is off the map or blocked contributes nothing
 * and is no error; with no seed left the whole field is GMS_REACH_FAR and the call returns GMS_OK.  A traversable seed has cost 0.
 * THE FIELD: cost(c) = the minimum, over legal paths from any seed, of the summed step costs.  One uint16_t per cell: cost where
 * cost <= max_cost (1 <= max_cost <= 0xFFFE), GMS_REACH_FAR otherwise -- blocked, unreachable, or farther than the cap.  Candidate
 * costs are formed in 32 bits: a path that leaves the cap can never wrap into it.  Paths use the WHOLE map; only the output is a
 * rectangle.  In metres along axis steps: cost / GMS_REACH_AXIS * resolution.
 *
 * The rectangle, the [h][w] row-major output, the argument checks before anything is enqueued (GMS_ERR_INVALID, nothing touched),
 * "sees the map as a download would return it at that moment" and "changes no later result of its handle" are the clearance fields'
 * rules.
 *
 * How: the blocked plane is a bit plane in the casts' layout -- with inflate = 0 the casts' plane or the clearance fields' second
 * plane itself, read in place and packed only when stale (gms_map_cast_plane_builds does not move for a current plane); with
 * inflate > 0 the clearance field of the whole map at max_radius = inflate, balloted into a scratch plane.  The field is relaxed in a
 * uint16 working field of the whole map on the handle (allocated by the first field) in ROUNDS: one launch, one workgroup per
 * 64 x 64 tile; an active tile loads its cells and a one-cell halo into LDS, relaxes to its own fixpoint there, writes back, and marks
 * the neighbours across every edge or corner that changed active for the next round.  No workgroup waits on another.  The host
 * launches rounds in batches and reads the count of active tiles back once per batch (GMS_REACH_BATCH in the environment, default 8
 * rounds), so EVERY form, _dev included, waits on the handle's stream between batches -- unlike the other _dev forms.  After round k
 * every cell whose cheapest path crosses fewer than k tile borders is final, so rounds <= max_cost / GMS_REACH_AXIS + 2; exceeding
 * that returns GMS_ERR_INTERNAL instead of looping. */
#define GMS_REACH_AXIS 5                                       /* the cost of a step along an axis */
#define GMS_REACH_DIAG 7                                       /* ... and of a diagonal one */
#define GMS_REACH_FAR 0xFFFF                                   /* blocked, unreachable, or farther than max_cost */
#define GMS_REACH_MAX_SEEDS 4096
typedef struct gms_reach {
    int32_t x0, y0, w, h;       /* the cell rectangle of the output */
    int32_t max_cost;           /* 1 .. 0xFFFE */
    int32_t inflate;            /* cells, 0 .. 255 */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_reach;
/* The output's size in cells and bytes (any of the three may be NULL).  Pure host code: checks w, h >= 1, x0, y0 >= 0, max_cost,
 * inflate and the mode -- not the map's bounds, which it does not know, nor K. */
int gms_reach_size(const gms_reach *r, int32_t *out_w, int32_t *out_h, int64_t *bytes);
/* Map mi of a shared or batched map.  out: [h][w] uint16_t of host memory, staged through the views' buffer (the seeds behind it).
 * _dev: dev_seeds (4-byte aligned) and dev_out (2-byte aligned) are device memory, read and written on the handle's stream; the call
 * waits on that stream between batches of rounds and returns with the copy into dev_out enqueued, not waited for. */
int gms_map_reach(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out);
int gms_map_reach_dev(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out);
/* One particle's map of the per-particle filter: `which`, GMS_VIEW_STRONGEST, r->filter, *shown and the GMS_ERR_STATE cases are
 * gms_slam_view's (gms_slam_clearance's pre-pass packs the shown particle's obstacle bits).  Here only, K == 0 with seeds NULL means:
 * the seed is the SHOWN particle's own pose cell, (int)((x - position.x) / resolution) as probabilityOf takes it (GridMap.java:273-274),
 * picked on the device -- with "strongest", nothing is read back to learn where to plant it. */
int gms_slam_reach(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out, int32_t *shown);
int gms_slam_reach_dev(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out, int32_t *dev_shown);
/* The last field made on this handle (either may be NULL): the rounds launched, and the tile relaxations that actually ran (a round
 * launches every tile; those that are not active leave at once).  A gms_slam's: on the gms_map of gms_slam_handles. */
int gms_map_reach_stats(const gms_map *m, int32_t *rounds, int64_t *tile_runs);

/* ---- frontier regions: where the exploration goals are -----------------------------------------------------------------------------
 * The known-free cells that border never-observed space, grouped into regions a caller can rank -- with a cost-to-go field, by how far
 * it is to drive there.  This library's own definition (the reference has no such method); all of it is integer arithmetic and every
 * output is unique.
 *
 * CELL CLASSES: FREE is logData < 0, OCCUPIED is logData > 0, UNKNOWN is neither: 0, -0.0 and NaN.  In the planes' terms: free = not the
 * clearance fields' second plane; unknown = the second plane and not the casts' plane.
 * A FRONTIER CELL is a FREE cell with at least one of its four axis neighbours INSIDE the map UNKNOWN.  Cells outside the map are not
 * unknown: the map's border makes no frontier (the clearance fields' rule).  A diagonal-only unknown neighbour does not count.  With
 * inflate > 0 (0 <= inflate <= 255 cells) a cell with an OCCUPIED cell within `inflate` cells of it, d2 <= inflate^2, is no frontier
 * cell: exactly the cost-to-go fields' BLOCKED under GMS_CLEAR_OCCUPIED, so a goal is a cell gms_map_reach can give a cost.
 * A REGION is a maximal 8-connected set of frontier cells (plain 8-connectivity, no corner rule), taken over the WHOLE map.  Its
 * ANCHOR is its member with the smallest linear index y * W + x.
 *
 * Two outputs, either may be omitted (NULL):
 *   the LABEL FIELD   of the rectangle [x0, x0 + w) x [y0, y0 + h) -- gms_view's rules: inside [0, W] x [0, H], GMS_ERR_INVALID
 *                     otherwise, nothing touched --, uint32_t [h][w], row 0 = y0: every frontier cell holds its region's anchor index
 *                     y * W + x (whatever min_size is), every other cell GMS_FRONTIER_NONE.  The rectangle is checked even when no
 *                     label field is asked for.
 *   the REGION TABLE  gms_frontier records of the regions with count >= min_size (min_size >= 1), in ascending anchor order; the first
 *                     `cap` of them are stored, *n_found (may be NULL) is the number that qualify and may exceed cap.  cap == 0 with
 *                     records == NULL is allowed.
 * THE GOAL: `cost` (may be NULL) is a WHOLE-MAP uint16_t [H][W] field, what gms_map_reach returns for the full rectangle.  With it a
 * region's goal is its member of the smallest cost, ties to the smallest linear index, and goal_cost that cost; a region whose members
 * are all GMS_REACH_FAR, and every region when cost is NULL, has goal = (-1, -1) and goal_cost = GMS_REACH_FAR.
 *
 * "Sees the map as a download would return it at that moment" (a deferred apply pass is flushed first, an owed resampling copy is
 * looked through, the generation of a per-particle map is picked from the epoch counters), "changes no later result of its handle"
 * and the argument checks before anything is enqueued are the clearance fields' rules.  A map of 2^32 - 1 cells or more is refused.
 *
 * How: (1) the frontier plane, one bit per cell in the casts' layout, a lane per 64-bit word from the casts' plane and the clearance
 * fields' second plane read in place (packed only when stale: gms_map_cast_plane_builds does not move for a current plane), with
 * inflate > 0 also from the cost-to-go fields' blocked plane; (2) one workgroup per 64 x 64 tile -- a tile without a frontier cell
 * leaves at once -- unites its cells in LDS and writes every cell's label as the global index of the tile-local smallest member;
 * (3) the pairs of cells adjacent across a tile edge or corner are united in the global label field, lock-free, the larger root
 * always hung under the smaller, so the final root is the anchor; (4) every frontier cell chases to its root; (5) the roots are
 * numbered in anchor order by a scan over the root plane's word counts; (6) count, box, sums and goal by integer atomics, the lanes
 * of a wavefront that share a label combined first; (7) a second scan keeps the regions with count >= min_size.  Scans that span
 * workgroups are separate launches; no workgroup waits on another.  The number of regions is known on the device only: every form
 * reads it back once, together with *n_found, so EVERY form, _dev included, waits on the handle's stream once -- and once more in a
 * call that finds more regions than the handle's table holds so far: the table grows (it never shrinks) and steps 6 and 7 run
 * again. */
#define GMS_FRONTIER_NONE 0xFFFFFFFFu                          /* a label: no frontier cell */
typedef struct gms_frontiers {
    int32_t x0, y0, w, h;       /* the cell rectangle of the label field */
    int32_t min_size;           /* >= 1: the smallest region the table lists */
    int32_t inflate;            /* cells, 0 .. 255 */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
    int32_t pad;                /* not read */
} gms_frontiers;
typedef struct gms_frontier {   /* 56 bytes */
    int32_t anchor_x, anchor_y; /*  0,  4: the member of the smallest linear index */
    int32_t count;              /*  8: members */
    int32_t goal_cost;          /* 12: the goal's cost, or GMS_REACH_FAR */
    int32_t min_x, min_y;       /* 16, 20: the bounding box, inclusive */
    int32_t max_x, max_y;       /* 24, 28 */
    int32_t goal_x, goal_y;     /* 32, 36: the member of the smallest cost, or (-1, -1) */
    int64_t sum_x, sum_y;       /* 40, 48: the members' coordinate sums; the centroid is sum / count, the caller's division */
} gms_frontier;
/* The label field's size in cells and bytes (any of the three may be NULL).  Pure host code: checks w, h >= 1, x0, y0 >= 0, min_size
 * and inflate -- not the map's bounds, which it does not know. */
int gms_frontiers_size(const gms_frontiers *f, int32_t *out_w, int32_t *out_h, int64_t *bytes);
/* Map mi of a shared or batched map.  cost, labels, records: host memory, staged through the views' buffer.
 * _dev: dev_cost (2-byte aligned), dev_labels (4-byte aligned) and dev_records (8-byte aligned) are device memory, read and written
 * on the handle's stream (a misaligned pointer: GMS_ERR_INVALID, nothing touched); n_found stays a HOST pointer, and the call waits
 * on that stream as said above, so both outputs are complete when it returns. */
int gms_map_frontiers(gms_map *m, int32_t mi, const gms_frontiers *f, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap,
                      int32_t *n_found);
int gms_map_frontiers_dev(gms_map *m, int32_t mi, const gms_frontiers *f, const uint16_t *dev_cost, uint32_t *dev_labels, gms_frontier *dev_records,
                          int32_t cap, int32_t *n_found);
/* One particle's own map of the per-particle filter: `which`, GMS_VIEW_STRONGEST, f->filter, *shown (may be NULL; _dev: a device
 * int32_t *) and the GMS_ERR_STATE cases are gms_slam_view's.  gms_slam_clearance's pre-pass packs both of the shown particle's
 * planes, and the shared maps' kernels run on those. */
int gms_slam_frontiers(gms_slam *s, int32_t which, const gms_frontiers *f, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap,
                       int32_t *n_found, int32_t *shown);
int gms_slam_frontiers_dev(gms_slam *s, int32_t which, const gms_frontiers *f, const uint16_t *dev_cost, uint32_t *dev_labels, gms_frontier *dev_records,
                           int32_t cap, int32_t *n_found, int32_t *dev_shown);

/* ---- rooms and doors: from geometry to places ----------------------------------------------------------------------------------------
 * Which room a cell, a frontier goal or a particle is in, which rooms exist, which are connected and where the door between two of
 * them is: what an exploration or task planner builds on top of the fields above (visit rooms one at a time, rank frontiers per room,
 * plan room to room before planning cells).  The method is the morphological room segmentation of the survey literature (Bormann et
 * al., "Room segmentation: survey, implementation, and analysis", ICRA 2016) -- erode the free space until rooms fall apart, then grow
 * the pieces back by a wavefront -- stated in this library's own integer terms (the reference has no such method), so every output is
 * unique.  All of it is over the WHOLE map; only the two field outputs are a rectangle (gms_view's rules, as the frontier label field).
 *
 * TRAVERSABLE: a cell that the cost-to-go fields do not call BLOCKED for (mode, inflate), 0 <= inflate <= 254: exactly gms_map_reach's
 * rule, cells off the map included (they do not exist).
 * CORE CELL: a cell not BLOCKED for (mode, core), inflate < core <= 255.  Every core cell is traversable.
 * CORE: a maximal 4-connected set of core cells.  This equals connectivity under the cost-to-go fields' MOVES restricted to core
 * cells: a legal diagonal step needs both cells it squeezes between, and either of them joins its two ends by axis steps.  Its ANCHOR
 * is its member of the smallest linear index y * W + x, its size its cell count.
 * ROOM: a core with size >= min_core (min_core >= 1).  Rooms are ranked 0, 1, ... in ascending anchor order.  More than GMS_ROOMS_MAX
 * rooms: GMS_ERR_INVALID with the count in gms_last_error, no output written, the handle as good as before for later calls.
 * GROWTH: for every traversable cell c, key(c) = the lexicographic minimum of (summed step cost, rank of the room the path starts in)
 * over the cost-to-go fields' legal paths (axis GMS_REACH_AXIS, diagonal GMS_REACH_DIAG, no corner cutting, through traversable cells
 * only) from any cell of any room to c; paths whose cost exceeds max_cost (1 .. 0xFFFE) are dropped, and candidate costs are formed so
 * that they cannot wrap.  A cell of a room has (0, own rank).  Cells of cores that did not qualify are grown into like any other
 * traversable cell.  A cell equally far from two rooms belongs to the one with the smaller anchor.  A traversable cell that no room
 * reaches within max_cost, and every blocked cell, has no room.  This is a shortest-path problem over an ordered pair, so the fixpoint
 * is unique however the relaxation is scheduled.
 *
 * The outputs (each may be NULL):
 *   labels  uint32_t [h][w]: the anchor index of the cell's room, else GMS_ROOM_NONE.
 *   depth   uint16_t [h][w]: the cost component of key -- how far outside its room's core the cell lies; 0 inside the core,
 *           GMS_REACH_FAR where there is no room.
 *   rooms   one gms_room per room in rank order; the first cap_rooms are stored, *n_rooms (may be NULL) is the true number.
 *   doors   one gms_door per unordered pair of rooms a < b (by anchor) with at least one CONTACT: a pair of axis-adjacent cells (p, q)
 *           with label(p) = a and label(q) = b.  Diagonal contact does not count.  `count` is the number of contacts -- the door's
 *           width in cells, summed over all openings between the two rooms --, the box is over all contact cells, sum_x2 / sum_y2 are
 *           the sums of px + qx and py + qy: the mean opening position is sum / (2 count) cells, the caller's division.  In ascending
 *           (a, b) order; the first cap_doors are stored, *n_doors (may be NULL) is the true number.
 * cap == 0 with a NULL table is allowed for either.
 *
 * "Sees the map as a download would return it at that moment", "changes no later result of its handle" and the argument checks before
 * anything is enqueued (GMS_ERR_INVALID, nothing touched) are the clearance fields' rules.  A map of 2^32 - 1 cells or more is refused.
 *
 * How: (1) the blocked plane at R = core (gms_map_reach's inflation) becomes the core plane in a plane of this call's own, so that the
 * inflation at R = inflate can follow; (2) the cores by the frontiers' labelling with 4-connectivity -- tile-local union in LDS, the
 * lock-free union across tile edges, the chase to the root -- and their sizes by integer atomics at the root; (3) the roots with
 * size >= min_core ranked by a scan; their number is read back once; (4) every room cell gets the working key 0 << 16 | rank in a
 * uint32 field of the whole map, every other cell 0xFFFFFFFF, and the tiles around the rooms' rims are marked; (5) ROUNDS as
 * gms_map_reach's, on the key cost << 16 | rank, whose numeric order is the lexicographic one: a relaxation is
 * min(cur, neighbour + (step << 16)), one 32-bit store publishes cost and label together; rounds <= max_cost / GMS_REACH_AXIS + 2,
 * GMS_ERR_INTERNAL beyond (GMS_ROOMS_BATCH in the environment: rounds per read-back, default 8); (6) the room records by integer
 * atomics, the lanes that share a room combined first; (7) the contacts -- every cell looks east and south -- into an open-addressing
 * table on the handle, which doubles and is filled again while it is more than half full; the entries leave in key order: the doors
 * whose smaller room is a form one run, the runs are laid out by a scan over the rooms, and an entry's place within its run is the
 * number of smaller keys there -- work of the sum of the squared run lengths (a hall with 1000 doors: 10^6 loads).  EVERY
 * form, _dev included, waits on the handle's stream: once for the number of rooms, once per batch of rounds, once per door table. */
#define GMS_ROOM_NONE 0xFFFFFFFFu                              /* a label: no room */
#define GMS_ROOMS_MAX 0xFFFF                                   /* rooms a call can rank */
typedef struct gms_rooms {
    int32_t x0, y0, w, h;       /* the cell rectangle of labels and depth */
    int32_t core;               /* cells, inflate + 1 .. 255: the erosion that makes rooms fall apart */
    int32_t inflate;            /* cells, 0 .. 254: the robot's inflation, as in gms_reach */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t min_core;           /* >= 1: the smallest core that is a room */
    int32_t max_cost;           /* 1 .. 0xFFFE: how far a room grows out of its core */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
    int32_t pad[2];             /* not read */
} gms_rooms;                    /* 48 bytes */
typedef struct gms_room {       /* 56 bytes */
    int32_t anchor_x, anchor_y; /*  0,  4: the core's member of the smallest linear index */
    int32_t core_count;         /*  8: cells of the core */
    int32_t count;              /* 12: cells labelled with this room */
    int32_t min_x, min_y;       /* 16, 20: the bounding box of those cells, inclusive */
    int32_t max_x, max_y;       /* 24, 28 */
    int32_t max_depth;          /* 32: the largest depth among them */
    int32_t doors;              /* 36: door records that name this room */
    int64_t sum_x, sum_y;       /* 40, 48: their coordinate sums; the centroid is sum / count, the caller's division */
} gms_room;
typedef struct gms_door {       /* 48 bytes */
    uint32_t a, b;              /*  0,  4: the two rooms' anchor indices, a < b */
    int32_t count;              /*  8: contacts */
    int32_t min_x, min_y;       /* 12, 16: the bounding box of all contact cells, inclusive */
    int32_t max_x, max_y;       /* 20, 24 */
    int32_t pad;                /* 28: zero */
    int64_t sum_x2, sum_y2;     /* 32, 40: the sums of px + qx and of py + qy over the contacts */
} gms_door;
/* Pure host code: everything about the request but the map's bounds, which it does not know -- w, h >= 1, x0, y0 >= 0,
 * 0 <= inflate <= 254, inflate < core <= 255, the mode, min_core >= 1, 1 <= max_cost <= 0xFFFE.  gms_rooms_size also returns the
 * rectangle's size in cells and the two fields' sizes in bytes (any of the four may be NULL). */
int gms_rooms_check(const gms_rooms *q);
int gms_rooms_size(const gms_rooms *q, int32_t *out_w, int32_t *out_h, int64_t *label_bytes, int64_t *depth_bytes);
/* Map mi of a shared or batched map.  labels, depth, rooms, doors: host memory, staged through the views' buffer.
 * _dev: dev_labels (4-byte aligned), dev_depth (2-byte aligned), dev_rooms and dev_doors (8-byte aligned) are device memory, written on
 * the handle's stream (a misaligned pointer: GMS_ERR_INVALID, nothing touched); n_rooms and n_doors stay HOST pointers, and the call
 * waits on that stream as said above; it returns with the last copies into the outputs enqueued, not waited for. */
int gms_map_rooms(gms_map *m, int32_t mi, const gms_rooms *q, uint32_t *labels, uint16_t *depth, gms_room *rooms, int32_t cap_rooms, int32_t *n_rooms,
                  gms_door *doors, int32_t cap_doors, int32_t *n_doors);
int gms_map_rooms_dev(gms_map *m, int32_t mi, const gms_rooms *q, uint32_t *dev_labels, uint16_t *dev_depth, gms_room *dev_rooms, int32_t cap_rooms,
                      int32_t *n_rooms, gms_door *dev_doors, int32_t cap_doors, int32_t *n_doors);
/* One particle's own map of the per-particle filter: `which`, GMS_VIEW_STRONGEST, q->filter, *shown (may be NULL; _dev: a device
 * int32_t *) and the GMS_ERR_STATE cases are gms_slam_view's.  gms_slam_clearance's pre-pass packs the shown particle's obstacle bits,
 * and the shared maps' kernels run on those. */
int gms_slam_rooms(gms_slam *s, int32_t which, const gms_rooms *q, uint32_t *labels, uint16_t *depth, gms_room *rooms, int32_t cap_rooms, int32_t *n_rooms,
                   gms_door *doors, int32_t cap_doors, int32_t *n_doors, int32_t *shown);
int gms_slam_rooms_dev(gms_slam *s, int32_t which, const gms_rooms *q, uint32_t *dev_labels, uint16_t *dev_depth, gms_room *dev_rooms, int32_t cap_rooms,
                       int32_t *n_rooms, gms_door *dev_doors, int32_t cap_doors, int32_t *n_doors, int32_t *dev_shown);
/* The last call on this handle (any may be NULL): the rounds launched, the tile relaxations that actually ran, and how often the door
 * table was doubled and filled again.  A gms_slam's: on the gms_map of gms_slam_handles. */
int gms_map_rooms_stats(const gms_map *m, int32_t *rounds, int64_t *tile_runs, int32_t *door_rebuilds);
/* Measurement: with GMS_ROOMS_STAGES set in the environment a call waits on the stream at the end of each of its parts -- planes,
 * cores, rounds, fields and records, doors -- and keeps the host clock's microseconds of each; us [GMS_ROOMS_STAGES] receives those of
 * the last call on this handle, all 0 without the variable (nothing is waited for then). */
#define GMS_ROOMS_STAGES 5
int gms_map_rooms_stage_us(const gms_map *m, double *us);

/* ---- view gain: what a scan from a candidate pose would reveal -------------------------------------------------------------------
 * What a goal picker asks after "where are the frontiers and what does each cost": how much never-observed space a scan taken at a
 * candidate pose would see.  This library's own definition (the reference has no such method); all of it is integer arithmetic.
 *
 * A PROBE is a gms_beam of which local_x, local_y and distance are read, as for the casts.  For a candidate pose p, B probes and a map:
 *   the WALK       probe b walks the cells of rayIterator.init(start + 0.5f, end + 0.5f, 0), start and end point as
 *                  GridMap.java:175-188: the casts' walk WITHOUT the extra_steps cells past the end point, a prefix of that walk.
 *   the RANGE CUT  with (cx, cy) the walk's first cell, a cell (x, y) belongs to the walk only while max(|x - cx|, |y - cy|) <=
 *                  max_range (cells, 1 <= max_range <= 255); the walk ends at the first cell beyond.  It is monotone in both axes, so it
 *                  never comes back.
 *   OCCLUSION      the walk ends at, and includes, its first OCCUPIED cell (logData > 0, the casts' predicate).  UNKNOWN cells (logData
 *                  0, -0.0 or NaN) are walked through, as FREE ones (logData < 0) are: the frontier regions' three classes.
 *   the VISIBLE SET  a walk that starts outside the map visits nothing (RayIterator.hasNext), a walk ends where it leaves the map; the
 *                  visible set of a pose is the union over its probes of the cells walked.  Each cell counts once, however many probes
 *                  cross it (near the sensor nearly all of them do).
 * Every walk's loop carries the bound 2 * max_range + 2 whatever its inputs (non-finite poses and probes included; no walk inside the
 * range cut is that long), so a call always terminates.
 *
 * "Sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment" (a deferred `logData +=` pass is applied
 * first, an owed resampling copy is looked through), "changes no later result of its handle" and the argument checks before anything is
 * enqueued (GMS_ERR_INVALID, nothing touched) are the casts' rules.
 *
 * How: one workgroup per pose.  Both bit planes of the map are read in place (the casts' plane and the clearance fields' second one,
 * packed only when stale: gms_map_cast_plane_builds does not move for a gain after a cast on an unchanged map).  The workgroup keeps a
 * visited bitmap of the square of side 2 * max_range + 1 around the start cell, clipped to the map, in LDS (at most 17 words x 511
 * rows, 35 KB); its lanes stride over the probes and set their cells' bits; then the bitmap is classed word by word against the planes
 * with population counts.  Where the bitmap and both plane windows fit 64 KiB of LDS together the plane windows are staged there too;
 * otherwise, and on every handle created with GMS_GAIN_WALK=mem in the environment (tests), plane bits are read from memory -- the
 * same records either way. */
typedef struct gms_gain {
    int32_t max_range;          /* cells, 1 .. 255: the half side of the square a scan is taken to see */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_gain;
typedef struct gms_gain_rec {   /* 32 bytes */
    int32_t unknown;            /*  0: distinct visible cells with logData 0, -0.0 or NaN */
    int32_t free_cells;         /*  4: ... with logData < 0 */
    int32_t occupied;           /*  8: ... with logData > 0 (each ended at least one walk) */
    int32_t hits;               /* 12: probes whose walk ended on an occupied cell */
    int32_t walked;             /* 16: probes that visited at least one cell */
    int32_t start_x, start_y;   /* 20, 24: the walks' first cell; -1, -1 when no probe walked (every count is then 0) */
    int32_t pad;                /* 28: always 0 */
} gms_gain_rec;
/* Map mi of a shared or batched map: P candidate poses (poses [P][3] = x, y, theta; 1 <= P <= GMS_MAX_PARTICLES) and the same B probes
 * for each (1 <= B <= the handle's max_beams); out [P].  The host form stages its inputs, reads the records back and synchronises; _dev
 * takes device pointers (out 16-byte aligned), runs on the handle's stream and synchronises nothing. */
int gms_map_gain(gms_map *m, int32_t mi, const gms_gain *g, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_gain_rec *out);
int gms_map_gain_dev(gms_map *m, int32_t mi, const gms_gain *g, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B,
                     gms_gain_rec *dev_out);
/* The per-particle filter: the CALLER'S candidate poses in the map of the shown particle.  `which`, GMS_VIEW_STRONGEST, g->filter,
 * *shown (may be NULL; _dev: a device int32_t *) and the GMS_ERR_STATE cases are gms_slam_view's; particle and generation are picked
 * on the device, nothing is read back in front of the launches.  There is no GMS_CAST_ALL form: candidates are places in ONE map.
 * gms_slam_frontiers' pre-pass packs both of the shown particle's planes, and the shared maps' kernel runs on those. */
int gms_slam_gain(gms_slam *s, int32_t which, const gms_gain *g, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_gain_rec *out,
                  int32_t *shown);
int gms_slam_gain_dev(gms_slam *s, int32_t which, const gms_gain *g, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B,
                      gms_gain_rec *dev_out, int32_t *dev_shown);

/* ---- particle seeding: spread a filter over the places the robot can be ------------------------------------------------------------
 * What global localisation on a known map starts from, and the recovery step of a Monte-Carlo localiser -- a share of the slots
 * replaced by fresh uniform samples after a resample -- needs on the per-scan path: slots of a shared-map filter receive poses drawn
 * uniformly over the eligible cells of their map, on the device.  This library's own definition (the reference has no such method: its
 * reset() puts every particle at the origin, as gms_pf_create does).
 *
 * ELIGIBLE: a cell of map mi is eligible if it is FREE (logData < 0, the frontier regions' class: NaN, 0 and -0.0 are not free), lies
 * inside the rectangle [x0, x0 + w) x [y0, y0 + h) (gms_view's rules) and is not BLOCKED exactly as the cost-to-go fields define it
 * under `mode` and `inflate`: no obstacle cell of the WHOLE map within d2 <= inflate^2.  With inflate = 0 both modes give the free
 * cells.  The map is seen as gms_map_download_log would return it at that moment: a deferred `logData +=` pass is applied first.
 * RANK: the eligible cells of a map in ascending order of y * W + x; M is their number, per map.
 * THE DRAW for slot i of map mi: one Philox4x32-10 block with key `seed` and counter {g, sequence}, g = (shard offset + i) +
 * ((uint64_t)mi << 40) -- the motion model's counter layout (gms_pf_sample_motion), so a shard draws what the stand-alone filter draws
 * for the same global slot; give seeding a `sequence` the motion model does not use.  With the output words c[0..3]:
 *   the cell   r = the high 64 bits of ((uint64_t)c[0] << 32 | c[1]) * M; the cell (cx, cy) is the r-th eligible one, 0-based.
 *   in it      jx = (float)(32768 + 7 * (c[2] >> 16)) * 2^-19, jy likewise from c[2] & 0xFFFF: multiples of 2^-19 in [1/16, 15/16),
 *              exact in float; with jitter == 0 both are 0.5f.
 *   the pose   fx = (float)cx + jx (one float add); x = (float)((double)position.x + (double)fx * (double)resolution) -- the product of
 *              two floats is exact in double, so nothing here can be contracted --; y likewise;
 *              theta = (float)(((double)(c[3] >> 8) - 8388607.5) * (pi * 2^-23)), inside (-pi, pi).
 * WRITTEN: a slot of [first, first + count) gets that pose, its cached trig, the weight 1.0 / n_global and the log-weight 0.0, as
 * gms_pf_create leaves them; every other slot is untouched, bit for bit.  Afterwards the filter is in the state gms_pf_set_poses
 * followed by gms_pf_set_weights leaves.  A map with M == 0 writes nothing to its filter, and the call still returns GMS_OK.
 * THE CELL GUARANTEE: the cell of a written pose under gms_map_clearance_poses' rule, (int)(((double)x - position.x) / resolution), is
 * the drawn cell.  With Q = (|position| + extent) / resolution along an axis: fx is off its exact value by at most Q * 2^-24 cells (one
 * float rounding of a number below Q), the float rounding of x moves it by at most |x| * 2^-24 <= Q * 2^-24 cells, and the three double
 * roundings on the way there and back by at most 3 * Q * 2^-53: Q * (2^-23 + 3 * 2^-53) in all, below the margin of 1/16 cell on either
 * side while Q < 2^19.  A map with Q > 2^18 along either axis (|error| <= 1/32 cell there) is refused with GMS_ERR_INVALID.
 *
 * Arguments are checked before anything is enqueued (GMS_ERR_INVALID, nothing touched): the rectangle inside the map, inflate, mode,
 * jitter 0 or 1, first >= 0, count >= 1, first + count <= n, and a map whose plane (H rows of (W + 63) / 64 words) exceeds 2^20 words.
 * GMS_ERR_STATE on the filter of a gms_slam: its particles live in their own maps and there is no one map to draw from.  A batched
 * handle (n_maps > 1) is served in one call: map mi's filter draws from map mi.
 * n_eligible [n_maps] may be NULL: nothing is read back and nothing is synchronised -- the per-scan injection path.  Otherwise the
 * call synchronises once and stores M per map.
 *
 * How: (1) a lane per 64-bit plane word forms ~not-free & ~blocked & the rectangle's mask from the clearance fields' second plane read
 * in place (packed only when stale: gms_map_cast_plane_builds does not move) and, with inflate > 0, the cost-to-go fields' blocked
 * plane, and stores the word and its population count; (2) the counts are scanned, per map, in two launches -- blocks of 1024 words,
 * then the blocks' totals, whose total is M; no workgroup waits on another --; (3) a lane per slot draws, searches the prefix for the
 * word that holds rank r -- every 32nd word's prefix (coarser on planes of more than 2^18 words, or with GMS_SCATTER_SHIFT in the
 * environment at the handle's creation: tests) staged in LDS, at most 32 KiB, the rest of the search in memory --, selects the set bit by
 * halving population counts and writes pose, trig and weight.  M is read from device memory by that launch, never by the host.
 * The table of (1) and (2) is kept on the gms_map and reused while logData is unchanged and the rectangle, inflate and mode are the
 * same: a scatter on an unchanged map is launch (3) alone (gms_map_scatter_table_builds does not move). */
typedef struct gms_scatter {
    int32_t x0, y0, w, h;       /* the cell rectangle the poses are drawn from */
    int32_t inflate;            /* cells, 0 .. 255 */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE: what `inflate` keeps away from */
    int32_t first, count;       /* slots [first, first + count) of every map's filter, local to this handle; count >= 1 */
    int32_t jitter;             /* 0: cell centres; 1: a position inside the cell */
    int32_t pad;                /* not read */
} gms_scatter;
/* Pure host code, as gms_reach_size: everything about the request but the map's and the filter's bounds, which it does not know. */
int gms_scatter_check(const gms_scatter *sc);
int gms_pf_scatter(gms_pf *pf, const gms_scatter *sc, uint64_t seed, uint64_t sequence, int64_t *n_eligible);
/* diagnostics: seeding tables built on this handle so far (tests: a scatter on an unchanged map with the same request builds none) */
int gms_map_scatter_table_builds(const gms_map *m, int64_t *builds);

/* ---- global scan matching: which poses explain a scan best, anywhere in the map ---------------------------------------------------
 * What start-up on a saved map, a kidnapped robot and a loop-closure check against an old map ask: given ONE scan and a map, the poses
 * of a whole rectangle that explain it best -- without a scattered filter and several revolutions.  The multi-resolution correlative
 * search (Olson 2009; what Cartographer uses for loop closure) on bit planes.  This library's own definition (the reference has no such
 * method: its findBestPose looks at 1210 poses around a start that is nearly right); all of it is integer arithmetic, and what is
 * returned is the result of the exhaustive search.
 *
 * The HIT PLANE: a cell is a HIT cell if an obstacle cell under `mode` (GMS_CLEAR_OCCUPIED: logData > 0; GMS_CLEAR_NOT_FREE:
 *   !(logData < 0)) of the whole map lies within tol cells of it, d2 <= tol^2, 0 <= tol <= 255: exactly the cost-to-go fields' BLOCKED
 *   plane at inflate = tol, and with tol == 0 the obstacle plane itself, read in place.  Cells outside the map are never hits.
 * The scan as OFFSETS: int16_t offsets [n_theta][B][2]; (dx, dy) is the end cell of beam b relative to the pose's cell under heading
 *   index k.  The pair (GMS_LOCATE_SKIP, GMS_LOCATE_SKIP) marks a beam that does not count; any other component must lie in
 *   [-4095, 4095].  The host forms check that (GMS_ERR_INVALID).  For the _dev forms it is a PRECONDITION: a pair with a component
 *   outside that range is treated as SKIP on the device and never used as an address.
 * gms_locate_offsets makes the table from a scan; pure host code, usable without a device.  For k = 0 .. n_theta - 1:
 *   theta = theta0 + (double)k * dtheta;  c = cos(theta), s = sin(theta) (libm);
 *   ex = (double)local_x * c - (double)local_y * s,  ey = (double)local_x * s + (double)local_y * c -- both products and the sum each
 *   rounded on their own, never fused (the library is compiled with -ffp-contract=off);
 *   dx = (int)floor(ex / (double)resolution + 0.5), dy likewise: the pose stands at the centre of its cell.
 *   A beam with hit == 0, a non-finite coordinate, or |dx| or |dy| > 4095 becomes SKIP.
 * CANDIDATES: (k, x, y) with 0 <= k < n_theta and (x, y) a cell of the rectangle [x0, x0 + w) x [y0, y0 + h) (gms_view's rectangle
 *   rules); with free_only = 1 only FREE cells (logData < 0, the frontier regions' class).  n_theta * w * h may not exceed 2^31 - 1, a
 *   side of the map not 2^20 cells.
 * SCORE(k, x, y): the number of non-SKIP beams b whose cell (x + dx, y + dy) is inside the map and is a HIT cell.
 * THE RESULT: with N the number of candidates of SCORE >= min_score (1 <= min_score <= B): *n_out = min(cap, N), 1 <= cap <= 4096;
 *   out[0 .. n_out) holds the first n_out of them in the order score descending, then k, then y, then x ascending; out[n_out .. cap) is
 *   set to {0, -1, -1, -1}.  N itself is NOT returned: the call may therefore raise its working threshold to the cap-th best score it
 *   has proven and never look at the candidates below it.  That changes nothing that is returned.
 *
 * "Sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment" (a deferred `logData +=` pass is applied
 * first, an owed resampling copy is looked through), "changes no later result of its handle" and the argument checks before anything is
 * enqueued (GMS_ERR_INVALID, nothing touched) are the casts' rules.  B ranges over 1 .. the handle's max_beams; a batched map handle
 * serves map mi.
 *
 * How: the obstacle plane comes from the query base, read in place (packed only when stale: gms_map_cast_plane_builds does not move
 * for a plane that is current), the hit plane for tol > 0 from the cost-to-go fields' inflation.  (1) An OR PYRAMID P_0 .. P_L in the
 * planes' layout: bit (x, y) of P_l is the OR of the hit plane over [x, x + 2^l) x [y, y + 2^l) clipped to the map -- the window slides,
 * nothing is decimated --, a lane per 64-bit word with funnel shifts across word boundaries.  (2) The search runs breadth first, one
 * launch per level l = L .. 0 over a work list: a level-l candidate (k, bx, by), bx - x0 and by - y0 multiples of 2^l, stands for the
 * translations of its 2^l x 2^l block; its BOUND, the number of non-SKIP beams with bit (bx + dx, by + dy) of P_l set (a coordinate in
 * [-(2^l - 1), -1] clamped to 0: the window only grows), is at least every SCORE in the block.  A wavefront per candidate strides its
 * lanes over the beams and counts with ballots.  A candidate whose BOUND is not below the threshold hands its children inside the
 * rectangle to the next level.  The threshold starts at min_score and rises to the cap-th largest score of the leaves proven so far
 * (every candidate also scores its block's own origin against P_0 into a histogram of B + 1 counters).  Pruning is strict, BOUND <
 * threshold, so ties at the cut survive to the ranking.  (3) Level 0 computes scores, applies free_only and the threshold, and one
 * workgroup selects and orders the best cap by the 64-bit key (B - score, k, y, x).  No workgroup waits on another.
 * L comes from the rectangle (the largest L <= 7 with 2^(L+2) <= max(w, h)); GMS_LOCATE_LEVELS=n in the environment at the handle's
 * creation forces it (tests; n = 0 is the exhaustive search on the device).  The same records at every L.
 * The call WAITS ON THE STREAM once per level -- it reads the next work list's length back, eight words, as gms_map_reach_dev does
 * between batches of rounds --, the _dev forms included; the host forms once more for the records.  A work list that would exceed 2^24
 * entries returns GMS_ERR_NOMEM with the advice to raise min_score or shrink the rectangle, and nothing is written to the outputs.
 * The pyramid (7 planes), the lists and the control words live on the handle, allocated by the first request; the lists only grow. */
#define GMS_LOCATE_SKIP (-32768)                               /* INT16_MIN in both components: a beam that does not count */
typedef struct gms_locate {
    int32_t x0, y0, w, h;       /* the cell rectangle of candidate positions */
    int32_t n_theta;            /* heading indices, 1 .. 1024: the rows of the offset table */
    int32_t tol;                /* cells, 0 .. 255: how far from an obstacle cell a beam's end cell still counts */
    int32_t mode;               /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE: what an obstacle cell is */
    int32_t min_score;          /* 1 .. B: candidates below it are never returned */
    int32_t cap;                /* 1 .. 4096: records returned at most */
    int32_t free_only;          /* 1: only FREE cells are candidates; 0: every cell of the rectangle */
    int32_t filter;             /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
    int32_t pad;                /* not read */
} gms_locate;
typedef struct gms_locate_rec { /* 16 bytes */
    int32_t score;              /*  0: SCORE(k, x, y); a filler record: 0 */
    int32_t k;                  /*  4: the heading index; a filler record: -1 */
    int32_t x, y;               /*  8, 12: the pose's cell; a filler record: -1, -1 */
} gms_locate_rec;
/* Pure host code, as gms_scatter_check: everything about the request but the map's bounds and B, which it does not know. */
int gms_locate_check(const gms_locate *lc);
/* Pure host code: the offset table of a scan (above); offsets [n_theta][B][2]. */
int gms_locate_offsets(const gms_beam *beams, int32_t B, double theta0, double dtheta, int32_t n_theta, double resolution, int16_t *offsets);
/* Map mi of a shared or batched map; out [cap], *n_out the records that count.  The host form stages the table, reads the records
 * back and synchronises; _dev takes device pointers (dev_out 16-byte aligned, dev_n_out a device int32_t *, the table 4-byte aligned)
 * and runs on the handle's stream, on which it waits once per level. */
int gms_map_locate(gms_map *m, int32_t mi, const gms_locate *lc, const int16_t *offsets, int32_t B, gms_locate_rec *out, int32_t *n_out);
int gms_map_locate_dev(gms_map *m, int32_t mi, const gms_locate *lc, const int16_t *dev_offsets, int32_t B, gms_locate_rec *dev_out,
                       int32_t *dev_n_out);
/* The per-particle filter: the scan against the map of the shown particle.  `which`, GMS_VIEW_STRONGEST, lc->filter, *shown (may be
 * NULL; _dev: a device int32_t *) and the GMS_ERR_STATE cases are gms_slam_view's; particle and generation are picked on the device. */
int gms_slam_locate(gms_slam *s, int32_t which, const gms_locate *lc, const int16_t *offsets, int32_t B, gms_locate_rec *out, int32_t *n_out,
                    int32_t *shown);
int gms_slam_locate_dev(gms_slam *s, int32_t which, const gms_locate *lc, const int16_t *dev_offsets, int32_t B, gms_locate_rec *dev_out,
                        int32_t *dev_n_out, int32_t *dev_shown);
/* diagnostics of the last request on this handle (a gms_slam's: gms_slam_handles' map), as gms_map_reach_stats: *levels = L, evaluated
 * [8] = the candidates evaluated at level l (0 beyond L, and below a level that left no candidate).  Either may be NULL. */
int gms_map_locate_stats(const gms_map *m, int32_t *levels, int64_t *evaluated);

/* ---- pose modes: the hypotheses a particle cloud still holds ---------------------------------------------------------------------------
 * What a localiser on a scattered filter asks every scan: how many hypotheses are left, where is each, how much weight does it hold and
 * how tight is it -- the heaviest cluster's pose and covariance, and "has the filter converged" as "does one cluster hold nearly all
 * the weight".  gms_pf_weighted_pose's single mean is a pose in the wall between two rooms that look alike.  This library's own
 * definition (the reference has no such method), in the frontier regions' style: everything that can be integer is integer, and the
 * floating-point sums have one stated order, so every output is unique.
 *
 * THE BIN of a particle (x, y, theta) of map mi's filter: its cell (gx, gy) is gms_map_clearance_poses' (NaN -> 0 and the toward-zero
 * cast included), and the particle is OUTSIDE exactly where that call returns GMS_CLEAR_OUTSIDE: gx < 0 || gy < 0 || gx >= W || gy >= H.
 * The heading bin: k = (double)n_theta * 0.15915494309189535 (one double multiply), v = (double)theta * k, f = floor(v); a non-finite
 * f, or |f| >= 2^31, makes the particle OUTSIDE; otherwise bt = f mod n_theta, taken non-negative in integer arithmetic.  No trig, no
 * loops.  With bx = gx / bin_cells, by = gy / bin_cells, BW = ceil(W / bin_cells) and BH likewise, the bin's linear index is
 * (bt * BH + by) * BW + bx.
 * MODES: a bin is OCCUPIED if at least one particle of the filter lies in it.  Two distinct bins are ADJACENT if |dbx| <= 1, |dby| <= 1
 * and their bt are equal or differ by 1 modulo n_theta: 26-connectivity with the heading wrapping.  n_theta = 1 has no heading
 * neighbours; with n_theta = 2 the two layers are adjacent.  A MODE is a maximal connected set of occupied bins, its ANCHOR its bin of
 * the smallest linear index.
 *
 * Two outputs, either may be omitted (NULL):
 *   the LABEL per particle, uint32_t [n]: the anchor's linear index of the particle's mode, whatever min_count is, or GMS_MODE_NONE
 *                     for an OUTSIDE particle.
 *   the MODE TABLE    gms_mode records of the modes with count >= min_count, in ascending anchor order; the first `cap` of them are
 *                     stored, *n_found (may be NULL) is the number that qualify and may exceed cap.  cap == 0 with records == NULL is
 *                     allowed.
 * *n_outside (may be NULL) is the number of OUTSIDE particles.
 * STRONGEST: among the members whose weight is not NaN, the one of the largest weight, the first in index order among equals (a scan
 * in index order under a strict >); -1 if every member's weight is NaN.
 * THE SUMS over a mode's members, with a = the particle's weight as it stands on the handle (a pending scoring pass is combined first,
 * as gms_pf_get_weights does), X = (double)x, Y = (double)y, C and S = the filter's cached cos and sin of the particle, widened (what
 * Transform.fromRobotToWorld uses): the terms a, a * X, a * Y, a * C, a * S, a * (X * X), a * (X * Y), a * (Y * Y).  The inner products
 * of two floats are exact in double, so each term has one rounding; nothing is contracted.
 * THE ORDER is part of the definition: partial s_l, l = 0 .. 255, starts at +0.0 and adds the terms of the members i = l, l + 256,
 * l + 512, ... in ascending i; the record holds ((s_0 + s_1) + s_2) + ... + s_255.  Adding +0.0 for a non-member gives the same bits as
 * skipping it.  Non-finite weights or poses propagate as IEEE says.
 *
 * Checked before anything is enqueued (GMS_ERR_INVALID, nothing touched): the request's ranges, mi, cap >= 0, records given with
 * cap == 0 (or missing with cap > 0), more than 2^22 bins (BW * BH * n_theta), and in the _dev form misaligned device pointers.
 * GMS_ERR_STATE: the filter of a gms_slam (its particles live in their own maps), and a shard of a filter (gms_pf_set_shard with
 * n_global != n: its bins would need an exchange).  The call changes no later result of its handle: poses, weights, log-weights, trig
 * and what the handle knows of them are as gms_pf_get_weights leaves them.
 *
 * How: (1) a lane per particle computes the bin, stores it and raises the bin's count, the lanes of a wavefront that share a bin
 * combined first; OUTSIDE particles are counted; (2) a lane per bin: an occupied bin starts as its own label and is united with its 13
 * forward neighbours in the global label field, the heading wrapping, lock-free, the larger root always hung under the smaller, so the
 * final root is the anchor (the frontier regions' rule); (3) every occupied bin chases to its root; (4) the roots are numbered in
 * anchor order by a scan; count, bins and box by integer atomics, the lanes of a wavefront that share a label combined first; a second
 * scan keeps count >= min_count; (5) a lane per particle writes its label; (6) one workgroup of 256 lanes per STORED record runs the
 * sums and `strongest` in exactly the order above: lane partials in registers, then LDS, then one lane per sum adds the 256 in
 * ascending order.  Scans and unions that span workgroups are separate launches; no workgroup waits on another.  Scratch (bin counts,
 * label field, root numbering, tables) lives on the gms_pf, grows and never shrinks.
 * COST: steps 1 to 5 are one pass over the particles and a few over the bins; step 6 reads all n labels once per stored record:
 * stored records x n label reads.  min_count and cap are the caller's control over it.
 * The number of modes is known on the device only: every form, _dev included, waits on the handle's stream once (the host form once
 * more for its copies), and both outputs are complete when it returns. */
#define GMS_MODE_NONE 0xFFFFFFFFu                              /* a label: the particle is OUTSIDE */
typedef struct gms_modes {          /* the request */
    int32_t bin_cells;              /* >= 1: cells per bin along x and y */
    int32_t n_theta;                /* 1 .. 64 heading bins */
    int32_t min_count;              /* >= 1: the smallest mode the table lists */
    int32_t pad;                    /* not read */
} gms_modes;
typedef struct gms_mode {           /* 112 bytes */
    int32_t anchor_bx, anchor_by, anchor_bt;  /*  0: the bin of the smallest linear index */
    int32_t count;                            /* 12: member particles */
    int32_t bins;                             /* 16: occupied bins */
    int32_t strongest;                        /* 20: the member of the largest weight, or -1 */
    int32_t min_bx, min_by, max_bx, max_by;   /* 24: the box in bins, inclusive (no heading box: it wraps) */
    int32_t pad[2];                           /* 40: zero */
    double  w, wx, wy, wc, ws, wxx, wxy, wyy; /* 48: the weighted sums */
} gms_mode;
/* Pure host code, as gms_scatter_check: the request's ranges -- not the map's bin limit, which it does not know. */
int gms_modes_check(const gms_modes *q);
/* Map mi's filter of a shared or batched handle.  labels [n], records [cap]: host memory, staged through the views' buffer.
 * _dev: dev_labels (4-byte aligned) and dev_records (8-byte aligned) are device memory, written on the handle's stream; n_found and
 * n_outside stay HOST pointers. */
int gms_pf_modes(gms_pf *pf, int32_t mi, const gms_modes *q, uint32_t *labels, gms_mode *records, int32_t cap, int32_t *n_found, int32_t *n_outside);
int gms_pf_modes_dev(gms_pf *pf, int32_t mi, const gms_modes *q, uint32_t *dev_labels, gms_mode *dev_records, int32_t cap, int32_t *n_found,
                     int32_t *n_outside);

/* ---- beam sensor model: weigh a particle by what lies BETWEEN the sensor and the end point -------------------------------------------
 * gms_pf_score is the reference's probabilityOf, a beam-END-POINT model: the likelihood field under each end point, nothing of the way
 * there.  A pose whose beams pass through a wall scores as well as one whose beams do not.  On a scattered filter (gms_pf_scatter) that
 * keeps look-alike rooms alive; the ray-cast "beam" model every Monte-Carlo localiser offers beside it compares each measured range
 * with the range the map predicts from the particle's pose.  This library's own definition (the reference has no such method), in
 * integers down to the table look-up, and with one stated order for the product and the sum, so every output is unique.
 *
 * THE TABLE.  T = behind + ahead + 2, 0 <= behind, ahead <= 255.  The caller passes factors[2][T], host doubles: row 0 for beams with
 * hit == 0, row 1 for beams with hit != 0; every entry finite and > 0.
 * THE WALK of particle i (its pose and cached trig as they stand on the handle) and beam b: start and end point as GridMap.java:175-188,
 * rayIterator.init(start + 0.5f, end + 0.5f, ahead) -- the predicted scans' walk with `ahead` in place of gms_params.extra_steps --,
 * cut after W + H + ahead + 2 cells, ending where RayIterator.hasNext fails (it left the map, or `ahead` cells past the end point).
 * THE RESIDUAL.  The first visited cell with logData > 0 (the casts' predicate: 0, -0.0 and NaN are not occupied) gives n_rem, the
 * iterator's remaining count `n` AT that cell, before the step.  d = ahead + 1 - n_rem: for finite coordinates the walk index of that
 * cell minus the walk index of the measured end cell; d < 0: the map has a wall in front of the end point, d > 0: behind it.  The
 * table index is idx = n_rem > behind + ahead + 1 ? 0 : behind + ahead + 1 - n_rem, i.e. d + behind with d held at -behind from
 * below.  A walk that finds no occupied cell -- it left the map, ended `ahead` steps past the end point, started outside or visited no
 * cell -- gives idx = T - 1.  All of it is integer arithmetic on the iterator's own state: non-finite inputs need no rule of their own.
 * THE WEIGHTS.  f[b] = factors[hit_b != 0][idx_b], lf[b] = logtab[hit_b != 0][idx_b], logtab = log() of every entry, taken once on the
 * host (libm).  THE ORDER is part of the definition: partial l, l = 0 .. 255, starts at 1.0 (the product) and +0.0 (the sum) and takes
 * the beams l, l + 256, ... in ascending order (an empty partial keeps its start); then the halving tree
 * `for s in 128, 64, .., 1: p[l] = p[l] o p[l + s] for l < s`.  p[0] of the product is the particle's weight, p[0] of the sum its
 * log-weight.  Nothing is contracted.
 *
 * beams [n_maps][B] as for gms_pf_score, 1 <= B <= the handle's max_beams; `factors` is a HOST pointer in both forms.  residuals may
 * be NULL; if given, [n_maps][n][B], it receives idx per particle and beam (_dev: device memory, 2-byte aligned).  The host form
 * synchronises only to read the residuals back; _dev synchronises nothing.
 * Afterwards the filter is in exactly the state a gms_pf_score leaves: gms_pf_normalize, gms_pf_resample[_if],
 * gms_pf_set_log_normalize, gms_pf_get_weights / _log_weights and gms_pf_modes work on these weights unchanged.  The call sees the map
 * as gms_map_download_log would (a deferred `logData +=` pass is applied first), through the casts' bit plane (repeated calls on an
 * unchanged map do not rebuild it, gms_map_cast_plane_builds), and changes neither poses nor map.  gms_pf_set_reference_order has no
 * effect: the order above is the only one.  A shard scores its own particles (the score is local to a particle).
 * Checked before anything is enqueued (GMS_ERR_INVALID, nothing touched): behind, ahead, B, NULL pointers, every entry of factors, the
 * residuals' alignment.  GMS_ERR_STATE: the filter of a gms_slam (its particles live in their own maps).
 *
 * How: one workgroup of 256 lanes per particle, lane l walking the beams of partial l one after another through the window of the bit
 * plane its scan can reach, staged in LDS as the predicted scans do (64 KiB at most; a larger window, or GMS_CAST_WALK=mem at creation,
 * walks the plane in memory); the tree runs through LDS. */
/* Pure host code: the ranges of behind and ahead, factors not NULL, 2 * (behind + ahead + 2) entries finite and > 0. */
int gms_beam_model_check(int32_t behind, int32_t ahead, const double *factors);
int gms_pf_score_beams(gms_pf *pf, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals);
int gms_pf_score_beams_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, int32_t behind, int32_t ahead, const double *factors,
                           uint16_t *dev_residuals);

/* ---- continuous scan alignment: from "about here" to a sub-cell pose ------------------------------------------------------------------
 * Every other pose the library derives from a scan lies on a lattice: gms_map_locate answers with a cell and a heading index,
 * gms_pf_refine_poses tries 1210 poses in 4 cm / 3 degree steps.  This is a damped Gauss-Newton scan matcher on the bilinearly
 * interpolated likelihood field (the fine matcher of Hector SLAM and Cartographer, on the field the library keeps anyway): a handful of
 * iterations of 4 x B field values each.  This library's own definition (the reference has no such method).  Everything is IEEE double
 * arithmetic unless marked float, every operation rounds on its own (nothing is contracted), every sum has one stated order: the
 * result is unique.
 *
 * INPUTS.  L = likelihoodData of map mi as gms_map_download_likelihood would return it at the time of the call (a lazy rebuild of the
 * field, with the counts of a deferred `logData +=` pass, is made first); W, H; res, pos_x, pos_y = the handle's float resolution and
 * position, widened; beams [B], 1 <= B <= max_beams, of which local_x, local_y and hit are read; a pose (x, y, theta) of three floats;
 * gms_align_params.
 * ONE EVALUATION at the pose (x, y, theta): c, s = the float-rounded cos and sin of (double)theta, widened (Transform.fromRobotToWorld's
 * trig, what every other entry point uses).  Only beams with hit != 0 take part; with lx = local_x, ly = local_y, each one:
 *   X = lx*c - ly*s + x,  Y = lx*s + ly*c + y                       (left to right; x, y widened)
 *   gu = (X - pos_x)/res - 0.5,  gv = (Y - pos_y)/res - 0.5         (the field value of cell i lives at its centre i + 0.5, consistent
 *                                                                    with the truncation at GridMap.java:273-274)
 *   fu = floor(gu), fv = floor(gv), as doubles;  fx = gu - fu, fy = gv - fv
 *   the beam is USED iff fu >= 0 && fu <= W - 2 && fv >= 0 && fv <= H - 2   (NaN and +-Inf fail; only then i0 = (int)fu, j0 = (int)fv)
 *   L00 = L[j0][i0], L10 = L[j0][i0 + 1], L01 = L[j0 + 1][i0], L11 = L[j0 + 1][i0 + 1]
 *   M  = (1 - fy)*((1 - fx)*L00 + fx*L10) + fy*((1 - fx)*L01 + fx*L11)
 *   Mu = (1 - fy)*(L10 - L00) + fy*(L11 - L01),  Mv = (1 - fx)*(L01 - L00) + fx*(L11 - L10)
 *   ax = (-lx*s - ly*c)/res,  ay = (lx*c - ly*s)/res,  J = (Mu, Mv, Mu*ax + Mv*ay),  r = 1 - M
 * and ten sums over the used beams, in this order of terms: H00 = sum J0*J0, H01 = J0*J1, H02 = J0*J2, H11 = J1*J1, H12 = J1*J2,
 * H22 = J2*J2; g0 = J0*r, g1 = J1*r, g2 = J2*r; S = sum M; beside them the integer count n_used.
 * THE ORDER is part of the definition: partial l, l = 0 .. 63, starts at +0.0 and takes the used beams among b = l, l + 64, ... in
 * ascending order (a beam that is not used adds nothing); then the halving tree `for s in 32, 16, .., 1: p[l] = p[l] + p[l + s] for
 * l < s`; p[0] is the sum.
 * ONE STEP.  A00 = H00 + damp_t, A11 = H11 + damp_t, A22 = H22 + damp_r, A01 = H01, A02 = H02, A12 = H12;
 *   C00 = A11*A22 - A12*A12,  C01 = A02*A12 - A01*A22,  C02 = A01*A12 - A02*A11,
 *   C11 = A00*A22 - A02*A02,  C12 = A01*A02 - A00*A12,  C22 = A00*A11 - A01*A01,
 *   det = A00*C00 + A01*C01 + A02*C02                                                   (left to right)
 * If n_used == 0 the pose stops with status 2; otherwise if !(fabs(det) > det_min) -- a NaN lands here -- it stops with status 3.
 * Otherwise d0 = (C00*g0 + C01*g1 + C02*g2)/det, d1 = (C01*g0 + C11*g1 + C12*g2)/det, d2 = (C02*g0 + C12*g1 + C22*g2)/det (left to
 * right), d0 and d1 clamped to +-max_t (cells), d2 to +-max_r (radians) by `v > m ? m : (v < -m ? -m : v)` (a NaN passes), and the pose
 * becomes x = (float)((double)x + d0*res), y = (float)((double)y + d1*res), theta = (float)((double)theta + d2); no wrap.  If the
 * clamped |d0| <= eps_t, |d1| <= eps_t and |d2| <= eps_r the pose stops as converged, status 1.
 * THE RUN.  Evaluate; unless stopped, step; at most `iters` steps.  After the last step one more evaluation at the final pose gives the
 * reported S, n_used and H (a pose that stopped with status 2 or 3 reports the evaluation it stopped on).  So a run costs at most
 * iters + 1 evaluations, and a pose that stops in its first step comes back bit-identical to its input.
 *
 * OUTPUT per pose: the final pose, and optionally one gms_align_record: status (0 ran all iters, 1 converged, 2 no usable beam,
 * 3 singular), iters_done (the steps taken), n_used at the final and n_used0 at the start pose, score0 and score = S at the start and
 * at the final pose, H[6] = H00, H01, H02, H11, H12, H22 at the final pose WITHOUT the damping: the information matrix of the match
 * in (cells, cells, radians), up to the residuals' variance; a caller turns it into a covariance.
 *
 * gms_map_align: poses_in [P][3], 1 <= P <= GMS_MAX_PARTICLES, poses_out [P][3] (may equal poses_in), records [P] or NULL; host memory,
 * staged through the views' buffer; it waits for the stream once.  _dev: the beams, poses and outputs are device memory (poses 4-byte,
 * records and beams 8-byte aligned), read and written on the handle's stream; nothing is synchronised.
 * gms_pf_align: every particle of a shared-map filter (every map's, on a batched handle: map i's particles on map i with beams
 * [n_maps][B], as for gms_pf_score) is aligned IN PLACE; records [n_maps][n] or NULL.  Afterwards the filter is exactly as
 * gms_pf_set_poses with the new poses would leave it: the cached trig is refreshed; weights, log-weights and the resampling state are
 * untouched, so a following gms_pf_score equals a score after gms_pf_set_poses of the same poses.  A shard aligns its own particles.
 * GMS_ERR_STATE: the filter of a gms_slam (its particles live in their own maps).  The host form synchronises only to read the
 * records back; _dev synchronises nothing.
 * None of these calls changes the map.  Checked before anything is enqueued (GMS_ERR_INVALID, the outputs untouched): NULL pointers,
 * mi, B, P, the parameters (gms_align_check), and in the _dev forms the alignment above.
 *
 * How: one wavefront per pose, four poses per workgroup of 256 lanes; lane l owns partial l; the beams' (lx, ly) -- NaN for a beam that
 * did not hit, which the USED test then refuses -- are staged once per workgroup in LDS, 16 bytes per beam; the tree runs as cross-lane
 * register moves; the loop over the iterations is uniform per wavefront, a stopped pose idles to the end of its workgroup. */
typedef struct gms_align_params {   /* 64 bytes */
    int32_t iters;                  /* 1 .. 64 steps at most */
    int32_t pad;                    /* not read */
    double  damp_t, damp_r;         /* finite, >= 0: added to H00 and H11 / to H22 (Levenberg's damping) */
    double  max_t, max_r;           /* > 0, +Inf allowed: the largest step along x and y in cells / of theta in radians */
    double  eps_t, eps_r;           /* finite, >= 0: a step no larger than these stops the pose as converged */
    double  det_min;                /* finite, >= 0: a determinant no larger in magnitude stops the pose as singular */
} gms_align_params;
typedef struct gms_align_record {   /* 80 bytes */
    int32_t status;                 /*  0: 0 ran all iters, 1 converged, 2 no usable beam, 3 singular */
    int32_t iters_done;             /*  4 */
    int32_t n_used;                 /*  8: used beams at the final pose */
    int32_t n_used0;                /* 12: ... at the start pose */
    double  score0, score;          /* 16: S at the start and at the final pose */
    double  H[6];                   /* 32: H00, H01, H02, H11, H12, H22 at the final pose */
} gms_align_record;
/* Pure host code.  The defaults: iters 8, damp_t 10, damp_r 1e4, max_t 2 cells, max_r 0.1 rad, eps_t 0.01 cells, eps_r 1e-4 rad,
 * det_min 1e-6 (DESIGN.md section 4n says why); the check: the ranges above, non-finite values refused (max_t, max_r may be +Inf). */
int gms_align_params_default(gms_align_params *p);
int gms_align_check(const gms_align_params *p);
int gms_map_align(gms_map *m, int32_t mi, const gms_beam *beams, int32_t B, const float *poses_in, int32_t P, const gms_align_params *params,
                  float *poses_out, gms_align_record *records);
int gms_map_align_dev(gms_map *m, int32_t mi, const gms_beam *dev_beams, int32_t B, const float *dev_poses_in, int32_t P,
                      const gms_align_params *params, float *dev_poses_out, gms_align_record *dev_records);
int gms_pf_align(gms_pf *pf, const gms_beam *beams, int32_t B, const gms_align_params *params, gms_align_record *records);
int gms_pf_align_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, const gms_align_params *params, gms_align_record *dev_records);

/* ---- per-particle scan alignment: every particle of a gms_slam against its own map ------------------------------------------------------
 * The reference's SLAM.update calls findBestPoseOptim(p.m, z, p.pose) for every particle against that particle's own field
 * (SLAM.java:96-97) between computeLikelihoodMap (:93) and the weighting (:99); its BOBYQA objective is 0 / NaN, so it moves nothing.
 * This is the build's stand-in at that place: the continuous scan alignment above, per particle (GMapping's per-particle scan matching).
 *
 * gms_slam_align: every particle i the handle holds is aligned IN PLACE.  The definition is exactly "continuous scan alignment" with
 * L = the field computeLikelihoodMap(p_i.m) would write from particle i's logData as it stands -- the field the next update scores
 * against --, W, H, res, pos the handle's, the start pose the particle's; 1 <= B <= max_beams; records [n] or NULL.  The call changes
 * no map and no weight, and what gms_slam_download_map returns for likelihoodData is what it returned before.  Afterwards the filter is
 * as gms_pf_set_poses with the new poses would leave it: the cached trig is refreshed.  A shard aligns its own block.  A batched handle
 * (n_maps > 1): GMS_ERR_STATE, nothing touched -- use gms_slam_set_align there.  The host form waits for the stream only to read the
 * records back.  _dev: dev_beams and dev_records are device memory, 8-byte aligned; runs on the handle's stream, synchronises nothing.
 * Checked before anything is enqueued (GMS_ERR_INVALID, the outputs untouched): NULL handle or beams, the parameters
 * (gms_align_check), B, and in the _dev form the alignment.
 *
 * gms_slam_set_align: non-NULL parameters are checked and copied; from then on every update of the handle -- gms_slam_update_per_particle
 * [_dev], gms_slam_update_batch[_dev], gms_slam_update_local[_dev], both frame calls -- aligns each particle between
 * computeLikelihoodMap and the weighting: the particle is weighted, its map updated and its history row written at the aligned pose.
 * Where the update draws the motion-model sample the alignment starts from it; with gms_slam_set_refine on as well the order is the
 * lattice search, then the alignment from the lattice's best pose (coarse to fine).  skipUpdate (|dTheta| > 30 degrees) skips only the
 * map update, as without it.  B == 0: every pose stays as it is (status 2).  NULL: off, the default; an update then issues exactly
 * the launches it issued before.
 * gms_slam_last_align: the records [n_maps * n] of the last aligned update (so a caller counts statuses without a second pass);
 * GMS_ERR_STATE before there is one (and after gms_slam_reset).  Synchronises.
 *
 * How: one workgroup per particle.  Where the handle keeps the particles' class planes (2 bits per cell) and a plane fits a workgroup's
 * LDS beside the scan, the plane is staged there and the four values per beam are computed on demand per evaluation -- the horizontal
 * sums of the rows j0 - k .. j0 + 1 + k at the columns i0 and i0 + 1, then the vertical sums: computeLikelihoodMap's operations in its
 * order for those cells -- and one wavefront forms the sums, the tree, the solve and the step (GMS_SLAM_ALIGN_PLANES).  Otherwise the
 * field is written to memory first and read there (GMS_SLAM_ALIGN_MEMORY).  Both give the same bits; the environment variable
 * GMS_SLAM_ALIGN_FIELD=memory|planes, read at creation, forces a form where it exists.  gms_slam_align_form (diagnostics): the form the
 * handle's last alignment launch took, 0 before the first. */
#define GMS_SLAM_ALIGN_PLANES 1
#define GMS_SLAM_ALIGN_MEMORY 2
int gms_slam_align(gms_slam *s, const gms_beam *beams, int32_t B, const gms_align_params *params, gms_align_record *records);
int gms_slam_align_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, const gms_align_params *params, gms_align_record *dev_records);
int gms_slam_set_align(gms_slam *s, const gms_align_params *params);
int gms_slam_last_align(gms_slam *s, gms_align_record *records);
int gms_slam_align_form(const gms_slam *s, int32_t *form);

/* ---- per-particle beam sensor model: every particle of a gms_slam against its own map ----------------------------------------------------
 * gms_slam's update weighs a particle by probabilityOf, the end-point model, on the field of the particle's own map.  In a
 * Rao-Blackwellised filter that is where the beam model matters most: a particle that has drifted sees its old walls in front of, or
 * behind, the measured end points, and the blurred field still gives a decent value next to a doubled wall, so a stale map survives
 * resampling as easily as a consistent one.
 *
 * The definition is "beam sensor model" above, word for word -- THE TABLE, THE WALK, THE RESIDUAL, THE WEIGHTS, THE ORDER (256 strided
 * partials, then the halving tree), gms_beam_model_check -- with ONE change: particle i's walk runs through particle i's own logData,
 * as gms_slam_download_map(i) would return it at that moment.  The predicate is the same, logData > 0: 0, -0.0 and NaN are not
 * occupied.  (The particles' class planes are thresholded for the likelihood field; they are not this predicate and are not used.)
 *
 * gms_slam_score_beams[_dev]: every particle the handle holds gets the weight and the log-weight the definition gives for its pose,
 * pose and cached trig taken as they stand.  1 <= B <= max_beams; residuals [n][B] or NULL.  The call changes no pose, no map and no
 * likelihoodData.  It leaves the filter with RAW weights, the state gms_slam_update_local_dev leaves: gms_pf_get_weights and
 * gms_pf_get_log_weights read them, gms_pf_normalize on the filter of gms_slam_handles finishes as an update does, and
 * gms_slam_resample_maps[_if] work unchanged after that.  A shard scores its own block.  A batched handle (n_maps > 1): GMS_ERR_STATE,
 * nothing touched -- use gms_slam_set_beam_model there.  Checked before anything is enqueued (GMS_ERR_INVALID, the outputs untouched):
 * NULL handle or beams, gms_beam_model_check, B, and in the _dev form the residuals' 2-byte alignment.  `factors` is a HOST pointer in
 * both forms.  The host form synchronises only to read the residuals back; _dev synchronises nothing.
 *
 * gms_slam_set_beam_model: the arguments are checked (gms_beam_model_check; combine one of the two below) and the table is copied
 * with its logarithms.  From then on every update of the handle -- gms_slam_update_per_particle[_dev], gms_slam_update_batch[_dev],
 * gms_slam_update_local[_dev], both frame calls -- applies the model: each particle is weighted through its own map as it stands BEFORE
 * this scan is integrated (behind it every particle would find its own end cell occupied), at the pose it is weighted at -- the pose
 * after the motion sample, the lattice refinement and the alignment, in that order, where each is on.  The raw weight and the raw
 * log-weight the update writes are then combined: MULTIPLY -- weight = probabilityOf(...) * beam weight, one double multiply, not
 * contracted, log-weight = the sum of the two; REPLACE -- both are the beam model's own.  skipUpdate (|dTheta| > 30 degrees) skips
 * only the map update, as without the model.  B == 0 (a batched handle: a filter whose count is 0) leaves the raw weight as the update
 * gives it.  On a batched handle each filter is scored with its own scan and count.  factors NULL: off, the default; an update then
 * issues exactly the launches it issued before.  gms_slam_reset keeps the setting, as it keeps gms_slam_set_align's.
 *
 * How: one workgroup of 256 lanes per particle.  No packed plane of a particle's map exists in memory and none is written: the
 * workgroup forms the box of its rays, pads it by ahead + 1, and packs that window of `logData > 0` straight from the particle's
 * logData into LDS -- a wavefront reads 64 consecutive cells of a row and its ballot is two words of the window (64 KiB at most).  A
 * larger window, or GMS_CAST_WALK=mem at creation, reads logData[y W + x] > 0 from memory at every step; all forms give the same bits.
 * Inside an update a second kernel, one lane per particle, combines the weights behind the update's own and in front of the
 * normalisation. */
#define GMS_SLAM_BEAMS_MULTIPLY 0   /* raw weight = probabilityOf(...) * beam weight (one double multiply, not contracted) */
#define GMS_SLAM_BEAMS_REPLACE  1   /* raw weight = beam weight */
int gms_slam_score_beams(gms_slam *s, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals);
int gms_slam_score_beams_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t behind, int32_t ahead, const double *factors,
                             uint16_t *dev_residuals);
int gms_slam_set_beam_model(gms_slam *s, int32_t behind, int32_t ahead, const double *factors, int32_t combine);  /* factors NULL: off (default) */

/* ---- trajectory rollouts: which velocity command can be sent without hitting something ---------------------------------------------
 * The inner loop of a local planner (dynamic window, lattice primitives): K candidate arcs, each sampled at T steps, the robot's
 * footprint tested against the inflated obstacle plane at every step, and the clearance and cost-to-go fields read along the way.  This
 * library's own definition (the reference has no such method); every result is an integer and unique.
 *
 * THE ARC TABLE  arcs [K][T] of gms_rollout_step {dx, dy, c, s} (four floats, 16 bytes): the robot's pose at step t of candidate k in
 *                the frame of the START pose -- a translation in metres and the cosine and sine of the heading change.  The table is the
 *                caller's, made on the host (gms_rollout_arcs makes unicycle arcs), like gms_map_locate's offsets and
 *                gms_pf_score_beams' factors: the device takes no trig per step.  1 <= K <= GMS_ROLLOUT_MAX_K, 1 <= T <= GMS_ROLLOUT_MAX_T.
 * THE FOOTPRINT  points [F][2] floats (fx, fy) in the robot frame, metres, 0 <= F <= GMS_ROLLOUT_MAX_F (F == 0: points may be NULL).  The
 *                robot's centre (0, 0) is always tested as well, LAST, and has point index F.
 * STEP ARITHMETIC  for a step {dx, dy, c, s} and a point (fx, fy), all widened to double, every product and sum rounded on its own
 *                (nothing is contracted):  qx = dx + (c*fx - s*fy),  qy = dy + (s*fx + c*fy);  the world point is Transform.transformX /
 *                transformY of (qx, qy) under the start pose (x, y, theta) with Transform.fromRobotToWorld's float-rounded trig, what
 *                every other entry point uses:  wx = qx*C - qy*S + x,  wy = qx*S + qy*C + y  (left to right);  the cell is
 *                gms_map_clearance_poses':  (int)((wx - position.x) / resolution), likewise y, with Java's cast (toward zero, NaN -> 0,
 *                saturating).  The IDENTITY step is {0, 0, 1, 0}; the START CELL is the centre's cell under it.
 * COLLISION      a point collides at a step if its cell is, tested in this order,
 *                  GMS_ROLLOUT_HIT_OUTSIDE   off the map;
 *                  GMS_ROLLOUT_HIT_RANGE     farther than max_range cells, Chebyshev, from the start cell (1 <= max_range <= 255: the view
 *                                            gain's cut);
 *                  GMS_ROLLOUT_HIT_BLOCKED   BLOCKED as the cost-to-go fields define it for `mode` and `inflate`.
 * THE RECORD     per (start pose p, candidate k) one gms_rollout_rec, out [P][K]:
 *                  first_hit   the smallest step at which any point collides; T if none.
 *                  hit_point   the smallest colliding point index at that step; 0xFFFF if none.
 *                  flags       the kind of that first hit (of point hit_point at step first_hit; 0 if none), and GMS_ROLLOUT_START_BLOCKED
 *                              if any point collides under the identity step -- at the start pose itself; this is independent of
 *                              first_hit.
 *                  min_d2      the minimum of clear [H][W] -- a WHOLE-MAP clearance field, what gms_map_clearance returns for the full
 *                              rectangle; may be NULL -- under the centre's cell over the steps < first_hit (the centre does not collide
 *                              there, so its cell is on the map); GMS_CLEAR_FAR without a field or without such a step.
 *                  best_step, best_cost   the smallest step < first_hit at which cost [H][W] -- a WHOLE-MAP cost-to-go field, the one
 *                              gms_map_frontiers accepts; may be NULL -- is least under the centre's cell, and that cost (GMS_REACH_FAR
 *                              if every such cell holds it: best_step is then the smallest such step, 0); 0xFFFF and GMS_REACH_FAR
 *                              without a field or without such a step.
 *                  end_cost    cost under the centre's cell at step first_hit - 1, the last collision-free one; GMS_REACH_FAR without a
 *                              field or when first_hit == 0.
 *                  last_x, last_y   the centre's cell at step first_hit - 1; the start cell when first_hit == 0.
 *                  start_x, start_y the start cell.
 * A non-finite pose, step or point is no error: the arithmetic above says which cell it lands in (a NaN coordinate: cell 0).
 *
 * "Sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment" (a deferred `logData +=` pass is applied
 * first, an owed resampling copy is looked through), "changes no later result of its handle" and the argument checks before anything is
 * enqueued (GMS_ERR_INVALID, nothing touched) are the casts' rules.
 *
 * How: the blocked plane is the cost-to-go fields' -- with inflate = 0 the map's plane of `mode` read in place and packed only when stale
 * (gms_map_cast_plane_builds does not move for a current plane), with inflate > 0 their scratch plane.  One workgroup of 256 lanes per
 * (start pose, block of GMS_ROLLOUT_CANDIDATES candidates) stages the square of side 2 * max_range + 1 around the start cell in LDS, one
 * bit per cell, off-map cells set (at most 16 words x 511 rows, 33 KB), and the footprint beside it: outside, range and blocked are then
 * one bounds test and one bit test.  One wavefront takes one candidate at a time: lanes own steps, 64 per pass, each lane loops over the
 * F + 1 points, a ballot gives the first colliding step and ends the candidate's passes, and the minima in front of it are cross-lane
 * reductions.  On a handle created with GMS_ROLLOUT_WALK=mem in the environment (tests) every look-up reads the plane in memory -- the
 * same records either way. */
#define GMS_ROLLOUT_MAX_K 4096
#define GMS_ROLLOUT_MAX_T 256
#define GMS_ROLLOUT_MAX_F 64
#define GMS_ROLLOUT_CANDIDATES 16                             /* candidates a workgroup takes (the probe that chose it) */
#define GMS_ROLLOUT_HIT_OUTSIDE 1u                            /* gms_rollout_rec.flags */
#define GMS_ROLLOUT_HIT_RANGE 2u
#define GMS_ROLLOUT_HIT_BLOCKED 4u
#define GMS_ROLLOUT_START_BLOCKED 8u
typedef struct gms_rollout_step {   /* 16 bytes */
    float dx, dy;                   /* the translation, metres, in the start pose's frame */
    float c, s;                     /* cosine and sine of the heading change */
} gms_rollout_step;
typedef struct gms_rollout {        /* 16 bytes */
    int32_t max_range;              /* cells, 1 .. 255 */
    int32_t inflate;                /* cells, 0 .. 255 */
    int32_t mode;                   /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t filter;                 /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_rollout;
typedef struct gms_rollout_rec {    /* 32 bytes */
    uint16_t first_hit;             /*  0 */
    uint16_t hit_point;             /*  2 */
    uint16_t min_d2;                /*  4 */
    uint16_t best_step;             /*  6 */
    uint16_t best_cost;             /*  8 */
    uint16_t end_cost;              /* 10 */
    uint16_t flags;                 /* 12 */
    uint16_t pad;                   /* 14: always 0 */
    int32_t last_x, last_y;         /* 16, 20 */
    int32_t start_x, start_y;       /* 24, 28 */
} gms_rollout_rec;
typedef struct gms_rollout_risk {   /* 32 bytes: one candidate over a filter's particles */
    uint32_t n_hit;                 /*  0: particles with first_hit < T */
    uint32_t n_start_blocked;       /*  4: particles whose footprint collides at their own pose */
    uint32_t min_first_hit;         /*  8: the smallest first_hit (T if no particle hits) */
    uint32_t pad;                   /* 12: always 0 */
    uint64_t sum_first_hit;         /* 16: the sum of first_hit over the particles; the mean is sum / n, the caller's division */
    uint64_t pad2;                  /* 24: always 0 */
} gms_rollout_risk;
/* Pure host code: the ranges of K, T and F above and of max_range, inflate and mode. */
int gms_rollout_check(const gms_rollout *r, int32_t K, int32_t T, int32_t F);
/* Pure host code: the table of K unicycle arcs, out [K][T].  Step j of candidate k is the pose after time t = (j + 1) * dt (dt finite,
 * > 0) at speed v[k] (m/s) and turn rate omega[k] (rad/s), libm in double, each value rounded to float:  th = omega * t;  c = cos(th),
 * s = sin(th);  with r = v / omega:  dx = r * sin(th),  dy = r * (1 - cos(th));  where |omega| < 1e-9 the straight line dx = v * t,
 * dy = 0.  In C so that every host language gets the same table. */
int gms_rollout_arcs(const double *v, const double *omega, int32_t K, double dt, int32_t T, gms_rollout_step *out);
/* GMS_ROLLOUT_CANDIDATES of the library as built. */
int gms_rollout_candidates_per_workgroup(void);
/* Map mi of a shared or batched map: P start poses (poses [P][3] = x, y, theta; 1 <= P <= GMS_MAX_PARTICLES), the same arcs and
 * footprint for each; clear and cost may each be NULL; out [P][K].  The host form stages its inputs (the fields too) through the views'
 * buffer, reads the records back and synchronises; _dev takes device pointers (arcs and out 16-byte aligned, poses and points 4-byte,
 * the fields 2-byte), runs on the handle's stream and synchronises nothing. */
int gms_map_rollout(gms_map *m, int32_t mi, const gms_rollout *r, const float *poses, int32_t P, const gms_rollout_step *arcs, int32_t K, int32_t T,
                    const float *points, int32_t F, const uint16_t *clear, const uint16_t *cost, gms_rollout_rec *out);
int gms_map_rollout_dev(gms_map *m, int32_t mi, const gms_rollout *r, const float *dev_poses, int32_t P, const gms_rollout_step *dev_arcs, int32_t K, int32_t T,
                        const float *dev_points, int32_t F, const uint16_t *dev_clear, const uint16_t *dev_cost, gms_rollout_rec *dev_out);
/* The per-particle filter: the rollouts in the map of the shown particle.  `which`, GMS_VIEW_STRONGEST, r->filter, *shown (may be
 * NULL; _dev: a device int32_t *) and the GMS_ERR_STATE cases are gms_slam_view's; particle and generation are picked on the device.
 * Here only, P == 0 with poses NULL means: ONE start pose, the SHOWN particle's own, read on the device (gms_slam_reach's seed idiom);
 * out is then [1][K]. */
int gms_slam_rollout(gms_slam *s, int32_t which, const gms_rollout *r, const float *poses, int32_t P, const gms_rollout_step *arcs, int32_t K, int32_t T,
                     const float *points, int32_t F, const uint16_t *clear, const uint16_t *cost, gms_rollout_rec *out, int32_t *shown);
int gms_slam_rollout_dev(gms_slam *s, int32_t which, const gms_rollout *r, const float *dev_poses, int32_t P, const gms_rollout_step *dev_arcs, int32_t K, int32_t T,
                         const float *dev_points, int32_t F, const uint16_t *dev_clear, const uint16_t *dev_cost, gms_rollout_rec *dev_out, int32_t *dev_shown);
/* A shared-map filter: EVERY particle is a start pose, read from the filter's device poses, and the output is one gms_rollout_risk per
 * candidate, out [K] (a batched handle: map i's particles in map i, out [n_maps][K]) -- n * K records would be hundreds of megabytes.
 * The same kernel counts with integer atomics, so the result is unique whatever the scheduling.  After a resample the weights are equal
 * and n_hit / n is the collision probability of the command; a weighted form is not offered.  A shard counts its own particles.
 * GMS_ERR_STATE: the filter of a gms_slam (its particles live in their own maps).  r->filter is not read.  The filter is not changed. */
int gms_pf_rollout(gms_pf *pf, const gms_rollout *r, const gms_rollout_step *arcs, int32_t K, int32_t T, const float *points, int32_t F, gms_rollout_risk *out);
int gms_pf_rollout_dev(gms_pf *pf, const gms_rollout *r, const gms_rollout_step *dev_arcs, int32_t K, int32_t T, const float *dev_points, int32_t F,
                       gms_rollout_risk *dev_out);

/* ---- routes: which way to drive, as a handful of straight legs ---------------------------------------------------------------------
 * The link between a cost-to-go field and the rollouts: for P start cells over a whole-map cost-to-go field, the cheapest 8-connected
 * path down to a seed, and that path pulled taut to waypoints by line of sight through the blocked plane.  This library's own
 * definition (the reference has no such method); all of it is integer arithmetic and every output is unique.
 *
 * INPUTS         cost [H][W]: a WHOLE-MAP cost-to-go field, what gms_map_reach returns for the full rectangle; required.
 *                clear [H][W]: a WHOLE-MAP clearance field, what gms_map_clearance returns for the full rectangle; may be NULL.
 *                starts [P][2]: int32_t (x, y) cells, 1 <= P <= GMS_ROUTE_MAX_P.
 *                gms_route {max_cells, max_waypoints, look, inflate, mode, filter}: 1 <= max_cells <= GMS_ROUTE_MAX_CELLS (a descent
 *                never has more than 0xFFFE / GMS_REACH_AXIS + 1 = 13107 cells), 1 <= max_waypoints <= max_cells, 1 <= look <=
 *                GMS_ROUTE_MAX_LOOK, inflate and mode as in gms_reach, filter as in the other requests.
 * BLOCKED        exactly the cost-to-go fields' predicate for `mode` and `inflate`.
 * THE DESCENT    With FAR = GMS_REACH_FAR: a start off the map, or with cost == FAR, has no path: n_cells = 0, n_waypoints = 0 and the
 *                flag GMS_ROUTE_NO_PATH.  Otherwise path[0] is the start cell, and while the current cell's cost is not 0 the next
 *                cell is the FIRST neighbour n in the order E, N, W, S, NE, NW, SW, SE (north = y + 1) for which all of these hold:
 *                n is on the map;  cost[n] != FAR;  cost[n] + step == cost[current], step GMS_REACH_AXIS along an axis and
 *                GMS_REACH_DIAG diagonally, formed in 32 bits;  for a diagonal, both cells it squeezes between -- (n.x, current.y)
 *                and (current.x, n.y) -- are on the map and not FAR.  If no neighbour qualifies the descent stops there with
 *                GMS_ROUTE_BROKEN: the field is no cost-to-go field; this is no error of the call.  If a next cell exists but the
 *                path already holds max_cells cells, it stays at those with GMS_ROUTE_CELLS_CUT.  The cost falls by at least 5 per
 *                step, so the descent ends whatever the field holds; nothing but the meaning of the result depends on the field
 *                being consistent with the map.
 * VISIBLE(a, b)  for cells a, b on the map with dx = b.x - a.x, dy = b.y - a.y: every cell (x, y) of the bounding box of a and b with
 *                    2 * |(x - a.x) * dy - (y - a.y) * dx| <= |dx| + |dy|
 *                is not BLOCKED.  This is the closed supercover of the segment between the two cell centres: a cell the segment only
 *                touches at a corner counts, a and b themselves count.  So a line of sight never passes between two diagonally
 *                adjacent blocked cells, and it agrees with the cost-to-go fields' "no corner cutting": a legal diagonal step is
 *                VISIBLE, an illegal one is not.  Two cells of one path that are k <= look indices apart differ by at most k <=
 *                4096 = 2^12 per axis, so both products are at most 2^24 and twice their difference at most 2^26: 32 bits hold them.
 * PULLING        w[0] = path[0], i = 0.  While i < n_cells - 1:  if max_waypoints waypoints are written already, stop with
 *                GMS_ROUTE_WAYPOINTS_CUT (in front of the search);  j = the LARGEST index in (i, min(i + look, n_cells - 1)] with
 *                VISIBLE(path[i], path[j]);  if there is none, j = i + 1 and GMS_ROUTE_MISMATCH is set -- the field was made for
 *                another mode or inflate, or for another map;  append path[j];  i = j.  Without a cut the last waypoint is the
 *                path's last cell.  look = 1 returns the path itself.
 * THE RECORD     per start one gms_route_rec, out [P]:
 *                  n_cells, n_waypoints   the cells of the descended path and the waypoints written.
 *                  start_cost  cost under the start cell; FAR for a start off the map.
 *                  end_cost    cost under the path's last cell: 0 when a seed was reached; FAR with NO_PATH.
 *                  min_d2, min_d2_at   the minimum of clear over the path's cells and the smallest path index where it is taken;
 *                              GMS_CLEAR_FAR and 0 without a field or without a path.
 *                  flags       the GMS_ROUTE_* flags above.
 *                  end_x, end_y   the path's last cell; the start cell with NO_PATH.
 * OUTPUTS        out [P];  waypoints [P][max_waypoints][2] int32_t (x, y);  cells [P][max_cells][2] int32_t, may be NULL.  Entries
 *                behind n_waypoints and n_cells are not written: they keep what the caller's buffer held.
 *
 * "Sees the map as gms_map_download_log / gms_slam_download_map would return it at that moment", "changes no later result of its
 * handle" and the argument checks before anything is enqueued (GMS_ERR_INVALID, nothing touched) are the casts' rules.
 *
 * How: the blocked plane is the cost-to-go fields' (gms_map_cast_plane_builds does not move for a current plane).  One wavefront per
 * start.  The descent is a chain of dependent loads, one round trip per step: nine lanes load the 3 x 3 block around the current cell
 * -- lane k < 8 the k-th neighbour in the order above, lane 8 the cell itself, off the map reads as FAR --, the side cells of a diagonal
 * come from the axis lanes by cross-lane moves, and a ballot's lowest bit is the next cell; the cells are kept one per lane and
 * stored 64 at a time.  The path lives in `cells`, or without it in a scratch buffer of the handle that only grows (P * max_cells * 8
 * bytes).  The clearance minimum is one pass over the path, 64 cells at a time.  The pull gives every lane one candidate j, 64 per
 * pass from the far end of the window down; a lane walks its supercover along the major axis from path[i] (at most three cells per
 * column, no division) and leaves at its first blocked cell; a ballot's lowest bit is the largest visible j and ends the passes. */
#define GMS_ROUTE_MAX_P 65536
#define GMS_ROUTE_MAX_CELLS 16384
#define GMS_ROUTE_MAX_LOOK 4096
#define GMS_ROUTE_NO_PATH 1u                                   /* gms_route_rec.flags */
#define GMS_ROUTE_BROKEN 2u
#define GMS_ROUTE_CELLS_CUT 4u
#define GMS_ROUTE_WAYPOINTS_CUT 8u
#define GMS_ROUTE_MISMATCH 16u
typedef struct gms_route {          /* 24 bytes */
    int32_t max_cells;              /* 1 .. GMS_ROUTE_MAX_CELLS */
    int32_t max_waypoints;          /* 1 .. max_cells */
    int32_t look;                   /* path indices a line of sight may skip, 1 .. GMS_ROUTE_MAX_LOOK */
    int32_t inflate;                /* cells, 0 .. 255 */
    int32_t mode;                   /* GMS_CLEAR_OCCUPIED / GMS_CLEAR_NOT_FREE */
    int32_t filter;                 /* batched gms_slam handles with GMS_VIEW_STRONGEST: whose strongest particle (ignored elsewhere) */
} gms_route;
typedef struct gms_route_rec {      /* 32 bytes */
    uint32_t n_cells;               /*  0 */
    uint32_t n_waypoints;           /*  4 */
    uint16_t start_cost;            /*  8 */
    uint16_t end_cost;              /* 10 */
    uint16_t min_d2;                /* 12 */
    uint16_t flags;                 /* 14 */
    uint32_t min_d2_at;             /* 16 */
    int32_t end_x, end_y;           /* 20, 24 */
    uint32_t pad;                   /* 28: always 0 */
} gms_route_rec;
/* Pure host code: the ranges of max_cells, max_waypoints, look, inflate and mode above. */
int gms_route_check(const gms_route *r);
/* Map mi of a shared or batched map.  The host form stages its inputs (both fields too) and the caller's waypoints and cells
 * through the views' buffer -- so what lies behind the counts comes back as it went --, reads everything back and synchronises
 * once; _dev takes device pointers (out 16-byte aligned, waypoints and cells 8-byte, starts 4-byte, the fields 2-byte), runs on the
 * handle's stream and synchronises nothing (but where the path scratch has to grow: then it waits for that stream first). */
int gms_map_route(gms_map *m, int32_t mi, const gms_route *r, const int32_t *starts, int32_t P, const uint16_t *cost, const uint16_t *clear,
                  gms_route_rec *out, int32_t *waypoints, int32_t *cells);
int gms_map_route_dev(gms_map *m, int32_t mi, const gms_route *r, const int32_t *dev_starts, int32_t P, const uint16_t *dev_cost, const uint16_t *dev_clear,
                      gms_route_rec *dev_out, int32_t *dev_waypoints, int32_t *dev_cells);
/* The per-particle filter: the routes through the map of the shown particle, over that particle's field.  `which`,
 * GMS_VIEW_STRONGEST, r->filter, *shown (may be NULL; _dev: a device int32_t *) and the GMS_ERR_STATE cases are gms_slam_rollout's.
 * Here only, P == 0 with starts NULL means: ONE start, the SHOWN particle's own pose cell, read on the device (gms_slam_reach's seed
 * idiom); out is then [1]. */
int gms_slam_route(gms_slam *s, int32_t which, const gms_route *r, const int32_t *starts, int32_t P, const uint16_t *cost, const uint16_t *clear,
                   gms_route_rec *out, int32_t *waypoints, int32_t *cells, int32_t *shown);
int gms_slam_route_dev(gms_slam *s, int32_t which, const gms_route *r, const int32_t *dev_starts, int32_t P, const uint16_t *dev_cost, const uint16_t *dev_clear,
                       gms_route_rec *dev_out, int32_t *dev_waypoints, int32_t *dev_cells, int32_t *dev_shown);

/* ---- map warps: one map read through a rigid transform, compared with another or merged into it -------------------------------------
 * Every map is fixed to the frame gms_params gave it; gms_map_copy and gms_map_combine need equal grids.  A warp reads the logData of a
 * SOURCE map through a pose and compares it with, copies it into, adds it to or fills it into a rectangle of a DESTINATION map of any
 * other size, corner and resolution: growing or re-centring a map, comparing two robots' or two sessions' maps, fusing them, and
 * taking a particle's map out of a gms_slam.  This library's own definition (the reference has no such method); every count is an
 * integer and every stored value is unique.
 *
 * THE POSE       gms_warp {tx, ty, c, s}: the pose of the SOURCE map's world frame in the DESTINATION's world,  p_dst = R p_src + t,
 *                R = [[c, -s], [s, c]].  Cosine and sine are stored, not an angle: the device takes no trig, exact quarter turns can be
 *                asked for (c = 0, s = 1), and a host that restates the arithmetic reads the doubles the kernel used.  gms_warp_pose
 *                fills them from (x, y, theta) with the host's libm.  The pose gms_map_locate -> gms_map_align return for the source
 *                map's occupied cells, handed over as beams, in the destination map IS this pose.
 * THE ARITHMETIC all in double; both maps' float position.x, position.y and resolution are widened to double; every product, sum and
 *                quotient is rounded on its own (nothing is contracted).  For cell (x, y) of the destination rectangle
 *                    cx = pos_x_d + (x + 0.5) * res_d,   cy likewise                          the cell's centre
 *                    dx = cx - tx,   dy = cy - ty
 *                    u  = c * dx + s * dy,   v = c * dy - s * dx                              ... in the source's world
 *                    qx = floor((u - pos_x_s) / res_s),   qy = floor((v - pos_y_s) / res_s)
 *                The cell HAS A SOURCE CELL (qx, qy) if and only if 0 <= qx < W_s and 0 <= qy < H_s, compared as doubles before any
 *                conversion to an integer (NaN fails); every other cell of the rectangle counts in n_outside and is left alone.
 *                Nearest cell only: sampling the centre leaves half a cell between the arithmetic and a cell edge whenever the
 *                transform is a whole-cell shift or a quarter turn.  Interpolation and coarsening rules are not offered.
 * THE CLASSES    occupied l > 0 (class 2), free l < 0 (class 1), unknown everything else -- 0, -0.0, NaN -- (class 0): the predicates
 *                of the planes and the casts.
 * THE OPS        with d the destination cell's value and v its source cell's, both as a download would return them at this moment:
 *                  GMS_WARP_COMPARE   writes nothing.
 *                  GMS_WARP_REPLACE   d := v bit for bit, NaN and -0.0 included.
 *                  GMS_WARP_ADD       only where v is known (class 1 or 2):  r = d + v;  with clamp > 0:  if (r > clamp) r = clamp;
 *                                     if (r < -clamp) r = -clamp;  d := r.  A NaN in d stays as it is, bit for bit; an unknown source
 *                                     cell never poisons or changes the destination.
 *                  GMS_WARP_FILL      d := v bit for bit only where d is unknown and v is known.
 * THE STATISTICS gms_warp_stats (may be NULL), filled for every op from the destination's values BEFORE the call:  pair[a][b] counts
 *                the cells with a source cell whose destination class is a and whose source class is b;  n_outside the cells without
 *                one.  The ten counters sum to w * h.  Both known: the overlap; pair[1][1] + pair[2][2] agree, pair[1][2] + pair[2][1]
 *                conflict -- the evidence to accept or reject a candidate pose by BEFORE merging under it.
 *
 * Refused with GMS_ERR_INVALID and nothing touched: a NULL handle or request; a map index out of range; x0, y0 < 0, w, h < 1 or a
 * rectangle that leaves the destination (the views' rule); an unknown op; a non-finite tx, ty, c, s or clamp; clamp < 0;
 * |c*c + s*s - 1| > 1e-6 (a sanity bound on the input, no tolerance of the arithmetic); handles on different devices; the same map as
 * source and destination (two maps of one batched handle are allowed); for gms_slam_warp the gms_slam's own map handle as destination.
 *
 * State: a destination written by REPLACE, ADD or FILL is left exactly as gms_map_upload_log of the resulting array would leave it -- a
 * deferred `logData +=` pass is applied first (ADD adds to the applied values), likelihoodData stays until the next build, the bit
 * planes, the factor table, the seeding table and the tiles' states are invalidated.  COMPARE changes no later result of either handle.
 * The source is read as a download would return it, its own deferred pass included.  Cells outside the rectangle and the other maps of
 * a batched handle are not touched.  The kernel runs on the DESTINATION's stream; where the source's handle runs on another one the two
 * are ordered in both directions by events, as gms_map_combine orders them, and the host waits for nothing.
 *
 * How: one kernel per op.  A workgroup of 256 lanes takes a tile of 64 x 64 cells of the rectangle, a wavefront a row of 64 destination
 * cells at a time -- one coalesced 512-byte load and store -- and gathers the source cells directly.  The counts are nine ballots per
 * row and one for the outside, summed in registers over the tile's rows, combined through LDS, and added with one 64-bit integer atomic
 * per non-zero counter and workgroup. */
enum { GMS_WARP_COMPARE = 0, GMS_WARP_REPLACE = 1, GMS_WARP_ADD = 2, GMS_WARP_FILL = 3 };
typedef struct gms_warp {           /* 64 bytes */
    double tx, ty, c, s;            /*  0: the pose of the source map's world frame in the destination's world */
    double clamp;                   /* 32: GMS_WARP_ADD: the result is clamped to [-clamp, clamp]; 0 = no clamp */
    int32_t x0, y0, w, h;           /* 40: the destination cell rectangle, as gms_view's */
    int32_t op, pad;                /* 56: GMS_WARP_*; pad is not read */
} gms_warp;
typedef struct gms_warp_stats {     /* 80 bytes */
    int64_t pair[3][3];             /*  0: [class of the destination cell BEFORE the call][class of its source cell]; 0 unknown, 1 free, 2 occupied */
    int64_t n_outside;              /* 72: cells of the rectangle without a source cell */
} gms_warp_stats;
/* Pure host code: tx = x, ty = y, c = cos(theta), s = sin(theta) with the host's libm (x, y, theta finite); the other fields stay. */
int gms_warp_pose(gms_warp *w, double x, double y, double theta);
/* Pure host code: every check above that needs no handle. */
int gms_warp_check(const gms_warp *w);
/* Map mi_src of src through w into map mi_dst of dst.  The host form synchronises the destination's stream and returns the counts;
 * _dev writes them to device memory (8-byte aligned) on the destination's stream and synchronises nothing. */
int gms_map_warp(gms_map *dst, int32_t mi_dst, gms_map *src, int32_t mi_src, const gms_warp *w, gms_warp_stats *stats);
int gms_map_warp_dev(gms_map *dst, int32_t mi_dst, gms_map *src, int32_t mi_src, const gms_warp *w, gms_warp_stats *dev_stats);
/* The per-particle filter as the source: the logData of the shown particle, as gms_slam_download_map would return it, into map mi_dst of
 * dst.  `which`, GMS_VIEW_STRONGEST, `filter`, *shown (may be NULL; _dev: a device int32_t *) and the GMS_ERR_STATE cases are
 * gms_slam_view's; particle and generation are picked on the device.  The filter is only read: no later result of it changes. */
int gms_slam_warp(gms_slam *s, int32_t which, int32_t filter, gms_map *dst, int32_t mi_dst, const gms_warp *w, gms_warp_stats *stats, int32_t *shown);
int gms_slam_warp_dev(gms_slam *s, int32_t which, int32_t filter, gms_map *dst, int32_t mi_dst, const gms_warp *w, gms_warp_stats *dev_stats,
                      int32_t *dev_shown);

/* ---- census of the particles' maps: what the ENSEMBLE of a gms_slam's maps says, cell by cell ------------------------------------------
 * Every other query of a gms_slam looks at one particle's map; gms_slam_combined looks at all of them, but as the reference's
 * noisy-OR picture (a never-observed cell is p = 0.5 in every particle and comes out "occupied").  The census is the unweighted vote
 * of one filter's particles -- after a resample the population itself carries the weights -- : a majority map to plan on that does
 * not jump when the strongest particle changes, the per-cell split that is the map uncertainty, and every particle's distance from the
 * consensus.  This library's own definition (the reference has no such method); everything is integer arithmetic and every output is
 * unique whatever the scheduling.
 *
 * THE CLASS      of a cell of a particle's logData l, the predicates of the planes, the casts and the warps: free (1) l < 0, occupied
 *                (2) l > 0, unknown (0) everything else -- +0.0, -0.0, NaN.  -inf is free, +inf occupied, denormals count by sign.
 * THE COUNTS     for filter f of the handle (n particles per filter, n <= 65535) and every cell of the whole map:  fr = how many of
 *                its particles hold the cell free, oc = how many occupied.  counts is uint16 [H][W][2] = {fr, oc}; equivalently one
 *                little-endian uint32 per cell, fr in the low half, oc in the high half.
 * THE CONSENSUS  of a cell under min_known in [1, n]:  unknown (0) if fr + oc < min_known;  else occupied (2) if oc >= fr -- a tie
 *                goes to the obstacle, the conservative side for planning --;  else free (1).  consensus is uint8 [H][W].
 * THE TOTALS     gms_census_totals:  cls[k] the cells of consensus class k;  contested the cells with fr > 0 and oc > 0;  minority
 *                the sum over all cells of min(fr, oc);  n and min_known as the call took them.
 * THE AGREEMENT  one record of ten uint32 per particle of the filter:  pair[3][3], indexed [the particle's class][the consensus
 *                class], counted over all cells of the map, and a tenth word that is 0.  The nine entries sum to W * H.  A depleted
 *                filter shows as identical records, a drifted particle as a large pair[1][2] + pair[2][1].
 * WRITE_MAP      GMS_CENSUS_WRITE_MAP in flags: the consensus is also written to logData of the handle's own map (a batched handle:
 *                map f), as gms_slam_combined writes there -- +1.0 occupied, -1.0 free, +0.0 unknown -- and the map is left exactly
 *                as gms_map_upload_log of that array would leave it (the deferred pass first, likelihoodData until the next build,
 *                planes and tables invalidated).  Every gms_map_* query then works on the consensus through gms_slam_handles.
 *
 * Any output may be NULL; all of them NULL without WRITE_MAP is refused.  Refused with GMS_ERR_INVALID and nothing touched: a NULL
 * handle or request, min_known outside [1, n], filter outside [0, n_filters), flag bits other than GMS_CENSUS_WRITE_MAP, a non-zero
 * reserved word, nothing asked for, and -- _dev -- counts or agree not 4-byte aligned or totals not 8-byte aligned.  GMS_ERR_STATE on
 * a shard of a filter (gms_slam_create_shard): the counts of shards are additive, so a sharded form is one all-reduce of the count
 * field away, and it is not built.  The call reads the current generation of the filter's logData (which flips on resampling,
 * picked on the device) and changes nothing of the filter: poses, weights, maps, class planes, field state and history stay.
 * The count field and, where the caller passes none, the consensus bytes are scratch of the handle, allocated by the first call.
 *
 * How: a counting pass that streams the filter's n x cells doubles once -- a workgroup takes a tile of cells and a chunk of
 * particles (gms_census_geometry), a lane a pair of cells by one 16-byte load per particle where the pair is 16-byte aligned, sums
 * `free | occupied << 16` in a register and adds its chunk with one integer atomic per non-zero cell word into the zeroed field --;
 * a pass over the field that writes the consensus and forms the totals by ballots; and, only where agree is asked for, a second pass
 * over the maps against the consensus bytes, nine ballots per cell, one atomic per counter and workgroup. */
enum { GMS_CENSUS_WRITE_MAP = 1 };
typedef struct gms_census {         /* 16 bytes */
    int32_t min_known;              /*  0: cells that fewer particles than this have seen stay unknown; 1 .. n */
    int32_t filter;                 /*  4: the filter of a batched handle; 0 on a plain one */
    int32_t flags;                  /*  8: GMS_CENSUS_WRITE_MAP */
    int32_t reserved;               /* 12: must be 0 */
} gms_census;
typedef struct gms_census_totals {  /* 32 bytes */
    uint32_t cls[3];                /*  0: cells by consensus class: unknown, free, occupied */
    uint32_t contested;             /* 12: cells with fr > 0 and oc > 0 */
    uint64_t minority;              /* 16: sum over all cells of min(fr, oc) */
    uint32_t n, min_known;          /* 24: as the call took them */
} gms_census_totals;
/* Pure host code: every bound of the request for a handle of n_filters filters of n_per particles each, with the reason. */
int gms_census_check(const gms_census *c, int32_t n_per, int32_t n_filters);
/* Pure host code: the cells a workgroup of the counting pass takes, the particles of its chunk, and the cells a workgroup of the
 * agreement pass takes (any may be NULL): where the kernels' edges are, for tests and for sizing. */
int gms_census_geometry(int32_t *tile_cells, int32_t *chunk_particles, int32_t *agree_cells);
/* counts uint16 [H][W][2], consensus uint8 [H][W], agree uint32 [n][10], totals: host memory; synchronises the handle's stream. */
int gms_slam_census(gms_slam *s, const gms_census *c, uint16_t *counts, uint8_t *consensus, uint32_t *agree, gms_census_totals *totals);
/* The same into device memory on the handle's stream: nothing is waited for and nothing read back. */
int gms_slam_census_dev(gms_slam *s, const gms_census *c, uint16_t *dev_counts, uint8_t *dev_consensus, uint32_t *dev_agree, gms_census_totals *dev_totals);

/* ---- device-resident inputs ---------------------------------------------------------------------
 * The same entry points for callers whose scans / poses already live in HBM (a trace staged once, a
 * torch tensor, the output of a device-side motion model).  dev_beams is [n_maps][B] gms_beam,
 * dev_poses [n_maps][3], dev_xytheta [n_maps][n][3]; all are read on the handle's stream, asynchronously: the call
 * returns before the kernels run, so the buffers must stay valid and unmodified until the stream has passed them
 * (gms_map_synchronize, or an event of the caller's on that stream) -- in particular, memory handed back to a caching
 * allocator that serves another stream may be reused too early. */
int gms_map_integrate_dev(gms_map *m, const gms_beam *dev_beams, int32_t B, const float *dev_poses);
int gms_map_integrate_at_dev(gms_map *m, const gms_beam *dev_beams, int32_t B, gms_pf *pf, int32_t which);
int gms_map_update_dev(gms_map *m, const gms_beam *dev_beams, int32_t B, const float *dev_poses);
int gms_map_update_at_dev(gms_map *m, const gms_beam *dev_beams, int32_t B, gms_pf *pf, int32_t which);
int gms_pf_set_poses_dev(gms_pf *pf, const float *dev_xytheta);
int gms_pf_score_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B);
/* One scan through the whole path: SLAM.update(z, u) (J/slam/SLAM.java:80-131) followed by its caller's
 * `if (neff < fraction * N) resample()` (J/app/GridMapApp.java:185-186).  dev_xytheta (may be NULL) are the
 * motion-model samples; resample_fraction < 0 skips the resampling; integrate = 0 is the skipUpdate case
 * (SLAM.java:82).  r01[n_maps] is read on the host.  Nothing is read back. */
int gms_slam_update_dev(gms_pf *pf, const float *dev_xytheta, const gms_beam *dev_beams, int32_t B, const double *r01,
                        double resample_fraction, int32_t integrate);
/* SLAM.update(z, u) with the motion-model sample inside (J/slam/SLAM.java:80-131, line 90 included) and the caller's resampling
 * rule: every particle takes Odometry.apply (J/slam/Odometry.java:77-96; the variates of gms_pf_sample_motion for the same seed
 * and sequence -- bit-identical to that call followed by gms_slam_update_dev with dev_xytheta = NULL) on its way into the scoring
 * launch: four launches per scan, no launch for the motion model.  Stand-alone filters. */
int gms_slam_update_u_dev(gms_pf *pf, double d_center, double d_theta, uint64_t seed, uint64_t sequence, const gms_beam *dev_beams,
                          int32_t B, const double *r01, double resample_fraction, int32_t integrate);
/* One recorded revolution as GridMapApp.onHandleData treats it (J/app/GridMapApp.java:133-192), in one call: the raw polar
 * measurements are de-skewed with the frame's odometry (:143-175, as gms_map_deskew), every particle takes a motion-model sample
 * (J/slam/SLAM.java:90, as gms_pf_sample_motion with the same seed and sequence), then the scan step of gms_slam_update_dev on
 * the de-skewed scan.  Bit-identical to those three calls; the de-skew and the motion model share a launch (five launches per
 * frame).  Single-map, stand-alone filters.  angle / distance / hit [length] are host arrays and may be reused on return. */
int gms_slam_frame(gms_pf *pf, const double *angle, const double *distance, const uint8_t *hit, int32_t length, double d_center,
                   double d_theta, uint64_t seed, uint64_t sequence, const double *r01, double resample_fraction, int32_t integrate);
/* The same scan step with HOST inputs (what a JNI caller holds): poses (may be NULL) and the scan are copied into
 * pinned staging rings before the call returns (the caller may reuse its buffers at once) and pulled in by the
 * device without a stream synchronise; stats (may be NULL; when given the call synchronises) receives SLAM.update's
 * return values. */
int gms_slam_update(gms_pf *pf, const float *xytheta, const gms_beam *beams, int32_t B, const double *r01,
                    double resample_fraction, int32_t integrate, gms_pf_stats *stats);

/* ---- multi-GPU plumbing (particles sharded over ranks; collectives stay with the caller) ------- */
/* Number of doubles of the block-partial vector exchanged by an all-reduce(SUM):
 * 9 per global block of GMS_BLOCK particles {sum w, max w, first index of max, zero count, max
 * log-weight, sum w^2, sum x*w, sum y*w, sum theta*w}: everything SLAM.update reports follows from them. */
int gms_pf_partials_len(const gms_pf *pf, int64_t *n_doubles);
/* Phase 1 of normalise on a shard: writes this shard's block partials into dev_partials (device
 * pointer, zero elsewhere), ready for all-reduce(SUM) -- adding zeros is exact, so the reduced
 * vector is the same for any number of ranks. */
int gms_pf_local_partials(gms_pf *pf, double *dev_partials);
/* Phase 2: consumes the all-reduced partials: weightSum, strongest, Neff, weighted pose,
 * weight /= weightSum; then packs
 * this shard's {weight, x, y, theta} (24 B per particle) into dev_packed for the all-gather. */
int gms_pf_apply_partials(gms_pf *pf, const double *dev_partials, void *dev_packed);
/* Statistics only (weighted pose, Neff) of the CURRENT particles from an all-reduced partial vector,
 * nothing rewritten: e.g. getWeightedPose after a resample (J/app/GridMapApp.java:192). */
int gms_pf_stats_from_partials(gms_pf *pf, const double *dev_partials);
/* Packs this shard's current {weight, x, y, theta} without normalising (e.g. to all-gather the
 * population again after a resample, for getWeightedPose). */
int gms_pf_pack(gms_pf *pf, void *dev_packed);
/* Phase 3: consumes the all-gathered [n_global] packed particles: they become the source population
 * of gms_pf_resample (every rank then fills its own slots from the same global array).  Zero copy: the
 * buffer is read in place by later calls and must stay valid and unmodified until the next
 * gms_pf_import_global / gms_pf_normalize on this handle, or its destruction. */
int gms_pf_import_global(gms_pf *pf, const void *dev_packed_global);

/* ---- multi-GPU with the exchanges inside the library (RCCL, one process per GPU) ---------------- */
/* RCCL is bound at run time.  gms_comm_load names the shared object (NULL/"" = the copy the process already
 * holds, else the loader's librccl.so); the other entry points load the default on first use. */
int gms_comm_load(const char *librccl_path);
/* 128 opaque bytes (ncclUniqueId): one rank makes them, the host distributes them to every rank. */
int gms_comm_unique_id(void *id128);
/* Joins the communicator; blocks until all `world` ranks have called it.  One communicator per device. */
int gms_comm_create(gms_comm **out, const void *id128, int32_t rank, int32_t world, int32_t device);
int gms_comm_destroy(gms_comm *c);
int gms_comm_rank(const gms_comm *c, int32_t *rank, int32_t *world);
/* SLAM.update's weight bookkeeping (J/slam/SLAM.java:100-124) for a filter sharded with gms_pf_set_shard into
 * equal shards in rank order: block partials -> all-reduce(SUM) -> normalise -> START of the all-gather of the
 * packed normalised particles on the communicator's side stream.  On return (stream order) the statistics and
 * the weighted / strongest pose are complete, so the map update can be enqueued beside the gather. */
int gms_pf_normalize_sharded_begin(gms_pf *pf, gms_comm *c);
/* Joins the gather; the global population becomes the source of gms_pf_resample[_if]. */
int gms_pf_normalize_sharded_end(gms_pf *pf, gms_comm *c);
/* gms_slam_update_dev for a sharded filter: every rank calls it with its shard's motion-model samples and the
 * same scan and r01.  ONE exchange per scan: the ranks all-gather their RAW weights + poses and their block partials
 * (one grouped RCCL launch); normalisation, statistics, map update and resample are local after that.  Results equal
 * the stand-alone filter's bit for bit. */
int gms_slam_update_sharded_dev(gms_pf *pf, gms_comm *c, const float *dev_xytheta, const gms_beam *dev_beams, int32_t B,
                                const double *r01, double resample_fraction, int32_t integrate);
/* The same with HOST inputs (what a JNI caller holds; see gms_slam_update): this rank's shard of the motion-model samples
 * (may be NULL) and the scan are staged through the pinned rings; stats (may be NULL; synchronises) receives
 * SLAM.update's return values, identical on every rank. */
int gms_slam_update_sharded(gms_pf *pf, gms_comm *c, const float *xytheta, const gms_beam *beams, int32_t B, const double *r01,
                            double resample_fraction, int32_t integrate, gms_pf_stats *stats);
/* The same step for a host that brings its own collectives: _begin (poses, weights, this shard's payloads), then the
 * caller all-gathers BOTH buffers of gms_pf_gather_buffers in place (rank r's payload sits at r * per-rank size;
 * equal shards in rank order), then _end.  The buffers belong to the handle and keep their addresses until
 * gms_pf_set_shard / destroy. */
int gms_slam_update_sharded_begin_dev(gms_pf *pf, const float *dev_xytheta, const gms_beam *dev_beams, int32_t B);
int gms_pf_gather_buffers(gms_pf *pf, void **dev_packed_global, int64_t *packed_bytes_per_rank, double **dev_partials_global,
                          int64_t *partials_doubles_per_rank);
int gms_slam_update_sharded_end_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, const double *r01,
                                    double resample_fraction, int32_t integrate);

/* ---- measurement ------------------------------------------------------------------------------- */
enum {
    GMS_K_RAYCAST = 0, GMS_K_APPLY = 1, GMS_K_LIKELIHOOD = 2, GMS_K_SCORE = 3, GMS_K_REDUCE = 4,
    GMS_K_RESAMPLE = 5, GMS_K_REFINE = 6, GMS_K_EXCHANGE = 7 /* the grouped RCCL launch of a sharded scan step */,
    GMS_K_ORDER = 8 /* the locality order of the particles ahead of a large scoring launch */,
    GMS_K_MAPCOPY = 9 /* resample()'s deep copies of the particles' maps (gms_slam_resample_maps) */, GMS_K_COUNT = 10
};
/* Bracket kernel launches of this map handle (and its filters) with HIP events on its stream:
 * bit k of `mask` enables kernel class k (GMS_K_*); 0 turns profiling off. */
int gms_profile_enable(gms_map *m, int32_t mask);
int gms_profile_reset(gms_map *m);
/* Bracket only every stride-th launch of an enabled class (default 1): the two event markers of a bracket cost
 * microseconds on the stream, which a 70 us scan step notices. */
int gms_profile_sample(gms_map *m, int32_t stride);
/* Total device milliseconds and launch count of kernel class k since the last reset. */
int gms_profile_get(gms_map *m, int32_t k, double *total_ms, int64_t *launches);
/* What such a bracket costs by itself: the mean event-to-event time around an EMPTY kernel (dispatch latency + the
 * ~1 us an empty kernel runs), over `reps` launches on the handle's stream.  A kernel-trace profiler reports the
 * kernel's own duration, i.e. roughly the bracketed time minus this. */
int gms_profile_calibrate(gms_map *m, int32_t reps, double *bracket_ms);
/* The same in its two parts: bracket_ms as above; kernel_ms = what one empty kernel takes when `reps` of them run back to back
 * with nothing between them (the floor of any launch in a kernel trace).  bracket_ms - kernel_ms is what the two event markers
 * add to a bracketed launch: subtract it from a bracketed duration to get what a kernel-trace profiler reports. */
int gms_profile_calibrate2(gms_map *m, int32_t reps, double *bracket_ms, double *kernel_ms);

/* Census of the likelihood-field tiles (64 x 32 cells) the rebuilds have walked since the last call, summed over the handle's
 * maps: out4 (may be NULL) = {left alone: no cell changes its thresholded code under the scan's counts; constants kept: a
 * uniform tile that already holds its constants; constants written: a uniform tile; blurred: both passes of
 * Util.doGaussianBlurdSeparable (J/app/Util.java:378-426)}.  Reads and clears the counters (synchronises when out4 is given);
 * enable != 0 keeps counting, 0 stops (the default: off).  The reference rebuilds every cell on every scan
 * (J/slam/GridMap.java:233-250); the sum of the four is what a dirty-tile rebuild looked at. */
int gms_map_tile_stats(gms_map *m, int32_t enable, int64_t *out4);

/* ---- diagnostics ------------------------------------------------------------------------------- */
/* The float-rounded device primitives the parity contract leans on, for tests: op 0 = (float)sqrt(a)
 * (GridMap.java:217), 1 = (float)cos((double)a), 2 = (float)sin((double)a) (J/math/MathUtil.java:30-40); 3 = self-check of the
 * wavefront butterflies every reduction uses (n a multiple of 64): out[i] = a bit code, bits 0-5 set where the exchange with lane
 * (i ^ 32, 16, 8, 4, 2, 1) does not deliver that lane's value (must be 0), bits 6-11 the same for the mirrored reading (must be 63 << 6 for the half-wave, row and quad-of-four steps that have one);
 * 4 / 5 = the squared thresholds the per-particle-map ray cast classifies cells with instead of a square root per cell: the smallest float s with
 * (float)sqrt(s) >= a, resp. the largest with (float)sqrt(s) <= a (SensorModel.java:31-41 compares (float)Math.sqrt(s) with a). */
int gms_debug_f32(gms_map *m, int32_t op, const float *in, float *out, int64_t n);
/* Launches of the casts' bit-plane pre-pass on this handle so far (gms_map_cast): casts of an unchanged map add none. */
int gms_map_cast_plane_builds(const gms_map *m, int64_t *builds);
/* Development: how many of this filter's scoring launches so far ordered their workgroups' lanes by the segment's end-point lines
 * (k_score_c<1, true>: single-map handles, 1024-lane workgroups; GMS_SCORE_SEGORDER, GMS_SCORE_ORDER=0).  Results
 * do not depend on it; tests read it to know which kernel ran. */
int gms_pf_segment_order_launches(const gms_pf *pf, int64_t *launches);
/* Development: instrumented builds (-DGMS_STAMPS) write wall-clock stamps of their kernels' stages to dev_buffer
 * ([workgroup][16] uint64, 10 ns units; NULL turns it off); a product build returns GMS_ERR_STATE.  tools/stamps.py. */
int gms_debug_set_stamps(gms_map *m, void *dev_buffer);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
