// gms_internal.h -- shared between the C-ABI host code and the gfx950 kernels of libgridmapslam.so.
// Not part of the public interface (that is include/gridmapslam.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "gridmapslam.h"

// ---- device-side view of a GridMap (J/slam/GridMap.java fields, widened once on the host) -------
struct GridDev {
    int32_t W, H;
    int64_t cells;        // W*H
    double posx, posy;    // (double) position.x / .y
    double res;           // (double) resolution
    double rinv;          // RN(1.0 / res), for j_cell_of
    float resf;           // resolution
    double l_free, l_occ; // log-odds increments
    int32_t extra;        // RayIterator additionalSteps
    float half_tol;       // hitTolerance / 2 (float arithmetic)
    double z_hit;         // zHit
    double c_rand;        // zRandom * 1.0 / SENSOR_MAX_RANGE
    double inv_max;       // 1.0 / SENSOR_MAX_RANGE
    int32_t ktaps, khalf;
    int32_t fpitch;       // factor table: row pitch W + 16; column W of every row and all of row H hold the neutral 1.0 (fac_index)
    uint32_t fneutral;    // factor table: index of one neutral entry (row H, column W)
    uint32_t *tile_stats; // [64][4] likelihood-tile census (gms_map_tile_stats) or nullptr: {left alone, constants kept, constants written, blurred}
};

// one ray of a scan in grid coordinates (GridMap.integrateObservation's locals)
struct RayIn {
    float sx, sy, ex, ey, measured;
    int32_t hit;
};

// device-resident statistics of one particle set (one per map)
struct PfStatsDev {
    double weight_sum;    // sum of raw weights
    double norm_sum;      // sum of normalised weights (calculateNeff's `sum`)
    double sq_sum;        // sum((w/norm_sum)^2)
    double xs, ys, ts;    // getWeightedPose numerators
    double max_w;         // largest raw weight
    double max_logw;
    int32_t strongest;
    int32_t n_zero;
    float wpose[3];       // weighted pose
    float spose[3];       // strongest particle's pose
    int32_t did_resample;
    int32_t n_ambiguous;
};

#define GMS_SCORE_MAXSEG 32
#ifndef GMS_SCORE_SEGLEN
#define GMS_SCORE_SEGLEN 45        // beams per segment product of the default scoring kernel, scans of more than GMS_SCORE_SHORT_SCAN beams
#endif
#define GMS_SCORE_SEGLEN_SHORT 12  // ... and of shorter scans (see gms_launch_pf_score)
#define GMS_SCORE_SHORT_SCAN 384
#define GMS_SCORE_SEGLEN_LONG 90   // ... and of scans of more than GMS_SCORE_LONG_SCAN beams
#define GMS_SCORE_LONG_SCAN 768
#define GMS_SCORE_SEGLEN_LONG_BATCHED 120   // ... on batched handles (which are never sharded)
static_assert(128 * GMS_SCORE_MAXSEG >= GMS_MAX_BEAMS, "a scan must fit GMS_SCORE_MAXSEG segments of 128 beams");
#define GMS_PARTIAL_STRIDE 9   // per block: sum w, max w, first argmax, n_zero, max logw, sum w^2, sum x*w, sum y*w, sum th*w

// packed particle exchanged by the all-gather (24 B)
struct PackedParticle {
    double w;
    float x, y, theta;
    uint32_t pad;
};

struct ProfSlot {
    hipEvent_t a, b;
    int32_t k;
};

// Pinned host staging for inputs that arrive as host buffers: a small ring, so that copying the next scan's inputs
// never waits for the stream to drain -- only (rarely) for the copy that last used the same slot.
#define GMS_STAGE_SLOTS 4
struct StageRing {
    void *slot[GMS_STAGE_SLOTS] = {};
    hipEvent_t ev[GMS_STAGE_SLOTS] = {};
    bool busy[GMS_STAGE_SLOTS] = {};
    int32_t next = 0;
};

// The beam sensor model's factor tables on the device (gms_beams.hip): n_tables slots of GMS_BEAM_TAB_BYTES, each factors [2][T] | their
// logarithms [2][T], T = behind + ahead + 2 <= GMS_BEAM_T_MAX; allocated by the first gms_beam_table_put, freed by gms_beam_table_free
struct BeamTables {
    double *d_tab;
    StageRing ring;                 // pinned staging of a table on its way
    int32_t ring_ready;
};

struct gms_map {
    gms_params prm;
    GridDev gd;
    int32_t n_maps;
    int32_t device;
    int32_t n_cus;            // compute units of the device (hipDeviceAttributeMultiprocessorCount; 256 on MI355X)
    int32_t lds_per_cu;       // bytes of LDS per compute unit (160 KiB on MI355X)
    int32_t max_beams;
    int32_t n_filters;        // live gms_pf handles bound to this map (gms_map_destroy refuses while > 0)
    hipStream_t own_stream;
    hipStream_t stream;
    double *d_log;        // [n_maps][H][W]
    double *d_lik;        // [n_maps][H][W]
    double *d_fac;        // [n_maps][fac_stride]: per-cell scoring factor f(likelihood) (GridMap.java:285-288), rows of g.fpitch entries with a neutral border (fac_index),
                          // kept in step with d_lik; entry [cells] of each map is the neutral factor 1.0
    int64_t fac_stride;   // (H + 1) * fpitch
    uint32_t *d_cnt;      // [n_maps][H][W] per-scan packed counts (n_free | n_occ << 16): the grid the NEXT ray cast accumulates into, all zero between scans
    uint32_t *d_cnt_pend; // the second grid: while apply_pending, the counts of the scan whose apply pass is deferred (the two swap roles
                          // when a scan's apply is deferred, so that the next ray cast can share a launch with that apply pass)
    int32_t *d_bbox;      // [2][n_maps][4] encoded box of the cells changed since the last likelihood build;
                          // double-buffered: k_apply clears the idle half, so no memset is ever queued
    int32_t bbox_cur;     // half in use
    int32_t bbox_dirty;   // an integrate ran since the last likelihood build
    double *d_taps;       // [ktaps]
    uint8_t *d_tile_state;  // [n_maps][likelihood tiles][2 halves of a tile's rows]: 0 unknown, 1..3 the tile of d_lik/d_fac holds the constants of a uniform tile of code 0 / 0.5 / 1
    uint32_t *d_tile_stats; // [64][4] counters behind gd.tile_stats (always allocated; gd.tile_stats points at them while the census is on)
    gms_beam *d_beams;    // [n_maps][max_beams] staging
    float *d_poses;       // [n_maps][3] staging
    double *d_scratch;    // small device scratch
    unsigned char *d_view; // staging of the host forms of the map queries (HostStage): [16 bytes: the shown index][the parts]; grows, never per request
    size_t view_cap;      // its size in bytes
    // the map's bit planes (gms_map_plane), indexed by GMS_CLEAR_OCCUPIED (logData > 0: what the casts walk) / GMS_CLEAR_NOT_FREE
    // (!(logData < 0)): d [n_maps][H][gms_plane_wpr], bit x & 31 of word x >> 5 of row y, allocated by the first request of that mode;
    // current: it is the plane of logData as it stands (map_planes_stale clears it)
    struct { uint32_t *d; int32_t current; } plane[2];
    int32_t cast_walk_mem;    // casts walk memory even where their window or class plane fits the LDS (GMS_CAST_WALK=mem: tests)
    int32_t gain_walk_mem;    // view gains read plane bits from memory even where the plane windows fit the LDS (GMS_GAIN_WALK=mem: tests)
    int32_t rollout_walk_mem; // rollouts read plane bits from memory instead of the LDS window (GMS_ROLLOUT_WALK=mem: tests)
    int32_t rollout_cpw;      // candidates a rollout workgroup takes: GMS_ROLLOUT_CANDIDATES (GMS_ROLLOUT_CPW = 1 .. 256: tools/rollout_probe.py)
    int64_t cast_plane_builds;    // launches of the GMS_CLEAR_OCCUPIED plane's pre-pass so far (tests: an unchanged map is not packed again)
    uint32_t *d_clear_scratch;    // [H][gms_plane_wpr] a gms_slam's queries: the shown particle's plane, packed per request (gms_slam_plane)
    // cost-to-go fields (gms_reach.hip); everything below is allocated by the first field that needs it and only ever grows
    uint16_t *d_reach_field;      // [H][W] the working field the tiles relax
    uint16_t *d_reach_d2;         // [H][W] inflate > 0: the whole map's clearance field at R = inflate ...
    uint32_t *d_reach_plane;      // [H][gms_plane_wpr] ... and the blocked plane balloted from it
    uint32_t *d_reach_ctl;        // {tile runs (64 bits), the active count of four rounds, 2 spare} | [2][tiles] the tiles' active flags of this round and the next
    uint32_t *h_reach_ctl;        // pinned: the first 8 words of it, read back once per batch of rounds
    int32_t reach_rounds;         // gms_map_reach_stats: rounds launched for the last field
    int64_t reach_tile_runs;      // ... and tile relaxations that ran
    // routes (gms_route.hip): the descended paths of a request that gave no `cells`, [P][max_cells][2]; grows and never shrinks
    int32_t *d_route_path;
    int64_t route_cap;            // cells it holds
    // sites and skeleton (gms_skeleton.hip): the site field the ridge pass reads, the request's rectangle and one cell around it; grows
    // and never shrinks
    uint32_t *d_site_field;
    int64_t site_cap;             // cells it holds
    // frontier regions (gms_frontier.hip); allocated by the first request, the region table grows and never shrinks
    uint32_t *d_front_plane;      // [2][H][gms_plane_wpr] the frontier plane, and the plane of the regions' roots (label == own index)
    uint32_t *d_front_nf;         // [H][gms_plane_wpr] a gms_slam's: the shown particle's second plane (its first: d_clear_scratch)
    uint32_t *d_front_label;      // [H][W] the label field of the whole map; defined where the frontier plane has a bit
    uint32_t *d_front_wscan;      // [words] the root plane's word counts, scanned within blocks of GMS_SCAN | [blocks] the blocks' offsets
    unsigned char *d_front_table; // [front_cap] gms_frontier | [front_cap] the goals' 64-bit keys | [front_cap] the kept flags, scanned | [blocks] their offsets
    int32_t front_cap;            // regions the table holds
    uint32_t *d_front_ctl;        // {regions, regions with count >= min_size}
    uint32_t *h_front_ctl;        // pinned: read back once per request
    // rooms and doors (gms_rooms.hip); allocated by the first request, the two tables grow and never shrink
    uint32_t *d_rooms_field;      // [H][W] the cores' cell counts at their roots, then the working keys cost << 16 | rank the tiles relax
    uint32_t *d_rooms_label;      // [H][W] the cores' label field; defined where the core plane has a bit
    uint32_t *d_rooms_plane;      // [2][H][gms_plane_wpr] the core plane, and the plane of the kept cores' roots
    uint32_t *d_rooms_wscan;      // [words] the kept roots' word counts, scanned within blocks of GMS_SCAN | [blocks] the blocks' offsets
    uint32_t *d_rooms_ctl;        // {tile runs (64 bits), the active count of four rounds, rooms, door entries, door table overflow, 7 spare} | [2][tiles] the tiles' active flags
    uint32_t *h_rooms_ctl;        // pinned: the first 16 words of it
    unsigned char *d_rooms_table; // [rooms_cap] gms_room | [rooms_cap] the rooms' anchor indices by rank | [3][rooms_cap] the doors per smaller room: scanned, kept, filled | [blocks + 1] the scan's offsets and total
    int32_t rooms_cap;            // rooms the table holds
    unsigned char *d_rooms_doors; // [rooms_door_cap] the pair keys rank_a << 16 | rank_b, open addressing | [rooms_door_cap] what each entry accumulates | [rooms_door_cap] the entries' indices by run
    int32_t rooms_door_cap;       // entries the door table holds, a power of two
    int32_t rooms_rounds;         // gms_map_rooms_stats: rounds launched by the last call
    int64_t rooms_tile_runs;      // ... tile relaxations that ran
    int32_t rooms_door_rebuilds;  // ... and how often the door table was doubled and filled again
    double rooms_stage_us[GMS_ROOMS_STAGES];  // gms_map_rooms_stage_us: the last call's parts on the host clock (GMS_ROOMS_STAGES in the environment), else 0
    // particle seeding (gms_scatter.hip): the table of the last request -- every map's eligible plane and its scanned counts --, allocated
    // by the first request; current: it is the table of logData as it stands for exactly that request (map_planes_stale clears it)
    struct {
        uint64_t *d_elig;         // [n_maps][words] the eligible plane, words = H * wpr64 64-bit words per map
        uint32_t *d_pre;          // [n_maps][words] its word counts, scanned within blocks | [n_maps][blocks] the blocks' offsets | [n_maps] M
        int32_t x0, y0, w, h, inflate, mode;      // the request it was built for (mode: GMS_CLEAR_NOT_FREE where inflate == 0)
        int32_t current;
        int64_t builds;           // tables built so far (tests: a scatter on an unchanged map builds none)
    } scatter;
    int32_t scatter_shift;        // the draw stages every (1 << shift)-th word's prefix at least this coarsely (GMS_SCATTER_SHIFT: tests of the search in memory)
    // global scan matching (gms_locate.hip); allocated by the first request, the work lists grow and never shrink
    struct {
        uint64_t *d_pyr;          // [7][H][wpr64] the OR pyramid's planes P_1 .. P_7 (P_0 is the hit plane, read in place)
        uint64_t *d_list[2];      // the work lists of alternate levels: entries k << 40 | y << 20 | x; after level 0 the survivors' keys
        int64_t list_cap[2];      // entries each holds
        uint32_t *d_ctl;          // {the two lists' counters, the threshold, 5 spare} | [GMS_MAX_BEAMS + 1] the proven leaves' score histogram
        uint32_t *h_ctl;          // pinned: the first 8 words of it, read back once per level
        int32_t levels;           // gms_map_locate_stats: the top level of the last request ...
        int64_t evaluated[8];     // ... and the candidates it evaluated per level
    } locate;
    int32_t locate_levels;        // the top level of every request, whatever its rectangle (GMS_LOCATE_LEVELS = 0 .. 7: tests; 0 is the exhaustive search); -1: from the rectangle
    int32_t need_full_build;  // likelihood field must be rebuilt everywhere (upload/reset/copy)
    int32_t apply_pending;    // the last scan's counts are not in logData yet (deferred apply pass, gms_flush_apply)
    int32_t raycast_tile;     // batched ray casts accumulate in LDS tiles (k_raycast_tile; GMS_RAYCAST_TILE=0 turns it off)
    int32_t raycast_tile_min; // ... when the launch has more rays than this in all (default 4096; GMS_RAYCAST_TILE_MIN)
    int32_t taps_plain;       // every tap is +0.0 or in [2^-900, 2^900]: sums of tap * {0, 1, 2} scale exactly by 0.5 and a tap * 0.0 may stand for a skipped one
    int32_t lik_kh;           // the likelihood kernels' compile-time half width (3 or 5), or 0 = the generic path: another kernel size, or a tap
                              // that is negative or outside 2^-900 .. 2^900 (the fast path computes twice the horizontal sums and halves them --
                              // exact only while nothing is subnormal -- and starts a sum with its first product instead of 0.0 + it -- the
                              // same bits only while that product is not -0.0; likelihood_body)
    int32_t lik_split;        // dirty-tile rebuilds of a single map give every tile two workgroups when the chip has them to spare (GMS_LIK_SPLIT=0: one)
    int32_t lik_lazy;         // scan steps' dirty-tile rebuilds write the factor table only, likelihoodData on demand (GMS_LIK_LAZY=0 turns it off)
    int32_t lik_stale;        // likelihoodData is behind the factor table somewhere (gms_ensure_lik brings it up to date)
    int32_t fac_current;      // the factor table is the field of logData + the pending counts as of the last rebuild, and logData has not moved since except by those counts
    int32_t lik_skip;         // dirty-tile rebuilds leave tiles alone whose codes the scan does not change (GMS_LIK_SKIP=0 turns it off; same bits)
    int32_t raycast_near;     // single-map ray casts: the first 64 steps of every ray go through near-field workgroups with an LDS tile (0 never, 1 for scans of 512 beams or more, 2 for every scan of 32 or more: GMS_RAYCAST_NEAR=0 / unset / 1)
    int32_t pair_launches;    // scan steps pair independent kernels in one launch (GMS_PAIR_LAUNCHES=0 turns it off)
    int32_t slam_threads;     // per-particle maps: lanes per workgroup of k_slam_particle (0 = the launcher decides; GMS_SLAM_THREADS = 512 / 1024)
    int32_t slam_tile_cells;  // per-particle maps: cap on the LDS count tile of k_slam_particle in cells (0 = what the LDS allows; GMS_SLAM_TILE_CELLS, for tests of the band walk)
    gms_beam *h_beams;    // pinned staging (de-skew inputs, single-ray entry)
    StageRing beam_ring;  // pinned staging of scans handed over as host buffers
    float *h_poses;       // pinned staging
    hipEvent_t pose_copy_ev;  // the last copy out of h_poses
    int32_t pose_copy_ev_set;
    int32_t *d_trace_cells; uint8_t *d_trace_cls; int32_t *d_trace_cnt;
    size_t trace_cap_cells, trace_cap_counts;   // capacities of d_trace_cells/d_trace_cls (cells) and d_trace_cnt (counts)
    // profiling
    int32_t prof_on;
    int32_t prof_stride;      // every prof_stride-th launch of an enabled class is bracketed (>= 1)
    int64_t prof_seen[GMS_K_COUNT];
    std::vector<ProfSlot> prof_pending;
    std::vector<ProfSlot> prof_free;
    double prof_ms[GMS_K_COUNT];
    int64_t prof_n[GMS_K_COUNT];
};

// ---- map state transitions (need_full_build, fac_current, lik_stale, apply_pending, bbox_dirty, bbox_cur): each is named for
// what happened and sets every field that event affects ----
// logData moved: neither bit plane is the plane of logData as it stands, nor is the seeding table its table
static inline void map_planes_stale(gms_map *m) { m->plane[GMS_CLEAR_OCCUPIED].current = m->plane[GMS_CLEAR_NOT_FREE].current = m->scatter.current = 0; }
// logData (or, gms_map_upload_likelihood, the field) was replaced: the next rebuild covers every tile and leaves none alone
static inline void map_log_replaced(gms_map *m) { m->need_full_build = 1; m->fac_current = 0; map_planes_stale(m); }
// likelihoodData is up to date everywhere (made so, or about to be replaced wholesale)
static inline void map_lik_current(gms_map *m) { m->lik_stale = 0; }
// an immediate apply pass added the counts to logData without a rebuild having seen them
static inline void map_counts_applied(gms_map *m) { m->bbox_dirty = 1; m->fac_current = 0; map_planes_stale(m); }
// a deferred apply pass has been enqueued: the box of the scan it applied is the current half now
static inline void gms_apply_done(gms_map *m) {
    m->bbox_cur = 1 - m->bbox_cur;
    m->bbox_dirty = 0;
    m->apply_pending = 0;
    map_planes_stale(m);
}
// the scan just cast (and already in the likelihood field) keeps its counts for a later launch
static inline void gms_defer_apply(gms_map *m) {
    uint32_t *t = m->d_cnt; m->d_cnt = m->d_cnt_pend; m->d_cnt_pend = t;       // the other grid is all zero: the next ray cast's
    m->apply_pending = 1;
    m->bbox_dirty = 0;
}
// a likelihood rebuild of `mode` (likelihood_body) has been enqueued: 1 likelihoodData from what the factor table's last rebuild saw;
// 2 the factor table only, 3 both, from logData + the pending counts
static inline void map_field_built(gms_map *m, int32_t mode) {
    if ((mode & 3) == 1) { map_lik_current(m); return; }
    m->lik_stale = (mode & 3) == 2;
    m->fac_current = 1;
    m->need_full_build = 0;
}
// an immediate rebuild has read the box of the cells changed since the last one; k_apply cleared the other half
static inline void map_box_consumed(gms_map *m) {
    if (m->bbox_dirty) { m->bbox_cur = 1 - m->bbox_cur; m->bbox_dirty = 0; }
}

struct gms_pf {
    gms_map *map;
    int32_t n;            // particles held here (per map)
    int64_t offset;       // global index of particle 0
    int64_t n_global;
    int32_t n_maps;
    float *d_pose;                  // [n_maps][n][3] current poses x,y,theta (as at the boundary)
    float *d_pose2;                 // resample double buffer
    float *d_cs2;                   // ... and its trig
    double *d_w, *d_w2;             // [n_maps][n] weights
    double *d_logw, *d_logw2;       // [n_maps][n] sum(log factor)
    float *d_cs;                    // [n_maps][n][2] float-rounded cos/sin of theta
    double *d_hitbeams;             // [n_maps][max_beams][2] compacted hit beams
    double *d_part;                 // [n_maps][GMS_SCORE_MAXSEG][n] per-segment products (k_score_c)
    int32_t *d_nhit;                // [n_maps]
    double *d_partials;             // [n_maps][nblk_global][GMS_PARTIAL_STRIDE]
    double *d_wave_partials;        // [nchunks][GMS_PARTIAL_STRIDE] one row per wavefront: the stand-alone single-map scan step (k_partials_wave)
    double *d_p2;                   // [n_maps][nblk_global][2] {sum wn, sum wn^2} of the normalised global population
    PackedParticle *d_global_own;   // the library's own buffer; d_global may alias a caller's all-gather result
    double *d_chunk_tot;            // [n_maps][nchunks] scan chunk totals / offsets
    double *d_cum;                  // [n_maps][n_global] in-chunk inclusive sums
    double *d_res_pre;              // [n_maps][nchunks + 3] chunk offsets + grand total, sum wn, sq_sum: folded by the paired step's normalise (resample_prefix_last)
    uint32_t *d_res_ticket;         // [n_maps] its ticket counter (0 between launches)
    PfStatsDev *d_stats;            // [2][n_maps]: [0] of the last normalise, [1] of the current particles (recomputed on demand)
    PfStatsDev *h_stats;            // pinned
    double *d_r01;                  // [n_maps] (unused since the kernels read the pinned ring slot; kept for the allocation's alignment slack)
    const double *d_r01_src;        // [n_maps] where the resample kernel reads the draws: the current pinned ring slot (batched maps)
    double r01_scalar;
    int32_t *d_idx;                 // [n_maps][n]
    float *h_stage;                 // pinned staging for poses (read-back)
    StageRing pose_ring;            // pinned staging of pose proposals handed over as host buffers
    StageRing r01_ring;             // pinned staging of the per-map resampling draws (n_maps > 1)
    int32_t refine;                 // scan steps run findBestPose on every particle before weighting (gms_pf_set_refine)
    float4 *d_ord;                  // [n_maps][n] {x, y, cos, sin} of the particles in locality order (k_order)
    int32_t *d_perm;                // [n_maps][n] the particle at each position of that order
    int32_t log_norm;               // gms_pf_set_log_normalize: weights = exp(logw - max logw) instead of the plain product (stand-alone filters)
    int32_t score_threads;          // 0 the launcher decides (the largest of 1024 / 512 / 256 lanes per scoring workgroup that still gives every CU one); GMS_SCORE_THREADS forces 64..1024
    int32_t reference_order;        // gms_pf_set_reference_order: the audit path -- every re-associated chain (the scan's product, weightSum, the
                                    // cumulative weights) as ONE chain in the reference's order (tests; slow)
    int32_t score_spread;           // -1 the launcher decides (launches of two or more workgroups per CU), 0 / 1 forced (GMS_SCORE_SPREAD, read at creation)
    int32_t order_mode;             // -1 the launcher decides (large launches only), 0 never, 1 always (GMS_SCORE_ORDER; results do not depend on it)
    int32_t seg_order;              // the scoring workgroups' lanes in the order of their segment's end-point lines (k_score_c<1, true>): -1 the launcher
                                    // decides (single map, 1024-lane workgroups), 0 / 1 forced for every multi-wavefront shape of a single map (GMS_SCORE_SEGORDER); GMS_SCORE_ORDER=0 turns it off too
    int64_t seg_order_launches;     // scoring launches that took that order so far (gms_pf_segment_order_launches: tests)
    // pose modes (gms_modes.hip): scratch of the last request, allocated by the first one; the bins' part and the table grow and never shrink
    struct {
        uint32_t *d_part;           // [n] every particle's bin | [n] its label
        uint32_t *d_bins;           // [bins_cap] the bins' counts | [bins_cap] the label field | [bins_cap] the root flags, scanned | [blocks] their offsets
        int64_t bins_cap;
        unsigned char *d_table;     // [table_cap] the modes' integers | [table_cap] the kept flags, scanned | [table_cap] the stored records' labels | [blocks] the flags' offsets
        int64_t table_cap;
        uint32_t *d_ctl;            // {modes, modes with count >= min_count, OUTSIDE particles, spare}
        uint32_t *h_ctl;            // pinned: read back once per request
    } modes;
    BeamTables beam;                // the beam sensor model (gms_beams.hip): ONE table, the last call's
    int32_t slam_owned;            // the filter of a gms_slam: its particles own maps, so resampling, sharding and the shared-map scan steps are refused on it
    int32_t *d_epoch2;              // the filter of a gms_slam, inside its draw only (slam_draw): {draws that ran so far, the last resample() drew}, kept by the resampling kernels (NULL otherwise)
    // What the derived device data describes.  Written by the pf_* transitions below only (and pf_alloc_global / pf_free_global).
    // weights:
    int32_t pending_nseg;           // > 0: d_w / d_logw are stale, the weights are still d_part's pending_nseg segment products
    int32_t score_fresh;            // d_w / d_logw (or the segment products) come from a scoring pass nothing has consumed yet: only those
                                    // may be log-normalised (gms_pf_lognorm_now); weights the caller set or a resample copied are taken as they are
    // statistics:
    int32_t stats_current;          // the d_stats slot that describes the current particles: 0 none, 1 d_stats[0] (a normalise), 2 d_stats[1] (recomputed)
    int32_t neff_folded;            // d_stats[0].norm_sum / sq_sum have been folded from d_p2 (d_p2 is produced with the chunk sums)
    // resampling source:
    PackedParticle *d_global;       // [n_maps][n_global] source population: d_global_own, or a caller's all-gather result (gms_pf_import_global)
    int32_t have_global;            // d_global holds the current population
    int32_t global_raw;             // ... with RAW weights (gathered before the normalisation): resample divides
    int32_t chunks_ready;           // d_cum / d_chunk_tot hold level 0 of the scan of d_global
    int32_t res_pre_ready;          // d_res_pre holds that level 0's chunk offsets, grand total, sum wn and sq_sum (folded by the paired normalise)
};

// ---- filter state transitions: each is named for what happened and sets every field that event affects ----
// one rank's block of a filter spread over several (gms_pf_set_shard), not a stand-alone filter
static inline bool pf_is_shard(const gms_pf *pf) { return pf->offset != 0 || pf->n_global != pf->n; }
// the poses changed (host, motion model, refinement) or how they are weighed did: the source and the statistics are stale
static inline void pf_particles_changed(gms_pf *pf) { pf->have_global = 0; pf->stats_current = 0; }
// a scoring launch wrote new weights: nseg > 1 segment products per particle, or the combined product (nseg <= 1)
static inline void pf_scored(gms_pf *pf, int64_t nseg) {
    pf_particles_changed(pf);
    pf->pending_nseg = nseg > 1 ? (int32_t)nseg : 0;
    pf->score_fresh = 1;
}
// a resample replaced the particles by copies: their weights are not the log-weights' (d_logw is not permuted)
static inline void pf_resampled(gms_pf *pf) { pf_particles_changed(pf); pf->score_fresh = 0; }
// the host set the weights (or reset the particles): d_w no longer belongs to d_logw
static inline void pf_weights_set(gms_pf *pf) { pf_particles_changed(pf); pf->pending_nseg = 0; pf->score_fresh = 0; }
// a launch stored the combined weights in d_w / d_logw
static inline void pf_weights_combined(gms_pf *pf) { pf->pending_nseg = 0; }
// the raw weights were combined and packed for an exchange: the scoring pass has been consumed
static inline void pf_raw_packed(gms_pf *pf) { pf->pending_nseg = 0; pf->score_fresh = 0; }
// the weights were normalised (the scoring pass consumed) and d_stats[0] describes the particles.  own: the population was packed into
// d_global_own with level 0 of its scan; folded: Neff and the chunk offsets as well (d_res_pre).  Otherwise it went to a caller's slot only.
static inline void pf_normalized(gms_pf *pf, bool own, bool folded) {
    pf->score_fresh = 0;
    pf->stats_current = 1;
    if (own) { pf->d_global = pf->d_global_own; pf->global_raw = 0; }
    pf->have_global = pf->chunks_ready = own;
    pf->neff_folded = pf->res_pre_ready = own && folded;
}
// the audit path normalised d_w in place (k_normalize_seq): no packed population
static inline void pf_normalized_in_place(gms_pf *pf) { pf->have_global = 0; pf->stats_current = 1; pf->score_fresh = 0; }
// d_stats[1] was recomputed from the current particles
static inline void pf_stats_recomputed(gms_pf *pf) { pf->stats_current = 2; }
// d_global's contents were rewritten: nothing derived from them holds
static inline void pf_source_written(gms_pf *pf, int32_t raw) {
    pf->global_raw = raw;
    pf->chunks_ready = 0;
    pf->neff_folded = 0;
    pf->res_pre_ready = 0;
}
// src (a gather, an import, a pack) is the current population now
static inline void pf_source_replaced(gms_pf *pf, PackedParticle *src, int32_t raw) {
    pf->d_global = src;
    pf->have_global = 1;
    pf_source_written(pf, raw);
}
// level 0 of the scan of d_global was made (k_chunk_sums or beside a normalise), without the paired prefix
static inline void pf_chunks_made(gms_pf *pf) { pf->chunks_ready = 1; pf->res_pre_ready = 0; }
// the own weights normalised beside the chunk sums of the gathered raw population (k_raycast_norm_chunks)
static inline void pf_normalized_gathered(gms_pf *pf) {
    pf_source_replaced(pf, pf->d_global_own, 1);
    pf_chunks_made(pf);
    pf->stats_current = 1;
}
static inline void pf_neff_folded(gms_pf *pf) { pf->neff_folded = 1; }
// a resampling launch folded Neff, from the paired prefix where there was one
static inline void pf_prefix_consumed(gms_pf *pf) { pf->res_pre_ready = 0; pf->neff_folded = 1; }

// one rank's side of the RCCL exchanges of a sharded filter (gms_host.hip)
struct gms_comm {
    void *nccl = nullptr;           // ncclComm_t
    int32_t rank = 0, world = 1, device = 0;
    int32_t overlap = 0;            // all-gather on the side stream (default: world > 2; GMS_COMM_OVERLAP=0/1 overrides)
    int32_t pending = 0;            // an all-gather is in flight
    int32_t broken = 0;             // an exchange failed: every later call on this communicator fails fast
    int32_t p2p = 0;                // GMS_EXCHANGE=p2p: the scan's exchange as grouped ncclSend/ncclRecv instead of all-gathers
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

// Every particle's GridMapData of a gms_slam, both generations, as the kernels see it.  WHICH generation is current is a device-side
// fact: resample() writes its deep copies into the other one, and `if (neff < n / 2) resample()` (GridMapApp.java:185-186) is decided on
// the device, so the host cannot know without a round trip.  epoch[0] counts the draws that ran (kept by the resampling kernels,
// gms_pf::d_epoch2): its parity is the current generation; epoch[1] says whether the last resample() drew.
// A batched handle (gms_params.n_maps = S filters of n_per particles each, particle p of filter p / n_per) keeps one such pair per
// filter: epoch[2 f], epoch[2 f + 1].
struct SlamBufs {
    double *log[2], *lik[2];        // [n][H][W]
    uint32_t *code[2];              // [n][2][code_words] class planes, or NULL
    int32_t *epoch;                 // [S][2]
    int32_t n_per;                  // particles per filter
};
// one filter of a batched update (gms_slam_update_batch): a table of S of them travels with the scans' beams, in the same copy
struct SlamFilterArgs {
    double d_center, d_theta, d_center_sd, d_theta_sd;     // its odometry and the motion model's deviations (Odometry.java:63-64)
    uint64_t seed;
    int32_t count;                  // beams of its scan
    int32_t flags;                  // bit 0: draw the motion-model sample (SLAM.java:90); bit 1: integrate the scan (not skipUpdate, :82)
};
static_assert(sizeof(SlamFilterArgs) % 16 == 0, "the table is staged behind the beams in 16-byte units");
// the update kernels' view of a batch: filter f = particle / n reads beams + f * beam_stride and tab[f] (tab NULL: not batched)
struct SlamBatch {
    const SlamFilterArgs *tab;
    int32_t n, beam_stride;
};
static inline SlamBatch slam_batch_of(const gms_pf *pf, const SlamBatch *batch) { return batch ? *batch : SlamBatch{nullptr, pf->n, 0}; }

// where the likelihoodData of a gms_slam's particles stands between the calls that write it
enum SlamField : int32_t {
    SLAM_FIELD_IN_MEMORY,           // the current generation holds it
    SLAM_FIELD_OWED_COPY,           // ... does not hold the last resample()'s copies yet (if it drew): slot m's field is the other generation's [d_idx_lik[m]]
    SLAM_FIELD_FROM_PLANES          // it is behind: every particle's is the field of plane 1 of its class planes (made on demand)
};

// SLAM as the reference has it (J/slam/SLAM.java): N particles, each with its own GridMapData (gms_slam_host.hip, gms_slam_kernels.hip)
struct gms_slam {
    gms_map *map;                   // ONE map's worth of handle: the GridMap (geometry, constants, taps), the stream, staging, profiling; its own
                                    // logData / likelihoodData receive the combined map (gms_slam_combined, GridMapApp.calculateCombined)
    gms_pf *pf;                     // the N particles' poses, weights, statistics and resampling indices (one "map" of N particles)
    int32_t n;                      // particles held: n_filters * n_per, filter f's particle k at f * n_per + k
    int32_t n_filters;              // independent filters of the handle (gms_params.n_maps): batched entry points only when > 1
    int32_t n_per;                  // particles per filter
    double *d_log[2], *d_lik[2];    // [n][H][W] every particle's GridMapData, double-buffered for resample()'s deep copies
    int32_t *d_epoch;               // [n_filters] x {draws that ran so far, the last resample() drew}: filter f's current generation is d_epoch[2 f] & 1 (SlamBufs)
    int64_t copies_base;            // maps copied by resampling steps before the last reset (the rest: sum of d_epoch[2 f] * n_per)
    gms_beam *d_batch;              // [n_filters][max_beams] beams | [n_filters] SlamFilterArgs: a batched update's inputs (gms_slam_update_batch)
    StageRing batch_ring;           // pinned staging of that block, or of a frame's raw revolutions and table (gms_slam_frame_batch)
    std::vector<int32_t> frame_counts;   // [n_filters] measurements of every filter's revolution in the last frame call (empty: none yet; gms_slam_last_beams)
    int32_t *d_plan;                // a shard's resample(): [3][n] device staging of {export list | local sources | positions in the received buffer}
    int32_t shard_moves;            // a shard: the last gms_slam_shard_draw drew and its copies are still to be made -- gms_slam_shard_export and
                                    // gms_slam_shard_gather are open (the gather closes them again; so do a draw that does not draw and gms_slam_reset)
    int32_t lazy_lik;               // resample() copies logData at once and likelihoodData when somebody asks for it: the next update's
                                    // computeLikelihoodMap overwrites every cell of it before anything on the path reads one (GMS_SLAM_LAZY_LIK_COPY=0: both at once)
    SlamField field;                // where every particle's likelihoodData stands (handle-wide).  Written by the slam_* transitions below only.
    int32_t *d_idx_lik;             // [n] SLAM_FIELD_OWED_COPY: the source indices of the resample() that owes the copies
    uint32_t *d_code[2];            // [n][2][code_words] every particle's class planes (gms_slam_kernels.hip), double-buffered with logData; NULL: not kept
                                    // (the blur kernel is wider than the on-demand evaluation takes, the plane does not fit the LDS, or GMS_SLAM_EAGER_LIK=1)
    int64_t code_words;             // 32-bit words per plane
    int32_t have_strongest;         // an update has normalised since the last reset: the filter's statistics name a strongest particle (gms_slam_view)
    int32_t refine;                 // gms_slam_set_refine: update() runs findBestPose on every particle against its own field before weighting it (SLAM.java:96)
    int32_t refine_field;           // the field in front of the refinement: -1 from the class plane where logData exceeds the infinity cache, 0 from logData
                                    // always, 1 from the plane always (GMS_SLAM_REFINE_FIELD=log|codes: tests of both forms)
    // the particles' paths (gms_slam_set_history; off while hist_cap == 0: nothing allocated, nothing launched)
    int32_t hist_cap;               // rows of the ring
    int32_t *d_hist_parent;         // [hist_cap][n]     (SlamHist)
    float *d_hist_pose;             // [hist_cap][n][3]
    int32_t *d_hist_lin[2];         // [n] the composed source of every slot over the draws since the last recorded update, and the buffer the next
                                    // draw composes into (a filter's slots may span workgroups: in place would race)
    int32_t hist_lin_cur;           // which of the two holds it: every draw's compose writes the other one, drawn or not, so the host knows
    int64_t *d_hist_steps;          // {updates recorded, ticket}: the count the kernels go by
    int64_t hist_steps;             // ... and the host's mirror of it: every update through slam_update_core records exactly one row
    int32_t hist_walk_mem;          // the back-trace chases through memory even where a row fits the LDS (GMS_SLAM_HISTORY_WALK=mem: tests)
    int32_t refine_lds;             // -1 the field in LDS whenever it fits (computed there from the class plane where it can be), 0 never, 2 staged from
                                    // memory wherever it fits (GMS_SLAM_REFINE_LDS: tests of the other forms)
    // per-particle scan alignment (gms_slam_set_align; gms_slam_align.hip)
    int32_t align_on;               // update() aligns every particle against its own field between computeLikelihoodMap and the weighting
    gms_align_params align_prm;     // ... with these parameters (checked when they were set)
    int32_t align_field;            // -1 the field's values from the class plane whenever it is kept and fits the LDS, 0 from memory always, 1 as -1
                                    // (GMS_SLAM_ALIGN_FIELD=memory|planes: tests of both forms)
    int32_t align_form;             // the form the last alignment launch took (gms_slam_align_form); 0: none yet
    gms_align_record *d_align_rec;  // [n] the records of the last aligned update (allocated by gms_slam_set_align)
    int32_t have_align_rec;         // an aligned update has run since they were allocated
    // the beam sensor model on the particles' own maps (gms_slam_score_beams, gms_slam_set_beam_model; gms_slam_beams.hip)
    struct : BeamTables {           // TWO tables: [0] the last stand-alone call's, [1] the model's that every update applies
        double *d_wgt;              // [n] beam weights | [n] beam log-weights of the update under way (allocated by gms_slam_set_beam_model)
        int32_t on;                 // update() weighs every particle by the model, through its own map as it stands in front of the scan
        int32_t behind, ahead;      // ... with this table (checked when it was set)
        int32_t combine;            // GMS_SLAM_BEAMS_MULTIPLY / _REPLACE
    } beam;
    // the census of the particles' maps (gms_slam_census; gms_census.hip): the count field [cells] uint32, then the consensus bytes
    // [cells] of a call that passes none; allocated by the first call (the map's size never changes)
    uint32_t *d_census;
};

// the history of a gms_slam as its kernels see it (gms_slam_set_history): a ring of cap rows, update number t in row t % cap
struct SlamHist {
    int32_t *parent;                // [cap][n] the filter-local slot of the row before that every slot's particle descends from
    float *pose;                    // [cap][n][3] every slot's pose when that update returned
    int64_t *steps;                 // {updates recorded since the history was cleared, the append kernel's ticket}
    int32_t cap, n, n_per;
};

// ---- field state transitions of a gms_slam (gms_slam::field): each is named for what happened; together they are its only writers.
// A batched handle keeps one state for all its filters: the copy kernels skip the filters that did not draw ----
// createMapData(null) per particle (GridMap.java:106-117): likelihoodData a fresh double[] = 0.0, written out
static inline void slam_was_reset(gms_slam *s) { s->field = SLAM_FIELD_IN_MEMORY; }
// an update rewrote every cell of every field (an owed copy is moot), or -- on_demand -- skipped it: probabilityOf reads the field under
// the scan's end points only (GridMap.java:273-277) and the kernels evaluate exactly those cells from the particle's plane; what a caller
// may read afterwards, the field of logData as it stands NOW, stays defined by plane 1 and is written when asked for
static inline void slam_field_updated(gms_slam *s, bool on_demand) { s->field = on_demand ? SLAM_FIELD_FROM_PLANES : SLAM_FIELD_IN_MEMORY; }
// a resample ran on a field that was not owed a copy.  From the planes: they travel with logData, and so does the field.  In memory:
// copied at once (GridMap.java:121), or -- lazy_lik -- when it is asked for: SLAM.update starts with computeLikelihoodMap of every
// particle (SLAM.java:93), which overwrites every cell of it, so nothing on the path ever reads the copies
static inline void slam_resampled(gms_slam *s, bool lazy_lik) {
    if (s->field == SLAM_FIELD_IN_MEMORY && lazy_lik) s->field = SLAM_FIELD_OWED_COPY;
}
// the field was written out for a reader (a download, an upload's other slots, a second resample() in a row)
static inline void slam_field_materialised(gms_slam *s) { s->field = SLAM_FIELD_IN_MEMORY; }
// a shard's draw: its likelihoodData is never copied, it is the field of plane 1 of the class planes, which travel.  Whatever was
// written out for a reader is dropped (the planes still define it)
static inline void slam_shard_drew(gms_slam *s) { s->field = SLAM_FIELD_FROM_PLANES; }

// the thread's last-error text + code (gms_host.hip); every C-ABI file reports through it
int gms_fail(int code, const char *fmt, ...);
#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return gms_fail(GMS_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)
#define REQUIRE(cond, msg)                                         \
    do {                                                           \
        if (!(cond)) return gms_fail(GMS_ERR_INVALID, "%s", msg);  \
    } while (0)
// gms_pf_set_shard behind its refuse_owned_maps guard (gms_host.hip; not exported): gms_slam_create_shard places its own filter through it
extern "C" int gms_pf_place_shard(gms_pf *pf, int64_t offset, int64_t n_global);
// `later` waits (stream order, no host synchronise) for everything enqueued on `earlier` so far (gms_host.hip; not exported): how two
// handles on different streams hand arrays to each other (gms_map_copy, gms_map_combine, the map warps)
extern "C" int gms_stream_after(hipStream_t later, hipStream_t earlier, const char *what);
// host beams [n_maps][B] -> the map's device staging buffer [n_maps][max_beams] through the pinned ring (gms_host.hip)
int gms_stage_beams(gms_map *m, const gms_beam *beams, int32_t B);
// the scan of a filter-wide request (one scan per map): the host form's is staged into m->d_beams, the maps max_beams apart; a device
// form's is the caller's own, the maps B apart
static inline int gms_request_scan(gms_map *m, const gms_beam *beams, int32_t B, bool on_device, const gms_beam **d_beams, int32_t *beam_stride) {
    *d_beams = beams; *beam_stride = B;
    if (on_device) return GMS_OK;
    const int rc = gms_stage_beams(m, beams, B);
    if (rc) return rc;
    *d_beams = m->d_beams; *beam_stride = m->max_beams;
    return GMS_OK;
}
// ---- the one launch path of the kernels that take dynamic LDS ----
// What a launch may ask for without opting in.  The runtime takes 64 KiB unasked on this hardware; 48 KiB, the threshold most launchers
// already went by, is the conservative choice: an opt-in too many costs one host call per kernel and device, once.
#define GMS_LDS_FREE ((size_t)48 * 1024)
// devices whose opt-ins are remembered; a handle on a device beyond them opts in at every launch above GMS_LDS_FREE
#define GMS_LDS_DEVICES 64
// The opt-in of Kernel to `bytes` of dynamic LDS on `device` (the handle's, which every entry point has made current: HIP keeps a
// function, and this attribute, per device).  The high-water mark of what was set is kept per (kernel, device) and the runtime is
// called only when a launch asks for more: the launchers pass whatever this launch needs, the units with a constant cap pass the cap.
// Handles may be driven from different threads: the mark is a relaxed atomic -- it orders nothing, it only has to be read and written
// whole -- and it is raised after the attribute was set, under a lock, so two threads may both set the attribute and can never both skip it
// or leave the mark above what the runtime holds.  A failed opt-in leaves the mark alone; the launch behind it then fails as well.
template <auto Kernel>
static inline hipError_t gms_kernel_lds(int32_t device, size_t bytes) {
    static std::atomic<size_t> mark[GMS_LDS_DEVICES];          // (0: nothing set, GMS_LDS_FREE holds)
    static std::mutex raising;
    if (bytes <= GMS_LDS_FREE) return hipSuccess;
    const bool known = device >= 0 && device < GMS_LDS_DEVICES;
    if (known && bytes <= mark[device].load(std::memory_order_relaxed)) return hipSuccess;
    std::lock_guard<std::mutex> lock(raising);
    if (known && bytes <= mark[device].load(std::memory_order_relaxed)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && known) mark[device].store(bytes, std::memory_order_relaxed);
    return e;
}
// Kernel on the handle's stream with smem bytes of dynamic LDS, opted in to where that is needed.  Errors surface as the launch's own:
// the entry point's hipGetLastError reports them
template <auto Kernel, typename... Args>
static inline void gms_launch(const gms_map *m, dim3 grid, dim3 block, size_t smem, const Args &...args) {
    (void)gms_kernel_lds<Kernel>(m->device, smem);
    hipLaunchKernelGGL(Kernel, grid, block, smem, m->stream, args...);
}
// a run-time choice as a type, for the launchers' dispatch to kernel template arguments: `if (k == 3) launch(gms_c<3>{})`, and the
// generic lambda `[&](auto kh)` names the instantiation k_x<kh()>.  Every launcher lists its combinations itself
template <auto V>
using gms_c = std::integral_constant<decltype(V), V>;
// the box of every map (gms_map::d_bbox: two halves of [n_maps][4]): the half in use, or -- idle -- the other one
static inline int32_t *map_box(const gms_map *m, bool idle = false) {
    return m->d_bbox + (size_t)(idle ? 1 - m->bbox_cur : m->bbox_cur) * m->n_maps * 4;
}
// host beams [rows][B] (or none: beams NULL) -> dst [rows][pitch], then tab_bytes of tab behind them, as ONE copy out of a slot of ring
// (gms_host.hip; the ring's slots hold rows * pitch beams + tab_bytes)
int gms_stage_block(gms_map *m, StageRing &ring, const gms_beam *beams, int32_t B, int32_t rows, int32_t pitch, const void *tab, size_t tab_bytes,
                    void *dst);
int gms_ring_alloc(StageRing &r, size_t bytes);
void gms_ring_free(StageRing &r);
// the ring's next slot, free for the host to fill; commit after enqueueing whatever reads it on `stream` (gms_host.hip)
int gms_ring_acquire(StageRing &r, void **out);
int gms_ring_commit(StageRing &r, hipStream_t stream);

// ---- kernel launchers (gms_map_kernels.hip / gms_pf_kernels.hip) -----------------------------
// Each enqueues on the handle's stream and returns; the entry point that called it checks hipGetLastError.  Kernels with dynamic LDS
// go through gms_launch above (the opt-in is nobody else's business); a launcher that picks among instantiations writes the argument
// list once, in a generic lambda over gms_c tags, and lists the combinations in plain ifs.  The geometry several launchers share is
// said once: map_box here, apply_blocks / lik_resident / lik_tile_blocks in gms_map_kernels.hip, slam_lik_blocks in gms_slam_kernels.hip.

void gms_launch_raycast(gms_map *m, const gms_beam *d_beams, int32_t B, int32_t beam_stride, const float *d_poses,
                        int32_t pose_stride, bool take_pending_apply = false);
bool gms_raycast_tiled(const gms_map *m, int32_t B);
void gms_launch_trace_scan(gms_map *m, const gms_beam *d_beams, int32_t B, const float *d_pose,
                           int32_t *d_cells, uint8_t *d_cls, int32_t cap, int32_t *d_counts);
void gms_launch_trace_ray(gms_map *m, float x0, float y0, float x1, float y1, int32_t extra,
                          int32_t *d_cells, int32_t cap, int32_t *d_count);
void gms_launch_apply_ray(gms_map *m, RayIn ray);
void gms_launch_apply_counts(gms_map *m);
void gms_launch_likelihood(gms_map *m, int32_t dirty_only, bool counts_pending = false, bool materialize = false);
void gms_ensure_lik(gms_map *m);        // likelihoodData up to date everywhere (the scan steps' rebuilds write the factor table only)
void gms_flush_apply(gms_map *m);       // the deferred apply pass, if one is pending
// likelihoodData up to date, then logData (the deferred apply pass): what entry points that read or replace logData open with
static inline void gms_map_settle(gms_map *m) { gms_ensure_lik(m); gms_flush_apply(m); }
bool gms_likelihood_split(const gms_map *m, int32_t blocks);      // likelihood_body's SPLIT = 2 for a dirty-tile rebuild launched with `blocks` workgroups?
size_t gms_likelihood_lds_bytes(int32_t khalf, bool coded = true);   // coded: the byte-coded staging of the compile-time half widths (gms_map::lik_kh != 0)
int32_t gms_likelihood_blocks_cap(const gms_map *m, size_t smem);
void gms_launch_raycast_apply(gms_map *m, const gms_beam *d_beams, int32_t B, int32_t beam_stride, const float *d_poses, int32_t pose_stride);
void gms_launch_fill(gms_map *m, double *d, double v, int64_t n);
void gms_launch_combine(gms_map *src, gms_map *dst);
void gms_launch_deskew(gms_map *m, const double *d_angle, const double *d_distance, const uint8_t *d_hit, int32_t length,
                       double d_center, double d_theta, gms_beam *d_out);
void gms_launch_factors(gms_map *m);   // d_fac from d_lik (after an upload / copy)
void gms_launch_noop(gms_map *m);
bool gms_set_stamp_buffer(gms_map *m, void *dev_buffer);
void gms_launch_spin(gms_map *m, double us);
void gms_launch_copy(gms_map *m, void *dst, const void *src, size_t nbytes);   // src may be pinned host memory
void gms_invalidate_tile_state(gms_map *m);
void gms_launch_get_raw(gms_map *m, int32_t mi, int32_t x, int32_t y, double *d_out2);
void gms_launch_debug_f32(gms_map *m, int32_t op, const float *d_a, float *d_out, int64_t n);
// a view of one map's array (GridMap.render's grey levels, gridmapslam.h "map views"; src: W x H doubles of v->source's kind)
void gms_launch_view(gms_map *m, const double *src, const gms_view *v, void *d_out);

// ---- map queries: views, predicted scans (gms_cast.hip), view gain (gms_gain.hip), clearance fields (gms_clearance.hip), cost-to-go fields
// (gms_reach.hip), frontier regions (gms_frontier.hip), particle seeding (gms_scatter.hip), global scan matching (gms_locate.hip), pose modes
// (gms_modes.hip), the beam sensor model (gms_beams.hip: beside cast, on the base alone) and trajectory rollouts (gms_rollout.hip: on reach,
// whose blocked plane they test).  The layering: the query base (gms_query.hip:
// everything down to query_plane), then clearance, then reach (it inflates with gms_clear_launch), then frontier, scatter and locate (they inflate
// with gms_reach_inflate); cast and gain beside clearance, on the base alone, as modes (it takes the staging only).  Cast and beams share their device-side
// probe geometry -- the staged plane window and the first-hit walk -- through gms_probe.h, a device header on gms_device.h alone; the two
// beam models share their whole workgroup body through gms_beams_device.h on top of it.  Clearance and sites and skeleton
// (gms_skeleton.hip, beside clearance on the base) are ONE separable transform under two policies, kernels, launcher and checks, in
// gms_nearest_device.h on gms_regions.h ----
struct gms_slam;
// the rectangle (x0, y0) + w x h (already w, h >= 1 and x0, y0 >= 0) inside a W x H map: the one copy of the test and its message
int gms_rect_check(int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t W, int32_t H, const char *what);
// gms_view_size's checks, then the rectangle; *bytes: the image's size
int gms_view_check(const gms_view *v, int32_t W, int32_t H, const char *what, int64_t *bytes);
// which particle of a gms_slam a request shows: `which` in range, or GMS_VIEW_STRONGEST with `filter` in range on a handle that is no
// shard and has updated.  *filter_out: the filter the kernels receive (0 when a particle is named)
int gms_slam_shown(const gms_slam *s, int32_t which, int32_t filter, const char *what, const char *filter_name, int32_t *filter_out);
// the one lazy allocator: *p stays what it is, or becomes `bytes` of device memory
template <typename T>
static inline int gms_dev_alloc(T **p, size_t bytes, const char *who, const char *what) {
    if (*p) return GMS_OK;
    if (hipMalloc(p, bytes) != hipSuccess) {
        *p = nullptr;
        return gms_fail(GMS_ERR_NOMEM, "%s: %s of %zu bytes could not be allocated", who, what, bytes);
    }
    return GMS_OK;
}
// its pinned counterpart, for the words a request reads back: *p stays what it is, or becomes `bytes` of pinned host memory
template <typename T>
static inline int gms_pinned_alloc(T **p, size_t bytes, const char *who) {
    if (*p) return GMS_OK;
    if (hipHostMalloc(reinterpret_cast<void **>(p), bytes) != hipSuccess) {
        *p = nullptr;
        return gms_fail(GMS_ERR_NOMEM, "%s: pinned memory for the read-back could not be allocated", who);
    }
    return GMS_OK;
}
// The one grow-only device buffer: *p keeps holding at least `need` items (*cap: how many it holds), or is replaced by one of `need`
// rounded up to a multiple of `round` items, bytes(items) bytes; it never shrinks.  wait: the stream whose work may still read the old
// buffer, waited on before that is freed, or NULL where the caller knows that nothing is in flight on it.
template <typename T, typename C, typename F>
static inline int gms_dev_grow(T **p, C *cap, int64_t need, int64_t round, const hipStream_t *wait, F bytes, const char *who, const char *what) {
    if (*p && (int64_t)*cap >= need) return GMS_OK;
    if (*p && wait) HIPCHK(hipStreamSynchronize(*wait));
    hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const int64_t c = (need + round - 1) / round * round;
    int rc = gms_dev_alloc(p, bytes((size_t)c), who, what);
    if (!rc) *cap = (C)c;
    return rc;
}
// workgroups for n items at per_block each: at least one, at most `most` (the kernels stride over the rest)
static inline unsigned gms_grid(int64_t n, int64_t per_block, int64_t most) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > most ? most : b);
}
// The exclusive scan of uint32 counts (gms_query.hip), two launches on st, no workgroup waits on another.  vals [n]: every item becomes
// the sum of those before it within its block of GMS_SCAN items, in place; sums [blocks = ceil(n_cap / GMS_SCAN)]: every block's
// offset, the sum of the blocks before it; *total: the sum of all -- so item i's prefix is sums[i / GMS_SCAN] + vals[i] (scan_prefix).
// n = n_cap, or -- n_dev, a count in device memory -- min(*n_dev, n_cap); what lies behind n counts as 0 and is neither read nor
// written.  batch > 1: as many scans at once, entry b's items at vals + b * stride, its offsets at sums + b * sum_stride, its total in
// total[b].  Any number of blocks: the second launch, one workgroup per entry, walks them GMS_SCAN at a time with a carry.
#define GMS_SCAN 1024
void gms_launch_scan(hipStream_t st, uint32_t *vals, const uint32_t *n_dev, int64_t n_cap, uint32_t *sums, uint32_t *total, int32_t batch = 1,
                     int64_t stride = 0, int64_t sum_stride = 0);
// a bit plane's 32-bit words per row (rows padded to 64 cells)
static inline int32_t gms_plane_wpr(const gms_map *m) { return 2 * ((m->gd.W + 63) / 64); }
// the plane of `mode` of logData as it stands, every map's: the deferred apply pass first, then the pre-pass unless the handle still
// holds the plane of this logData
int gms_map_plane(gms_map *m, int32_t mode, const uint32_t **plane);
// its per-particle counterpart: the shown particle's plane under `mode` into gms_map::d_clear_scratch (d_dst: into that plane instead)
// and its handle-wide index into d_shown (may be NULL); which / filter as gms_slam_shown passed them
int gms_slam_plane(gms_slam *s, int32_t which, int32_t filter, int32_t mode, int32_t *d_shown, uint32_t *d_dst = nullptr);
// The device staging of a request's host form (none for a device form), over gms_map::d_view: [16 bytes: the shown index][the parts,
// each padded to 16 bytes].  Reserve the parts, open (the buffer grows only after a stream synchronise), take their device addresses
// (a device form's: the caller's own pointer), copy inputs up; after the launches queue the outputs and finish: the copies back, the
// shown index, ONE stream synchronise.
struct HostStage {
    gms_map *m;
    bool on_device;
    unsigned char *base = nullptr;
    size_t total = 0;
    struct { void *dst; size_t part, bytes; } out[4];
    int32_t n_out = 0;
    HostStage(gms_map *mm, bool dev) : m(mm), on_device(dev) {}
    size_t part(size_t bytes) { const size_t at = 16 + total; total += (bytes + 15) & ~(size_t)15; return at; }
    int open();
    template <typename T> T *at(size_t part, T *dev) const { return on_device ? dev : reinterpret_cast<T *>(base + part); }
    int32_t *shown(int32_t *dev) const { return at(0, dev); }
    int up(size_t part, const void *src, size_t bytes);
    void fetch(void *dst, size_t part, size_t bytes) { out[n_out].dst = dst; out[n_out].part = part; out[n_out++].bytes = bytes; }
    int finish(int32_t *shown);
};
// Where a query reads: map `index` of a shared handle (s NULL), or particle `index` (GMS_VIEW_STRONGEST: the strongest of `filter`) of
// a per-particle handle, m its map.  query_check: the map index in range, or gms_slam_shown (which settles `filter`); query_plane:
// ONE map's plane of `mode` -- gms_map_plane at the map's offset, or gms_slam_plane into the scratch plane / d_dst
struct QuerySource {
    gms_map *m;
    gms_slam *s;
    int32_t index, filter;
};
static inline QuerySource query_map(gms_map *m, int32_t mi) { return {m, nullptr, mi, 0}; }
static inline QuerySource query_slam(gms_slam *s, int32_t which) { return {s ? s->map : nullptr, s, which, 0}; }
int query_check(QuerySource &src, const char *what, const char *filter_name);
int query_plane(const QuerySource &src, int32_t mode, int32_t *d_shown, uint32_t *d_dst, const uint32_t **plane);
// the field of rectangle c of ONE map's plane into d_out (gms_clearance.hip; the cost-to-go fields inflate with it)
int gms_clear_launch(gms_map *m, const uint32_t *d_plane, const gms_clearance *c, uint16_t *d_out);
// the cost-to-go fields' blocked plane for inflate > 0 (gms_reach.hip): the clearance field of ONE map's obstacle plane at R = inflate over
// the whole map, balloted into gms_map::d_reach_plane (both allocated by the first request); the frontier regions share it
int gms_reach_inflate(gms_map *m, const uint32_t *d_obstacles, int32_t inflate, int32_t mode, const uint32_t **d_blocked);

void gms_launch_pf_init(gms_pf *pf);
void gms_launch_pf_pose_trig(gms_pf *pf, const float *d_src);
void gms_launch_pf_combine(gms_pf *pf);
void gms_launch_pf_motion(gms_pf *pf, double d_center, double d_theta, uint64_t seed, uint64_t sequence);
void gms_launch_pf_chunk_sums(gms_pf *pf);
// paired launches (gms_fused_kernels.hip)
void gms_launch_partials_apply(gms_pf *pf, double *d_partials, bool apply_rides_later = false);
bool gms_can_pair_launches(const gms_pf *pf, int32_t B);
void gms_launch_norm_raycast(gms_pf *pf, const double *d_partials, PackedParticle *d_packed_local, bool own,
                             const gms_beam *d_beams, int32_t B, bool wave_rows = false);
void gms_launch_lik_resample(gms_pf *pf, double fraction);
void gms_launch_deskew_motion(gms_pf *pf, const double *d_angle, const double *d_distance, const uint8_t *d_hit, int32_t length,
                              double d_center, double d_theta, uint64_t seed, uint64_t sequence);
void gms_launch_partials_pack_apply(gms_pf *pf, bool apply_rides_later = false);
void gms_launch_raycast_norm_chunks(gms_pf *pf, const gms_beam *d_beams, int32_t B, bool raycast);
void gms_launch_pf_fold_neff(gms_pf *pf);
struct MotionModel {            // one odometry step for gms_launch_pf_score's motion-model sample (Odometry.java:60-96)
    double d_center, d_theta;
    uint64_t seed, sequence;
};
// the motion model's deviations for one odometry step: the ONE copy of the two expressions -- bit parity between a batched filter, a
// stand-alone one and the shared-map filters rests on it (motion_args in gms_pf_kernels.hip, slam_filter_args)
static inline void motion_deviations(double d_center, double d_theta, double *d_center_sd, double *d_theta_sd) {
    *d_center_sd = (0.01 + fabs(d_center) * 0.05) / 2;                           // Odometry.java:63
    *d_theta_sd = 5 * (3.141592653589793 / 180.0) + 0.1 * fabs(d_theta);         // :64
}
void gms_launch_pf_score(gms_pf *pf, const gms_beam *d_beams, int32_t B, int32_t beam_stride, const float *d_pose_src = nullptr,
                         const MotionModel *motion = nullptr);   // d_pose_src: set the poses in the same launch
void gms_launch_pf_partials(gms_pf *pf, double *d_partials);
bool gms_pf_lognorm_now(const gms_pf *pf);
bool gms_pf_wave_partials_now(const gms_pf *pf);
void gms_launch_pf_partials_wave(gms_pf *pf);
void gms_launch_pf_pack(gms_pf *pf, PackedParticle *d_packed);
void gms_launch_pf_apply_partials(gms_pf *pf, const double *d_partials, PackedParticle *d_packed_local, bool own);
void gms_launch_pf_stats_only(gms_pf *pf, const double *d_partials, PfStatsDev *d_stats_out);
void gms_launch_pf_resample(gms_pf *pf, double fraction /* <0: unconditional */);
void gms_launch_pf_refine(gms_pf *pf, const gms_beam *d_beams, int32_t B, int32_t beam_stride);
void gms_launch_pf_normalize_seq(gms_pf *pf, PfStatsDev *d_stats_out, bool normalise);
void gms_launch_pf_resample_seq(gms_pf *pf, double fraction);
// one GridMapData per particle (gms_slam_kernels.hip); the buffers' current generation is read on the device (SlamBufs)
SlamBufs gms_slam_bufs(const gms_slam *s);
void gms_launch_slam_likelihood(gms_map *m, const SlamBufs &sb, int32_t n);
// the de-skew of a frame call: one raw revolution (tab_src NULL: length, d_center, d_theta) into d_out, or S of them -- rows of L raw
// measurements, filter f's length and odometry from tab_src[f], which the launch also copies to tab_dst[f] -- into rows of out_pitch beams
void gms_launch_slam_deskew(gms_map *m, const double *angle, const double *distance, const uint8_t *hit, int32_t L, int32_t S, int32_t Lmax,
                            int32_t length, double d_center, double d_theta, const SlamFilterArgs *tab_src, SlamFilterArgs *tab_dst, gms_beam *d_out,
                            int32_t out_pitch);
// batch (may be NULL): the filters' own beams, counts, motion and skipUpdate (B is then the largest count, motion non-NULL: the sequence)
void gms_launch_slam_particle(gms_pf *pf, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, bool field_in_memory, const MotionModel *motion,
                              int32_t integrate, int64_t code_words, const SlamBatch *batch = nullptr);
void gms_launch_slam_likelihood_codes(gms_map *m, const SlamBufs &sb, int64_t code_words, int32_t n, int32_t plane);
void gms_launch_slam_codes_from_log(gms_map *m, const SlamBufs &sb, int32_t first, int32_t count, int64_t code_words);
int64_t gms_slam_code_words(int64_t cells);
void gms_launch_slam_trace(gms_pf *pf, const gms_beam *d_beams, int32_t B, int32_t particle, int32_t *d_cells, uint8_t *d_cls, int32_t cap, int32_t *d_counts);
bool gms_launch_slam_refine(gms_pf *pf, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, const MotionModel *motion, int32_t field_in_lds,
                            int64_t code_words, const SlamBatch *batch = nullptr);
bool gms_slam_refine_from_planes(const gms_map *m, int32_t B, int32_t field_in_lds, int64_t code_words);
// per-particle scan alignment (gms_slam_align.hip): whether a scan of B beams is aligned on values computed from the class planes (no
// field has to be written in front of the launch), and the launch -- every particle held, in place; from_planes as that answer, else
// sb.lik's current generation holds the field of logData as it stands; motion (may be NULL): the motion-model sample is drawn first;
// d_rec [n] or NULL
int gms_align_check_for(const gms_align_params *p, const char *who);       // gms_align_check with the caller's name in the message (gms_align.hip)
bool gms_slam_align_from_planes(const gms_slam *s, int32_t B);
int gms_launch_slam_align(gms_slam *s, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, bool from_planes, const MotionModel *motion,
                          const gms_align_params *prm, gms_align_record *d_rec, const SlamBatch *batch = nullptr);
// the beam sensor model (gms_beams.hip, gms_slam_beams.hip): a table is factors [2][T] | their logarithms [2][T], T = behind + ahead + 2
#define GMS_BEAM_T_MAX 512
#define GMS_BEAM_TAB_BYTES (4 * GMS_BEAM_T_MAX * sizeof(double))
int gms_beam_model_check_for(int32_t behind, int32_t ahead, const double *factors, const char *who);   // gms_beam_model_check with the caller's name in the message
// the factors (checked by the caller) and their logarithms through the pinned ring into slot `which` of the n_tables in bt.d_tab, on m's stream
int gms_beam_table_put(gms_map *m, BeamTables &bt, const char *who, int32_t behind, int32_t ahead, const double *factors, int32_t which, int32_t n_tables);
void gms_beam_table_free(BeamTables &bt);
// ... on the particles' own maps (gms_slam_beams.hip): the launch -- every particle held walks its own logData of the current generation
// at its pose (motion non-NULL: the motion-model sample is drawn first and written) with table `which` of s->beam, weights into d_wgt /
// d_logw [n], d_res [n][B] or NULL; and the update's combine of beam.d_wgt into the filter's raw weights behind gms_launch_slam_particle
void gms_launch_slam_beams(gms_slam *s, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, const MotionModel *motion, int32_t behind, int32_t ahead,
                           int32_t which, double *d_wgt, double *d_logw, uint16_t *d_res, const SlamBatch *batch = nullptr);
void gms_launch_slam_weight_combine(gms_slam *s, int32_t B, const SlamBatch *batch = nullptr);
// resample()'s copies into the generation the draw has just made current, where it drew (epoch[1]); what: bit 0 logData (+ the class
// planes), bit 1 likelihoodData; d_idx_keep (may be NULL) receives the indices for a likelihoodData copy that is still owed
void gms_launch_slam_gather(gms_pf *pf, const SlamBufs &sb, int32_t what, const int32_t *d_idx, int32_t *d_idx_keep, int64_t code_words);
void gms_launch_slam_combine(gms_map *dst, const SlamBufs &sb, int32_t n_filters);   // filter f's particles into map f of dst
// the census of filter `filter`'s maps (gms_census.hip).  count: a workgroup per GMS_CENSUS_TILE cells and GMS_CENSUS_CHUNK particles adds
// `free | occupied << 16` into d_field [cells], which the caller has zeroed; consensus: d_field into the bytes, map f's logData (+-1.0 /
// +0.0) and the totals (zeroed by the caller), each where non-NULL; agree: a workgroup per particle and GMS_CENSUS_AGREE cells adds the
// class pairs into d_agree [n_per][10], zeroed by the caller
#define GMS_CENSUS_TILE 512
#define GMS_CENSUS_CHUNK 32
#define GMS_CENSUS_AGREE 4096
void gms_launch_census_count(gms_map *m, const SlamBufs &sb, int32_t filter, uint32_t *d_field);
void gms_launch_census_consensus(gms_map *m, const uint32_t *d_field, int32_t n, int32_t min_known, uint8_t *d_consensus, double *d_log, gms_census_totals *d_totals);
void gms_launch_census_agree(gms_map *m, const SlamBufs &sb, int32_t filter, const uint8_t *d_consensus, uint32_t *d_agree);
// a view of one particle's map: which >= 0 the particle, which < 0 the strongest of `filter` by d_stats[filter] (picked on the device).
// field: where a likelihood view reads (ignored by a log view) -- SLAM_FIELD_IN_MEMORY the current generation, SLAM_FIELD_OWED_COPY the
// source d_idx_lik names in the other one where the last resample() drew.  d_shown (may be NULL) receives the handle-wide index.
void gms_launch_slam_view(gms_map *m, const SlamBufs &sb, const PfStatsDev *d_stats, int32_t which, int32_t filter, SlamField field,
                          const int32_t *d_idx_lik, const gms_view *v, void *d_out, int32_t *d_shown);
// likelihoodData of that ONE particle from plane 1 of its class planes, into its slot of the current generation (SLAM_FIELD_FROM_PLANES)
void gms_launch_slam_likelihood_shown(gms_map *m, const SlamBufs &sb, const PfStatsDev *d_stats, int32_t which, int32_t filter, int64_t code_words);
void gms_launch_slam_export_records(gms_pf *pf, const SlamBufs &sb, const int32_t *d_list, int32_t count, int64_t code_words, double *d_dst);
void gms_launch_slam_shard_gather(gms_pf *pf, const SlamBufs &sb, const int32_t *d_src_local, const int32_t *d_recv_pos, const double *d_recv, int64_t code_words);

// the particles' paths (gms_slam_set_history): lin := identity and the count 0; a row appended from lin and the poses; a draw composed
// into lin_out (epoch: whether each filter drew); the back-trace -- bundle: every chain of `filter`, d_out [kept][n_per][3], d_anc
// [kept][n_per] or NULL; else the chain of `which` (< 0: the strongest of `filter` by d_stats), d_out [kept][3], d_shown or NULL --
// with `rows` parent rows per LDS buffer (gms_slam_hist_walk_rows; 0: through memory)
void gms_launch_slam_hist_init(gms_map *m, const SlamHist &h, int32_t *d_lin);
void gms_launch_slam_hist_append(gms_map *m, const SlamHist &h, const float *d_pose, int32_t *d_lin);
void gms_launch_slam_hist_compose(gms_map *m, const SlamHist &h, const int32_t *d_lin, int32_t *d_lin_out, const int32_t *d_idx, const int32_t *d_epoch);
int32_t gms_slam_hist_walk_rows(int32_t n_per, int32_t force_mem);
void gms_launch_slam_hist_walk(gms_map *m, const SlamHist &h, const int32_t *d_lin, const PfStatsDev *d_stats, int32_t which, int32_t filter, bool bundle,
                               int32_t kept, int32_t rows, float *d_out, int32_t *d_anc, int32_t *d_shown);

// profiling brackets
void gms_prof_begin(gms_map *m, int32_t k);
void gms_prof_end(gms_map *m);

struct ProfScope {
    gms_map *m;
    bool on;
    ProfScope(gms_map *mm, int32_t k) : m(mm), on(((mm->prof_on >> k) & 1) && (mm->prof_seen[k]++ % mm->prof_stride) == 0) {
        if (on) gms_prof_begin(m, k);
    }
    ~ProfScope() { if (on) gms_prof_end(m); }
};
