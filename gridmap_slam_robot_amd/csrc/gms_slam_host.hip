// gms_slam_host.hip -- C-ABI of the reference's own filter shape: SLAM (J/slam/SLAM.java), every particle with its own GridMapData.
// Handle lifetime and the launch sequences of SLAM.update / SLAM.resample; the kernels are in gms_slam_kernels.hip.  No CPU path.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "gms_internal.h"

SlamBufs gms_slam_bufs(const gms_slam *s) {
    SlamBufs b;
    for (int k = 0; k < 2; k++) { b.log[k] = s->d_log[k]; b.lik[k] = s->d_lik[k]; b.code[k] = s->d_code[k]; }
    b.epoch = s->d_epoch;
    b.n_per = s->n_per;
    return b;
}

// The current generations on the HOST: a stream synchronise and an 8-byte read per filter.  Only where the host itself must address a
// particle's arrays -- downloads, uploads, reset, the copy counter -- never on the update / resample path.  gen [n_filters] (may be
// NULL): filter f's current generation; draws: the draws that ran, summed over the filters' particles (maps copied).
static int slam_host_gen(gms_slam *s, int32_t *gen, int64_t *copies = nullptr) {
    std::vector<int32_t> e((size_t)2 * s->n_filters);
    HIPCHK(hipStreamSynchronize(s->map->stream));
    HIPCHK(hipMemcpy(e.data(), s->d_epoch, e.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t c = 0;
    for (int32_t f = 0; f < s->n_filters; f++) {
        if (gen) gen[f] = e[2 * (size_t)f] & 1;
        c += (int64_t)e[2 * (size_t)f] * s->n_per;
    }
    if (copies) *copies = c;
    return GMS_OK;
}

// What the entry points open with: the null handle, then the kinds of handle the entry does not take (allow: those it does).  A shard
// of a filter has its own calls, since the weights and the sources of its copies may live on other ranks; the calls that take one scan,
// one odometry or one draw for the whole handle are for one filter only.
enum { SLAM_ALLOW_SHARD = 1, SLAM_ALLOW_BATCHED = 2 };
static int slam_enter(const gms_slam *s, const char *what, int allow) {
    if (!s) return gms_fail(GMS_ERR_INVALID, "%s: null handle", what);
    if (!(allow & SLAM_ALLOW_SHARD) && pf_is_shard(s->pf))
        return gms_fail(GMS_ERR_STATE, "%s: a shard of a filter (de-skew, gms_slam_update_local[_dev] and the weight exchange stay with the caller; "
                                       "gms_slam_shard_draw / export / gather move its maps)", what);
    if (!(allow & SLAM_ALLOW_BATCHED) && s->n_filters > 1)
        return gms_fail(GMS_ERR_STATE, "%s: this handle holds %d filters (gms_params.n_maps): use the batch form (gms_slam_update_batch[_dev], "
                                       "gms_slam_resample_maps[_if]_batch, gms_slam_frame_batch)", what, s->n_filters);
    return GMS_OK;
}

// ---- the particles' paths (gridmapslam.h "trajectories") ----
static SlamHist slam_hist(const gms_slam *s) {
    SlamHist h;
    h.parent = s->d_hist_parent; h.pose = s->d_hist_pose; h.steps = s->d_hist_steps;
    h.cap = s->hist_cap; h.n = s->n; h.n_per = s->n_per;
    return h;
}
static void slam_hist_free(gms_slam *s) {
    hipFree(s->d_hist_parent); hipFree(s->d_hist_pose); hipFree(s->d_hist_lin[0]); hipFree(s->d_hist_lin[1]); hipFree(s->d_hist_steps);
    s->d_hist_parent = nullptr; s->d_hist_pose = nullptr; s->d_hist_lin[0] = s->d_hist_lin[1] = nullptr; s->d_hist_steps = nullptr;
    s->hist_cap = 0; s->hist_steps = 0; s->hist_lin_cur = 0;
}
// no row kept, every slot its own source (the capacity stays)
static void slam_hist_clear(gms_slam *s) {
    s->hist_steps = 0; s->hist_lin_cur = 0;
    gms_launch_slam_hist_init(s->map, slam_hist(s), s->d_hist_lin[0]);
}
// what a history of `capacity` rows over n particles allocates: the two planes of the ring, the two lineage arrays, the count and its ticket
static int slam_hist_bytes(int64_t n, int64_t capacity, int64_t *bytes) {
    int64_t rows = 0, ring = 0, all = 0;
    if (__builtin_mul_overflow(n, capacity, &rows) || __builtin_mul_overflow(rows, (int64_t)16, &ring) ||
        __builtin_add_overflow(ring, n * 8 + 16, &all))
        return gms_fail(GMS_ERR_INVALID, "gms_slam_set_history: %lld rows of %lld particles overflow the allocation's size", (long long)capacity, (long long)n);
    *bytes = all;
    return GMS_OK;
}

extern "C" {

int gms_slam_destroy(gms_slam *s) {
    if (!s) return GMS_OK;
    if (s->map) { hipSetDevice(s->map->device); hipStreamSynchronize(s->map->stream); }
    for (int k = 0; k < 2; k++) { hipFree(s->d_log[k]); hipFree(s->d_lik[k]); }
    hipFree(s->d_idx_lik);
    hipFree(s->d_code[0]); hipFree(s->d_code[1]);
    hipFree(s->d_epoch);
    hipFree(s->d_plan);
    hipFree(s->d_batch);
    hipFree(s->d_align_rec);
    hipFree(s->d_census);
    gms_beam_table_free(s->beam); hipFree(s->beam.d_wgt);
    slam_hist_free(s);
    gms_ring_free(s->batch_ring);
    if (s->pf) gms_pf_destroy(s->pf);
    if (s->map) gms_map_destroy(s->map);
    delete s;
    return GMS_OK;
}

static int slam_create(const gms_params *p, int32_t n_particles, int64_t offset, int64_t n_global, gms_slam **out, bool shard_api = false);

int gms_slam_create(const gms_params *p, int32_t n_particles, gms_slam **out) {            // SLAM.java:56-62
    return slam_create(p, n_particles, 0, n_particles, out);
}

// One rank's block [offset, offset + n_local) of a filter of n_global particles with their maps (equal blocks in rank order, multiples
// of GMS_BLOCK): see gridmapslam.h "the reference-shape filter over several GPUs"
int gms_slam_create_shard(const gms_params *p, int32_t n_local, int64_t offset, int64_t n_global, gms_slam **out) {
    REQUIRE(n_global >= 1 && offset >= 0 && offset + n_local <= n_global, "gms_slam_create_shard: the block does not fit the population");
    REQUIRE(n_global == n_local || (n_local % GMS_BLOCK == 0 && offset % n_local == 0 && n_global % n_local == 0),
            "gms_slam_create_shard: equal blocks in rank order, each a multiple of GMS_BLOCK particles (the reductions' blocks must not straddle ranks)");
    return slam_create(p, n_local, offset, n_global, out, true);       // (a "shard" that is the whole population is both: one rank's view of a one-rank group)
}

static int slam_create(const gms_params *p, int32_t n_particles, int64_t offset, int64_t n_global, gms_slam **out, bool shard_api) {
    REQUIRE(p && out, "gms_slam_create: null argument");
    *out = nullptr;
    const bool shard_call = shard_api || offset != 0 || n_global != n_particles;
    if (shard_call) REQUIRE(p->n_maps == 1, "gms_slam_create_shard: gms_params.n_maps must be 1 (a shard holds one block of one filter)");
    REQUIRE(p->n_maps >= 1 && p->n_maps <= 1024, "gms_slam_create: gms_params.n_maps (the number of filters) out of range (1 .. 1024)");
    REQUIRE(n_particles >= 1 && n_particles <= 65535, "gms_slam_create: particle count out of range (1 .. 65535)");
    if ((int64_t)p->n_maps * n_particles > 65535)
        return gms_fail(GMS_ERR_INVALID, "gms_slam_create: %d filters x %d particles exceed the handle's 65535 particles", p->n_maps, n_particles);
    gms_slam *s = new (std::nothrow) gms_slam();
    if (!s) return gms_fail(GMS_ERR_NOMEM, "out of host memory");
    s->n_filters = p->n_maps;
    s->n_per = n_particles;
    s->n = p->n_maps * n_particles;
    int rc = gms_map_create(p, &s->map);                                                   // new GridMap(...) :57
    if (!rc) rc = gms_pf_create(s->map, n_particles, &s->pf);                              // the particle list :59
    if (rc) { gms_slam_destroy(s); return rc; }
    gms_map *m = s->map;
    // the per-particle kernel keeps one row of the count tile at the very least (gms_launch_slam_particle)
    // (per beam: factor 8 B, thresholds 8 B, end-point cell 4 B; slots and ray records 13.3 KB; a class plane of at most 24 KiB)
    if (((size_t)m->max_beams + 8) * 20 + 16384 + 24576 + (size_t)m->gd.W * 4 + 4096 > (size_t)m->lds_per_cu) {
        gms_slam_destroy(s);
        return gms_fail(GMS_ERR_INVALID, "gms_slam_create: %d beams and rows of %d cells do not fit a workgroup's LDS", m->max_beams, m->gd.W);
    }
    const size_t bytes = (size_t)s->n * (size_t)m->gd.cells * sizeof(double);
    const char *lazy_env = getenv("GMS_SLAM_LAZY_LIK_COPY");
    s->lazy_lik = !(lazy_env && lazy_env[0] == '0');
    const char *rl_env = getenv("GMS_SLAM_REFINE_LDS");
    s->refine_lds = rl_env && rl_env[0] == '0' ? 0 : (rl_env && rl_env[0] == '2' ? 2 : -1);
    const char *rf_env = getenv("GMS_SLAM_REFINE_FIELD");
    s->refine_field = rf_env && rf_env[0] == 'c' ? 1 : (rf_env && rf_env[0] == 'l' ? 0 : -1);
    const char *af_env = getenv("GMS_SLAM_ALIGN_FIELD");
    s->align_field = af_env && af_env[0] == 'm' ? 0 : (af_env && af_env[0] == 'p' ? 1 : -1);
    const char *hw_env = getenv("GMS_SLAM_HISTORY_WALK");
    s->hist_walk_mem = hw_env && hw_env[0] == 'm';
    bool ok = true;
    for (int k = 0; k < 2; k++)
        ok = ok && hipMalloc(&s->d_log[k], bytes) == hipSuccess && hipMalloc(&s->d_lik[k], bytes) == hipSuccess;
    ok = ok && hipMalloc(&s->d_idx_lik, (size_t)s->n * sizeof(int32_t)) == hipSuccess;
    const size_t epoch_bytes = (size_t)2 * s->n_filters * sizeof(int32_t);
    ok = ok && hipMalloc(&s->d_epoch, epoch_bytes) == hipSuccess && hipMemset(s->d_epoch, 0, epoch_bytes) == hipSuccess;
    s->pf->slam_owned = 1;          // its particles own maps: resampling goes through gms_slam_resample_maps[_if], which moves them
    // The class planes (gms_slam_kernels.hip): kept unless the blur kernel is wider than the on-demand evaluation takes, a plane would
    // crowd the count tile out of a workgroup's LDS, or GMS_SLAM_EAGER_LIK=1 asks for the reference's own schedule -- every cell of every
    // particle's likelihoodData rebuilt by every update (the like-for-like figure of bench.py)
    const char *eager_env = getenv("GMS_SLAM_EAGER_LIK");
    s->code_words = gms_slam_code_words(m->gd.cells);
    if (!(eager_env && eager_env[0] == '1') && m->gd.khalf <= 7 && s->code_words * 4 <= 24 * 1024 && m->gd.W <= 65535 && m->gd.H <= 65535) {
        const size_t cb = (size_t)s->n * 2 * (size_t)s->code_words * sizeof(uint32_t);
        for (int k = 0; k < 2; k++) ok = ok && hipMalloc(&s->d_code[k], cb) == hipSuccess;
    }
    const bool sharded = shard_call;
    if (sharded) ok = ok && hipMalloc(&s->d_plan, (size_t)3 * n_particles * sizeof(int32_t)) == hipSuccess;
    if (!ok) {
        gms_slam_destroy(s);
        return gms_fail(GMS_ERR_NOMEM, "gms_slam_create: device allocation failed (%d particles x %lld cells x 32 bytes)", s->n, (long long)m->gd.cells);
    }
    if (sharded) {
        if (!s->d_code[0]) {
            gms_slam_destroy(s);
            return gms_fail(GMS_ERR_INVALID, "gms_slam_create_shard: a sharded filter moves a particle as logData + its class planes; this map's planes are "
                                             "not kept (blur kernel wider than 15 taps, a plane over 24 KiB, or GMS_SLAM_EAGER_LIK=1)");
        }
        rc = gms_pf_place_shard(s->pf, offset, n_global);      // (gms_pf_set_shard itself is closed to a filter whose particles own maps)
        if (rc) { gms_slam_destroy(s); return rc; }
    }
    *out = s;
    return gms_slam_reset(s);
}

int gms_slam_reset(gms_slam *s) {                                                           // SLAM.java:65-77
    REQUIRE(s, "null handle");
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    const size_t bytes = (size_t)s->n * (size_t)m->gd.cells * sizeof(double);
    int64_t copies = 0;
    int rc0 = slam_host_gen(s, nullptr, &copies);
    if (rc0) return rc0;
    s->copies_base += copies;                                                                // (the copy counter outlives a reset)
    HIPCHK(hipMemsetAsync(s->d_epoch, 0, (size_t)2 * s->n_filters * sizeof(int32_t), m->stream));   // generation 0 is current again
    // createMapData(null) per particle (GridMap.java:106-117): logData = logOdds(0.5) = 0.0, likelihoodData a fresh double[] = 0.0
    HIPCHK(hipMemsetAsync(s->d_log[0], 0, bytes, m->stream));
    HIPCHK(hipMemsetAsync(s->d_lik[0], 0, bytes, m->stream));
    if (s->d_code[0]) HIPCHK(hipMemsetAsync(s->d_code[0], 0, (size_t)s->n * 2 * (size_t)s->code_words * sizeof(uint32_t), m->stream));   // every class "logData == 0"
    slam_was_reset(s);
    s->have_strongest = 0;                                                                   // (no update yet: nothing names a strongest particle)
    s->have_align_rec = 0;                                                                   // (... and no aligned one: gms_slam_last_align)
    s->shard_moves = 0;                                                                      // (... and no draw whose copies a shard still owes)
    if (s->hist_cap) slam_hist_clear(s);                                                     // (the history starts over, at the same capacity)
    gms_launch_pf_init(s->pf);                                                               // Pose(0, 0, 0), weight 1 / numParticles (:68-71)
    pf_weights_set(s->pf);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

int gms_slam_set_refine(gms_slam *s, int32_t on) {                                          // SLAM.java:96
    REQUIRE(s, "null handle");
    s->refine = on != 0;
    return GMS_OK;
}

int gms_slam_handles(gms_slam *s, gms_map **map, gms_pf **pf) {
    REQUIRE(s, "null handle");
    if (map) *map = s->map;
    if (pf) *pf = s->pf;
    return GMS_OK;
}

int gms_slam_count(const gms_slam *s, int32_t *n, int32_t *W, int32_t *H) {
    REQUIRE(s, "null handle");
    if (n) *n = s->n_per;
    if (W) *W = s->map->gd.W;
    if (H) *H = s->map->gd.H;
    return GMS_OK;
}

static bool slam_skip_update(double d_theta) { return fabs(d_theta) > (3.141592653589793 / 180.0) * 30; }    // SLAM.java:82

// computeLikelihoodMap(p.m) of every particle (SLAM.java:93) into sb.lik's current generation, from logData as it stands
static void slam_write_field(gms_slam *s, const SlamBufs &sb) {
    gms_map *m = s->map;
    // (plane 0 == the classes of logData, 1/32 of the bytes: 623 us against 793 at 4096 x 256^2, where logData is 2 GB; at
    //  500 x 120^2 -- 58 MB, inside the 256 MB infinity cache -- the blur's arithmetic binds and reading logData is 1.6 us FASTER)
    const bool big = (size_t)s->n * (size_t)m->gd.cells * sizeof(double) > ((size_t)256 << 20);
    if (s->d_code[0] && (s->refine_field < 0 ? big : s->refine_field == 1)) gms_launch_slam_likelihood_codes(m, sb, s->code_words, s->n, 0);
    else gms_launch_slam_likelihood(m, sb, s->n);
}

// the per-particle body of SLAM.update(z, u) (SLAM.java:88-107) for the particles this handle holds; the weights stay raw.  batch (may be
// NULL): every filter's own scan, count, odometry, seed and skipUpdate (B: the largest count; motion: the sequence, drawn where the
// filter's table says so)
static int slam_update_core(gms_slam *s, const gms_beam *dev_beams, int32_t B, const MotionModel *motion, bool skip_update, const SlamBatch *batch) {
    gms_map *m = s->map;
    gms_pf *pf = s->pf;
    // :93 for every particle.  With the class planes and no refinement the field is not written here (slam_field_updated; written when
    // asked for: slam_lik_current).  The pose refinement looks up most of a field: it gets all of it.
    // ... unless it computes it itself: a field that fits a workgroup's LDS is computed there from the same plane.
    const bool planes = s->d_code[0] != nullptr;
    // The scan alignment reads four values per beam and evaluation: computed from the same plane where that fits, else the field is written.
    const bool align_planes = s->align_on && gms_slam_align_from_planes(s, B);
    const bool on_demand = planes && (!s->refine || gms_slam_refine_from_planes(m, B, s->refine_lds, s->code_words)) && (!s->align_on || align_planes);
    const SlamBufs sb = gms_slam_bufs(s);
    if (!on_demand) slam_write_field(s, sb);
    slam_field_updated(s, on_demand);
    bool drawn = false;
    if (s->refine) {                                                                                        // :90, then :96 (the lattice form of :97)
        if (!gms_launch_slam_refine(pf, dev_beams, B, sb, motion, s->refine_lds, planes ? s->code_words : 0, batch))
            return gms_fail(GMS_ERR_INVALID, "gms_slam_update_per_particle: the pose refinement's tables do not fit the LDS for a scan of %d beams", B);
        drawn = true;
    }
    if (s->align_on) {                                                                                      // :97's place: from the sample, or the lattice's best pose
        const int rc = gms_launch_slam_align(s, dev_beams, B, sb, align_planes, drawn ? nullptr : motion, &s->align_prm, s->d_align_rec, batch);
        if (rc) return rc;
        s->have_align_rec = 1;
        drawn = true;
    }
    // the beam sensor model (gms_slam_set_beam_model): through the particle's own map as it stands BEFORE this scan goes into it -- behind
    // it every particle would find its own end cell occupied --, at the pose it is weighted at: the sample, the lattice's, the aligned one
    const bool beams = s->beam.on && B > 0;
    if (beams) {
        gms_launch_slam_beams(s, dev_beams, B, sb, drawn ? nullptr : motion, s->beam.behind, s->beam.ahead, 1, s->beam.d_wgt, s->beam.d_wgt + s->n, nullptr, batch);
        drawn = true;
    }
    gms_launch_slam_particle(pf, dev_beams, B, sb, !on_demand, drawn ? nullptr : motion, skip_update ? 0 : 1, s->code_words, batch);   // :90, :99, :102-107
    if (beams) gms_launch_slam_weight_combine(s, B, batch);                                                 // p.weight (:99) times the model's, or the model's
    if (s->hist_cap) {                                                                                      // the poses stand (the normalisation moves none): one row
        gms_launch_slam_hist_append(m, slam_hist(s), pf->d_pose, s->d_hist_lin[s->hist_lin_cur]);
        s->hist_steps++;
    }
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

static int slam_update_local(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                             uint64_t seed, uint64_t sequence) {
    REQUIRE(s && dev_beams, "null argument");
    int rc = slam_enter(s, "gms_slam_update_per_particle / update_local", SLAM_ALLOW_SHARD);
    if (rc) return rc;
    REQUIRE(B >= 0 && B <= s->map->max_beams, "beam count exceeds gms_params.max_beams");
    HIPCHK(hipSetDevice(s->map->device));
    MotionModel mo;
    mo.d_center = d_center; mo.d_theta = d_theta; mo.seed = seed; mo.sequence = sequence;
    return slam_update_core(s, dev_beams, B, sample_motion ? &mo : nullptr, slam_skip_update(d_theta), nullptr);
}

// SLAM.update(z, u) on a device-resident scan (SLAM.java:80-131)
int gms_slam_update_per_particle_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                                     uint64_t seed, uint64_t sequence, gms_pf_stats *stats) {
    int rc = slam_enter(s, "gms_slam_update_per_particle_dev", 0);
    if (rc) return rc;
    rc = slam_update_local(s, dev_beams, B, sample_motion, d_center, d_theta, seed, sequence);
    if (rc) return rc;
    rc = gms_pf_normalize(s->pf, stats);                                                                   // :100, :110-124 (stats: synchronises)
    if (!rc) s->have_strongest = 1;
    return rc;
}

// ... and for one rank's block of a sharded filter: the local half of update() -- motion sample (keyed by the GLOBAL particle index),
// field, weight, map update of this block's particles; weightSum / strongest / normalise / Neff follow from the exchange of the block
// partials (gms_pf_local_partials -> all-reduce -> gms_pf_apply_partials -> all-gather -> gms_pf_import_global), as for a sharded gms_pf
int gms_slam_update_local_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                              uint64_t seed, uint64_t sequence) {
    return slam_update_local(s, dev_beams, B, sample_motion, d_center, d_theta, seed, sequence);
}
int gms_slam_update_local(gms_slam *s, const gms_beam *beams, int32_t B, int32_t sample_motion, double d_center, double d_theta, uint64_t seed,
                          uint64_t sequence) {
    REQUIRE(s && beams, "null argument");
    int rc = slam_enter(s, "gms_slam_update_local", SLAM_ALLOW_SHARD);
    if (rc) return rc;
    rc = gms_stage_beams(s->map, beams, B);
    if (rc) return rc;
    return slam_update_local(s, s->map->d_beams, B, sample_motion, d_center, d_theta, seed, sequence);
}

int gms_slam_update_per_particle(gms_slam *s, const gms_beam *beams, int32_t B, int32_t sample_motion, double d_center, double d_theta,
                                 uint64_t seed, uint64_t sequence, gms_pf_stats *stats) {
    REQUIRE(s && beams, "null argument");
    int rc = slam_enter(s, "gms_slam_update_per_particle", SLAM_ALLOW_SHARD);       // (a shard: refused behind the staging, by the _dev form)
    if (rc) return rc;
    rc = gms_stage_beams(s->map, beams, B);
    if (rc) return rc;
    return gms_slam_update_per_particle_dev(s, s->map->d_beams, B, sample_motion, d_center, d_theta, seed, sequence, stats);
}

// rows x L raw measurements as a frame call lays them into a slot of a pinned ring: [rows][L] angle | [rows][L] distance | [rows][L] hit,
// 17 bytes per measurement; `behind` (slam_raw_bytes): the offset of what follows them (the filters' table), on a 16-byte boundary
static size_t slam_raw_bytes(size_t rows, size_t L) { return (rows * L * 17 + 15) & ~(size_t)15; }
struct RawRows {
    double *angle, *distance;
    uint8_t *hit;
    size_t behind;
};
static RawRows slam_lay_raw(void *slot, size_t rows, size_t L, const double *angle, const double *distance, const uint8_t *hit) {
    const size_t n = rows * L;
    RawRows r;
    r.angle = static_cast<double *>(slot); r.distance = r.angle + n;
    r.hit = reinterpret_cast<uint8_t *>(r.distance + n);
    r.behind = slam_raw_bytes(rows, L);
    memcpy(r.angle, angle, n * 8); memcpy(r.distance, distance, n * 8); memcpy(r.hit, hit, n);
    return r;
}

// the staging of a batched handle, made by its first batched call: d_batch = [S][max_beams] beams | [S] SlamFilterArgs, and the pinned ring
// whose slots hold that block or a frame's raw revolutions with the table behind them (never more than the beams)
static int slam_batch_staging(gms_slam *s, const char *what) {
    if (s->d_batch) return GMS_OK;
    const size_t S = (size_t)s->n_filters, mb = (size_t)s->map->max_beams;
    const size_t bytes = std::max(S * mb * sizeof(gms_beam), slam_raw_bytes(S, mb)) + S * sizeof(SlamFilterArgs);
    if (hipMalloc(&s->d_batch, bytes) != hipSuccess || gms_ring_alloc(s->batch_ring, bytes) != GMS_OK) {
        hipFree(s->d_batch); s->d_batch = nullptr; gms_ring_free(s->batch_ring);
        return gms_fail(GMS_ERR_NOMEM, "%s: staging allocation failed", what);
    }
    return GMS_OK;
}
static SlamFilterArgs *slam_batch_tab(const gms_slam *s) {
    return reinterpret_cast<SlamFilterArgs *>(s->d_batch + (size_t)s->n_filters * s->map->max_beams);
}
// one filter's row of the table: odometry {dCenter, dTheta}
static SlamFilterArgs slam_filter_args(const double *odometry, uint64_t seed, int32_t count, bool sample_motion) {
    SlamFilterArgs a;
    a.d_center = odometry[0]; a.d_theta = odometry[1];
    motion_deviations(a.d_center, a.d_theta, &a.d_center_sd, &a.d_theta_sd);
    a.seed = seed;
    a.count = count;
    a.flags = (sample_motion ? 1 : 0) | (slam_skip_update(a.d_theta) ? 0 : 2);
    return a;
}
// update() of every filter once the table is on its way to slam_batch_tab: filter f's beams at d_beams + f * beam_stride
static int slam_update_staged_batch(gms_slam *s, const gms_beam *d_beams, int32_t beam_stride, int32_t Bmax, uint64_t sequence, gms_pf_stats *stats) {
    SlamBatch bt;
    bt.tab = slam_batch_tab(s); bt.n = s->n_per; bt.beam_stride = beam_stride;
    MotionModel mo;                                    // (the kernels take the odometry and seed from the table; the draw where its flag says so)
    mo.d_center = 0.0; mo.d_theta = 0.0; mo.seed = 0; mo.sequence = sequence;
    int rc = slam_update_core(s, d_beams, Bmax, &mo, false, &bt);
    if (rc) return rc;
    rc = gms_pf_normalize(s->pf, stats);
    if (!rc) s->have_strongest = 1;
    return rc;
}

// SLAM.update(z, u) of every filter of the handle (filter f: beams [f][0 .. counts[f]) of the [S][B] block, odometry [f][2], seeds[f],
// sample_motion[f]; one sequence).  One filter: exactly the scalar call.  Several: one launch of each update kernel for all of them, the
// filters' table (SlamFilterArgs) in the same copy as the beams where those come from the host (on_device: the beams are the caller's)
static int slam_update_batch(gms_slam *s, const gms_beam *beams, bool on_device, int32_t B, const int32_t *counts, const double *odometry,
                             const uint64_t *seeds, const int32_t *sample_motion, uint64_t sequence, gms_pf_stats *stats) {
    REQUIRE(s && beams && odometry && seeds && sample_motion,
            "gms_slam_update_batch: null argument (the handle, beams, odometry, seeds and sample_motion are required)");
    int rc = slam_enter(s, "gms_slam_update_batch", SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    gms_map *m = s->map;
    const int32_t S = s->n_filters;
    if (B < 0 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "gms_slam_update_batch: B = %d outside 0 .. gms_params.max_beams (%d)", B, m->max_beams);
    int32_t Bmax = 0;
    for (int32_t f = 0; f < S; f++) {
        const int32_t c = counts ? counts[f] : B;
        if (c < 0 || c > B) return gms_fail(GMS_ERR_INVALID, "gms_slam_update_batch: counts[%d] = %d outside 0 .. B (%d)", f, c, B);
        Bmax = std::max(Bmax, c);
    }
    HIPCHK(hipSetDevice(m->device));
    if (S == 1) {
        const int32_t c = counts ? counts[0] : B;
        const gms_beam *d = beams;
        if (!on_device) { rc = gms_stage_beams(m, beams, c); d = m->d_beams; }
        if (!rc) rc = gms_slam_update_per_particle_dev(s, d, c, sample_motion[0], odometry[0], odometry[1], seeds[0], sequence, stats);
        return rc;
    }
    rc = slam_batch_staging(s, "gms_slam_update_batch");
    if (rc) return rc;
    std::vector<SlamFilterArgs> tab((size_t)S);
    for (int32_t f = 0; f < S; f++) tab[f] = slam_filter_args(odometry + 2 * (size_t)f, seeds[f], counts ? counts[f] : B, sample_motion[f] != 0);
    SlamFilterArgs *d_tab = slam_batch_tab(s);
    rc = gms_stage_block(m, s->batch_ring, on_device ? nullptr : beams, B, S, m->max_beams, tab.data(), tab.size() * sizeof(SlamFilterArgs),
                         on_device ? static_cast<void *>(d_tab) : static_cast<void *>(s->d_batch));
    if (rc) return rc;
    return slam_update_staged_batch(s, on_device ? beams : s->d_batch, on_device ? B : m->max_beams, Bmax, sequence, stats);
}

int gms_slam_update_batch(gms_slam *s, const gms_beam *beams, int32_t B, const int32_t *counts, const double *odometry, const uint64_t *seeds,
                          const int32_t *sample_motion, uint64_t sequence, gms_pf_stats *stats) {
    return slam_update_batch(s, beams, false, B, counts, odometry, seeds, sample_motion, sequence, stats);
}
int gms_slam_update_batch_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, const int32_t *counts, const double *odometry,
                              const uint64_t *seeds, const int32_t *sample_motion, uint64_t sequence, gms_pf_stats *stats) {
    return slam_update_batch(s, dev_beams, true, B, counts, odometry, seeds, sample_motion, sequence, stats);
}

// likelihoodData as the last resample() left it, for whoever reads it before the next update (downloads; a second resample())
static int slam_lik_current(gms_slam *s) {
    switch (s->field) {
    case SLAM_FIELD_IN_MEMORY: return GMS_OK;
    case SLAM_FIELD_FROM_PLANES:                                                                           // computeLikelihoodMap(p.m) of the last update (:93), late
        gms_launch_slam_likelihood_codes(s->map, gms_slam_bufs(s), s->code_words, s->n, 1);
        break;
    case SLAM_FIELD_OWED_COPY:                                                                             // GridMap.java:121, late (if that resample() drew)
        gms_launch_slam_gather(s->pf, gms_slam_bufs(s), 2, s->d_idx_lik, nullptr, s->code_words);
        break;
    }
    slam_field_materialised(s);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// The draw of resample() over the particles' weights (SLAM.java:136-145 + pose, weight, :42-43; fraction >= 0: where the rule says so).
// The one place that opens the filter to it (refuse_owned_maps): the draw counts itself in the handle's generation pair (k_resample),
// which the maps follow, and the pair is lent for exactly this call.
static int slam_draw(gms_slam *s, const double *r01, double fraction, int32_t *indices, int32_t *n_ambiguous) {
    s->pf->d_epoch2 = s->d_epoch;
    const int rc = fraction >= 0.0 ? gms_pf_resample_if(s->pf, r01, fraction) : gms_pf_resample(s->pf, r01, indices, n_ambiguous);
    s->pf->d_epoch2 = nullptr;
    return rc;
}

// SLAM.resample() (SLAM.java:133-153): the systematic draw over the particles' weights, then every slot's deep copy into the OTHER
// generation of the maps, which the draw makes current (:152); fraction >= 0: only where Neff < fraction * n (GridMapApp.java:185-186),
// decided on the device -- where the rule says no, nothing is drawn, no generation changes and the copy kernels return at once (the
// reference does nothing either).  r01 [n_filters]; a batched handle draws, and decides, per filter (its own generation pair: the
// handle-wide field state holds for every filter, since the copy kernels skip the filters that did not draw)
static int slam_resample(gms_slam *s, const double *r01, double fraction, int32_t *indices, int32_t *n_ambiguous) {
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    int rc = s->field == SLAM_FIELD_OWED_COPY ? slam_lik_current(s) : GMS_OK;                              // (two resample() calls in a row)
    if (rc) return rc;
    rc = slam_draw(s, r01, fraction, indices, n_ambiguous);
    if (rc) return rc;
    if (s->hist_cap) {                                                                                      // the lineage follows the draw, where there was one
        gms_launch_slam_hist_compose(m, slam_hist(s), s->d_hist_lin[s->hist_lin_cur], s->d_hist_lin[s->hist_lin_cur ^ 1], s->pf->d_idx, s->d_epoch);
        s->hist_lin_cur ^= 1;
    }
    const SlamBufs sb = gms_slam_bufs(s);
    slam_resampled(s, s->lazy_lik != 0);
    switch (s->field) {                                                                                     // (what each state copies, and why: slam_resampled)
    case SLAM_FIELD_FROM_PLANES: gms_launch_slam_gather(s->pf, sb, 1, s->pf->d_idx, nullptr, s->code_words); break;
    case SLAM_FIELD_OWED_COPY: gms_launch_slam_gather(s->pf, sb, 1, s->pf->d_idx, s->d_idx_lik, s->code_words); break;   // logData now (GridMap.java:120); keeps the indices
    case SLAM_FIELD_IN_MEMORY: gms_launch_slam_gather(s->pf, sb, 3, s->pf->d_idx, nullptr, s->code_words); break;        // :44
    }
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

int gms_slam_resample_maps(gms_slam *s, double r01, int32_t *indices, int32_t *n_ambiguous) {
    int rc = slam_enter(s, "gms_slam_resample_maps", 0);
    if (rc) return rc;
    return slam_resample(s, &r01, -1.0, indices, n_ambiguous);
}

// resample() of every filter: r01 [S], indices [S][n] filter-local (may be NULL), n_ambiguous [S] (may be NULL)
int gms_slam_resample_maps_batch(gms_slam *s, const double *r01, int32_t *indices, int32_t *n_ambiguous) {
    REQUIRE(s && r01, "gms_slam_resample_maps_batch: null handle or r01");
    int rc = slam_enter(s, "gms_slam_resample_maps_batch", SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    return slam_resample(s, r01, -1.0, indices, n_ambiguous);
}

// ---- resample() of a sharded filter -------------------------------------------------------------------------------------------
// 1. the draw for this rank's slots from the gathered population (every rank: the same r01): poses and weights are filled from it, the
//    maps' generation advances if it drew.  sources[n_local] = the GLOBAL index of every slot's source particle; *did as the rule decided.
int gms_slam_shard_draw(gms_slam *s, double r01, double fraction, int32_t *did, int32_t *sources) {
    REQUIRE(s && did && sources, "null argument");
    int rc = slam_enter(s, "gms_slam_shard_draw", SLAM_ALLOW_SHARD);
    if (rc) return rc;
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    slam_shard_drew(s);
    s->shard_moves = 0;
    rc = slam_draw(s, &r01, fraction, nullptr, nullptr);
    if (rc) return rc;
    int32_t e[2] = {0, 0};
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(e, s->d_epoch, sizeof(e), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sources, s->pf->d_idx, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    *did = e[1];
    s->shard_moves = e[1] != 0;                        // (where the rule said no, no generation changed: there is no "previous" one to move maps from)
    return GMS_OK;
}
// what export and gather open with behind slam_enter: a shard whose last draw drew and has not been gathered yet.  Without one the
// generation pair has not advanced, the kernels' "previous" generation is a stale one and a gather would overwrite the live maps from it
static int slam_shard_moves_open(const gms_slam *s, const char *what) {
    if (!s->d_plan) return gms_fail(GMS_ERR_INVALID, "%s: not a shard", what);
    if (!s->shard_moves)
        return gms_fail(GMS_ERR_STATE, "%s: no draw to move maps for (gms_slam_shard_draw has not run since the last reset, its rule said no, or "
                                       "gms_slam_shard_gather has made that draw's copies already)", what);
    return GMS_OK;
}
// doubles per record of a particle: logData + its two class planes
int gms_slam_record_doubles(const gms_slam *s, int64_t *doubles) {
    REQUIRE(s && doubles, "null argument");
    REQUIRE(s->d_code[0], "gms_slam_record_doubles: the class planes are not kept on this handle");
    *doubles = s->map->gd.cells + s->code_words;
    return GMS_OK;
}
// 2. the records of `count` local particles (indices into this rank's block) as they stood BEFORE the draw, into dev_dst
//    [count][record_doubles]: what the ranks whose slots drew them receive
int gms_slam_shard_export(gms_slam *s, const int32_t *local_indices, int32_t count, double *dev_dst) {
    REQUIRE(s && (count == 0 || (local_indices && dev_dst)), "null argument");
    int rc0 = slam_enter(s, "gms_slam_shard_export", SLAM_ALLOW_SHARD);
    if (rc0) return rc0;
    rc0 = slam_shard_moves_open(s, "gms_slam_shard_export");
    if (rc0) return rc0;
    REQUIRE(count >= 0 && count <= s->n, "gms_slam_shard_export: more records than particles");
    if (count == 0) return GMS_OK;
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    for (int32_t k = 0; k < count; k++) REQUIRE(local_indices[k] >= 0 && local_indices[k] < s->n, "gms_slam_shard_export: particle index out of range");
    HIPCHK(hipMemcpyAsync(s->d_plan, local_indices, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));           // (the host array may be pageable: the copy must not outlive the call)
    gms_launch_slam_export_records(s->pf, gms_slam_bufs(s), s->d_plan, count, s->code_words, dev_dst);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}
// 3. the copies: slot m of the new generation <- local particle src_local[m] of the previous one, or, where src_local[m] < 0, record
//    recv_pos[m] of dev_recv (the records this rank received).  Both arrays [n_local], host.
int gms_slam_shard_gather(gms_slam *s, const int32_t *src_local, const int32_t *recv_pos, const double *dev_recv) {
    REQUIRE(s && src_local && recv_pos, "null argument");
    int rc0 = slam_enter(s, "gms_slam_shard_gather", SLAM_ALLOW_SHARD);
    if (rc0) return rc0;
    rc0 = slam_shard_moves_open(s, "gms_slam_shard_gather");
    if (rc0) return rc0;
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    for (int32_t k = 0; k < s->n; k++) {
        REQUIRE(src_local[k] < s->n, "gms_slam_shard_gather: local source out of range");
        REQUIRE(src_local[k] >= 0 || (dev_recv && recv_pos[k] >= 0), "gms_slam_shard_gather: a remote source without a received record");
    }
    HIPCHK(hipMemcpyAsync(s->d_plan + s->n, src_local, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(s->d_plan + 2 * (size_t)s->n, recv_pos, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    gms_launch_slam_shard_gather(s->pf, gms_slam_bufs(s), s->d_plan + s->n, s->d_plan + 2 * (size_t)s->n, dev_recv, s->code_words);
    s->shard_moves = 0;                                // the draw's copies are made: a second gather (after an update: over the live maps) is refused
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

int gms_slam_resample_maps_if(gms_slam *s, double r01, double fraction) {
    int rc = slam_enter(s, "gms_slam_resample_maps_if", 0);
    if (rc) return rc;
    REQUIRE(fraction >= 0.0, "gms_slam_resample_maps_if: fraction must be non-negative");
    return slam_resample(s, &r01, fraction, nullptr, nullptr);
}

// `if (neff < fraction * n) resample()` for every filter, each decided on the device from its own Neff: r01 [S]
int gms_slam_resample_maps_if_batch(gms_slam *s, const double *r01, double fraction) {
    REQUIRE(s && r01, "gms_slam_resample_maps_if_batch: null handle or r01");
    int rc = slam_enter(s, "gms_slam_resample_maps_if_batch", SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    REQUIRE(fraction >= 0.0, "gms_slam_resample_maps_if_batch: fraction must be non-negative");
    return slam_resample(s, r01, fraction, nullptr, nullptr);
}

// ---- per-particle scan alignment (gridmapslam.h "per-particle scan alignment") ----
// Every particle held, in place, against the field of its own logData as it stands.  Where the values do not come from the class planes
// that field is written first -- into the OTHER generation's likelihoodData, which nothing reads once the current one is written out
// (resample() overwrites every cell of it): what a download returns for likelihoodData stays what it was.
static int slam_align(gms_slam *s, const gms_beam *beams, int32_t B, const gms_align_params *prm, gms_align_record *records, bool on_device) {
    const char *who = on_device ? "gms_slam_align_dev" : "gms_slam_align";
    if (!s || !beams) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle and the beams are required)", who);
    int rc = gms_align_check_for(prm, who);
    if (rc) return rc;
    if (!s->map || !s->pf) return gms_fail(GMS_ERR_INVALID, "%s: not a gms_slam handle", who);
    rc = slam_enter(s, who, SLAM_ALLOW_SHARD);
    if (rc) return rc;
    gms_map *m = s->map;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (on_device && (((uintptr_t)records & 7) != 0 || ((uintptr_t)beams & 7) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the records and the beams must be 8-byte aligned", who);
    HIPCHK(hipSetDevice(m->device));
    const gms_beam *d_beams;
    int32_t beam_stride;
    rc = gms_request_scan(m, beams, B, on_device, &d_beams, &beam_stride);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t rec_bytes = records ? (size_t)s->n * sizeof(gms_align_record) : 0;
    const size_t p_rec = st.part(rec_bytes);
    if (rec_bytes) {
        rc = st.open();
        if (rc) return rc;
    }
    const bool from_planes = gms_slam_align_from_planes(s, B);
    SlamBufs sb = gms_slam_bufs(s);
    if (!from_planes) {
        rc = slam_lik_current(s);
        if (rc) return rc;
        std::swap(sb.lik[0], sb.lik[1]);
        slam_write_field(s, sb);
    }
    rc = gms_launch_slam_align(s, d_beams, B, sb, from_planes, nullptr, prm, records ? st.at(p_rec, records) : nullptr);
    if (rc) return rc;
    pf_particles_changed(s->pf);                                                // the state a gms_pf_set_poses leaves
    if (!rec_bytes) return GMS_OK;
    st.fetch(records, p_rec, rec_bytes);
    return st.finish(nullptr);
}

int gms_slam_align(gms_slam *s, const gms_beam *beams, int32_t B, const gms_align_params *params, gms_align_record *records) {
    return slam_align(s, beams, B, params, records, false);
}
int gms_slam_align_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, const gms_align_params *params, gms_align_record *dev_records) {
    return slam_align(s, dev_beams, B, params, dev_records, true);
}

// update() aligns every particle between computeLikelihoodMap and the weighting (slam_update_core); NULL: off
int gms_slam_set_align(gms_slam *s, const gms_align_params *params) {
    REQUIRE(s, "gms_slam_set_align: null handle");
    int rc = params ? gms_align_check_for(params, "gms_slam_set_align") : GMS_OK;
    if (rc) return rc;
    REQUIRE(s->map && s->pf, "gms_slam_set_align: not a gms_slam handle");
    rc = slam_enter(s, "gms_slam_set_align", SLAM_ALLOW_SHARD | SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    if (!params) { s->align_on = 0; return GMS_OK; }
    if (!s->d_align_rec) {
        HIPCHK(hipSetDevice(s->map->device));
        if (hipMalloc(&s->d_align_rec, (size_t)s->n * sizeof(gms_align_record)) != hipSuccess) {
            s->d_align_rec = nullptr;
            return gms_fail(GMS_ERR_NOMEM, "gms_slam_set_align: device allocation failed (%d records)", s->n);
        }
        s->have_align_rec = 0;
    }
    s->align_prm = *params;
    s->align_on = 1;
    return GMS_OK;
}

// the records [n_filters * n] of the last aligned update.  Synchronises.
int gms_slam_last_align(gms_slam *s, gms_align_record *records) {
    REQUIRE(s && records, "gms_slam_last_align: null argument");
    REQUIRE(s->map && s->pf, "gms_slam_last_align: not a gms_slam handle");
    const int rc = slam_enter(s, "gms_slam_last_align", SLAM_ALLOW_SHARD | SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    if (!s->have_align_rec) return gms_fail(GMS_ERR_STATE, "gms_slam_last_align: no aligned update has run on this handle (gms_slam_set_align)");
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipMemcpyAsync(records, s->d_align_rec, (size_t)s->n * sizeof(gms_align_record), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

// diagnostics: the form the last alignment launch of the handle took (GMS_SLAM_ALIGN_PLANES / _MEMORY; 0: none yet)
int gms_slam_align_form(const gms_slam *s, int32_t *form) {
    REQUIRE(s && form, "gms_slam_align_form: null argument");
    *form = s->align_form;
    return GMS_OK;
}

// ---- the beam sensor model on the particles' own maps (gridmapslam.h "per-particle beam sensor model"; kernels: gms_slam_beams.hip) ----
static int slam_score_beams(gms_slam *s, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals,
                            bool on_device) {
    const char *who = on_device ? "gms_slam_score_beams_dev" : "gms_slam_score_beams";
    if (!s || !beams) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the beams and the factors are required)", who);
    int rc = gms_beam_model_check_for(behind, ahead, factors, who);
    if (rc) return rc;
    if (!s->map || !s->pf) return gms_fail(GMS_ERR_INVALID, "%s: not a gms_slam handle", who);
    rc = slam_enter(s, who, SLAM_ALLOW_SHARD);
    if (rc) return rc;
    gms_map *m = s->map;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (on_device && ((uintptr_t)residuals & 1) != 0) return gms_fail(GMS_ERR_INVALID, "%s: the residuals must be 2-byte aligned", who);
    HIPCHK(hipSetDevice(m->device));
    rc = gms_beam_table_put(m, s->beam, who, behind, ahead, factors, 0, 2);
    if (rc) return rc;
    const gms_beam *d_beams;
    int32_t beam_stride;
    rc = gms_request_scan(m, beams, B, on_device, &d_beams, &beam_stride);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t res_bytes = residuals ? (size_t)s->n * (size_t)B * sizeof(uint16_t) : 0;
    const size_t p_res = st.part(res_bytes);
    if (res_bytes) {
        rc = st.open();
        if (rc) return rc;
    }
    gms_launch_slam_beams(s, d_beams, B, gms_slam_bufs(s), nullptr, behind, ahead, 0, s->pf->d_w, s->pf->d_logw,
                          residuals ? st.at(p_res, residuals) : nullptr);
    HIPCHK(hipGetLastError());
    pf_scored(s->pf, 0);                                                        // raw weights: the state gms_slam_update_local_dev leaves
    if (!res_bytes) return GMS_OK;
    st.fetch(residuals, p_res, res_bytes);
    return st.finish(nullptr);
}

int gms_slam_score_beams(gms_slam *s, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals) {
    return slam_score_beams(s, beams, B, behind, ahead, factors, residuals, false);
}
int gms_slam_score_beams_dev(gms_slam *s, const gms_beam *dev_beams, int32_t B, int32_t behind, int32_t ahead, const double *factors,
                             uint16_t *dev_residuals) {
    return slam_score_beams(s, dev_beams, B, behind, ahead, factors, dev_residuals, true);
}

// update() weighs every particle by the model through its own map, in front of the scan's integration (slam_update_core); factors NULL: off
int gms_slam_set_beam_model(gms_slam *s, int32_t behind, int32_t ahead, const double *factors, int32_t combine) {
    REQUIRE(s, "gms_slam_set_beam_model: null handle");
    int rc = factors ? gms_beam_model_check_for(behind, ahead, factors, "gms_slam_set_beam_model") : GMS_OK;
    if (rc) return rc;
    if (factors && combine != GMS_SLAM_BEAMS_MULTIPLY && combine != GMS_SLAM_BEAMS_REPLACE)
        return gms_fail(GMS_ERR_INVALID, "gms_slam_set_beam_model: combine must be GMS_SLAM_BEAMS_MULTIPLY or GMS_SLAM_BEAMS_REPLACE, not %d", combine);
    REQUIRE(s->map && s->pf, "gms_slam_set_beam_model: not a gms_slam handle");
    rc = slam_enter(s, "gms_slam_set_beam_model", SLAM_ALLOW_SHARD | SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    if (!factors) { s->beam.on = 0; return GMS_OK; }
    HIPCHK(hipSetDevice(s->map->device));
    rc = gms_dev_alloc(&s->beam.d_wgt, (size_t)2 * s->n * sizeof(double), "gms_slam_set_beam_model", "the beam weights");
    if (rc) return rc;
    rc = gms_beam_table_put(s->map, s->beam, "gms_slam_set_beam_model", behind, ahead, factors, 1, 2);
    if (rc) return rc;
    s->beam.behind = behind; s->beam.ahead = ahead; s->beam.combine = combine;
    s->beam.on = 1;
    return GMS_OK;
}

// One recorded revolution as GridMapApp.onHandleData treats it (J/app/GridMapApp.java:133-192) for the filter with a map per particle:
// the de-skew (:143-175), SLAM.update(z, u) (:178) and `if (neff < fraction * n) resample()` (:185-186) as one call -- what
// gms_map_deskew on the handle's map, gms_slam_update_per_particle_dev and gms_slam_resample_maps_if do in three, the same bits.  The raw
// revolution goes into a slot of the map's pinned ring and is read there by the de-skew launch (as gms_map_deskew does).
int gms_slam_frame_per_particle(gms_slam *s, const double *angle, const double *distance, const uint8_t *hit, int32_t length, double d_center,
                                double d_theta, uint64_t seed, uint64_t sequence, double r01, double resample_fraction, gms_pf_stats *stats) {
    REQUIRE(s && angle && distance && hit, "gms_slam_frame_per_particle: null argument (the handle, angle, distance and hit are required)");
    int rc = slam_enter(s, "gms_slam_frame_per_particle", 0);
    if (rc) return rc;
    gms_map *m = s->map;
    if (length <= 0 || length > m->max_beams)
        return gms_fail(GMS_ERR_INVALID, "gms_slam_frame_per_particle: length = %d outside 1 .. gms_params.max_beams (%d)", length, m->max_beams);
    REQUIRE(slam_raw_bytes(1, length) + 16 <= (size_t)m->max_beams * sizeof(gms_beam), "gms_slam_frame_per_particle: scan too long for the staging buffer");
    HIPCHK(hipSetDevice(m->device));
    void *slot = nullptr;
    rc = gms_ring_acquire(m->beam_ring, &slot);
    if (rc) return rc;
    const RawRows raw = slam_lay_raw(slot, 1, length, angle, distance, hit);
    gms_launch_slam_deskew(m, raw.angle, raw.distance, raw.hit, length, 1, length, length, d_center, d_theta, nullptr, nullptr, m->d_beams, m->max_beams);
    rc = gms_ring_commit(m->beam_ring, m->stream);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    s->frame_counts.assign(1, length);
    rc = gms_slam_update_per_particle_dev(s, m->d_beams, length, 1, d_center, d_theta, seed, sequence, stats);      // :178 (stats: synchronises)
    if (!rc && resample_fraction >= 0.0) rc = slam_resample(s, &r01, resample_fraction, nullptr, nullptr);          // :185-186
    return rc;
}

// The same for every filter of a handle: angle / distance / hit [S][L], filter f's revolution its first lengths[f] measurements (NULL:
// all L), de-skewed with its own length and odometry[f] in ONE launch, then gms_slam_update_batch_dev with every filter drawing its
// motion sample and gms_slam_resample_maps_if_batch.  The raw rows and the filters' table share one slot of the pinned ring; the
// de-skew launch reads both in place and carries the table over to the device for the update kernels behind it.
int gms_slam_frame_batch(gms_slam *s, const double *angle, const double *distance, const uint8_t *hit, int32_t L, const int32_t *lengths,
                         const double *odometry, const uint64_t *seeds, uint64_t sequence, const double *r01, double resample_fraction,
                         gms_pf_stats *stats) {
    REQUIRE(s && angle && distance && hit && odometry && seeds && r01,
            "gms_slam_frame_batch: null argument (the handle, angle, distance, hit, odometry, seeds and r01 are required)");
    int rc = slam_enter(s, "gms_slam_frame_batch", SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    gms_map *m = s->map;
    const int32_t S = s->n_filters;
    if (L <= 0 || L > m->max_beams) return gms_fail(GMS_ERR_INVALID, "gms_slam_frame_batch: L = %d outside 1 .. gms_params.max_beams (%d)", L, m->max_beams);
    int32_t Lmax = 0;
    for (int32_t f = 0; f < S; f++) {
        const int32_t c = lengths ? lengths[f] : L;
        if (c < 1 || c > L) return gms_fail(GMS_ERR_INVALID, "gms_slam_frame_batch: lengths[%d] = %d outside 1 .. L (%d)", f, c, L);
        Lmax = std::max(Lmax, c);
    }
    if (S == 1)
        return gms_slam_frame_per_particle(s, angle, distance, hit, Lmax, odometry[0], odometry[1], seeds[0], sequence, r01[0], resample_fraction, stats);
    HIPCHK(hipSetDevice(m->device));
    rc = slam_batch_staging(s, "gms_slam_frame_batch");
    if (rc) return rc;
    void *slot = nullptr;
    rc = gms_ring_acquire(s->batch_ring, &slot);
    if (rc) return rc;
    const RawRows raw = slam_lay_raw(slot, S, L, angle, distance, hit);                // ... | [S] SlamFilterArgs
    SlamFilterArgs *h_tab = reinterpret_cast<SlamFilterArgs *>(static_cast<unsigned char *>(slot) + raw.behind);
    s->frame_counts.resize((size_t)S);
    for (int32_t f = 0; f < S; f++) {
        s->frame_counts[f] = lengths ? lengths[f] : L;
        h_tab[f] = slam_filter_args(odometry + 2 * (size_t)f, seeds[f], s->frame_counts[f], true);
    }
    gms_launch_slam_deskew(m, raw.angle, raw.distance, raw.hit, L, S, Lmax, 0, 0.0, 0.0, h_tab, slam_batch_tab(s), s->d_batch, m->max_beams);
    rc = gms_ring_commit(s->batch_ring, m->stream);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    rc = slam_update_staged_batch(s, s->d_batch, m->max_beams, Lmax, sequence, stats);
    if (!rc && resample_fraction >= 0.0) rc = slam_resample(s, r01, resample_fraction, nullptr, nullptr);
    return rc;
}

// Diagnostics: filter f's de-skewed revolution of the last frame call, out [cap] beams, *count its length.  Holds until the next call
// that stages a scan on this handle.  Synchronises.
int gms_slam_last_beams(gms_slam *s, int32_t f, gms_beam *out, int32_t cap, int32_t *count) {
    REQUIRE(s && out && count, "gms_slam_last_beams: null argument");
    REQUIRE(f >= 0 && f < s->n_filters, "gms_slam_last_beams: filter index out of range");
    if (s->frame_counts.size() != (size_t)s->n_filters) return gms_fail(GMS_ERR_STATE, "gms_slam_last_beams: no frame call has run on this handle");
    const int32_t c = s->frame_counts[(size_t)f];
    REQUIRE(cap >= c, "gms_slam_last_beams: capacity below the revolution's length");
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    const gms_beam *src = s->n_filters == 1 ? m->d_beams : s->d_batch + (size_t)f * m->max_beams;
    HIPCHK(hipMemcpyAsync(out, src, (size_t)c * sizeof(gms_beam), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    *count = c;
    return GMS_OK;
}

// logData and / or likelihoodData (NULL: not that one) of particles [first, first + count), between the host and every filter's current
// generation.  Opens with the device, likelihoodData written out if it is the subject (an upload: the other slots' fields first, then this
// one's over its copy) and the generations; closes when the copies have landed.
static int slam_maps_xfer(gms_slam *s, int32_t first, int32_t count, double *log_data, double *lik, bool to_device) {
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    int rc = lik ? slam_lik_current(s) : GMS_OK;
    std::vector<int32_t> gen((size_t)s->n_filters);
    if (!rc) rc = slam_host_gen(s, gen.data());
    if (rc) return rc;
    const size_t cells = (size_t)m->gd.cells;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    for (int32_t i = first, end; i < first + count; i = end) {                // (every filter from its own current generation)
        const int32_t f = i / s->n_per, cur = gen[(size_t)f];
        end = std::min(first + count, (f + 1) * s->n_per);
        const size_t at = (size_t)i * cells, host_at = (size_t)(i - first) * cells, bytes = (size_t)(end - i) * cells * sizeof(double);
        double *const host[2] = {log_data, lik}, *const dev[2] = {s->d_log[cur], s->d_lik[cur]};
        for (int k = 0; k < 2; k++) {
            if (!host[k]) continue;
            HIPCHK(hipMemcpyAsync(to_device ? dev[k] + at : host[k] + host_at, to_device ? host[k] + host_at : dev[k] + at, bytes, kind, m->stream));
            if (k == 0 && to_device && s->d_code[0])                          // the slots' class plane 0 follows their logData (plane 1, their field's, does not)
                gms_launch_slam_codes_from_log(m, gms_slam_bufs(s), i, end - i, s->code_words);
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

int gms_slam_download_map(gms_slam *s, int32_t i, double *log_data, double *lik) {          // Particle.m (SLAM.java:33)
    REQUIRE(s && i >= 0 && i < s->n, "gms_slam_download_map: particle index out of range");
    return slam_maps_xfer(s, i, 1, log_data, lik, false);
}

int gms_slam_download_maps(gms_slam *s, double *log_all, double *lik_all) {
    REQUIRE(s, "null handle");
    return slam_maps_xfer(s, 0, s->n, log_all, lik_all, false);
}

int gms_slam_upload_map(gms_slam *s, int32_t i, const double *log_data, const double *lik) {
    REQUIRE(s && i >= 0 && i < s->n, "gms_slam_upload_map: particle index out of range");
    return slam_maps_xfer(s, i, 1, const_cast<double *>(log_data), const_cast<double *>(lik), true);
}

// GridMapApp.calculateCombined (J/app/GridMapApp.java:439-458) over the particles' maps, into the handle's own GridMap:
// read it with gms_map_download_log / gms_map_download_likelihood on the map of gms_slam_handles.
int gms_slam_combined(gms_slam *s) {
    REQUIRE(s, "null handle");
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    gms_map_settle(m);
    gms_launch_slam_combine(m, gms_slam_bufs(s), s->n_filters);                               // :441-455 (filter f into map f)
    map_log_replaced(m);
    HIPCHK(hipGetLastError());
    return gms_map_build_likelihood(m);                                                       // :457
}

// ---- the census of the particles' maps (gridmapslam.h; the kernels are gms_census.hip's) ----
static int census_check(const gms_census *c, int32_t n_per, int32_t n_filters, const char *who) {
    if (!c) return gms_fail(GMS_ERR_INVALID, "%s: null request", who);
    if (n_per < 1 || n_per > 65535) return gms_fail(GMS_ERR_INVALID, "%s: %d particles per filter (1 .. 65535: a count is 16 bits)", who, n_per);
    if (n_filters < 1) return gms_fail(GMS_ERR_INVALID, "%s: %d filters", who, n_filters);
    if (c->min_known < 1 || c->min_known > n_per)
        return gms_fail(GMS_ERR_INVALID, "%s: gms_census.min_known must be in 1 .. %d (the particles of a filter), not %d", who, n_per, c->min_known);
    if (c->filter < 0 || c->filter >= n_filters)
        return gms_fail(GMS_ERR_INVALID, "%s: gms_census.filter must be in 0 .. %d, not %d", who, n_filters - 1, c->filter);
    if (c->flags & ~GMS_CENSUS_WRITE_MAP) return gms_fail(GMS_ERR_INVALID, "%s: gms_census.flags holds bits other than GMS_CENSUS_WRITE_MAP", who);
    if (c->reserved != 0) return gms_fail(GMS_ERR_INVALID, "%s: gms_census.reserved must be 0", who);
    return GMS_OK;
}

// The checks first, nothing touched.  Then the handle's own map settled where it is written, the field zeroed and counted, the pass
// over the field where anything but the counts is asked for, the pass over the maps where the records are.
static int slam_census(gms_slam *s, const gms_census *c, uint16_t *counts, uint8_t *consensus, uint32_t *agree, gms_census_totals *totals, bool on_device,
                       const char *who) {
    int rc = slam_enter(s, who, SLAM_ALLOW_BATCHED);
    if (rc) return rc;
    rc = census_check(c, s->n_per, s->n_filters, who);
    if (rc) return rc;
    const bool write_map = (c->flags & GMS_CENSUS_WRITE_MAP) != 0;
    if (!counts && !consensus && !agree && !totals && !write_map)
        return gms_fail(GMS_ERR_INVALID, "%s: nothing asked for (every output NULL and no GMS_CENSUS_WRITE_MAP)", who);
    if (on_device && ((((uintptr_t)counts | (uintptr_t)agree) & 3) != 0 || ((uintptr_t)totals & 7) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: counts and agree must be 4-byte aligned, totals 8-byte aligned", who);
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    const size_t cells = (size_t)m->gd.cells;
    rc = gms_dev_alloc(&s->d_census, cells * 5, who, "the count field and the consensus bytes");
    if (rc) return rc;
    if (write_map) gms_map_settle(m);                                                          // what gms_map_upload_log opens with
    const size_t agree_bytes = agree ? (size_t)s->n_per * 10 * sizeof(uint32_t) : 0;
    HostStage st(m, on_device);
    const size_t p_counts = st.part(counts ? cells * 4 : 0), p_cons = st.part(consensus ? cells : 0), p_agree = st.part(agree_bytes),
                 p_totals = st.part(totals ? sizeof(gms_census_totals) : 0);
    rc = st.open();
    if (rc) return rc;
    // the field is the caller's counts where they are asked for: {fr, oc} as uint16 pairs ARE the little-endian count words
    uint32_t *d_field = counts ? reinterpret_cast<uint32_t *>(st.at(p_counts, counts)) : s->d_census;
    uint8_t *d_cons = consensus ? st.at(p_cons, consensus) : agree ? reinterpret_cast<uint8_t *>(s->d_census + cells) : nullptr;
    uint32_t *d_agree = agree ? st.at(p_agree, agree) : nullptr;
    gms_census_totals *d_totals = totals ? st.at(p_totals, totals) : nullptr;
    const SlamBufs sb = gms_slam_bufs(s);
    HIPCHK(hipMemsetAsync(d_field, 0, cells * 4, m->stream));
    gms_launch_census_count(m, sb, c->filter, d_field);
    if (d_cons || d_totals || write_map) {
        if (d_totals) HIPCHK(hipMemsetAsync(d_totals, 0, sizeof(gms_census_totals), m->stream));
        gms_launch_census_consensus(m, d_field, s->n_per, c->min_known, d_cons, write_map ? m->d_log + (size_t)c->filter * cells : nullptr, d_totals);
    }
    if (d_agree) {
        HIPCHK(hipMemsetAsync(d_agree, 0, agree_bytes, m->stream));
        gms_launch_census_agree(m, sb, c->filter, d_cons, d_agree);
    }
    HIPCHK(hipGetLastError());
    if (write_map) map_log_replaced(m);
    if (counts) st.fetch(counts, p_counts, cells * 4);
    if (consensus) st.fetch(consensus, p_cons, cells);
    if (agree) st.fetch(agree, p_agree, agree_bytes);
    if (totals) st.fetch(totals, p_totals, sizeof(gms_census_totals));
    return st.finish(nullptr);
}

int gms_census_check(const gms_census *c, int32_t n_per, int32_t n_filters) { return census_check(c, n_per, n_filters, "gms_census_check"); }
int gms_census_geometry(int32_t *tile_cells, int32_t *chunk_particles, int32_t *agree_cells) {
    if (tile_cells) *tile_cells = GMS_CENSUS_TILE;
    if (chunk_particles) *chunk_particles = GMS_CENSUS_CHUNK;
    if (agree_cells) *agree_cells = GMS_CENSUS_AGREE;
    return GMS_OK;
}
int gms_slam_census(gms_slam *s, const gms_census *c, uint16_t *counts, uint8_t *consensus, uint32_t *agree, gms_census_totals *totals) {
    return slam_census(s, c, counts, consensus, agree, totals, false, "gms_slam_census");
}
int gms_slam_census_dev(gms_slam *s, const gms_census *c, uint16_t *dev_counts, uint8_t *dev_consensus, uint32_t *dev_agree, gms_census_totals *dev_totals) {
    return slam_census(s, c, dev_counts, dev_consensus, dev_agree, dev_totals, true, "gms_slam_census_dev");
}

// A view of one particle's map (gridmapslam.h "map views"): GridMapApp.render's "strongest" and "chosen" cases (GridMapApp.java:374-393)
// handed to GridMap.render (GridMap.java:371-388), on the device.  The strongest particle and the maps' current generation are read
// there; the host decides only what it knows without a round trip: where the fields stand (gms_slam::field).
static int slam_view(gms_slam *s, int32_t which, const gms_view *v, void *out, int32_t *shown, bool on_device) {
    REQUIRE(s && v && out, "gms_slam_view: null argument (the handle, the view and the output are required)");
    gms_map *m = s->map;
    int64_t bytes = 0;
    int rc = gms_view_check(v, m->gd.W, m->gd.H, "gms_slam_view", &bytes);
    if (rc) return rc;
    REQUIRE(!on_device || v->format != GMS_VIEW_PACKED32 || ((uintptr_t)out & 3) == 0, "gms_slam_view_dev: a packed view needs a 4-byte aligned output");
    int32_t filter = 0;
    rc = gms_slam_shown(s, which, v->filter, "gms_slam_view", "gms_view.filter", &filter);
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    const SlamBufs sb = gms_slam_bufs(s);
    SlamField field = s->field;
    if (v->source == GMS_VIEW_LIKELIHOOD && field == SLAM_FIELD_FROM_PLANES) {       // the shown particle's field alone; the state stays as it is
        gms_launch_slam_likelihood_shown(m, sb, s->pf->d_stats, which, filter, s->code_words);
        field = SLAM_FIELD_IN_MEMORY;
    }
    HostStage st(m, on_device);
    const size_t p_out = st.part((size_t)bytes);
    rc = st.open();
    if (rc) return rc;
    gms_launch_slam_view(m, sb, s->pf->d_stats, which, filter, field, s->d_idx_lik, v, st.at(p_out, out), st.shown(shown));
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, (size_t)bytes);
    return st.finish(shown);
}
int gms_slam_view(gms_slam *s, int32_t which, const gms_view *v, void *out, int32_t *shown) { return slam_view(s, which, v, out, shown, false); }
int gms_slam_view_dev(gms_slam *s, int32_t which, const gms_view *v, void *dev_out, int32_t *dev_shown) { return slam_view(s, which, v, dev_out, dev_shown, true); }

// The cell walk of SLAM.update's integrateObservation(p.m, z, p.pose) for particle i at its current pose, as k_slam_particle walks and
// classifies it, written out instead of counted (tests): gms_map_trace_scan's layout.
int gms_slam_trace_scan(gms_slam *s, int32_t i, const gms_beam *beams, int32_t B, int32_t *cells_xy, uint8_t *classes, int32_t cap, int32_t *counts) {
    REQUIRE(s && beams && counts, "null argument");
    REQUIRE(i >= 0 && i < s->n, "gms_slam_trace_scan: particle index out of range");
    REQUIRE(B >= 0 && B <= s->map->max_beams && cap >= 0, "gms_slam_trace_scan: beam count or capacity out of range");
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    int rc = GMS_OK;
    if (s->n_filters == 1) rc = gms_stage_beams(m, beams, B);
    else HIPCHK(hipMemcpyAsync(m->d_beams, beams, (size_t)B * sizeof(gms_beam), hipMemcpyHostToDevice, m->stream));   // (one scan: the map stages S)
    if (rc) return rc;
    int32_t *d_cells = nullptr, *d_counts = nullptr;
    uint8_t *d_cls = nullptr;
    const size_t n = (size_t)B * (size_t)cap;
    bool ok = hipMalloc(&d_cells, (n ? n : 1) * 2 * sizeof(int32_t)) == hipSuccess && hipMalloc(&d_cls, n ? n : 1) == hipSuccess &&
              hipMalloc(&d_counts, (size_t)(B ? B : 1) * sizeof(int32_t)) == hipSuccess;
    if (ok) {
        gms_launch_slam_trace(s->pf, m->d_beams, B, i, d_cells, d_cls, cap, d_counts);
        ok = hipGetLastError() == hipSuccess;
        if (ok && B) ok = hipMemcpyAsync(counts, d_counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream) == hipSuccess;
        if (ok && n && cells_xy) ok = hipMemcpyAsync(cells_xy, d_cells, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream) == hipSuccess;
        if (ok && n && classes) ok = hipMemcpyAsync(classes, d_cls, n, hipMemcpyDeviceToHost, m->stream) == hipSuccess;
        ok = hipStreamSynchronize(m->stream) == hipSuccess && ok;
    }
    hipFree(d_cells); hipFree(d_cls); hipFree(d_counts);
    if (!ok) return gms_fail(GMS_ERR_HIP, "gms_slam_trace_scan: device allocation, launch or copy failed");
    return GMS_OK;
}

// ---- trajectories (gridmapslam.h): the ring is written by slam_update_core and slam_resample; these calls only read it ----
int gms_slam_history_bytes(int32_t n_particles_total, int32_t capacity, int64_t *bytes) {
    REQUIRE(bytes, "gms_slam_history_bytes: null argument");
    REQUIRE(n_particles_total >= 1 && capacity >= 0, "gms_slam_history_bytes: the particle count must be positive and the capacity non-negative");
    if (capacity == 0) { *bytes = 0; return GMS_OK; }
    return slam_hist_bytes(n_particles_total, capacity, bytes);
}

int gms_slam_set_history(gms_slam *s, int32_t capacity) {
    REQUIRE(s, "gms_slam_set_history: null handle");
    if (pf_is_shard(s->pf))
        return gms_fail(GMS_ERR_STATE, "gms_slam_set_history: a shard of a filter (a particle's ancestors cross ranks)");
    REQUIRE(capacity >= 0, "gms_slam_set_history: negative capacity");
    int64_t bytes = 0;
    if (capacity > 0) { int rc = slam_hist_bytes(s->n, capacity, &bytes); if (rc) return rc; }
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    if (s->hist_cap) HIPCHK(hipStreamSynchronize(m->stream));                                // (launches in flight still write the old ring)
    slam_hist_free(s);
    if (capacity == 0) return GMS_OK;
    const size_t slots = (size_t)capacity * (size_t)s->n;
    const bool ok = hipMalloc(&s->d_hist_parent, slots * sizeof(int32_t)) == hipSuccess && hipMalloc(&s->d_hist_pose, slots * 3 * sizeof(float)) == hipSuccess &&
                    hipMalloc(&s->d_hist_lin[0], (size_t)s->n * sizeof(int32_t)) == hipSuccess &&
                    hipMalloc(&s->d_hist_lin[1], (size_t)s->n * sizeof(int32_t)) == hipSuccess && hipMalloc(&s->d_hist_steps, 2 * sizeof(int64_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        slam_hist_free(s);
        return gms_fail(GMS_ERR_NOMEM, "gms_slam_set_history: device allocation of %lld bytes failed", (long long)bytes);
    }
    s->hist_cap = capacity;
    slam_hist_clear(s);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

int gms_slam_history_len(gms_slam *s, int64_t *steps_total, int32_t *steps_kept) {
    REQUIRE(s, "gms_slam_history_len: null handle");
    if (!s->hist_cap) return gms_fail(GMS_ERR_STATE, "gms_slam_history_len: the history is off (gms_slam_set_history)");
    if (steps_total) *steps_total = s->hist_steps;
    if (steps_kept) *steps_kept = (int32_t)std::min<int64_t>(s->hist_steps, s->hist_cap);
    return GMS_OK;
}

int gms_slam_history_walk_rows(gms_slam *s, int32_t *rows) {
    REQUIRE(s && rows, "gms_slam_history_walk_rows: null argument");
    *rows = gms_slam_hist_walk_rows(s->n_per, s->hist_walk_mem);
    return GMS_OK;
}

// one chain (bundle false: `which`, or the strongest of `filter`) or all of `filter`'s, into host or device memory
static int slam_trajectory(gms_slam *s, const char *what, bool bundle, int32_t which, int32_t filter, float *xytheta, int32_t *ancestors, int32_t cap,
                           int32_t *count, int32_t *shown, bool on_device) {
    if (!s) return gms_fail(GMS_ERR_INVALID, "%s: null handle", what);
    if (!s->hist_cap) return gms_fail(GMS_ERR_STATE, "%s: the history is off (gms_slam_set_history)", what);
    if (bundle) {
        if (filter < 0 || filter >= s->n_filters) return gms_fail(GMS_ERR_INVALID, "%s: filter out of range", what);
    } else {
        int rc = gms_slam_shown(s, which, filter, what, "filter", &filter);
        if (rc) return rc;
    }
    const int32_t kept = (int32_t)std::min<int64_t>(s->hist_steps, s->hist_cap);
    if (count) *count = kept;
    if (cap < kept) return gms_fail(GMS_ERR_INVALID, "%s: room for %d steps, %d are kept", what, cap, kept);
    if (kept == 0) return GMS_OK;
    if (!xytheta) return gms_fail(GMS_ERR_INVALID, "%s: null output", what);
    gms_map *m = s->map;
    HIPCHK(hipSetDevice(m->device));
    const int32_t nch = bundle ? s->n_per : 1;
    const size_t pose_bytes = (size_t)kept * nch * 3 * sizeof(float), anc_bytes = ancestors ? (size_t)kept * nch * sizeof(int32_t) : 0;
    HostStage st(m, on_device);
    const size_t p_out = st.part(pose_bytes), p_anc = st.part(anc_bytes);
    int rc = st.open();
    if (rc) return rc;
    gms_launch_slam_hist_walk(m, slam_hist(s), s->d_hist_lin[s->hist_lin_cur], s->pf->d_stats, which, filter, bundle, kept,
                              gms_slam_hist_walk_rows(s->n_per, s->hist_walk_mem), st.at(p_out, xytheta), ancestors ? st.at(p_anc, ancestors) : nullptr,
                              bundle ? nullptr : st.shown(shown));
    HIPCHK(hipGetLastError());
    st.fetch(xytheta, p_out, pose_bytes);
    st.fetch(ancestors, p_anc, anc_bytes);
    return st.finish(bundle ? nullptr : shown);
}

int gms_slam_trajectory(gms_slam *s, int32_t which, int32_t filter, float *xytheta, int32_t cap, int32_t *count, int32_t *shown) {
    return slam_trajectory(s, "gms_slam_trajectory", false, which, filter, xytheta, nullptr, cap, count, shown, false);
}
int gms_slam_trajectory_dev(gms_slam *s, int32_t which, int32_t filter, float *dev_xytheta, int32_t cap, int32_t *dev_shown) {
    return slam_trajectory(s, "gms_slam_trajectory_dev", false, which, filter, dev_xytheta, nullptr, cap, nullptr, dev_shown, true);
}
int gms_slam_trajectories(gms_slam *s, int32_t filter, float *xytheta, int32_t *ancestors, int32_t cap, int32_t *count) {
    return slam_trajectory(s, "gms_slam_trajectories", true, 0, filter, xytheta, ancestors, cap, count, nullptr, false);
}

int gms_slam_copies(const gms_slam *s, int64_t *maps_copied) {
    REQUIRE(s && maps_copied, "null argument");
    int64_t copies = 0;
    gms_slam *sm = const_cast<gms_slam *>(s);
    HIPCHK(hipSetDevice(sm->map->device));
    int rc = slam_host_gen(sm, nullptr, &copies);              // (the draws are counted on the device: a conditional resample() may not have run)
    if (rc) return rc;
    *maps_copied = s->copies_base + copies;
    return GMS_OK;
}

}  // extern "C"
