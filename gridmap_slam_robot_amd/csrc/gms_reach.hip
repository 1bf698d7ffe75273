// gms_reach.hip -- cost-to-go fields (gridmapslam.h "cost-to-go fields"): the cost of the cheapest 8-connected path, axis step 5, diagonal
// step 7, no corner cutting, from a set of seed cells to every cell of the map through the cells that are not blocked, capped at
// max_cost.  All integer arithmetic; the field is unique, so however the relaxation is scheduled the result is the same.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the blocked plane   one bit per cell in the casts' layout (rows of 64-bit words, the padding zero).  inflate == 0: the casts' plane
//                       or the map's second plane, read in place (query_plane; a gms_slam's: the shown particle's, packed per request).
//                       inflate > 0: k_clear_field over the whole map at R = inflate into d_reach_d2, then k_reach_block ballots
//                       d2 != FAR into d_reach_plane, a wavefront per 64 cells.
//   k_reach_init        the working field all FAR, the control words and the tiles' flags zero.
//   k_reach_seeds       a lane per seed: on the map and not blocked -> cost 0, and the tiles of the cell and of its eight neighbours active
//                       (relax_mark_around: a seed never changes, so it marks by itself).  A gms_slam without seeds: the shown particle's
//                       own cell, from its pose on the device.
//   k_reach_round       ONE ROUND of the tile relaxation on the uint16 field: relax_round<ReachCells> of gms_relax_device.h, which holds the
//                       scheme, its proof, the sweeps and the LDS banks' argument.
//   k_reach_copy        the rectangle out of the working field.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_relax_device.h"

#define RCH_T RLX_T                      // tile edge in cells = cells of a plane word
#define RCH_FAR ReachCells::FAR
#define RCH_CTL_WORDS ReachCells::CTL_WORDS                                     // d_reach_ctl: [0..1] tile runs, [2..5] active counts, [6..7] spare; the flags behind them

static_assert(GMS_REACH_FAR == RCH_FAR && GMS_REACH_AXIS == 5 && GMS_REACH_DIAG == 7, "the header's constants are the kernels'");

// inflate > 0: the blocked plane from the clearance field d2 of the whole map (the planes' layout and ballot, gms_device.h)
__global__ void __launch_bounds__(256)
k_reach_block(const uint16_t *__restrict__ d2, int32_t W, int32_t wpr64, uint64_t *__restrict__ plane) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t wx = plane_wave_word(), y = (int32_t)blockIdx.y;
    if (wx >= wpr64) return;                                                    // (uniform per wavefront)
    const int32_t x = wx * 64 + lane;
    const uint32_t v = x < W ? d2[(size_t)y * (size_t)W + (size_t)x] : RCH_FAR;                   // (padding: not blocked, as the planes have it)
    plane_pack_word(plane, (size_t)y * (size_t)wpr64 + (size_t)wx, v != RCH_FAR);
}

// field: words32 32-bit words; ctl: ctl_words
__global__ void __launch_bounds__(256)
k_reach_init(uint32_t *__restrict__ field, int64_t words32, uint32_t *__restrict__ ctl, int32_t ctl_words) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < words32; i += step) field[i] = 0xffffffffu;
    for (int64_t i = i0; i < ctl_words; i += step) ctl[i] = 0u;
}

// seeds [K][2] (x, y), or -- seeds NULL -- the cell of particle `which` (>= 0, or the strongest of `filter` by the last update's
// statistics, as k_slam_plane picks it) under its pose
__global__ void __launch_bounds__(256)
k_reach_seeds(GridDev g, uint16_t *__restrict__ field, const uint64_t *__restrict__ plane, int32_t wpr64, int32_t ntx, uint32_t *__restrict__ ctl,
              const int32_t *__restrict__ seeds, int32_t K, const PfStatsDev *__restrict__ stats, int32_t which, int32_t filter, int32_t n_per,
              const float *__restrict__ pose) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    int32_t gx, gy;
    if (seeds) {
        if (i >= K) return;
        gx = seeds[2 * (size_t)i];
        gy = seeds[2 * (size_t)i + 1];
    } else {
        if (i != 0) return;
        const int32_t p = which >= 0 ? which : filter * n_per + stats[filter].strongest;
        gx = j_cell_exact((double)pose[3 * (size_t)p] - g.posx, g.res);                         // GridMap.java:273
        gy = j_cell_exact((double)pose[3 * (size_t)p + 1] - g.posy, g.res);                     // :274
    }
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) return;
    if ((plane[(size_t)gy * (size_t)wpr64 + (size_t)(gx >> 6)] >> (gx & 63)) & 1ull) return;
    field[(size_t)gy * (size_t)g.W + (size_t)gx] = 0;
    relax_mark_around(ctl + RCH_CTL_WORDS, ctl + 2, gx, gy, g.W, g.H, ntx);
}

// field [H][W]; plane: ONE map's, H rows of wpr64 words; grid (ntx, nty), a wavefront per tile; ctl as d_reach_ctl
__global__ void __launch_bounds__(RCH_T)
k_reach_round(uint16_t *field, const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *ctl, int32_t round, uint32_t max_cost) {
    __shared__ uint16_t s[RLX_ROWS * ReachCells::PITCH];
    relax_round<ReachCells>(s, field, plane, wpr64, W, H, ctl, round, ReachCells::Params{max_cost});
}

// out [h][w]
__global__ void __launch_bounds__(256)
k_reach_copy(const uint16_t *__restrict__ field, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h, uint16_t *__restrict__ out) {
    const int64_t n = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t y = (int32_t)(i / w), x = (int32_t)(i - (int64_t)y * w);
        out[i] = field[(size_t)(y0 + y) * (size_t)W + (size_t)(x0 + x)];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// what a field needs on the handle (a handle's W and H never change, so nothing ever has to grow)
static int reach_buffers(gms_map *m, bool inflated) {
    const size_t cells = (size_t)m->gd.cells, ntiles = (size_t)((m->gd.W + RCH_T - 1) / RCH_T) * (size_t)((m->gd.H + RCH_T - 1) / RCH_T);
    int rc = gms_dev_alloc(&m->d_reach_field, ((cells + 1) & ~(size_t)1) * sizeof(uint16_t), "gms_reach", "the working field");
    if (!rc) rc = gms_dev_alloc(&m->d_reach_ctl, (RCH_CTL_WORDS + 2 * ntiles) * sizeof(uint32_t), "gms_reach", "the tiles' flags");
    // (inflate > 0: the clearance field and the blocked plane are gms_reach_inflate's)
    if (!rc) rc = gms_pinned_alloc(&m->h_reach_ctl, RCH_CTL_WORDS * sizeof(uint32_t), "gms_reach");
    return rc;
}

// inflate > 0: the blocked plane of ONE map's obstacle plane -- "clearance at R = inflate, balloted" -- in d_reach_plane
int gms_reach_inflate(gms_map *m, const uint32_t *d_obstacles, int32_t inflate, int32_t mode, const uint32_t **d_blocked) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64;
    int rc = gms_dev_alloc(&m->d_reach_d2, (size_t)m->gd.cells * sizeof(uint16_t), "gms_reach", "the inflation's clearance field");
    if (!rc) rc = gms_dev_alloc(&m->d_reach_plane, (size_t)H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), "gms_reach", "the blocked plane");
    if (rc) return rc;
    const gms_clearance c = {0, 0, W, H, inflate, mode, 0};
    rc = gms_clear_launch(m, d_obstacles, &c, m->d_reach_d2);
    if (rc) return rc;
    hipLaunchKernelGGL(k_reach_block, dim3((unsigned)((wpr64 + 3) / 4), (unsigned)H), dim3(256), 0, m->stream, m->d_reach_d2, W, wpr64,
                       reinterpret_cast<uint64_t *>(m->d_reach_plane));
    HIPCHK(hipGetLastError());
    *d_blocked = m->d_reach_plane;
    return GMS_OK;
}

// who plants the seeds: a list on the device, or (seeds NULL) the shown particle of a gms_slam
struct ReachSeeds {
    const int32_t *d_seeds;
    int32_t K;
    const PfStatsDev *stats;
    int32_t which, filter, n_per;
    const float *pose;
};

// the field of ONE map's obstacle plane (already of logData as it stands) into d_out; the handle's buffers exist
static int reach_run(gms_map *m, const uint32_t *d_obstacles, const gms_reach *r, const ReachSeeds &sd, uint16_t *d_out) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64, ntx = (W + RCH_T - 1) / RCH_T, nty = (H + RCH_T - 1) / RCH_T;
    if (nty > 65535) return gms_fail(GMS_ERR_INVALID, "gms_reach: a map of %d rows exceeds one launch", H);
    const uint32_t *d_blocked = d_obstacles;
    if (r->inflate > 0) {
        int rc = gms_reach_inflate(m, d_obstacles, r->inflate, r->mode, &d_blocked);
        if (rc) return rc;
    }
    const uint64_t *plane = reinterpret_cast<const uint64_t *>(d_blocked);
    const int64_t words32 = (m->gd.cells + 1) / 2;
    const int32_t ctl_words = RCH_CTL_WORDS + 2 * ntx * nty;
    hipLaunchKernelGGL(k_reach_init, dim3((unsigned)std::min<int64_t>(2048, (words32 + 255) / 256)), dim3(256), 0, m->stream,
                       reinterpret_cast<uint32_t *>(m->d_reach_field), words32, m->d_reach_ctl, ctl_words);
    HIPCHK(hipGetLastError());
    const int32_t n_seeds = sd.d_seeds ? sd.K : 1;
    hipLaunchKernelGGL(k_reach_seeds, dim3((unsigned)((n_seeds + 255) / 256)), dim3(256), 0, m->stream, m->gd, m->d_reach_field, plane, wpr64, ntx, m->d_reach_ctl,
                       sd.d_seeds, sd.K, sd.stats, sd.which, sd.filter, sd.n_per, sd.pose);
    HIPCHK(hipGetLastError());
    m->reach_rounds = 0;
    m->reach_tile_runs = 0;
    const auto round = [&](int32_t k) {
        hipLaunchKernelGGL(k_reach_round, dim3((unsigned)ntx, (unsigned)nty), dim3(RCH_T), 0, m->stream, m->d_reach_field, plane, wpr64, W, H, m->d_reach_ctl, k,
                           (uint32_t)r->max_cost);
    };
    const int rc = relax_rounds(m->stream, m->d_reach_ctl, m->h_reach_ctl, RCH_CTL_WORDS, r->max_cost, relax_batch("GMS_REACH_BATCH"), round, "gms_reach",
                                &m->reach_rounds, &m->reach_tile_runs);
    if (rc) return rc;
    const int64_t n = (int64_t)r->w * r->h;
    hipLaunchKernelGGL(k_reach_copy, dim3((unsigned)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0, m->stream, m->d_reach_field, W, r->x0, r->y0, r->w, r->h,
                       d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the field of one map of a shared handle (seeds required) or of the shown particle of a per-particle one (K == 0 and no seeds: its own
// cell); `shown` exists for a particle only
static int reach(QuerySource src, const char *what, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !r || !out || (!src.s && !seeds))
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the output and -- for a map -- the seeds are required)", what);
    gms_map *m = src.m;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (rc) return rc;
    if (!((seeds && K >= 1 && K <= GMS_REACH_MAX_SEEDS) || (src.s && K == 0 && !seeds)))
        return gms_fail(GMS_ERR_INVALID, "%s: 1 <= K <= GMS_REACH_MAX_SEEDS seeds%s", what, src.s ? ", or K = 0 and no seeds (the shown particle's own cell)" : "");
    int64_t bytes = 0;
    rc = gms_reach_size(r, nullptr, nullptr, &bytes);
    if (!rc) rc = gms_rect_check(r->x0, r->y0, r->w, r->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if (on_device && (((uintptr_t)out & 1) != 0 || ((uintptr_t)seeds & 3) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s_dev: the output must be 2-byte aligned, the seeds 4-byte aligned", what);
    src.filter = r->filter;
    if (src.s && (rc = query_check(src, what, "gms_reach.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    rc = reach_buffers(m, r->inflate > 0);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t seed_bytes = (size_t)K * 2 * sizeof(int32_t), p_out = st.part((size_t)bytes), p_seeds = st.part(seed_bytes);
    rc = st.open();
    if (!rc && seeds) rc = st.up(p_seeds, seeds, seed_bytes);
    if (rc) return rc;
    ReachSeeds sd = {seeds ? st.at(p_seeds, seeds) : nullptr, K, nullptr, 0, 0, 0, nullptr};
    if (src.s) sd = {sd.d_seeds, K, src.s->pf->d_stats, src.index, src.filter, src.s->n_per, src.s->pf->d_pose};
    const uint32_t *plane = nullptr;
    rc = query_plane(src, r->mode, st.shown(shown), nullptr, &plane);
    if (!rc) rc = reach_run(m, plane, r, sd, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, (size_t)bytes);
    return st.finish(shown);
}

extern "C" {

int gms_reach_size(const gms_reach *r, int32_t *out_w, int32_t *out_h, int64_t *bytes) {
    REQUIRE(r, "gms_reach: null request");
    REQUIRE(r->w >= 1 && r->h >= 1, "gms_reach: w and h must be at least 1");
    REQUIRE(r->x0 >= 0 && r->y0 >= 0, "gms_reach: x0 and y0 must not be negative");
    REQUIRE(r->max_cost >= 1 && r->max_cost <= 0xFFFE, "gms_reach: 1 <= max_cost <= 0xFFFE");
    REQUIRE(r->inflate >= 0 && r->inflate <= 255, "gms_reach: 0 <= inflate <= 255 cells");
    REQUIRE(r->mode == GMS_CLEAR_OCCUPIED || r->mode == GMS_CLEAR_NOT_FREE, "gms_reach: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    if (out_w) *out_w = r->w;
    if (out_h) *out_h = r->h;
    if (bytes) *bytes = (int64_t)r->w * r->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_reach(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out) { return reach(query_map(m, mi), "gms_map_reach", r, seeds, K, out, nullptr, false); }
int gms_map_reach_dev(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out) {
    return reach(query_map(m, mi), "gms_map_reach", r, dev_seeds, K, dev_out, nullptr, true);
}
int gms_slam_reach(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out, int32_t *shown) {
    return reach(query_slam(s, which), "gms_slam_reach", r, seeds, K, out, shown, false);
}
int gms_slam_reach_dev(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out, int32_t *dev_shown) {
    return reach(query_slam(s, which), "gms_slam_reach", r, dev_seeds, K, dev_out, dev_shown, true);
}
int gms_map_reach_stats(const gms_map *m, int32_t *rounds, int64_t *tile_runs) {
    REQUIRE(m, "gms_map_reach_stats: null handle");
    if (rounds) *rounds = m->reach_rounds;
    if (tile_runs) *tile_runs = m->reach_tile_runs;
    return GMS_OK;
}

}  // extern "C"
