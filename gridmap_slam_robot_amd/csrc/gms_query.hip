// gms_query.hip -- what the map queries share (gms_internal.h "map queries"): the request checks, the map's and the particles' bit
// planes, the host forms' staging and the source a query reads.  The feature units (gms_cast.hip, gms_clearance.hip, gms_reach.hip,
// gms_frontier.hip; the views in gms_host.hip / gms_slam_host.hip) keep their kernels, their launch arithmetic and their own checks.
//
// A translation unit of its own: nothing here is on the scan step's path, and no kernel of the other units is compiled differently
// for it.
//
//   the planes     one bit per cell, rows of gms_plane_wpr 32-bit words (padded to 64 cells).  A shared map keeps one per mode on the
//                  handle until logData moves (map_planes_stale): k_map_plane packs logData > 0 (GMS_CLEAR_OCCUPIED, the padding not
//                  occupied: the plane the casts walk) or !(logData < 0) (GMS_CLEAR_NOT_FREE, the padding free), a wavefront's ballot over
//                  64 consecutive cells being one 64-bit word; 2048 x 2048 cells: 512 KB, cache-resident.  The per-particle filter keeps
//                  none: k_slam_plane packs the SHOWN particle's -- from plane 0 of its class planes (code 2 occupied, code 1 free), or
//                  from logData where the handle keeps no planes -- into a scratch plane of the handle; particle and generation are
//                  picked there, on the device.
#undef GMS_STAMPS
#include "gms_device.h"

template <int MODE>
__global__ void __launch_bounds__(256)
k_map_plane(const double *__restrict__ logd, int32_t W, int32_t H, int64_t cells, int32_t wpr64, uint64_t *__restrict__ plane) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t wx = plane_wave_word(), y = (int32_t)blockIdx.y, mi = (int32_t)blockIdx.z;
    if (wx >= wpr64) return;                                                    // (uniform per wavefront)
    const int32_t x = wx * 64 + lane;
    const double v = x < W ? logd[(size_t)mi * (size_t)cells + (size_t)y * (size_t)W + (size_t)x] : (MODE == GMS_CLEAR_OCCUPIED ? 0.0 : -1.0);
    // GridMap.java:239: NaN, 0 and -0.0 are not occupied; not free: occupied, never observed, or NaN
    plane_pack_word(plane, ((size_t)mi * (size_t)H + (size_t)y) * (size_t)wpr64 + (size_t)wx, MODE == GMS_CLEAR_OCCUPIED ? v > 0.0 : !(v < 0.0));
}

// the shown particle's plane under `mode`: which >= 0 that particle, GMS_VIEW_STRONGEST the strongest of `filter` by the last update's
// statistics (as k_cast_slam picks it); the generation from the epoch counters
template <bool CODES>
__global__ void __launch_bounds__(256)
k_slam_plane(GridDev g, SlamBufs sb, int64_t code_words, const PfStatsDev *__restrict__ stats, int32_t which, int32_t filter, int32_t mode,
             int32_t wpr64, uint64_t *__restrict__ plane, int32_t *__restrict__ shown) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t wx = plane_wave_word(), y = (int32_t)blockIdx.y;
    const int32_t p = which >= 0 ? which : filter * sb.n_per + stats[filter].strongest;
    if (shown && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *shown = p;
    if (wx >= wpr64) return;                                                    // (uniform per wavefront)
    const int32_t cur = sb.epoch[2 * (p / sb.n_per)] & 1;                       // the current generation of the particle's filter
    const int32_t x = wx * 64 + lane;
    bool obstacle = false;
    if (x < g.W) {
        if (CODES) {
            const uint32_t *__restrict__ codes = (cur ? sb.code[1] : sb.code[0]) + (size_t)p * 2 * (size_t)code_words;     // plane 0: logData as it stands
            const int32_t c = x + y * g.W;
            const uint32_t code = (codes[c >> 4] >> (2 * (c & 15))) & 3u;       // 0: logData == 0 or NaN, 1: < 0, 2: > 0
            obstacle = mode == GMS_CLEAR_OCCUPIED ? code == 2u : code != 1u;
        } else {
            const double v = ((cur ? sb.log[1] : sb.log[0]) + (size_t)p * (size_t)g.cells)[(size_t)x + (size_t)y * (size_t)g.W];
            obstacle = mode == GMS_CLEAR_OCCUPIED ? v > 0.0 : !(v < 0.0);
        }
    }
    plane_pack_word(plane, (size_t)y * (size_t)wpr64 + (size_t)wx, obstacle);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int gms_rect_check(int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t W, int32_t H, const char *what) {
    if ((int64_t)x0 + w > W || (int64_t)y0 + h > H)
        return gms_fail(GMS_ERR_INVALID, "%s: the rectangle (%d, %d) + %d x %d leaves the map's %d x %d cells", what, x0, y0, w, h, W, H);
    return GMS_OK;
}

int gms_view_check(const gms_view *v, int32_t W, int32_t H, const char *what, int64_t *bytes) {
    int rc = gms_view_size(v, nullptr, nullptr, bytes);
    return rc ? rc : gms_rect_check(v->x0, v->y0, v->w, v->h, W, H, what);
}

int gms_slam_shown(const gms_slam *s, int32_t which, int32_t filter, const char *what, const char *filter_name, int32_t *filter_out) {
    *filter_out = 0;
    if (which != GMS_VIEW_STRONGEST) {
        if (which < 0 || which >= s->n) return gms_fail(GMS_ERR_INVALID, "%s: particle index out of range", what);
        return GMS_OK;
    }
    if (filter < 0 || filter >= s->n_filters) return gms_fail(GMS_ERR_INVALID, "%s: %s out of range", what, filter_name);
    if (pf_is_shard(s->pf)) return gms_fail(GMS_ERR_STATE, "%s: a shard of a filter (its strongest particle may live on another rank): name the particle", what);
    if (!s->have_strongest) return gms_fail(GMS_ERR_STATE, "%s: no update since the handle was created or reset: there is no strongest particle yet", what);
    *filter_out = filter;
    return GMS_OK;
}

int gms_map_plane(gms_map *m, int32_t mode, const uint32_t **plane) {
    gms_flush_apply(m);
    auto &pl = m->plane[mode];
    const int32_t wpr64 = (m->gd.W + 63) / 64;
    int rc = gms_dev_alloc(&pl.d, (size_t)m->n_maps * (size_t)m->gd.H * (size_t)wpr64 * sizeof(uint64_t), "gms_map_plane",
                           mode == GMS_CLEAR_OCCUPIED ? "the occupied bit plane" : "the not-free bit plane");
    if (rc) return rc;
    if (!pl.current) {
        const dim3 grid((unsigned)((wpr64 + 3) / 4), (unsigned)m->gd.H, (unsigned)m->n_maps);
        uint64_t *dst = reinterpret_cast<uint64_t *>(pl.d);
        if (mode == GMS_CLEAR_OCCUPIED)
            hipLaunchKernelGGL((k_map_plane<GMS_CLEAR_OCCUPIED>), grid, dim3(256), 0, m->stream, m->d_log, m->gd.W, m->gd.H, m->gd.cells, wpr64, dst);
        else
            hipLaunchKernelGGL((k_map_plane<GMS_CLEAR_NOT_FREE>), grid, dim3(256), 0, m->stream, m->d_log, m->gd.W, m->gd.H, m->gd.cells, wpr64, dst);
        HIPCHK(hipGetLastError());
        pl.current = 1;
        if (mode == GMS_CLEAR_OCCUPIED) m->cast_plane_builds++;
    }
    *plane = pl.d;
    return GMS_OK;
}

int gms_slam_plane(gms_slam *s, int32_t which, int32_t filter, int32_t mode, int32_t *d_shown, uint32_t *d_dst) {
    gms_map *m = s->map;
    const int32_t wpr64 = (m->gd.W + 63) / 64;
    if (!d_dst) {
        int rc = gms_dev_alloc(&m->d_clear_scratch, (size_t)m->gd.H * (size_t)wpr64 * sizeof(uint64_t), "gms_slam_plane", "the particle's bit plane");
        if (rc) return rc;
    }
    const SlamBufs sb = gms_slam_bufs(s);
    uint64_t *dst = reinterpret_cast<uint64_t *>(d_dst ? d_dst : m->d_clear_scratch);
    const dim3 grid((unsigned)((wpr64 + 3) / 4), (unsigned)m->gd.H);
    if (s->d_code[0])
        hipLaunchKernelGGL((k_slam_plane<true>), grid, dim3(256), 0, m->stream, m->gd, sb, s->code_words, s->pf->d_stats, which, filter, mode, wpr64, dst, d_shown);
    else
        hipLaunchKernelGGL((k_slam_plane<false>), grid, dim3(256), 0, m->stream, m->gd, sb, s->code_words, s->pf->d_stats, which, filter, mode, wpr64, dst, d_shown);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// The host forms' device staging: 16 bytes for the shown index, `bytes` behind them.  Kept on the handle and only ever grown (a stream
// synchronise, then a larger allocation), so a sequence of requests of one size allocates once
static int gms_view_staging(gms_map *m, size_t bytes, unsigned char **base) {
    const size_t need = 16 + bytes;
    if (m->view_cap < need) {
        HIPCHK(hipStreamSynchronize(m->stream));
        hipFree(m->d_view); m->d_view = nullptr; m->view_cap = 0;
        const size_t cap = (need + 65535) & ~(size_t)65535;
        int rc = gms_dev_alloc(&m->d_view, cap, "gms_view", "the host forms' staging");
        if (rc) return rc;
        m->view_cap = cap;
    }
    *base = m->d_view;
    return GMS_OK;
}
int HostStage::open() { return on_device ? GMS_OK : gms_view_staging(m, total, &base); }
int HostStage::up(size_t part, const void *src, size_t bytes) {
    if (!on_device) HIPCHK(hipMemcpyAsync(base + part, src, bytes, hipMemcpyHostToDevice, m->stream));
    return GMS_OK;
}
int HostStage::finish(int32_t *shown) {
    if (on_device) return GMS_OK;
    for (int32_t i = 0; i < n_out; i++)
        if (out[i].bytes) HIPCHK(hipMemcpyAsync(out[i].dst, base + out[i].part, out[i].bytes, hipMemcpyDeviceToHost, m->stream));
    if (shown) HIPCHK(hipMemcpyAsync(shown, base, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

int query_check(QuerySource &src, const char *what, const char *filter_name) {
    if (src.s) return gms_slam_shown(src.s, src.index, src.filter, what, filter_name, &src.filter);
    if (src.index < 0 || src.index >= src.m->n_maps) return gms_fail(GMS_ERR_INVALID, "%s: map index out of range", what);
    return GMS_OK;
}

int query_plane(const QuerySource &src, int32_t mode, int32_t *d_shown, uint32_t *d_dst, const uint32_t **plane) {
    gms_map *m = src.m;
    if (src.s) {
        int rc = gms_slam_plane(src.s, src.index, src.filter, mode, d_shown, d_dst);
        *plane = d_dst ? d_dst : m->d_clear_scratch;
        return rc;
    }
    int rc = gms_map_plane(m, mode, plane);
    if (!rc) *plane += (size_t)src.index * (size_t)m->gd.H * (size_t)gms_plane_wpr(m);
    return rc;
}
