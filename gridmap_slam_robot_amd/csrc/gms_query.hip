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
//   the scan       gms_launch_scan (gms_internal.h): the exclusive scan of uint32 counts that frontier regions, pose modes and particle
//                  seeding number their roots, kept records and eligible cells with.  k_scan_blocks: a workgroup of 256 lanes per
//                  GMS_SCAN items, four per lane, an inclusive scan by shuffles inside each wavefront and the four wavefronts' sums
//                  through LDS -- one barrier; k_scan_top: ONE workgroup per batch entry walks the blocks' totals with the same body,
//                  GMS_SCAN at a time, the carry in a register.
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

// The scan's block body: the workgroup's GMS_SCAN items v[base ..], four per lane, become carry + the sum of those before them; items
// behind n count as 0 and are neither read nor written.  Returns the sum of the GMS_SCAN items, in every lane.  s_wave: 4 words of LDS
__device__ __forceinline__ uint32_t scan_block(uint32_t *__restrict__ v, int64_t base, int64_t n, uint32_t carry, uint32_t *s_wave) {
    const int32_t t = (int32_t)threadIdx.x, lane = t & 63;
    const int64_t at = base + t * 4;
    uint32_t c[4], mine = 0u;
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
        c[k] = at + k < n ? v[at + k] : 0u;
        mine += c[k];
    }
    uint32_t inc = mine;                                                        // the inclusive scan within the wavefront
#pragma unroll
    for (int32_t off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= off) inc += up;
    }
    if (lane == 63) s_wave[t >> 6] = inc;
    __syncthreads();
    const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
    uint32_t run = carry + inc - mine + (t >= 64 ? w0 : 0u) + (t >= 128 ? w1 : 0u) + (t >= 192 ? w2 : 0u);
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
        if (at + k < n) v[at + k] = run;
        run += c[k];
    }
    return w0 + w1 + w2 + w3;
}
static_assert(GMS_SCAN == 4 * 256, "scan_block: 256 lanes, four items each");

// grid (blocks, batch): entry blockIdx.y's items at vals + y * stride, its blocks' totals into sums + y * sum_stride (gms_launch_scan)
__global__ void __launch_bounds__(256)
k_scan_blocks(uint32_t *__restrict__ vals, const uint32_t *__restrict__ n_dev, int64_t n_cap, int64_t stride, uint32_t *__restrict__ sums, int64_t sum_stride) {
    __shared__ uint32_t s_wave[4];
    const int64_t n = n_dev ? (*n_dev < n_cap ? (int64_t)*n_dev : n_cap) : n_cap;
    const uint32_t sum = scan_block(vals + (size_t)blockIdx.y * (size_t)stride, (int64_t)blockIdx.x * GMS_SCAN, n, 0u, s_wave);
    if (threadIdx.x == 0) sums[(size_t)blockIdx.y * (size_t)sum_stride + blockIdx.x] = sum;
}
// grid (1, batch), ONE workgroup per entry: its nb totals -> their exclusive prefix in place, the sum of all into total[blockIdx.y]
__global__ void __launch_bounds__(256)
k_scan_top(uint32_t *__restrict__ sums, int64_t nb, int64_t sum_stride, uint32_t *__restrict__ total) {
    __shared__ uint32_t s_wave[4];
    uint32_t *__restrict__ v = sums + (size_t)blockIdx.y * (size_t)sum_stride;
    uint32_t carry = 0u;
    for (int64_t base = 0; base < nb; base += GMS_SCAN) {
        carry += scan_block(v, base, nb, carry, s_wave);
        __syncthreads();                                                        // (the next round writes s_wave again)
    }
    if (threadIdx.x == 0) total[blockIdx.y] = carry;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
void gms_launch_scan(hipStream_t st, uint32_t *vals, const uint32_t *n_dev, int64_t n_cap, uint32_t *sums, uint32_t *total, int32_t batch, int64_t stride,
                     int64_t sum_stride) {
    const int64_t nb = (n_cap + GMS_SCAN - 1) / GMS_SCAN;
    hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)nb, (unsigned)batch), dim3(256), 0, st, vals, n_dev, n_cap, stride, sums, sum_stride);
    hipLaunchKernelGGL(k_scan_top, dim3(1, (unsigned)batch), dim3(256), 0, st, sums, nb, sum_stride, total);
}

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
    int rc = gms_dev_grow(&m->d_view, &m->view_cap, (int64_t)(16 + bytes), 65536, &m->stream, [](size_t c) { return c; }, "gms_view", "the host forms' staging");
    *base = m->d_view;
    return rc;
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
