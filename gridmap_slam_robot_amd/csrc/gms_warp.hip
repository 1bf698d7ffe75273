// gms_warp.hip -- maps under a rigid transform (gridmapslam.h "map warps"): one map's logData read through a pose and compared with,
// copied into, added to or filled into a rectangle of another map's, with the class-pair counts a caller accepts or rejects the pose
// by.  Kernel and C-ABI; a translation unit of its own: nothing here is on the scan step's path.
//
//   the launch     grid (ceil(w / 64), ceil(h / 64)), 256 lanes: a workgroup takes a tile of 64 x 64 cells of the rectangle, a
//                  wavefront a row of 64 consecutive destination cells at a time (rows wave, wave + 4, ...: sixteen of them), so the
//                  destination load and store are one coalesced 512-byte segment each.  The source cell is gathered directly: a rotated
//                  row of 64 cells crosses a handful of 128-byte lines, and the rows next to it find them in L2.
//   the counts     nine ballots (destination class x source class) and one for the cells without a source cell per row, their
//                  population counts summed in wave-uniform registers over the wavefront's rows, the four wavefronts' sums combined
//                  through LDS, one 64-bit integer atomic add per non-zero counter and workgroup: integers, so the order is immaterial.
//   the source     a map of a gms_map handle, or a particle of a gms_slam: particle and generation are picked on the device from the
//                  statistics and the epoch counters, as k_slam_plane picks them; every particle's logData is kept as doubles.
#include <math.h>

#include "gms_internal.h"

// the request as the kernel sees it: both grids' geometry widened once on the host, the pose, the rectangle
struct WarpDev {
    double pxd, pyd, rd;            // destination: (double) position.x / .y, resolution
    double pxs, pys, rs;            // source
    double tx, ty, c, s, clamp;
    int32_t Wd, x0, y0, w, h;       // destination row pitch and the rectangle
    int32_t Ws, Hs;
};
// where the source's logData is: src (a shared map's), or -- sb.n_per > 0 -- the shown particle's slab of a gms_slam
struct WarpSource {
    const double *src;
    SlamBufs sb;
    const PfStatsDev *stats;
    int32_t which, filter;
};

__device__ __forceinline__ int32_t warp_class(double l) { return l > 0.0 ? 2 : l < 0.0 ? 1 : 0; }        // NaN, 0 and -0.0: unknown

template <int OP, bool SLAM>
__global__ void __launch_bounds__(256)
k_warp(WarpDev g, double *__restrict__ dst, WarpSource from, int64_t src_cells, unsigned long long *__restrict__ stats_out, int32_t *__restrict__ shown) {
    __shared__ uint32_t s_cnt[4][10];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *__restrict__ src = from.src;
    if (SLAM) {
        const int32_t p = from.which >= 0 ? from.which : from.filter * from.sb.n_per + from.stats[from.filter].strongest;
        if (shown && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *shown = p;
        const int32_t cur = from.sb.epoch[2 * (p / from.sb.n_per)] & 1;                 // the current generation of the particle's filter
        src = (cur ? from.sb.log[1] : from.sb.log[0]) + (size_t)p * (size_t)src_cells;
    }
    const bool count = stats_out != nullptr;
    const bool read_d = count || OP == GMS_WARP_ADD || OP == GMS_WARP_FILL;
    const int32_t rx = (int32_t)blockIdx.x * 64 + lane;                                // the cell within the rectangle
    const int32_t x = g.x0 + rx;
    const double cx = g.pxd + ((double)x + 0.5) * g.rd;
    const double dx = cx - g.tx;
    uint32_t cnt[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int32_t r = wave; r < 64; r += 4) {
        const int32_t ry = (int32_t)blockIdx.y * 64 + r;
        if (ry >= g.h) break;                                                           // (uniform per wavefront)
        const int32_t y = g.y0 + ry;
        const bool valid = rx < g.w;
        const double cy = g.pyd + ((double)y + 0.5) * g.rd;
        const double dy = cy - g.ty;
        const double u = g.c * dx + g.s * dy, v = g.c * dy - g.s * dx;                  // the centre in the source's world
        const double qx = floor((u - g.pxs) / g.rs), qy = floor((v - g.pys) / g.rs);
        const bool inside = valid && qx >= 0.0 && qx < (double)g.Ws && qy >= 0.0 && qy < (double)g.Hs;     // compared as doubles: NaN fails
        const size_t at = (size_t)y * (size_t)g.Wd + (size_t)x;
        unsigned long long vb = 0ull, db = 0ull;
        if (inside) vb = reinterpret_cast<const unsigned long long *>(src)[(size_t)(int32_t)qy * (size_t)g.Ws + (size_t)(int32_t)qx];
        if (read_d && valid) db = reinterpret_cast<const unsigned long long *>(dst)[at];
        const double sv = __longlong_as_double((long long)vb), dv = __longlong_as_double((long long)db);
        const int32_t cs = warp_class(sv), cd = warp_class(dv);
        if (count) {
#pragma unroll
            for (int32_t k = 0; k < 9; k++) cnt[k] += (uint32_t)__popcll(__ballot(inside && cd == k / 3 && cs == k % 3));
            cnt[9] += (uint32_t)__popcll(__ballot(valid && !inside));
        }
        if (OP == GMS_WARP_REPLACE) {
            if (inside) reinterpret_cast<unsigned long long *>(dst)[at] = vb;           // bit for bit
        } else if (OP == GMS_WARP_ADD) {
            if (inside && cs != 0 && !(dv != dv)) {                                     // an unknown source cell changes nothing; a NaN stays
                double sum = dv + sv;
                if (g.clamp > 0.0) {
                    if (sum > g.clamp) sum = g.clamp;
                    if (sum < -g.clamp) sum = -g.clamp;
                }
                dst[at] = sum;
            }
        } else if (OP == GMS_WARP_FILL) {
            if (inside && cd == 0 && cs != 0) reinterpret_cast<unsigned long long *>(dst)[at] = vb;
        }
    }
    if (!count) return;                                                                 // (uniform per launch)
    if (lane == 0) {
#pragma unroll
        for (int32_t k = 0; k < 10; k++) s_cnt[wave][k] = cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const uint32_t sum = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (sum) atomicAdd(stats_out + threadIdx.x, (unsigned long long)sum);
    }
}
static_assert(sizeof(gms_warp_stats) == 10 * sizeof(unsigned long long), "k_warp adds into pair[3][3] and n_outside as ten 64-bit counters");

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int warp_check(const gms_warp *w, const char *who) {
    if (!w) return gms_fail(GMS_ERR_INVALID, "%s: null request", who);
    if (w->op != GMS_WARP_COMPARE && w->op != GMS_WARP_REPLACE && w->op != GMS_WARP_ADD && w->op != GMS_WARP_FILL)
        return gms_fail(GMS_ERR_INVALID, "%s: gms_warp.op must be GMS_WARP_COMPARE, _REPLACE, _ADD or _FILL", who);
    if (!isfinite(w->tx) || !isfinite(w->ty)) return gms_fail(GMS_ERR_INVALID, "%s: gms_warp.tx and ty must be finite", who);
    if (!isfinite(w->c) || !isfinite(w->s)) return gms_fail(GMS_ERR_INVALID, "%s: gms_warp.c and s must be finite", who);
    if (!isfinite(w->clamp) || w->clamp < 0.0) return gms_fail(GMS_ERR_INVALID, "%s: gms_warp.clamp must be finite and >= 0 (0: no clamp)", who);
    if (!(fabs(w->c * w->c + w->s * w->s - 1.0) <= 1e-6))
        return gms_fail(GMS_ERR_INVALID, "%s: gms_warp.c and s must be a cosine and a sine: |c*c + s*s - 1| <= 1e-6", who);
    if (w->x0 < 0 || w->y0 < 0 || w->w < 1 || w->h < 1)
        return gms_fail(GMS_ERR_INVALID, "%s: the rectangle needs x0, y0 >= 0 and w, h >= 1", who);
    return GMS_OK;
}

template <bool SLAM>
static void warp_launch_op(gms_map *dst, const WarpDev &g, double *d_dst, const WarpSource &from, int64_t src_cells, int32_t op, unsigned long long *d_stats,
                           int32_t *d_shown) {
    const dim3 grid((unsigned)((g.w + 63) / 64), (unsigned)((g.h + 63) / 64));
    switch (op) {
    case GMS_WARP_COMPARE: hipLaunchKernelGGL((k_warp<GMS_WARP_COMPARE, SLAM>), grid, dim3(256), 0, dst->stream, g, d_dst, from, src_cells, d_stats, d_shown); break;
    case GMS_WARP_REPLACE: hipLaunchKernelGGL((k_warp<GMS_WARP_REPLACE, SLAM>), grid, dim3(256), 0, dst->stream, g, d_dst, from, src_cells, d_stats, d_shown); break;
    case GMS_WARP_ADD: hipLaunchKernelGGL((k_warp<GMS_WARP_ADD, SLAM>), grid, dim3(256), 0, dst->stream, g, d_dst, from, src_cells, d_stats, d_shown); break;
    default: hipLaunchKernelGGL((k_warp<GMS_WARP_FILL, SLAM>), grid, dim3(256), 0, dst->stream, g, d_dst, from, src_cells, d_stats, d_shown); break;
    }
}

// Map mi_src of src (s NULL), or the shown particle of s (src then its map handle: the geometry and the stream), through w into map
// mi_dst of dst.  The checks first, nothing touched; then both sides settled, the two streams ordered in both directions by events,
// and the destination left as an upload of the result would leave it.
static int warp(gms_map *dst, int32_t mi_dst, gms_map *src, int32_t mi_src, gms_slam *s, int32_t which, int32_t filter, const gms_warp *w, gms_warp_stats *stats,
                int32_t *shown, bool on_device, const char *who) {
    if (!dst || !src) return gms_fail(GMS_ERR_INVALID, "%s: null handle", who);
    int rc = warp_check(w, who);
    if (rc) return rc;
    if (mi_dst < 0 || mi_dst >= dst->n_maps) return gms_fail(GMS_ERR_INVALID, "%s: destination map index out of range", who);
    if (s) {
        if (dst == src) return gms_fail(GMS_ERR_INVALID, "%s: the destination is the gms_slam's own map handle", who);
        rc = gms_slam_shown(s, which, filter, who, "filter", &filter);
        if (rc) return rc;
    } else {
        if (mi_src < 0 || mi_src >= src->n_maps) return gms_fail(GMS_ERR_INVALID, "%s: source map index out of range", who);
        if (dst == src && mi_dst == mi_src) return gms_fail(GMS_ERR_INVALID, "%s: source and destination are the same map", who);
    }
    rc = gms_rect_check(w->x0, w->y0, w->w, w->h, dst->gd.W, dst->gd.H, who);
    if (rc) return rc;
    if (dst->device != src->device) return gms_fail(GMS_ERR_INVALID, "%s: both handles must live on the same device", who);
    if (on_device && ((uintptr_t)stats & 7) != 0) return gms_fail(GMS_ERR_INVALID, "%s: the statistics must be 8-byte aligned", who);
    HIPCHK(hipSetDevice(dst->device));
    const bool writes = w->op != GMS_WARP_COMPARE;
    // the source as a download would return it: a shared map's deferred apply pass first (a particle's logData is never behind)
    if (!s) gms_flush_apply(src);
    // the destination: what gms_map_upload_log opens with where it is written, what gms_map_download_log opens with where it is only read
    if (writes) gms_map_settle(dst);
    else gms_flush_apply(dst);
    HostStage st(dst, on_device);
    const size_t p_stats = st.part(stats ? sizeof(gms_warp_stats) : 0);
    rc = st.open();
    if (rc) return rc;
    unsigned long long *d_stats = stats ? reinterpret_cast<unsigned long long *>(st.at(p_stats, stats)) : nullptr;
    if (d_stats) HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(gms_warp_stats), dst->stream));
    // The kernel runs on dst's stream and reads src's arrays: dst's stream waits for what src's holds so far (the flushed apply pass, an
    // update's kernels), and src's stream waits for the kernel before anything enqueued on it later may write those arrays again
    // (gms_map_combine's two directions; no host synchronise)
    rc = gms_stream_after(dst->stream, src->stream, who);
    if (rc) return rc;
    const GridDev &gd = dst->gd, &gs = src->gd;
    const WarpDev g = {gd.posx, gd.posy, gd.res, gs.posx, gs.posy, gs.res, w->tx, w->ty, w->c, w->s, w->clamp, gd.W, w->x0, w->y0, w->w, w->h, gs.W, gs.H};
    double *d_dst = dst->d_log + (size_t)mi_dst * (size_t)gd.cells;
    if (s) {
        const WarpSource from = {nullptr, gms_slam_bufs(s), s->pf->d_stats, which, filter};
        warp_launch_op<true>(dst, g, d_dst, from, gs.cells, w->op, d_stats, st.shown(shown));
    } else {
        const WarpSource from = {src->d_log + (size_t)mi_src * (size_t)gs.cells, {}, nullptr, 0, 0};
        warp_launch_op<false>(dst, g, d_dst, from, gs.cells, w->op, d_stats, nullptr);
    }
    HIPCHK(hipGetLastError());
    rc = gms_stream_after(src->stream, dst->stream, who);
    if (rc) return rc;
    if (writes) map_log_replaced(dst);
    if (stats) st.fetch(stats, p_stats, sizeof(gms_warp_stats));
    return st.finish(s ? shown : nullptr);
}

extern "C" {

int gms_warp_pose(gms_warp *w, double x, double y, double theta) {
    REQUIRE(w, "gms_warp_pose: null request");
    REQUIRE(isfinite(x) && isfinite(y) && isfinite(theta), "gms_warp_pose: x, y and theta must be finite");
    w->tx = x;
    w->ty = y;
    w->c = cos(theta);
    w->s = sin(theta);
    return GMS_OK;
}

int gms_warp_check(const gms_warp *w) { return warp_check(w, "gms_warp_check"); }

int gms_map_warp(gms_map *dst, int32_t mi_dst, gms_map *src, int32_t mi_src, const gms_warp *w, gms_warp_stats *stats) {
    return warp(dst, mi_dst, src, mi_src, nullptr, 0, 0, w, stats, nullptr, false, "gms_map_warp");
}
int gms_map_warp_dev(gms_map *dst, int32_t mi_dst, gms_map *src, int32_t mi_src, const gms_warp *w, gms_warp_stats *dev_stats) {
    return warp(dst, mi_dst, src, mi_src, nullptr, 0, 0, w, dev_stats, nullptr, true, "gms_map_warp_dev");
}
int gms_slam_warp(gms_slam *s, int32_t which, int32_t filter, gms_map *dst, int32_t mi_dst, const gms_warp *w, gms_warp_stats *stats, int32_t *shown) {
    return warp(dst, mi_dst, s ? s->map : nullptr, 0, s, which, filter, w, stats, shown, false, "gms_slam_warp");
}
int gms_slam_warp_dev(gms_slam *s, int32_t which, int32_t filter, gms_map *dst, int32_t mi_dst, const gms_warp *w, gms_warp_stats *dev_stats, int32_t *dev_shown) {
    return warp(dst, mi_dst, s ? s->map : nullptr, 0, s, which, filter, w, dev_stats, dev_shown, true, "gms_slam_warp_dev");
}

}  // extern "C"
