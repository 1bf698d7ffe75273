// gms_clearance.hip -- clearance fields (gridmapslam.h "clearance fields"): the squared distance, in cells, from every cell of a rectangle
// to the nearest obstacle cell of the whole map, capped at max_radius.  All integer arithmetic.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the planes       one bit per cell, rows of cast_wpr 32-bit words (padded to 64 cells, the padding zero).  GMS_CLEAR_OCCUPIED of a shared
//                    map IS the casts' plane (gms_cast_plane: logData > 0, kept on the handle until logData moves); GMS_CLEAR_NOT_FREE is a
//                    second plane, !(logData < 0), packed by k_clear_plane_map with the same ballot and kept beside it
//                    (gms_map::clear_plane_current, cleared wherever cast_plane_current is).  The per-particle filter has no plane kept
//                    per mode: k_clear_plane_slam packs the SHOWN particle's -- from plane 0 of its class planes (code 2 occupied, code 1
//                    free), or from logData where the handle keeps no planes -- into a scratch plane of the handle; particle and
//                    generation are picked there, on the device.
//   k_clear_field    the exact separable transform, capped at R.  A workgroup owns ONE WORD of the plane's columns (32 cells) x TY rows
//                    of the rectangle, plus R rows of halo above and below (clipped to the map).  Stage 1a, a lane per staged row: the
//                    row's word and the distance from its ends to the nearest set bit of the (R + 31) / 32 words on either side (count
//                    leading / trailing zeros).  Stage 1b, a lane per cell: g = the horizontal distance to the nearest set bit of the row
//                    (the word itself, else its ends' distances), 0xFFFF beyond R, into LDS.  Stage 2, a lane per output cell: min over
//                    dy of g(x, y + dy)^2 + dy^2, dy = 0, -+1, -+2, ..., left once dy^2 >= the best so far.
//   k_clear_poses    a wavefront per pose: its lanes take the 2 R + 1 rows around the pose's cell, each the horizontal distance of that
//                    row at the cell's column from the plane's words in memory; a butterfly takes the minimum.  No field is made.
//
// LDS of k_clear_field: 72 bytes per staged row (the word, the two end distances, 32 x uint16 of g; a half-wave of stage 2 reads 32
// consecutive uint16 = 16 banks, no conflict), TY + 2 R rows: TY = 2 R rounded up to 8 and held to 64 .. 256 (and to the rectangle's h), so
// that the halo at most doubles stage 1: 8.0 KiB at R = 25, 18 KiB at R = 64, 53.9 KiB (766 rows) at R = 255 -- within the cast's 64 KiB.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_device.h"

#define CLR_NT 256
#define CLR_LDS_CAP (64 * 1024)          // what k_clear_field asks for at most (the cast's cap)
#define CLR_ROW_BYTES 72                 // LDS per staged row: 4 (word) + 4 (end distances) + 64 (g)
#define CLR_NONE 0x3fffu                 // an end distance: no set bit within reach (x + CLR_NONE stays below 2^15)
#define CLR_G_FAR 0xffffu                // g: no set bit of the row within R

static_assert((256 + 2 * 255) * CLR_ROW_BYTES <= CLR_LDS_CAP, "the tallest tile at the largest radius fits the LDS the kernel may ask for");

// the second plane of the shared maps: !(logData < 0) -- occupied, never observed, or NaN (k_cast_plane's layout and ballot)
__global__ void __launch_bounds__(256)
k_clear_plane_map(const double *__restrict__ logd, int32_t W, int32_t H, int64_t cells, int32_t wpr64, uint64_t *__restrict__ plane) {
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t wx = (int32_t)blockIdx.x * 4 + wave, y = (int32_t)blockIdx.y, mi = (int32_t)blockIdx.z;
    if (wx >= wpr64) return;                                                    // (uniform per wavefront)
    const int32_t x = wx * 64 + lane;
    const double v = x < W ? logd[(size_t)mi * (size_t)cells + (size_t)y * (size_t)W + (size_t)x] : -1.0;     // (padding: free)
    const uint64_t bits = __ballot(!(v < 0.0));
    if (lane == 0) plane[((size_t)mi * (size_t)H + (size_t)y) * (size_t)wpr64 + (size_t)wx] = bits;
}

// the shown particle's plane under `mode`: which >= 0 that particle, GMS_VIEW_STRONGEST the strongest of `filter` by the last update's
// statistics (as k_cast_slam picks it); the generation from the epoch counters
template <bool CODES>
__global__ void __launch_bounds__(256)
k_clear_plane_slam(GridDev g, SlamBufs sb, int64_t code_words, const PfStatsDev *__restrict__ stats, int32_t which, int32_t filter, int32_t mode,
                   int32_t wpr64, uint64_t *__restrict__ plane, int32_t *__restrict__ shown) {
    const int32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t wx = (int32_t)blockIdx.x * 4 + wave, y = (int32_t)blockIdx.y;
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
    const uint64_t bits = __ballot(obstacle);
    if (lane == 0) plane[(size_t)y * (size_t)wpr64 + (size_t)wx] = bits;
}

// Word wx of a plane row of nw words: L = the distance from its bit 0 to the nearest set bit of the K words on its left, Rr = from its bit
// 31 to the nearest of the K on its right (CLR_NONE: none; words outside the row hold nothing)
__device__ __forceinline__ void clear_reach(const uint32_t *__restrict__ row, int32_t nw, int32_t wx, int32_t K, uint32_t &L, uint32_t &Rr) {
    L = Rr = CLR_NONE;
    for (int32_t k = 0; k < K && wx - 1 - k >= 0; k++) {
        const uint32_t w = row[wx - 1 - k];
        if (w) { L = 1u + (uint32_t)__builtin_clz(w) + 32u * (uint32_t)k; break; }
    }
    for (int32_t k = 0; k < K && wx + 1 + k < nw; k++) {
        const uint32_t w = row[wx + 1 + k];
        if (w) { Rr = 1u + (uint32_t)__builtin_ctz(w) + 32u * (uint32_t)k; break; }
    }
}
// the horizontal distance from bit x of word c to the nearest set bit of its row (>= CLR_NONE: none within reach)
__device__ __forceinline__ uint32_t clear_g(uint32_t c, int32_t x, uint32_t L, uint32_t Rr) {
    const uint32_t lo = c & (0xffffffffu >> (31 - x)), hi = c >> x;             // the bits at and below x; at and above x, shifted down
    const uint32_t dl = lo ? (uint32_t)x - (31u - (uint32_t)__builtin_clz(lo)) : (uint32_t)x + L;
    const uint32_t dr = hi ? (uint32_t)__builtin_ctz(hi) : (31u - (uint32_t)x) + Rr;
    return min(dl, dr);
}

// plane: the map's, H rows of wpr words.  Workgroup (bx, by): word (x0 >> 5) + bx of the columns, rows y0 + by * TY ... of the rectangle;
// rows_cap = the staged rows the launch asked LDS for (>= min(TY + 2 R, H)); out [h][w]
__global__ void __launch_bounds__(CLR_NT)
k_clear_field(const uint32_t *__restrict__ plane, int32_t wpr, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t R, int32_t TY,
              int32_t rows_cap, uint16_t *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t s_mem[];
    uint32_t *s_word = s_mem, *s_ends = s_mem + rows_cap;
    uint16_t *s_g = reinterpret_cast<uint16_t *>(s_mem + 2 * (size_t)rows_cap);
    const int32_t wx = (x0 >> 5) + (int32_t)blockIdx.x;
    const int32_t ys = y0 + (int32_t)blockIdx.y * TY, ye = min(ys + TY, y0 + h);
    const int32_t r0 = max(0, ys - R), r1 = min(H, ye + R), rows = min(r1 - r0, rows_cap);     // (r1 - r0 <= rows_cap by the launch's arithmetic)
    const int32_t K = (R + 31) >> 5;
    for (int32_t r = (int32_t)threadIdx.x; r < rows; r += CLR_NT) {                            // stage 1a
        const uint32_t *__restrict__ row = plane + (size_t)(r0 + r) * (size_t)wpr;
        uint32_t L, Rr;
        clear_reach(row, wpr, wx, K, L, Rr);
        s_word[r] = row[wx];
        s_ends[r] = L | (Rr << 16);
    }
    __syncthreads();
    for (int32_t i = (int32_t)threadIdx.x; i < rows * 32; i += CLR_NT) {                       // stage 1b
        const int32_t r = i >> 5;
        const uint32_t e = s_ends[r], gg = clear_g(s_word[r], i & 31, e & 0xffffu, e >> 16);
        s_g[i] = (uint16_t)(gg <= (uint32_t)R ? gg : CLR_G_FAR);
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x & 31, x = wx * 32 + col;                          // stage 2
    if (x < x0 || x >= x0 + w) return;
    const uint32_t cap = (uint32_t)(R * R);
    for (int32_t y = ys + ((int32_t)threadIdx.x >> 5); y < ye; y += CLR_NT / 32) {
        const int32_t lr = y - r0;
        uint32_t gg = s_g[lr * 32 + col];
        uint32_t best = gg != CLR_G_FAR ? gg * gg : 0xffffffffu;
        for (int32_t k = 1; k <= R; k++) {
            const uint32_t kk = (uint32_t)(k * k);
            if (kk >= best) break;
            if (lr - k >= 0) {
                gg = s_g[(lr - k) * 32 + col];
                if (gg != CLR_G_FAR) best = min(best, gg * gg + kk);
            }
            if (lr + k < rows) {
                gg = s_g[(lr + k) * 32 + col];
                if (gg != CLR_G_FAR) best = min(best, gg * gg + kk);
            }
        }
        out[(size_t)(y - y0) * (size_t)w + (size_t)(x - x0)] = (uint16_t)(best <= cap ? best : (uint32_t)GMS_CLEAR_FAR);
    }
}

// a wavefront per pose; out [P]
__global__ void __launch_bounds__(CLR_NT)
k_clear_poses(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, const float *__restrict__ poses, int32_t P, int32_t R, uint16_t *__restrict__ out) {
    const int32_t pi = (int32_t)blockIdx.x * (CLR_NT / 64) + ((int32_t)threadIdx.x >> 6), lane = (int32_t)threadIdx.x & 63;
    if (pi >= P) return;                                                                       // (uniform per wavefront)
    const int32_t gx = j_cell_exact((double)poses[3 * (size_t)pi] - g.posx, g.res);            // GridMap.java:273
    const int32_t gy = j_cell_exact((double)poses[3 * (size_t)pi + 1] - g.posy, g.res);        // :274
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) {                                          // :276 (uniform per wavefront)
        if (lane == 0) out[pi] = (uint16_t)GMS_CLEAR_OUTSIDE;
        return;
    }
    const int32_t wx = gx >> 5, K = (R + 31) >> 5;
    uint32_t best = 0xffffffffu;
    for (int32_t dy = lane - R; dy <= R; dy += 64) {
        const int32_t y = gy + dy;
        if (y < 0 || y >= g.H) continue;
        const uint32_t *__restrict__ row = plane + (size_t)y * (size_t)wpr;
        uint32_t L, Rr;
        clear_reach(row, wpr, wx, K, L, Rr);
        const uint32_t gg = clear_g(row[wx], gx & 31, L, Rr);
        if (gg <= (uint32_t)R) best = min(best, gg * gg + (uint32_t)(dy * dy));
    }
#define GMS_STEP_(O) best = min(best, wave_xor<O>(best));
    GMS_BUTTERFLY(GMS_STEP_)
#undef GMS_STEP_
    if (lane == 0) out[pi] = (uint16_t)(best <= (uint32_t)(R * R) ? best : (uint32_t)GMS_CLEAR_FAR);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the plane of `mode` of logData as it stands, every map's: the casts' own, or the second one (apply pass, allocation, pre-pass as there)
int gms_clear_plane(gms_map *m, int32_t mode, const uint32_t **plane) {
    if (mode == GMS_CLEAR_OCCUPIED) {
        int rc = gms_cast_plane(m);
        *plane = m->d_cast_plane;
        return rc;
    }
    gms_flush_apply(m);
    const int32_t wpr64 = (m->gd.W + 63) / 64;
    if (!m->d_clear_plane) {
        const size_t bytes = (size_t)m->n_maps * (size_t)m->gd.H * (size_t)wpr64 * sizeof(uint64_t);
        if (hipMalloc(&m->d_clear_plane, bytes) != hipSuccess) {
            m->d_clear_plane = nullptr;
            return gms_fail(GMS_ERR_NOMEM, "gms_map_clearance: the second bit plane's %zu bytes could not be allocated", bytes);
        }
        m->clear_plane_current = 0;
    }
    if (!m->clear_plane_current) {
        hipLaunchKernelGGL(k_clear_plane_map, dim3((unsigned)((wpr64 + 3) / 4), (unsigned)m->gd.H, (unsigned)m->n_maps), dim3(256), 0, m->stream, m->d_log,
                           m->gd.W, m->gd.H, m->gd.cells, wpr64, reinterpret_cast<uint64_t *>(m->d_clear_plane));
        HIPCHK(hipGetLastError());
        m->clear_plane_current = 1;
    }
    *plane = m->d_clear_plane;
    return GMS_OK;
}

// the rows of the rectangle a workgroup of k_clear_field owns
static inline int32_t clear_tile_rows(int32_t R, int32_t h) { return std::min(h, std::min(256, std::max(64, (2 * R + 7) & ~7))); }

// the field of rectangle c of ONE map's plane into d_out
int gms_clear_launch(gms_map *m, const uint32_t *d_plane, const gms_clearance *c, uint16_t *d_out) {
    const int32_t R = c->max_radius, TY = clear_tile_rows(R, c->h), rows_cap = std::min(TY + 2 * R, m->gd.H);
    const size_t lds = (size_t)rows_cap * CLR_ROW_BYTES;
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_clear_field), hipFuncAttributeMaxDynamicSharedMemorySize, CLR_LDS_CAP));
        attr_set = true;
    }
    const int32_t words = ((c->x0 + c->w - 1) >> 5) - (c->x0 >> 5) + 1, bands = (c->h + TY - 1) / TY;
    if (bands > 65535) return gms_fail(GMS_ERR_INVALID, "gms_clearance: a rectangle of %d rows exceeds one launch", c->h);
    hipLaunchKernelGGL(k_clear_field, dim3((unsigned)words, (unsigned)bands), dim3(CLR_NT), lds, m->stream, d_plane, gms_clear_wpr(m), m->gd.H, c->x0, c->y0,
                       c->w, c->h, R, TY, rows_cap, d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// c against a W x H map: gms_clearance_size's checks, then the rectangle inside [0, W] x [0, H] (gms_view_check's rule)
static int clear_check(const gms_clearance *c, int32_t W, int32_t H, const char *what, int64_t *bytes) {
    int rc = gms_clearance_size(c, nullptr, nullptr, bytes);
    if (rc) return rc;
    if ((int64_t)c->x0 + c->w > W || (int64_t)c->y0 + c->h > H)
        return gms_fail(GMS_ERR_INVALID, "%s: the rectangle (%d, %d) + %d x %d leaves the map's %d x %d cells", what, c->x0, c->y0, c->w, c->h, W, H);
    return GMS_OK;
}

static int map_clearance(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *out, bool on_device) {
    REQUIRE(m && c && out, "gms_map_clearance: null argument (the map, the request and the output are required)");
    REQUIRE(mi >= 0 && mi < m->n_maps, "gms_map_clearance: map index out of range");
    int64_t bytes = 0;
    int rc = clear_check(c, m->gd.W, m->gd.H, "gms_map_clearance", &bytes);
    if (rc) return rc;
    REQUIRE(!on_device || ((uintptr_t)out & 1) == 0, "gms_map_clearance_dev: the output must be 2-byte aligned");
    HIPCHK(hipSetDevice(m->device));
    unsigned char *base = nullptr;
    if (!on_device) { rc = gms_view_staging(m, bytes, &base); if (rc) return rc; }
    const uint32_t *plane = nullptr;
    rc = gms_clear_plane(m, c->mode, &plane);
    if (rc) return rc;
    uint16_t *d_out = on_device ? out : reinterpret_cast<uint16_t *>(base + 16);
    rc = gms_clear_launch(m, plane + (size_t)mi * (size_t)m->gd.H * (size_t)gms_clear_wpr(m), c, d_out);
    if (rc || on_device) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

static int map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out, bool on_device) {
    REQUIRE(m && poses && out, "gms_map_clearance_poses: null argument (the map, the poses and the output are required)");
    REQUIRE(mi >= 0 && mi < m->n_maps, "gms_map_clearance_poses: map index out of range");
    REQUIRE(P >= 1 && P <= GMS_MAX_PARTICLES, "gms_map_clearance_poses: 1 <= P <= GMS_MAX_PARTICLES poses");
    REQUIRE(max_radius >= 1 && max_radius <= 255, "gms_map_clearance_poses: 1 <= max_radius <= 255 cells");
    REQUIRE(mode == GMS_CLEAR_OCCUPIED || mode == GMS_CLEAR_NOT_FREE, "gms_map_clearance_poses: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(!on_device || ((uintptr_t)out & 1) == 0, "gms_map_clearance_poses_dev: the output must be 2-byte aligned");
    HIPCHK(hipSetDevice(m->device));
    const size_t out_bytes = ((size_t)P * sizeof(uint16_t) + 15) & ~(size_t)15, pose_bytes = (size_t)P * 3 * sizeof(float);
    unsigned char *base = nullptr;
    const float *d_poses = poses;
    uint16_t *d_out = out;
    if (!on_device) {                                       // the views' staging: [16 bytes][out][poses]
        int rc = gms_view_staging(m, (int64_t)(out_bytes + pose_bytes), &base);
        if (rc) return rc;
        d_out = reinterpret_cast<uint16_t *>(base + 16);
        float *stage = reinterpret_cast<float *>(base + 16 + out_bytes);
        HIPCHK(hipMemcpyAsync(stage, poses, pose_bytes, hipMemcpyHostToDevice, m->stream));
        d_poses = stage;
    }
    const uint32_t *plane = nullptr;
    int rc = gms_clear_plane(m, mode, &plane);
    if (rc) return rc;
    hipLaunchKernelGGL(k_clear_poses, dim3((unsigned)((P + CLR_NT / 64 - 1) / (CLR_NT / 64))), dim3(CLR_NT), 0, m->stream, m->gd,
                       plane + (size_t)mi * (size_t)m->gd.H * (size_t)gms_clear_wpr(m), gms_clear_wpr(m), d_poses, P, max_radius, d_out);
    HIPCHK(hipGetLastError());
    if (on_device) return GMS_OK;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)P * sizeof(uint16_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

// the shown particle's plane under `mode` into gms_map::d_clear_scratch (allocated by the first request), and its handle-wide index into
// d_shown (may be NULL); which / filter as gms_slam_view takes them, already checked.  d_dst: a plane of the caller's instead
int gms_clear_plane_slam(gms_slam *s, int32_t which, int32_t filter, int32_t mode, int32_t *d_shown, uint32_t *d_dst) {
    gms_map *m = s->map;
    const int32_t wpr64 = (m->gd.W + 63) / 64;
    if (!d_dst && !m->d_clear_scratch) {
        const size_t plane_bytes = (size_t)m->gd.H * (size_t)wpr64 * sizeof(uint64_t);
        if (hipMalloc(&m->d_clear_scratch, plane_bytes) != hipSuccess) {
            m->d_clear_scratch = nullptr;
            return gms_fail(GMS_ERR_NOMEM, "gms_slam_clearance: the particle's bit plane of %zu bytes could not be allocated", plane_bytes);
        }
    }
    const SlamBufs sb = gms_slam_bufs(s);
    if (which != GMS_VIEW_STRONGEST) filter = 0;
    uint64_t *dst = reinterpret_cast<uint64_t *>(d_dst ? d_dst : m->d_clear_scratch);
    const dim3 grid((unsigned)((wpr64 + 3) / 4), (unsigned)m->gd.H);
    if (s->d_code[0])
        hipLaunchKernelGGL((k_clear_plane_slam<true>), grid, dim3(256), 0, m->stream, m->gd, sb, s->code_words, s->pf->d_stats, which, filter, mode, wpr64,
                           dst, d_shown);
    else
        hipLaunchKernelGGL((k_clear_plane_slam<false>), grid, dim3(256), 0, m->stream, m->gd, sb, s->code_words, s->pf->d_stats, which, filter, mode, wpr64,
                           dst, d_shown);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

static int slam_clearance(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *out, int32_t *shown, bool on_device) {
    REQUIRE(s && c && out, "gms_slam_clearance: null argument (the handle, the request and the output are required)");
    gms_map *m = s->map;
    int64_t bytes = 0;
    int rc = clear_check(c, m->gd.W, m->gd.H, "gms_slam_clearance", &bytes);
    if (rc) return rc;
    REQUIRE(!on_device || ((uintptr_t)out & 1) == 0, "gms_slam_clearance_dev: the output must be 2-byte aligned");
    if (which == GMS_VIEW_STRONGEST) {
        REQUIRE(c->filter >= 0 && c->filter < s->n_filters, "gms_slam_clearance: gms_clearance.filter out of range");
        if (pf_is_shard(s->pf)) return gms_fail(GMS_ERR_STATE, "gms_slam_clearance: a shard of a filter (its strongest particle may live on another rank): name the particle");
        if (!s->have_strongest) return gms_fail(GMS_ERR_STATE, "gms_slam_clearance: no update since the handle was created or reset: there is no strongest particle yet");
    } else REQUIRE(which >= 0 && which < s->n, "gms_slam_clearance: particle index out of range");
    HIPCHK(hipSetDevice(m->device));
    unsigned char *base = nullptr;
    if (!on_device) { rc = gms_view_staging(m, bytes, &base); if (rc) return rc; }
    int32_t *d_shown = on_device ? shown : reinterpret_cast<int32_t *>(base);
    uint16_t *d_out = on_device ? out : reinterpret_cast<uint16_t *>(base + 16);
    rc = gms_clear_plane_slam(s, which, c->filter, c->mode, d_shown);
    if (rc) return rc;
    rc = gms_clear_launch(m, m->d_clear_scratch, c, d_out);
    if (rc || on_device) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)bytes, hipMemcpyDeviceToHost, m->stream));
    if (shown) HIPCHK(hipMemcpyAsync(shown, base, sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return GMS_OK;
}

extern "C" {

int gms_clearance_size(const gms_clearance *c, int32_t *out_w, int32_t *out_h, int64_t *bytes) {
    REQUIRE(c, "gms_clearance: null request");
    REQUIRE(c->w >= 1 && c->h >= 1, "gms_clearance: w and h must be at least 1");
    REQUIRE(c->x0 >= 0 && c->y0 >= 0, "gms_clearance: x0 and y0 must not be negative");
    REQUIRE(c->max_radius >= 1 && c->max_radius <= 255, "gms_clearance: 1 <= max_radius <= 255 cells");
    REQUIRE(c->mode == GMS_CLEAR_OCCUPIED || c->mode == GMS_CLEAR_NOT_FREE, "gms_clearance: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    if (out_w) *out_w = c->w;
    if (out_h) *out_h = c->h;
    if (bytes) *bytes = (int64_t)c->w * c->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_clearance(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *out) { return map_clearance(m, mi, c, out, false); }
int gms_map_clearance_dev(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *dev_out) { return map_clearance(m, mi, c, dev_out, true); }
int gms_map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out) {
    return map_clearance_poses(m, mi, poses, P, max_radius, mode, out, false);
}
int gms_map_clearance_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *dev_out) {
    return map_clearance_poses(m, mi, dev_poses, P, max_radius, mode, dev_out, true);
}
int gms_slam_clearance(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *out, int32_t *shown) {
    return slam_clearance(s, which, c, out, shown, false);
}
int gms_slam_clearance_dev(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *dev_out, int32_t *dev_shown) {
    return slam_clearance(s, which, c, dev_out, dev_shown, true);
}

}  // extern "C"
