// gms_clearance.hip -- clearance fields (gridmapslam.h "clearance fields"): the squared distance, in cells, from every cell of a rectangle
// to the nearest obstacle cell of the whole map, capped at max_radius.  All integer arithmetic.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the planes       one bit per cell, rows of gms_plane_wpr 32-bit words (padded to 64 cells, the padding zero): the map's plane of the
//                    request's mode, or the shown particle's, packed per request (query_plane, gms_query.hip).
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
// the rows of the rectangle a workgroup of k_clear_field owns
static inline int32_t clear_tile_rows(int32_t R, int32_t h) { return std::min(h, std::min(256, std::max(64, (2 * R + 7) & ~7))); }

// the field of rectangle c of ONE map's plane into d_out
int gms_clear_launch(gms_map *m, const uint32_t *d_plane, const gms_clearance *c, uint16_t *d_out) {
    const int32_t R = c->max_radius, TY = clear_tile_rows(R, c->h), rows_cap = std::min(TY + 2 * R, m->gd.H);
    const size_t lds = (size_t)rows_cap * CLR_ROW_BYTES;
    HIPCHK(gms_kernel_lds<k_clear_field>(m->device, CLR_LDS_CAP));
    const int32_t words = ((c->x0 + c->w - 1) >> 5) - (c->x0 >> 5) + 1, bands = (c->h + TY - 1) / TY;
    if (bands > 65535) return gms_fail(GMS_ERR_INVALID, "gms_clearance: a rectangle of %d rows exceeds one launch", c->h);
    hipLaunchKernelGGL(k_clear_field, dim3((unsigned)words, (unsigned)bands), dim3(CLR_NT), lds, m->stream, d_plane, gms_plane_wpr(m), m->gd.H, c->x0, c->y0,
                       c->w, c->h, R, TY, rows_cap, d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the field of one map of a shared handle or of the shown particle of a per-particle one; `shown` exists for a particle only
static int clearance(QuerySource src, const char *what, const gms_clearance *c, uint16_t *out, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !c || !out) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request and the output are required)", what);
    gms_map *m = src.m;
    int64_t bytes = 0;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (!rc) rc = gms_clearance_size(c, nullptr, nullptr, &bytes);
    if (!rc) rc = gms_rect_check(c->x0, c->y0, c->w, c->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if (on_device && ((uintptr_t)out & 1) != 0) return gms_fail(GMS_ERR_INVALID, "%s_dev: the output must be 2-byte aligned", what);
    src.filter = c->filter;
    if (src.s && (rc = query_check(src, what, "gms_clearance.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t p_out = st.part((size_t)bytes);
    rc = st.open();
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(src, c->mode, st.shown(shown), nullptr, &plane);
    if (!rc) rc = gms_clear_launch(m, plane, c, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, (size_t)bytes);
    return st.finish(shown);
}

static int map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out, bool on_device) {
    REQUIRE(m && poses && out, "gms_map_clearance_poses: null argument (the map, the poses and the output are required)");
    REQUIRE(mi >= 0 && mi < m->n_maps, "gms_map_clearance_poses: map index out of range");
    REQUIRE(P >= 1 && P <= GMS_MAX_PARTICLES, "gms_map_clearance_poses: 1 <= P <= GMS_MAX_PARTICLES poses");
    REQUIRE(max_radius >= 1 && max_radius <= 255, "gms_map_clearance_poses: 1 <= max_radius <= 255 cells");
    REQUIRE(mode == GMS_CLEAR_OCCUPIED || mode == GMS_CLEAR_NOT_FREE, "gms_map_clearance_poses: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(!on_device || ((uintptr_t)out & 1) == 0, "gms_map_clearance_poses_dev: the output must be 2-byte aligned");
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)P * sizeof(uint16_t), pose_bytes = (size_t)P * 3 * sizeof(float);
    const size_t p_out = st.part(out_bytes), p_poses = st.part(pose_bytes);
    int rc = st.open();
    if (!rc) rc = st.up(p_poses, poses, pose_bytes);
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(query_map(m, mi), mode, nullptr, nullptr, &plane);
    if (rc) return rc;
    hipLaunchKernelGGL(k_clear_poses, dim3((unsigned)((P + CLR_NT / 64 - 1) / (CLR_NT / 64))), dim3(CLR_NT), 0, m->stream, m->gd, plane, gms_plane_wpr(m),
                       st.at(p_poses, poses), P, max_radius, st.at(p_out, out));
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, out_bytes);
    return st.finish(nullptr);
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
int gms_map_clearance(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *out) { return clearance(query_map(m, mi), "gms_map_clearance", c, out, nullptr, false); }
int gms_map_clearance_dev(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *dev_out) { return clearance(query_map(m, mi), "gms_map_clearance", c, dev_out, nullptr, true); }
int gms_map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out) {
    return map_clearance_poses(m, mi, poses, P, max_radius, mode, out, false);
}
int gms_map_clearance_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *dev_out) {
    return map_clearance_poses(m, mi, dev_poses, P, max_radius, mode, dev_out, true);
}
int gms_slam_clearance(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *out, int32_t *shown) {
    return clearance(query_slam(s, which), "gms_slam_clearance", c, out, shown, false);
}
int gms_slam_clearance_dev(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *dev_out, int32_t *dev_shown) {
    return clearance(query_slam(s, which), "gms_slam_clearance", c, dev_out, dev_shown, true);
}

}  // extern "C"
