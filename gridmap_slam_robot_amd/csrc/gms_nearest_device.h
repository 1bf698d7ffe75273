// gms_nearest_device.h -- the exact separable nearest-obstacle transform, capped at R: ONE copy of the row helpers, the field kernel, the
// poses kernel, their launcher and their checks for the clearance fields (gms_clearance.hip: the squared distance) and the sites
// (gms_skeleton.hip: the nearest obstacle cell itself).  All integer arithmetic.  The two differ in WHAT A CELL KEEPS of its nearest
// obstacle alone, a compile-time policy:
//   Keep::Stored, Keep::FAR    the 2-byte value stage 1b leaves per cell of a staged row, and "no set bit of the row within R"
//   Keep::row(dl, dr, R)       that value from the distances to the nearest set bit on the left and on the right
//   Keep::Acc, Keep::NONE      what stage 2 takes the minimum of, and "nothing yet"
//   Keep::cand(v, dy, dd, ...) the candidate of the row dy away (dd = dy^2), v its stored value at column x; (x, y) the cell, W the map
//   Keep::done(kk, best)       may stage 2 leave at distance k, kk = k^2?
//   Keep::wmin(best)           the wavefront's minimum
//   Keep::Field, ::field(best, cap); Keep::Pose, ::pose(best, cap), ::outside()   the output elements, cap = R^2
//
//   k_nearest_field  A workgroup owns ONE WORD of the plane's columns (32 cells) x TY rows of the rectangle, plus R rows of halo above and
//                    below (clipped to the map).  Stage 1a, a lane per staged row: the row's word and the distance from its ends to the
//                    nearest set bit of the (R + 31) / 32 words on either side (count leading / trailing zeros).  Stage 1b, a lane per
//                    cell: Keep::row of the horizontal distances to the nearest set bit of the row (the word itself, else its ends'
//                    distances), into LDS.  Stage 2, a lane per output cell: the minimum over dy of Keep::cand, dy = 0, -1, +1, -2, +2,
//                    ..., until Keep::done.
//   k_nearest_poses  a wavefront per pose: its lanes take the 2 R + 1 rows around the pose's cell, each Keep::row of that row at the
//                    cell's column from the plane's words in memory; Keep::wmin takes the minimum.  No field is made.
//
// LDS of k_nearest_field: 72 bytes per staged row (the word, the two end distances, 32 x Keep::Stored; a half-wave of stage 2 reads 32
// consecutive 2-byte values = 16 banks, no conflict), TY + 2 R rows: TY = 2 R rounded up to 8 and held to 64 .. 256 (and to the
// rectangle's h), so that the halo at most doubles stage 1: 8.0 KiB at R = 25, 18 KiB at R = 64, 53.9 KiB (766 rows) at R = 255 -- within
// the cast's 64 KiB.
#pragma once

#include <algorithm>

#include "gms_regions.h"

#define NEAR_NT 256
#define NEAR_LDS_CAP (64 * 1024)         // what k_nearest_field asks for at most (the cast's cap)
#define NEAR_ROW_BYTES 72                // LDS per staged row: 4 (word) + 4 (end distances) + 64 (Keep::Stored)
#define NEAR_END_NONE 0x3fffu            // an end distance: no set bit within reach (x + NEAR_END_NONE stays below 2^15)

static_assert((256 + 2 * 255) * NEAR_ROW_BYTES <= NEAR_LDS_CAP, "the tallest tile at the largest radius fits the LDS the kernel may ask for");

// ---- what a cell keeps ----
// the distance alone: g = min(dl, dr) per row, g^2 + dy^2 per candidate
struct KeepDistance {
    typedef uint16_t Stored;
    typedef uint32_t Acc;
    typedef uint16_t Field;
    typedef uint16_t Pose;
    static constexpr uint32_t FAR = 0xffffu;
    static constexpr Acc NONE = 0xffffffffu;
    __device__ static uint32_t row(uint32_t dl, uint32_t dr, int32_t R) {
        const uint32_t g = min(dl, dr);
        __builtin_assume(g < FAR);                                              // (at most 31 + NEAR_END_NONE)
        return g <= (uint32_t)R ? g : FAR;
    }
    __device__ static Acc cand(uint32_t g, int32_t, uint32_t dd, int32_t, int32_t, int32_t) { return g * g + dd; }
    __device__ static bool done(uint32_t kk, Acc best) { return kk >= best; }
    __device__ static Acc wmin(Acc best) { return wave_min(best); }
    __device__ static Field field(Acc best, uint32_t cap) { return (uint16_t)(best <= cap ? best : (uint32_t)GMS_CLEAR_FAR); }
    __device__ static Pose pose(Acc best, uint32_t cap) { return field(best, cap); }
    __device__ static Pose outside() { return (uint16_t)GMS_CLEAR_OUTSIDE; }
};
// the site: per row the SIGNED offset to the nearest set bit, the LEFT one at equal distance (smaller x, hence smaller index) -- within
// one row that bit is also the row's smallest key, so stage 2 takes one candidate per row --, per candidate the 64-bit key
// (off^2 + dy^2) << 32 | (y + dy) * W + x + off
struct KeepSite {
    typedef int16_t Stored;
    typedef uint64_t Acc;
    typedef uint32_t Field;
    typedef gms_nearest Pose;
    static constexpr int32_t FAR = 0x7fff;
    static constexpr Acc NONE = 0xffffffffffffffffull;
    __device__ static int32_t row(uint32_t dl, uint32_t dr, int32_t R) {
        if (min(dl, dr) > (uint32_t)R) return FAR;
        return dl <= dr ? -(int32_t)dl : (int32_t)dr;
    }
    __device__ static Acc cand(int32_t off, int32_t dy, uint32_t dd, int32_t x, int32_t y, int32_t W) {
        return ((uint64_t)((uint32_t)(off * off) + dd) << 32) | (uint64_t)((uint32_t)(y + dy) * (uint32_t)W + (uint32_t)(x + off));
    }
    // > and not >=: a row at dy^2 == best's d2 with off == 0 ties on d2 and wins on the index when it lies above, so equality must still
    // be visited (the distance may leave on >=: it keeps no argument)
    __device__ static bool done(uint32_t kk, Acc best) { return kk > (uint32_t)(best >> 32); }
    __device__ static Acc wmin(Acc best) { return wave_min(best); }
    __device__ static Field field(Acc best, uint32_t cap) { return (uint32_t)(best >> 32) <= cap ? (uint32_t)best : (uint32_t)GMS_SITE_NONE; }
    __device__ static Pose pose(Acc best, uint32_t cap) {
        return (uint32_t)(best >> 32) <= cap ? gms_nearest{(uint32_t)best, (uint32_t)(best >> 32)} : gms_nearest{(uint32_t)GMS_SITE_NONE, (uint32_t)GMS_CLEAR_FAR};
    }
    __device__ static Pose outside() { return gms_nearest{(uint32_t)GMS_SITE_OUTSIDE, (uint32_t)GMS_CLEAR_OUTSIDE}; }
};

// ---- the rows ----
// Word wx of a plane row of nw words: L = the distance from its bit 0 to the nearest set bit of the K words on its left, Rr = from its bit
// 31 to the nearest of the K on its right (NEAR_END_NONE: none; words outside the row hold nothing)
__device__ __forceinline__ void near_reach(const uint32_t *__restrict__ row, int32_t nw, int32_t wx, int32_t K, uint32_t &L, uint32_t &Rr) {
    L = Rr = NEAR_END_NONE;
    for (int32_t k = 0; k < K && wx - 1 - k >= 0; k++) {
        const uint32_t w = row[wx - 1 - k];
        if (w) { L = 1u + (uint32_t)__builtin_clz(w) + 32u * (uint32_t)k; break; }
    }
    for (int32_t k = 0; k < K && wx + 1 + k < nw; k++) {
        const uint32_t w = row[wx + 1 + k];
        if (w) { Rr = 1u + (uint32_t)__builtin_ctz(w) + 32u * (uint32_t)k; break; }
    }
}
// what bit x of word c keeps of its row: Keep::row of the horizontal distances to the nearest set bit at or left of it and at or right of
// it (>= NEAR_END_NONE: none within reach)
template <class Keep>
__device__ __forceinline__ auto near_row(uint32_t c, int32_t x, uint32_t L, uint32_t Rr, int32_t R) {
    const uint32_t lo = c & (0xffffffffu >> (31 - x)), hi = c >> x;             // the bits at and below x; at and above x, shifted down
    const uint32_t dl = lo ? (uint32_t)x - (31u - (uint32_t)__builtin_clz(lo)) : (uint32_t)x + L;
    const uint32_t dr = hi ? (uint32_t)__builtin_ctz(hi) : (31u - (uint32_t)x) + Rr;
    return Keep::row(dl, dr, R);
}

// plane: the map's, H rows of wpr words, W cells each.  Workgroup (bx, by): word (x0 >> 5) + bx of the columns, rows y0 + by * TY ... of
// the rectangle; rows_cap = the staged rows the launch asked LDS for (>= min(TY + 2 R, H)); out [h][w]
template <class Keep>
__global__ void __launch_bounds__(NEAR_NT)
k_nearest_field(const uint32_t *__restrict__ plane, int32_t wpr, int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t R, int32_t TY,
                int32_t rows_cap, typename Keep::Field *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t s_mem[];
    uint32_t *s_word = s_mem, *s_ends = s_mem + rows_cap;
    typename Keep::Stored *s_row = reinterpret_cast<typename Keep::Stored *>(s_mem + 2 * (size_t)rows_cap);
    const int32_t wx = (x0 >> 5) + (int32_t)blockIdx.x;
    const int32_t ys = y0 + (int32_t)blockIdx.y * TY, ye = min(ys + TY, y0 + h);
    const int32_t r0 = max(0, ys - R), r1 = min(H, ye + R), rows = min(r1 - r0, rows_cap);     // (r1 - r0 <= rows_cap by the launch's arithmetic)
    const int32_t K = (R + 31) >> 5;
    for (int32_t r = (int32_t)threadIdx.x; r < rows; r += NEAR_NT) {                           // stage 1a
        const uint32_t *__restrict__ row = plane + (size_t)(r0 + r) * (size_t)wpr;
        uint32_t L, Rr;
        near_reach(row, wpr, wx, K, L, Rr);
        s_word[r] = row[wx];
        s_ends[r] = L | (Rr << 16);
    }
    __syncthreads();
    for (int32_t i = (int32_t)threadIdx.x; i < rows * 32; i += NEAR_NT) {                      // stage 1b
        const int32_t r = i >> 5;
        const uint32_t e = s_ends[r];
        s_row[i] = (typename Keep::Stored)near_row<Keep>(s_word[r], i & 31, e & 0xffffu, e >> 16, R);
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x & 31, x = wx * 32 + col;                          // stage 2
    if (x < x0 || x >= x0 + w) return;
    const uint32_t cap = (uint32_t)(R * R);
    for (int32_t y = ys + ((int32_t)threadIdx.x >> 5); y < ye; y += NEAR_NT / 32) {
        const int32_t lr = y - r0;
        const auto visit = [&](typename Keep::Acc best, int32_t r, int32_t dy, uint32_t dd) {               // best with the candidate of staged row r = lr + dy
            const auto v = (decltype(Keep::row(0u, 0u, 0)))s_row[r * 32 + col];
            if (v != Keep::FAR) best = min(best, Keep::cand(v, dy, dd, x, y, W));
            return best;
        };
        typename Keep::Acc best = visit(Keep::NONE, lr, 0, 0u);
        for (int32_t k = 1; k <= R; k++) {
            const uint32_t kk = (uint32_t)(k * k);
            if (Keep::done(kk, best)) break;
            if (lr - k >= 0) best = visit(best, lr - k, -k, kk);
            if (lr + k < rows) best = visit(best, lr + k, k, kk);
        }
        out[(size_t)(y - y0) * (size_t)w + (size_t)(x - x0)] = Keep::field(best, cap);
    }
}

// a wavefront per pose; out [P]
template <class Keep>
__global__ void __launch_bounds__(NEAR_NT)
k_nearest_poses(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, const float *__restrict__ poses, int32_t P, int32_t R,
                typename Keep::Pose *__restrict__ out) {
    const int32_t pi = (int32_t)blockIdx.x * (NEAR_NT / 64) + ((int32_t)threadIdx.x >> 6), lane = (int32_t)threadIdx.x & 63;
    if (pi >= P) return;                                                                       // (uniform per wavefront)
    const int32_t gx = j_cell_exact((double)poses[3 * (size_t)pi] - g.posx, g.res);            // GridMap.java:273
    const int32_t gy = j_cell_exact((double)poses[3 * (size_t)pi + 1] - g.posy, g.res);        // :274
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) {                                          // :276 (uniform per wavefront)
        if (lane == 0) out[pi] = Keep::outside();
        return;
    }
    const int32_t wx = gx >> 5, K = (R + 31) >> 5;
    typename Keep::Acc best = Keep::NONE;
    for (int32_t dy = lane - R; dy <= R; dy += 64) {
        const int32_t y = gy + dy;
        if (y < 0 || y >= g.H) continue;
        const uint32_t *__restrict__ row = plane + (size_t)y * (size_t)wpr;
        uint32_t L, Rr;
        near_reach(row, wpr, wx, K, L, Rr);
        const auto v = near_row<Keep>(row[wx], gx & 31, L, Rr, R);
        if (v != Keep::FAR) best = min(best, Keep::cand(v, dy, (uint32_t)(dy * dy), gx, gy, g.W));
    }
    best = Keep::wmin(best);
    if (lane == 0) out[pi] = Keep::pose(best, (uint32_t)(R * R));
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the radius and the mode of a request or of a poses call, under the caller's prefix
static inline int nearest_reach_check(int32_t max_radius, int32_t mode, const char *what) {
    if (!(max_radius >= 1 && max_radius <= 255)) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= max_radius <= 255 cells", what);
    if (!(mode == GMS_CLEAR_OCCUPIED || mode == GMS_CLEAR_NOT_FREE)) return gms_fail(GMS_ERR_INVALID, "%s: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE", what);
    return GMS_OK;
}
// what gms_clearance and gms_skeleton share of a request
static inline int nearest_request_check(int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t max_radius, int32_t mode, const char *what) {
    if (!(w >= 1 && h >= 1)) return gms_fail(GMS_ERR_INVALID, "%s: w and h must be at least 1", what);
    if (!(x0 >= 0 && y0 >= 0)) return gms_fail(GMS_ERR_INVALID, "%s: x0 and y0 must not be negative", what);
    return nearest_reach_check(max_radius, mode, what);
}

// Field, an instantiation of k_nearest_field, over rectangle (x0, y0) + w x h of ONE map's plane into d_out [h][w]; a workgroup owns TY
// rows of the rectangle
template <auto Field, typename Out>
static inline int nearest_launch(gms_map *m, const uint32_t *d_plane, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t R, Out *d_out, const char *what) {
    const int32_t TY = std::min(h, std::min(256, std::max(64, (2 * R + 7) & ~7))), rows_cap = std::min(TY + 2 * R, m->gd.H);
    const int32_t words = ((x0 + w - 1) >> 5) - (x0 >> 5) + 1, bands = (h + TY - 1) / TY;
    if (bands > 65535) return gms_fail(GMS_ERR_INVALID, "%s: a rectangle of %d rows exceeds one launch", what, h);
    gms_launch<Field>(m, dim3((unsigned)words, (unsigned)bands), dim3(NEAR_NT), (size_t)rows_cap * NEAR_ROW_BYTES, d_plane, gms_plane_wpr(m), m->gd.W, m->gd.H,
                      x0, y0, w, h, R, TY, rows_cap, d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// Poses, an instantiation of k_nearest_poses, under P poses on map mi; map_check: a further test of the map behind the arguments', or NULL
template <auto Poses, typename Out>
static int nearest_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, Out *out, bool on_device, const char *what,
                         int (*map_check)(const gms_map *, const char *)) {
    if (!(m && poses && out)) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the map, the poses and the output are required)", what);
    if (!(mi >= 0 && mi < m->n_maps)) return gms_fail(GMS_ERR_INVALID, "%s: map index out of range", what);
    if (!(P >= 1 && P <= GMS_MAX_PARTICLES)) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= P <= GMS_MAX_PARTICLES poses", what);
    int rc = nearest_reach_check(max_radius, mode, what);
    if (rc) return rc;
    constexpr size_t align = alignof(Out);
    if (on_device && ((uintptr_t)out & (align - 1)) != 0) return gms_fail(GMS_ERR_INVALID, "%s_dev: the output must be %zu-byte aligned", what, align);
    if (map_check && (rc = map_check(m, what)) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)P * sizeof(Out), pose_bytes = (size_t)P * 3 * sizeof(float);
    const size_t p_out = st.part(out_bytes), p_poses = st.part(pose_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_poses, poses, pose_bytes);
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(query_map(m, mi), mode, nullptr, nullptr, &plane);
    if (rc) return rc;
    hipLaunchKernelGGL(Poses, dim3((unsigned)((P + NEAR_NT / 64 - 1) / (NEAR_NT / 64))), dim3(NEAR_NT), 0, m->stream, m->gd, plane,
                       gms_plane_wpr(m), st.at(p_poses, poses), P, max_radius, st.at(p_out, out));
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, out_bytes);
    return st.finish(nullptr);
}
