// gms_skeleton.hip -- nearest-obstacle sites and the free-space skeleton (gridmapslam.h "sites and skeleton"): for every cell of a
// rectangle the obstacle cell of the whole map that is nearest to it under a stated tie rule, and the cells that lie equally far from two
// separated pieces of wall.  All integer arithmetic.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the planes       the clearance fields' (gms_clearance.hip): the map's plane of the request's mode, or the shown particle's, packed
//                    per request (query_plane, gms_query.hip).  The padding of a row holds no bit under either mode.
//   k_site_field     k_clear_field's separable scheme with the arg-min kept.  A workgroup owns ONE WORD of the plane's columns (32 cells)
//                    x TY rows of the rectangle, plus R rows of halo above and below (clipped to the map).  Stage 1a, a lane per staged
//                    row: the row's word and the distance from its ends to the nearest set bit of the (R + 31) / 32 words on either
//                    side.  Stage 1b, a lane per cell: the SIGNED horizontal offset to the nearest set bit of the row, the LEFT one at
//                    equal distance (smaller x, hence smaller index), SITE_OFF_FAR beyond R, into LDS as int16.  Within one row that bit
//                    is also the row's smallest key, so stage 2 takes one candidate per row.  Stage 2, a lane per output cell: the
//                    minimum over dy of the 64-bit key (off^2 + dy^2) << 32 | (y + dy) * W + x + off, dy = 0, -1, +1, -2, +2, ...,
//                    left only once dy^2 > the best d2 so far: a row at dy^2 == best with off == 0 ties on d2 and wins on the index when
//                    it lies above, so equality must still be visited (the clearance field may leave on >=: it keeps no argument).
//   k_site_ridge     the three skeleton rules, a lane per cell of the rectangle, over a site field of the rectangle grown by one cell
//                    on every side that lies inside the map (gms_map::d_site_field, grow-only).  Whether a cell is an obstacle and its
//                    d2 are both recomputed from its site (an obstacle cell, and no other, is its own site): no second field and no
//                    plane is read.  Copies the rectangle's sites out, writes the skeleton's d2 and counts the totals -- ballots, one
//                    row of LDS per wavefront, one 64-bit atomic per counter and workgroup.
//   k_site_poses     k_clear_poses' shape: a wavefront per pose, its lanes take the 2 R + 1 rows around the pose's cell from the plane's
//                    words in memory, wave_min(uint64_t) takes the smallest key.  No field is made.
//
// Why a second launch for the ridge and not a halo in the site kernel: a workgroup of k_site_field owns one plane word; a column of halo
// on either side is two more words, that is three times stage 1 and three times the LDS for two columns of output.  The ridge pass is a
// gather of five 4-byte words per cell from a field that has just been written (16 MiB at 2048 x 2048: cache-resident) and not the
// expensive part.  A request for sites alone runs no second launch: k_site_field writes the caller's array itself.
//
// LDS of k_site_field: k_clear_field's, 72 bytes per staged row (the word, the two end distances, 32 x int16 of offsets; a half-wave of
// stage 2 reads 32 consecutive int16 = 16 banks, no conflict), TY + 2 R rows with the same TY: 53.9 KiB (766 rows) at R = 255.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_regions.h"

#define SITE_NT 256
#define SITE_LDS_CAP (64 * 1024)         // what k_site_field asks for at most (the clearance field's cap)
#define SITE_ROW_BYTES 72                // LDS per staged row: 4 (word) + 4 (end distances) + 64 (offsets)
#define SITE_END_NONE 0x3fffu            // an end distance: no set bit within reach (x + SITE_END_NONE stays below 2^15)
#define SITE_OFF_FAR 0x7fff              // an offset: no set bit of the row within R
#define SITE_KEY_NONE 0xffffffffffffffffull
#define SITE_RIDGE_ROWS 16               // rows of the rectangle a workgroup of k_site_ridge takes, 64 columns wide

static_assert((256 + 2 * 255) * SITE_ROW_BYTES <= SITE_LDS_CAP, "the tallest tile at the largest radius fits the LDS the kernel may ask for");
static_assert(sizeof(gms_skeleton) == 48 && sizeof(gms_skeleton_totals) == 32 && sizeof(gms_nearest) == 8, "the records' layout is part of the interface");

// Word wx of a plane row of nw words: L = the distance from its bit 0 to the nearest set bit of the K words on its left, Rr = from its bit
// 31 to the nearest of the K on its right (SITE_END_NONE: none; words outside the row hold nothing)
__device__ __forceinline__ void site_reach(const uint32_t *__restrict__ row, int32_t nw, int32_t wx, int32_t K, uint32_t &L, uint32_t &Rr) {
    L = Rr = SITE_END_NONE;
    for (int32_t k = 0; k < K && wx - 1 - k >= 0; k++) {
        const uint32_t w = row[wx - 1 - k];
        if (w) { L = 1u + (uint32_t)__builtin_clz(w) + 32u * (uint32_t)k; break; }
    }
    for (int32_t k = 0; k < K && wx + 1 + k < nw; k++) {
        const uint32_t w = row[wx + 1 + k];
        if (w) { Rr = 1u + (uint32_t)__builtin_ctz(w) + 32u * (uint32_t)k; break; }
    }
}
// the signed horizontal offset from bit x of word c to the nearest set bit of its row within R, the left one at equal distance
// (SITE_OFF_FAR: none)
__device__ __forceinline__ int32_t site_off(uint32_t c, int32_t x, uint32_t L, uint32_t Rr, int32_t R) {
    const uint32_t lo = c & (0xffffffffu >> (31 - x)), hi = c >> x;             // the bits at and below x; at and above x, shifted down
    const uint32_t dl = lo ? (uint32_t)x - (31u - (uint32_t)__builtin_clz(lo)) : (uint32_t)x + L;
    const uint32_t dr = hi ? (uint32_t)__builtin_ctz(hi) : (31u - (uint32_t)x) + Rr;
    const uint32_t d = min(dl, dr);
    if (d > (uint32_t)R) return SITE_OFF_FAR;
    return dl <= dr ? -(int32_t)dl : (int32_t)dr;
}
// the key of the candidate of the row dy away: its bit `off` beside column x of row y
__device__ __forceinline__ uint64_t site_key(int32_t off, int32_t dy, int32_t x, int32_t y, int32_t W) {
    return ((uint64_t)(uint32_t)(off * off + dy * dy) << 32) | (uint64_t)((uint32_t)(y + dy) * (uint32_t)W + (uint32_t)(x + off));
}
// a key as the site it names: SITE_NONE beyond R^2
__device__ __forceinline__ uint32_t site_of_key(uint64_t key, uint32_t cap) { return (uint32_t)(key >> 32) <= cap ? (uint32_t)key : (uint32_t)GMS_SITE_NONE; }

// plane: the map's, H rows of wpr words, W cells each.  Workgroup (bx, by): word (x0 >> 5) + bx of the columns, rows y0 + by * TY ... of
// the rectangle; rows_cap = the staged rows the launch asked LDS for (>= min(TY + 2 R, H)); out [h][w]
__global__ void __launch_bounds__(SITE_NT)
k_site_field(const uint32_t *__restrict__ plane, int32_t wpr, int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t R, int32_t TY,
             int32_t rows_cap, uint32_t *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t s_mem[];
    uint32_t *s_word = s_mem, *s_ends = s_mem + rows_cap;
    int16_t *s_off = reinterpret_cast<int16_t *>(s_mem + 2 * (size_t)rows_cap);
    const int32_t wx = (x0 >> 5) + (int32_t)blockIdx.x;
    const int32_t ys = y0 + (int32_t)blockIdx.y * TY, ye = min(ys + TY, y0 + h);
    const int32_t r0 = max(0, ys - R), r1 = min(H, ye + R), rows = min(r1 - r0, rows_cap);     // (r1 - r0 <= rows_cap by the launch's arithmetic)
    const int32_t K = (R + 31) >> 5;
    for (int32_t r = (int32_t)threadIdx.x; r < rows; r += SITE_NT) {                           // stage 1a
        const uint32_t *__restrict__ row = plane + (size_t)(r0 + r) * (size_t)wpr;
        uint32_t L, Rr;
        site_reach(row, wpr, wx, K, L, Rr);
        s_word[r] = row[wx];
        s_ends[r] = L | (Rr << 16);
    }
    __syncthreads();
    for (int32_t i = (int32_t)threadIdx.x; i < rows * 32; i += SITE_NT) {                      // stage 1b
        const int32_t r = i >> 5;
        const uint32_t e = s_ends[r];
        s_off[i] = (int16_t)site_off(s_word[r], i & 31, e & 0xffffu, e >> 16, R);
    }
    __syncthreads();
    const int32_t col = (int32_t)threadIdx.x & 31, x = wx * 32 + col;                          // stage 2
    if (x < x0 || x >= x0 + w) return;
    const uint32_t cap = (uint32_t)(R * R);
    for (int32_t y = ys + ((int32_t)threadIdx.x >> 5); y < ye; y += SITE_NT / 32) {
        const int32_t lr = y - r0;
        int32_t off = s_off[lr * 32 + col];
        uint64_t best = off != SITE_OFF_FAR ? site_key(off, 0, x, y, W) : SITE_KEY_NONE;
        for (int32_t k = 1; k <= R; k++) {
            if ((uint32_t)(k * k) > (uint32_t)(best >> 32)) break;                             // (> and not >=: a tie on d2 may still win on the index)
            if (lr - k >= 0) {
                off = s_off[(lr - k) * 32 + col];
                if (off != SITE_OFF_FAR) best = min(best, site_key(off, -k, x, y, W));
            }
            if (lr + k < rows) {
                off = s_off[(lr + k) * 32 + col];
                if (off != SITE_OFF_FAR) best = min(best, site_key(off, k, x, y, W));
            }
        }
        out[(size_t)(y - y0) * (size_t)w + (size_t)(x - x0)] = site_of_key(best, cap);
    }
}

// a wavefront per pose; out [P]
__global__ void __launch_bounds__(SITE_NT)
k_site_poses(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, const float *__restrict__ poses, int32_t P, int32_t R, gms_nearest *__restrict__ out) {
    const int32_t pi = (int32_t)blockIdx.x * (SITE_NT / 64) + ((int32_t)threadIdx.x >> 6), lane = (int32_t)threadIdx.x & 63;
    if (pi >= P) return;                                                                       // (uniform per wavefront)
    const int32_t gx = j_cell_exact((double)poses[3 * (size_t)pi] - g.posx, g.res);            // GridMap.java:273
    const int32_t gy = j_cell_exact((double)poses[3 * (size_t)pi + 1] - g.posy, g.res);        // :274
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) {                                          // :276 (uniform per wavefront)
        if (lane == 0) out[pi] = gms_nearest{(uint32_t)GMS_SITE_OUTSIDE, (uint32_t)GMS_CLEAR_OUTSIDE};
        return;
    }
    const int32_t wx = gx >> 5, K = (R + 31) >> 5;
    uint64_t best = SITE_KEY_NONE;
    for (int32_t dy = lane - R; dy <= R; dy += 64) {
        const int32_t y = gy + dy;
        if (y < 0 || y >= g.H) continue;
        const uint32_t *__restrict__ row = plane + (size_t)y * (size_t)wpr;
        uint32_t L, Rr;
        site_reach(row, wpr, wx, K, L, Rr);
        const int32_t off = site_off(row[wx], gx & 31, L, Rr, R);
        if (off != SITE_OFF_FAR) best = min(best, site_key(off, dy, gx, gy, g.W));
    }
    best = wave_min(best);
    if (lane == 0) {
        const bool within = (uint32_t)(best >> 32) <= (uint32_t)(R * R);
        out[pi] = within ? gms_nearest{(uint32_t)best, (uint32_t)(best >> 32)} : gms_nearest{(uint32_t)GMS_SITE_NONE, (uint32_t)GMS_CLEAR_FAR};
    }
}

// the squared distance between cells a and b of a map W wide
__device__ __forceinline__ uint32_t site_d2(uint32_t a, uint32_t b, uint32_t W) {
    const int32_t dx = (int32_t)(a % W) - (int32_t)(b % W), dy = (int32_t)(a / W) - (int32_t)(b / W);
    return (uint32_t)(dx * dx + dy * dy);
}

// field: the sites of the rectangle (fx0, fy0) + fw x fh, which holds (x0, y0) + w x h and every axis neighbour of its cells that lies
// inside the W x H map.  Workgroup (bx, by): columns x0 + 64 bx ..., rows y0 + SITE_RIDGE_ROWS by ... of the rectangle, a wavefront per
// row.  site / skel [h][w] and totals (zeroed by the launcher), each where non-NULL
__global__ void __launch_bounds__(SITE_NT)
k_site_ridge(const uint32_t *__restrict__ field, int32_t fx0, int32_t fy0, int32_t fw, int32_t fh, int32_t W, int32_t H, int32_t x0, int32_t y0, int32_t w,
             int32_t h, uint32_t clear2, uint32_t gap2, uint32_t *__restrict__ site, uint16_t *__restrict__ skel, gms_skeleton_totals *__restrict__ totals) {
    __shared__ uint32_t s_cnt[SITE_NT / 64][4];
    const int32_t lane = (int32_t)threadIdx.x & 63, wave = (int32_t)threadIdx.x >> 6;
    const int32_t rx = (int32_t)blockIdx.x * 64 + lane, x = x0 + rx;
    const bool valid = rx < w;
    uint32_t n_sited = 0u, n_skel = 0u, lo = 0xffffffffu, hi = 0u;
    for (int32_t r = wave; r < SITE_RIDGE_ROWS; r += SITE_NT / 64) {
        const int32_t ry = (int32_t)blockIdx.y * SITE_RIDGE_ROWS + r;
        if (ry >= h) break;                                                                    // (uniform per wavefront)
        const int32_t y = y0 + ry;
        uint32_t s = (uint32_t)GMS_SITE_NONE, d2 = 0u;
        bool ridge = false;
        if (valid) {
            const uint32_t *__restrict__ at = field + (size_t)(y - fy0) * (size_t)fw + (size_t)(x - fx0);
            const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x;
            s = *at;
            if (s != (uint32_t)GMS_SITE_NONE && s != c) {                                      // rule 1 (an obstacle cell is its own site)
                d2 = site_d2(c, s, (uint32_t)W);
                if (d2 >= clear2) {
#pragma unroll
                    for (int32_t k = 0; k < 4; k++) {
                        const int32_t dx = k == 0 ? -1 : k == 1 ? 1 : 0, dy = k == 2 ? -1 : k == 3 ? 1 : 0;
                        if (x + dx < 0 || x + dx >= W || y + dy < 0 || y + dy >= H) continue;
                        const uint32_t n = (uint32_t)((int32_t)c + dy * W + dx), sn = at[dy * fw + dx];
                        if (sn == (uint32_t)GMS_SITE_NONE || sn == n) continue;               // rule 2: no site, or an obstacle
                        if (site_d2(s, sn, (uint32_t)W) < gap2) continue;
                        const uint32_t dn = site_d2(n, sn, (uint32_t)W);
                        ridge = ridge || d2 > dn || (d2 == dn && c < n);                       // rule 3
                    }
                }
            }
        }
        if (site && valid) site[(size_t)ry * (size_t)w + (size_t)rx] = s;
        if (skel && valid) skel[(size_t)ry * (size_t)w + (size_t)rx] = (uint16_t)(ridge ? d2 : 0u);
        if (totals) {
            n_sited += (uint32_t)__popcll(__ballot(valid && s != (uint32_t)GMS_SITE_NONE));
            n_skel += (uint32_t)__popcll(__ballot(ridge));
            if (ridge) { lo = min(lo, d2); hi = max(hi, d2); }
        }
    }
    if (!totals) return;                                                                       // (uniform per launch)
    lo = (uint32_t)wave_min((int32_t)min(lo, 0x7fffffffu));
    hi = (uint32_t)wave_max((int32_t)hi);
    if (lane == 0) { s_cnt[wave][0] = n_sited; s_cnt[wave][1] = n_skel; s_cnt[wave][2] = lo; s_cnt[wave][3] = hi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int32_t k = 1; k < SITE_NT / 64; k++) {
        n_sited += s_cnt[k][0]; n_skel += s_cnt[k][1];
        lo = min(lo, s_cnt[k][2]); hi = max(hi, s_cnt[k][3]);
    }
    if (n_sited) atomicAdd(reinterpret_cast<unsigned long long *>(&totals->sited), (unsigned long long)n_sited);
    if (!n_skel) return;
    atomicAdd(reinterpret_cast<unsigned long long *>(&totals->skeleton), (unsigned long long)n_skel);
    atomicMax(&totals->max_d2, (int32_t)hi);
    int32_t seen = __atomic_load_n(&totals->min_d2, __ATOMIC_RELAXED);                         // 0: no skeleton cell yet (theirs are >= 1)
    while (seen == 0 || (int32_t)lo < seen) {
        const int32_t was = atomicCAS(&totals->min_d2, seen, (int32_t)lo);
        if (was == seen) break;
        seen = was;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the rows of the rectangle a workgroup of k_site_field owns (the clearance field's choice)
static inline int32_t site_tile_rows(int32_t R, int32_t h) { return std::min(h, std::min(256, std::max(64, (2 * R + 7) & ~7))); }

// the sites of rectangle (x0, y0) + w x h of ONE map's plane into d_out [h][w]
static int site_launch(gms_map *m, const uint32_t *d_plane, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t R, uint32_t *d_out, const char *what) {
    const int32_t TY = site_tile_rows(R, h), rows_cap = std::min(TY + 2 * R, m->gd.H);
    const int32_t words = ((x0 + w - 1) >> 5) - (x0 >> 5) + 1, bands = (h + TY - 1) / TY;
    if (bands > 65535) return gms_fail(GMS_ERR_INVALID, "%s: a rectangle of %d rows exceeds one launch", what, h);
    gms_launch<k_site_field>(m, dim3((unsigned)words, (unsigned)bands), dim3(SITE_NT), (size_t)rows_cap * SITE_ROW_BYTES, d_plane, gms_plane_wpr(m), m->gd.W,
                             m->gd.H, x0, y0, w, h, R, TY, rows_cap, d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// a site is 32 bits of cell index below the two sentinels
static int site_map_check(const gms_map *m, const char *what) {
    if (m->gd.cells >= (int64_t)GMS_SITE_OUTSIDE) return gms_fail(GMS_ERR_INVALID, "%s: a map of 2^32 - 2 cells or more has no 32-bit sites", what);
    return GMS_OK;
}

// sites, skeleton and totals of one map of a shared handle or of the shown particle of a per-particle one; `shown` exists for a particle only
static int skeleton(QuerySource src, const char *what, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals, int32_t *shown,
                    bool on_device) {
    if ((!src.m && !src.s) || !q) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle and the request are required)", what);
    if (!site && !skel && !totals) return gms_fail(GMS_ERR_INVALID, "%s: site, skel and totals are all NULL: nothing to compute", what);
    gms_map *m = src.m;
    int64_t site_bytes = 0, skel_bytes = 0;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (!rc) rc = gms_skeleton_size(q, nullptr, nullptr, &site_bytes, &skel_bytes);
    if (!rc) rc = gms_rect_check(q->x0, q->y0, q->w, q->h, m->gd.W, m->gd.H, what);
    if (!rc) rc = site_map_check(m, what);
    if (rc) return rc;
    if (on_device && (((uintptr_t)site & 3) != 0 || ((uintptr_t)skel & 1) != 0 || ((uintptr_t)totals & 7) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s_dev: site must be 4-byte, skel 2-byte and totals 8-byte aligned", what);
    src.filter = q->filter;
    if (src.s && (rc = query_check(src, what, "gms_skeleton.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    // the ridge pass reads the rectangle grown by one cell on every side that lies inside the map; sites alone need no ridge pass
    const bool ridge = skel || totals;
    const int32_t fx0 = std::max(q->x0 - 1, 0), fy0 = std::max(q->y0 - 1, 0);
    const int32_t fw = std::min(q->x0 + q->w + 1, m->gd.W) - fx0, fh = std::min(q->y0 + q->h + 1, m->gd.H) - fy0;
    if (ridge) {
        rc = gms_dev_grow(&m->d_site_field, &m->site_cap, (int64_t)fw * fh, 65536, &m->stream, [](size_t c) { return c * sizeof(uint32_t); }, what,
                          "the site field the ridge pass reads");
        if (rc) return rc;
    }
    HostStage st(m, on_device);
    const size_t p_site = site ? st.part((size_t)site_bytes) : 0, p_skel = skel ? st.part((size_t)skel_bytes) : 0;
    const size_t p_totals = totals ? st.part(sizeof(gms_skeleton_totals)) : 0;
    rc = st.open();
    if (rc) return rc;
    uint32_t *d_site = site ? st.at(p_site, site) : nullptr;
    uint16_t *d_skel = skel ? st.at(p_skel, skel) : nullptr;
    gms_skeleton_totals *d_totals = totals ? st.at(p_totals, totals) : nullptr;
    const uint32_t *plane = nullptr;
    rc = query_plane(src, q->mode, st.shown(shown), nullptr, &plane);
    if (rc) return rc;
    if (!ridge) {
        rc = site_launch(m, plane, q->x0, q->y0, q->w, q->h, q->max_radius, d_site, what);
        if (rc) return rc;
    } else {
        rc = site_launch(m, plane, fx0, fy0, fw, fh, q->max_radius, m->d_site_field, what);
        if (rc) return rc;
        if (d_totals) HIPCHK(hipMemsetAsync(d_totals, 0, sizeof(gms_skeleton_totals), m->stream));
        const dim3 grid((unsigned)((q->w + 63) / 64), (unsigned)((q->h + SITE_RIDGE_ROWS - 1) / SITE_RIDGE_ROWS));
        hipLaunchKernelGGL(k_site_ridge, grid, dim3(SITE_NT), 0, m->stream, m->d_site_field, fx0, fy0, fw, fh, m->gd.W, m->gd.H, q->x0, q->y0, q->w, q->h,
                           (uint32_t)(q->min_clear * q->min_clear), (uint32_t)(q->min_gap * q->min_gap), d_site, d_skel, d_totals);
        HIPCHK(hipGetLastError());
    }
    if (site) st.fetch(site, p_site, (size_t)site_bytes);
    if (skel) st.fetch(skel, p_skel, (size_t)skel_bytes);
    if (totals) st.fetch(totals, p_totals, sizeof(gms_skeleton_totals));
    return st.finish(shown);
}

static int map_nearest_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *out, bool on_device) {
    REQUIRE(m && poses && out, "gms_map_nearest_poses: null argument (the map, the poses and the output are required)");
    REQUIRE(mi >= 0 && mi < m->n_maps, "gms_map_nearest_poses: map index out of range");
    REQUIRE(P >= 1 && P <= GMS_MAX_PARTICLES, "gms_map_nearest_poses: 1 <= P <= GMS_MAX_PARTICLES poses");
    REQUIRE(max_radius >= 1 && max_radius <= 255, "gms_map_nearest_poses: 1 <= max_radius <= 255 cells");
    REQUIRE(mode == GMS_CLEAR_OCCUPIED || mode == GMS_CLEAR_NOT_FREE, "gms_map_nearest_poses: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(!on_device || ((uintptr_t)out & 3) == 0, "gms_map_nearest_poses_dev: the output must be 4-byte aligned");
    int rc = site_map_check(m, "gms_map_nearest_poses");
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)P * sizeof(gms_nearest), pose_bytes = (size_t)P * 3 * sizeof(float);
    const size_t p_out = st.part(out_bytes), p_poses = st.part(pose_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_poses, poses, pose_bytes);
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(query_map(m, mi), mode, nullptr, nullptr, &plane);
    if (rc) return rc;
    hipLaunchKernelGGL(k_site_poses, dim3((unsigned)((P + SITE_NT / 64 - 1) / (SITE_NT / 64))), dim3(SITE_NT), 0, m->stream, m->gd, plane, gms_plane_wpr(m),
                       st.at(p_poses, poses), P, max_radius, st.at(p_out, out));
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, out_bytes);
    return st.finish(nullptr);
}

extern "C" {

int gms_skeleton_size(const gms_skeleton *q, int32_t *out_w, int32_t *out_h, int64_t *site_bytes, int64_t *skel_bytes) {
    REQUIRE(q, "gms_skeleton: null request");
    REQUIRE(q->w >= 1 && q->h >= 1, "gms_skeleton: w and h must be at least 1");
    REQUIRE(q->x0 >= 0 && q->y0 >= 0, "gms_skeleton: x0 and y0 must not be negative");
    REQUIRE(q->max_radius >= 1 && q->max_radius <= 255, "gms_skeleton: 1 <= max_radius <= 255 cells");
    REQUIRE(q->mode == GMS_CLEAR_OCCUPIED || q->mode == GMS_CLEAR_NOT_FREE, "gms_skeleton: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(q->min_clear >= 1 && q->min_clear <= q->max_radius, "gms_skeleton: 1 <= min_clear <= max_radius cells");
    REQUIRE(q->min_gap >= 2 && q->min_gap <= 2 * q->max_radius, "gms_skeleton: 2 <= min_gap <= 2 * max_radius cells");
    if (out_w) *out_w = q->w;
    if (out_h) *out_h = q->h;
    if (site_bytes) *site_bytes = (int64_t)q->w * q->h * (int64_t)sizeof(uint32_t);
    if (skel_bytes) *skel_bytes = (int64_t)q->w * q->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_skeleton(gms_map *m, int32_t mi, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals) {
    return skeleton(query_map(m, mi), "gms_map_skeleton", q, site, skel, totals, nullptr, false);
}
int gms_map_skeleton_dev(gms_map *m, int32_t mi, const gms_skeleton *q, uint32_t *dev_site, uint16_t *dev_skel, gms_skeleton_totals *dev_totals) {
    return skeleton(query_map(m, mi), "gms_map_skeleton", q, dev_site, dev_skel, dev_totals, nullptr, true);
}
int gms_map_nearest_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *out) {
    return map_nearest_poses(m, mi, poses, P, max_radius, mode, out, false);
}
int gms_map_nearest_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *dev_out) {
    return map_nearest_poses(m, mi, dev_poses, P, max_radius, mode, dev_out, true);
}
int gms_slam_skeleton(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals, int32_t *shown) {
    return skeleton(query_slam(s, which), "gms_slam_skeleton", q, site, skel, totals, shown, false);
}
int gms_slam_skeleton_dev(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *dev_site, uint16_t *dev_skel, gms_skeleton_totals *dev_totals,
                          int32_t *dev_shown) {
    return skeleton(query_slam(s, which), "gms_slam_skeleton", q, dev_site, dev_skel, dev_totals, dev_shown, true);
}

}  // extern "C"
