// gms_skeleton.hip -- nearest-obstacle sites and the free-space skeleton (gridmapslam.h "sites and skeleton"): for every cell of a
// rectangle the obstacle cell of the whole map that is nearest to it under a stated tie rule, and the cells that lie equally far from two
// separated pieces of wall.  All integer arithmetic.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the planes       the clearance fields' (gms_clearance.hip): the map's plane of the request's mode, or the shown particle's, packed
//                    per request (query_plane, gms_query.hip).  The padding of a row holds no bit under either mode.
//   k_site_field     the separable nearest-obstacle transform (gms_nearest_device.h: the stages, the tile, the LDS) keeping the SITE:
//                    the signed offset to the row's nearest set bit, the left one at equal distance, as int16 per staged cell; the
//                    minimum over dy of the 64-bit key d2 << 32 | index, left only once dy^2 > the best d2 so far (KeepSite).
//   k_site_ridge     the three skeleton rules, a lane per cell of the rectangle, over a site field of the rectangle grown by one cell
//                    on every side that lies inside the map (gms_map::d_site_field, grow-only).  Whether a cell is an obstacle and its
//                    d2 are both recomputed from its site (an obstacle cell, and no other, is its own site): no second field and no
//                    plane is read.  Copies the rectangle's sites out, writes the skeleton's d2 and counts the totals -- ballots, one
//                    row of LDS per wavefront, one 64-bit atomic per counter and workgroup.
//   k_site_poses     the same rows under a wavefront per pose, wave_min(uint64_t) takes the smallest key.  No field is made.
//
// Why a second launch for the ridge and not a halo in the site kernel: a workgroup of k_site_field owns one plane word; a column of halo
// on either side is two more words, that is three times stage 1 and three times the LDS for two columns of output.  The ridge pass is a
// gather of five 4-byte words per cell from a field that has just been written (16 MiB at 2048 x 2048: cache-resident) and not the
// expensive part.  A request for sites alone runs no second launch: k_site_field writes the caller's array itself.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include "gms_nearest_device.h"

#define SITE_NT 256                      // lanes of a workgroup of k_site_ridge
#define SITE_RIDGE_ROWS 16               // rows of the rectangle a workgroup of k_site_ridge takes, 64 columns wide

constexpr auto k_site_field = k_nearest_field<KeepSite>;
constexpr auto k_site_poses = k_nearest_poses<KeepSite>;

static_assert(sizeof(gms_skeleton) == 48 && sizeof(gms_skeleton_totals) == 32 && sizeof(gms_nearest) == 8, "the records' layout is part of the interface");

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
        rc = nearest_launch<k_site_field>(m, plane, q->x0, q->y0, q->w, q->h, q->max_radius, d_site, what);
        if (rc) return rc;
    } else {
        rc = nearest_launch<k_site_field>(m, plane, fx0, fy0, fw, fh, q->max_radius, m->d_site_field, what);
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

extern "C" {

int gms_skeleton_size(const gms_skeleton *q, int32_t *out_w, int32_t *out_h, int64_t *site_bytes, int64_t *skel_bytes) {
    REQUIRE(q, "gms_skeleton: null request");
    const int rc = nearest_request_check(q->x0, q->y0, q->w, q->h, q->max_radius, q->mode, "gms_skeleton");
    if (rc) return rc;
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
    return nearest_poses<k_site_poses>(m, mi, poses, P, max_radius, mode, out, false, "gms_map_nearest_poses", site_map_check);
}
int gms_map_nearest_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, gms_nearest *dev_out) {
    return nearest_poses<k_site_poses>(m, mi, dev_poses, P, max_radius, mode, dev_out, true, "gms_map_nearest_poses", site_map_check);
}
int gms_slam_skeleton(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *site, uint16_t *skel, gms_skeleton_totals *totals, int32_t *shown) {
    return skeleton(query_slam(s, which), "gms_slam_skeleton", q, site, skel, totals, shown, false);
}
int gms_slam_skeleton_dev(gms_slam *s, int32_t which, const gms_skeleton *q, uint32_t *dev_site, uint16_t *dev_skel, gms_skeleton_totals *dev_totals,
                          int32_t *dev_shown) {
    return skeleton(query_slam(s, which), "gms_slam_skeleton", q, dev_site, dev_skel, dev_totals, dev_shown, true);
}

}  // extern "C"
