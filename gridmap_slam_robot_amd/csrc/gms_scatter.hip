// gms_scatter.hip -- particle seeding (gridmapslam.h "particle seeding"): slots of a shared-map filter are given poses drawn uniformly
// over the eligible cells of their map -- free, inside a rectangle, not within `inflate` cells of an obstacle.
//
// A translation unit of its own, kernels and C-ABI, layered on the query base beside gms_cast.hip and gms_gain.hip (and on
// gms_reach_inflate for inflate > 0): no kernel of the other units is compiled differently for it.
//
//   k_scat_plane   (1) a lane per 64-bit plane word: eligible = ~not-free & ~blocked & the rectangle's mask; the word and its population
//                  count are stored.  The not-free plane is the query base's (query_plane, packed only when stale); blocked, for
//                  inflate > 0, is the cost-to-go fields' plane (gms_reach_inflate) of the obstacle plane of `mode`.  With inflate = 0
//                  every obstacle of either mode is not free already, so the not-free plane alone decides.
//   gms_launch_scan  (2) the exclusive scan of the counts, every map's at once (gms_query.hip, its batched form): the words' counts
//                  scanned within blocks of GMS_SCAN, the blocks' offsets, and the total, which is M.  A plane of more than GMS_SCAN^2
//                  words is refused.
//   k_scat_draw    (3) a lane per slot: the Philox block, r = mulhi64(c0:c1, M), the word that holds rank r, its r'-th set bit, the
//                  pose, its trig and the weight.  The prefix of word w is top[w / GMS_SCAN] + pre[w] (scan_prefix); a workgroup stages that sum for
//                  every (1 << shift)-th word in LDS (at most SCT_STAGE entries, shift >= SCT_SHIFT_MIN), searches there first -- the
//                  first steps of all lanes read the same few entries, which broadcast; the last ones scatter over the 32 banks of a
//                  half-wave as 32 random addresses do, a few lanes to a bank at worst -- and finishes within the (1 << shift) words
//                  of its bracket in memory.  The set bit is found by halving population counts.  M comes from device memory.
//
// The table -- the eligible plane, the scanned counts, the blocks' offsets and M, for every map of the handle -- stays on the gms_map
// with the request it was built for (rectangle, inflate, mode) and is reused until logData moves (map_planes_stale): a scatter on an
// unchanged map is launch (3) alone.
#undef GMS_STAMPS
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "gms_regions.h"

#define SCT_NT 256
#define SCT_STAGE 8192                   // staged prefix entries at most: 32 KiB of LDS
#define SCT_SHIFT_MIN 5                  // every 32nd word is staged, or a coarser power of two where that exceeds SCT_STAGE
#define SCT_BOUND 262144.0               // (|position| + extent) / resolution at most, per axis (gridmapslam.h: the cell guarantee)

static_assert(sizeof(gms_scatter) == 40, "gms_scatter is ten int32_t");

// nf, blocked (NULL: none): ONE map's planes, H rows of wpr64 words; elig, cnt: that map's part of the table
__global__ void __launch_bounds__(SCT_NT)
k_scat_plane(const uint64_t *__restrict__ nf, const uint64_t *__restrict__ blocked, int32_t wpr64, int32_t words, int32_t x0, int32_t y0, int32_t w,
             int32_t h, uint64_t *__restrict__ elig, uint32_t *__restrict__ cnt) {
    const int32_t i = (int32_t)blockIdx.x * SCT_NT + (int32_t)threadIdx.x;
    if (i >= words) return;
    const int32_t y = i / wpr64, xw = i - y * wpr64;
    uint64_t e = 0ull;
    if (y >= y0 && y < y0 + h) {
        const int32_t lo = max(x0 - xw * 64, 0), hi = min(x0 + w - xw * 64, 64);      // the rectangle's bits [lo, hi) of this word
        if (hi > lo) {
            const uint64_t mask = (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
            e = ~nf[i] & mask;
            if (blocked) e &= ~blocked[i];
        }
    }
    elig[i] = e;
    cnt[i] = (uint32_t)__popcll(e);
}

// what k_scat_draw needs of the table and the request
struct ScatDraw {
    const uint64_t *elig;       // [n_maps][words]
    const uint32_t *pre;        // [n_maps][words] the counts scanned within blocks of GMS_SCAN
    const uint32_t *top;        // [n_maps][nb] the blocks' offsets
    const uint32_t *M;          // [n_maps]
    int32_t words, wpr64, nb, shift, nst;
    int32_t n, first, count, jitter;
    int64_t offset;             // global index of slot 0
    uint64_t seed, sequence;
    double w0;                  // 1.0 / n_global
};

// grid (workgroups over the slots, maps); dynamic LDS: nst staged entries
__global__ void __launch_bounds__(SCT_NT)
k_scat_draw(GridDev g, ScatDraw a, float *__restrict__ pose, float *__restrict__ cs, double *__restrict__ wgt, double *__restrict__ logw) {
    extern __shared__ uint32_t s_pre[];
    const int32_t mi = (int32_t)blockIdx.y, tid = (int32_t)threadIdx.x;
    const uint32_t M = a.M[mi];
    if (M == 0u) return;                                                        // (uniform) nothing eligible: nothing written
    const uint64_t *__restrict__ elig = a.elig + (size_t)mi * (size_t)a.words;
    const uint32_t *__restrict__ pre = a.pre + (size_t)mi * (size_t)a.words, *__restrict__ top = a.top + (size_t)mi * (size_t)a.nb;
    for (int32_t j = tid; j < a.nst; j += SCT_NT) s_pre[j] = scan_prefix(pre, top, j << a.shift);
    __syncthreads();
    const int32_t i = (int32_t)blockIdx.x * SCT_NT + tid;
    if (i >= a.count) return;
    const int32_t slot = a.first + i;
    const uint64_t index = (uint64_t)(a.offset + slot) + ((uint64_t)mi << 40);  // the motion model's counter layout (motion_body)
    uint32_t c[4] = { (uint32_t)index, (uint32_t)(index >> 32), (uint32_t)a.sequence, (uint32_t)(a.sequence >> 32) };
    uint32_t k[2] = { (uint32_t)a.seed, (uint32_t)(a.seed >> 32) };
#pragma unroll
    for (int r = 0; r < 10; r++) {                                              // Philox4x32-10
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    const uint32_t r = (uint32_t)__umul64hi(((uint64_t)c[0] << 32) | c[1], (uint64_t)M);          // < M
    // the last staged entry with prefix <= r (entry 0 is 0), then the last word of its bracket with prefix <= r: since the prefix
    // of the next word is larger, that word holds rank r
    int32_t lo = 0, hi = a.nst;
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (s_pre[mid] <= r) lo = mid; else hi = mid;
    }
    lo <<= a.shift;
    hi = min(lo + (1 << a.shift), a.words);
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (scan_prefix(pre, top, mid) <= r) lo = mid; else hi = mid;
    }
    uint32_t kth = r - scan_prefix(pre, top, lo);                               // < popcount of the word
    uint64_t v = elig[lo];
    int32_t bit = 0;
#pragma unroll
    for (int32_t half = 32; half >= 1; half >>= 1) {                            // the kth set bit: halve the population counts
        const uint32_t below = (uint32_t)__popcll(v & ((1ull << half) - 1ull));
        if (kth >= below) { kth -= below; v >>= half; bit += half; }
    }
    const int32_t cy = lo / a.wpr64, cx = (lo - cy * a.wpr64) * 64 + bit;
    float jx = 0.5f, jy = 0.5f;
    if (a.jitter) {                                                             // multiples of 2^-19 in [1/16, 15/16): exact
        jx = (float)(32768u + 7u * (c[2] >> 16)) * 0x1p-19f;
        jy = (float)(32768u + 7u * (c[2] & 0xFFFFu)) * 0x1p-19f;
    }
    const float fx = (float)cx + jx, fy = (float)cy + jy;
    const float x = (float)(g.posx + (double)fx * g.res), y = (float)(g.posy + (double)fy * g.res);       // (the products are exact)
    const float th = (float)(((double)(c[3] >> 8) - 8388607.5) * (3.141592653589793 * 0x1p-23));
    float fc, fs;
    pose_trig(th, fc, fs);
    const size_t gi = (size_t)mi * (size_t)a.n + (size_t)slot;
    pose[3 * gi] = x; pose[3 * gi + 1] = y; pose[3 * gi + 2] = th;
    cs[2 * gi] = fc; cs[2 * gi + 1] = fs;
    wgt[gi] = a.w0;
    logw[gi] = 0.0;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int32_t scat_shift(const gms_map *m, int64_t words) {
    int32_t shift = std::max(SCT_SHIFT_MIN, m->scatter_shift);
    while (((words + ((int64_t)1 << shift) - 1) >> shift) > SCT_STAGE) shift++;
    return shift;
}

// the table of every map of the handle for request sc, unless the handle holds exactly that
static int scat_table(gms_map *m, const gms_scatter *sc) {
    gms_flush_apply(m);                                                         // (it moves logData: the table is stale behind it)
    auto &t = m->scatter;
    const int32_t mode = sc->inflate > 0 ? sc->mode : GMS_CLEAR_NOT_FREE;       // (inflate = 0: both modes give the free cells)
    if (t.current && t.x0 == sc->x0 && t.y0 == sc->y0 && t.w == sc->w && t.h == sc->h && t.inflate == sc->inflate && t.mode == mode) return GMS_OK;
    const int32_t wpr64 = (m->gd.W + 63) / 64, words = m->gd.H * wpr64, nb = (words + GMS_SCAN - 1) / GMS_SCAN;
    const size_t all = (size_t)m->n_maps * (size_t)words;
    int rc = gms_dev_alloc(&t.d_elig, all * sizeof(uint64_t), "gms_pf_scatter", "the eligible plane");
    if (!rc) rc = gms_dev_alloc(&t.d_pre, (all + (size_t)m->n_maps * (size_t)(nb + 1)) * sizeof(uint32_t), "gms_pf_scatter", "the plane's scanned counts");
    if (rc) return rc;
    uint32_t *d_top = t.d_pre + all, *d_M = d_top + (size_t)m->n_maps * (size_t)nb;
    t.current = 0;
    for (int32_t mi = 0; mi < m->n_maps; mi++) {
        const QuerySource src = query_map(m, mi);
        const uint32_t *nf = nullptr, *blocked = nullptr;
        rc = query_plane(src, GMS_CLEAR_NOT_FREE, nullptr, nullptr, &nf);
        if (!rc && sc->inflate > 0) {
            const uint32_t *obstacles = nf;
            if (mode == GMS_CLEAR_OCCUPIED) rc = query_plane(src, GMS_CLEAR_OCCUPIED, nullptr, nullptr, &obstacles);
            if (!rc) rc = gms_reach_inflate(m, obstacles, sc->inflate, mode, &blocked);           // (one scratch plane: map by map)
        }
        if (rc) return rc;
        hipLaunchKernelGGL(k_scat_plane, dim3((unsigned)((words + SCT_NT - 1) / SCT_NT)), dim3(SCT_NT), 0, m->stream, reinterpret_cast<const uint64_t *>(nf),
                           reinterpret_cast<const uint64_t *>(blocked), wpr64, words, sc->x0, sc->y0, sc->w, sc->h, t.d_elig + (size_t)mi * (size_t)words,
                           t.d_pre + (size_t)mi * (size_t)words);
    }
    gms_launch_scan(m->stream, t.d_pre, nullptr, words, d_top, d_M, m->n_maps, words, nb);
    HIPCHK(hipGetLastError());
    t.x0 = sc->x0; t.y0 = sc->y0; t.w = sc->w; t.h = sc->h; t.inflate = sc->inflate; t.mode = mode;
    t.current = 1;
    t.builds++;
    return GMS_OK;
}

extern "C" {

int gms_scatter_check(const gms_scatter *sc) {
    REQUIRE(sc, "gms_scatter: null request");
    REQUIRE(sc->w >= 1 && sc->h >= 1, "gms_scatter: w and h must be at least 1");
    REQUIRE(sc->x0 >= 0 && sc->y0 >= 0, "gms_scatter: x0 and y0 must not be negative");
    REQUIRE(sc->inflate >= 0 && sc->inflate <= 255, "gms_scatter: 0 <= inflate <= 255 cells");
    REQUIRE(sc->mode == GMS_CLEAR_OCCUPIED || sc->mode == GMS_CLEAR_NOT_FREE, "gms_scatter: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(sc->first >= 0 && sc->count >= 1, "gms_scatter: first >= 0 and count >= 1 slots");
    REQUIRE(sc->jitter == 0 || sc->jitter == 1, "gms_scatter: jitter must be 0 or 1");
    return GMS_OK;
}

int gms_pf_scatter(gms_pf *pf, const gms_scatter *sc, uint64_t seed, uint64_t sequence, int64_t *n_eligible) {
    if (!pf || !sc) return gms_fail(GMS_ERR_INVALID, "gms_pf_scatter: null argument (the filter and the request are required)");
    int rc = gms_scatter_check(sc);
    if (rc) return rc;
    if (pf->slam_owned)
        return gms_fail(GMS_ERR_STATE, "gms_pf_scatter: this filter's particles own maps (gms_slam): there is no one map to draw from");
    if ((int64_t)sc->first + sc->count > pf->n)
        return gms_fail(GMS_ERR_INVALID, "gms_pf_scatter: the slots [%d, %d + %d) leave the filter's %d", sc->first, sc->first, sc->count, pf->n);
    gms_map *m = pf->map;
    rc = gms_rect_check(sc->x0, sc->y0, sc->w, sc->h, m->gd.W, m->gd.H, "gms_pf_scatter");
    if (rc) return rc;
    const GridDev &g = m->gd;
    if ((fabs(g.posx) + (double)g.W * g.res) / g.res > SCT_BOUND || (fabs(g.posy) + (double)g.H * g.res) / g.res > SCT_BOUND)
        return gms_fail(GMS_ERR_INVALID, "gms_pf_scatter: (|position| + extent) / resolution exceeds 2^18 cells: a pose's cell would not be certain");
    const int64_t words = (int64_t)g.H * ((g.W + 63) / 64);
    if (words > (int64_t)GMS_SCAN * GMS_SCAN)
        return gms_fail(GMS_ERR_INVALID, "gms_pf_scatter: a plane of %lld words exceeds the two scan levels' %d", (long long)words, GMS_SCAN * GMS_SCAN);
    HIPCHK(hipSetDevice(m->device));
    rc = scat_table(m, sc);
    if (rc) return rc;
    gms_launch_pf_combine(pf);                                                  // the other slots' weights out of a pending scoring pass
    const auto &t = m->scatter;
    const int32_t nb = (int32_t)((words + GMS_SCAN - 1) / GMS_SCAN), shift = scat_shift(m, words);
    const size_t all = (size_t)m->n_maps * (size_t)words;
    ScatDraw a;
    a.elig = t.d_elig; a.pre = t.d_pre; a.top = t.d_pre + all; a.M = a.top + (size_t)m->n_maps * (size_t)nb;
    a.words = (int32_t)words; a.wpr64 = (g.W + 63) / 64; a.nb = nb; a.shift = shift;
    a.nst = (int32_t)((words + ((int64_t)1 << shift) - 1) >> shift);
    a.n = pf->n; a.first = sc->first; a.count = sc->count; a.jitter = sc->jitter;
    a.offset = pf->offset; a.seed = seed; a.sequence = sequence;
    a.w0 = 1.0 / (double)pf->n_global;
    hipLaunchKernelGGL(k_scat_draw, dim3((unsigned)((sc->count + SCT_NT - 1) / SCT_NT), (unsigned)pf->n_maps), dim3(SCT_NT), (size_t)a.nst * sizeof(uint32_t),
                       m->stream, m->gd, a, pf->d_pose, pf->d_cs, pf->d_w, pf->d_logw);
    HIPCHK(hipGetLastError());
    pf_particles_changed(pf);                                                   // gms_pf_set_poses, then
    pf_weights_set(pf);                                                         // gms_pf_set_weights
    if (n_eligible) {
        std::vector<uint32_t> M((size_t)m->n_maps);
        HIPCHK(hipMemcpyAsync(M.data(), a.M, M.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        for (int32_t mi = 0; mi < m->n_maps; mi++) n_eligible[mi] = (int64_t)M[(size_t)mi];
    }
    return GMS_OK;
}

int gms_map_scatter_table_builds(const gms_map *m, int64_t *builds) {
    REQUIRE(m && builds, "gms_map_scatter_table_builds: null argument");
    *builds = m->scatter.builds;
    return GMS_OK;
}

}  // extern "C"
