// gms_frontier.hip -- frontier regions (gridmapslam.h "frontier regions"): the FREE cells with an UNKNOWN axis neighbour inside the map,
// grouped into maximal 8-connected regions; per region its anchor (the member of the smallest linear index), count, box, coordinate sums
// and -- with a cost-to-go field -- the member that is cheapest to drive to.  All integer arithmetic; every output is unique, so
// however the unions and the atomics are scheduled the result is the same.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   k_front_plane       the frontier plane in the casts' layout (rows of 64-bit words, the padding zero), a lane per word: unknown = the
//                       second plane and not the casts' plane; a word's east / west shifts carry a bit from the neighbouring words, north
//                       and south are the words of the rows above and below; free = not the second plane; inflate > 0: and not the
//                       cost-to-go fields' blocked plane (gms_reach_inflate).  Both planes are read in place (query_plane; a gms_slam's:
//                       the shown particle's, packed per request, twice).
//   k_front_tiles, k_front_merge   the 8-connected labelling: region_tile_label and region_border_merge of gms_regions.h with the
//                       diagonal links -- the tile-local union in LDS, then the cells behind a tile border united with their (up to)
//                       three neighbours across it.
//   k_front_flatten     a wavefront per plane word: every frontier cell chases to its root and stores it; the ballot of "I am my own
//                       root" is the root plane's word, its popcount the word's count.
//   gms_launch_scan     the exclusive scan of those counts: the roots in linear order = the regions in anchor order; the total is the
//                       number of regions.
//   k_front_table_init, k_front_reduce, k_front_finish
//                       the table: a wavefront per plane word looks up every cell's region index, and the lanes that share one combine
//                       (wave_each_key: count, box and sums from the group's ballot alone; the goal key cost << 32 | index by a
//                       butterfly) before ONE lane issues the atomics -- integer min / max / add only.  The finish decodes the goal and
//                       flags count >= min_size.
//   gms_launch_scan, k_front_emit   the flags scanned, the kept regions' records stored in order, the first `cap` of them.
//   k_front_labels      the label rectangle: the label where the plane has a bit, GMS_FRONTIER_NONE elsewhere.
//
// The union, the labelling, the group loop, the wavefront minimum and the scan's look-up are the shared ones of gms_regions.h; the scan
// itself is the query base's (gms_query.hip).
#undef GMS_STAMPS
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_regions.h"

#define FRT_T REGION_T                   // tile edge in cells = cells of a plane word
#define FRT_NT REGION_NT
#define FRT_CAP0 4096                    // regions the handle's table holds at first (a multiple of GMS_SCAN)
#define FRT_NONE 0xffffffffu
#define FRT_NO_GOAL 0xffffffffffffffffull

static_assert(GMS_FRONTIER_NONE == FRT_NONE, "the header's constant is the kernels'");
static_assert(sizeof(gms_frontiers) == 32 && sizeof(gms_frontier) == 56 && offsetof(gms_frontier, count) == 8 && offsetof(gms_frontier, goal_cost) == 12 &&
              offsetof(gms_frontier, min_x) == 16 && offsetof(gms_frontier, max_x) == 24 && offsetof(gms_frontier, goal_x) == 32 &&
              offsetof(gms_frontier, sum_x) == 40 && offsetof(gms_frontier, sum_y) == 48, "the header fixes the record's offsets");
static_assert(FRT_CAP0 % GMS_SCAN == 0, "the table's parts stay 8-byte aligned");

// occ, nf, blocked (NULL: inflate == 0): ONE map's planes, H rows of wpr64 words; out likewise
__global__ void __launch_bounds__(FRT_NT)
k_front_plane(const uint64_t *__restrict__ occ, const uint64_t *__restrict__ nf, const uint64_t *__restrict__ blocked, int32_t W, int32_t H, int32_t wpr64,
              uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FRT_NT + threadIdx.x;
    if (i >= (int64_t)H * wpr64) return;
    const int32_t y = (int32_t)(i / wpr64), wx = (int32_t)(i - (int64_t)y * wpr64);
    auto unknown = [&](int32_t yy, int32_t ww) -> uint64_t {                    // (off the map: nothing is unknown)
        if (yy < 0 || yy >= H || ww < 0 || ww >= wpr64) return 0ull;
        const size_t k = (size_t)yy * (size_t)wpr64 + (size_t)ww;
        return nf[k] & ~occ[k];
    };
    const uint64_t u = unknown(y, wx);
    const uint64_t beside = (u << 1) | (unknown(y, wx - 1) >> 63) | (u >> 1) | (unknown(y, wx + 1) << 63) | unknown(y - 1, wx) | unknown(y + 1, wx);
    const uint64_t on_map = wx == wpr64 - 1 && (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
    uint64_t f = ~nf[i] & on_map & beside;
    if (blocked) f &= ~blocked[i];
    out[i] = f;
}

// plane: the frontier plane; label [H][W]; grid (ntx, nty)
__global__ void __launch_bounds__(FRT_NT)
k_front_tiles(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *__restrict__ label) {
    region_tile_label<true>(plane, wpr64, W, H, label);
}

// a lane per cell behind a tile border, united with its (up to) three neighbours across it
__global__ void __launch_bounds__(FRT_NT)
k_front_merge(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, int32_t ntx, int32_t nty, uint32_t *label) {
    region_border_merge<true>(plane, wpr64, W, H, ntx, nty, label);
}

// a wavefront per word of the plane; roots: the root plane; wcount [words]
__global__ void __launch_bounds__(FRT_NT)
k_front_flatten(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *label, uint64_t *__restrict__ roots,
                uint32_t *__restrict__ wcount) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (FRT_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const uint64_t bits = plane[word];
    bool root = false;
    if ((bits >> lane) & 1ull) {
        const int32_t y = (int32_t)(word / wpr64), x = (int32_t)(word - (int64_t)y * wpr64) * 64 + lane;
        const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x, r = region_find(label, c);
        if (r != c) __atomic_store_n(label + c, r, __ATOMIC_RELAXED);           // (another lane's chase reads the old parent or the root: both lead there)
        root = r == c;
    }
    const uint64_t rb = __ballot(root);
    if (lane == 0) {
        roots[word] = rb;
        wcount[word] = (uint32_t)__popcll(rb);
    }
}

// the first min(ctl[0], cap) entries of the table
__global__ void __launch_bounds__(FRT_NT)
k_front_table_init(gms_frontier *__restrict__ rec, unsigned long long *__restrict__ goal, const uint32_t *__restrict__ ctl, int32_t cap) {
    const int64_t n = std::min<int64_t>((int64_t)ctl[0], cap);
    for (int64_t i = (int64_t)blockIdx.x * FRT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FRT_NT) {
        rec[i] = gms_frontier{0, 0, 0, GMS_REACH_FAR, INT_MAX, INT_MAX, -1, -1, -1, -1, 0, 0};
        goal[i] = FRT_NO_GOAL;
    }
}

// a wavefront per word of the plane.  roots / wscan / wblocks: the root plane and the scan of its counts; cost (may be NULL) [H][W];
// regions behind cap are left out (the host grows the table and runs this again)
__global__ void __launch_bounds__(FRT_NT)
k_front_reduce(const uint64_t *__restrict__ plane, const uint64_t *__restrict__ roots, const uint32_t *__restrict__ wscan, const uint32_t *__restrict__ wblocks,
               int32_t wpr64, int32_t W, int32_t H, const uint32_t *__restrict__ label, const uint16_t *__restrict__ cost, gms_frontier *rec,
               unsigned long long *goal, int32_t cap) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (FRT_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const uint64_t bits = plane[word];
    if (bits == 0ull) return;                                                   // (uniform)
    const int32_t y = (int32_t)(word / wpr64), xw = (int32_t)(word - (int64_t)y * wpr64) * 64, x = xw + lane;
    uint32_t region = FRT_NONE;
    uint64_t key = FRT_NO_GOAL;
    if ((bits >> lane) & 1ull) {
        const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x, r = label[c];
        const uint32_t ry = r / (uint32_t)W, rx = r - ry * (uint32_t)W;
        const size_t rw = (size_t)ry * (size_t)wpr64 + (size_t)(rx >> 6);
        region = scan_prefix(wscan, wblocks, rw) + (uint32_t)__popcll(roots[rw] & ((1ull << (rx & 63u)) - 1ull));
        if (region >= (uint32_t)cap) region = FRT_NONE;
        else if (r == c) { rec[region].anchor_x = x; rec[region].anchor_y = y; }                  // (the root alone writes these)
        if (cost) {
            const uint32_t v = cost[c];
            if (v != (uint32_t)GMS_REACH_FAR) key = ((uint64_t)v << 32) | c;
        }
    }
    wave_each_key(region, FRT_NONE, [&](uint32_t R, bool in, uint64_t grp, bool leader) {
        const uint64_t best = cost ? wave_min(in ? key : (uint64_t)FRT_NO_GOAL) : FRT_NO_GOAL;
        if (!leader) return;
        const int32_t n = __popcll(grp);
        gms_frontier *q = rec + R;
        atomicAdd(&q->count, n);
        atomicMin(&q->min_x, xw + __builtin_ctzll(grp));
        atomicMax(&q->max_x, xw + 63 - __builtin_clzll(grp));
        atomicMin(&q->min_y, y);
        atomicMax(&q->max_y, y);
        atomicAdd(reinterpret_cast<unsigned long long *>(&q->sum_x), (unsigned long long)((int64_t)n * xw + region_bit_sum(grp)));
        atomicAdd(reinterpret_cast<unsigned long long *>(&q->sum_y), (unsigned long long)((int64_t)n * y));
        if (best != FRT_NO_GOAL) atomicMin(goal + R, (unsigned long long)best);
    });
}

// the goals decoded; kept [i] = count >= min_size
__global__ void __launch_bounds__(FRT_NT)
k_front_finish(gms_frontier *__restrict__ rec, const unsigned long long *__restrict__ goal, const uint32_t *__restrict__ ctl, int32_t cap, int32_t min_size,
               int32_t W, uint32_t *__restrict__ kept) {
    const int64_t n = std::min<int64_t>((int64_t)ctl[0], cap);
    for (int64_t i = (int64_t)blockIdx.x * FRT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FRT_NT) {
        const uint64_t k = goal[i];
        if (k != FRT_NO_GOAL) {
            const uint32_t c = (uint32_t)k, gy = c / (uint32_t)W;
            rec[i].goal_x = (int32_t)(c - gy * (uint32_t)W);
            rec[i].goal_y = (int32_t)gy;
            rec[i].goal_cost = (int32_t)(k >> 32);
        }
        kept[i] = rec[i].count >= min_size ? 1u : 0u;
    }
}

// kept / kblocks: the scan of the flags; out [out_cap]
__global__ void __launch_bounds__(FRT_NT)
k_front_emit(const gms_frontier *__restrict__ rec, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ kblocks, const uint32_t *__restrict__ ctl,
             int32_t cap, int32_t min_size, gms_frontier *__restrict__ out, int32_t out_cap) {
    const int64_t n = std::min<int64_t>((int64_t)ctl[0], cap);
    for (int64_t i = (int64_t)blockIdx.x * FRT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FRT_NT) {
        if (rec[i].count < min_size) continue;
        const uint32_t at = scan_prefix(kept, kblocks, i);
        if (at < (uint32_t)out_cap) out[at] = rec[i];
    }
}

// out [h][w]
__global__ void __launch_bounds__(FRT_NT)
k_front_labels(const uint64_t *__restrict__ plane, int32_t wpr64, const uint32_t *__restrict__ label, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
               uint32_t *__restrict__ out) {
    const int64_t n = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * FRT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * FRT_NT) {
        const int32_t y = y0 + (int32_t)(i / w), x = x0 + (int32_t)(i % w);
        const bool on = (plane[(size_t)y * (size_t)wpr64 + (size_t)(x >> 6)] >> (x & 63)) & 1ull;
        out[i] = on ? label[(size_t)y * (size_t)W + (size_t)x] : FRT_NONE;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the checks the four entry points share behind the source's, before anything is touched; *bytes: the label rectangle's size
static int front_args(const gms_frontiers *f, int32_t W, int32_t H, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap, bool on_device,
                      const char *what, int64_t *bytes) {
    int rc = gms_frontiers_size(f, nullptr, nullptr, bytes);
    if (!rc) rc = gms_rect_check(f->x0, f->y0, f->w, f->h, W, H, what);
    if (rc) return rc;
    if ((int64_t)W * H >= (int64_t)FRT_NONE) return gms_fail(GMS_ERR_INVALID, "%s: a map of %d x %d cells exceeds a 32-bit label", what, W, H);
    const char *dev = on_device ? "_dev" : "";
    if (cap < 0 || (cap > 0 && !records)) return gms_fail(GMS_ERR_INVALID, "%s%s: cap >= 0, and records unless cap == 0", what, dev);
    if (on_device && ((uintptr_t)cost & 1 || (uintptr_t)labels & 3 || (uintptr_t)records & 7))
        return gms_fail(GMS_ERR_INVALID, "%s%s: the cost field must be 2-byte aligned, the labels 4-byte aligned, the records 8-byte aligned", what, dev);
    return GMS_OK;
}

static inline size_t front_table_bytes(int32_t cap) {
    return (size_t)cap * (sizeof(gms_frontier) + sizeof(uint64_t) + sizeof(uint32_t)) + ((size_t)cap / GMS_SCAN + 1) * sizeof(uint32_t);
}
struct FrontTable {
    gms_frontier *rec;
    unsigned long long *goal;
    uint32_t *kept, *kblocks;
};
static inline FrontTable front_table(const gms_map *m) {
    FrontTable t;
    const size_t cap = (size_t)m->front_cap;
    t.rec = reinterpret_cast<gms_frontier *>(m->d_front_table);
    t.goal = reinterpret_cast<unsigned long long *>(m->d_front_table + cap * sizeof(gms_frontier));
    t.kept = reinterpret_cast<uint32_t *>(m->d_front_table + cap * (sizeof(gms_frontier) + sizeof(uint64_t)));
    t.kblocks = t.kept + cap;
    return t;
}
// a table of at least `need` regions (nothing of the handle's is in flight on it: the caller has waited)
static int front_table_grow(gms_map *m, int64_t need) {
    const int64_t cap = (std::max<int64_t>(need, FRT_CAP0) + GMS_SCAN - 1) / GMS_SCAN * GMS_SCAN;
    if (cap > INT_MAX / 2) return gms_fail(GMS_ERR_NOMEM, "gms_frontiers: a table of %lld regions", (long long)cap);
    return gms_dev_grow(&m->d_front_table, &m->front_cap, cap, GMS_SCAN, nullptr, [](size_t c) { return front_table_bytes((int32_t)c); }, "gms_frontiers", "the region table");
}

// what a request needs on the handle (a handle's W and H never change: only the table ever grows)
static int front_buffers(gms_map *m, bool per_particle) {
    const size_t plane_bytes = (size_t)m->gd.H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), words = plane_bytes / sizeof(uint64_t);
    int rc = gms_dev_alloc(&m->d_front_plane, 2 * plane_bytes, "gms_frontiers", "the frontier plane and the root plane");
    if (!rc) rc = gms_dev_alloc(&m->d_front_label, (size_t)m->gd.cells * sizeof(uint32_t), "gms_frontiers", "the label field");
    if (!rc) rc = gms_dev_alloc(&m->d_front_wscan, (words + words / GMS_SCAN + 1) * sizeof(uint32_t), "gms_frontiers", "the root plane's scan");
    if (!rc) rc = gms_dev_alloc(&m->d_front_ctl, 2 * sizeof(uint32_t), "gms_frontiers", "the region counts");
    if (!rc && per_particle) rc = gms_dev_alloc(&m->d_front_nf, plane_bytes, "gms_frontiers", "the particle's second plane");
    if (!rc) rc = front_table_grow(m, FRT_CAP0);
    if (!rc) rc = gms_pinned_alloc(&m->h_front_ctl, 2 * sizeof(uint32_t), "gms_frontiers");
    return rc;
}

// The regions of ONE map's two planes (of logData as it stands) into the caller's device buffers; the handle's buffers exist.  Waits
// on the stream once -- twice where the table has to grow -- and leaves the numbers of regions in h_front_ctl.
static int front_run(gms_map *m, const uint32_t *d_occ, const uint32_t *d_nf, const gms_frontiers *f, const uint16_t *d_cost, uint32_t *d_labels,
                     gms_frontier *d_records, int32_t cap) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64, ntx = (W + FRT_T - 1) / FRT_T, nty = (H + FRT_T - 1) / FRT_T;
    if (nty > 65535) return gms_fail(GMS_ERR_INVALID, "gms_frontiers: a map of %d rows exceeds one launch", H);
    const uint32_t *d_blocked = nullptr;
    if (f->inflate > 0) {
        int rc = gms_reach_inflate(m, d_occ, f->inflate, GMS_CLEAR_OCCUPIED, &d_blocked);
        if (rc) return rc;
    }
    const int64_t words = (int64_t)H * wpr64;
    uint64_t *plane = reinterpret_cast<uint64_t *>(m->d_front_plane), *roots = plane + words;
    uint32_t *wscan = m->d_front_wscan, *wblocks = wscan + words, *ctl = m->d_front_ctl, *label = m->d_front_label;
    hipStream_t st = m->stream;
    hipLaunchKernelGGL(k_front_plane, dim3((unsigned)((words + FRT_NT - 1) / FRT_NT)), dim3(FRT_NT), 0, st, reinterpret_cast<const uint64_t *>(d_occ),
                       reinterpret_cast<const uint64_t *>(d_nf), reinterpret_cast<const uint64_t *>(d_blocked), W, H, wpr64, plane);
    hipLaunchKernelGGL(k_front_tiles, dim3((unsigned)ntx, (unsigned)nty), dim3(FRT_NT), 0, st, plane, wpr64, W, H, label);
    const int64_t border = (int64_t)(ntx - 1) * H + (int64_t)(nty - 1) * W;
    if (border > 0)
        hipLaunchKernelGGL(k_front_merge, dim3((unsigned)((border + FRT_NT - 1) / FRT_NT)), dim3(FRT_NT), 0, st, plane, wpr64, W, H, ntx, nty, label);
    const unsigned word_waves = (unsigned)((words + FRT_NT / 64 - 1) / (FRT_NT / 64));
    hipLaunchKernelGGL(k_front_flatten, dim3(word_waves), dim3(FRT_NT), 0, st, plane, wpr64, W, H, label, roots, wscan);
    gms_launch_scan(st, wscan, nullptr, words, wblocks, ctl);
    HIPCHK(hipGetLastError());
    if (d_labels) {
        const int64_t n = (int64_t)f->w * f->h;
        hipLaunchKernelGGL(k_front_labels, dim3(gms_grid(n, FRT_NT, 4096)), dim3(FRT_NT), 0, st, plane, wpr64, label, W, f->x0, f->y0, f->w, f->h, d_labels);
        HIPCHK(hipGetLastError());
    }
    for (int32_t pass = 0;; pass++) {
        const int32_t tcap = m->front_cap;
        const FrontTable t = front_table(m);
        const unsigned tgrid = gms_grid(tcap, FRT_NT, 1024);
        hipLaunchKernelGGL(k_front_table_init, dim3(tgrid), dim3(FRT_NT), 0, st, t.rec, t.goal, ctl, tcap);
        hipLaunchKernelGGL(k_front_reduce, dim3(word_waves), dim3(FRT_NT), 0, st, plane, roots, wscan, wblocks, wpr64, W, H, label, d_cost, t.rec, t.goal, tcap);
        hipLaunchKernelGGL(k_front_finish, dim3(tgrid), dim3(FRT_NT), 0, st, t.rec, t.goal, ctl, tcap, f->min_size, W, t.kept);
        gms_launch_scan(st, t.kept, ctl, tcap, t.kblocks, ctl + 1);
        if (cap > 0) hipLaunchKernelGGL(k_front_emit, dim3(tgrid), dim3(FRT_NT), 0, st, t.rec, t.kept, t.kblocks, ctl, tcap, f->min_size, d_records, cap);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(m->h_front_ctl, ctl, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if ((int64_t)m->h_front_ctl[0] <= tcap) return GMS_OK;
        if (pass > 0) return gms_fail(GMS_ERR_INTERNAL, "gms_frontiers: %u regions after the table grew to %d", m->h_front_ctl[0], tcap);
        int rc = front_table_grow(m, (int64_t)m->h_front_ctl[0]);                // (more regions than the table held: steps 6 and 7 again)
        if (rc) return rc;
    }
}

// the regions of one map of a shared handle or of the shown particle of a per-particle one; `shown` exists for a particle only
static int frontiers(QuerySource src, const char *what, const gms_frontiers *f, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap,
                     int32_t *n_found, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !f) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle and the request are required)", what);
    gms_map *m = src.m;
    int64_t bytes = 0;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (!rc) rc = front_args(f, m->gd.W, m->gd.H, cost, labels, records, cap, on_device, what, &bytes);
    if (rc) return rc;
    src.filter = f->filter;
    if (src.s && (rc = query_check(src, what, "gms_frontiers.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    rc = front_buffers(m, src.s != nullptr);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t label_bytes = labels ? (size_t)bytes : 0, cost_bytes = cost ? (size_t)m->gd.cells * sizeof(uint16_t) : 0;
    const size_t p_labels = st.part(label_bytes), p_records = st.part((size_t)cap * sizeof(gms_frontier)), p_cost = st.part(cost_bytes);
    rc = st.open();
    if (!rc && cost) rc = st.up(p_cost, cost, cost_bytes);
    if (rc) return rc;
    // both predicates: the map's two planes in place; a particle's packed per request, the second into d_front_nf
    const uint32_t *occ = nullptr, *nf = nullptr;
    rc = query_plane(src, GMS_CLEAR_OCCUPIED, st.shown(shown), nullptr, &occ);
    if (!rc) rc = query_plane(src, GMS_CLEAR_NOT_FREE, nullptr, src.s ? m->d_front_nf : nullptr, &nf);
    if (!rc)
        rc = front_run(m, occ, nf, f, cost ? st.at(p_cost, cost) : nullptr, labels ? st.at(p_labels, labels) : nullptr, cap > 0 ? st.at(p_records, records) : nullptr, cap);
    if (rc) return rc;
    if (n_found) *n_found = (int32_t)m->h_front_ctl[1];
    st.fetch(labels, p_labels, label_bytes);
    st.fetch(records, p_records, (size_t)std::min<int64_t>(m->h_front_ctl[1], cap) * sizeof(gms_frontier));
    return st.finish(shown);
}

extern "C" {

int gms_frontiers_size(const gms_frontiers *f, int32_t *out_w, int32_t *out_h, int64_t *bytes) {
    REQUIRE(f, "gms_frontiers: null request");
    REQUIRE(f->w >= 1 && f->h >= 1, "gms_frontiers: w and h must be at least 1");
    REQUIRE(f->x0 >= 0 && f->y0 >= 0, "gms_frontiers: x0 and y0 must not be negative");
    REQUIRE(f->min_size >= 1, "gms_frontiers: min_size must be at least 1");
    REQUIRE(f->inflate >= 0 && f->inflate <= 255, "gms_frontiers: 0 <= inflate <= 255 cells");
    if (out_w) *out_w = f->w;
    if (out_h) *out_h = f->h;
    if (bytes) *bytes = (int64_t)f->w * f->h * (int64_t)sizeof(uint32_t);
    return GMS_OK;
}
int gms_map_frontiers(gms_map *m, int32_t mi, const gms_frontiers *f, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap,
                      int32_t *n_found) {
    return frontiers(query_map(m, mi), "gms_map_frontiers", f, cost, labels, records, cap, n_found, nullptr, false);
}
int gms_map_frontiers_dev(gms_map *m, int32_t mi, const gms_frontiers *f, const uint16_t *dev_cost, uint32_t *dev_labels, gms_frontier *dev_records,
                          int32_t cap, int32_t *n_found) {
    return frontiers(query_map(m, mi), "gms_map_frontiers", f, dev_cost, dev_labels, dev_records, cap, n_found, nullptr, true);
}
int gms_slam_frontiers(gms_slam *s, int32_t which, const gms_frontiers *f, const uint16_t *cost, uint32_t *labels, gms_frontier *records, int32_t cap,
                       int32_t *n_found, int32_t *shown) {
    return frontiers(query_slam(s, which), "gms_slam_frontiers", f, cost, labels, records, cap, n_found, shown, false);
}
int gms_slam_frontiers_dev(gms_slam *s, int32_t which, const gms_frontiers *f, const uint16_t *dev_cost, uint32_t *dev_labels, gms_frontier *dev_records,
                           int32_t cap, int32_t *n_found, int32_t *dev_shown) {
    return frontiers(query_slam(s, which), "gms_slam_frontiers", f, dev_cost, dev_labels, dev_records, cap, n_found, dev_shown, true);
}

}  // extern "C"
