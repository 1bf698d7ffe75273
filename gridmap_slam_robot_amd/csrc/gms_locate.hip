// gms_locate.hip -- global scan matching (gridmapslam.h "global scan matching"): the poses of a whole rectangle of the map that explain one
// scan best, by the multi-resolution correlative search on bit planes.  All integer arithmetic; what is returned is what the exhaustive
// search returns, however the search is pruned.
//
// A translation unit of its own, kernels and C-ABI, layered on the query base and on gms_reach_inflate as gms_frontier.hip and
// gms_scatter.hip are: nothing here is on the scan step's path, and no kernel of the other units is compiled differently for it.
//
//   the hit plane   P_0: the obstacle plane of `mode` read in place (query_plane; tol == 0) or the cost-to-go fields' blocked plane at
//                   inflate = tol (gms_reach_inflate).  The casts' layout, rows of 64-bit words, the padding beyond W zero.
//   k_loc_pyramid   P_l from P_(l-1), a lane per 64-bit word: bit (x, y) of P_l is the OR of the hit plane over [x, x + 2^l) x
//                   [y, y + 2^l) clipped to the map -- the window slides, nothing is decimated.  With h = 2^(l-1): the word, the word
//                   funnel-shifted down by h across the word boundary, and the same two of row y + h.  What lies beyond the row's last
//                   word or the map's last row is 0, so the padding stays 0 at every level.
//   k_loc_level     ONE LEVEL of the breadth-first search: a wavefront per candidate (k, bx, by), LOC_CPW candidates in turn, the beams
//                   strided over its lanes and counted with ballots.  BOUND = beams whose bit (bx + dx, by + dy) of P_l is set -- a
//                   coordinate in [-(2^l - 1), -1] clamped to 0 (the window only grows), one at or below -(2^l) or beyond the map
//                   contributing 0 -- is at least every SCORE of the block.  The same pass scores the block's own origin against P_0: a
//                   proven leaf, counted in a histogram of B + 1 counters.  A candidate with BOUND >= threshold appends its children
//                   inside the rectangle to the next list; the workgroup sums its 16 candidates' appends in LDS and takes ONE returning
//                   atomic on the list's counter.  Level 0: BOUND is the score; a candidate that is free (free_only) and scores
//                   >= threshold appends its 64-bit key.  List order is arbitrary, the set is not.
//   k_loc_thresh    between two levels, one workgroup: the threshold rises to the cap-th largest score in the level's histogram (each
//                   level's origins are distinct leaves, so that score is proven), the histogram and the next counter are zeroed.
//                   Pruning is on BOUND < threshold only: ties at the cut survive to the ranking.
//   k_loc_select    one workgroup of 1024 lanes: the `cap` smallest keys -- (B - score) << 50 | k << 40 | y << 20 | x, all distinct --
//                   by an 8-bit radix select over the survivors where they exceed 4096, then a bitonic sort in LDS; the records, the
//                   filler records behind them and n_out.
//
// No workgroup waits on another.  The host reads 8 control words back once per level (the next list's length: it sizes the next launch)
// and nothing else until the caller's own outputs.
#undef GMS_STAMPS
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "gms_device.h"

#define LOC_NT 256
#define LOC_CPW 4                            // candidates a wavefront evaluates in turn
#define LOC_CPB (LOC_CPW * LOC_NT / 64)      // ... and a workgroup: one atomic on the list's counter for all of them
#define LOC_MAX_LEVEL 7
#define LOC_LIST_MAX (1 << 24)               // entries of a work list at most
#define LOC_CTL_WORDS 8                      // d_ctl: [0..1] the two lists' counters, [2] the threshold, 5 spare; the histogram behind them
#define LOC_SEL_NT 1024
#define LOC_SEL_N 4096                       // keys k_loc_select sorts = the largest cap
#define LOC_XY_BITS 20                       // of a cell coordinate in a list entry: maps of up to 2^20 cells a side
#define LOC_OFF_MAX 4095

static_assert(sizeof(gms_locate_rec) == 16, "gms_locate_rec is one 16-byte store");
static_assert(sizeof(gms_locate) == 48, "gms_locate is twelve int32_t");
static_assert(GMS_LOCATE_SKIP == INT16_MIN, "the SKIP marker");
static_assert(GMS_MAX_BEAMS < (1 << 14) && 1024 <= (1 << 10), "the key's fields: B - score above bit 50, k in 10 bits");

__device__ __forceinline__ uint64_t loc_entry(int32_t k, int32_t x, int32_t y) {
    return ((uint64_t)(uint32_t)k << (2 * LOC_XY_BITS)) | ((uint64_t)(uint32_t)y << LOC_XY_BITS) | (uint64_t)(uint32_t)x;
}
__device__ __forceinline__ bool loc_bit(const uint64_t *__restrict__ p, int32_t wpr64, int32_t x, int32_t y) {
    return (p[(size_t)y * (size_t)wpr64 + (size_t)(x >> 6)] >> (x & 63)) & 1ull;
}

// prev, next: H rows of wpr64 words; half = 2^(l-1), 1 .. 64
__global__ void __launch_bounds__(LOC_NT)
k_loc_pyramid(const uint64_t *__restrict__ prev, uint64_t *__restrict__ next, int32_t wpr64, int32_t H, int32_t half) {
    const int32_t i = (int32_t)blockIdx.x * LOC_NT + (int32_t)threadIdx.x;
    if (i >= wpr64 * H) return;
    const int32_t y = i / wpr64, xw = i - y * wpr64;
    uint64_t r = 0ull;
#pragma unroll
    for (int32_t row = 0; row < 2; row++) {
        const int32_t yy = y + row * half;
        if (yy >= H) break;
        const uint64_t a = prev[(size_t)yy * (size_t)wpr64 + (size_t)xw];
        const uint64_t up = xw + 1 < wpr64 ? prev[(size_t)yy * (size_t)wpr64 + (size_t)(xw + 1)] : 0ull;     // (beyond the row: 0)
        r |= a | (half == 64 ? up : (a >> half) | (up << (64 - half)));                                   // the funnel shift across the word boundary
    }
    next[i] = r;
}

// what one level's launch needs
struct LocLevel {
    const uint64_t *p0;         // the hit plane
    const uint64_t *pl;         // P_level (level 0: the hit plane again)
    const uint64_t *nf;         // free_only: the not-free plane; else NULL
    const uint32_t *off;        // [n_theta][B] the offsets, dx | dy << 16
    const uint64_t *src;        // this level's list, or NULL: every block of the level over the rectangle, nbx x nby x n_theta
    uint64_t *dst;              // the next level's list; level 0: the survivors' keys
    uint32_t *ctl, *hist;
    int64_t n;                  // candidates
    int32_t dst_cap, dst_ctl;   // entries dst holds, and which counter counts them
    int32_t W, H, wpr64, B, level, x0, y0, x1, y1, nbx, nby, min_score;
};

__global__ void __launch_bounds__(LOC_NT)
k_loc_level(LocLevel a) {
    __shared__ uint32_t s_nc[LOC_CPB];
    __shared__ uint32_t s_base;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t thr = a.ctl[2];
    const int32_t S = 1 << a.level, half = S >> 1;
    int32_t ck[LOC_CPW], cx[LOC_CPW], cy[LOC_CPW], cs[LOC_CPW];
    uint32_t cn[LOC_CPW];
#pragma unroll
    for (int32_t c = 0; c < LOC_CPW; c++) {
        const int64_t i = (int64_t)blockIdx.x * LOC_CPB + wv * LOC_CPW + c;
        ck[c] = cx[c] = cy[c] = cs[c] = 0;
        cn[c] = 0u;
        if (i < a.n) {                                                          // (uniform per wavefront)
            int32_t k, bx, by;
            if (a.src) {
                const uint64_t e = a.src[i];
                k = (int32_t)(e >> (2 * LOC_XY_BITS));
                by = (int32_t)((e >> LOC_XY_BITS) & ((1u << LOC_XY_BITS) - 1u));
                bx = (int32_t)(e & ((1u << LOC_XY_BITS) - 1u));
            } else {
                const int64_t per = (int64_t)a.nbx * a.nby;
                k = (int32_t)(i / per);
                const int32_t r = (int32_t)(i - (int64_t)k * per), iy = r / a.nbx;
                bx = a.x0 + ((r - iy * a.nbx) << a.level);
                by = a.y0 + (iy << a.level);
            }
            const uint32_t *__restrict__ off = a.off + (size_t)k * (size_t)a.B;
            uint32_t bound = 0u, leaf = 0u;
            for (int32_t b0 = 0; b0 < a.B; b0 += 64) {
                const int32_t b = b0 + lane;
                const uint32_t o = b < a.B ? off[b] : 0x80008000u;              // (SKIP)
                const int32_t dx = (int32_t)(int16_t)(o & 0xffffu), dy = (int32_t)(int16_t)(o >> 16);
                const bool ok = abs(dx) <= LOC_OFF_MAX && abs(dy) <= LOC_OFF_MAX;                     // SKIP, or beyond the precondition: never an address
                const int32_t px = bx + dx, py = by + dy;
                const bool hit0 = ok && px >= 0 && px < a.W && py >= 0 && py < a.H && loc_bit(a.p0, a.wpr64, px, py);
                leaf += (uint32_t)__popcll(__ballot(hit0));
                if (a.level > 0) {
                    const bool hit = ok && px > -S && px < a.W && py > -S && py < a.H && loc_bit(a.pl, a.wpr64, max(px, 0), max(py, 0));
                    bound += (uint32_t)__popcll(__ballot(hit));
                }
            }
            const bool is_free = !a.nf || !loc_bit(a.nf, a.wpr64, bx, by);
            ck[c] = k; cx[c] = bx; cy[c] = by; cs[c] = (int32_t)leaf;
            if (a.level > 0) {
                if (lane == 0 && is_free && leaf >= (uint32_t)a.min_score) atomicAdd(&a.hist[leaf], 1u);          // a proven leaf: the block's own origin
                if (bound >= thr) cn[c] = (bx + half < a.x1 ? 2u : 1u) * (by + half < a.y1 ? 2u : 1u);            // strictly below the threshold: pruned
            } else if (is_free && leaf >= thr)
                cn[c] = 1u;
        }
        if (lane == 0) s_nc[wv * LOC_CPW + c] = cn[c];
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0u;
        for (int32_t j = 0; j < LOC_CPB; j++) total += s_nc[j];
        s_base = total ? atomicAdd(&a.ctl[a.dst_ctl], total) : 0u;
    }
    __syncthreads();
    uint32_t pos = s_base;
    for (int32_t j = 0; j < wv * LOC_CPW; j++) pos += s_nc[j];
#pragma unroll
    for (int32_t c = 0; c < LOC_CPW; c++) {
        const uint32_t nc = cn[c];
        if ((uint32_t)lane < nc && (uint64_t)pos + nc <= (uint64_t)a.dst_cap) {           // (a list that overflows: the host sees the counter)
            uint64_t e;
            if (a.level > 0) {
                const int32_t two_x = cx[c] + half < a.x1 ? 1 : 0;              // children beyond the rectangle are dropped
                const int32_t ix = two_x ? (lane & 1) : 0, iy = two_x ? (lane >> 1) : lane;
                e = loc_entry(ck[c], cx[c] + ix * half, cy[c] + iy * half);
            } else
                e = ((uint64_t)(uint32_t)(a.B - cs[c]) << 50) | loc_entry(ck[c], cx[c], cy[c]);
            a.dst[(size_t)pos + (size_t)lane] = e;
        }
        pos += nc;
    }
}

// the control words and the histogram of a new request
__global__ void __launch_bounds__(LOC_NT)
k_loc_init(uint32_t *__restrict__ ctl, uint32_t *__restrict__ hist, int32_t B, int32_t min_score) {
    const int32_t tid = (int32_t)threadIdx.x;
    if (tid < LOC_CTL_WORDS) ctl[tid] = tid == 2 ? (uint32_t)min_score : 0u;
    for (int32_t t = tid; t <= B; t += LOC_NT) hist[t] = 0u;
}

// one workgroup: ctl[2] = max(ctl[2], the cap-th largest score counted in hist [B + 1]); hist and ctl[zero] zeroed
__global__ void __launch_bounds__(LOC_NT)
k_loc_thresh(uint32_t *__restrict__ ctl, uint32_t *__restrict__ hist, int32_t B, int32_t cap, int32_t zero) {
    __shared__ uint32_t s_sum[LOC_NT];
    const int32_t tid = (int32_t)threadIdx.x, n = B + 1, chunk = (n + LOC_NT - 1) / LOC_NT;
    uint32_t sum = 0u;
    for (int32_t t = tid * chunk; t < min(n, (tid + 1) * chunk); t++) sum += hist[t];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t acc = 0u, found = 0u;
        for (int32_t c = LOC_NT - 1; c >= 0 && !found; c--) {
            if (acc + s_sum[c] >= (uint32_t)cap) {
                for (int32_t t = min(n, (c + 1) * chunk) - 1; t >= c * chunk; t--) {
                    acc += hist[t];
                    if (acc >= (uint32_t)cap) { found = (uint32_t)t; break; }
                }
                break;
            }
            acc += s_sum[c];
        }
        if (found > ctl[2]) ctl[2] = found;
        ctl[zero] = 0u;
    }
    __syncthreads();
    for (int32_t t = tid; t < n; t += LOC_NT) hist[t] = 0u;
}

// one workgroup: the min(R, cap) smallest of keys [R] in ascending order as records, fillers behind them, and their number
__global__ void __launch_bounds__(LOC_SEL_NT)
k_loc_select(const uint64_t *__restrict__ keys, int32_t R, int32_t cap, int32_t B, gms_locate_rec *__restrict__ out, int32_t *__restrict__ n_out) {
    __shared__ uint64_t s_key[LOC_SEL_N];
    __shared__ uint32_t s_hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_want, s_cnt;
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t n_sel = min(R, cap);
    int32_t held = R;                                                           // keys in s_key
    if (R <= LOC_SEL_N) {
        for (int32_t i = tid; i < LOC_SEL_N; i += LOC_SEL_NT) s_key[i] = i < R ? keys[i] : ~0ull;
    } else {
        // the cap-th smallest key, eight bits at a time from the top: the bin in which the running count reaches the rank
        if (tid == 0) { s_prefix = 0ull; s_want = (uint32_t)cap; s_cnt = 0u; }
        for (int32_t pass = 7; pass >= 0; pass--) {
            const int32_t shift = 8 * pass;
            if (tid < 256) s_hist[tid] = 0u;
            __syncthreads();
            const uint64_t prefix = s_prefix;
            for (int32_t i = tid; i < R; i += LOC_SEL_NT) {
                const uint64_t key = keys[i];
                if (pass == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t acc = 0u;
                const uint32_t want = s_want;
                for (uint32_t bin = 0; bin < 256u; bin++) {                     // (R > cap >= want: some bin reaches it)
                    if (acc + s_hist[bin] >= want) { s_prefix = prefix | ((uint64_t)bin << shift); s_want = want - acc; break; }
                    acc += s_hist[bin];
                }
            }
            __syncthreads();
        }
        const uint64_t pivot = s_prefix;
        for (int32_t i = tid; i < LOC_SEL_N; i += LOC_SEL_NT) s_key[i] = ~0ull;
        __syncthreads();
        for (int32_t i = tid; i < R; i += LOC_SEL_NT) {
            const uint64_t key = keys[i];
            if (key <= pivot) {                                                 // the keys are distinct: exactly cap of them
                const uint32_t slot = atomicAdd(&s_cnt, 1u);
                if (slot < LOC_SEL_N) s_key[slot] = key;
            }
        }
        held = cap;
    }
    __syncthreads();
    int32_t N = 2;
    while (N < held) N <<= 1;                                                   // (uniform) the padding sorts behind every key
    for (int32_t k = 2; k <= N; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t i = tid; i < N; i += LOC_SEL_NT) {
                const int32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = s_key[i], b = s_key[l];
                    if (((i & k) == 0) == (a > b)) { s_key[i] = b; s_key[l] = a; }
                }
            }
            __syncthreads();
        }
    for (int32_t i = tid; i < cap; i += LOC_SEL_NT) {
        int4 rec = make_int4(0, -1, -1, -1);
        if (i < n_sel) {
            const uint64_t key = s_key[i];
            rec = make_int4(B - (int32_t)(key >> 50), (int32_t)((key >> (2 * LOC_XY_BITS)) & 1023u), (int32_t)(key & ((1u << LOC_XY_BITS) - 1u)),
                            (int32_t)((key >> LOC_XY_BITS) & ((1u << LOC_XY_BITS) - 1u)));
        }
        reinterpret_cast<int4 *>(out)[i] = rec;
    }
    if (tid == 0) *n_out = n_sel;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the levels of a request: the handle's forced number (GMS_LOCATE_LEVELS), or from the rectangle -- the top level's blocks a quarter of
// the longer side at most, so that it still has a few blocks to tell apart
static int32_t loc_levels(const gms_map *m, const gms_locate *lc) {
    if (m->locate_levels >= 0) return std::min(m->locate_levels, LOC_MAX_LEVEL);
    int32_t L = 0;
    while (L < LOC_MAX_LEVEL && (4 << (L + 1)) <= std::max(lc->w, lc->h)) L++;
    return L;
}

// what a request needs on the handle besides the lists (a handle's W and H never change)
static int loc_buffers(gms_map *m, int32_t L) {
    auto &t = m->locate;
    const size_t words = (size_t)m->gd.H * (size_t)((m->gd.W + 63) / 64);
    int rc = gms_dev_alloc(&t.d_ctl, (LOC_CTL_WORDS + GMS_MAX_BEAMS + 1) * sizeof(uint32_t), "gms_locate", "the control words and the histogram");
    if (!rc && L > 0) rc = gms_dev_alloc(&t.d_pyr, LOC_MAX_LEVEL * words * sizeof(uint64_t), "gms_locate", "the OR pyramid");
    if (!rc) rc = gms_pinned_alloc(&t.h_ctl, LOC_CTL_WORDS * sizeof(uint32_t), "gms_locate");
    return rc;
}

// list `which` holds `need` entries at least (the stream is idle: the caller has just waited on it, or nothing of this request reads the list yet)
static int loc_list_grow(gms_map *m, int32_t which, int64_t need) {
    auto &t = m->locate;
    if (t.d_list[which] && t.list_cap[which] >= need) return GMS_OK;
    HIPCHK(hipStreamSynchronize(m->stream));
    hipFree(t.d_list[which]);
    t.d_list[which] = nullptr;
    t.list_cap[which] = 0;
    const int64_t cap = std::min<int64_t>(LOC_LIST_MAX, (need + 65535) & ~(int64_t)65535);
    int rc = gms_dev_alloc(&t.d_list[which], (size_t)cap * sizeof(uint64_t), "gms_locate", "a work list");
    if (rc) return rc;
    t.list_cap[which] = cap;
    return GMS_OK;
}

// The best poses of ONE map's planes (of logData as it stands) into the caller's device buffers; waits on the stream once per level
static int loc_run(gms_map *m, const uint32_t *d_hit, const uint32_t *d_nf, const gms_locate *lc, const int16_t *d_off, int32_t B, gms_locate_rec *d_out,
                   int32_t *d_nout) {
    auto &t = m->locate;
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64, L = loc_levels(m, lc);
    int rc = loc_buffers(m, L);
    if (rc) return rc;
    const int64_t words = (int64_t)H * wpr64;
    hipStream_t st = m->stream;
    uint32_t *ctl = t.d_ctl, *hist = ctl + LOC_CTL_WORDS;
    hipLaunchKernelGGL(k_loc_init, dim3(1), dim3(LOC_NT), 0, st, ctl, hist, B, lc->min_score);
    const uint64_t *plane[LOC_MAX_LEVEL + 1];
    plane[0] = reinterpret_cast<const uint64_t *>(d_hit);
    for (int32_t l = 1; l <= L; l++) {
        uint64_t *next = t.d_pyr + (size_t)(l - 1) * (size_t)words;
        hipLaunchKernelGGL(k_loc_pyramid, dim3((unsigned)((words + LOC_NT - 1) / LOC_NT)), dim3(LOC_NT), 0, st, plane[l - 1], next, wpr64, H, 1 << (l - 1));
        plane[l] = next;
    }
    HIPCHK(hipGetLastError());
    LocLevel a;
    a.p0 = plane[0]; a.nf = reinterpret_cast<const uint64_t *>(d_nf); a.off = reinterpret_cast<const uint32_t *>(d_off);
    a.ctl = ctl; a.hist = hist;
    a.W = W; a.H = H; a.wpr64 = wpr64; a.B = B; a.x0 = lc->x0; a.y0 = lc->y0; a.x1 = lc->x0 + lc->w; a.y1 = lc->y0 + lc->h; a.min_score = lc->min_score;
    a.nbx = (lc->w + (1 << L) - 1) >> L; a.nby = (lc->h + (1 << L) - 1) >> L;
    a.src = nullptr;
    int64_t n = (int64_t)lc->n_theta * a.nbx * a.nby;                          // the top level: every block, no list
    t.levels = L;
    for (int32_t l = 0; l < 8; l++) t.evaluated[l] = 0;
    for (int32_t l = L; l >= 0; l--) {
        // this level's survivors: four children each at most, and never more than the level below has blocks (level 0: one key each)
        const int32_t lb = std::max(l - 1, 0);
        const int64_t below = (int64_t)lc->n_theta * ((lc->w + (1 << lb) - 1) >> lb) * ((lc->h + (1 << lb) - 1) >> lb);
        const int64_t need = std::min<int64_t>(LOC_LIST_MAX, std::min(l > 0 ? 4 * n : n, below));
        const int32_t which = l & 1;
        rc = loc_list_grow(m, which, need);
        if (rc) return rc;
        a.pl = plane[l]; a.level = l; a.n = n; a.dst = t.d_list[which]; a.dst_cap = (int32_t)t.list_cap[which]; a.dst_ctl = which;
        hipLaunchKernelGGL(k_loc_level, dim3((unsigned)((n + LOC_CPB - 1) / LOC_CPB)), dim3(LOC_NT), 0, st, a);
        if (l > 0) hipLaunchKernelGGL(k_loc_thresh, dim3(1), dim3(LOC_NT), 0, st, ctl, hist, B, lc->cap, which ^ 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(t.h_ctl, ctl, LOC_CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        t.evaluated[l] = n;
        n = (int64_t)t.h_ctl[which];
        if (n > t.list_cap[which])
            return gms_fail(GMS_ERR_NOMEM, "gms_locate: level %d leaves %lld candidates, a work list holds 2^24: raise min_score or shrink the rectangle", l,
                            (long long)n);
        a.src = t.d_list[which];
        if (n == 0) break;                                                      // nothing reaches min_score
    }
    hipLaunchKernelGGL(k_loc_select, dim3(1), dim3(LOC_SEL_NT), 0, st, a.src, (int32_t)n, lc->cap, B, d_out, d_nout);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// a host table's entries: SKIP pairs, or both components within the range the device form takes for granted
static bool loc_offsets_ok(const int16_t *off, size_t pairs) {
    for (size_t i = 0; i < pairs; i++) {
        const int32_t dx = off[2 * i], dy = off[2 * i + 1];
        if (dx == GMS_LOCATE_SKIP && dy == GMS_LOCATE_SKIP) continue;
        if (abs(dx) > LOC_OFF_MAX || abs(dy) > LOC_OFF_MAX) return false;
    }
    return true;
}

// the best poses in one map of a shared handle or in the shown particle's map of a per-particle one; `shown` exists for a particle only
static int locate(QuerySource src, const char *what, const gms_locate *lc, const int16_t *offsets, int32_t B, gms_locate_rec *out, int32_t *n_out,
                  int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !lc || !offsets || !out || !n_out)
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the offsets, the output and n_out are required)", what);
    gms_map *m = src.m;
    int rc = gms_locate_check(lc);
    if (rc) return rc;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", what);
    if (lc->min_score > B) return gms_fail(GMS_ERR_INVALID, "%s: gms_locate.min_score = %d exceeds the %d beams", what, lc->min_score, B);
    rc = gms_rect_check(lc->x0, lc->y0, lc->w, lc->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if (m->gd.W > (1 << LOC_XY_BITS) || m->gd.H > (1 << LOC_XY_BITS)) return gms_fail(GMS_ERR_INVALID, "%s: a map of more than 2^20 cells a side", what);
    if ((int64_t)lc->n_theta * lc->w * lc->h > (int64_t)INT_MAX) return gms_fail(GMS_ERR_INVALID, "%s: n_theta * w * h exceeds 2^31 - 1 candidates", what);
    if (on_device && (((uintptr_t)out & 15) != 0 || ((uintptr_t)n_out & 3) != 0 || ((uintptr_t)offsets & 3) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the device output must be 16-byte aligned, n_out and the offsets 4-byte aligned", what);
    const size_t pairs = (size_t)lc->n_theta * (size_t)B;
    if (!on_device && !loc_offsets_ok(offsets, pairs))
        return gms_fail(GMS_ERR_INVALID, "%s: an offset is neither the SKIP pair nor within [-4095, 4095]", what);
    src.filter = lc->filter;
    rc = query_check(src, what, "gms_locate.filter");                           // the map's index, or the shown particle
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    if (src.s && lc->free_only && lc->mode != GMS_CLEAR_NOT_FREE) {
        rc = gms_dev_alloc(&m->d_front_nf, (size_t)m->gd.H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), what, "the particle's second plane");
        if (rc) return rc;
    }
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)lc->cap * sizeof(gms_locate_rec), off_bytes = pairs * 2 * sizeof(int16_t);
    const size_t p_out = st.part(out_bytes), p_nout = st.part(sizeof(int32_t)), p_off = st.part(off_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_off, offsets, off_bytes);
    if (rc) return rc;
    // the obstacle plane of `mode` in place (a particle's: packed per request), the hit plane from it; free_only: the not-free plane too
    const uint32_t *obstacles = nullptr, *hit = nullptr, *nf = nullptr;
    rc = query_plane(src, lc->mode, st.shown(shown), nullptr, &obstacles);
    if (!rc && lc->free_only) {
        if (lc->mode == GMS_CLEAR_NOT_FREE) nf = obstacles;
        else rc = query_plane(src, GMS_CLEAR_NOT_FREE, nullptr, src.s ? m->d_front_nf : nullptr, &nf);
    }
    hit = obstacles;
    if (!rc && lc->tol > 0) rc = gms_reach_inflate(m, obstacles, lc->tol, lc->mode, &hit);
    if (!rc) rc = loc_run(m, hit, nf, lc, st.at(p_off, offsets), B, st.at(p_out, out), st.at(p_nout, n_out));
    if (rc) return rc;
    st.fetch(out, p_out, out_bytes);
    st.fetch(n_out, p_nout, sizeof(int32_t));
    return st.finish(shown);
}

extern "C" {

int gms_locate_check(const gms_locate *lc) {
    REQUIRE(lc, "gms_locate: null request");
    REQUIRE(lc->w >= 1 && lc->h >= 1, "gms_locate: w and h must be at least 1");
    REQUIRE(lc->x0 >= 0 && lc->y0 >= 0, "gms_locate: x0 and y0 must not be negative");
    REQUIRE(lc->n_theta >= 1 && lc->n_theta <= 1024, "gms_locate: 1 <= n_theta <= 1024 headings");
    REQUIRE(lc->tol >= 0 && lc->tol <= 255, "gms_locate: 0 <= tol <= 255 cells");
    REQUIRE(lc->mode == GMS_CLEAR_OCCUPIED || lc->mode == GMS_CLEAR_NOT_FREE, "gms_locate: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(lc->min_score >= 1 && lc->min_score <= GMS_MAX_BEAMS, "gms_locate: 1 <= min_score <= the beams of the scan");
    REQUIRE(lc->cap >= 1 && lc->cap <= LOC_SEL_N, "gms_locate: 1 <= cap <= 4096 records");
    REQUIRE(lc->free_only == 0 || lc->free_only == 1, "gms_locate: free_only must be 0 or 1");
    return GMS_OK;
}

// (this unit is compiled with -ffp-contract=off, as the whole library is: every product and the sum below round on their own)
int gms_locate_offsets(const gms_beam *beams, int32_t B, double theta0, double dtheta, int32_t n_theta, double resolution, int16_t *offsets) {
    REQUIRE(beams && offsets, "gms_locate_offsets: null argument");
    REQUIRE(B >= 1 && B <= GMS_MAX_BEAMS, "gms_locate_offsets: 1 <= B <= GMS_MAX_BEAMS beams");
    REQUIRE(n_theta >= 1 && n_theta <= 1024, "gms_locate_offsets: 1 <= n_theta <= 1024 headings");
    REQUIRE(resolution > 0.0 && isfinite(resolution), "gms_locate_offsets: the resolution must be positive and finite");
    for (int32_t k = 0; k < n_theta; k++) {
        const double theta = theta0 + (double)k * dtheta;
        const double c = cos(theta), s = sin(theta);
        for (int32_t b = 0; b < B; b++) {
            int16_t *o = offsets + 2 * ((size_t)k * (size_t)B + (size_t)b);
            const double lx = beams[b].local_x, ly = beams[b].local_y;
            const double xc = lx * c, ys = ly * s, xs = lx * s, yc = ly * c;
            const double ex = xc - ys, ey = xs + yc;
            const double fx = floor(ex / resolution + 0.5), fy = floor(ey / resolution + 0.5);
            // (a NaN fails every comparison: SKIP)
            if (beams[b].hit && isfinite(lx) && isfinite(ly) && fabs(fx) <= (double)LOC_OFF_MAX && fabs(fy) <= (double)LOC_OFF_MAX) {
                o[0] = (int16_t)(int)fx;
                o[1] = (int16_t)(int)fy;
            } else
                o[0] = o[1] = GMS_LOCATE_SKIP;
        }
    }
    return GMS_OK;
}

int gms_map_locate(gms_map *m, int32_t mi, const gms_locate *lc, const int16_t *offsets, int32_t B, gms_locate_rec *out, int32_t *n_out) {
    return locate(query_map(m, mi), "gms_map_locate", lc, offsets, B, out, n_out, nullptr, false);
}
int gms_map_locate_dev(gms_map *m, int32_t mi, const gms_locate *lc, const int16_t *dev_offsets, int32_t B, gms_locate_rec *dev_out, int32_t *dev_n_out) {
    return locate(query_map(m, mi), "gms_map_locate_dev", lc, dev_offsets, B, dev_out, dev_n_out, nullptr, true);
}
int gms_slam_locate(gms_slam *s, int32_t which, const gms_locate *lc, const int16_t *offsets, int32_t B, gms_locate_rec *out, int32_t *n_out,
                    int32_t *shown) {
    return locate(query_slam(s, which), "gms_slam_locate", lc, offsets, B, out, n_out, shown, false);
}
int gms_slam_locate_dev(gms_slam *s, int32_t which, const gms_locate *lc, const int16_t *dev_offsets, int32_t B, gms_locate_rec *dev_out,
                        int32_t *dev_n_out, int32_t *dev_shown) {
    return locate(query_slam(s, which), "gms_slam_locate_dev", lc, dev_offsets, B, dev_out, dev_n_out, dev_shown, true);
}
int gms_map_locate_stats(const gms_map *m, int32_t *levels, int64_t *evaluated) {
    REQUIRE(m, "gms_map_locate_stats: null handle");
    if (levels) *levels = m->locate.levels;
    if (evaluated)
        for (int32_t l = 0; l < 8; l++) evaluated[l] = m->locate.evaluated[l];
    return GMS_OK;
}

}  // extern "C"
