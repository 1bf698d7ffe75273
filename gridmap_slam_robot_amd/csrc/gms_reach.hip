// gms_reach.hip -- cost-to-go fields (gridmapslam.h "cost-to-go fields"): the cost of the cheapest 8-connected path, axis step 5, diagonal
// step 7, no corner cutting, from a set of seed cells to every cell of the map through the cells that are not blocked, capped at
// max_cost.  All integer arithmetic; the field is unique, so however the relaxation is scheduled the result is the same.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the blocked plane   one bit per cell in the casts' layout (rows of 64-bit words, the padding zero).  inflate == 0: the casts' plane
//                       or the map's second plane, read in place (query_plane; a gms_slam's: the shown particle's, packed per request).
//                       inflate > 0: k_clear_field over the whole map at R = inflate into d_reach_d2, then k_reach_block ballots
//                       d2 != FAR into d_reach_plane, a wavefront per 64 cells.
//   k_reach_init        the working field all FAR, the control words and the tiles' flags zero.
//   k_reach_seeds       a lane per seed: on the map and not blocked -> cost 0, and the tiles of the cell and of its eight neighbours active:
//                       a round marks across an edge only where a cell CHANGED, and the seed's own cell never does, so a seed whose
//                       neighbours inside its tile are all blocked (or whose tile is one cell) would hand nothing on.  A gms_slam
//                       without seeds: the shown particle's own cell, from its pose on the device.
//   k_reach_round       ONE ROUND: a workgroup of one wavefront per 64 x 64 tile; the tiles that are not active leave at once.  An active
//                       tile loads its cells and a one-cell halo into LDS (66 x 66 uint16), relaxes to ITS fixpoint against that halo,
//                       writes back what changed and marks the neighbours across every edge or corner whose cell changed active for the
//                       NEXT round.  No workgroup waits on another; a halo that a neighbour rewrites in the same round is read old or
//                       new, both upper bounds of the true cost, and the neighbour's mark brings the tile back.
//   k_reach_copy        the rectangle out of the working field.
//
// The relaxation inside a tile is four directional sweeps, east, west, south, north, repeated until a whole pass changes nothing (and
// never more than the tile has cells).  The east sweep: lane y owns row y and walks x = 0 .. 63; the value it needs from the west is
// the one it has just computed, in a register, and the two diagonal ones are its neighbour lanes' registers, one DPP wavefront shift
// each -- the chain from one column to the next holds no LDS access.  Lanes 0 and 63 take the halo row's value instead (held in a
// register per lane, fetched with a uniform lane read).  The south and north sweeps are the same code with lane = column.  A sweep
// carries a cost across the whole tile, so open space settles in two passes and a third sees nothing move.
//
// LDS: 66 x 66 uint16 = 8712 bytes, row pitch 66 uint16 = 33 dwords.  A lane per row reads and writes dword 33 lane + c / 2: bank
// (33 lane + const) mod 32 = (lane + const) mod 32, distinct within each half-wave (16-bit accesses bank by 32 per 32 lanes).  A lane per
// column touches 64 consecutive uint16: 16 consecutive dwords per half-wave, two lanes to a dword.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_device.h"

#define RCH_T 64                         // tile edge in cells = lanes of the workgroup = cells of a plane word
#define RCH_P (RCH_T + 2)                // LDS pitch: the tile and its halo
#define RCH_FAR 0xffffu
#define RCH_CTL_WORDS 8                  // d_reach_ctl: [0..1] tile runs, [2..5] active counts, [6..7] spare; the flags behind them
#define RCH_BATCH_DEFAULT 8              // rounds per read-back (GMS_REACH_BATCH)

static_assert(GMS_REACH_FAR == RCH_FAR && GMS_REACH_AXIS == 5 && GMS_REACH_DIAG == 7, "the header's constants are the kernels'");

// lane l receives lane l - 1's v (lane 0 keeps its own) / lane l + 1's (lane 63 keeps its own): DPP wave_shr:1 / wave_shl:1
__device__ __forceinline__ uint32_t reach_from_below(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t reach_from_above(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false); }

// inflate > 0: the blocked plane from the clearance field d2 of the whole map (the planes' layout and ballot, gms_device.h)
__global__ void __launch_bounds__(256)
k_reach_block(const uint16_t *__restrict__ d2, int32_t W, int32_t wpr64, uint64_t *__restrict__ plane) {
    const int32_t lane = threadIdx.x & 63;
    const int32_t wx = plane_wave_word(), y = (int32_t)blockIdx.y;
    if (wx >= wpr64) return;                                                    // (uniform per wavefront)
    const int32_t x = wx * 64 + lane;
    const uint32_t v = x < W ? d2[(size_t)y * (size_t)W + (size_t)x] : RCH_FAR;                   // (padding: not blocked, as the planes have it)
    plane_pack_word(plane, (size_t)y * (size_t)wpr64 + (size_t)wx, v != RCH_FAR);
}

// field: words32 32-bit words; ctl: ctl_words
__global__ void __launch_bounds__(256)
k_reach_init(uint32_t *__restrict__ field, int64_t words32, uint32_t *__restrict__ ctl, int32_t ctl_words) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < words32; i += step) field[i] = 0xffffffffu;
    for (int64_t i = i0; i < ctl_words; i += step) ctl[i] = 0u;
}

__device__ __forceinline__ void reach_mark(uint32_t *flags, uint32_t *count, int32_t tile) {
    if (atomicExch(&flags[tile], 1u) == 0u) atomicAdd(count, 1u);
}

// seeds [K][2] (x, y), or -- seeds NULL -- the cell of particle `which` (>= 0, or the strongest of `filter` by the last update's
// statistics, as k_slam_plane picks it) under its pose
__global__ void __launch_bounds__(256)
k_reach_seeds(GridDev g, uint16_t *__restrict__ field, const uint64_t *__restrict__ plane, int32_t wpr64, int32_t ntx, uint32_t *__restrict__ ctl,
              const int32_t *__restrict__ seeds, int32_t K, const PfStatsDev *__restrict__ stats, int32_t which, int32_t filter, int32_t n_per,
              const float *__restrict__ pose) {
    const int32_t i = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    int32_t gx, gy;
    if (seeds) {
        if (i >= K) return;
        gx = seeds[2 * (size_t)i];
        gy = seeds[2 * (size_t)i + 1];
    } else {
        if (i != 0) return;
        const int32_t p = which >= 0 ? which : filter * n_per + stats[filter].strongest;
        gx = j_cell_exact((double)pose[3 * (size_t)p] - g.posx, g.res);                         // GridMap.java:273
        gy = j_cell_exact((double)pose[3 * (size_t)p + 1] - g.posy, g.res);                     // :274
    }
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) return;
    if ((plane[(size_t)gy * (size_t)wpr64 + (size_t)(gx >> 6)] >> (gx & 63)) & 1ull) return;
    field[(size_t)gy * (size_t)g.W + (size_t)gx] = 0;
    for (int32_t dy = -1; dy <= 1; dy++)                                        // (a seed inside its tile marks that tile nine times: one count)
        for (int32_t dx = -1; dx <= 1; dx++) {
            const int32_t nx = gx + dx, ny = gy + dy;
            if (nx >= 0 && ny >= 0 && nx < g.W && ny < g.H) reach_mark(ctl + RCH_CTL_WORDS, ctl + 2, (ny >> 6) * ntx + (nx >> 6));
        }
}

// One directional sweep of the tile s (66 x 66, cell (t, l) at s[(l + 1) * SL + (t + 1) * ST]): lane l owns line l and walks t = 0 .. 63
// (DIR > 0) or 63 .. 0.  me / lo / hi: the blocked bits (bit t) of lines l, l - 1 and l + 1; start_blocked: the halo cell the walk starts
// from.  true: the lane lowered a cell
template <int SL, int ST, int DIR>
__device__ __forceinline__ bool reach_sweep(uint16_t *s, int32_t lane, uint64_t me, uint64_t lo, uint64_t hi, bool start_blocked, uint32_t max_cost) {
    constexpr int T0 = DIR > 0 ? 0 : RCH_T - 1;
    uint16_t *cell = s + (lane + 1) * SL + (T0 + 1) * ST;
    // the halo lines beside lane 0 and lane 63, entry t in lane t; the corner the walk starts beside, everywhere
    const uint32_t line_lo = s[0 * SL + (lane + 1) * ST], line_hi = s[(RCH_P - 1) * SL + (lane + 1) * ST];
    uint32_t halo_lo = s[0 * SL + (T0 - DIR + 1) * ST], halo_hi = s[(RCH_P - 1) * SL + (T0 - DIR + 1) * ST];
    uint32_t prev = cell[-DIR * ST];
    bool prev_free = !start_blocked, changed = false;
    uint32_t cur = *cell;
#pragma unroll 4
    for (int32_t i = 0; i < RCH_T; i++) {
        const int32_t t = T0 + DIR * i;
        const uint32_t next = i + 1 < RCH_T ? cell[DIR * ST] : 0u;              // (nobody writes it before this lane does)
        uint32_t from_lo = reach_from_below(prev), from_hi = reach_from_above(prev);
        if (lane == 0) from_lo = halo_lo;
        if (lane == RCH_T - 1) from_hi = halo_hi;
        const bool me_b = (me >> t) & 1ull, lo_b = (lo >> t) & 1ull, hi_b = (hi >> t) & 1ull;
        uint32_t best = min(cur, prev + GMS_REACH_AXIS);                                          // (32 bits: FAR + 7 stays above every cap)
        if (prev_free && !lo_b) best = min(best, from_lo + GMS_REACH_DIAG);                       // the two cells the step squeezes between
        if (prev_free && !hi_b) best = min(best, from_hi + GMS_REACH_DIAG);
        if (best > max_cost || me_b) best = RCH_FAR;
        if (best != cur) { *cell = (uint16_t)best; changed = true; }
        prev = best;
        prev_free = !me_b;
        halo_lo = (uint32_t)__builtin_amdgcn_readlane((int)line_lo, t);
        halo_hi = (uint32_t)__builtin_amdgcn_readlane((int)line_hi, t);
        cur = next;
        cell += DIR * ST;
    }
    return changed;
}

// field [H][W]; plane: ONE map's, H rows of wpr64 words; grid (ntx, nty), a wavefront per tile; ctl as d_reach_ctl
__global__ void __launch_bounds__(RCH_T)
k_reach_round(uint16_t *field, const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *ctl, int32_t round, uint32_t max_cost) {
    __shared__ uint16_t s[RCH_P * RCH_P];
    const int32_t lane = (int32_t)threadIdx.x, tx = (int32_t)blockIdx.x, ty = (int32_t)blockIdx.y, ntx = (int32_t)gridDim.x, nty = (int32_t)gridDim.y;
    const int32_t tile = ty * ntx + tx, ntiles = ntx * nty;
    uint32_t *count = ctl + 2, *flags_cur = ctl + RCH_CTL_WORDS + (size_t)(round & 1) * (size_t)ntiles;
    uint32_t *flags_next = ctl + RCH_CTL_WORDS + (size_t)((round + 1) & 1) * (size_t)ntiles;
    if (tile == 0 && lane == 0) count[(round + 2) & 3] = 0u;                   // (this round counts into slot round + 1; round - 1 counted into this round's)
    if (flags_cur[tile] == 0u) return;                                          // (uniform)
    __syncthreads();
    if (lane == 0) {
        flags_cur[tile] = 0u;                                                   // (nobody else touches this round's flag of this tile)
        atomicAdd(reinterpret_cast<unsigned long long *>(ctl), 1ull);
    }
    const int32_t x0 = tx * RCH_T, y0 = ty * RCH_T, x = x0 + lane;
    for (int32_t r = 0; r < RCH_P; r++) {                                       // the tile and its halo; what lies off the map is FAR
        const int32_t y = y0 + r - 1;
        const bool row_in = y >= 0 && y < H;
        const uint16_t *__restrict__ src = field + (size_t)(row_in ? y : 0) * (size_t)W;
        s[r * RCH_P + lane + 1] = row_in && x < W ? src[x] : (uint16_t)RCH_FAR;
        if (lane < 2) {
            const int32_t xe = lane == 0 ? x0 - 1 : x0 + RCH_T;
            s[r * RCH_P + (lane == 0 ? 0 : RCH_P - 1)] = row_in && xe >= 0 && xe < W ? src[xe] : (uint16_t)RCH_FAR;
        }
    }
    // the blocked bits: a tile's row is one word of the plane; what lies off the map is blocked
    const uint64_t ragged = W - x0 < RCH_T ? ~0ull << (W - x0) : 0ull;
    auto row_word = [&](int32_t y) -> uint64_t { return y >= 0 && y < H ? (plane[(size_t)y * (size_t)wpr64 + (size_t)tx] | ragged) : ~0ull; };
    auto left_bit = [&](int32_t y) -> bool { return y >= 0 && y < H && tx > 0 ? (plane[(size_t)y * (size_t)wpr64 + (size_t)(tx - 1)] >> 63) != 0ull : true; };
    auto right_bit = [&](int32_t y) -> bool { return y >= 0 && y < H && x0 + RCH_T < W ? (plane[(size_t)y * (size_t)wpr64 + (size_t)(tx + 1)] & 1ull) != 0ull : true; };
    const uint64_t row_me = row_word(y0 + lane), row_lo = row_word(y0 + lane - 1), row_hi = row_word(y0 + lane + 1);
    const bool row_left = left_bit(y0 + lane), row_right = right_bit(y0 + lane);
    uint64_t col_me = 0ull;                                                     // lane = column: bit y of it
    for (int32_t r = 0; r < RCH_T; r++) col_me |= ((row_word(y0 + r) >> lane) & 1ull) << r;
    uint64_t col_lo = (uint64_t)__shfl_up((long long)col_me, 1), col_hi = (uint64_t)__shfl_down((long long)col_me, 1);
    const uint64_t halo_left = __ballot(row_left), halo_right = __ballot(row_right);
    if (lane == 0) col_lo = halo_left;
    if (lane == RCH_T - 1) col_hi = halo_right;
    const bool col_top = (row_word(y0 - 1) >> lane) & 1ull, col_bottom = (row_word(y0 + RCH_T) >> lane) & 1ull;
    __syncthreads();
    for (int32_t pass = 0; pass < RCH_T * RCH_T; pass++) {                      // (the vote ends it; the bound is the tile's cells)
        bool changed = reach_sweep<RCH_P, 1, 1>(s, lane, row_me, row_lo, row_hi, row_left, max_cost);
        changed |= reach_sweep<RCH_P, 1, -1>(s, lane, row_me, row_lo, row_hi, row_right, max_cost);
        __syncthreads();
        changed |= reach_sweep<1, RCH_P, 1>(s, lane, col_me, col_lo, col_hi, col_top, max_cost);
        changed |= reach_sweep<1, RCH_P, -1>(s, lane, col_me, col_lo, col_hi, col_bottom, max_cost);
        __syncthreads();
        if (!__any(changed)) break;
    }
    uint32_t moved = 0u;                                                        // bit 0: a cell of row 0 changed, 1: of row 63, 2: of column 0, 3: of column 63
    const int32_t rows = min(RCH_T, H - y0);
    if (x < W)
        for (int32_t r = 0; r < rows; r++) {
            uint16_t *dst = field + (size_t)(y0 + r) * (size_t)W + (size_t)x;
            const uint16_t v = s[(r + 1) * RCH_P + lane + 1];
            if (v != *dst) {
                *dst = v;
                moved |= (r == 0 ? 1u : 0u) | (r == RCH_T - 1 ? 2u : 0u) | (lane == 0 ? 4u : 0u) | (lane == RCH_T - 1 ? 8u : 0u);
            }
        }
    const uint64_t top = __ballot(moved & 1u), bottom = __ballot(moved & 2u), left = __ballot(moved & 4u), right = __ballot(moved & 8u);
    if (lane != 0) return;
    uint32_t *cnt = count + ((round + 1) & 3);
    const bool n = ty > 0, so = ty + 1 < nty, w = tx > 0, e = tx + 1 < ntx;
    if (top && n) reach_mark(flags_next, cnt, tile - ntx);
    if (bottom && so) reach_mark(flags_next, cnt, tile + ntx);
    if (left && w) reach_mark(flags_next, cnt, tile - 1);
    if (right && e) reach_mark(flags_next, cnt, tile + 1);
    if ((top & 1ull) && n && w) reach_mark(flags_next, cnt, tile - ntx - 1);                      // the corner cells: the tile across the corner
    if ((top >> 63) && n && e) reach_mark(flags_next, cnt, tile - ntx + 1);
    if ((bottom & 1ull) && so && w) reach_mark(flags_next, cnt, tile + ntx - 1);
    if ((bottom >> 63) && so && e) reach_mark(flags_next, cnt, tile + ntx + 1);
}

// out [h][w]
__global__ void __launch_bounds__(256)
k_reach_copy(const uint16_t *__restrict__ field, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h, uint16_t *__restrict__ out) {
    const int64_t n = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t y = (int32_t)(i / w), x = (int32_t)(i - (int64_t)y * w);
        out[i] = field[(size_t)(y0 + y) * (size_t)W + (size_t)(x0 + x)];
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int32_t reach_batch() {
    const char *e = getenv("GMS_REACH_BATCH");
    const int32_t b = e ? atoi(e) : RCH_BATCH_DEFAULT;
    return std::min(64, std::max(1, b));
}

// what a field needs on the handle (a handle's W and H never change, so nothing ever has to grow)
static int reach_buffers(gms_map *m, bool inflated) {
    const size_t cells = (size_t)m->gd.cells, ntiles = (size_t)((m->gd.W + RCH_T - 1) / RCH_T) * (size_t)((m->gd.H + RCH_T - 1) / RCH_T);
    int rc = gms_dev_alloc(&m->d_reach_field, ((cells + 1) & ~(size_t)1) * sizeof(uint16_t), "gms_reach", "the working field");
    if (!rc) rc = gms_dev_alloc(&m->d_reach_ctl, (RCH_CTL_WORDS + 2 * ntiles) * sizeof(uint32_t), "gms_reach", "the tiles' flags");
    // (inflate > 0: the clearance field and the blocked plane are gms_reach_inflate's)
    if (!rc) rc = gms_pinned_alloc(&m->h_reach_ctl, RCH_CTL_WORDS * sizeof(uint32_t), "gms_reach");
    return rc;
}

// inflate > 0: the blocked plane of ONE map's obstacle plane -- "clearance at R = inflate, balloted" -- in d_reach_plane
int gms_reach_inflate(gms_map *m, const uint32_t *d_obstacles, int32_t inflate, int32_t mode, const uint32_t **d_blocked) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64;
    int rc = gms_dev_alloc(&m->d_reach_d2, (size_t)m->gd.cells * sizeof(uint16_t), "gms_reach", "the inflation's clearance field");
    if (!rc) rc = gms_dev_alloc(&m->d_reach_plane, (size_t)H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), "gms_reach", "the blocked plane");
    if (rc) return rc;
    const gms_clearance c = {0, 0, W, H, inflate, mode, 0};
    rc = gms_clear_launch(m, d_obstacles, &c, m->d_reach_d2);
    if (rc) return rc;
    hipLaunchKernelGGL(k_reach_block, dim3((unsigned)((wpr64 + 3) / 4), (unsigned)H), dim3(256), 0, m->stream, m->d_reach_d2, W, wpr64,
                       reinterpret_cast<uint64_t *>(m->d_reach_plane));
    HIPCHK(hipGetLastError());
    *d_blocked = m->d_reach_plane;
    return GMS_OK;
}

// who plants the seeds: a list on the device, or (seeds NULL) the shown particle of a gms_slam
struct ReachSeeds {
    const int32_t *d_seeds;
    int32_t K;
    const PfStatsDev *stats;
    int32_t which, filter, n_per;
    const float *pose;
};

// the field of ONE map's obstacle plane (already of logData as it stands) into d_out; the handle's buffers exist
static int reach_run(gms_map *m, const uint32_t *d_obstacles, const gms_reach *r, const ReachSeeds &sd, uint16_t *d_out) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64, ntx = (W + RCH_T - 1) / RCH_T, nty = (H + RCH_T - 1) / RCH_T;
    if (nty > 65535) return gms_fail(GMS_ERR_INVALID, "gms_reach: a map of %d rows exceeds one launch", H);
    const uint32_t *d_blocked = d_obstacles;
    if (r->inflate > 0) {
        int rc = gms_reach_inflate(m, d_obstacles, r->inflate, r->mode, &d_blocked);
        if (rc) return rc;
    }
    const uint64_t *plane = reinterpret_cast<const uint64_t *>(d_blocked);
    const int64_t words32 = (m->gd.cells + 1) / 2;
    const int32_t ctl_words = RCH_CTL_WORDS + 2 * ntx * nty;
    hipLaunchKernelGGL(k_reach_init, dim3((unsigned)std::min<int64_t>(2048, (words32 + 255) / 256)), dim3(256), 0, m->stream,
                       reinterpret_cast<uint32_t *>(m->d_reach_field), words32, m->d_reach_ctl, ctl_words);
    HIPCHK(hipGetLastError());
    const int32_t n_seeds = sd.d_seeds ? sd.K : 1;
    hipLaunchKernelGGL(k_reach_seeds, dim3((unsigned)((n_seeds + 255) / 256)), dim3(256), 0, m->stream, m->gd, m->d_reach_field, plane, wpr64, ntx, m->d_reach_ctl,
                       sd.d_seeds, sd.K, sd.stats, sd.which, sd.filter, sd.n_per, sd.pose);
    HIPCHK(hipGetLastError());
    // Rounds in batches, the active count read back once per batch.  After round k every cell whose cheapest path crosses fewer than k
    // tile borders is final, a path within the cap has at most max_cost / 5 steps, and one more round sees nothing move.
    const int32_t bound = r->max_cost / GMS_REACH_AXIS + 2, batch = reach_batch();
    int32_t rounds = 0;
    m->reach_rounds = 0;
    m->reach_tile_runs = 0;
    for (;;) {
        const int32_t now = std::min(batch, bound - rounds);
        for (int32_t i = 0; i < now; i++, rounds++)
            hipLaunchKernelGGL(k_reach_round, dim3((unsigned)ntx, (unsigned)nty), dim3(RCH_T), 0, m->stream, m->d_reach_field, plane, wpr64, W, H, m->d_reach_ctl,
                               rounds, (uint32_t)r->max_cost);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(m->h_reach_ctl, m->d_reach_ctl, RCH_CTL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        m->reach_rounds = rounds;
        m->reach_tile_runs = (int64_t)(((uint64_t)m->h_reach_ctl[1] << 32) | m->h_reach_ctl[0]);
        if (m->h_reach_ctl[2 + (rounds & 3)] == 0u) break;                      // what the last round marked for the next one
        if (rounds >= bound)
            return gms_fail(GMS_ERR_INTERNAL, "gms_reach: tiles still active after %d rounds, the bound for max_cost = %d", rounds, r->max_cost);
    }
    const int64_t n = (int64_t)r->w * r->h;
    hipLaunchKernelGGL(k_reach_copy, dim3((unsigned)std::min<int64_t>(4096, (n + 255) / 256)), dim3(256), 0, m->stream, m->d_reach_field, W, r->x0, r->y0, r->w, r->h,
                       d_out);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the field of one map of a shared handle (seeds required) or of the shown particle of a per-particle one (K == 0 and no seeds: its own
// cell); `shown` exists for a particle only
static int reach(QuerySource src, const char *what, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !r || !out || (!src.s && !seeds))
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the output and -- for a map -- the seeds are required)", what);
    gms_map *m = src.m;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (rc) return rc;
    if (!((seeds && K >= 1 && K <= GMS_REACH_MAX_SEEDS) || (src.s && K == 0 && !seeds)))
        return gms_fail(GMS_ERR_INVALID, "%s: 1 <= K <= GMS_REACH_MAX_SEEDS seeds%s", what, src.s ? ", or K = 0 and no seeds (the shown particle's own cell)" : "");
    int64_t bytes = 0;
    rc = gms_reach_size(r, nullptr, nullptr, &bytes);
    if (!rc) rc = gms_rect_check(r->x0, r->y0, r->w, r->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if (on_device && (((uintptr_t)out & 1) != 0 || ((uintptr_t)seeds & 3) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s_dev: the output must be 2-byte aligned, the seeds 4-byte aligned", what);
    src.filter = r->filter;
    if (src.s && (rc = query_check(src, what, "gms_reach.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    rc = reach_buffers(m, r->inflate > 0);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t seed_bytes = (size_t)K * 2 * sizeof(int32_t), p_out = st.part((size_t)bytes), p_seeds = st.part(seed_bytes);
    rc = st.open();
    if (!rc && seeds) rc = st.up(p_seeds, seeds, seed_bytes);
    if (rc) return rc;
    ReachSeeds sd = {seeds ? st.at(p_seeds, seeds) : nullptr, K, nullptr, 0, 0, 0, nullptr};
    if (src.s) sd = {sd.d_seeds, K, src.s->pf->d_stats, src.index, src.filter, src.s->n_per, src.s->pf->d_pose};
    const uint32_t *plane = nullptr;
    rc = query_plane(src, r->mode, st.shown(shown), nullptr, &plane);
    if (!rc) rc = reach_run(m, plane, r, sd, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, (size_t)bytes);
    return st.finish(shown);
}

extern "C" {

int gms_reach_size(const gms_reach *r, int32_t *out_w, int32_t *out_h, int64_t *bytes) {
    REQUIRE(r, "gms_reach: null request");
    REQUIRE(r->w >= 1 && r->h >= 1, "gms_reach: w and h must be at least 1");
    REQUIRE(r->x0 >= 0 && r->y0 >= 0, "gms_reach: x0 and y0 must not be negative");
    REQUIRE(r->max_cost >= 1 && r->max_cost <= 0xFFFE, "gms_reach: 1 <= max_cost <= 0xFFFE");
    REQUIRE(r->inflate >= 0 && r->inflate <= 255, "gms_reach: 0 <= inflate <= 255 cells");
    REQUIRE(r->mode == GMS_CLEAR_OCCUPIED || r->mode == GMS_CLEAR_NOT_FREE, "gms_reach: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    if (out_w) *out_w = r->w;
    if (out_h) *out_h = r->h;
    if (bytes) *bytes = (int64_t)r->w * r->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_reach(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out) { return reach(query_map(m, mi), "gms_map_reach", r, seeds, K, out, nullptr, false); }
int gms_map_reach_dev(gms_map *m, int32_t mi, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out) {
    return reach(query_map(m, mi), "gms_map_reach", r, dev_seeds, K, dev_out, nullptr, true);
}
int gms_slam_reach(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *seeds, int32_t K, uint16_t *out, int32_t *shown) {
    return reach(query_slam(s, which), "gms_slam_reach", r, seeds, K, out, shown, false);
}
int gms_slam_reach_dev(gms_slam *s, int32_t which, const gms_reach *r, const int32_t *dev_seeds, int32_t K, uint16_t *dev_out, int32_t *dev_shown) {
    return reach(query_slam(s, which), "gms_slam_reach", r, dev_seeds, K, dev_out, dev_shown, true);
}
int gms_map_reach_stats(const gms_map *m, int32_t *rounds, int64_t *tile_runs) {
    REQUIRE(m, "gms_map_reach_stats: null handle");
    if (rounds) *rounds = m->reach_rounds;
    if (tile_runs) *tile_runs = m->reach_tile_runs;
    return GMS_OK;
}

}  // extern "C"
