// gms_relax_device.h -- the tile relaxation of the cost-to-go fields (gms_reach.hip) and of the rooms' growth (gms_rooms.hip): ONE copy of
// the round's body, its directional sweep, the tiles' marks and the host's round loop.  Both fields hold, per cell, a key whose numeric
// order is the order the relaxation minimises in, moved by the cost-to-go fields' steps (axis 5, diagonal 7, no corner cutting) through
// the cells that are not blocked, capped at max_cost.  All integer arithmetic; the field is unique, so however the relaxation is scheduled
// the result is the same.  The two differ in WHAT A CELL HOLDS alone, a compile-time policy P:
//   P::Cell, P::FAR           the cell's type and "no path": a uint16 cost / 0xFFFF, or the uint32 key cost << 16 | rank / 0xFFFFFFFF, whose
//                             numeric order is the lexicographic order of (cost, rank)
//   P::PITCH                  the LDS row pitch in cells (the bank argument below)
//   P::CTL_WORDS              the control words ahead of the tiles' flags: [0..1] tile runs, [2..5] active counts, the rest the unit's own
//   P::load, P::store         a cell of the field in memory: plain, or relaxed atomic where one aligned store must publish cost and rank together
//   P::Params, P::KEYED       the cap's limits, by value, and which of the two relaxations of ONE cell from its three neighbours behind the
//                             walk relax_sweep takes.  The two steps stand in the sweep itself, under if constexpr, and not behind a call
//                             of the policy's: values that arrive as a function's arguments are known to be defined, the compiler then
//                             joins their tests with a plain `or` where the sweep's own locals get the poison-safe select, and both
//                             kernels come out a few instructions longer than the code this body was taken from.
// Each unit keeps its __global__ kernel, supplies the __shared__ array and makes a single call to relax_round<P>.
//
//   relax_round         ONE ROUND: a workgroup of one wavefront per 64 x 64 tile; the tiles that are not active leave at once.  An active
//                       tile loads its cells and a one-cell halo into LDS (66 x 66 cells), relaxes to ITS fixpoint against that halo,
//                       writes back what changed and marks the neighbours across every edge or corner whose cell changed active for the
//                       NEXT round.  No workgroup waits on another; a halo that a neighbour rewrites in the same round is read old or
//                       new, both upper bounds of the true key, and the neighbour's mark brings the tile back.
//   the seeds           a round marks across an edge only where a cell CHANGED, and a seed's own cell never does, so a seed whose
//                       neighbours inside its tile are all blocked (or whose tile is one cell) would hand nothing on: whoever plants a
//                       seed marks its tile and the tiles of its eight neighbours by itself (relax_mark_around, or relax_mark per word).
//
// The relaxation inside a tile is four directional sweeps, east, west, south, north, repeated until a whole pass changes nothing (and
// never more than the tile has cells).  The east sweep: lane y owns row y and walks x = 0 .. 63; the value it needs from the west is
// the one it has just computed, in a register, and the two diagonal ones are its neighbour lanes' registers, one DPP wavefront shift
// each -- the chain from one column to the next holds no LDS access.  Lanes 0 and 63 take the halo row's value instead (held in a
// register per lane, fetched with a uniform lane read).  The south and north sweeps are the same code with lane = column.  A sweep
// carries a key across the whole tile, so open space settles in two passes and a third sees nothing move.
//
// LDS, 66 rows of P::PITCH cells.  The east / west sweeps have a lane per row, the south / north sweeps and the tile's load and store
// a lane per column.
//   uint16, pitch 66    8712 bytes, row pitch 33 dwords.  A lane per row reads and writes dword 33 lane + c / 2: bank (33 lane + const)
//                       mod 32 = (lane + const) mod 32, distinct within each half-wave (16-bit accesses bank by 32 per 32 lanes).  A lane
//                       per column touches 64 consecutive uint16: 16 consecutive dwords per half-wave, two lanes to a dword.
//   uint32, pitch 67    17688 bytes.  ds_read_b32 / ds_write_b32 bank by (address / 4) mod 32 within each 32-lane half.  A lane per row
//                       touches dword 67 l + c, bank (3 l + c) mod 32, and 3 is odd, so the 32 lanes of a half hit 32 different banks.
//                       An even pitch -- the 66 dwords the tile's width suggests, or twice the uint16 field's 33 -- would put lanes l
//                       and l + 16 of a half on one bank (16 * 66 = 33 * 32), two-way on every access of the sweep.  A lane per column:
//                       64 consecutive dwords, conflict-free at any pitch.
#pragma once

#include <stdlib.h>

#include <algorithm>

#include "gms_device.h"

#define RLX_T 64                         // tile edge in cells = lanes of the round's workgroup = cells of a plane word
#define RLX_ROWS (RLX_T + 2)             // the tile and its halo
#define RLX_BATCH_DEFAULT 8              // rounds per read-back

// ---- what a cell holds ----
// the cost alone (gms_reach.hip)
struct ReachCells {
    typedef uint16_t Cell;
    struct Params { uint32_t max_cost; };
    static constexpr uint32_t FAR = 0xffffu;
    static constexpr int PITCH = RLX_ROWS;
    static constexpr int CTL_WORDS = 8;
    static constexpr bool KEYED = false;
    __device__ __forceinline__ static Cell load(const Cell *p) { return *p; }
    __device__ __forceinline__ static void store(Cell *p, Cell v) { *p = v; }
};
// cost << 16 | rank (gms_rooms.hip), KEYED: a relaxation is min(cur, neighbour + (step << 16)).  The cap test is made on the neighbour's
// key BEFORE the add (key < lim = (max_cost - step + 1) << 16, 0 where max_cost < step), so no candidate is ever formed that could wrap
struct RoomKeys {
    typedef uint32_t Cell;
    struct Params { uint32_t lim_axis, lim_diag; };
    static constexpr uint32_t FAR = 0xffffffffu;
    static constexpr int PITCH = 67;
    static constexpr int CTL_WORDS = 16;
    static constexpr bool KEYED = true;
    __device__ __forceinline__ static Cell load(const Cell *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    __device__ __forceinline__ static void store(Cell *p, Cell v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }   // (one aligned dword: cost and rank are published together)
};

// lane l receives lane l - 1's v (lane 0 keeps its own) / lane l + 1's (lane 63 keeps its own): DPP wave_shr:1 / wave_shl:1
__device__ __forceinline__ uint32_t relax_from_below(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t relax_from_above(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false); }

// tile active in the round whose flags and count these are; the first to raise a flag counts it
__device__ __forceinline__ void relax_mark(uint32_t *flags, uint32_t *count, int32_t tile) {
    if (atomicExch(&flags[tile], 1u) == 0u) atomicAdd(count, 1u);
}

// the tile of cell (gx, gy) of a W x H map and the tiles of its eight neighbours on the map (a cell inside its tile marks that tile nine
// times: one count)
__device__ __forceinline__ void relax_mark_around(uint32_t *flags, uint32_t *count, int32_t gx, int32_t gy, int32_t W, int32_t H, int32_t ntx) {
    for (int32_t dy = -1; dy <= 1; dy++)
        for (int32_t dx = -1; dx <= 1; dx++) {
            const int32_t nx = gx + dx, ny = gy + dy;
            if (nx >= 0 && ny >= 0 && nx < W && ny < H) relax_mark(flags, count, (ny >> 6) * ntx + (nx >> 6));
        }
}

// One directional sweep of the tile s (66 x 66, cell (t, l) at s[(l + 1) * SL + (t + 1) * ST]): lane l owns line l and walks t = 0 .. 63
// (DIR > 0) or 63 .. 0.  me / lo / hi: the blocked bits (bit t) of lines l, l - 1 and l + 1; start_blocked: the halo cell the walk starts
// from.  true: the lane lowered a cell
template <typename P, int SL, int ST, int DIR>
__device__ __forceinline__ bool relax_sweep(typename P::Cell *s, int32_t lane, uint64_t me, uint64_t lo, uint64_t hi, bool start_blocked, typename P::Params q) {
    constexpr int T0 = DIR > 0 ? 0 : RLX_T - 1;
    typename P::Cell *cell = s + (lane + 1) * SL + (T0 + 1) * ST;
    // the halo lines beside lane 0 and lane 63, entry t in lane t; the corner the walk starts beside, everywhere
    const uint32_t line_lo = s[0 * SL + (lane + 1) * ST], line_hi = s[(RLX_ROWS - 1) * SL + (lane + 1) * ST];
    uint32_t halo_lo = s[0 * SL + (T0 - DIR + 1) * ST], halo_hi = s[(RLX_ROWS - 1) * SL + (T0 - DIR + 1) * ST];
    uint32_t prev = cell[-DIR * ST];
    bool prev_free = !start_blocked, changed = false;
    uint32_t cur = *cell;
#pragma unroll 4
    for (int32_t i = 0; i < RLX_T; i++) {
        const int32_t t = T0 + DIR * i;
        const uint32_t next = i + 1 < RLX_T ? cell[DIR * ST] : 0u;              // (nobody writes it before this lane does)
        uint32_t from_lo = relax_from_below(prev), from_hi = relax_from_above(prev);
        if (lane == 0) from_lo = halo_lo;
        if (lane == RLX_T - 1) from_hi = halo_hi;
        const bool me_b = (me >> t) & 1ull, lo_b = (lo >> t) & 1ull, hi_b = (hi >> t) & 1ull;
        uint32_t best;
        if constexpr (!P::KEYED) {
            best = min(cur, prev + GMS_REACH_AXIS);                                               // (32 bits: FAR + 7 stays above every cap)
            if (prev_free && !lo_b) best = min(best, from_lo + GMS_REACH_DIAG);                   // the two cells the step squeezes between
            if (prev_free && !hi_b) best = min(best, from_hi + GMS_REACH_DIAG);
            if (best > q.max_cost || me_b) best = P::FAR;
        } else {
            best = cur;
            if (prev < q.lim_axis) best = min(best, prev + ((uint32_t)GMS_REACH_AXIS << 16));      // (the cap test ahead of the add: nothing wraps)
            if (prev_free && !lo_b && from_lo < q.lim_diag) best = min(best, from_lo + ((uint32_t)GMS_REACH_DIAG << 16));
            if (prev_free && !hi_b && from_hi < q.lim_diag) best = min(best, from_hi + ((uint32_t)GMS_REACH_DIAG << 16));
            if (me_b) best = P::FAR;
        }
        if (best != cur) { *cell = (typename P::Cell)best; changed = true; }
        prev = best;
        prev_free = !me_b;
        halo_lo = (uint32_t)__builtin_amdgcn_readlane((int)line_lo, t);
        halo_hi = (uint32_t)__builtin_amdgcn_readlane((int)line_hi, t);
        cur = next;
        cell += DIR * ST;
    }
    return changed;
}

// The body of a round's kernel, launched (ntx, nty) x RLX_T: s the unit's LDS of RLX_ROWS * P::PITCH cells; field [H][W]; plane: ONE
// map's blocked plane, H rows of wpr64 words; ctl: P::CTL_WORDS control words, then the tiles' flags of the even and of the odd rounds
template <typename P>
__device__ __forceinline__ void relax_round(typename P::Cell *s, typename P::Cell *field, const uint64_t *plane, int32_t wpr64, int32_t W, int32_t H,
                                            uint32_t *ctl, int32_t round, typename P::Params q) {
    typedef typename P::Cell Cell;
    constexpr int PITCH = P::PITCH;
    const int32_t lane = (int32_t)threadIdx.x, tx = (int32_t)blockIdx.x, ty = (int32_t)blockIdx.y, ntx = (int32_t)gridDim.x, nty = (int32_t)gridDim.y;
    const int32_t tile = ty * ntx + tx, ntiles = ntx * nty;
    uint32_t *count = ctl + 2, *flags_cur = ctl + P::CTL_WORDS + (size_t)(round & 1) * (size_t)ntiles;
    uint32_t *flags_next = ctl + P::CTL_WORDS + (size_t)((round + 1) & 1) * (size_t)ntiles;
    if (tile == 0 && lane == 0) count[(round + 2) & 3] = 0u;                   // (this round counts into slot round + 1; round - 1 counted into this round's)
    if (flags_cur[tile] == 0u) return;                                          // (uniform)
    __syncthreads();
    if (lane == 0) {
        flags_cur[tile] = 0u;                                                   // (nobody else touches this round's flag of this tile)
        atomicAdd(reinterpret_cast<unsigned long long *>(ctl), 1ull);
    }
    const int32_t x0 = tx * RLX_T, y0 = ty * RLX_T, x = x0 + lane;
    for (int32_t r = 0; r < RLX_ROWS; r++) {                                    // the tile and its halo; what lies off the map is FAR
        const int32_t y = y0 + r - 1;
        const bool row_in = y >= 0 && y < H;
        const Cell *src = field + (size_t)(row_in ? y : 0) * (size_t)W;
        s[r * PITCH + lane + 1] = row_in && x < W ? P::load(src + x) : (Cell)P::FAR;
        if (lane < 2) {
            const int32_t xe = lane == 0 ? x0 - 1 : x0 + RLX_T;
            s[r * PITCH + (lane == 0 ? 0 : RLX_ROWS - 1)] = row_in && xe >= 0 && xe < W ? P::load(src + xe) : (Cell)P::FAR;
        }
    }
    // the blocked bits: a tile's row is one word of the plane; what lies off the map is blocked
    const uint64_t ragged = W - x0 < RLX_T ? ~0ull << (W - x0) : 0ull;
    auto row_word = [&](int32_t y) -> uint64_t { return y >= 0 && y < H ? (plane[(size_t)y * (size_t)wpr64 + (size_t)tx] | ragged) : ~0ull; };
    auto left_bit = [&](int32_t y) -> bool { return y >= 0 && y < H && tx > 0 ? (plane[(size_t)y * (size_t)wpr64 + (size_t)(tx - 1)] >> 63) != 0ull : true; };
    auto right_bit = [&](int32_t y) -> bool { return y >= 0 && y < H && x0 + RLX_T < W ? (plane[(size_t)y * (size_t)wpr64 + (size_t)(tx + 1)] & 1ull) != 0ull : true; };
    const uint64_t row_me = row_word(y0 + lane), row_lo = row_word(y0 + lane - 1), row_hi = row_word(y0 + lane + 1);
    const bool row_left = left_bit(y0 + lane), row_right = right_bit(y0 + lane);
    uint64_t col_me = 0ull;                                                     // lane = column: bit y of it
    for (int32_t r = 0; r < RLX_T; r++) col_me |= ((row_word(y0 + r) >> lane) & 1ull) << r;
    uint64_t col_lo = (uint64_t)__shfl_up((long long)col_me, 1), col_hi = (uint64_t)__shfl_down((long long)col_me, 1);
    const uint64_t halo_left = __ballot(row_left), halo_right = __ballot(row_right);
    if (lane == 0) col_lo = halo_left;
    if (lane == RLX_T - 1) col_hi = halo_right;
    const bool col_top = (row_word(y0 - 1) >> lane) & 1ull, col_bottom = (row_word(y0 + RLX_T) >> lane) & 1ull;
    __syncthreads();
    for (int32_t pass = 0; pass < RLX_T * RLX_T; pass++) {                      // (the vote ends it; the bound is the tile's cells)
        bool changed = relax_sweep<P, PITCH, 1, 1>(s, lane, row_me, row_lo, row_hi, row_left, q);
        changed |= relax_sweep<P, PITCH, 1, -1>(s, lane, row_me, row_lo, row_hi, row_right, q);
        __syncthreads();
        changed |= relax_sweep<P, 1, PITCH, 1>(s, lane, col_me, col_lo, col_hi, col_top, q);
        changed |= relax_sweep<P, 1, PITCH, -1>(s, lane, col_me, col_lo, col_hi, col_bottom, q);
        __syncthreads();
        if (!__any(changed)) break;
    }
    uint32_t moved = 0u;                                                        // bit 0: a cell of row 0 changed, 1: of row 63, 2: of column 0, 3: of column 63
    const int32_t rows = min(RLX_T, H - y0);
    if (x < W)
        for (int32_t r = 0; r < rows; r++) {
            Cell *dst = field + (size_t)(y0 + r) * (size_t)W + (size_t)x;
            const Cell v = s[(r + 1) * PITCH + lane + 1];
            if (v != *dst) {
                P::store(dst, v);
                moved |= (r == 0 ? 1u : 0u) | (r == RLX_T - 1 ? 2u : 0u) | (lane == 0 ? 4u : 0u) | (lane == RLX_T - 1 ? 8u : 0u);
            }
        }
    const uint64_t top = __ballot(moved & 1u), bottom = __ballot(moved & 2u), left = __ballot(moved & 4u), right = __ballot(moved & 8u);
    if (lane != 0) return;
    uint32_t *cnt = count + ((round + 1) & 3);
    const bool n = ty > 0, so = ty + 1 < nty, w = tx > 0, e = tx + 1 < ntx;
    if (top && n) relax_mark(flags_next, cnt, tile - ntx);
    if (bottom && so) relax_mark(flags_next, cnt, tile + ntx);
    if (left && w) relax_mark(flags_next, cnt, tile - 1);
    if (right && e) relax_mark(flags_next, cnt, tile + 1);
    if ((top & 1ull) && n && w) relax_mark(flags_next, cnt, tile - ntx - 1);                      // the corner cells: the tile across the corner
    if ((top >> 63) && n && e) relax_mark(flags_next, cnt, tile - ntx + 1);
    if ((bottom & 1ull) && so && w) relax_mark(flags_next, cnt, tile + ntx - 1);
    if ((bottom >> 63) && so && e) relax_mark(flags_next, cnt, tile + ntx + 1);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// rounds per read-back, from the environment variable `name`, read per call
static inline int32_t relax_batch(const char *name) {
    const char *e = getenv(name);
    const int32_t b = e ? atoi(e) : RLX_BATCH_DEFAULT;
    return std::min(64, std::max(1, b));
}

// the first ctl_words control words into their pinned mirror; waits on the stream
static inline int relax_read_ctl(hipStream_t st, const uint32_t *d_ctl, uint32_t *h_ctl, int32_t ctl_words) {
    HIPCHK(hipMemcpyAsync(h_ctl, d_ctl, (size_t)ctl_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GMS_OK;
}

// Rounds in batches, the active count read back once per batch; launch(round) enqueues one round.  After round k every cell whose best
// path crosses fewer than k tile borders is final, a path within the cap has at most max_cost / 5 steps, and one more round sees nothing
// move: max_cost / 5 + 2 rounds bound the loop.  *rounds and *tile_runs follow every read-back; who: the error message's prefix
template <typename Launch>
static int relax_rounds(hipStream_t st, const uint32_t *d_ctl, uint32_t *h_ctl, int32_t ctl_words, int32_t max_cost, int32_t batch, Launch launch, const char *who,
                        int32_t *rounds_out, int64_t *tile_runs) {
    const int32_t bound = max_cost / GMS_REACH_AXIS + 2;
    int32_t rounds = 0;
    for (;;) {
        const int32_t now = std::min(batch, bound - rounds);
        for (int32_t i = 0; i < now; i++, rounds++) launch(rounds);
        HIPCHK(hipGetLastError());
        const int rc = relax_read_ctl(st, d_ctl, h_ctl, ctl_words);
        if (rc) return rc;
        *rounds_out = rounds;
        *tile_runs = (int64_t)(((uint64_t)h_ctl[1] << 32) | h_ctl[0]);
        if (h_ctl[2 + (rounds & 3)] == 0u) return GMS_OK;                       // what the last round marked for the next one
        if (rounds >= bound) return gms_fail(GMS_ERR_INTERNAL, "%s: tiles still active after %d rounds, the bound for max_cost = %d", who, rounds, max_cost);
    }
}
