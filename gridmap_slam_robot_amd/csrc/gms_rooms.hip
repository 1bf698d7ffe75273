// gms_rooms.hip -- rooms and doors (gridmapslam.h "rooms and doors"): the free space eroded until rooms fall apart (the CORES: the
// 4-connected sets of cells not blocked at inflation `core`), the cores of at least min_core cells ranked by their anchors (the ROOMS),
// grown back over the cells not blocked at inflation `inflate` by the cost-to-go fields' moves -- every cell to the room that
// minimises (cost, rank) -- and the DOORS: the pairs of rooms whose cells touch across a cell edge.  All integer arithmetic; every
// output is unique, so however the unions, the relaxation and the atomics are scheduled the result is the same.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.  The union, the group loop, the wavefront reductions and the scan's look-up are gms_regions.h's, the scan
// is the query base's, the blocked planes are gms_reach_inflate's.
//
//   the two blocked planes   gms_reach_inflate at R = core into the handle's scratch plane; k_rooms_core turns it into the CORE PLANE (a
//                       bit per core cell, the padding zero) in a plane of this unit's own, so that the scratch plane is free for
//                       gms_reach_inflate at R = inflate (inflate == 0: the obstacle plane itself, read in place).
//   k_rooms_tiles, k_rooms_merge, k_rooms_flatten   the 4-connected labelling: region_tile_label and region_border_merge of gms_regions.h
//                       without the diagonal links, then the chase to the root; the flatten also counts every core's cells at its root
//                       (wave_each_key, one atomic per group) -- in the working field, which nobody uses yet.
//   k_rooms_keep        the plane of the roots with count >= min_core and its word counts; gms_launch_scan ranks them in anchor order;
//                       the total, the number of rooms, is read back once (the tables' size, the 0xFFFF check).
//   k_rooms_seed        every cell of a room gets the working key 0 << 16 | rank, every other cell 0xFFFFFFFF; the root writes its
//                       record's anchor and core_count.  A room cell with one of its eight neighbours on the map outside the core
//                       plane is on the RIM; the tile of a rim cell and the tiles of its eight neighbours are marked active (a seed
//                       never changes, so it must mark by itself), one lane per wavefront from the rim's ballot.
//   k_rooms_round       ONE ROUND of the tile relaxation on the uint32 field cost << 16 | rank: relax_round<RoomKeys> of
//                       gms_relax_device.h, which holds the scheme, its proof, the sweeps, the cap test and the LDS banks' argument.
//   k_rooms_out         labels and depth of the rectangle through the rank -> anchor table.
//   k_rooms_records     count, box, sums and max_depth per room by integer atomics, the lanes that share a room combined first.
//   k_rooms_contacts    a lane per cell looks east and south, so every contact is seen once; the pair's key rank_a << 16 | rank_b
//                       (a < b) is inserted into an open-addressing table on the handle by atomicCAS and count, box and sums are
//                       accumulated by integer atomics, the lanes that share a pair combined first.  A table more than half full
//                       raises a flag: the host doubles it and runs the step again.
//   k_rooms_door_count, gms_launch_scan, k_rooms_door_bucket, k_rooms_doors
//                       the entries in key order: the doors whose SMALLER room is a form one run of the output; the runs' lengths
//                       are counted and scanned over the rooms, every entry takes a slot of its run, and its place is the run's
//                       start plus the number of smaller keys within the run -- the sum of the squared run lengths in all, not the
//                       square of the table.  It writes its record there and adds one to `doors` of both rooms.  k_rooms_emit
//                       copies the first cap_rooms room records out.
#undef GMS_STAMPS
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>

#include "gms_regions.h"
#include "gms_relax_device.h"

#define RMS_T RLX_T                      // tile edge in cells = cells of a plane word
#define RMS_NT 256
#define RMS_NONE RoomKeys::FAR
#define RMS_CTL_WORDS RoomKeys::CTL_WORDS                                       // d_rooms_ctl: [0..1] tile runs, [2..5] active counts, [6] rooms, [7] door entries, [8] door table overflow; the flags behind
#define RMS_DOOR_CAP0 64                 // entries the handle's door table holds at first (a power of two; it is kept at most half full)

static_assert(GMS_ROOM_NONE == RMS_NONE && GMS_ROOMS_MAX == 0xFFFF, "the header's constants are the kernels'");
static_assert(RMS_T == REGION_T && RMS_NT == REGION_NT, "the labelling's tile and workgroup are the relaxation's tile and this unit's workgroup");
static_assert(sizeof(gms_rooms) == 48 && sizeof(gms_room) == 56 && offsetof(gms_room, core_count) == 8 && offsetof(gms_room, min_x) == 16 &&
              offsetof(gms_room, max_depth) == 32 && offsetof(gms_room, doors) == 36 && offsetof(gms_room, sum_x) == 40, "the header fixes the room record's offsets");
static_assert(sizeof(gms_door) == 48 && offsetof(gms_door, count) == 8 && offsetof(gms_door, min_x) == 12 && offsetof(gms_door, sum_x2) == 32,
              "the header fixes the door record's offsets");

// what a door table entry accumulates beside its key
struct RoomsDoorAcc {
    int32_t count, min_x, min_y, max_x, max_y, pad;
    unsigned long long sum_x2, sum_y2;
};

// blocked: ONE map's blocked plane at inflation `core`, H rows of wpr64 words; core: the core plane; field: [cells] zeroed (the cores'
// counts); ctl zeroed
__global__ void __launch_bounds__(RMS_NT)
k_rooms_core(const uint64_t *__restrict__ blocked, int32_t W, int32_t H, int32_t wpr64, uint64_t *__restrict__ core, uint32_t *__restrict__ field, int64_t cells,
             uint32_t *__restrict__ ctl, int32_t ctl_words) {
    const int64_t i0 = (int64_t)blockIdx.x * RMS_NT + threadIdx.x, step = (int64_t)gridDim.x * RMS_NT, words = (int64_t)H * wpr64;
    for (int64_t i = i0; i < words; i += step) {
        const int32_t wx = (int32_t)(i % wpr64);
        const uint64_t on_map = wx == wpr64 - 1 && (W & 63) ? (1ull << (W & 63)) - 1ull : ~0ull;
        core[i] = ~blocked[i] & on_map;
    }
    for (int64_t i = i0; i < cells; i += step) field[i] = 0u;
    for (int64_t i = i0; i < ctl_words; i += step) ctl[i] = 0u;
}

// plane: the core plane; label [H][W]; grid (ntx, nty)
__global__ void __launch_bounds__(RMS_NT)
k_rooms_tiles(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *__restrict__ label) {
    region_tile_label<false>(plane, wpr64, W, H, label);
}

// a lane per cell behind a tile border, united with the ONE cell across the edge -- 4-connectivity has no link across a corner
__global__ void __launch_bounds__(RMS_NT)
k_rooms_merge(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, int32_t ntx, int32_t nty, uint32_t *label) {
    region_border_merge<false>(plane, wpr64, W, H, ntx, nty, label);
}

// a wavefront per word of the core plane: the chase to the root, and every core's cells counted at its root (count [cells], zeroed)
__global__ void __launch_bounds__(RMS_NT)
k_rooms_flatten(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *label, uint32_t *count) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (RMS_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const uint64_t bits = plane[word];
    if (bits == 0ull) return;                                                   // (uniform)
    uint32_t root = RMS_NONE;
    if ((bits >> lane) & 1ull) {
        const int32_t y = (int32_t)(word / wpr64), x = (int32_t)(word - (int64_t)y * wpr64) * 64 + lane;
        const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        root = region_find(label, c);
        if (root != c) __atomic_store_n(label + c, root, __ATOMIC_RELAXED);     // (another lane's chase reads the old parent or the root: both lead there)
    }
    wave_each_key(root, RMS_NONE, [&](uint32_t R, bool, uint64_t grp, bool leader) {
        if (leader) atomicAdd(count + R, (uint32_t)__popcll(grp));
    });
}

// a wavefront per word: kept = the plane of the roots whose core has at least min_core cells; wcount [words] its word counts
__global__ void __launch_bounds__(RMS_NT)
k_rooms_keep(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, const uint32_t *__restrict__ label, const uint32_t *__restrict__ count,
             uint32_t min_core, uint64_t *__restrict__ kept, uint32_t *__restrict__ wcount) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (RMS_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const uint64_t bits = plane[word];
    bool keep = false;
    if ((bits >> lane) & 1ull) {
        const int32_t y = (int32_t)(word / wpr64), x = (int32_t)(word - (int64_t)y * wpr64) * 64 + lane;
        const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        keep = label[c] == c && count[c] >= min_core;
    }
    const uint64_t kb = __ballot(keep);
    if (lane == 0) {
        kept[word] = kb;
        wcount[word] = (uint32_t)__popcll(kb);
    }
}

// the first n room records and the rooms' door buckets: dcnt / dsize / dfill [n], the doors whose smaller room it is
__global__ void __launch_bounds__(RMS_NT)
k_rooms_table_init(gms_room *__restrict__ rec, uint32_t *__restrict__ dcnt, uint32_t *__restrict__ dsize, uint32_t *__restrict__ dfill, int32_t n) {
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RMS_NT) {
        rec[i] = gms_room{0, 0, 0, 0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0, 0};
        dcnt[i] = dsize[i] = dfill[i] = 0u;
    }
}

// a wavefront per word of the planes.  core / kept: the core plane and the kept roots' plane, wscan / wblocks the scan of its counts;
// field: the cores' counts in, the working keys out; rec / anchor: the rooms' tables (cap entries: a rank behind it writes nothing)
__global__ void __launch_bounds__(RMS_NT)
k_rooms_seed(const uint64_t *__restrict__ core, const uint64_t *__restrict__ kept, const uint32_t *__restrict__ wscan, const uint32_t *__restrict__ wblocks,
             int32_t wpr64, int32_t W, int32_t H, const uint32_t *__restrict__ label, uint32_t *field, int32_t ntx, int32_t nty, uint32_t *ctl,
             gms_room *__restrict__ rec, uint32_t *__restrict__ anchor, int32_t cap) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (RMS_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const int32_t y = (int32_t)(word / wpr64), wx = (int32_t)(word - (int64_t)y * wpr64), x = wx * 64 + lane;
    const uint64_t bits = core[word];
    uint32_t key = RMS_NONE;
    if ((bits >> lane) & 1ull) {
        const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x, r = label[c];
        const uint32_t ry = r / (uint32_t)W, rx = r - ry * (uint32_t)W;
        const size_t rw = (size_t)ry * (size_t)wpr64 + (size_t)(rx >> 6);
        const uint64_t kw = kept[rw];
        if ((kw >> (rx & 63u)) & 1ull) {
            key = scan_prefix(wscan, wblocks, rw) + (uint32_t)__popcll(kw & ((1ull << (rx & 63u)) - 1ull));
            if (r == c && key < (uint32_t)cap) {                                // (the root alone writes these)
                anchor[key] = c;
                rec[key].anchor_x = x;
                rec[key].anchor_y = y;
                rec[key].core_count = (int32_t)field[c];
            }
        }
    }
    if (x < W) field[(size_t)y * (size_t)W + (size_t)x] = key;
    const uint64_t room = __ballot(key != RMS_NONE);
    if (room == 0ull) return;                                                   // (uniform)
    // the rim: a room cell with one of its eight neighbours ON THE MAP outside the core plane (what is off the map counts as inside)
    const uint64_t ragged = wx == wpr64 - 1 && (W & 63) ? ~0ull << (W & 63) : 0ull;
    uint64_t inside = ~0ull;
    for (int32_t d = -1; d <= 1; d++) {
        const int32_t yy = y + d;
        if (yy < 0 || yy >= H) continue;
        const uint64_t *row = core + (size_t)yy * (size_t)wpr64;
        const uint64_t w = row[wx] | ragged;
        const uint64_t from_w = wx > 0 ? row[wx - 1] >> 63 : 1ull, from_e = wx + 1 < wpr64 ? row[wx + 1] & 1ull : 1ull;
        inside &= w & ((w << 1) | from_w) & ((w >> 1) | (from_e << 63));
    }
    const uint64_t rim = room & ~inside;
    if (rim == 0ull || lane != 0) return;
    uint32_t *flags = ctl + RMS_CTL_WORDS, *cnt = ctl + 2;                      // round 0's flags and count
    const int32_t ty = y >> 6, tile = ty * ntx + wx;
    const bool w = (rim & 1ull) && wx > 0, e = (rim >> 63) && wx + 1 < ntx, n = (y & 63) == 0 && ty > 0, s = (y & 63) == 63 && ty + 1 < nty;
    relax_mark(flags, cnt, tile);
    if (w) relax_mark(flags, cnt, tile - 1);
    if (e) relax_mark(flags, cnt, tile + 1);
    if (n) relax_mark(flags, cnt, tile - ntx);
    if (s) relax_mark(flags, cnt, tile + ntx);
    if (n && w) relax_mark(flags, cnt, tile - ntx - 1);
    if (n && e) relax_mark(flags, cnt, tile - ntx + 1);
    if (s && w) relax_mark(flags, cnt, tile + ntx - 1);
    if (s && e) relax_mark(flags, cnt, tile + ntx + 1);
}

// field [H][W] of keys; plane: ONE map's blocked plane at inflation `inflate`, H rows of wpr64 words; grid (ntx, nty), a wavefront per
// tile; ctl as d_rooms_ctl
__global__ void __launch_bounds__(RMS_T)
k_rooms_round(uint32_t *field, const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *ctl, int32_t round, uint32_t lim_axis,
              uint32_t lim_diag) {
    __shared__ uint32_t s[RLX_ROWS * RoomKeys::PITCH];
    relax_round<RoomKeys>(s, field, plane, wpr64, W, H, ctl, round, RoomKeys::Params{lim_axis, lim_diag});
}

// labels, depth (either may be NULL) [h][w]
__global__ void __launch_bounds__(RMS_NT)
k_rooms_out(const uint32_t *__restrict__ field, const uint32_t *__restrict__ anchor, int32_t W, int32_t x0, int32_t y0, int32_t w, int32_t h,
            uint32_t *__restrict__ labels, uint16_t *__restrict__ depth) {
    const int64_t n = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RMS_NT) {
        const int32_t y = y0 + (int32_t)(i / w), x = x0 + (int32_t)(i % w);
        const uint32_t key = field[(size_t)y * (size_t)W + (size_t)x];
        if (labels) labels[i] = key != RMS_NONE ? anchor[key & 0xffffu] : RMS_NONE;
        if (depth) depth[i] = (uint16_t)(key >> 16);                            // (no room: 0xFFFF = GMS_REACH_FAR)
    }
}

// a wavefront per 64 cells of a row: count, box, sums and max_depth of every room
__global__ void __launch_bounds__(RMS_NT)
k_rooms_records(const uint32_t *__restrict__ field, int32_t wpr64, int32_t W, int32_t H, gms_room *rec) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (RMS_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const int32_t y = (int32_t)(word / wpr64), xw = (int32_t)(word - (int64_t)y * wpr64) * 64, x = xw + lane;
    const uint32_t key = x < W ? field[(size_t)y * (size_t)W + (size_t)x] : RMS_NONE;
    const uint32_t rank = key != RMS_NONE ? key & 0xffffu : RMS_NONE;
    wave_each_key(rank, RMS_NONE, [&](uint32_t R, bool in, uint64_t grp, bool leader) {
        const int32_t deepest = wave_max(in ? (int32_t)(key >> 16) : 0);
        if (!leader) return;
        const int32_t n = __popcll(grp);
        gms_room *q = rec + R;
        atomicAdd(&q->count, n);
        atomicMin(&q->min_x, xw + __builtin_ctzll(grp));
        atomicMax(&q->max_x, xw + 63 - __builtin_clzll(grp));
        atomicMin(&q->min_y, y);
        atomicMax(&q->max_y, y);
        atomicMax(&q->max_depth, deepest);
        atomicAdd(reinterpret_cast<unsigned long long *>(&q->sum_x), (unsigned long long)((int64_t)n * xw + region_bit_sum(grp)));
        atomicAdd(reinterpret_cast<unsigned long long *>(&q->sum_y), (unsigned long long)((int64_t)n * y));
    });
}

// keys / acc [cap]; the two door counters of ctl
__global__ void __launch_bounds__(RMS_NT)
k_rooms_doors_init(uint32_t *__restrict__ keys, RoomsDoorAcc *__restrict__ acc, int32_t cap, uint32_t *__restrict__ ctl) {
    const int64_t i0 = (int64_t)blockIdx.x * RMS_NT + threadIdx.x;
    for (int64_t i = i0; i < cap; i += (int64_t)gridDim.x * RMS_NT) {
        keys[i] = RMS_NONE;
        acc[i] = RoomsDoorAcc{0, INT_MAX, INT_MAX, -1, -1, 0, 0ull, 0ull};
    }
    if (i0 < 2) ctl[7 + i0] = 0u;
}

// the entry of `key` in the table of cap = mask + 1 entries, inserted if it is new; -1: no entry (the table is full); ctl[7] counts the
// entries, ctl[8] is raised as soon as the table is more than half full
__device__ __forceinline__ int32_t rooms_door_entry(uint32_t *keys, uint32_t mask, uint32_t key, uint32_t *ctl) {
    uint32_t h = ((key * 0x9E3779B1u) >> 12) & mask;
    for (uint32_t i = 0; i <= mask; i++, h = (h + 1u) & mask) {
        const uint32_t old = atomicCAS(keys + h, RMS_NONE, key);
        if (old == RMS_NONE) {
            if (2u * (atomicAdd(ctl + 7, 1u) + 1u) > mask + 1u) atomicOr(ctl + 8, 1u);
            return (int32_t)h;
        }
        if (old == key) return (int32_t)h;
    }
    atomicOr(ctl + 8, 1u);
    return -1;
}

// a wavefront per 64 cells of a row: the contacts with the cell to the east and with the cell to the south
__global__ void __launch_bounds__(RMS_NT)
k_rooms_contacts(const uint32_t *__restrict__ field, int32_t wpr64, int32_t W, int32_t H, uint32_t *keys, RoomsDoorAcc *acc, uint32_t mask, uint32_t *ctl) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * (RMS_NT / 64) + ((int32_t)threadIdx.x >> 6);
    if (word >= (int64_t)H * wpr64) return;                                     // (uniform per wavefront)
    const int32_t y = (int32_t)(word / wpr64), xw = (int32_t)(word - (int64_t)y * wpr64) * 64, x = xw + lane;
    auto rank_at = [&](int32_t cx, int32_t cy) -> uint32_t {
        if (cx >= W || cy >= H) return RMS_NONE;
        const uint32_t k = field[(size_t)cy * (size_t)W + (size_t)cx];
        return k != RMS_NONE ? k & 0xffffu : RMS_NONE;
    };
    auto pair = [](uint32_t a, uint32_t b) -> uint32_t { return a == RMS_NONE || b == RMS_NONE || a == b ? RMS_NONE : (min(a, b) << 16) | max(a, b); };
    const uint32_t a = rank_at(x, y);
    const uint32_t k_east = pair(a, rank_at(x + 1, y)), k_south = pair(a, rank_at(x, y + 1));
    if (__ballot(k_east != RMS_NONE || k_south != RMS_NONE) == 0ull) return;    // (uniform)
    // east: p = (x, y), q = (x + 1, y); south: q = (x, y + 1)
    for (int32_t dir = 0; dir < 2; dir++)
        wave_each_key(dir == 0 ? k_east : k_south, RMS_NONE, [&](uint32_t K, bool, uint64_t grp, bool leader) {
            if (!leader) return;
            const int32_t e = rooms_door_entry(keys, mask, K, ctl);
            if (e < 0) return;
            const int32_t n = __popcll(grp), dx = dir == 0 ? 1 : 0, dy = 1 - dx;
            const int64_t sx = (int64_t)n * xw + region_bit_sum(grp);           // the sum of the group's px
            RoomsDoorAcc *q = acc + e;
            atomicAdd(&q->count, n);
            atomicMin(&q->min_x, xw + __builtin_ctzll(grp));
            atomicMax(&q->max_x, xw + 63 - __builtin_clzll(grp) + dx);
            atomicMin(&q->min_y, y);
            atomicMax(&q->max_y, y + dy);
            atomicAdd(&q->sum_x2, (unsigned long long)(2 * sx + (int64_t)n * dx));
            atomicAdd(&q->sum_y2, (unsigned long long)((int64_t)n * (2 * y + dy)));
        });
}

// The entries leave in key order without a sort over the table: the key's upper half is the smaller room's rank a, so the doors of
// room a form one run of the output.  k_rooms_door_count: a lane per entry counts the runs' lengths (dcnt, scanned next, and dsize, kept).
__global__ void __launch_bounds__(RMS_NT)
k_rooms_door_count(const uint32_t *__restrict__ keys, int32_t cap, uint32_t *dcnt, uint32_t *dsize) {
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < cap; i += (int64_t)gridDim.x * RMS_NT) {
        const uint32_t key = keys[i];
        if (key == RMS_NONE) continue;
        atomicAdd(dcnt + (key >> 16), 1u);
        atomicAdd(dsize + (key >> 16), 1u);
    }
}

// a lane per entry takes a slot of its room's run, in whatever order the atomics fall: order [doors] holds the entries' indices
__global__ void __launch_bounds__(RMS_NT)
k_rooms_door_bucket(const uint32_t *__restrict__ keys, int32_t cap, const uint32_t *__restrict__ dcnt, const uint32_t *__restrict__ dblocks, uint32_t *dfill,
                    uint32_t *__restrict__ order) {
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < cap; i += (int64_t)gridDim.x * RMS_NT) {
        const uint32_t key = keys[i];
        if (key == RMS_NONE) continue;
        const uint32_t a = key >> 16;
        order[scan_prefix(dcnt, dblocks, a) + atomicAdd(dfill + a, 1u)] = (uint32_t)i;
    }
}

// a lane per entry: its place is its run's start plus the number of smaller keys within the run -- the work is the sum of the squared
// run lengths, not the square of the table
__global__ void __launch_bounds__(RMS_NT)
k_rooms_doors(const uint32_t *__restrict__ keys, const RoomsDoorAcc *__restrict__ acc, int32_t cap, const uint32_t *__restrict__ dcnt,
              const uint32_t *__restrict__ dblocks, const uint32_t *__restrict__ dsize, const uint32_t *__restrict__ order, const uint32_t *__restrict__ anchor,
              gms_room *rec, gms_door *__restrict__ out, int32_t out_cap) {
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < cap; i += (int64_t)gridDim.x * RMS_NT) {
        const uint32_t key = keys[i];
        if (key == RMS_NONE) continue;
        const uint32_t a = key >> 16, b = key & 0xffffu, first = scan_prefix(dcnt, dblocks, a), n = dsize[a];
        int32_t at = (int32_t)first;
        for (uint32_t j = 0; j < n; j++) at += keys[order[first + j]] < key ? 1 : 0;
        atomicAdd(&rec[a].doors, 1);
        atomicAdd(&rec[b].doors, 1);
        if (at >= out_cap) continue;
        const RoomsDoorAcc q = acc[i];
        out[at] = gms_door{anchor[a], anchor[b], q.count, q.min_x, q.min_y, q.max_x, q.max_y, 0, (int64_t)q.sum_x2, (int64_t)q.sum_y2};
    }
}

// the first min(n, cap) room records
__global__ void __launch_bounds__(RMS_NT)
k_rooms_emit(const gms_room *__restrict__ rec, int32_t n, gms_room *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * RMS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RMS_NT) out[i] = rec[i];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static inline size_t rooms_door_bytes(size_t cap) { return cap * (2 * sizeof(uint32_t) + sizeof(RoomsDoorAcc)); }
static inline size_t rooms_table_bytes(size_t cap) { return cap * (sizeof(gms_room) + 4 * sizeof(uint32_t)) + (cap / GMS_SCAN + 2) * sizeof(uint32_t); }

// GMS_ROOMS_STAGES in the environment (tools/rooms_probe.py): the call waits on the stream at the end of each of its five parts and
// keeps the host clock's microseconds for gms_map_rooms_stage_us; without it nothing is waited for or kept
struct RoomsStages {
    gms_map *m;
    bool on;
    double t0;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
    explicit RoomsStages(gms_map *mm) : m(mm), on(getenv("GMS_ROOMS_STAGES") != nullptr), t0(0.0) {
        for (double &u : m->rooms_stage_us) u = 0.0;
        if (on) { (void)hipStreamSynchronize(m->stream); t0 = now(); }
    }
    void end(int32_t stage) {
        if (!on) return;
        (void)hipStreamSynchronize(m->stream);
        const double t = now();
        m->rooms_stage_us[stage] += t - t0;
        t0 = t;
    }
};
static int rooms_door_grow(gms_map *m, int64_t cap) {
    if (cap > INT_MAX / 4) return gms_fail(GMS_ERR_NOMEM, "gms_rooms: a door table of %lld entries", (long long)cap);
    return gms_dev_grow(&m->d_rooms_doors, &m->rooms_door_cap, cap, RMS_DOOR_CAP0, nullptr, rooms_door_bytes, "gms_rooms", "the door table");
}

// what a request needs on the handle (a handle's W and H never change: only the two tables ever grow)
static int rooms_buffers(gms_map *m) {
    const size_t cells = (size_t)m->gd.cells, plane_bytes = (size_t)m->gd.H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), words = plane_bytes / sizeof(uint64_t);
    const size_t ntiles = (size_t)((m->gd.W + RMS_T - 1) / RMS_T) * (size_t)((m->gd.H + RMS_T - 1) / RMS_T);
    int rc = gms_dev_alloc(&m->d_rooms_field, cells * sizeof(uint32_t), "gms_rooms", "the working field");
    if (!rc) rc = gms_dev_alloc(&m->d_rooms_label, cells * sizeof(uint32_t), "gms_rooms", "the cores' label field");
    if (!rc) rc = gms_dev_alloc(&m->d_rooms_plane, 2 * plane_bytes, "gms_rooms", "the core plane and the kept roots' plane");
    if (!rc) rc = gms_dev_alloc(&m->d_rooms_wscan, (words + words / GMS_SCAN + 1) * sizeof(uint32_t), "gms_rooms", "the kept roots' scan");
    if (!rc) rc = gms_dev_alloc(&m->d_rooms_ctl, (RMS_CTL_WORDS + 2 * ntiles) * sizeof(uint32_t), "gms_rooms", "the tiles' flags");
    if (!rc) rc = gms_pinned_alloc(&m->h_rooms_ctl, RMS_CTL_WORDS * sizeof(uint32_t), "gms_rooms");
    if (!rc) rc = rooms_door_grow(m, RMS_DOOR_CAP0);
    return rc;
}

static int rooms_read_ctl(gms_map *m) { return relax_read_ctl(m->stream, m->d_rooms_ctl, m->h_rooms_ctl, RMS_CTL_WORDS); }

// Rooms and doors of ONE map's obstacle plane (already of logData as it stands) into the caller's device buffers; the handle's buffers
// exist.  Leaves the numbers of rooms and doors in *n_rooms and *n_doors.
static int rooms_run(gms_map *m, const uint32_t *d_obstacles, const gms_rooms *q, uint32_t *d_labels, uint16_t *d_depth, gms_room *d_rooms, int32_t cap_rooms,
                     gms_door *d_doors, int32_t cap_doors, int32_t *n_rooms, int32_t *n_doors) {
    const int32_t W = m->gd.W, H = m->gd.H, wpr64 = (W + 63) / 64, ntx = (W + RMS_T - 1) / RMS_T, nty = (H + RMS_T - 1) / RMS_T;
    if (nty > 65535) return gms_fail(GMS_ERR_INVALID, "gms_rooms: a map of %d rows exceeds one launch", H);
    hipStream_t st = m->stream;
    const int64_t words = (int64_t)H * wpr64, cells = m->gd.cells;
    uint64_t *core = reinterpret_cast<uint64_t *>(m->d_rooms_plane), *kept = core + words;
    uint32_t *wscan = m->d_rooms_wscan, *wblocks = wscan + words, *ctl = m->d_rooms_ctl, *label = m->d_rooms_label, *field = m->d_rooms_field;
    const int32_t ctl_words = RMS_CTL_WORDS + 2 * ntx * nty;
    RoomsStages stages(m);                                                      // parts 0 .. 4: planes, cores, rounds, records, doors
    // the core plane out of the handle's scratch plane, which the second inflation may then reuse
    const uint32_t *d_blocked = nullptr;
    int rc = gms_reach_inflate(m, d_obstacles, q->core, q->mode, &d_blocked);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rooms_core, dim3(gms_grid(cells, RMS_NT, 4096)), dim3(RMS_NT), 0, st, reinterpret_cast<const uint64_t *>(d_blocked), W, H, wpr64, core, field,
                       cells, ctl, ctl_words);
    HIPCHK(hipGetLastError());
    d_blocked = d_obstacles;
    if (q->inflate > 0 && (rc = gms_reach_inflate(m, d_obstacles, q->inflate, q->mode, &d_blocked)) != 0) return rc;
    const uint64_t *plane = reinterpret_cast<const uint64_t *>(d_blocked);
    stages.end(0);
    // the cores, their sizes, the rooms' ranks
    hipLaunchKernelGGL(k_rooms_tiles, dim3((unsigned)ntx, (unsigned)nty), dim3(RMS_NT), 0, st, core, wpr64, W, H, label);
    const int64_t border = (int64_t)(ntx - 1) * H + (int64_t)(nty - 1) * W;
    if (border > 0) hipLaunchKernelGGL(k_rooms_merge, dim3((unsigned)((border + RMS_NT - 1) / RMS_NT)), dim3(RMS_NT), 0, st, core, wpr64, W, H, ntx, nty, label);
    const unsigned word_waves = (unsigned)((words + RMS_NT / 64 - 1) / (RMS_NT / 64));
    hipLaunchKernelGGL(k_rooms_flatten, dim3(word_waves), dim3(RMS_NT), 0, st, core, wpr64, W, H, label, field);
    hipLaunchKernelGGL(k_rooms_keep, dim3(word_waves), dim3(RMS_NT), 0, st, core, wpr64, W, H, label, field, (uint32_t)q->min_core, kept, wscan);
    gms_launch_scan(st, wscan, nullptr, words, wblocks, ctl + 6);
    HIPCHK(hipGetLastError());
    if ((rc = rooms_read_ctl(m)) != 0) return rc;
    stages.end(1);
    const int64_t rooms = (int64_t)m->h_rooms_ctl[6];
    if (rooms > GMS_ROOMS_MAX)
        return gms_fail(GMS_ERR_INVALID, "gms_rooms: %lld rooms exceed GMS_ROOMS_MAX = %d (raise min_core or core)", (long long)rooms, GMS_ROOMS_MAX);
    rc = gms_dev_grow(&m->d_rooms_table, &m->rooms_cap, std::max<int64_t>(rooms, 1), 1024, nullptr, rooms_table_bytes, "gms_rooms", "the room table");
    if (rc) return rc;
    gms_room *rec = reinterpret_cast<gms_room *>(m->d_rooms_table);
    uint32_t *anchor = reinterpret_cast<uint32_t *>(m->d_rooms_table + (size_t)m->rooms_cap * sizeof(gms_room));
    uint32_t *dcnt = anchor + m->rooms_cap, *dsize = dcnt + m->rooms_cap, *dfill = dsize + m->rooms_cap, *dblocks = dfill + m->rooms_cap;
    uint32_t *dtotal = dblocks + m->rooms_cap / GMS_SCAN + 1;
    const int32_t R = (int32_t)rooms;
    if (R > 0) hipLaunchKernelGGL(k_rooms_table_init, dim3(gms_grid(R, RMS_NT, 1024)), dim3(RMS_NT), 0, st, rec, dcnt, dsize, dfill, R);
    hipLaunchKernelGGL(k_rooms_seed, dim3(word_waves), dim3(RMS_NT), 0, st, core, kept, wscan, wblocks, wpr64, W, H, label, field, ntx, nty, ctl, rec, anchor, R);
    HIPCHK(hipGetLastError());
    const uint32_t lim_axis = q->max_cost >= GMS_REACH_AXIS ? (uint32_t)(q->max_cost - GMS_REACH_AXIS + 1) << 16 : 0u;
    const uint32_t lim_diag = q->max_cost >= GMS_REACH_DIAG ? (uint32_t)(q->max_cost - GMS_REACH_DIAG + 1) << 16 : 0u;
    m->rooms_rounds = 0;
    m->rooms_tile_runs = 0;
    m->rooms_door_rebuilds = 0;
    const auto round = [&](int32_t k) {
        hipLaunchKernelGGL(k_rooms_round, dim3((unsigned)ntx, (unsigned)nty), dim3(RMS_T), 0, st, field, plane, wpr64, W, H, ctl, k, lim_axis, lim_diag);
    };
    if (R > 0 && (rc = relax_rounds(st, ctl, m->h_rooms_ctl, RMS_CTL_WORDS, q->max_cost, relax_batch("GMS_ROOMS_BATCH"), round, "gms_rooms", &m->rooms_rounds,
                                    &m->rooms_tile_runs)) != 0)
        return rc;
    stages.end(2);
    if (d_labels || d_depth) {
        const int64_t n = (int64_t)q->w * q->h;
        hipLaunchKernelGGL(k_rooms_out, dim3(gms_grid(n, RMS_NT, 4096)), dim3(RMS_NT), 0, st, field, anchor, W, q->x0, q->y0, q->w, q->h, d_labels, d_depth);
        HIPCHK(hipGetLastError());
    }
    *n_rooms = R;
    *n_doors = 0;
    if (R == 0) return GMS_OK;
    hipLaunchKernelGGL(k_rooms_records, dim3(word_waves), dim3(RMS_NT), 0, st, field, wpr64, W, H, rec);
    stages.end(3);
    // the doors: the table doubles until it is at most half full
    for (;;) {
        const int32_t cap = m->rooms_door_cap;
        uint32_t *keys = reinterpret_cast<uint32_t *>(m->d_rooms_doors);
        RoomsDoorAcc *acc = reinterpret_cast<RoomsDoorAcc *>(m->d_rooms_doors + (size_t)cap * sizeof(uint32_t));
        hipLaunchKernelGGL(k_rooms_doors_init, dim3(gms_grid(cap, RMS_NT, 1024)), dim3(RMS_NT), 0, st, keys, acc, cap, ctl);
        hipLaunchKernelGGL(k_rooms_contacts, dim3(word_waves), dim3(RMS_NT), 0, st, field, wpr64, W, H, keys, acc, (uint32_t)(cap - 1), ctl);
        HIPCHK(hipGetLastError());
        if ((rc = rooms_read_ctl(m)) != 0) return rc;
        if (m->h_rooms_ctl[8] == 0u) {
            *n_doors = (int32_t)m->h_rooms_ctl[7];
            uint32_t *order = reinterpret_cast<uint32_t *>(m->d_rooms_doors + (size_t)cap * (sizeof(uint32_t) + sizeof(RoomsDoorAcc)));
            const dim3 tgrid(gms_grid(cap, RMS_NT, 4096));
            hipLaunchKernelGGL(k_rooms_door_count, tgrid, dim3(RMS_NT), 0, st, keys, cap, dcnt, dsize);
            gms_launch_scan(st, dcnt, nullptr, R, dblocks, dtotal);
            hipLaunchKernelGGL(k_rooms_door_bucket, tgrid, dim3(RMS_NT), 0, st, keys, cap, dcnt, dblocks, dfill, order);
            hipLaunchKernelGGL(k_rooms_doors, tgrid, dim3(RMS_NT), 0, st, keys, acc, cap, dcnt, dblocks, dsize, order, anchor, rec, d_doors, d_doors ? cap_doors : 0);
            break;
        }
        m->rooms_door_rebuilds++;
        if ((rc = rooms_door_grow(m, 2 * (int64_t)cap)) != 0) return rc;        // (nothing is in flight on the table: the read-back has waited)
    }
    const int32_t stored = std::min(R, cap_rooms);
    if (d_rooms && stored > 0) hipLaunchKernelGGL(k_rooms_emit, dim3(gms_grid(stored, RMS_NT, 1024)), dim3(RMS_NT), 0, st, rec, stored, d_rooms);
    HIPCHK(hipGetLastError());
    stages.end(4);
    return GMS_OK;
}

// rooms and doors of one map of a shared handle or of the shown particle of a per-particle one; `shown` exists for a particle only
static int rooms(QuerySource src, const char *what, const gms_rooms *q, uint32_t *labels, uint16_t *depth, gms_room *records, int32_t cap_rooms, int32_t *n_rooms,
                 gms_door *doors, int32_t cap_doors, int32_t *n_doors, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !q) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle and the request are required)", what);
    gms_map *m = src.m;
    int64_t label_bytes = 0, depth_bytes = 0;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (!rc) rc = gms_rooms_size(q, nullptr, nullptr, &label_bytes, &depth_bytes);
    if (!rc) rc = gms_rect_check(q->x0, q->y0, q->w, q->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if ((int64_t)m->gd.W * m->gd.H >= (int64_t)RMS_NONE) return gms_fail(GMS_ERR_INVALID, "%s: a map of %d x %d cells exceeds a 32-bit label", what, m->gd.W, m->gd.H);
    const char *dev = on_device ? "_dev" : "";
    if (cap_rooms < 0 || (cap_rooms > 0 && !records) || cap_doors < 0 || (cap_doors > 0 && !doors))
        return gms_fail(GMS_ERR_INVALID, "%s%s: cap_rooms, cap_doors >= 0, and rooms / doors unless their cap is 0", what, dev);
    if (on_device && ((uintptr_t)labels & 3 || (uintptr_t)depth & 1 || (uintptr_t)records & 7 || (uintptr_t)doors & 7))
        return gms_fail(GMS_ERR_INVALID, "%s%s: the labels must be 4-byte aligned, the depth 2-byte aligned, the rooms and the doors 8-byte aligned", what, dev);
    src.filter = q->filter;
    if (src.s && (rc = query_check(src, what, "gms_rooms.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    rc = rooms_buffers(m);
    if (rc) return rc;
    if (!labels) label_bytes = 0;
    if (!depth) depth_bytes = 0;
    HostStage st(m, on_device);
    const size_t p_labels = st.part((size_t)label_bytes), p_depth = st.part((size_t)depth_bytes), p_rooms = st.part((size_t)cap_rooms * sizeof(gms_room)),
                 p_doors = st.part((size_t)cap_doors * sizeof(gms_door));
    rc = st.open();
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    int32_t nr = 0, nd = 0;
    rc = query_plane(src, q->mode, st.shown(shown), nullptr, &plane);
    if (!rc)
        rc = rooms_run(m, plane, q, labels ? st.at(p_labels, labels) : nullptr, depth ? st.at(p_depth, depth) : nullptr,
                       cap_rooms > 0 ? st.at(p_rooms, records) : nullptr, cap_rooms, cap_doors > 0 ? st.at(p_doors, doors) : nullptr, cap_doors, &nr, &nd);
    if (rc) return rc;
    if (n_rooms) *n_rooms = nr;
    if (n_doors) *n_doors = nd;
    st.fetch(labels, p_labels, (size_t)label_bytes);
    st.fetch(depth, p_depth, (size_t)depth_bytes);
    st.fetch(records, p_rooms, (size_t)std::min(nr, cap_rooms) * sizeof(gms_room));
    st.fetch(doors, p_doors, (size_t)std::min(nd, cap_doors) * sizeof(gms_door));
    return st.finish(shown);
}

extern "C" {

int gms_rooms_check(const gms_rooms *q) {
    REQUIRE(q, "gms_rooms: null request");
    REQUIRE(q->w >= 1 && q->h >= 1, "gms_rooms: w and h must be at least 1");
    REQUIRE(q->x0 >= 0 && q->y0 >= 0, "gms_rooms: x0 and y0 must not be negative");
    REQUIRE(q->inflate >= 0 && q->inflate <= 254, "gms_rooms: 0 <= inflate <= 254 cells");
    REQUIRE(q->core > q->inflate && q->core <= 255, "gms_rooms: inflate < core <= 255 cells");
    REQUIRE(q->mode == GMS_CLEAR_OCCUPIED || q->mode == GMS_CLEAR_NOT_FREE, "gms_rooms: mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE");
    REQUIRE(q->min_core >= 1, "gms_rooms: min_core must be at least 1");
    REQUIRE(q->max_cost >= 1 && q->max_cost <= 0xFFFE, "gms_rooms: 1 <= max_cost <= 0xFFFE");
    return GMS_OK;
}
int gms_rooms_size(const gms_rooms *q, int32_t *out_w, int32_t *out_h, int64_t *label_bytes, int64_t *depth_bytes) {
    const int rc = gms_rooms_check(q);
    if (rc) return rc;
    if (out_w) *out_w = q->w;
    if (out_h) *out_h = q->h;
    if (label_bytes) *label_bytes = (int64_t)q->w * q->h * (int64_t)sizeof(uint32_t);
    if (depth_bytes) *depth_bytes = (int64_t)q->w * q->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_rooms(gms_map *m, int32_t mi, const gms_rooms *q, uint32_t *labels, uint16_t *depth, gms_room *rooms_out, int32_t cap_rooms, int32_t *n_rooms,
                  gms_door *doors, int32_t cap_doors, int32_t *n_doors) {
    return rooms(query_map(m, mi), "gms_map_rooms", q, labels, depth, rooms_out, cap_rooms, n_rooms, doors, cap_doors, n_doors, nullptr, false);
}
int gms_map_rooms_dev(gms_map *m, int32_t mi, const gms_rooms *q, uint32_t *dev_labels, uint16_t *dev_depth, gms_room *dev_rooms, int32_t cap_rooms,
                      int32_t *n_rooms, gms_door *dev_doors, int32_t cap_doors, int32_t *n_doors) {
    return rooms(query_map(m, mi), "gms_map_rooms", q, dev_labels, dev_depth, dev_rooms, cap_rooms, n_rooms, dev_doors, cap_doors, n_doors, nullptr, true);
}
int gms_slam_rooms(gms_slam *s, int32_t which, const gms_rooms *q, uint32_t *labels, uint16_t *depth, gms_room *rooms_out, int32_t cap_rooms, int32_t *n_rooms,
                   gms_door *doors, int32_t cap_doors, int32_t *n_doors, int32_t *shown) {
    return rooms(query_slam(s, which), "gms_slam_rooms", q, labels, depth, rooms_out, cap_rooms, n_rooms, doors, cap_doors, n_doors, shown, false);
}
int gms_slam_rooms_dev(gms_slam *s, int32_t which, const gms_rooms *q, uint32_t *dev_labels, uint16_t *dev_depth, gms_room *dev_rooms, int32_t cap_rooms,
                       int32_t *n_rooms, gms_door *dev_doors, int32_t cap_doors, int32_t *n_doors, int32_t *dev_shown) {
    return rooms(query_slam(s, which), "gms_slam_rooms", q, dev_labels, dev_depth, dev_rooms, cap_rooms, n_rooms, dev_doors, cap_doors, n_doors, dev_shown, true);
}
int gms_map_rooms_stats(const gms_map *m, int32_t *rounds, int64_t *tile_runs, int32_t *door_rebuilds) {
    REQUIRE(m, "gms_map_rooms_stats: null handle");
    if (rounds) *rounds = m->rooms_rounds;
    if (tile_runs) *tile_runs = m->rooms_tile_runs;
    if (door_rebuilds) *door_rebuilds = m->rooms_door_rebuilds;
    return GMS_OK;
}
int gms_map_rooms_stage_us(const gms_map *m, double *us) {
    REQUIRE(m && us, "gms_map_rooms_stage_us: null argument");
    for (int32_t i = 0; i < GMS_ROOMS_STAGES; i++) us[i] = m->rooms_stage_us[i];
    return GMS_OK;
}

}  // extern "C"
