// gms_regions.h -- the device helpers the feature units that label components and compact records share (gms_frontier.hip, gms_rooms.hip,
// gms_modes.hip; gms_scatter.hip for the scan's look-up; gms_nearest_device.h for the wavefront minima): the lock-free union, the ONE tile
// labelling and border merge of a bit plane (gms_frontier.hip: 8-connected, gms_rooms.hip: 4-connected), the "one turn per
// distinct key of the wavefront" loop, the integer wavefront reductions and the look-up into a scan made by gms_launch_scan (gms_query.hip).  The step kernels' unit
// (gms_fused_kernels.hip) does not include it, and gms_device.h stays what it was: no kernel of the other units is compiled differently.
#pragma once

#include "gms_device.h"

// ---- the lock-free union over a label field L, every label at most its own index (a root: L[a] == a) ----
// region_unite finds both roots, hangs the LARGER under the smaller with atomicMin, and if that root had moved in the meantime (the
// old value is not the root itself) goes on with what it moved to.  A label only ever decreases and never exceeds its own index, so
// chains end, nothing cycles, and nobody waits for anybody: a retry follows another lane's progress.  The final root of a component is
// its smallest member, however the unions are scheduled.
__device__ __forceinline__ uint32_t region_find(const uint32_t *L, uint32_t a) {
    for (;;) {
        const uint32_t p = __atomic_load_n(L + a, __ATOMIC_RELAXED);
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void region_unite(uint32_t *L, uint32_t a, uint32_t b) {
    for (;;) {
        a = region_find(L, a);
        b = region_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(L + a, b);                               // the larger root under the smaller
        if (old == a) return;
        a = old;                                                                // a had moved: unite what it moved to
    }
}

// ---- the labelling of a bit plane (rows of wpr64 64-bit words, the padding zero) in 64 x 64 tiles, with the links W and N (4-connected)
// or W, N, NW and NE (DIAGONAL: 8-connected); label [H][W] ----
#define REGION_T 64                      // tile edge in cells = cells of a plane word
#define REGION_NT 256                    // lanes of a workgroup of both bodies

// The body of a kernel launched (ntx, nty) x REGION_NT, a workgroup per tile; a tile whose 64 words are all zero leaves at once.  Every
// set cell starts as its own root in LDS and is united with its neighbours inside the tile; then every cell chases to its root and
// writes the root's GLOBAL linear index into the label field.  Tile-local order is the global order restricted to the tile, so that
// root is the tile's smallest member of the cell's component.  LDS: 64 words + 4096 uint32 labels = 16.5 KiB.  A lane owns 16 cells of
// a row and visits the set bits only.
template <bool DIAGONAL>
__device__ __forceinline__ void region_tile_label(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, uint32_t *__restrict__ label) {
    __shared__ uint64_t s_word[REGION_T];
    __shared__ uint32_t s_lab[REGION_T * REGION_T];
    const int32_t t = (int32_t)threadIdx.x, tx = (int32_t)blockIdx.x, x0 = tx * REGION_T, y0 = (int32_t)blockIdx.y * REGION_T;
    uint64_t w = 0ull;
    if (t < REGION_T) {
        w = y0 + t < H ? plane[(size_t)(y0 + t) * (size_t)wpr64 + (size_t)tx] : 0ull;
        s_word[t] = w;
    }
    if (!__syncthreads_or(w != 0ull)) return;
    const int32_t r = t >> 2, c0 = (t & 3) * 16;                                // this lane's 16 cells of row r
    const uint32_t mine = (uint32_t)(s_word[r] >> c0) & 0xffffu;
    for (uint32_t b = mine; b; b &= b - 1u) {
        const uint32_t c = (uint32_t)(r * REGION_T + c0 + __builtin_ctz(b));
        s_lab[c] = c;
    }
    __syncthreads();
    const uint64_t row = s_word[r], up = r > 0 ? s_word[r - 1] : 0ull;
    for (uint32_t b = mine; b; b &= b - 1u) {
        const int32_t lx = c0 + __builtin_ctz(b);
        const uint32_t c = (uint32_t)(r * REGION_T + lx);
        if (lx > 0 && ((row >> (lx - 1)) & 1ull)) region_unite(s_lab, c, c - 1u);
        if ((up >> lx) & 1ull) region_unite(s_lab, c, c - REGION_T);            // (N joins NW and NE through its own W link and NE's)
        else if constexpr (DIAGONAL) {
            if (lx > 0 && ((up >> (lx - 1)) & 1ull)) region_unite(s_lab, c, c - REGION_T - 1u);
            if (lx < REGION_T - 1 && ((up >> (lx + 1)) & 1ull)) region_unite(s_lab, c, c - REGION_T + 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = mine; b; b &= b - 1u) {
        const int32_t lx = c0 + __builtin_ctz(b);
        const uint32_t root = region_find(s_lab, (uint32_t)(r * REGION_T + lx));
        label[(size_t)(y0 + r) * (size_t)W + (size_t)(x0 + lx)] = (uint32_t)(y0 + (int32_t)(root >> 6)) * (uint32_t)W + (uint32_t)(x0 + (int32_t)(root & 63u));
    }
}

// The body of a kernel of REGION_NT lanes a workgroup: a lane per cell of column 64 k (k = 1 .. ntx - 1; the first (ntx - 1) * H lanes)
// and of row 64 k (k = 1 .. nty - 1; W lanes each), united in the global label field with the ONE cell across that border, or --
// DIAGONAL -- with its (up to) three neighbours across it: every pair adjacent across an edge or a corner, both diagonals.  (x, y >= 64
// on its axis, so the one cell straight across is on the map: only the diagonal ones need the bounds test)
template <bool DIAGONAL>
__device__ __forceinline__ void region_border_merge(const uint64_t *__restrict__ plane, int32_t wpr64, int32_t W, int32_t H, int32_t ntx, int32_t nty, uint32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * REGION_NT + threadIdx.x, nv = (int64_t)(ntx - 1) * H, nh = (int64_t)(nty - 1) * W;
    if (i >= nv + nh) return;
    auto bit = [&](int32_t x, int32_t y) -> bool {
        if constexpr (DIAGONAL) return x >= 0 && x < W && y >= 0 && y < H && ((plane[(size_t)y * (size_t)wpr64 + (size_t)(x >> 6)] >> (x & 63)) & 1ull) != 0ull;
        else return ((plane[(size_t)y * (size_t)wpr64 + (size_t)(x >> 6)] >> (x & 63)) & 1ull) != 0ull;
    };
    const bool column = i < nv;
    int32_t x, y;
    if (column) { x = ((int32_t)(i / H) + 1) * REGION_T; y = (int32_t)(i % H); }
    else { const int64_t j = i - nv; y = ((int32_t)(j / W) + 1) * REGION_T; x = (int32_t)(j % W); }
    if (!bit(x, y)) return;
    const uint32_t c = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    constexpr int32_t D = DIAGONAL ? 1 : 0;
    for (int32_t d = -D; d <= D; d++) {
        const int32_t ox = column ? x - 1 : x + d, oy = column ? y + d : y - 1;
        if (bit(ox, oy)) region_unite(label, c, (uint32_t)oy * (uint32_t)W + (uint32_t)ox);
    }
}

// the sum of the positions of mask's set bits
__device__ __forceinline__ uint32_t region_bit_sum(uint64_t mask) {
    return (uint32_t)__popcll(mask & 0xaaaaaaaaaaaaaaaaull) + 2u * (uint32_t)__popcll(mask & 0xccccccccccccccccull) +
           4u * (uint32_t)__popcll(mask & 0xf0f0f0f0f0f0f0f0ull) + 8u * (uint32_t)__popcll(mask & 0xff00ff00ff00ff00ull) +
           16u * (uint32_t)__popcll(mask & 0xffff0000ffff0000ull) + 32u * (uint32_t)__popcll(mask & 0xffffffff00000000ull);
}

// One turn per distinct key of the wavefront (uniform: every lane of the wavefront must call it): f(R, in, grp, leader) with the key
// R, whether this lane holds it, the ballot of the lanes that do and whether this lane is the one that acts for them -- so that the
// lanes that share a key combine first and ONE lane issues the atomics.  A lane whose key is `none` takes part in no group.
template <typename F>
__device__ __forceinline__ void wave_each_key(uint32_t key, uint32_t none, F f) {
    const int32_t lane = (int32_t)threadIdx.x & 63;
    uint64_t todo = __ballot(key != none);
    while (todo) {
        const int32_t leader = __builtin_ctzll(todo);
        const uint32_t R = (uint32_t)__shfl((int)key, leader);
        const bool in = key == R;
        const uint64_t grp = __ballot(in);
        f(R, in, grp, lane == leader);
        todo &= ~grp;
    }
}

// ---- integer reductions over the wavefront, the result in every lane ----
#define GMS_WAVE_REDUCE_(NAME, T, STEP)                      \
    __device__ __forceinline__ T NAME(T v) {                 \
        GMS_BUTTERFLY(STEP)                                  \
        return v;                                            \
    }
#define GMS_STEP_ADD_(O) v += wave_xor<O>(v);
#define GMS_STEP_MIN_(O) v = min(v, wave_xor<O>(v));
#define GMS_STEP_MAX_(O) v = max(v, wave_xor<O>(v));
#define GMS_STEP_MIN64_(O)                                                                                                 \
    {                                                                                                                      \
        const uint64_t o = ((uint64_t)wave_xor<O>((uint32_t)(v >> 32)) << 32) | (uint64_t)wave_xor<O>((uint32_t)v);        \
        v = o < v ? o : v;                                                                                                 \
    }
GMS_WAVE_REDUCE_(wave_add, int32_t, GMS_STEP_ADD_)
GMS_WAVE_REDUCE_(wave_min, int32_t, GMS_STEP_MIN_)
GMS_WAVE_REDUCE_(wave_max, int32_t, GMS_STEP_MAX_)
GMS_WAVE_REDUCE_(wave_min, uint32_t, GMS_STEP_MIN_)
GMS_WAVE_REDUCE_(wave_min, uint64_t, GMS_STEP_MIN64_)
#undef GMS_STEP_ADD_
#undef GMS_STEP_MIN_
#undef GMS_STEP_MAX_
#undef GMS_STEP_MIN64_
#undef GMS_WAVE_REDUCE_

// the exclusive prefix of item i of a scan made by gms_launch_scan: vals the items scanned within their blocks, blocks the blocks' offsets
// (I: the caller's index type, so that its arithmetic stays what it was)
template <typename I>
__device__ __forceinline__ uint32_t scan_prefix(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ blocks, I i) {
    return blocks[i / GMS_SCAN] + vals[i];
}
