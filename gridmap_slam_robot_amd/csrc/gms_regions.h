// gms_regions.h -- the device helpers the feature units that label components and compact records share (gms_frontier.hip, gms_modes.hip;
// gms_scatter.hip for the scan's look-up; gms_nearest_device.h for the wavefront minima): the lock-free union, the "one turn per
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
