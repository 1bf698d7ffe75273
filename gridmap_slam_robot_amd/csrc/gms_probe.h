// gms_probe.h -- the probe geometry the ray queries share (device only; DESIGN.md "the probe geometry the ray queries share"): the window
// of a bit plane a workgroup stages in LDS for its rays, and the walk to the first set bit; k_cast_map and the beam models' one body
// (gms_beams_device.h) use it.  The pose's transform and the ray's locals (pose_xform, make_ray) live in gms_device.h, where the scan
// step takes them from as well.
//
// Every expression keeps the reference's operand order and casts (gms_device.h; the build never contracts a multiply with an add).
#pragma once

#include "gms_device.h"

// a coordinate of a ray's end as a cell for the window's box: saturated, then held to one cell around the map
__device__ __forceinline__ int32_t box_cell(float v, int32_t n) { return max(-1, min(n, j_d2i(floor((double)v)))); }

// the bit of cell (x, y) of a plane in memory, the cell inside the map (base and pitch are kernel arguments, i.e. scalar registers: a
// lane's address is one multiply-add on top)
__device__ __forceinline__ bool plane_bit(const uint32_t *__restrict__ plane, int32_t wpr, int32_t x, int32_t y) {
    return ((plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)] >> (x & 31)) & 1u) != 0u;
}

// The window of a plane a workgroup keeps in LDS: ww words x wh rows from word wx0 of row wy0 (0 x 0: none, every bit from memory).
//   the box     a lane takes the box of its ray's start and end cells (box_of), or folds those of several rays into one (box_none, then
//               box_add in a loop), and merges it into the workgroup's int32_t[4] in LDS (box_merge; the caller sets that to box_none's
//               values and places the barriers)
//   clip        the box grown by `pad` cells -- the walk's extra steps + 1 -- and clipped to the map, in words; a window of more than
//               lds_words words does not fit: 0 x 0, this workgroup walks memory
//   stage       the window's words into LDS from a packed plane, the workgroup's nt lanes striding over them (the caller's barrier
//               follows); a plane that exists nowhere but in the window is packed there by its owner (gms_slam_beams.hip)
//   bit         THE rule: a cell inside the window is read from LDS, any other is answered by mem(x, y) -- plane_bit, or whatever the
//               window was filled from.  The box is an estimate of the float walk, never a promise, so the window only ever decides
//               WHERE a bit is read, never what is returned.
struct PlaneWindow {
    int32_t wx0 = 0, wy0 = 0, ww = 0, wh = 0;

    static __device__ __forceinline__ void box_none(int32_t (&b)[4], int32_t W, int32_t H) { b[0] = W; b[1] = H; b[2] = -1; b[3] = -1; }
    static __device__ __forceinline__ void box_of(int32_t (&b)[4], const RayIn &ray, int32_t W, int32_t H) {
        const int32_t ax = box_cell(ray.sx + 0.5f, W), ay = box_cell(ray.sy + 0.5f, H);
        const int32_t bx = box_cell(ray.ex + 0.5f, W), by = box_cell(ray.ey + 0.5f, H);
        b[0] = min(ax, bx); b[1] = min(ay, by); b[2] = max(ax, bx); b[3] = max(ay, by);
    }
    static __device__ __forceinline__ void box_add(int32_t (&b)[4], const RayIn &ray, int32_t W, int32_t H) {
        int32_t r[4];
        box_of(r, ray, W, H);
        b[0] = min(b[0], r[0]); b[1] = min(b[1], r[1]); b[2] = max(b[2], r[2]); b[3] = max(b[3], r[3]);
    }
    static __device__ __forceinline__ void box_merge(int32_t *s_box, const int32_t (&b)[4]) {
        atomicMin(&s_box[0], b[0]); atomicMin(&s_box[1], b[1]);
        atomicMax(&s_box[2], b[2]); atomicMax(&s_box[3], b[3]);
    }
    static __device__ __forceinline__ PlaneWindow clip(const int32_t *box, int32_t pad, int32_t W, int32_t H, int32_t lds_words) {
        PlaneWindow w;
        const int32_t x0 = max(0, box[0] - pad), y0 = max(0, box[1] - pad), x1 = min(W - 1, box[2] + pad), y1 = min(H - 1, box[3] + pad);
        if (x1 >= x0 && y1 >= y0) {
            w.wx0 = x0 >> 5; w.wy0 = y0;
            w.ww = (x1 >> 5) - w.wx0 + 1; w.wh = y1 - y0 + 1;
            if ((int64_t)w.ww * w.wh > (int64_t)lds_words) w.ww = w.wh = 0;
        }
        return w;
    }
    __device__ __forceinline__ void stage(uint32_t *dst, const uint32_t *__restrict__ plane, int32_t wpr, int32_t tid, int32_t nt) const {
        const int32_t n = ww * wh;
        for (int32_t i = tid; i < n; i += nt) {
            const int32_t row = i / ww, w = i - row * ww;
            dst[i] = plane[(size_t)(wy0 + row) * (size_t)wpr + (size_t)(wx0 + w)];
        }
    }
    template <class Mem>
    __device__ __forceinline__ bool bit(const uint32_t *s_win, int32_t x, int32_t y, Mem mem) const {
        const uint32_t cw = (uint32_t)((x >> 5) - wx0), cr = (uint32_t)(y - wy0);
        if (cw < (uint32_t)ww && cr < (uint32_t)wh) return ((s_win[cr * (uint32_t)ww + cw] >> (x & 31)) & 1u) != 0u;
        return mem(x, y);
    }
};

// integrateObservation's walk (GridMap.java:210-211) with `extra` steps past the end, to the FIRST cell for which occ(x, y) holds; occ is
// only ever asked for cells inside the map.  The result is found(step, r) there -- r stands on that cell, reached after `step` steps --
// or `none` where the walk ends without one.  The loop carries the bound W + H + extra + 2.  (found is called inside the loop: with the
// record built behind it the compiler splits the loop's condition into three branches, and the casts walk a fifth slower.)
template <class Occ, class Found, class T>
__device__ __forceinline__ T ray_first(const GridDev &g, const RayIn &ray, int32_t extra, Occ occ, Found found, T none) {
    RayDev r;
    ray_init(r, ray.sx + 0.5f, ray.sy + 0.5f, ray.ex + 0.5f, ray.ey + 0.5f, extra);            // :210
    const int32_t bound = g.W + g.H + extra + 2;
    for (int32_t step = 0; step < bound && ray_has_next(r, g.W, g.H); step++) {                 // :211
        if (occ(r.x, r.y)) return found(step, r);
        ray_step(r);
    }
    return none;
}

// the beam sensor model's table index of one beam from the iterator's remaining count at the first wall: top = behind + ahead + 1
template <class Occ>
__device__ __forceinline__ int32_t beam_walk(const GridDev &g, const RayIn &ray, int32_t ahead, int32_t top, Occ occ) {
    return ray_first(g, ray, ahead, occ, [&](int32_t, const RayDev &r) { return r.n > top ? 0 : top - r.n; }, top);   // (r.n >= 1 there: at most top - 1; top: none)
}
