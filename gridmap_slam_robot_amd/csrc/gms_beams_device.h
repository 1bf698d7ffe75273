// gms_beams_device.h -- the beam sensor model's workgroup body (device only): ONE copy of the window, the walks, the partials and the
// tree for k_beam_score (gms_beams.hip: a packed plane of a shared map) and k_slam_beam_score (gms_slam_beams.hip: a particle's logData).
// The two kernels differ in their SOURCE of occupancy bits alone:
//   src.fill(win, s_win, tid)   the clipped window's words into LDS, PlaneWindow's layout (the body's barrier follows)
//   src.mem(x, y)               the bit of cell (x, y), inside the map, from memory
// With every particle's map equal to the shared map the two give the same bits (tests/test_gpu_beams_forms_agree.py).
#pragma once

#include "gms_probe.h"

#define BEAM_NT 256                      // lanes of a workgroup
#define BEAM_LDS_CAP (64 * 1024)         // the window: bytes of LDS a workgroup asks for at most

struct BeamSums { double p, s; };

// Lane l owns partial l: it walks the beams l, l + 256, ... in ascending order with `ahead` extra cells to the first set bit (beam_walk),
// takes the table index from the iterator's remaining count there, and multiplies / adds the entries of tab -- factors [2][T], then
// their logarithms [2][T], T = behind + ahead + 2 -- into its partials; residuals: the beams' indices go to its row `row` of B, or NULL.  In front of the walks the
// workgroup fills the window of its rays (every lane's box over its beams, padded by ahead + 1) when it fits lds_words; else, or
// lds_words = 0: every bit from memory.  The partials meet in a halving tree, tid with tid + h, through s_p / s_s [BEAM_NT]; s_box [4]:
// the workgroup's box.  Every lane calls this.
template <class Source>
__device__ __forceinline__ BeamSums beam_score(const GridDev &g, const XformDev &t, const gms_beam *__restrict__ beams, int32_t B, int32_t behind,
                                               int32_t ahead, const double *__restrict__ tab, uint16_t *__restrict__ residuals, size_t row, int32_t lds_words,
                                               uint32_t *s_win, double *s_p, double *s_s, int32_t (&s_box)[4], const Source &src) {
    const int32_t tid = (int32_t)threadIdx.x, top = behind + ahead + 1, T = top + 1;
    PlaneWindow win;                                                                            // (none: walk memory)
    if (lds_words > 0) {
        if (tid == 0) PlaneWindow::box_none(s_box, g.W, g.H);
        __syncthreads();
        int32_t box[4];
        PlaneWindow::box_none(box, g.W, g.H);
        for (int32_t b = tid; b < B; b += BEAM_NT) PlaneWindow::box_add(box, make_ray(g, t, beams[b]), g.W, g.H);
        if (tid < B) PlaneWindow::box_merge(s_box, box);
        __syncthreads();
        win = PlaneWindow::clip(s_box, ahead + 1, g.W, g.H, lds_words);
        src.fill(win, s_win, tid);
        __syncthreads();
    }
    const auto mem = [&](int32_t x, int32_t y) { return src.mem(x, y); };
    double p = 1.0, s = 0.0;
    uint16_t *__restrict__ res = residuals ? residuals + row * (size_t)B : nullptr;             // (here, not in the caller: a branch in front of the window keeps the kernel's argument loads apart)
    for (int32_t b = tid; b < B; b += BEAM_NT) {
        const RayIn ray = make_ray(g, t, beams[b]);
        int32_t idx;
        if (win.ww > 0) idx = beam_walk(g, ray, ahead, top, [&](int32_t x, int32_t y) { return win.bit(s_win, x, y, mem); });
        else idx = beam_walk(g, ray, ahead, top, mem);
        const int32_t at = (ray.hit ? T : 0) + idx;
        p = p * tab[at];
        s = s + tab[2 * T + at];
        if (res) res[b] = (uint16_t)idx;
    }
    s_p[tid] = p; s_s[tid] = s;
    __syncthreads();
    for (int32_t h = BEAM_NT / 2; h >= 1; h >>= 1) {
        if (tid < h) { s_p[tid] = s_p[tid] * s_p[tid + h]; s_s[tid] = s_s[tid] + s_s[tid + h]; }
        __syncthreads();
    }
    return {s_p[0], s_s[0]};
}
