// gms_beams.hip -- the beam sensor model (gridmapslam.h "beam sensor model"): every particle of a shared-map filter is weighted by where
// the map's first wall lies on each beam's walk, relative to the measured end point.
//
// A translation unit of its own, kernels and C-ABI, on the query base beside gms_cast.hip: no kernel of the other units is compiled
// differently for it.
//
//   k_beam_score   one workgroup of 256 lanes per (particle, map).  Lane l owns partial l: it walks the beams l, l + 256, ... of the scan
//                  one after another -- RayIterator's float recurrence (ray_init / ray_has_next / ray_step, gms_device.h) with `ahead`
//                  extra cells, through the map's GMS_CLEAR_OCCUPIED plane -- to the first set bit, takes the table index from the
//                  iterator's remaining count there, and multiplies / adds the two tables' entries into its partials.  In front of the
//                  walks the workgroup takes the box of its rays' start and end cells (+ ahead + 1, clipped to the map) and stages those
//                  rows' words of the plane in LDS when they fit what the launch asked for, as k_cast_map does; a cell outside the
//                  staged window is read from the plane in memory, so the window only ever decides WHERE a bit is read.  A window that
//                  does not fit, or GMS_CAST_WALK=mem: every bit from memory.  The 256 partials meet in a halving tree through LDS.
//
// LDS: min(64 KiB, the whole plane of one map) of window + 4 KiB of partials -- two workgroups per CU at the cap.  Every walk's loop
// carries the bound W + H + ahead + 2; the loop over a lane's beams ends at B <= max_beams.
#undef GMS_STAMPS
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_device.h"

#define BEAM_NT 256
#define BEAM_LDS_CAP (64 * 1024)         // the window: bytes of LDS a workgroup asks for at most
#define BEAM_T_MAX 512                   // behind + ahead + 2 at most
#define BEAM_TAB_BYTES (4 * BEAM_T_MAX * sizeof(double))

// a coordinate of a ray's end as a cell for the window's box: saturated, then held to one cell around the map
__device__ __forceinline__ int32_t beam_box_cell(float v, int32_t n) { return max(-1, min(n, j_d2i(floor((double)v)))); }

// the table index of one beam: top = behind + ahead + 1.  occ(x, y) is only ever asked for cells inside the map
template <class Occ>
__device__ __forceinline__ int32_t beam_walk(const GridDev &g, const RayIn &ray, int32_t ahead, int32_t top, Occ occ) {
    RayDev r;
    ray_init(r, ray.sx + 0.5f, ray.sy + 0.5f, ray.ex + 0.5f, ray.ey + 0.5f, ahead);
    const int32_t bound = g.W + g.H + ahead + 2;
    for (int32_t step = 0; step < bound && ray_has_next(r, g.W, g.H); step++) {
        if (occ(r.x, r.y)) return r.n > top ? 0 : top - r.n;                                   // (r.n >= 1 here: at most top - 1)
        ray_step(r);
    }
    return top;                                                                                 // none
}

__device__ __forceinline__ RayIn beam_ray(const GridDev &g, const XformDev &t, const gms_beam &m) {
    RayIn ray;
    ray.sx = (float)((xform_x(t, 0.0, 0.0) - g.posx) / g.res);                                  // GridMap.java:178
    ray.sy = (float)((xform_y(t, 0.0, 0.0) - g.posy) / g.res);                                  // :179
    ray.ex = (float)((xform_x(t, m.local_x, m.local_y) - g.posx) / g.res);                      // :185
    ray.ey = (float)((xform_y(t, m.local_x, m.local_y) - g.posy) / g.res);                      // :186
    ray.measured = 0.0f;
    ray.hit = m.hit != 0;
    return ray;
}

// grid (particles, maps).  plane: map 0's, the maps plane_stride words apart; beams: map 0's, the maps beam_stride apart; tab:
// factors [2][T] then their logarithms [2][T]; residuals: [n_maps][n][B] or NULL; lds_words: the window the launch asked for (0: walk memory)
__global__ void __launch_bounds__(BEAM_NT)
k_beam_score(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, int64_t plane_stride, const gms_beam *__restrict__ beams, int32_t B,
             int32_t beam_stride, const float *__restrict__ pose, const float *__restrict__ cs, int32_t n, int32_t behind, int32_t ahead,
             const double *__restrict__ tab, double *__restrict__ wgt, double *__restrict__ logw, uint16_t *__restrict__ residuals,
             int32_t lds_words) {
    extern __shared__ __align__(16) uint32_t s_win[];
    __shared__ double s_p[BEAM_NT], s_s[BEAM_NT];
    __shared__ int32_t s_box[4];
    const int32_t tid = (int32_t)threadIdx.x, mi = (int32_t)blockIdx.y;
    const size_t gi = (size_t)mi * (size_t)n + (size_t)blockIdx.x;
    plane += (size_t)mi * (size_t)plane_stride;
    beams += (size_t)mi * (size_t)beam_stride;
    const int32_t top = behind + ahead + 1, T = top + 1;
    XformDev t;
    t.px = (double)pose[3 * gi]; t.py = (double)pose[3 * gi + 1]; t.c = (double)cs[2 * gi]; t.s = (double)cs[2 * gi + 1];
    int32_t wx0 = 0, wy0 = 0, ww = 0, wh = 0;                                                   // the staged window: words x rows (0: none)
    if (lds_words > 0) {
        if (tid == 0) { s_box[0] = g.W; s_box[1] = g.H; s_box[2] = -1; s_box[3] = -1; }
        __syncthreads();
        int32_t lx = g.W, ly = g.H, hx = -1, hy = -1;
        for (int32_t b = tid; b < B; b += BEAM_NT) {
            const RayIn ray = beam_ray(g, t, beams[b]);
            const int32_t ax = beam_box_cell(ray.sx + 0.5f, g.W), ay = beam_box_cell(ray.sy + 0.5f, g.H);
            const int32_t bx = beam_box_cell(ray.ex + 0.5f, g.W), by = beam_box_cell(ray.ey + 0.5f, g.H);
            lx = min(lx, min(ax, bx)); ly = min(ly, min(ay, by));
            hx = max(hx, max(ax, bx)); hy = max(hy, max(ay, by));
        }
        if (tid < B) {
            atomicMin(&s_box[0], lx); atomicMin(&s_box[1], ly);
            atomicMax(&s_box[2], hx); atomicMax(&s_box[3], hy);
        }
        __syncthreads();
        const int32_t pad = ahead + 1;
        const int32_t x0 = max(0, s_box[0] - pad), y0 = max(0, s_box[1] - pad), x1 = min(g.W - 1, s_box[2] + pad), y1 = min(g.H - 1, s_box[3] + pad);
        if (x1 >= x0 && y1 >= y0) {
            wx0 = x0 >> 5; wy0 = y0;
            ww = (x1 >> 5) - wx0 + 1; wh = y1 - y0 + 1;
            if ((int64_t)ww * wh > (int64_t)lds_words) ww = wh = 0;                             // does not fit: this workgroup walks memory
        }
        const int32_t nw = ww * wh;
        for (int32_t i = tid; i < nw; i += BEAM_NT) {
            const int32_t row = i / ww, w = i - row * ww;
            s_win[i] = plane[(size_t)(wy0 + row) * (size_t)wpr + (size_t)(wx0 + w)];
        }
        __syncthreads();
    }
    double p = 1.0, s = 0.0;
    uint16_t *__restrict__ res = residuals ? residuals + gi * (size_t)B : nullptr;
    for (int32_t b = tid; b < B; b += BEAM_NT) {
        const RayIn ray = beam_ray(g, t, beams[b]);
        int32_t idx;
        if (ww > 0) {
            idx = beam_walk(g, ray, ahead, top, [&](int32_t x, int32_t y) {
                const uint32_t cw = (uint32_t)((x >> 5) - wx0), cr = (uint32_t)(y - wy0);
                const uint32_t word = (cw < (uint32_t)ww && cr < (uint32_t)wh) ? s_win[cr * (uint32_t)ww + cw] : plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)];
                return ((word >> (x & 31)) & 1u) != 0u;
            });
        } else {
            idx = beam_walk(g, ray, ahead, top, [&](int32_t x, int32_t y) { return ((plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)] >> (x & 31)) & 1u) != 0u; });
        }
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
    if (tid == 0) { wgt[gi] = s_p[0]; logw[gi] = s_s[0]; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int beam_model_check(int32_t behind, int32_t ahead, const double *factors, const char *who) {
    if (behind < 0 || behind > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= behind <= 255 steps", who);
    if (ahead < 0 || ahead > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= ahead <= 255 steps", who);
    if (!factors) return gms_fail(GMS_ERR_INVALID, "%s: null factors (two rows of behind + ahead + 2 doubles are required)", who);
    const int32_t T = behind + ahead + 2;
    for (int32_t i = 0; i < 2 * T; i++)
        if (!(factors[i] > 0.0) || !(factors[i] < INFINITY))
            return gms_fail(GMS_ERR_INVALID, "%s: factors[%d][%d] must be finite and > 0", who, i / T, i % T);
    return GMS_OK;
}

static int pf_score_beams(gms_pf *pf, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals,
                          bool on_device) {
    const char *who = on_device ? "gms_pf_score_beams_dev" : "gms_pf_score_beams";
    if (!pf || !beams) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the filter, the beams and the factors are required)", who);
    int rc = beam_model_check(behind, ahead, factors, who);
    if (rc) return rc;
    if (pf->slam_owned)
        return gms_fail(GMS_ERR_STATE, "%s: this filter's particles own maps (gms_slam): there is no one map to walk", who);
    gms_map *m = pf->map;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (on_device && ((uintptr_t)residuals & 1) != 0) return gms_fail(GMS_ERR_INVALID, "%s: the residuals must be 2-byte aligned", who);
    HIPCHK(hipSetDevice(m->device));
    // the tables: factors [2][T], then log() of each, through a pinned slot into the filter's device copy
    const int32_t T = behind + ahead + 2;
    auto &bm = pf->beam;
    if (!bm.ring_ready) {
        rc = gms_ring_alloc(bm.ring, BEAM_TAB_BYTES);
        if (rc) { gms_ring_free(bm.ring); return rc; }
        bm.ring_ready = 1;
    }
    rc = gms_dev_alloc(&bm.d_tab, BEAM_TAB_BYTES, who, "the factor tables");
    if (rc) return rc;
    void *slot = nullptr;
    rc = gms_ring_acquire(bm.ring, &slot);
    if (rc) return rc;
    double *h = static_cast<double *>(slot);
    for (int32_t i = 0; i < 2 * T; i++) { h[i] = factors[i]; h[2 * T + i] = log(factors[i]); }
    gms_launch_copy(m, bm.d_tab, h, (size_t)4 * T * sizeof(double));
    rc = gms_ring_commit(bm.ring, m->stream);
    if (rc) return rc;
    const gms_beam *d_beams = beams;
    int32_t beam_stride = B;
    if (!on_device) {
        rc = gms_stage_beams(m, beams, B);
        if (rc) return rc;
        d_beams = m->d_beams; beam_stride = m->max_beams;
    }
    HostStage st(m, on_device);
    const size_t res_bytes = residuals ? (size_t)pf->n_maps * (size_t)pf->n * (size_t)B * sizeof(uint16_t) : 0;
    const size_t p_res = st.part(res_bytes);
    if (res_bytes) {
        rc = st.open();
        if (rc) return rc;
    }
    const uint32_t *plane = nullptr;
    rc = query_plane(query_map(m, 0), GMS_CLEAR_OCCUPIED, nullptr, nullptr, &plane);            // (the deferred apply pass first)
    if (rc) return rc;
    const int32_t wpr = gms_plane_wpr(m);
    const int64_t plane_stride = (int64_t)m->gd.H * wpr;
    const int64_t lds_words = m->cast_walk_mem ? 0 : std::min<int64_t>(BEAM_LDS_CAP / 4, plane_stride);
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_beam_score), hipFuncAttributeMaxDynamicSharedMemorySize, BEAM_LDS_CAP));
        attr_set = true;
    }
    hipLaunchKernelGGL(k_beam_score, dim3((unsigned)pf->n, (unsigned)pf->n_maps), dim3(BEAM_NT), (size_t)lds_words * 4, m->stream, m->gd, plane, wpr,
                       plane_stride, d_beams, B, beam_stride, pf->d_pose, pf->d_cs, pf->n, behind, ahead, bm.d_tab, pf->d_w, pf->d_logw,
                       residuals ? st.at(p_res, residuals) : nullptr, (int32_t)lds_words);
    HIPCHK(hipGetLastError());
    pf_scored(pf, 0);                                                                           // the state a gms_pf_score leaves
    if (!res_bytes) return GMS_OK;
    st.fetch(residuals, p_res, res_bytes);
    return st.finish(nullptr);
}

extern "C" {

int gms_beam_model_check(int32_t behind, int32_t ahead, const double *factors) { return beam_model_check(behind, ahead, factors, "gms_beam_model"); }

int gms_pf_score_beams(gms_pf *pf, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals) {
    return pf_score_beams(pf, beams, B, behind, ahead, factors, residuals, false);
}
int gms_pf_score_beams_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, int32_t behind, int32_t ahead, const double *factors,
                           uint16_t *dev_residuals) {
    return pf_score_beams(pf, dev_beams, B, behind, ahead, factors, dev_residuals, true);
}

}  // extern "C"
