// gms_slam_beams.hip -- the beam sensor model of every particle of a gms_slam on ITS OWN map (gridmapslam.h "per-particle beam sensor
// model"): a Rao-Blackwellised particle is weighted by how well the scan agrees with the map it built itself.  The definition is
// gms_beams.hip's, the geometry gms_probe.h's; what is new is where the occupancy bits come from.  A kernel unit: the C-ABI is
// gms_slam_host.hip's, as for gms_slam_align.hip.
//
//   k_slam_beam_score      one workgroup of 256 lanes per particle, grid (particles per filter, filters).  Wavefront 0 draws the
//                          motion-model sample where the update asked for one and no launch in front drew it (the Philox counters of
//                          k_slam_particle / k_slam_refine / k_slam_align) and writes pose and trig.  The workgroup forms the box of
//                          its rays and clips it as k_beam_score does, then packs that window of `logData > 0` straight from the
//                          particle's logData of the current generation into LDS, in PlaneWindow's word layout: a wavefront reads 64
//                          consecutive cells of a row -- 512 bytes, coalesced -- and its ballot is two words of the window.  No
//                          packed plane of a particle's map is ever in memory.  Then lane l walks the beams l, l + 256, ... and the
//                          partials meet in the halving tree, exactly as in k_beam_score.  A window that does not fit what the launch
//                          asked for, or GMS_CAST_WALK=mem: every bit is `logData[y W + x] > 0` from memory; so is a cell outside
//                          the window (PlaneWindow::bit_else).  All three give the same bits.
//   k_slam_weight_combine  one lane per particle, behind k_slam_particle and in front of the normalisation: the raw weight and
//                          log-weight the update wrote, times / plus the beam model's (MULTIPLY) or replaced by them (REPLACE).
//
// LDS: min(64 KiB, the whole plane of one map) of window + 4 KiB of partials.  Bounds: the staging loop ends at the window's pairs of
// words (<= its words), a staged cell has x < W and wy0 <= y <= H - 1 (clip); every walk's loop carries W + H + ahead + 2 and asks for
// cells inside the map only (ray_first); the loop over a lane's beams ends at B <= max_beams.
#undef GMS_STAMPS
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_probe.h"
#include "gms_slam_device.h"

#define SB_NT 256
#define SB_LDS_CAP (64 * 1024)          // the window: bytes of LDS a workgroup asks for at most (BEAM_LDS_CAP)
#define SB_FLIGHT 4                     // rows of 64 cells a wavefront has in flight while it stages

// grid (n_per, n_filters).  beams: the scan (BATCH: filter 0's, the filters bt.beam_stride apart, B the table's count); tab: factors
// [2][T] then their logarithms [2][T]; wgt / logw [n]; residuals [n][B] or NULL (never with BATCH); lds_words: the window the launch
// asked for (0: walk memory)
template <bool BATCH>
__global__ void __launch_bounds__(SB_NT)
k_slam_beam_score(GridDev g, const gms_beam *__restrict__ beams, int32_t B, SlamBufs sb, float *pose, float *cs, int32_t behind, int32_t ahead,
                  const double *__restrict__ tab, double *__restrict__ wgt, double *__restrict__ logw, uint16_t *__restrict__ residuals,
                  int32_t lds_words, MotionArgs mo, SlamBatch bt) {
    extern __shared__ __align__(16) uint32_t s_win[];
    __shared__ double s_p[SB_NT], s_s[SB_NT];
    __shared__ int32_t s_box[4];
    __shared__ float s_pose[5];                                                                 // x, y, theta, (float)cos, (float)sin
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63;
    const int32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t p = (int32_t)blockIdx.y * (int32_t)gridDim.x + (int32_t)blockIdx.x;
    const int32_t *epoch = sb.epoch;
    if constexpr (BATCH) {
        int32_t integrate = 0;
        slam_batch_filter(bt, p, beams, B, mo, integrate, epoch);
    }
    const int32_t cur = epoch[0] & 1;                                                           // the current generation of the particles' maps (SlamBufs)
    const double *__restrict__ logd = sb_log(sb, cur) + (size_t)p * (size_t)g.cells;
    const int32_t top = behind + ahead + 1, T = top + 1;
    if (wave == 0) {                                   // sampleMotionModel (SLAM.java:90), as k_slam_particle draws it, or the pose and trig as they stand
        float x = pose[3 * (size_t)p], y = pose[3 * (size_t)p + 1], th = pose[3 * (size_t)p + 2], c = cs[2 * (size_t)p], sn = cs[2 * (size_t)p + 1];
        if (mo.on) {
            motion_apply(x, y, th, c, sn, (uint64_t)(mo.index0 + p), mo.d_center, mo.d_theta, mo.d_center_sd, mo.d_theta_sd, mo.seed, mo.sequence);
            if (lane == 0) {
                pose[3 * (size_t)p] = x; pose[3 * (size_t)p + 1] = y; pose[3 * (size_t)p + 2] = th;
                cs[2 * (size_t)p] = c; cs[2 * (size_t)p + 1] = sn;
            }
        }
        if (lane == 0) { s_pose[0] = x; s_pose[1] = y; s_pose[2] = th; s_pose[3] = c; s_pose[4] = sn; }
    }
    if (tid == SB_NT - 1) { s_box[0] = g.W; s_box[1] = g.H; s_box[2] = -1; s_box[3] = -1; }
    __syncthreads();
    const XformDev t = pose_xform(s_pose, s_pose + 3);
    PlaneWindow win;                                                                            // (none: walk memory)
    if (lds_words > 0) {
        int32_t box[4];
        PlaneWindow::box_none(box, g.W, g.H);
        for (int32_t b = tid; b < B; b += SB_NT) PlaneWindow::box_add(box, make_ray(g, t, beams[b]), g.W, g.H);
        if (tid < B) PlaneWindow::box_merge(s_box, box);
        __syncthreads();
        win = PlaneWindow::clip(s_box, ahead + 1, g.W, g.H, lds_words);
        // the window's words from logData: unit u is the pair of words 2 pr, 2 pr + 1 of row u / pairs -- 64 cells, one per lane
        const int32_t pairs = (win.ww + 1) >> 1, units = pairs * win.wh;
        for (int32_t u0 = SB_FLIGHT * wave; u0 < units; u0 += SB_FLIGHT * (SB_NT / 64)) {
            bool occ[SB_FLIGHT];
#pragma unroll
            for (int k = 0; k < SB_FLIGHT; k++) {
                const int32_t u = u0 + k, row = u / pairs, pr = u - row * pairs;
                const int32_t x = ((win.wx0 + 2 * pr) << 5) + lane, y = win.wy0 + row;
                occ[k] = u < units && x < g.W && logd[(size_t)y * (size_t)g.W + (size_t)x] > 0.0;   // (0, -0.0 and NaN: not occupied)
            }
#pragma unroll
            for (int k = 0; k < SB_FLIGHT; k++) {
                const int32_t u = u0 + k, row = u / pairs, pr = u - row * pairs;
                const uint64_t bits = __ballot(occ[k]);
                const int32_t w = 2 * pr + lane;
                if (lane < 2 && u < units && w < win.ww) s_win[row * win.ww + w] = (uint32_t)(bits >> (32 * lane));
            }
        }
        __syncthreads();
    }
    const auto mem = [&](int32_t x, int32_t y) { return logd[(size_t)y * (size_t)g.W + (size_t)x] > 0.0; };
    double pr = 1.0, s = 0.0;
    uint16_t *__restrict__ res = residuals ? residuals + (size_t)p * (size_t)B : nullptr;
    for (int32_t b = tid; b < B; b += SB_NT) {
        const RayIn ray = make_ray(g, t, beams[b]);
        int32_t idx;
        if (win.ww > 0) idx = beam_walk(g, ray, ahead, top, [&](int32_t x, int32_t y) { return win.bit_else(s_win, x, y, mem); });
        else idx = beam_walk(g, ray, ahead, top, mem);
        const int32_t at = (ray.hit ? T : 0) + idx;
        pr = pr * tab[at];
        s = s + tab[2 * T + at];
        if (res) res[b] = (uint16_t)idx;
    }
    s_p[tid] = pr; s_s[tid] = s;
    __syncthreads();
    for (int32_t h = SB_NT / 2; h >= 1; h >>= 1) {
        if (tid < h) { s_p[tid] = s_p[tid] * s_p[tid + h]; s_s[tid] = s_s[tid] + s_s[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { wgt[p] = s_p[0]; logw[p] = s_s[0]; }
}

// w / logw: the raw weights k_slam_particle wrote; bw / blogw: k_slam_beam_score's.  A filter whose scan is empty keeps what the update gave
__global__ void __launch_bounds__(256)
k_slam_weight_combine(double *__restrict__ w, double *__restrict__ logw, const double *__restrict__ bw, const double *__restrict__ blogw, int32_t n,
                      int32_t B, int32_t combine, SlamBatch bt) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (bt.tab) B = bt.tab[i / bt.n].count;
    if (B == 0) return;
    if (combine == GMS_SLAM_BEAMS_REPLACE) { w[i] = bw[i]; logw[i] = blogw[i]; }
    else { w[i] = w[i] * bw[i]; logw[i] = logw[i] + blogw[i]; }                                 // (one multiply, one add: nothing is contracted)
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int gms_slam_beam_table(gms_slam *s, const char *who, int32_t behind, int32_t ahead, const double *factors, int32_t which) {
    gms_map *m = s->map;
    auto &bm = s->beam;
    if (!bm.ring_ready) {
        const int rc = gms_ring_alloc(bm.ring, GMS_BEAM_TAB_BYTES);
        if (rc) { gms_ring_free(bm.ring); return rc; }
        bm.ring_ready = 1;
    }
    int rc = gms_dev_alloc(&bm.d_tab, 2 * GMS_BEAM_TAB_BYTES, who, "the factor tables");
    if (rc) return rc;
    void *slot = nullptr;
    rc = gms_ring_acquire(bm.ring, &slot);
    if (rc) return rc;
    const int32_t T = behind + ahead + 2;
    double *h = static_cast<double *>(slot);
    for (int32_t i = 0; i < 2 * T; i++) { h[i] = factors[i]; h[2 * T + i] = log(factors[i]); }
    gms_launch_copy(m, bm.d_tab + (size_t)which * 4 * GMS_BEAM_T_MAX, h, (size_t)4 * T * sizeof(double));
    return gms_ring_commit(bm.ring, m->stream);
}

void gms_launch_slam_beams(gms_slam *s, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, const MotionModel *motion, int32_t behind, int32_t ahead,
                           int32_t which, double *d_wgt, double *d_logw, uint16_t *d_res, const SlamBatch *batch) {
    gms_pf *pf = s->pf;
    gms_map *m = s->map;
    const MotionArgs mo = motion_args(motion, pf->offset);
    const SlamBatch bt = batch ? *batch : SlamBatch{nullptr, pf->n, 0};
    const int64_t plane_words = (int64_t)m->gd.H * gms_plane_wpr(m);
    const int32_t lds_words = m->cast_walk_mem ? 0 : (int32_t)std::min<int64_t>(SB_LDS_CAP / 4, plane_words);
    const double *d_tab = s->beam.d_tab + (size_t)which * 4 * GMS_BEAM_T_MAX;
    auto launch = [&](auto batched) {
        gms_launch<k_slam_beam_score<batched()>>(m, dim3((unsigned)pf->n, (unsigned)pf->n_maps), dim3(SB_NT), (size_t)lds_words * 4, m->gd, d_beams, B, sb,
                                                 pf->d_pose, pf->d_cs, behind, ahead, d_tab, d_wgt, d_logw, d_res, lds_words, mo, bt);
    };
    if (batch) launch(gms_c<true>{}); else launch(gms_c<false>{});
}

void gms_launch_slam_weight_combine(gms_slam *s, int32_t B, const SlamBatch *batch) {
    gms_pf *pf = s->pf;
    const SlamBatch bt = batch ? *batch : SlamBatch{nullptr, pf->n, 0};
    hipLaunchKernelGGL(k_slam_weight_combine, dim3(gms_grid(s->n, 256, INT32_MAX)), dim3(256), 0, s->map->stream, pf->d_w, pf->d_logw, s->beam.d_wgt,
                       s->beam.d_wgt + s->n, s->n, B, s->beam.combine, bt);
    pf_scored(pf, 0);                                                                           // raw weights in d_w / d_logw, as the update leaves them
}
