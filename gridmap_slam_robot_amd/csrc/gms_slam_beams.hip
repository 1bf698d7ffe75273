// gms_slam_beams.hip -- the beam sensor model of every particle of a gms_slam on ITS OWN map (gridmapslam.h "per-particle beam sensor
// model"): a Rao-Blackwellised particle is weighted by how well the scan agrees with the map it built itself.  The definition is
// gms_beams.hip's and the workgroup's body is the same one (gms_beams_device.h); this unit supplies where the occupancy bits come
// from.  A kernel unit: the C-ABI is gms_slam_host.hip's, as for gms_slam_align.hip.
//
//   k_slam_beam_score      one workgroup of 256 lanes per particle, grid (particles per filter, filters), with the per-particle
//                          prologue (gms_slam_device.h: slam_generation, slam_pose_draw -- the motion-model sample where the update
//                          asked for one and no launch in front drew it).  Then beam_score (gms_beams_device.h: the window, the
//                          walks, the partials, the tree -- k_beam_score's very body) over BeamLogSource: the window of `logData > 0`
//                          is packed straight from the particle's logData of the current generation into LDS, in PlaneWindow's word
//                          layout -- a wavefront reads 64 consecutive cells of a row, 512 bytes, coalesced, and its ballot is two
//                          words of the window -- so no packed plane of a particle's map is ever in memory; a bit outside the
//                          window, or every bit where there is none, is `logData[y W + x] > 0`.
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

#include "gms_beams_device.h"
#include "gms_slam_device.h"

#define SB_FLIGHT 4                     // rows of 64 cells a wavefront has in flight while it stages

// beam_score's source over one particle's logData [H][W]: occupied is `> 0` (0, -0.0 and NaN: not occupied)
struct BeamLogSource {
    const double *__restrict__ logd;
    int32_t W;
    __device__ __forceinline__ bool mem(int32_t x, int32_t y) const { return logd[(size_t)y * (size_t)W + (size_t)x] > 0.0; }
    // unit u is the pair of words 2 pr, 2 pr + 1 of row u / pairs -- 64 cells, one per lane
    __device__ __forceinline__ void fill(const PlaneWindow &win, uint32_t *s_win, int32_t tid) const {
        const int32_t lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int32_t pairs = (win.ww + 1) >> 1, units = pairs * win.wh;
        for (int32_t u0 = SB_FLIGHT * wave; u0 < units; u0 += SB_FLIGHT * (BEAM_NT / 64)) {
            bool occ[SB_FLIGHT];
#pragma unroll
            for (int k = 0; k < SB_FLIGHT; k++) {
                const int32_t u = u0 + k, row = u / pairs, pr = u - row * pairs;
                const int32_t x = ((win.wx0 + 2 * pr) << 5) + lane, y = win.wy0 + row;
                occ[k] = u < units && x < W && mem(x, y);
            }
#pragma unroll
            for (int k = 0; k < SB_FLIGHT; k++) {
                const int32_t u = u0 + k, row = u / pairs, pr = u - row * pairs;
                const uint64_t bits = __ballot(occ[k]);
                const int32_t w = 2 * pr + lane;
                if (lane < 2 && u < units && w < win.ww) s_win[row * win.ww + w] = (uint32_t)(bits >> (32 * lane));
            }
        }
    }
};

// grid (n_per, n_filters).  beams: the scan (BATCH: filter 0's, the filters bt.beam_stride apart, B the table's count); tab: factors
// [2][T] then their logarithms [2][T]; wgt / logw [n]; residuals [n][B] or NULL (never with BATCH); lds_words: the window the launch
// asked for (0: walk memory)
template <bool BATCH>
__global__ void __launch_bounds__(BEAM_NT)
k_slam_beam_score(GridDev g, const gms_beam *__restrict__ beams, int32_t B, SlamBufs sb, float *pose, float *cs, int32_t behind, int32_t ahead,
                  const double *__restrict__ tab, double *__restrict__ wgt, double *__restrict__ logw, uint16_t *__restrict__ residuals,
                  int32_t lds_words, MotionArgs mo, SlamBatch bt) {
    extern __shared__ __align__(16) uint32_t s_win[];
    __shared__ double s_p[BEAM_NT], s_s[BEAM_NT];
    __shared__ int32_t s_box[4];
    __shared__ float s_pose[5];                                                                 // x, y, theta, (float)cos, (float)sin
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t p = (int32_t)blockIdx.y * (int32_t)gridDim.x + (int32_t)blockIdx.x;
    const int32_t cur = slam_generation<BATCH>(sb, bt, p, beams, B, mo);
    if (tid < 64) slam_pose_draw<true>(mo, p, tid, pose, cs, s_pose);
    __syncthreads();
    const BeamLogSource src{sb_log(sb, cur) + (size_t)p * (size_t)g.cells, g.W};
    const BeamSums sums = beam_score(g, pose_xform(s_pose, s_pose + 3), beams, B, behind, ahead, tab,
                                     residuals, (size_t)p, lds_words, s_win, s_p, s_s, s_box, src);
    if (tid == 0) { wgt[p] = sums.p; logw[p] = sums.s; }
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
void gms_launch_slam_beams(gms_slam *s, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, const MotionModel *motion, int32_t behind, int32_t ahead,
                           int32_t which, double *d_wgt, double *d_logw, uint16_t *d_res, const SlamBatch *batch) {
    gms_pf *pf = s->pf;
    gms_map *m = s->map;
    const MotionArgs mo = motion_args(motion, pf->offset);
    const SlamBatch bt = slam_batch_of(pf, batch);
    const int64_t plane_words = (int64_t)m->gd.H * gms_plane_wpr(m);
    const int32_t lds_words = m->cast_walk_mem ? 0 : (int32_t)std::min<int64_t>(BEAM_LDS_CAP / 4, plane_words);
    const double *d_tab = s->beam.d_tab + (size_t)which * 4 * GMS_BEAM_T_MAX;
    auto launch = [&](auto batched) {
        gms_launch<k_slam_beam_score<batched()>>(m, dim3((unsigned)pf->n, (unsigned)pf->n_maps), dim3(BEAM_NT), (size_t)lds_words * 4, m->gd, d_beams, B, sb,
                                                 pf->d_pose, pf->d_cs, behind, ahead, d_tab, d_wgt, d_logw, d_res, lds_words, mo, bt);
    };
    if (batch) launch(gms_c<true>{}); else launch(gms_c<false>{});
}

void gms_launch_slam_weight_combine(gms_slam *s, int32_t B, const SlamBatch *batch) {
    gms_pf *pf = s->pf;
    const SlamBatch bt = slam_batch_of(pf, batch);
    hipLaunchKernelGGL(k_slam_weight_combine, dim3(gms_grid(s->n, 256, INT32_MAX)), dim3(256), 0, s->map->stream, pf->d_w, pf->d_logw, s->beam.d_wgt,
                       s->beam.d_wgt + s->n, s->n, B, s->beam.combine, bt);
    pf_scored(pf, 0);                                                                           // raw weights in d_w / d_logw, as the update leaves them
}
