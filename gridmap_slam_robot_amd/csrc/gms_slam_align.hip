// gms_slam_align.hip -- continuous scan alignment of every particle of a gms_slam against ITS OWN field (gridmapslam.h "per-particle scan
// alignment"): the build's stand-in for findBestPoseOptim(p.m, z, p.pose) inside SLAM.update (SLAM.java:96-97), and GMapping's
// per-particle scan matching step.  The definition is gms_align.hip's, the arithmetic gms_align_device.h's; what is new is where the
// field's values come from.
//
//   k_slam_align   one workgroup per particle, with the per-particle prologue (gms_slam_device.h: slam_generation, slam_pose_draw -- the
//                  motion-model sample where the update asked for one and no refinement launch ran in front); the workgroup stages
//                  the scan's (local_x, local_y) in LDS (align_stage_scan).
//     PLANES       the particle's class plane 0 (2 bits per cell: the classes of logData as it stands) is staged beside them.  Per
//                  evaluation, sixteen lanes per beam form the field's four values round the beam's end point on demand: lane r the
//                  horizontal sums of row j0 - k + r at the columns i0 and i0 + 1 (rows j0 - k .. j0 + 1 + k: at most sixteen), then
//                  lane q < 4 the vertical sum of cell (i0 + (q & 1), j0 + (q >> 1)) from its group's row sums -- computeLikelihoodMap's
//                  operations in its order for these cells, the literal taps or gms_map::taps_plain's exact image of them, as
//                  k_slam_particle's field_pass / field_pass_plain form one cell -- into LDS, 32 bytes per beam.  Then wavefront 0 runs
//                  align_eval on those values, lane l owning partial l, the halving tree, the solve and the step; the new pose and
//                  the end of the loop go back through LDS, so the loop is uniform per workgroup.
//     !PLANES      one wavefront per particle reads the four values from the particle's likelihoodData as k_align does; the caller
//                  has written the field of logData as it stands in front of the launch.
//
// Bounds: a used beam has 0 <= i0 <= W - 2 and 0 <= j0 <= H - 2 (align_cell, on the doubles), so its four cells are the map's; a row
// outside the map takes no part; a row's window of classes starts at cell y W + gx - k >= -k, i.e. at word -1 at the lowest, which is
// the last word of the values in front of the plane (its fields are masked), and ends inside the spare word behind the plane
// (slam_code_words).  Beams: b < B <= Bpad.  The loop over the iterations ends at iters + 1 <= 65 evaluations.
// LDS (PLANES): 48 bytes x Bpad + 4 x code_words (<= 24 KiB: gms_slam_create) + 144 bytes static.
#undef GMS_STAMPS
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gms_align_device.h"
#include "gms_slam_device.h"

#define SA_NT 256                       // PLANES: four wavefronts, sixteen beams per pass of the field's values
#define SA_MAXTAPS 15                  // the class planes are kept for blur kernels of up to 15 taps (gms_slam_create)

// the horizontal sum of row y at column gx (Util.java:391-401 over the columns inside the map), literal taps: field_pass's
__device__ __forceinline__ double sa_hsum(const GridDev &g, const uint32_t *s_plane, const double *s_taps, int32_t kh, int32_t ntaps, int32_t y, int32_t gx) {
    const int32_t jlo = max(-kh, -gx), jhi = min(kh, g.W - 1 - gx);
    const int32_t c0 = y * g.W + gx + jlo;
    const uint32_t w0 = s_plane[c0 >> 4], w1 = s_plane[(c0 >> 4) + 1];
    const uint64_t win = (((uint64_t)w1 << 32) | w0) >> (2 * (c0 & 15));
    double h = 0.0;
#pragma unroll
    for (int t = 0; t < SA_MAXTAPS; t++) {
        const int32_t j = jlo + t;
        const uint32_t e = (uint32_t)(win >> (2 * t)) & 3u;
        const double term = s_taps[min(j + kh, ntaps - 1)] * (e == 0u ? 0.5 : (e == 2u ? 1.0 : 0.0));   // GridMap.java:239-244; Util.java:399
        if (j <= jhi) h += term;
    }
    return h;
}
// ... where every tap is +0.0 or a normal number well inside the range (gms_map::taps_plain): field_pass_plain's
__device__ __forceinline__ double sa_hsum_plain(const GridDev &g, const uint32_t *s_plane, const double (&tp)[SA_MAXTAPS], int32_t kh, int32_t y, int32_t gx) {
    const int32_t c0 = y * g.W + gx - kh;                                      // (>= -kh: word -1 is readable, its fields are masked)
    const uint32_t w0 = s_plane[c0 >> 4], w1 = s_plane[(c0 >> 4) + 1];
    const uint32_t wv = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (2 * (c0 & 15)));
    const int32_t tlo = max(0, kh - gx), thi = min(2 * kh, g.W - 1 - gx + kh);   // columns inside the map (:396)
    const uint32_t inside = (uint32_t)((1ull << (2 * thi + 2)) - 1ull) & ~((1u << (2 * tlo)) - 1u);
    const uint32_t cw = (((~(wv | (wv >> 1))) & 0x55555555u) | (wv & 0xaaaaaaaau)) & inside;
    double h = 0.0;
#pragma unroll
    for (int t = 0; t < SA_MAXTAPS; t++) h += tp[t] * (double)((cw >> (2 * t)) & 3u);
    return h * 0.5;
}

// the four values of every used beam at the pose (x, y, theta) into s_val [B][4] = {L00, L10, L01, L11}; every lane of the workgroup
template <bool PLAIN>
__device__ __forceinline__ void sa_field_values(const GridDev &g, const uint32_t *s_plane, const double *s_taps, const double *__restrict__ taps_g,
                                                const double2 *s_beam, double *s_val, int32_t B, float x, float y, float theta) {
    const int32_t kh = g.khalf, ntaps = 2 * kh + 1;
    const int32_t lane = (int32_t)threadIdx.x & 63, r = lane & 15, grp = lane & ~15, q = r & 3, di = q & 1, dj = q >> 1;
    const XformDev t = align_xform(x, y, theta);
    double tp[SA_MAXTAPS];
#pragma unroll
    for (int i = 0; i < SA_MAXTAPS; i++) tp[i] = PLAIN && i < ntaps ? taps_g[i] : 0.0;
    for (int32_t base = 0; base < (B << 4); base += SA_NT) {                   // (every lane stays in the loop: the shuffles read all of a group)
        const int32_t b = (base + (int32_t)threadIdx.x) >> 4;
        AlignCell c;
        bool used = false;
        if (b < B) {
            const double2 l = s_beam[b];
            used = align_cell(g, t, l.x, l.y, c);
        }
        const int32_t i0 = used ? (int32_t)c.fu : 0, j0 = used ? (int32_t)c.fv : 0;
        const int32_t yr = j0 - kh + r;
        double h0 = 0.0, h1 = 0.0;
        if (used && r <= ntaps && yr >= 0 && yr < g.H) {                       // Util.java:418
            if (PLAIN) { h0 = sa_hsum_plain(g, s_plane, tp, kh, yr, i0); h1 = sa_hsum_plain(g, s_plane, tp, kh, yr, i0 + 1); }
            else { h0 = sa_hsum(g, s_plane, s_taps, kh, ntaps, yr, i0); h1 = sa_hsum(g, s_plane, s_taps, kh, ntaps, yr, i0 + 1); }
        }
        double total = 0.0;
#pragma unroll
        for (int rr = 0; rr < SA_MAXTAPS; rr++) {
            const double ha = __shfl(h0, grp + rr + dj), hb = __shfl(h1, grp + rr + dj);
            const double hh = di ? hb : ha;
            if (PLAIN) {
                total += tp[rr] * hh;                                          // :418-420 (a row outside the map, a tap past the last: + tap * 0.0)
            } else {
                const int32_t yy = j0 + dj - kh + rr;
                if (rr < ntaps && yy >= 0 && yy < g.H) total += s_taps[min(rr, ntaps - 1)] * hh;
            }
        }
        if (used && r < 4) s_val[4 * b + q] = total;
    }
}

struct AlignFetchLds {
    const double *val;
    __device__ __forceinline__ void operator()(int32_t b, int32_t, int32_t, double &l00, double &l10, double &l01, double &l11) const {
        const double2 a = reinterpret_cast<const double2 *>(val)[2 * b], c = reinterpret_cast<const double2 *>(val)[2 * b + 1];
        l00 = a.x; l10 = a.y; l01 = c.x; l11 = c.y;
    }
};

// grid: one workgroup per particle held (every filter's, BATCH).  pose / cs: the filter's, aligned in place; rec [n] or NULL
template <bool PLANES, bool BATCH>
__global__ void __launch_bounds__(PLANES ? SA_NT : GMS_WAVE)
k_slam_align(GridDev g, const gms_beam *__restrict__ beams, int32_t B, int32_t Bpad, SlamBufs sb, float *pose, float *cs,
             gms_align_record *__restrict__ rec, MotionArgs mo, int32_t code_words, const double *__restrict__ taps_g, int32_t taps_plain,
             gms_align_params prm, SlamBatch bt) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NT = PLANES ? SA_NT : GMS_WAVE;
    const int32_t p = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x, lane = tid & 63;
    const int32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t cur = slam_generation<BATCH>(sb, bt, p, beams, B, mo);
    double2 *s_beam = reinterpret_cast<double2 *>(smem);                       // [Bpad]
    double *s_val = reinterpret_cast<double *>(s_beam + Bpad);                 // [Bpad][4] (PLANES)
    uint32_t *s_plane = reinterpret_cast<uint32_t *>(s_val + 4 * (size_t)Bpad);   // [code_words] (PLANES)
    __shared__ float s_pose[3];
    __shared__ int32_t s_stop;
    __shared__ double s_taps[SA_MAXTAPS + 1];

    align_stage_scan(s_beam, beams, B, tid, NT);
    if (PLANES) {
        const uint32_t *__restrict__ gplane = sb_code(sb, cur) + (size_t)p * 2 * (size_t)code_words;     // plane 0: logData as it stands
        for (int32_t i = tid; i < code_words; i += NT) s_plane[i] = gplane[i];
        if (tid < SA_MAXTAPS + 1) s_taps[tid] = tid < g.ktaps ? taps_g[tid] : 0.0;
    }
    if (wave == 0) slam_pose_draw<false>(mo, p, lane, pose, cs, s_pose);
    __syncthreads();
    float x = s_pose[0], y = s_pose[1], theta = s_pose[2];
    const double *lik = PLANES ? nullptr : sb_lik(sb, cur) + (size_t)p * (size_t)g.cells;
    int32_t status = 0, done = 0, n0 = 0;
    double s0 = 0.0;
    AlignSums e;
    e.h00 = e.h01 = e.h02 = e.h11 = e.h12 = e.h22 = e.g0 = e.g1 = e.g2 = e.s = 0.0;
    e.n = 0;
    for (int32_t k = 0;; k++) {                        // (uniform per workgroup: the pose and the end of the loop come back through LDS)
        if (PLANES) {
            if (taps_plain) sa_field_values<true>(g, s_plane, s_taps, taps_g, s_beam, s_val, B, x, y, theta);
            else sa_field_values<false>(g, s_plane, s_taps, taps_g, s_beam, s_val, B, x, y, theta);
            __syncthreads();
        }
        if (wave == 0) {
            if (PLANES) e = align_eval(g, AlignFetchLds{s_val}, s_beam, B, x, y, theta, lane);
            else e = align_eval(g, AlignFetchMemory{lik, g.W}, s_beam, B, x, y, theta, lane);
            if (k == 0) { n0 = e.n; s0 = e.s; }
            const bool stop = align_advance(e, k, prm, g.res, x, y, theta, status, done);
            if (lane == 0) { s_pose[0] = x; s_pose[1] = y; s_pose[2] = theta; s_stop = stop ? 1 : 0; }
        }
        __syncthreads();
        x = s_pose[0]; y = s_pose[1]; theta = s_pose[2];
        if (s_stop) break;                             // (wavefront 0 writes both again only behind the next barrier, which every reader of this round has then passed)
    }
    if (tid != 0) return;
    align_store(pose, cs, rec, (size_t)p, x, y, theta, e, status, done, n0, s0);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static size_t slam_align_lds(int32_t Bpad, int64_t code_words) { return (size_t)Bpad * 48 + (size_t)code_words * 4; }

// whether an alignment of a scan of B beams computes its field's values itself from the class planes (no field is written in front of
// it): the planes are kept, and a plane fits a workgroup's LDS beside the beams and their values.  GMS_SLAM_ALIGN_FIELD=memory|planes
// (gms_slam::align_field) forces a form where it exists: tests of both
bool gms_slam_align_from_planes(const gms_slam *s, int32_t B) {
    if (!s->d_code[0] || s->align_field == 0) return false;
    const int32_t Bpad = B < 8 ? 8 : (B + 7) & ~7;
    return slam_align_lds(Bpad, s->code_words) + 4096 <= (size_t)s->map->lds_per_cu;
}

// The alignment of every particle the handle holds, in place, on the handle's stream.  from_planes: gms_slam_align_from_planes said so;
// else sb.lik's current generation holds every particle's field.  motion (may be NULL): the motion-model sample is drawn first.
// d_rec [n] or NULL; batch as for gms_launch_slam_particle
int gms_launch_slam_align(gms_slam *s, const gms_beam *d_beams, int32_t B, const SlamBufs &sb, bool from_planes, const MotionModel *motion,
                          const gms_align_params *prm, gms_align_record *d_rec, const SlamBatch *batch) {
    gms_pf *pf = s->pf;
    gms_map *m = s->map;
    const MotionArgs mo = motion_args(motion, pf->offset);
    const int32_t Bpad = B < 8 ? 8 : (B + 7) & ~7;
    const SlamBatch bt = slam_batch_of(pf, batch);
    const unsigned grid = (unsigned)pf->n * (unsigned)pf->n_maps;
    const size_t smem = from_planes ? slam_align_lds(Bpad, s->code_words) : (size_t)Bpad * 16;
    auto launch = [&](auto planes, auto batched) {
        gms_launch<k_slam_align<planes(), batched()>>(m, dim3(grid), dim3(planes() ? SA_NT : GMS_WAVE), smem, m->gd, d_beams, B, Bpad, sb, pf->d_pose,
                                                      pf->d_cs, d_rec, mo, (int32_t)s->code_words, m->d_taps, m->taps_plain, *prm, bt);
    };
    if (from_planes) { if (batch) launch(gms_c<true>{}, gms_c<true>{}); else launch(gms_c<true>{}, gms_c<false>{}); }
    else { if (batch) launch(gms_c<false>{}, gms_c<true>{}); else launch(gms_c<false>{}, gms_c<false>{}); }
    HIPCHK(hipGetLastError());
    s->align_form = from_planes ? GMS_SLAM_ALIGN_PLANES : GMS_SLAM_ALIGN_MEMORY;
    return GMS_OK;
}
