// gms_beams.hip -- the beam sensor model (gridmapslam.h "beam sensor model"): every particle of a shared-map filter is weighted by where
// the map's first wall lies on each beam's walk, relative to the measured end point.
//
// A translation unit of its own, kernels and C-ABI, on the query base beside gms_cast.hip: no kernel of the other units is compiled
// differently for it.
//
//   k_beam_score   one workgroup of 256 lanes per (particle, map): the pose's transform, beam_score (gms_beams_device.h: the window, the
//                  walks, the partials, the tree) over the map's GMS_CLEAR_OCCUPIED plane, the store.  The per-particle form is
//                  k_slam_beam_score (gms_slam_beams.hip): the same body over another source.
//
// LDS: min(64 KiB, the whole plane of one map) of window + 4 KiB of partials -- two workgroups per CU at the cap.  Every walk's loop
// carries the bound W + H + ahead + 2; the loop over a lane's beams ends at B <= max_beams.
#undef GMS_STAMPS
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_beams_device.h"

// beam_score's source over a packed plane in memory
struct BeamPlaneSource {
    const uint32_t *__restrict__ plane;
    int32_t wpr;
    __device__ __forceinline__ void fill(const PlaneWindow &win, uint32_t *s_win, int32_t tid) const { win.stage(s_win, plane, wpr, tid, BEAM_NT); }
    __device__ __forceinline__ bool mem(int32_t x, int32_t y) const { return plane_bit(plane, wpr, x, y); }
};

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
    const int32_t mi = (int32_t)blockIdx.y;
    const size_t gi = (size_t)mi * (size_t)n + (size_t)blockIdx.x;
    const BeamPlaneSource src{plane + (size_t)mi * (size_t)plane_stride, wpr};
    const BeamSums sums = beam_score(g, pose_xform(pose + 3 * gi, cs + 2 * gi), beams + (size_t)mi * (size_t)beam_stride, B, behind, ahead, tab,
                                     residuals, gi, lds_words, s_win, s_p, s_s, s_box, src);
    if (threadIdx.x == 0) { wgt[gi] = sums.p; logw[gi] = sums.s; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int gms_beam_model_check_for(int32_t behind, int32_t ahead, const double *factors, const char *who) {
    if (behind < 0 || behind > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= behind <= 255 steps", who);
    if (ahead < 0 || ahead > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= ahead <= 255 steps", who);
    if (!factors) return gms_fail(GMS_ERR_INVALID, "%s: null factors (two rows of behind + ahead + 2 doubles are required)", who);
    const int32_t T = behind + ahead + 2;
    for (int32_t i = 0; i < 2 * T; i++)
        if (!(factors[i] > 0.0) || !(factors[i] < INFINITY))
            return gms_fail(GMS_ERR_INVALID, "%s: factors[%d][%d] must be finite and > 0", who, i / T, i % T);
    return GMS_OK;
}

int gms_beam_table_put(gms_map *m, BeamTables &bt, const char *who, int32_t behind, int32_t ahead, const double *factors, int32_t which, int32_t n_tables) {
    if (!bt.ring_ready) {
        const int rc = gms_ring_alloc(bt.ring, GMS_BEAM_TAB_BYTES);
        if (rc) { gms_ring_free(bt.ring); return rc; }
        bt.ring_ready = 1;
    }
    int rc = gms_dev_alloc(&bt.d_tab, (size_t)n_tables * GMS_BEAM_TAB_BYTES, who, "the factor tables");
    if (rc) return rc;
    void *slot = nullptr;
    rc = gms_ring_acquire(bt.ring, &slot);
    if (rc) return rc;
    const int32_t T = behind + ahead + 2;
    double *h = static_cast<double *>(slot);
    for (int32_t i = 0; i < 2 * T; i++) { h[i] = factors[i]; h[2 * T + i] = log(factors[i]); }
    gms_launch_copy(m, bt.d_tab + (size_t)which * 4 * GMS_BEAM_T_MAX, h, (size_t)4 * T * sizeof(double));
    return gms_ring_commit(bt.ring, m->stream);
}
void gms_beam_table_free(BeamTables &bt) {
    hipFree(bt.d_tab); gms_ring_free(bt.ring);
    bt.d_tab = nullptr; bt.ring_ready = 0;
}

static int pf_score_beams(gms_pf *pf, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals,
                          bool on_device) {
    const char *who = on_device ? "gms_pf_score_beams_dev" : "gms_pf_score_beams";
    if (!pf || !beams) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the filter, the beams and the factors are required)", who);
    int rc = gms_beam_model_check_for(behind, ahead, factors, who);
    if (rc) return rc;
    if (pf->slam_owned)
        return gms_fail(GMS_ERR_STATE, "%s: this filter's particles own maps (gms_slam): there is no one map to walk", who);
    gms_map *m = pf->map;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (on_device && ((uintptr_t)residuals & 1) != 0) return gms_fail(GMS_ERR_INVALID, "%s: the residuals must be 2-byte aligned", who);
    HIPCHK(hipSetDevice(m->device));
    rc = gms_beam_table_put(m, pf->beam, who, behind, ahead, factors, 0, 1);
    if (rc) return rc;
    const gms_beam *d_beams;
    int32_t beam_stride;
    rc = gms_request_scan(m, beams, B, on_device, &d_beams, &beam_stride);
    if (rc) return rc;
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
    HIPCHK(gms_kernel_lds<k_beam_score>(m->device, BEAM_LDS_CAP));
    hipLaunchKernelGGL(k_beam_score, dim3((unsigned)pf->n, (unsigned)pf->n_maps), dim3(BEAM_NT), (size_t)lds_words * 4, m->stream, m->gd, plane, wpr,
                       plane_stride, d_beams, B, beam_stride, pf->d_pose, pf->d_cs, pf->n, behind, ahead, pf->beam.d_tab, pf->d_w, pf->d_logw,
                       residuals ? st.at(p_res, residuals) : nullptr, (int32_t)lds_words);
    HIPCHK(hipGetLastError());
    pf_scored(pf, 0);                                                                           // the state a gms_pf_score leaves
    if (!res_bytes) return GMS_OK;
    st.fetch(residuals, p_res, res_bytes);
    return st.finish(nullptr);
}

extern "C" {

int gms_beam_model_check(int32_t behind, int32_t ahead, const double *factors) { return gms_beam_model_check_for(behind, ahead, factors, "gms_beam_model"); }

int gms_pf_score_beams(gms_pf *pf, const gms_beam *beams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals) {
    return pf_score_beams(pf, beams, B, behind, ahead, factors, residuals, false);
}
int gms_pf_score_beams_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, int32_t behind, int32_t ahead, const double *factors,
                           uint16_t *dev_residuals) {
    return pf_score_beams(pf, dev_beams, B, behind, ahead, factors, dev_residuals, true);
}

}  // extern "C"
