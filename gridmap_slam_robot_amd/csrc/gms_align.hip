// gms_align.hip -- continuous scan alignment (gridmapslam.h "continuous scan alignment"): a damped Gauss-Newton scan matcher on the
// bilinearly interpolated likelihood field, for a list of poses on a map (gms_map_align) and for the particles of a shared-map filter
// in place (gms_pf_align).
//
// A translation unit of its own, kernel and C-ABI, on the query base beside gms_beams.hip: no kernel of the other units is compiled
// differently for it.
//
//   k_align        one wavefront per pose, four poses per workgroup of 256 lanes, grid (ceil(P / 4), maps).  The workgroup stages the
//                  scan's (local_x, local_y) in LDS once, 16 bytes per beam (align_stage_scan).  Lane l owns partial l: it walks the
//                  beams l, l + 64, ... in ascending order, two adjacent field values per row (16 bytes, 8-byte aligned) and two rows
//                  per look-up, and adds the ten terms into its registers (gms_align_device.h, shared with k_slam_align: staging,
//                  evaluation, step and store).  The halving tree p[l] += p[l + s], s = 32 .. 1, runs as cross-lane register moves
//                  (wave_xor: for l < s lane l ^ s IS lane l + s) with the add kept to the lanes l < s; lane 0's sums are broadcast and
//                  every lane solves the 3 x 3 system alike, so the loop over the iterations is uniform per wavefront.  A stopped
//                  pose leaves the loop; its wavefront idles until the workgroup's other three are done.
//
// Bounds: i0 <= W - 2 and j0 <= H - 2 are tested on the doubles before anything is cast, so the four reads stay inside the map's W x H
// doubles; the loop over a lane's beams ends at B <= max_beams, the loop over the iterations at iters + 1 <= 65 evaluations.
// LDS: 16 bytes x B, 64 KiB at GMS_MAX_BEAMS; no static LDS beside it (the dynamic base stays 16-byte aligned).
#undef GMS_STAMPS
#include <math.h>
#include <string.h>

#include "gms_align_device.h"

#define ALIGN_NT 256
#define ALIGN_WAVES (ALIGN_NT / GMS_WAVE)

// grid (ceil(P / 4), maps).  lik: map blockIdx.y's field at lik + y * lik_stride; beams likewise beam_stride apart; pose_in / pose_out
// [maps][P][3] (may be the same), cs [maps][P][2] or NULL: the final poses' float-rounded trig; rec [maps][P] or NULL
__global__ void __launch_bounds__(ALIGN_NT)
k_align(GridDev g, const double *__restrict__ lik, int64_t lik_stride, const gms_beam *__restrict__ beams, int32_t B, int32_t beam_stride,
        const float *pose_in, float *pose_out, float *__restrict__ cs, gms_align_record *__restrict__ rec, int32_t P, gms_align_params prm) {
    extern __shared__ __align__(16) double2 s_beam[];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, mi = (int32_t)blockIdx.y;
    lik += (size_t)mi * (size_t)lik_stride;
    beams += (size_t)mi * (size_t)beam_stride;
    align_stage_scan(s_beam, beams, B, tid, ALIGN_NT);
    __syncthreads();
    const int32_t p = (int32_t)blockIdx.x * ALIGN_WAVES + (tid >> 6);
    if (p >= P) return;                                                         // (uniform per wavefront; no barrier follows)
    const size_t gi = (size_t)mi * (size_t)P + (size_t)p;
    float x = pose_in[3 * gi], y = pose_in[3 * gi + 1], theta = pose_in[3 * gi + 2];
    int32_t status = 0, done = 0, n0 = 0;
    double s0 = 0.0;
    AlignSums e;
    const AlignFetchMemory fetch{lik, g.W};
    for (int32_t k = 0;; k++) {
        e = align_eval(g, fetch, s_beam, B, x, y, theta, lane);
        if (k == 0) { n0 = e.n; s0 = e.s; }
        if (align_advance(e, k, prm, g.res, x, y, theta, status, done)) break;
    }
    if (lane != 0) return;
    align_store(pose_out, cs, rec, gi, x, y, theta, e, status, done, n0, s0);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int gms_align_check_for(const gms_align_params *p, const char *who) {
    if (!p) return gms_fail(GMS_ERR_INVALID, "%s: null parameters", who);
    if (p->iters < 1 || p->iters > 64) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= iters <= 64", who);
    if (!(p->damp_t >= 0.0) || !(p->damp_t < INFINITY)) return gms_fail(GMS_ERR_INVALID, "%s: damp_t must be finite and >= 0", who);
    if (!(p->damp_r >= 0.0) || !(p->damp_r < INFINITY)) return gms_fail(GMS_ERR_INVALID, "%s: damp_r must be finite and >= 0", who);
    if (!(p->max_t > 0.0)) return gms_fail(GMS_ERR_INVALID, "%s: max_t must be > 0 (+Inf: no clamp)", who);
    if (!(p->max_r > 0.0)) return gms_fail(GMS_ERR_INVALID, "%s: max_r must be > 0 (+Inf: no clamp)", who);
    if (!(p->eps_t >= 0.0) || !(p->eps_t < INFINITY)) return gms_fail(GMS_ERR_INVALID, "%s: eps_t must be finite and >= 0", who);
    if (!(p->eps_r >= 0.0) || !(p->eps_r < INFINITY)) return gms_fail(GMS_ERR_INVALID, "%s: eps_r must be finite and >= 0", who);
    if (!(p->det_min >= 0.0) || !(p->det_min < INFINITY)) return gms_fail(GMS_ERR_INVALID, "%s: det_min must be finite and >= 0", who);
    return GMS_OK;
}

// lik: map 0's field of the launch, the maps lik_stride apart; poses and records [maps][P]
static int align_launch(gms_map *m, const double *lik, int64_t lik_stride, int32_t maps, const gms_beam *d_beams, int32_t B, int32_t beam_stride,
                        const float *d_in, float *d_out, float *d_cs, gms_align_record *d_rec, int32_t P, const gms_align_params *prm) {
    HIPCHK(gms_kernel_lds<k_align>(m->device, GMS_MAX_BEAMS * 16));
    hipLaunchKernelGGL(k_align, dim3((unsigned)((P + ALIGN_WAVES - 1) / ALIGN_WAVES), (unsigned)maps), dim3(ALIGN_NT), (size_t)B * 16, m->stream, m->gd, lik,
                       lik_stride, d_beams, B, beam_stride, d_in, d_out, d_cs, d_rec, P, *prm);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

static int map_align(gms_map *m, int32_t mi, const gms_beam *beams, int32_t B, const float *poses_in, int32_t P, const gms_align_params *prm,
                     float *poses_out, gms_align_record *records, bool on_device) {
    const char *who = on_device ? "gms_map_align_dev" : "gms_map_align";
    if (!m || !beams || !poses_in || !poses_out)
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the beams and both pose arrays are required)", who);
    int rc = gms_align_check_for(prm, who);
    if (rc) return rc;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (P < 1 || P > GMS_MAX_PARTICLES) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= P <= GMS_MAX_PARTICLES poses", who);
    if (on_device && (((uintptr_t)poses_in & 3) != 0 || ((uintptr_t)poses_out & 3) != 0 || ((uintptr_t)records & 7) != 0 || ((uintptr_t)beams & 7) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the poses must be 4-byte aligned, the records and the beams 8-byte aligned", who);
    QuerySource src = query_map(m, mi);
    rc = query_check(src, who, "");
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t beam_bytes = (size_t)B * sizeof(gms_beam), pose_bytes = (size_t)P * 3 * sizeof(float);
    const size_t rec_bytes = records ? (size_t)P * sizeof(gms_align_record) : 0;
    const size_t p_beams = st.part(beam_bytes), p_pose = st.part(pose_bytes), p_rec = st.part(rec_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_beams, beams, beam_bytes);
    if (!rc) rc = st.up(p_pose, poses_in, pose_bytes);                          // (the host form aligns its staged copy in place)
    if (rc) return rc;
    gms_ensure_lik(m);                                                          // likelihoodData as a download would see it
    float *d_out = st.at(p_pose, poses_out);
    rc = align_launch(m, m->d_lik + (size_t)mi * (size_t)m->gd.cells, 0, 1, st.at(p_beams, beams), B, B, on_device ? poses_in : d_out, d_out, nullptr,
                      records ? st.at(p_rec, records) : nullptr, P, prm);
    if (rc) return rc;
    st.fetch(poses_out, p_pose, pose_bytes);
    st.fetch(records, p_rec, rec_bytes);
    return st.finish(nullptr);
}

static int pf_align(gms_pf *pf, const gms_beam *beams, int32_t B, const gms_align_params *prm, gms_align_record *records, bool on_device) {
    const char *who = on_device ? "gms_pf_align_dev" : "gms_pf_align";
    if (!pf || !beams) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the filter and the beams are required)", who);
    int rc = gms_align_check_for(prm, who);
    if (rc) return rc;
    if (pf->slam_owned)
        return gms_fail(GMS_ERR_STATE, "%s: this filter's particles own maps (gms_slam): there is no one field to align on", who);
    gms_map *m = pf->map;
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams beams", who);
    if (on_device && (((uintptr_t)records & 7) != 0 || ((uintptr_t)beams & 7) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the records and the beams must be 8-byte aligned", who);
    HIPCHK(hipSetDevice(m->device));
    const gms_beam *d_beams;
    int32_t beam_stride;
    rc = gms_request_scan(m, beams, B, on_device, &d_beams, &beam_stride);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t rec_bytes = records ? (size_t)pf->n_maps * (size_t)pf->n * sizeof(gms_align_record) : 0;
    const size_t p_rec = st.part(rec_bytes);
    if (rec_bytes) {
        rc = st.open();
        if (rc) return rc;
    }
    gms_ensure_lik(m);
    rc = align_launch(m, m->d_lik, m->gd.cells, pf->n_maps, d_beams, B, beam_stride, pf->d_pose, pf->d_pose, pf->d_cs,
                      records ? st.at(p_rec, records) : nullptr, pf->n, prm);
    if (rc) return rc;
    pf_particles_changed(pf);                                                   // the state a gms_pf_set_poses leaves
    if (!rec_bytes) return GMS_OK;
    st.fetch(records, p_rec, rec_bytes);
    return st.finish(nullptr);
}

extern "C" {

int gms_align_params_default(gms_align_params *p) {
    REQUIRE(p, "gms_align_params_default: null argument");
    memset(p, 0, sizeof(*p));
    p->iters = 8;
    p->damp_t = 10.0; p->damp_r = 1e4;
    p->max_t = 2.0; p->max_r = 0.1;
    p->eps_t = 0.01; p->eps_r = 1e-4;
    p->det_min = 1e-6;
    return GMS_OK;
}

int gms_align_check(const gms_align_params *p) { return gms_align_check_for(p, "gms_align_params"); }

int gms_map_align(gms_map *m, int32_t mi, const gms_beam *beams, int32_t B, const float *poses_in, int32_t P, const gms_align_params *params,
                  float *poses_out, gms_align_record *records) {
    return map_align(m, mi, beams, B, poses_in, P, params, poses_out, records, false);
}
int gms_map_align_dev(gms_map *m, int32_t mi, const gms_beam *dev_beams, int32_t B, const float *dev_poses_in, int32_t P,
                      const gms_align_params *params, float *dev_poses_out, gms_align_record *dev_records) {
    return map_align(m, mi, dev_beams, B, dev_poses_in, P, params, dev_poses_out, dev_records, true);
}
int gms_pf_align(gms_pf *pf, const gms_beam *beams, int32_t B, const gms_align_params *params, gms_align_record *records) {
    return pf_align(pf, beams, B, params, records, false);
}
int gms_pf_align_dev(gms_pf *pf, const gms_beam *dev_beams, int32_t B, const gms_align_params *params, gms_align_record *dev_records) {
    return pf_align(pf, dev_beams, B, params, dev_records, true);
}

}  // extern "C"
