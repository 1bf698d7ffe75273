// gms_align.hip -- continuous scan alignment (gridmapslam.h "continuous scan alignment"): a damped Gauss-Newton scan matcher on the
// bilinearly interpolated likelihood field, for a list of poses on a map (gms_map_align) and for the particles of a shared-map filter
// in place (gms_pf_align).
//
// A translation unit of its own, kernel and C-ABI, on the query base beside gms_beams.hip: no kernel of the other units is compiled
// differently for it.
//
//   k_align        one wavefront per pose, four poses per workgroup of 256 lanes, grid (ceil(P / 4), maps).  The workgroup stages the
//                  scan's (local_x, local_y) in LDS once, 16 bytes per beam, NaN for a beam that did not hit -- the USED test refuses a
//                  NaN by itself, so the loop needs no hit flag.  Lane l owns partial l: it walks the beams l, l + 64, ... in ascending
//                  order, two adjacent field values per row (16 bytes, 8-byte aligned) and two rows per look-up, and adds the ten
//                  terms into its registers.  The halving tree p[l] += p[l + s], s = 32 .. 1, runs as cross-lane register moves
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

#include "gms_device.h"

#define ALIGN_NT 256
#define ALIGN_WAVES (ALIGN_NT / GMS_WAVE)
static_assert(sizeof(gms_align_record) == 80 && sizeof(gms_align_params) == 64, "gridmapslam.h states both sizes");

// two adjacent doubles of a field row: 8-byte aligned, so one 16-byte load where the target takes it
typedef double align_pair __attribute__((ext_vector_type(2), aligned(8)));

// lane 0's value in every lane
__device__ __forceinline__ double wave_first(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// the sums of one evaluation, in the header's order of terms
struct AlignSums {
    double h00, h01, h02, h11, h12, h22, g0, g1, g2, s;
    int32_t n;
};

// the header's halving tree over the 64 lanes' partials; lane 0 holds the sums afterwards, the broadcast makes them uniform
__device__ __forceinline__ void align_tree(AlignSums &a, int32_t lane) {
#define GMS_STEP_(O)                                                                          \
    {                                                                                         \
        const bool low = lane < (O);                                                          \
        const double t0 = wave_xor<O>(a.h00), t1 = wave_xor<O>(a.h01), t2 = wave_xor<O>(a.h02), t3 = wave_xor<O>(a.h11), t4 = wave_xor<O>(a.h12); \
        const double t5 = wave_xor<O>(a.h22), t6 = wave_xor<O>(a.g0), t7 = wave_xor<O>(a.g1), t8 = wave_xor<O>(a.g2), t9 = wave_xor<O>(a.s);      \
        const int32_t tn = wave_xor<O>(a.n);                                                  \
        if (low) {                                                                            \
            a.h00 = a.h00 + t0; a.h01 = a.h01 + t1; a.h02 = a.h02 + t2; a.h11 = a.h11 + t3; a.h12 = a.h12 + t4; \
            a.h22 = a.h22 + t5; a.g0 = a.g0 + t6; a.g1 = a.g1 + t7; a.g2 = a.g2 + t8; a.s = a.s + t9;           \
            a.n += tn;                                                                        \
        }                                                                                     \
    }
    GMS_BUTTERFLY(GMS_STEP_)
#undef GMS_STEP_
    a.h00 = wave_first(a.h00); a.h01 = wave_first(a.h01); a.h02 = wave_first(a.h02); a.h11 = wave_first(a.h11); a.h12 = wave_first(a.h12);
    a.h22 = wave_first(a.h22); a.g0 = wave_first(a.g0); a.g1 = wave_first(a.g1); a.g2 = wave_first(a.g2); a.s = wave_first(a.s);
    a.n = __builtin_amdgcn_readfirstlane(a.n);
}

// one evaluation at the pose (x, y, theta): every lane returns the same sums
__device__ __forceinline__ AlignSums align_eval(const GridDev &g, const double *__restrict__ lik, const double2 *s_beam, int32_t B, float x, float y,
                                               float theta, int32_t lane) {
    float cf, sf;
    pose_trig(theta, cf, sf);
    XformDev t;
    t.c = (double)cf; t.s = (double)sf; t.px = (double)x; t.py = (double)y;
    const double wmax = (double)(g.W - 2), hmax = (double)(g.H - 2);
    AlignSums a;
    a.h00 = a.h01 = a.h02 = a.h11 = a.h12 = a.h22 = a.g0 = a.g1 = a.g2 = a.s = 0.0;
    a.n = 0;
    for (int32_t b = lane; b < B; b += GMS_WAVE) {
        const double2 l = s_beam[b];
        const double lx = l.x, ly = l.y;
        const double gu = (xform_x(t, lx, ly) - g.posx) / g.res - 0.5;
        const double gv = (xform_y(t, lx, ly) - g.posy) / g.res - 0.5;
        const double fu = floor(gu), fv = floor(gv);
        if (fu >= 0.0 && fu <= wmax && fv >= 0.0 && fv <= hmax) {              // (a NaN or an infinity fails: nothing else is ever cast)
            const int32_t i0 = (int32_t)fu, j0 = (int32_t)fv;
            const double fx = gu - fu, fy = gv - fv;
            const double *row = lik + (size_t)j0 * (size_t)g.W + (size_t)i0;
            const align_pair r0 = *reinterpret_cast<const align_pair *>(row), r1 = *reinterpret_cast<const align_pair *>(row + g.W);
            const double l00 = r0.x, l10 = r0.y, l01 = r1.x, l11 = r1.y;
            const double m = (1.0 - fy) * ((1.0 - fx) * l00 + fx * l10) + fy * ((1.0 - fx) * l01 + fx * l11);
            const double mu = (1.0 - fy) * (l10 - l00) + fy * (l11 - l01);
            const double mv = (1.0 - fx) * (l01 - l00) + fx * (l11 - l10);
            const double ax = (-lx * t.s - ly * t.c) / g.res;
            const double ay = (lx * t.c - ly * t.s) / g.res;
            const double j2 = mu * ax + mv * ay;
            const double r = 1.0 - m;
            a.h00 = a.h00 + mu * mu; a.h01 = a.h01 + mu * mv; a.h02 = a.h02 + mu * j2;
            a.h11 = a.h11 + mv * mv; a.h12 = a.h12 + mv * j2; a.h22 = a.h22 + j2 * j2;
            a.g0 = a.g0 + mu * r; a.g1 = a.g1 + mv * r; a.g2 = a.g2 + j2 * r;
            a.s = a.s + m;
            a.n++;
        }
    }
    align_tree(a, lane);
    return a;
}

__device__ __forceinline__ double align_clamp(double v, double m) { return v > m ? m : (v < -m ? -m : v); }

// grid (ceil(P / 4), maps).  lik: map blockIdx.y's field at lik + y * lik_stride; beams likewise beam_stride apart; pose_in / pose_out
// [maps][P][3] (may be the same), cs [maps][P][2] or NULL: the final poses' float-rounded trig; rec [maps][P] or NULL
__global__ void __launch_bounds__(ALIGN_NT)
k_align(GridDev g, const double *__restrict__ lik, int64_t lik_stride, const gms_beam *__restrict__ beams, int32_t B, int32_t beam_stride,
        const float *pose_in, float *pose_out, float *__restrict__ cs, gms_align_record *__restrict__ rec, int32_t P, gms_align_params prm) {
    extern __shared__ __align__(16) double2 s_beam[];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, mi = (int32_t)blockIdx.y;
    lik += (size_t)mi * (size_t)lik_stride;
    beams += (size_t)mi * (size_t)beam_stride;
    for (int32_t b = tid; b < B; b += ALIGN_NT) {
        const gms_beam m = beams[b];
        s_beam[b] = m.hit != 0 ? make_double2(m.local_x, m.local_y) : make_double2(NAN, NAN);
    }
    __syncthreads();
    const int32_t p = (int32_t)blockIdx.x * ALIGN_WAVES + (tid >> 6);
    if (p >= P) return;                                                         // (uniform per wavefront; no barrier follows)
    const size_t gi = (size_t)mi * (size_t)P + (size_t)p;
    float x = pose_in[3 * gi], y = pose_in[3 * gi + 1], theta = pose_in[3 * gi + 2];
    int32_t status = 0, done = 0, n0 = 0;
    double s0 = 0.0;
    AlignSums e;
    for (int32_t k = 0;; k++) {
        e = align_eval(g, lik, s_beam, B, x, y, theta, lane);
        if (k == 0) { n0 = e.n; s0 = e.s; }
        if (status != 0 || k >= prm.iters) break;
        if (e.n == 0) { status = 2; break; }
        const double a00 = e.h00 + prm.damp_t, a01 = e.h01, a02 = e.h02, a11 = e.h11 + prm.damp_t, a12 = e.h12, a22 = e.h22 + prm.damp_r;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        if (!(fabs(det) > prm.det_min)) { status = 3; break; }
        const double d0 = align_clamp((c00 * e.g0 + c01 * e.g1 + c02 * e.g2) / det, prm.max_t);
        const double d1 = align_clamp((c01 * e.g0 + c11 * e.g1 + c12 * e.g2) / det, prm.max_t);
        const double d2 = align_clamp((c02 * e.g0 + c12 * e.g1 + c22 * e.g2) / det, prm.max_r);
        x = (float)((double)x + d0 * g.res);
        y = (float)((double)y + d1 * g.res);
        theta = (float)((double)theta + d2);
        done++;
        if (fabs(d0) <= prm.eps_t && fabs(d1) <= prm.eps_t && fabs(d2) <= prm.eps_r) status = 1;
    }
    if (lane != 0) return;
    pose_out[3 * gi] = x; pose_out[3 * gi + 1] = y; pose_out[3 * gi + 2] = theta;
    if (cs) {
        float cf, sf;
        pose_trig(theta, cf, sf);
        cs[2 * gi] = cf; cs[2 * gi + 1] = sf;
    }
    if (rec) {
        gms_align_record r;
        r.status = status; r.iters_done = done; r.n_used = e.n; r.n_used0 = n0;
        r.score0 = s0; r.score = e.s;
        r.H[0] = e.h00; r.H[1] = e.h01; r.H[2] = e.h02; r.H[3] = e.h11; r.H[4] = e.h12; r.H[5] = e.h22;
        rec[gi] = r;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int align_check(const gms_align_params *p, const char *who) {
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
    int rc = gms_kernel_lds<k_align>(GMS_MAX_BEAMS * 16);
    if (rc) return rc;
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
    int rc = align_check(prm, who);
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
    int rc = align_check(prm, who);
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

int gms_align_check(const gms_align_params *p) { return align_check(p, "gms_align_params"); }

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
