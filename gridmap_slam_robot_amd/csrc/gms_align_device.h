// gms_align_device.h -- the arithmetic of the continuous scan alignment (gridmapslam.h "continuous scan alignment") that its kernels
// share: k_align (gms_align.hip: poses on one field in memory) and k_slam_align (gms_slam_align.hip: every particle on its own field).
// One copy of the scan's staging, the per-beam terms, the halving tree, the adjugate solve, the step and the final store: bit parity
// between the two rests on it.
#pragma once
#include <math.h>

#include "gms_device.h"

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

// the transform of an evaluation at the pose (x, y, theta): the float trig, widened
__device__ __forceinline__ XformDev align_xform(float x, float y, float theta) {
    float cf, sf;
    pose_trig(theta, cf, sf);
    XformDev t;
    t.c = (double)cf; t.s = (double)sf; t.px = (double)x; t.py = (double)y;
    return t;
}

// where the beam (lx, ly) ends, in cells from the first cell's centre, and the USED test on the doubles: true where the four cells
// (i0, j0) .. (i0 + 1, j0 + 1) = ((int)fu, (int)fv) .. lie inside the map (a NaN or an infinity fails: nothing else is ever cast)
struct AlignCell {
    double gu, gv, fu, fv;
};
__device__ __forceinline__ bool align_cell(const GridDev &g, const XformDev &t, double lx, double ly, AlignCell &c) {
    c.gu = (xform_x(t, lx, ly) - g.posx) / g.res - 0.5;
    c.gv = (xform_y(t, lx, ly) - g.posy) / g.res - 0.5;
    c.fu = floor(c.gu); c.fv = floor(c.gv);
    return c.fu >= 0.0 && c.fu <= (double)(g.W - 2) && c.fv >= 0.0 && c.fv <= (double)(g.H - 2);
}

// one used beam's ten terms onto a lane's partials, from the field's four values round its end point
__device__ __forceinline__ void align_add(AlignSums &a, const GridDev &g, const XformDev &t, double lx, double ly, const AlignCell &c, double l00,
                                          double l10, double l01, double l11) {
    const double fx = c.gu - c.fu, fy = c.gv - c.fv;
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

// the scan's (local_x, local_y) into s_beam [B], NaN for a beam that did not hit -- the USED test refuses a NaN by itself, so the
// evaluation needs no hit flag; the workgroup's nt lanes stride over the beams (the caller's barrier follows)
__device__ __forceinline__ void align_stage_scan(double2 *s_beam, const gms_beam *__restrict__ beams, int32_t B, int32_t tid, int32_t nt) {
    for (int32_t b = tid; b < B; b += nt) {
        const gms_beam m = beams[b];
        s_beam[b] = m.hit != 0 ? make_double2(m.local_x, m.local_y) : make_double2(NAN, NAN);
    }
}

// one evaluation at the pose (x, y, theta) by one wavefront: lane l owns partial l and walks the beams l, l + 64, ... in ascending
// order; every lane returns the same sums.  s_beam: the scan's (local_x, local_y), NaN for a beam that did not hit (the USED test
// refuses it).  fetch(b, i0, j0, l00, l10, l01, l11): the field's four values of beam b, whose cells have passed the test
template <typename Fetch>
__device__ __forceinline__ AlignSums align_eval(const GridDev &g, Fetch fetch, const double2 *s_beam, int32_t B, float x, float y, float theta,
                                               int32_t lane) {
    const XformDev t = align_xform(x, y, theta);
    AlignSums a;
    a.h00 = a.h01 = a.h02 = a.h11 = a.h12 = a.h22 = a.g0 = a.g1 = a.g2 = a.s = 0.0;
    a.n = 0;
    for (int32_t b = lane; b < B; b += GMS_WAVE) {
        const double2 l = s_beam[b];
        AlignCell c;
        if (align_cell(g, t, l.x, l.y, c)) {
            double l00, l10, l01, l11;
            fetch(b, (int32_t)c.fu, (int32_t)c.fv, l00, l10, l01, l11);
            align_add(a, g, t, l.x, l.y, c, l00, l10, l01, l11);
        }
    }
    align_tree(a, lane);
    return a;
}

// the four values from a field in memory: two adjacent values per row, two rows (i0 <= W - 2 and j0 <= H - 2: inside the W x H doubles)
struct AlignFetchMemory {
    const double *lik;
    int32_t W;
    __device__ __forceinline__ void operator()(int32_t, int32_t i0, int32_t j0, double &l00, double &l10, double &l01, double &l11) const {
        const double *row = lik + (size_t)j0 * (size_t)W + (size_t)i0;
        const align_pair r0 = *reinterpret_cast<const align_pair *>(row), r1 = *reinterpret_cast<const align_pair *>(row + W);
        l00 = r0.x; l10 = r0.y; l01 = r1.x; l11 = r1.y;
    }
};

__device__ __forceinline__ double align_clamp(double v, double m) { return v > m ? m : (v < -m ? -m : v); }

// What follows evaluation k of a pose: the end of the loop (true; status says why) or the damped Gauss-Newton step from the sums e --
// the adjugate solve of (H + diag(damp_t, damp_t, damp_r)) delta = g, the clamp, the pose's floats moved on (false)
__device__ __forceinline__ bool align_advance(const AlignSums &e, int32_t k, const gms_align_params &prm, double res, float &x, float &y, float &theta,
                                              int32_t &status, int32_t &done) {
    if (status != 0 || k >= prm.iters) return true;
    if (e.n == 0) { status = 2; return true; }
    const double a00 = e.h00 + prm.damp_t, a01 = e.h01, a02 = e.h02, a11 = e.h11 + prm.damp_t, a12 = e.h12, a22 = e.h22 + prm.damp_r;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = a00 * c00 + a01 * c01 + a02 * c02;
    if (!(fabs(det) > prm.det_min)) { status = 3; return true; }
    const double d0 = align_clamp((c00 * e.g0 + c01 * e.g1 + c02 * e.g2) / det, prm.max_t);
    const double d1 = align_clamp((c01 * e.g0 + c11 * e.g1 + c12 * e.g2) / det, prm.max_t);
    const double d2 = align_clamp((c02 * e.g0 + c12 * e.g1 + c22 * e.g2) / det, prm.max_r);
    x = (float)((double)x + d0 * res);
    y = (float)((double)y + d1 * res);
    theta = (float)((double)theta + d2);
    done++;
    if (fabs(d0) <= prm.eps_t && fabs(d1) <= prm.eps_t && fabs(d2) <= prm.eps_r) status = 1;
    return false;
}

// What one lane stores of pose i when its loop has ended: the pose, its float-rounded trig (cs NULL: none) and its record (rec NULL:
// none) from the last evaluation e and the first one's (n0, s0)
__device__ __forceinline__ void align_store(float *pose, float *cs, gms_align_record *rec, size_t i, float x, float y, float theta, const AlignSums &e,
                                            int32_t status, int32_t done, int32_t n0, double s0) {
    pose[3 * i] = x; pose[3 * i + 1] = y; pose[3 * i + 2] = theta;
    if (cs) {
        float cf, sf;
        pose_trig(theta, cf, sf);
        cs[2 * i] = cf; cs[2 * i + 1] = sf;
    }
    if (!rec) return;
    gms_align_record r;
    r.status = status; r.iters_done = done; r.n_used = e.n; r.n_used0 = n0;
    r.score0 = s0; r.score = e.s;
    r.H[0] = e.h00; r.H[1] = e.h01; r.H[2] = e.h02; r.H[3] = e.h11; r.H[4] = e.h12; r.H[5] = e.h22;
    rec[i] = r;
}
