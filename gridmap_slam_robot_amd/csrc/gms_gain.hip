// gms_gain.hip -- view gain (gridmapslam.h "view gain"): the distinct cells a scan from a candidate pose would see, by class.
//
// A translation unit of its own, kernel and C-ABI, layered on the query base beside gms_cast.hip: nothing here is on the scan step's
// path, and no kernel of the other units is compiled differently for it.
//
//   the planes     both planes of the query base (query_plane, gms_query.hip), read in place: GMS_CLEAR_OCCUPIED (logData > 0, what ends
//                  a walk) and GMS_CLEAR_NOT_FREE (!(logData < 0)).  A shared map keeps them until logData moves, so a gain after a cast
//                  packs nothing; a gms_slam's are the shown particle's, packed per request into the two scratch planes the frontier
//                  regions use (d_clear_scratch, d_front_nf).
//   k_gain         one workgroup of 256 lanes per pose.  Every probe of a pose starts in the same cell (cx, cy), so the cells a pose can
//                  see lie in the square of side 2 * max_range + 1 around it, clipped to the map: the WINDOW, columns in 32-bit words
//                  from x0 >> 5.  The workgroup zeroes a visited bitmap of the window in LDS, the lanes stride over the probes and walk
//                  ray_init(.., 0) / ray_step (gms_device.h, the casts' float recurrence) to the range cut, the map's edge or the first
//                  occupied cell, setting their cells' bits -- the bit is tested first and the LDS atomic issued only where it is still
//                  clear: all rays of a pose share their first cells, the race is benign (a lost test costs one atomic) and the near
//                  field does not serialise on one address.  After a barrier the window is classed word by word: occupied = popc(vis &
//                  occ), unknown = popc(vis & nf & ~occ), free = popc(vis & ~nf); the five counts are reduced over the workgroup and one
//                  lane stores the 32-byte record as two 16-byte vector stores.
//   staging        where bitmap and both plane windows fit GAIN_LDS_CAP together the plane windows are staged in LDS as well and walk
//                  and classing read them there; otherwise, or with GMS_GAIN_WALK=mem, plane words come from memory.  The bitmap is
//                  always in LDS: max_range <= 255 bounds it by 17 words x 511 rows = 34,748 bytes.  Staging decides where a bit is read,
//                  never what is returned.
//   its own code   k_gain does not take its ray set-up, window geometry and staging from gms_probe.h as the casts and the beam model do:
//                  written on those helpers it computed the same records 0.4 to 1.3 % slower on two of the probe's figures, outside the
//                  parent's own spread ("the probe geometry the ray queries share"), so the kernel stays as it was.
//
// LDS: at most GAIN_LDS_CAP = 64 KiB per workgroup (two per CU at the cap, k_cast_map's reasoning), the 128 bytes of bookkeeping
// included.  Every walk's loop carries the bound 2 * max_range + 2: a monotone walk inside the square has at most 2 * max_range + 1 cells.
#undef GMS_STAMPS
#include <algorithm>

#include "gms_device.h"

#define GAIN_NT 256
#define GAIN_LDS_CAP (64 * 1024)         // bytes of LDS a workgroup uses at most, static and dynamic
#define GAIN_LDS_STATIC 128              // what k_gain declares statically: the pose, the start cell, the waves' partial counts

static_assert(sizeof(gms_gain_rec) == 32, "gms_gain_rec is two 16-byte stores");
static_assert(sizeof(gms_gain) == 8, "gms_gain is two int32_t");

// the window's size bound for a request: words per row and rows (the kernel's own window never exceeds it)
static inline int32_t gain_win_words(int32_t max_range, int32_t wpr) { return std::min(wpr, (2 * max_range + 31) / 32 + 1); }   // 2R + 1 cells from bit 31
static inline int32_t gain_win_rows(int32_t max_range, int32_t H) { return std::min(H, 2 * max_range + 1); }

template <int O> __device__ __forceinline__ void gain_fold(int32_t (&c)[5]) {
#pragma unroll
    for (int i = 0; i < 5; i++) c[i] += wave_xor<O>(c[i]);
}

// cap_words: the words of ONE window the launch asked LDS for (the visited bitmap; staged: the two plane windows behind it)
__global__ void __launch_bounds__(GAIN_NT)
k_gain(GridDev g, const uint32_t *__restrict__ occ, const uint32_t *__restrict__ nf, int32_t wpr, const gms_beam *__restrict__ probes, int32_t B,
       const float *__restrict__ poses, int32_t max_range, gms_gain_rec *__restrict__ out, int32_t cap_words, int32_t staged) {
    extern __shared__ __align__(16) uint32_t s_vis[];
    __shared__ XformDev s_t;
    __shared__ int32_t s_start[2];
    __shared__ int32_t s_part[GAIN_NT / 64][5];
    const int32_t pi = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x;
    if (tid == 0) {
        const float *pose = poses + (size_t)pi * 3;
        float c, s;
        pose_trig(pose[2], c, s);                                                               // GridMap.java:175
        XformDev t;
        t.c = (double)c; t.s = (double)s; t.px = (double)pose[0]; t.py = (double)pose[1];
        s_t = t;
        const float sx = (float)((xform_x(t, 0.0, 0.0) - g.posx) / g.res), sy = (float)((xform_y(t, 0.0, 0.0) - g.posy) / g.res);
        s_start[0] = j_d2i(floor((double)(sx + 0.5f)));                                         // RayIterator.java:71-72: every probe's first cell
        s_start[1] = j_d2i(floor((double)(sy + 0.5f)));
    }
    __syncthreads();
    const XformDev t = s_t;
    const int32_t cx = s_start[0], cy = s_start[1], R = max_range;
    // the window: the square around the start cell, clipped to the map; none where the start lies outside (no probe walks then)
    int32_t wx0 = 0, wy0 = 0, ww = 0, wh = 0;
    if (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) {
        const int32_t x0 = max(0, cx - R), x1 = min(g.W - 1, cx + R), y0 = max(0, cy - R), y1 = min(g.H - 1, cy + R);
        wx0 = x0 >> 5; wy0 = y0;
        ww = (x1 >> 5) - wx0 + 1; wh = y1 - y0 + 1;
        if (ww * wh > cap_words) ww = wh = 0;                                                   // (never: gain_win_words x gain_win_rows bounds it)
    }
    const int32_t n = ww * wh;
    uint32_t *__restrict__ s_occ = s_vis + cap_words, *__restrict__ s_nf = s_vis + 2 * (size_t)cap_words;
    for (int32_t i = tid; i < n; i += GAIN_NT) {
        s_vis[i] = 0u;
        if (staged) {
            const int32_t row = i / ww, w = i - row * ww;
            const size_t at = (size_t)(wy0 + row) * (size_t)wpr + (size_t)(wx0 + w);
            s_occ[i] = occ[at];
            s_nf[i] = nf[at];
        }
    }
    __syncthreads();
    int32_t cnt[5] = {0, 0, 0, 0, 0};                                                           // unknown, free, occupied, hits, walked
    if (n > 0) {
        const float sx = (float)((xform_x(t, 0.0, 0.0) - g.posx) / g.res);                      // GridMap.java:178
        const float sy = (float)((xform_y(t, 0.0, 0.0) - g.posy) / g.res);                      // :179
        const int32_t bound = 2 * R + 2;
        for (int32_t b = tid; b < B; b += GAIN_NT) {
            const gms_beam m = probes[b];
            const float ex = (float)((xform_x(t, m.local_x, m.local_y) - g.posx) / g.res);      // :185
            const float ey = (float)((xform_y(t, m.local_x, m.local_y) - g.posy) / g.res);      // :186
            RayDev r;
            ray_init(r, sx + 0.5f, sy + 0.5f, ex + 0.5f, ey + 0.5f, 0);                         // :210 without the extra steps
            for (int32_t step = 0; step < bound && ray_has_next(r, g.W, g.H); step++) {
                if (max(abs(r.x - cx), abs(r.y - cy)) > R) break;                               // the range cut (monotone: it never comes back)
                if (step == 0) cnt[4]++;
                const int32_t i = (r.y - wy0) * ww + ((r.x >> 5) - wx0);
                const uint32_t bit = 1u << (r.x & 31);
                if (!(s_vis[i] & bit)) atomicOr(&s_vis[i], bit);
                const uint32_t word = staged ? s_occ[i] : occ[(size_t)r.y * (size_t)wpr + (size_t)(r.x >> 5)];
                if (word & bit) { cnt[3]++; break; }                                            // the first occupied cell ends the walk, and counts
                ray_step(r);
            }
        }
    }
    __syncthreads();
    for (int32_t i = tid; i < n; i += GAIN_NT) {
        const uint32_t v = s_vis[i];
        if (!v) continue;
        uint32_t o, f;
        if (staged) { o = s_occ[i]; f = s_nf[i]; }
        else {
            const int32_t row = i / ww, w = i - row * ww;
            const size_t at = (size_t)(wy0 + row) * (size_t)wpr + (size_t)(wx0 + w);
            o = occ[at]; f = nf[at];
        }
        cnt[0] += __popc(v & f & ~o);
        cnt[1] += __popc(v & ~f);
        cnt[2] += __popc(v & o);
    }
    gain_fold<32>(cnt); gain_fold<16>(cnt); gain_fold<8>(cnt); gain_fold<4>(cnt); gain_fold<2>(cnt); gain_fold<1>(cnt);
    if ((tid & 63) == 0)
        for (int i = 0; i < 5; i++) s_part[tid >> 6][i] = cnt[i];
    __syncthreads();
    if (tid == 0) {
        int32_t tot[5];
        for (int i = 0; i < 5; i++) tot[i] = s_part[0][i] + s_part[1][i] + s_part[2][i] + s_part[3][i];
        const bool any = tot[4] > 0;
        int4 *dst = reinterpret_cast<int4 *>(out + pi);
        dst[0] = make_int4(tot[0], tot[1], tot[2], tot[3]);
        dst[1] = make_int4(tot[4], any ? cx : -1, any ? cy : -1, 0);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// P poses at d_poses see d_probes [B] in ONE map's two planes: the records into d_out [P]
static int gain_launch(gms_map *m, const uint32_t *d_occ, const uint32_t *d_nf, int32_t max_range, const float *d_poses, int32_t P, const gms_beam *d_probes,
                       int32_t B, gms_gain_rec *d_out) {
    const int32_t wpr = gms_plane_wpr(m);
    const int64_t cap_words = (int64_t)gain_win_words(max_range, wpr) * gain_win_rows(max_range, m->gd.H);
    const int64_t budget = GAIN_LDS_CAP - GAIN_LDS_STATIC;
    if (cap_words * 4 > budget) return gms_fail(GMS_ERR_INTERNAL, "gms_gain: a visited bitmap of %lld bytes", (long long)(cap_words * 4));
    const bool staged = !m->gain_walk_mem && 3 * cap_words * 4 <= budget;
    HIPCHK(gms_kernel_lds<k_gain>(m->device, GAIN_LDS_CAP - GAIN_LDS_STATIC));
    hipLaunchKernelGGL(k_gain, dim3((unsigned)P), dim3(GAIN_NT), (size_t)(staged ? 3 : 1) * (size_t)cap_words * 4, m->stream, m->gd, d_occ, d_nf, wpr, d_probes, B,
                       d_poses, max_range, d_out, (int32_t)cap_words, staged ? 1 : 0);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the gain of P poses in one map of a shared handle or in the shown particle's map of a per-particle one; `shown` exists for a particle only
static int gain(QuerySource src, const char *what, const gms_gain *g, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_gain_rec *out,
                int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !g || !poses || !probes || !out)
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the poses, the probes and the output are required)", what);
    gms_map *m = src.m;
    if (g->max_range < 1 || g->max_range > 255) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= gms_gain.max_range <= 255 cells", what);
    if (P < 1 || P > GMS_MAX_PARTICLES) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= P <= GMS_MAX_PARTICLES poses", what);
    if (on_device && ((uintptr_t)out & 15) != 0) return gms_fail(GMS_ERR_INVALID, "%s: the device output must be 16-byte aligned", what);
    if (B < 1 || B > m->max_beams) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= B <= gms_params.max_beams probes", what);
    src.filter = g->filter;
    int rc = query_check(src, what, "gms_gain.filter");                         // the map's index, or the shown particle
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    if (src.s) {
        rc = gms_dev_alloc(&m->d_front_nf, (size_t)m->gd.H * (size_t)gms_plane_wpr(m) * sizeof(uint32_t), what, "the particle's second plane");
        if (rc) return rc;
    }
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)P * sizeof(gms_gain_rec), probe_bytes = (size_t)B * sizeof(gms_beam), pose_bytes = (size_t)P * 3 * sizeof(float);
    const size_t p_out = st.part(out_bytes), p_probes = st.part(probe_bytes), p_poses = st.part(pose_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_probes, probes, probe_bytes);
    if (!rc) rc = st.up(p_poses, poses, pose_bytes);
    if (rc) return rc;
    // both predicates: the map's two planes in place; a particle's packed per request, the second into d_front_nf
    const uint32_t *occ = nullptr, *nf = nullptr;
    rc = query_plane(src, GMS_CLEAR_OCCUPIED, st.shown(shown), nullptr, &occ);
    if (!rc) rc = query_plane(src, GMS_CLEAR_NOT_FREE, nullptr, src.s ? m->d_front_nf : nullptr, &nf);
    if (!rc) rc = gain_launch(m, occ, nf, g->max_range, st.at(p_poses, poses), P, st.at(p_probes, probes), B, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, out_bytes);
    return st.finish(shown);
}

extern "C" {

int gms_map_gain(gms_map *m, int32_t mi, const gms_gain *g, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_gain_rec *out) {
    return gain(query_map(m, mi), "gms_map_gain", g, poses, P, probes, B, out, nullptr, false);
}
int gms_map_gain_dev(gms_map *m, int32_t mi, const gms_gain *g, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B, gms_gain_rec *dev_out) {
    return gain(query_map(m, mi), "gms_map_gain_dev", g, dev_poses, P, dev_probes, B, dev_out, nullptr, true);
}
int gms_slam_gain(gms_slam *s, int32_t which, const gms_gain *g, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_gain_rec *out,
                  int32_t *shown) {
    return gain(query_slam(s, which), "gms_slam_gain", g, poses, P, probes, B, out, shown, false);
}
int gms_slam_gain_dev(gms_slam *s, int32_t which, const gms_gain *g, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B,
                      gms_gain_rec *dev_out, int32_t *dev_shown) {
    return gain(query_slam(s, which), "gms_slam_gain_dev", g, dev_poses, P, dev_probes, B, dev_out, dev_shown, true);
}

}  // extern "C"
