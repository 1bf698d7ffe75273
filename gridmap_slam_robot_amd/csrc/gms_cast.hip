// gms_cast.hip -- predicted scans (gridmapslam.h "predicted scans"): the first occupied cell of integrateObservation's walk, per probe.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the plane      the shared-map casts walk the map's GMS_CLEAR_OCCUPIED plane (gms_map_plane, gms_query.hip): logData > 0 of every map
//                  at one bit per cell, kept on the handle until logData moves.
//   k_cast_map     lane = probe, workgroup = 256 neighbouring probes of ONE pose.  The workgroup stages the window of its rays
//                  (PlaneWindow, gms_probe.h: the box of one ray per lane, padded by extra_steps + 1) when it fits what the launch
//                  asked for, and every lane walks to the first set bit (ray_first).  A window that does not fit, or
//                  GMS_CAST_WALK=mem: every bit from memory (plane_bit).  What the window may and may not decide: PlaneWindow::bit.
//   k_cast_slam    the per-particle filter, one workgroup per particle: pose, trig and the maps' generation from device state; plane 0 of
//                  the particle's class planes (2 bits per cell, gms_slam_kernels.hip: 0 logData == 0 or NaN, 1 logData < 0, 2 logData > 0
//                  -- code 2 IS "occupied", the class k_slam_codes_from_log and the apply pass of k_slam_particle write for logData > 0)
//                  staged in LDS (at most 24 KiB), lanes stride over the probes.  No planes kept, or GMS_CAST_WALK=mem: logData itself.
//
// LDS: k_cast_map asks for min(64 KiB, the whole plane of one map) + 64 bytes of bookkeeping -- two workgroups per CU at the cap;
// k_cast_slam for the particle's plane (3.6 KB at 120 x 120, at most 24 KiB).  Every walk's loop carries the bound W + H + extra + 2.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gms_probe.h"

#define CAST_NT 256
#define CAST_LDS_CAP (64 * 1024)         // k_cast_map's window: bytes of LDS a workgroup asks for at most

static_assert(sizeof(gms_cast_hit) == 16, "gms_cast_hit is one 16-byte store");

// the record of a probe whose walk found no occupied cell
__device__ __forceinline__ gms_cast_hit cast_miss(float measured) {
    gms_cast_hit h;
    h.step = -1; h.x = -1; h.y = -1; h.range = measured;
    return h;
}
__device__ __forceinline__ void cast_store(gms_cast_hit *__restrict__ out, const gms_cast_hit &h) {
    *reinterpret_cast<int4 *>(out) = make_int4(h.step, h.x, h.y, (int32_t)__float_as_uint(h.range));
}
// the record of the first occupied cell of a probe's walk (ray_first, gms_probe.h), or of none
template <class Occ>
__device__ __forceinline__ gms_cast_hit cast_walk(const GridDev &g, const RayIn &ray, Occ occ) {
    return ray_first(g, ray, g.extra, occ, [&](int32_t step, const RayDev &r) {
        gms_cast_hit h;
        h.step = step; h.x = r.x; h.y = r.y;
        h.range = cell_distance(ray.sx, ray.sy, r.x, r.y);                                      // GridMap.java:215-217
        return h;
    }, cast_miss(ray.measured));
}

// poses: pose i at poses + i * pose_stride floats; per_map: pose i is cast in map i's plane (gms_map_cast_at of a batched handle),
// else every pose in `plane` as given.  lds_words: the window the launch asked for (0: walk memory)
__global__ void __launch_bounds__(CAST_NT)
k_cast_map(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, int64_t plane_stride, int32_t per_map, const gms_beam *__restrict__ probes,
           int32_t B, int32_t bpp, const float *__restrict__ poses, int32_t pose_stride, gms_cast_hit *__restrict__ out, int32_t lds_words) {
    extern __shared__ __align__(16) uint32_t s_win[];
    __shared__ XformDev s_t;
    __shared__ int32_t s_box[4];
    const int32_t pi = (int32_t)(blockIdx.x / (uint32_t)bpp), b = (int32_t)(blockIdx.x % (uint32_t)bpp) * CAST_NT + (int32_t)threadIdx.x;
    if (per_map) plane += (size_t)pi * (size_t)plane_stride;
    if (threadIdx.x == 0) {
        s_t = pose_xform(poses + (size_t)pi * (size_t)pose_stride);                             // GridMap.java:175
        s_box[0] = g.W; s_box[1] = g.H; s_box[2] = -1; s_box[3] = -1;
    }
    __syncthreads();
    const XformDev t = s_t;
    RayIn ray;
    ray.sx = ray.sy = ray.ex = ray.ey = ray.measured = 0.0f; ray.hit = 0;
    if (b < B) ray = make_ray(g, t, probes[b]);
    PlaneWindow win;                                                                            // (none: walk memory)
    if (lds_words > 0) {
        if (b < B) {
            int32_t box[4];
            PlaneWindow::box_of(box, ray, g.W, g.H);
            PlaneWindow::box_merge(s_box, box);
        }
        __syncthreads();
        win = PlaneWindow::clip(s_box, g.extra + 1, g.W, g.H, lds_words);
        win.stage(s_win, plane, wpr, (int32_t)threadIdx.x, CAST_NT);
        __syncthreads();
    }
    if (b >= B) return;
    gms_cast_hit h;
    const auto mem = [&](int32_t x, int32_t y) { return plane_bit(plane, wpr, x, y); };
    if (win.ww > 0) h = cast_walk(g, ray, [&](int32_t x, int32_t y) { return win.bit(s_win, x, y, mem); });
    else h = cast_walk(g, ray, mem);
    cast_store(out + (size_t)pi * (size_t)B + (size_t)b, h);
}

// which >= 0: that particle; GMS_VIEW_STRONGEST: the strongest of `filter` by the last update's statistics (as k_slam_view picks it);
// GMS_CAST_ALL: particle blockIdx.x, its records at out + blockIdx.x * B
template <bool CODES>
__global__ void __launch_bounds__(CAST_NT)
k_cast_slam(GridDev g, SlamBufs sb, int64_t code_words, const PfStatsDev *__restrict__ stats, int32_t which, int32_t filter, const float *__restrict__ pose,
            const float *__restrict__ cs, const gms_beam *__restrict__ probes, int32_t B, gms_cast_hit *__restrict__ out, int32_t *__restrict__ shown) {
    extern __shared__ __align__(16) uint32_t s_codes[];
    const int32_t p = which == GMS_CAST_ALL ? (int32_t)blockIdx.x : (which >= 0 ? which : filter * sb.n_per + stats[filter].strongest);
    const int32_t cur = sb.epoch[2 * (p / sb.n_per)] & 1;                                       // the current generation of the particle's filter
    if (which == GMS_CAST_ALL) out += (size_t)blockIdx.x * (size_t)B;
    else if (shown && threadIdx.x == 0) *shown = p;
    const double *__restrict__ logd = (cur ? sb.log[1] : sb.log[0]) + (size_t)p * (size_t)g.cells;
    if (CODES) {
        const uint32_t *__restrict__ codes = (cur ? sb.code[1] : sb.code[0]) + (size_t)p * 2 * (size_t)code_words;     // plane 0: logData as it stands
        for (int32_t i = (int32_t)threadIdx.x; i < (int32_t)code_words; i += CAST_NT) s_codes[i] = codes[i];
        __syncthreads();
    }
    const XformDev t = pose_xform(pose + 3 * (size_t)p, cs + 2 * (size_t)p);
    for (int32_t b = (int32_t)threadIdx.x; b < B; b += CAST_NT) {
        const RayIn ray = make_ray(g, t, probes[b]);
        gms_cast_hit h;
        if (CODES) {
            h = cast_walk(g, ray, [&](int32_t x, int32_t y) {
                const int32_t c = x + y * g.W;
                return ((s_codes[c >> 4] >> (2 * (c & 15))) & 3u) == 2u;                        // code 2: logData > 0
            });
        } else {
            h = cast_walk(g, ray, [&](int32_t x, int32_t y) { return logd[(size_t)x + (size_t)y * (size_t)g.W] > 0.0; });
        }
        cast_store(out + b, h);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// P poses at d_poses (pose_stride floats apart) cast d_probes [B] in map mi (per_map: pose i in map i) into d_out [P][B]
static int cast_launch(gms_map *m, int32_t mi, bool per_map, const float *d_poses, int32_t pose_stride, int32_t P, const gms_beam *d_probes, int32_t B,
                       gms_cast_hit *d_out) {
    const uint32_t *plane = nullptr;
    int rc = gms_map_plane(m, GMS_CLEAR_OCCUPIED, &plane);
    if (rc) return rc;
    const int32_t wpr = gms_plane_wpr(m);
    const int64_t plane_stride = (int64_t)m->gd.H * wpr;
    const int64_t lds_words = m->cast_walk_mem ? 0 : std::min<int64_t>(CAST_LDS_CAP / 4, plane_stride);
    const int32_t bpp = (B + CAST_NT - 1) / CAST_NT;
    HIPCHK(gms_kernel_lds<k_cast_map>(m->device, CAST_LDS_CAP));
    hipLaunchKernelGGL(k_cast_map, dim3((unsigned)((int64_t)P * bpp)), dim3(CAST_NT), (size_t)lds_words * 4, m->stream, m->gd,
                       plane + (size_t)mi * (size_t)plane_stride, wpr, plane_stride, per_map ? 1 : 0, d_probes, B, bpp, d_poses, pose_stride,
                       d_out, (int32_t)lds_words);
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the tail map_cast and map_cast_at share: the host form's probes (and poses, where they are the caller's) staged, the launch, the records back
static int cast_run(gms_map *m, int32_t mi, bool per_map, const float *poses, int32_t pose_stride, int32_t P, const gms_beam *probes, int32_t B, gms_cast_hit *out,
                    bool on_device) {
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)P * (size_t)B * sizeof(gms_cast_hit), probe_bytes = (size_t)B * sizeof(gms_beam);
    const size_t pose_bytes = per_map ? 0 : (size_t)P * 3 * sizeof(float);                      // (per_map: the filter's statistics, on the device already)
    const size_t p_out = st.part(out_bytes), p_probes = st.part(probe_bytes), p_poses = st.part(pose_bytes);
    int rc = st.open();
    if (!rc) rc = st.up(p_probes, probes, probe_bytes);
    if (!rc && pose_bytes) rc = st.up(p_poses, poses, pose_bytes);
    if (!rc) rc = cast_launch(m, mi, per_map, pose_bytes ? st.at(p_poses, poses) : poses, pose_stride, P, st.at(p_probes, probes), B, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, out_bytes);
    return st.finish(nullptr);
}

static int map_cast(gms_map *m, int32_t mi, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_cast_hit *out, bool on_device) {
    REQUIRE(m && poses && probes && out, "gms_map_cast: null argument (the map, the poses, the probes and the output are required)");
    REQUIRE(mi >= 0 && mi < m->n_maps, "gms_map_cast: map index out of range");
    REQUIRE(B >= 1 && B <= m->max_beams, "gms_map_cast: 1 <= B <= gms_params.max_beams probes");
    REQUIRE(P >= 1 && P <= GMS_MAX_PARTICLES, "gms_map_cast: 1 <= P <= GMS_MAX_PARTICLES poses");
    REQUIRE(!on_device || ((uintptr_t)out & 15) == 0, "gms_map_cast_dev: the output must be 16-byte aligned");
    HIPCHK(hipSetDevice(m->device));
    return cast_run(m, mi, false, poses, 3, P, probes, B, out, on_device);
}

static int map_cast_at(gms_map *m, const gms_beam *probes, int32_t B, gms_pf *pf, int32_t which, gms_cast_hit *out, bool on_device) {
    REQUIRE(m && probes && pf && out, "gms_map_cast_at: null argument (the map, the probes, the filter and the output are required)");
    REQUIRE(pf->map == m, "gms_map_cast_at: the filter does not belong to this map");
    REQUIRE(which == 0 || which == 1, "gms_map_cast_at: which must be 0 (weighted pose) or 1 (strongest particle)");
    REQUIRE(B >= 1 && B <= m->max_beams, "gms_map_cast_at: 1 <= B <= gms_params.max_beams probes");
    REQUIRE(!on_device || ((uintptr_t)out & 15) == 0, "gms_map_cast_at_dev: the output must be 16-byte aligned");
    HIPCHK(hipSetDevice(m->device));
    // the pose where gms_map_integrate_at reads it: map i's in d_stats[i], at the PfStatsDev stride
    const char *stats = reinterpret_cast<const char *>(pf->d_stats);
    const float *d_poses = reinterpret_cast<const float *>(stats + (which == 0 ? offsetof(PfStatsDev, wpose) : offsetof(PfStatsDev, spose)));
    const int32_t stride = (int32_t)(sizeof(PfStatsDev) / sizeof(float));
    return cast_run(m, 0, true, d_poses, stride, m->n_maps, probes, B, out, on_device);
}

static int slam_cast(gms_slam *s, int32_t which, int32_t filter, const gms_beam *probes, int32_t B, gms_cast_hit *out, int32_t *shown, bool on_device) {
    REQUIRE(s && probes && out, "gms_slam_cast: null argument (the handle, the probes and the output are required)");
    gms_map *m = s->map;
    REQUIRE(B >= 1 && B <= m->max_beams, "gms_slam_cast: 1 <= B <= gms_params.max_beams probes");
    REQUIRE(!on_device || ((uintptr_t)out & 15) == 0, "gms_slam_cast_dev: the output must be 16-byte aligned");
    if (which != GMS_CAST_ALL) {
        int rc = gms_slam_shown(s, which, filter, "gms_slam_cast", "filter", &filter);
        if (rc) return rc;
    } else shown = nullptr;
    HIPCHK(hipSetDevice(m->device));
    const int32_t n_cast = which == GMS_CAST_ALL ? s->n : 1;
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)n_cast * (size_t)B * sizeof(gms_cast_hit), probe_bytes = (size_t)B * sizeof(gms_beam);
    const size_t p_out = st.part(out_bytes), p_probes = st.part(probe_bytes);
    int rc = st.open();
    if (!rc) rc = st.up(p_probes, probes, probe_bytes);
    if (rc) return rc;
    const SlamBufs sb = gms_slam_bufs(s);
    const gms_beam *d_probes = st.at(p_probes, probes);
    gms_cast_hit *d_out = st.at(p_out, out);
    int32_t *d_shown = which == GMS_CAST_ALL ? nullptr : st.shown(shown);
    const bool codes = s->d_code[0] && !m->cast_walk_mem;
    if (codes)
        hipLaunchKernelGGL((k_cast_slam<true>), dim3((unsigned)n_cast), dim3(CAST_NT), (size_t)s->code_words * 4, m->stream, m->gd, sb, s->code_words, s->pf->d_stats,
                           which, filter, s->pf->d_pose, s->pf->d_cs, d_probes, B, d_out, d_shown);
    else
        hipLaunchKernelGGL((k_cast_slam<false>), dim3((unsigned)n_cast), dim3(CAST_NT), 0, m->stream, m->gd, sb, s->code_words, s->pf->d_stats, which, filter,
                           s->pf->d_pose, s->pf->d_cs, d_probes, B, d_out, d_shown);
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, out_bytes);
    return st.finish(shown);
}

extern "C" {

int gms_map_cast(gms_map *m, int32_t mi, const float *poses, int32_t P, const gms_beam *probes, int32_t B, gms_cast_hit *out) {
    return map_cast(m, mi, poses, P, probes, B, out, false);
}
int gms_map_cast_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, const gms_beam *dev_probes, int32_t B, gms_cast_hit *dev_out) {
    return map_cast(m, mi, dev_poses, P, dev_probes, B, dev_out, true);
}
int gms_map_cast_at(gms_map *m, const gms_beam *probes, int32_t B, gms_pf *pf, int32_t which, gms_cast_hit *out) {
    return map_cast_at(m, probes, B, pf, which, out, false);
}
int gms_map_cast_at_dev(gms_map *m, const gms_beam *dev_probes, int32_t B, gms_pf *pf, int32_t which, gms_cast_hit *dev_out) {
    return map_cast_at(m, dev_probes, B, pf, which, dev_out, true);
}
int gms_slam_cast(gms_slam *s, int32_t which, int32_t filter, const gms_beam *probes, int32_t B, gms_cast_hit *out, int32_t *shown) {
    return slam_cast(s, which, filter, probes, B, out, shown, false);
}
int gms_slam_cast_dev(gms_slam *s, int32_t which, int32_t filter, const gms_beam *dev_probes, int32_t B, gms_cast_hit *dev_out, int32_t *dev_shown) {
    return slam_cast(s, which, filter, dev_probes, B, dev_out, dev_shown, true);
}
int gms_map_cast_plane_builds(const gms_map *m, int64_t *builds) {
    REQUIRE(m && builds, "gms_map_cast_plane_builds: null argument");
    *builds = m->cast_plane_builds;
    return GMS_OK;
}

}  // extern "C"
