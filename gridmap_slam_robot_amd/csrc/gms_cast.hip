// gms_cast.hip -- predicted scans (gridmapslam.h "predicted scans"): the first occupied cell of integrateObservation's walk, per probe.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the plane      the shared-map casts walk the map's GMS_CLEAR_OCCUPIED plane (gms_map_plane, gms_query.hip): logData > 0 of every map
//                  at one bit per cell, kept on the handle until logData moves.
//   k_cast_map     lane = probe, workgroup = 256 neighbouring probes of ONE pose.  The workgroup takes the box of its rays' start and end
//                  cells (+ extra_steps + 1, clipped to the map), stages those rows' words of the plane in LDS when they fit what the
//                  launch asked for, and every lane walks RayIterator's float recurrence (ray_init / ray_step, gms_device.h) to the first
//                  set bit.  A cell outside the staged window (the box is an estimate of the float walk, never a promise) is read from the
//                  plane in memory, so the window only ever decides WHERE a bit is read.  A window that does not fit, or
//                  GMS_CAST_WALK=mem: every bit from memory (the plane's base and pitch are kernel arguments, i.e. scalar registers; a
//                  lane's address is one multiply-add on top).
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

#include "gms_device.h"

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
// a coordinate of a ray's end as a cell for the window's box: saturated, then held to one cell around the map
__device__ __forceinline__ int32_t cast_box_cell(float v, int32_t n) { return max(-1, min(n, j_d2i(floor((double)v)))); }

// FIRST: does the walk's current cell hold an occupied cell?  occ(x, y) is only ever asked for cells inside the map.
template <class Occ>
__device__ __forceinline__ gms_cast_hit cast_walk(const GridDev &g, const RayIn &ray, Occ occ) {
    RayDev r;
    ray_init(r, ray.sx + 0.5f, ray.sy + 0.5f, ray.ex + 0.5f, ray.ey + 0.5f, g.extra);          // GridMap.java:210
    const int32_t bound = g.W + g.H + g.extra + 2;
    for (int32_t step = 0; step < bound && ray_has_next(r, g.W, g.H); step++) {                 // :211
        if (occ(r.x, r.y)) {
            gms_cast_hit h;
            h.step = step; h.x = r.x; h.y = r.y;
            h.range = cell_distance(ray.sx, ray.sy, r.x, r.y);                                  // :215-217
            return h;
        }
        ray_step(r);
    }
    return cast_miss(ray.measured);
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
        const float *pose = poses + (size_t)pi * (size_t)pose_stride;
        float c, s;
        pose_trig(pose[2], c, s);                                                               // GridMap.java:175
        XformDev t;
        t.c = (double)c; t.s = (double)s; t.px = (double)pose[0]; t.py = (double)pose[1];
        s_t = t;
        s_box[0] = g.W; s_box[1] = g.H; s_box[2] = -1; s_box[3] = -1;
    }
    __syncthreads();
    const XformDev t = s_t;
    RayIn ray;
    ray.sx = ray.sy = ray.ex = ray.ey = ray.measured = 0.0f; ray.hit = 0;
    if (b < B) {
        const gms_beam m = probes[b];
        ray.sx = (float)((xform_x(t, 0.0, 0.0) - g.posx) / g.res);                              // :178
        ray.sy = (float)((xform_y(t, 0.0, 0.0) - g.posy) / g.res);                              // :179
        ray.ex = (float)((xform_x(t, m.local_x, m.local_y) - g.posx) / g.res);                  // :185
        ray.ey = (float)((xform_y(t, m.local_x, m.local_y) - g.posy) / g.res);                  // :186
        ray.measured = (float)m.distance / g.resf;                                              // :188
    }
    int32_t wx0 = 0, wy0 = 0, ww = 0, wh = 0;                                                   // the staged window: words x rows (0: none)
    if (lds_words > 0) {
        if (b < B) {
            const int32_t ax = cast_box_cell(ray.sx + 0.5f, g.W), ay = cast_box_cell(ray.sy + 0.5f, g.H);
            const int32_t bx = cast_box_cell(ray.ex + 0.5f, g.W), by = cast_box_cell(ray.ey + 0.5f, g.H);
            atomicMin(&s_box[0], min(ax, bx)); atomicMin(&s_box[1], min(ay, by));
            atomicMax(&s_box[2], max(ax, bx)); atomicMax(&s_box[3], max(ay, by));
        }
        __syncthreads();
        const int32_t pad = g.extra + 1;
        const int32_t x0 = max(0, s_box[0] - pad), y0 = max(0, s_box[1] - pad), x1 = min(g.W - 1, s_box[2] + pad), y1 = min(g.H - 1, s_box[3] + pad);
        if (x1 >= x0 && y1 >= y0) {
            wx0 = x0 >> 5; wy0 = y0;
            ww = (x1 >> 5) - wx0 + 1; wh = y1 - y0 + 1;
            if ((int64_t)ww * wh > (int64_t)lds_words) ww = wh = 0;                             // does not fit: this workgroup walks memory
        }
        const int32_t n = ww * wh;
        for (int32_t i = (int32_t)threadIdx.x; i < n; i += CAST_NT) {
            const int32_t row = i / ww, w = i - row * ww;
            s_win[i] = plane[(size_t)(wy0 + row) * (size_t)wpr + (size_t)(wx0 + w)];
        }
        __syncthreads();
    }
    if (b >= B) return;
    gms_cast_hit h;
    if (ww > 0) {
        h = cast_walk(g, ray, [&](int32_t x, int32_t y) {
            const uint32_t cw = (uint32_t)((x >> 5) - wx0), cr = (uint32_t)(y - wy0);
            const uint32_t word = (cw < (uint32_t)ww && cr < (uint32_t)wh) ? s_win[cr * (uint32_t)ww + cw] : plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)];
            return ((word >> (x & 31)) & 1u) != 0u;
        });
    } else {
        h = cast_walk(g, ray, [&](int32_t x, int32_t y) { return ((plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)] >> (x & 31)) & 1u) != 0u; });
    }
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
    XformDev t;
    t.px = (double)pose[3 * (size_t)p]; t.py = (double)pose[3 * (size_t)p + 1]; t.c = (double)cs[2 * (size_t)p]; t.s = (double)cs[2 * (size_t)p + 1];
    for (int32_t b = (int32_t)threadIdx.x; b < B; b += CAST_NT) {
        const gms_beam m = probes[b];
        RayIn ray;
        ray.sx = (float)((xform_x(t, 0.0, 0.0) - g.posx) / g.res);                              // GridMap.java:178
        ray.sy = (float)((xform_y(t, 0.0, 0.0) - g.posy) / g.res);                              // :179
        ray.ex = (float)((xform_x(t, m.local_x, m.local_y) - g.posx) / g.res);                  // :185
        ray.ey = (float)((xform_y(t, m.local_x, m.local_y) - g.posy) / g.res);                  // :186
        ray.measured = (float)m.distance / g.resf;                                              // :188
        ray.hit = 0;
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
    static bool attr_set = false;
    if (!attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cast_map), hipFuncAttributeMaxDynamicSharedMemorySize, CAST_LDS_CAP));
        attr_set = true;
    }
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
