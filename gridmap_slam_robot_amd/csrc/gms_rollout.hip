// gms_rollout.hip -- trajectory rollouts (gridmapslam.h "trajectory rollouts"): for a start pose and K candidate arcs of T steps each,
// the first step at which the robot's footprint collides, and the clearance and cost-to-go minima along the steps in front of it.
//
// A translation unit of its own, kernel and C-ABI, layered on the query base beside gms_gain.hip and on the cost-to-go fields' blocked
// plane (gms_reach_inflate): nothing here is on the scan step's path, and no kernel of the other units is compiled differently for it.
//
//   the blocked plane  reach's: with inflate == 0 the map's plane of `mode`, read in place (query_plane; a gms_slam's: the shown particle's,
//                      packed per request); with inflate > 0 gms_reach_inflate's scratch plane.
//   k_rollout          one workgroup of 256 lanes per (start pose, block of `cpw` candidates): grid (P, ceil(K / cpw)).  Lane 0 takes the
//                      pose's trig and its start cell; the workgroup stages the footprint (the centre behind it, point F) and -- unless
//                      MEM -- the WINDOW: the square of side 2 R + 1 cells around the start cell, one bit per cell, rows of
//                      ceil((2 R + 1) / 32) words, bit set = collides (blocked, or off the map); what lies outside the window is out of
//                      range or off the map, so a look-up is one bounds test and one bit test in LDS.  A start cell farther than R from
//                      the map has an empty window: everything collides.  Then one wavefront takes one candidate at a time: lanes own
//                      steps, 64 per pass, each lane loops over the F + 1 points in ascending order and stops at its first colliding one;
//                      a ballot gives the pass's first colliding step, the lanes in front of it read `clear` and `cost` under their centre
//                      cell (collision-free, so on the map) and two butterflies take the minima -- the cost's as the key cost << 16 | step,
//                      so the smallest step wins a tie --; the candidate's passes stop at the first hit.  Lane 0 stores the 32-byte record
//                      as two 16-byte vector stores.
//   RISK               the aggregate form for a filter's particles: no fields, no per-pose records; lane 0 issues integer atomics into the
//                      candidate's gms_rollout_risk (k_rollout_risk_init sets min_first_hit = T in front of the launch).
//   MEM                GMS_ROLLOUT_WALK=mem at handle creation: no window, every look-up tests the map's bounds, the range and the plane's
//                      bit in memory (tests).  The kind of a record's first hit is always taken that way, once per candidate.
//
// LDS: the window is at most 16 words x 511 rows = 32,704 bytes at R = 255, the footprint and the pose 560 bytes beside it.
#undef GMS_STAMPS
#include <math.h>
#include <string.h>

#include <algorithm>

#include "gms_device.h"

#define ROLL_NT 256
#define ROLL_WAVES (ROLL_NT / 64)

static_assert(sizeof(gms_rollout_step) == 16, "gms_rollout_step is one 16-byte load");
static_assert(sizeof(gms_rollout_rec) == 32, "gms_rollout_rec is two 16-byte stores");
static_assert(sizeof(gms_rollout_risk) == 32 && sizeof(gms_rollout) == 16, "the header's sizes");
static_assert(GMS_ROLLOUT_MAX_T <= 0xFFFF && GMS_ROLLOUT_MAX_F < 0xFFFF, "steps and points are stored in 16 bits");

// whose pose a launch starts from: pose blockIdx.x of `poses`, or -- n_per > 0, a gms_slam without poses -- the shown particle's own
struct RollStart {
    const float *poses;
    const PfStatsDev *stats;
    int32_t which, filter, n_per;
};

// the window's words per row and its words in all, for a request's range
static inline int32_t roll_win_wpw(int32_t R) { return (2 * R + 1 + 31) / 32; }
static inline int32_t roll_win_words(int32_t R) { return roll_win_wpw(R) * (2 * R + 1); }

// the cell of footprint point (fx, fy) at step st under the start pose t: gridmapslam.h "step arithmetic", every operation rounded
__device__ __forceinline__ void roll_cell(const GridDev &g, const XformDev &t, const gms_rollout_step &st, float fx, float fy, int32_t &cx, int32_t &cy) {
    const double c = (double)st.c, s = (double)st.s, px = (double)fx, py = (double)fy;
    const double qx = (double)st.dx + (c * px - s * py);
    const double qy = (double)st.dy + (s * px + c * py);
    const double wx = xform_x(t, qx, qy) - g.posx, wy = xform_y(t, qx, qy) - g.posy;
    // (int)(w / res) by way of the reciprocal where that is provably the same int (j_cell_fast's guard), the division itself otherwise
    const double ax = wx * g.rinv, ay = wy * g.rinv;
    if (fabs(ax - rint(ax)) <= 0x1p-19 || fabs(ay - rint(ay)) <= 0x1p-19) {
        cx = j_d2i(wx / g.res);
        cy = j_d2i(wy / g.res);
    } else {
        cx = j_d2i(ax);
        cy = j_d2i(ay);
    }
}

// 0, or why cell (cx, cy) collides for a start cell (sx, sy): off the map, out of range, blocked -- in that order; from memory
__device__ __forceinline__ uint32_t roll_kind(const GridDev &g, const uint32_t *__restrict__ plane, int32_t wpr, int32_t sx, int32_t sy, int32_t R, int32_t cx,
                                              int32_t cy) {
    if (cx < 0 || cy < 0 || cx >= g.W || cy >= g.H) return GMS_ROLLOUT_HIT_OUTSIDE;
    const int64_t ddx = (int64_t)cx - (int64_t)sx, ddy = (int64_t)cy - (int64_t)sy;
    if (max(ddx < 0 ? -ddx : ddx, ddy < 0 ? -ddy : ddy) > (int64_t)R) return GMS_ROLLOUT_HIT_RANGE;
    return (plane[(size_t)cy * (size_t)wpr + (size_t)(cx >> 5)] >> (cx & 31)) & 1u ? GMS_ROLLOUT_HIT_BLOCKED : 0u;
}

// word j of plane row `row` with the cells at and behind column W set (the planes' padding is clear); a word off the row: all set
__device__ __forceinline__ uint32_t roll_row_word(const uint32_t *__restrict__ row, int32_t wpr, int32_t W, int32_t j) {
    if (j < 0 || j >= wpr) return 0xffffffffu;
    const int32_t left = W - 32 * j;                                            // cells of the word that are on the map
    return row[j] | (left <= 0 ? 0xffffffffu : left >= 32 ? 0u : 0xffffffffu << left);
}

template <int O> __device__ __forceinline__ uint32_t roll_min(uint32_t v) { return min(v, wave_xor<O>(v)); }

__global__ void __launch_bounds__(256)
k_rollout_risk_init(gms_rollout_risk *__restrict__ risk, int32_t K, int32_t T) {
    const int32_t k = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (k >= K) return;
    gms_rollout_risk r;
    r.n_hit = 0u; r.n_start_blocked = 0u; r.min_first_hit = (uint32_t)T; r.pad = 0u; r.sum_first_hit = 0ull; r.pad2 = 0ull;
    risk[k] = r;
}

// plane: ONE map's blocked plane; arcs [K][T]; points [F][2]; clear, cost: [H][W] or NULL; out [gridDim.x][K] (!RISK), risk [K] (RISK)
template <bool RISK, bool MEM>
__global__ void __launch_bounds__(ROLL_NT)
k_rollout(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, RollStart start, const gms_rollout_step *__restrict__ arcs, int32_t K, int32_t T,
          const float *__restrict__ points, int32_t F, int32_t R, int32_t cpw, const uint16_t *__restrict__ clear, const uint16_t *__restrict__ cost,
          gms_rollout_rec *__restrict__ out, gms_rollout_risk *__restrict__ risk) {
    extern __shared__ __align__(16) uint32_t s_win[];
    __shared__ XformDev s_t;
    __shared__ int32_t s_start[2];
    __shared__ float s_pts[GMS_ROLLOUT_MAX_F + 1][2];
    const int32_t pi = (int32_t)blockIdx.x, tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const gms_rollout_step ident = {0.0f, 0.0f, 1.0f, 0.0f};
    if (tid == 0) {
        const int32_t p = start.n_per > 0 ? (start.which >= 0 ? start.which : start.filter * start.n_per + start.stats[start.filter].strongest) : pi;
        const XformDev t = pose_xform(start.poses + (size_t)p * 3);
        s_t = t;
        int32_t sx, sy;
        roll_cell(g, t, ident, 0.0f, 0.0f, sx, sy);                             // the start cell: the centre's under the identity step
        s_start[0] = sx; s_start[1] = sy;
    }
    for (int32_t i = tid; i <= F; i += ROLL_NT) {
        s_pts[i][0] = i < F ? points[2 * (size_t)i] : 0.0f;
        s_pts[i][1] = i < F ? points[2 * (size_t)i + 1] : 0.0f;
    }
    __syncthreads();
    const XformDev t = s_t;
    const int32_t sx = s_start[0], sy = s_start[1];
    // the window: empty where the start cell lies farther than R from the map (every cell is then off the map or out of range)
    const bool far = sx < -R || sy < -R || sx > g.W - 1 + R || sy > g.H - 1 + R;
    const uint32_t side = MEM || far ? 0u : (uint32_t)(2 * R + 1), wpw = (side + 31u) >> 5;
    const int32_t ox = far ? 0 : sx - R, oy = far ? 0 : sy - R;
    if (!MEM) {
        const int32_t n = (int32_t)(side * wpw);
        for (int32_t i = tid; i < n; i += ROLL_NT) {
            const int32_t r = i / (int32_t)wpw, w = i - r * (int32_t)wpw, y = oy + r, x0 = ox + 32 * w;
            uint32_t v = 0xffffffffu;
            if (y >= 0 && y < g.H) {
                const uint32_t *__restrict__ row = plane + (size_t)y * (size_t)wpr;
                const int32_t j = x0 >> 5, sh = x0 & 31;                        // (x0 may be negative: the shift floors)
                const uint64_t both = ((uint64_t)roll_row_word(row, wpr, g.W, j + 1) << 32) | (uint64_t)roll_row_word(row, wpr, g.W, j);
                v = (uint32_t)(both >> sh);
            }
            s_win[i] = v;
        }
        __syncthreads();
    }
    auto collides = [&](int32_t cx, int32_t cy) -> bool {
        if (MEM) return roll_kind(g, plane, wpr, sx, sy, R, cx, cy) != 0u;
        const uint32_t lx = (uint32_t)cx - (uint32_t)ox, ly = (uint32_t)cy - (uint32_t)oy;
        if (lx >= side || ly >= side) return true;
        return (s_win[ly * wpw + (lx >> 5)] >> (lx & 31u)) & 1u;
    };
    // the footprint at the start pose itself: lanes over the points
    bool sb = false;
    for (int32_t f = lane; f <= F; f += 64) {
        int32_t cx, cy;
        roll_cell(g, t, ident, s_pts[f][0], s_pts[f][1], cx, cy);
        sb = sb || collides(cx, cy);
    }
    const bool start_blocked = __any(sb);
    const bool fields = !RISK && (clear || cost);

    const int32_t kb = (int32_t)blockIdx.y * cpw;
    for (int32_t kk = wave; kk < cpw; kk += ROLL_WAVES) {
        const int32_t k = kb + kk;
        if (k >= K) break;                                                      // (uniform per wavefront; no barrier follows)
        int32_t first = T, hit_point = 0xFFFF, hit_x = 0, hit_y = 0, last_x = sx, last_y = sy;
        uint32_t min_d2 = GMS_CLEAR_FAR, key = 0xffffffffu, end_cost = GMS_REACH_FAR;
        for (int32_t base = 0; base < T; base += 64) {
            const int32_t step = base + lane;
            int32_t mine = -1, cx = 0, cy = 0;
            if (step < T) {
                const gms_rollout_step st = arcs[(size_t)k * (size_t)T + (size_t)step];
                for (int32_t f = 0; f <= F; f++) {
                    roll_cell(g, t, st, s_pts[f][0], s_pts[f][1], cx, cy);
                    if (collides(cx, cy)) { mine = f; break; }
                }
            }
            const uint64_t hits = __ballot(mine >= 0);
            const int32_t L = hits ? __ffsll((unsigned long long)hits) - 1 : 64;
            const int32_t lim = min(L, min(64, T - base));                      // the lanes in front of it hold collision-free steps
            if (lim > 0) {
                uint32_t c_here = GMS_REACH_FAR;
                if (fields) {
                    uint32_t d2 = GMS_CLEAR_FAR, ky = 0xffffffffu;
                    if (lane < lim) {                                           // (the centre was the last point tested: cx, cy are its cell, on the map)
                        const size_t at = (size_t)cy * (size_t)g.W + (size_t)cx;
                        if (clear) d2 = clear[at];
                        if (cost) { c_here = cost[at]; ky = (c_here << 16) | (uint32_t)step; }
                    }
#define GMS_STEP_(O) d2 = roll_min<O>(d2); ky = roll_min<O>(ky);
                    GMS_BUTTERFLY(GMS_STEP_)
#undef GMS_STEP_
                    min_d2 = min(min_d2, d2);
                    key = min(key, ky);
                }
                if (!RISK) {
                    last_x = __shfl(cx, lim - 1);
                    last_y = __shfl(cy, lim - 1);
                    end_cost = (uint32_t)__shfl((int)c_here, lim - 1);
                }
            }
            if (L < 64) {
                first = base + L;
                hit_point = __shfl(mine, L);
                hit_x = __shfl(cx, L);
                hit_y = __shfl(cy, L);
                break;
            }
        }
        if (lane != 0) {
        } else if (RISK) {
            gms_rollout_risk *r = risk + k;
            if (first < T) atomicAdd(&r->n_hit, 1u);
            if (start_blocked) atomicAdd(&r->n_start_blocked, 1u);
            if (first < T) atomicMin(&r->min_first_hit, (uint32_t)first);
            if (first > 0) atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_first_hit), (unsigned long long)first);
        } else {
            const uint32_t flags = (first < T ? roll_kind(g, plane, wpr, sx, sy, R, hit_x, hit_y) : 0u) | (start_blocked ? GMS_ROLLOUT_START_BLOCKED : 0u);
            int4 *dst = reinterpret_cast<int4 *>(out + (size_t)pi * (size_t)K + (size_t)k);
            dst[0] = make_int4((int32_t)((uint32_t)first | ((uint32_t)hit_point << 16)), (int32_t)(min_d2 | ((key & 0xffffu) << 16)),
                               (int32_t)((key >> 16) | (end_cost << 16)), (int32_t)flags);
            dst[1] = make_int4(last_x, last_y, sx, sy);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int rollout_check(const gms_rollout *r, int32_t K, int32_t T, int32_t F, const char *who) {
    if (!r) return gms_fail(GMS_ERR_INVALID, "%s: null request", who);
    if (K < 1 || K > GMS_ROLLOUT_MAX_K) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= K <= GMS_ROLLOUT_MAX_K candidates", who);
    if (T < 1 || T > GMS_ROLLOUT_MAX_T) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= T <= GMS_ROLLOUT_MAX_T steps", who);
    if (F < 0 || F > GMS_ROLLOUT_MAX_F) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= F <= GMS_ROLLOUT_MAX_F footprint points", who);
    if (r->max_range < 1 || r->max_range > 255) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= gms_rollout.max_range <= 255 cells", who);
    if (r->inflate < 0 || r->inflate > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= gms_rollout.inflate <= 255 cells", who);
    if (r->mode != GMS_CLEAR_OCCUPIED && r->mode != GMS_CLEAR_NOT_FREE)
        return gms_fail(GMS_ERR_INVALID, "%s: gms_rollout.mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE", who);
    return GMS_OK;
}

// P start poses (or the shown particle's own: start.n_per > 0, P = 1) roll K arcs in ONE map's blocked plane: records into d_out [P][K], or
// -- d_risk -- the counts over the poses into d_risk [K]
static int rollout_launch(gms_map *m, const uint32_t *d_blocked, const gms_rollout *r, const RollStart &start, int32_t P, const gms_rollout_step *d_arcs, int32_t K,
                          int32_t T, const float *d_points, int32_t F, const uint16_t *d_clear, const uint16_t *d_cost, gms_rollout_rec *d_out,
                          gms_rollout_risk *d_risk) {
    const int32_t cpw = m->rollout_cpw, R = r->max_range, wpr = gms_plane_wpr(m);
    const bool mem = m->rollout_walk_mem != 0;
    const size_t lds = mem ? 0 : (size_t)roll_win_words(R) * sizeof(uint32_t);
    const dim3 grid((unsigned)P, (unsigned)((K + cpw - 1) / cpw));
    if (d_risk) {
        hipLaunchKernelGGL(k_rollout_risk_init, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, m->stream, d_risk, K, T);
        if (mem)
            hipLaunchKernelGGL((k_rollout<true, true>), grid, dim3(ROLL_NT), lds, m->stream, m->gd, d_blocked, wpr, start, d_arcs, K, T, d_points, F, R, cpw, d_clear,
                               d_cost, d_out, d_risk);
        else
            hipLaunchKernelGGL((k_rollout<true, false>), grid, dim3(ROLL_NT), lds, m->stream, m->gd, d_blocked, wpr, start, d_arcs, K, T, d_points, F, R, cpw, d_clear,
                               d_cost, d_out, d_risk);
    } else if (mem) {
        hipLaunchKernelGGL((k_rollout<false, true>), grid, dim3(ROLL_NT), lds, m->stream, m->gd, d_blocked, wpr, start, d_arcs, K, T, d_points, F, R, cpw, d_clear,
                           d_cost, d_out, d_risk);
    } else {
        hipLaunchKernelGGL((k_rollout<false, false>), grid, dim3(ROLL_NT), lds, m->stream, m->gd, d_blocked, wpr, start, d_arcs, K, T, d_points, F, R, cpw, d_clear,
                           d_cost, d_out, d_risk);
    }
    HIPCHK(hipGetLastError());
    return GMS_OK;
}

// the rollouts of P poses in one map of a shared handle, or of P poses (P == 0 and no poses: its own) in the shown particle's map of a
// per-particle one; `shown` exists for a particle only
static int rollout(QuerySource src, const char *what, const gms_rollout *r, const float *poses, int32_t P, const gms_rollout_step *arcs, int32_t K, int32_t T,
                   const float *points, int32_t F, const uint16_t *clear, const uint16_t *cost, gms_rollout_rec *out, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !r || !arcs || !out || (F > 0 && !points) || (!src.s && !poses))
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the arcs, the output, the points of F > 0 and -- for a map -- the poses are required)",
                        what);
    gms_map *m = src.m;
    int rc = rollout_check(r, K, T, F, what);
    if (rc) return rc;
    const bool own = src.s && P == 0 && !poses;
    if (!own && (!poses || P < 1 || P > GMS_MAX_PARTICLES))
        return gms_fail(GMS_ERR_INVALID, "%s: 1 <= P <= GMS_MAX_PARTICLES poses%s", what, src.s ? ", or P = 0 and no poses (the shown particle's own pose)" : "");
    if (on_device && ((((uintptr_t)out | (uintptr_t)arcs) & 15) != 0 || (((uintptr_t)poses | (uintptr_t)points) & 3) != 0 || (((uintptr_t)clear | (uintptr_t)cost) & 1) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the arcs and the output must be 16-byte aligned, the poses and points 4-byte, the fields 2-byte", what);
    src.filter = r->filter;
    rc = query_check(src, what, "gms_rollout.filter");                          // the map's index, or the shown particle
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    const int32_t n_poses = own ? 1 : P;
    HostStage st(m, on_device);
    const size_t cells = (size_t)m->gd.cells, out_bytes = (size_t)n_poses * (size_t)K * sizeof(gms_rollout_rec), arc_bytes = (size_t)K * (size_t)T * sizeof(gms_rollout_step);
    const size_t point_bytes = (size_t)F * 2 * sizeof(float), pose_bytes = own ? 0 : (size_t)P * 3 * sizeof(float);
    const size_t clear_bytes = clear ? cells * sizeof(uint16_t) : 0, cost_bytes = cost ? cells * sizeof(uint16_t) : 0;
    const size_t p_out = st.part(out_bytes), p_arcs = st.part(arc_bytes), p_points = st.part(point_bytes), p_poses = st.part(pose_bytes);
    const size_t p_clear = st.part(clear_bytes), p_cost = st.part(cost_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_arcs, arcs, arc_bytes);
    if (!rc && F > 0) rc = st.up(p_points, points, point_bytes);
    if (!rc && !own) rc = st.up(p_poses, poses, pose_bytes);
    if (!rc && clear) rc = st.up(p_clear, clear, clear_bytes);
    if (!rc && cost) rc = st.up(p_cost, cost, cost_bytes);
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(src, r->mode, st.shown(shown), nullptr, &plane);
    if (!rc && r->inflate > 0) rc = gms_reach_inflate(m, plane, r->inflate, r->mode, &plane);
    if (rc) return rc;
    RollStart start = {own ? src.s->pf->d_pose : st.at(p_poses, poses), nullptr, 0, 0, 0};
    if (own) start = {src.s->pf->d_pose, src.s->pf->d_stats, src.index, src.filter, src.s->n_per};
    rc = rollout_launch(m, plane, r, start, n_poses, st.at(p_arcs, arcs), K, T, F > 0 ? st.at(p_points, points) : nullptr, F, clear ? st.at(p_clear, clear) : nullptr,
                        cost ? st.at(p_cost, cost) : nullptr, st.at(p_out, out), nullptr);
    if (rc) return rc;
    st.fetch(out, p_out, out_bytes);
    return st.finish(shown);
}

static int pf_rollout(gms_pf *pf, const gms_rollout *r, const gms_rollout_step *arcs, int32_t K, int32_t T, const float *points, int32_t F, gms_rollout_risk *out,
                      bool on_device) {
    const char *who = on_device ? "gms_pf_rollout_dev" : "gms_pf_rollout";
    if (!pf || !r || !arcs || !out || (F > 0 && !points))
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the filter, the request, the arcs, the output and the points of F > 0 are required)", who);
    int rc = rollout_check(r, K, T, F, who);
    if (rc) return rc;
    if (pf->slam_owned) return gms_fail(GMS_ERR_STATE, "%s: this filter's particles own maps (gms_slam): there is no one map to roll out in", who);
    if (on_device && ((((uintptr_t)out | (uintptr_t)arcs) & 15) != 0 || ((uintptr_t)points & 3) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the arcs and the output must be 16-byte aligned, the points 4-byte", who);
    gms_map *m = pf->map;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t out_bytes = (size_t)pf->n_maps * (size_t)K * sizeof(gms_rollout_risk), arc_bytes = (size_t)K * (size_t)T * sizeof(gms_rollout_step);
    const size_t point_bytes = (size_t)F * 2 * sizeof(float);
    const size_t p_out = st.part(out_bytes), p_arcs = st.part(arc_bytes), p_points = st.part(point_bytes);
    rc = st.open();
    if (!rc) rc = st.up(p_arcs, arcs, arc_bytes);
    if (!rc && F > 0) rc = st.up(p_points, points, point_bytes);
    if (rc) return rc;
    for (int32_t mi = 0; mi < pf->n_maps; mi++) {                               // map mi's particles in map mi (a batched handle's inflated plane: one scratch, in stream order)
        const uint32_t *plane = nullptr;
        rc = query_plane(query_map(m, mi), r->mode, nullptr, nullptr, &plane);
        if (!rc && r->inflate > 0) rc = gms_reach_inflate(m, plane, r->inflate, r->mode, &plane);
        if (rc) return rc;
        const RollStart start = {pf->d_pose + (size_t)mi * (size_t)pf->n * 3, nullptr, 0, 0, 0};
        rc = rollout_launch(m, plane, r, start, pf->n, st.at(p_arcs, arcs), K, T, F > 0 ? st.at(p_points, points) : nullptr, F, nullptr, nullptr, nullptr,
                            st.at(p_out, out) + (size_t)mi * (size_t)K);
        if (rc) return rc;
    }
    st.fetch(out, p_out, out_bytes);
    return st.finish(nullptr);
}

extern "C" {

int gms_rollout_check(const gms_rollout *r, int32_t K, int32_t T, int32_t F) { return rollout_check(r, K, T, F, "gms_rollout"); }

int gms_rollout_candidates_per_workgroup(void) { return GMS_ROLLOUT_CANDIDATES; }

int gms_rollout_arcs(const double *v, const double *omega, int32_t K, double dt, int32_t T, gms_rollout_step *out) {
    REQUIRE(v && omega && out, "gms_rollout_arcs: null argument");
    REQUIRE(K >= 1 && K <= GMS_ROLLOUT_MAX_K, "gms_rollout_arcs: 1 <= K <= GMS_ROLLOUT_MAX_K candidates");
    REQUIRE(T >= 1 && T <= GMS_ROLLOUT_MAX_T, "gms_rollout_arcs: 1 <= T <= GMS_ROLLOUT_MAX_T steps");
    REQUIRE(dt > 0.0 && dt < INFINITY, "gms_rollout_arcs: dt must be finite and > 0");
    for (int32_t k = 0; k < K; k++)
        for (int32_t j = 0; j < T; j++) {
            const double time = (double)(j + 1) * dt, th = omega[k] * time;
            gms_rollout_step s;
            if (fabs(omega[k]) < 1e-9) {                                        // the straight line: the arc's limit
                s.dx = (float)(v[k] * time);
                s.dy = 0.0f;
            } else {
                const double rad = v[k] / omega[k];
                s.dx = (float)(rad * sin(th));
                s.dy = (float)(rad * (1.0 - cos(th)));
            }
            s.c = (float)cos(th);
            s.s = (float)sin(th);
            out[(size_t)k * (size_t)T + (size_t)j] = s;
        }
    return GMS_OK;
}

int gms_map_rollout(gms_map *m, int32_t mi, const gms_rollout *r, const float *poses, int32_t P, const gms_rollout_step *arcs, int32_t K, int32_t T,
                    const float *points, int32_t F, const uint16_t *clear, const uint16_t *cost, gms_rollout_rec *out) {
    return rollout(query_map(m, mi), "gms_map_rollout", r, poses, P, arcs, K, T, points, F, clear, cost, out, nullptr, false);
}
int gms_map_rollout_dev(gms_map *m, int32_t mi, const gms_rollout *r, const float *dev_poses, int32_t P, const gms_rollout_step *dev_arcs, int32_t K, int32_t T,
                        const float *dev_points, int32_t F, const uint16_t *dev_clear, const uint16_t *dev_cost, gms_rollout_rec *dev_out) {
    return rollout(query_map(m, mi), "gms_map_rollout_dev", r, dev_poses, P, dev_arcs, K, T, dev_points, F, dev_clear, dev_cost, dev_out, nullptr, true);
}
int gms_slam_rollout(gms_slam *s, int32_t which, const gms_rollout *r, const float *poses, int32_t P, const gms_rollout_step *arcs, int32_t K, int32_t T,
                     const float *points, int32_t F, const uint16_t *clear, const uint16_t *cost, gms_rollout_rec *out, int32_t *shown) {
    return rollout(query_slam(s, which), "gms_slam_rollout", r, poses, P, arcs, K, T, points, F, clear, cost, out, shown, false);
}
int gms_slam_rollout_dev(gms_slam *s, int32_t which, const gms_rollout *r, const float *dev_poses, int32_t P, const gms_rollout_step *dev_arcs, int32_t K, int32_t T,
                         const float *dev_points, int32_t F, const uint16_t *dev_clear, const uint16_t *dev_cost, gms_rollout_rec *dev_out, int32_t *dev_shown) {
    return rollout(query_slam(s, which), "gms_slam_rollout_dev", r, dev_poses, P, dev_arcs, K, T, dev_points, F, dev_clear, dev_cost, dev_out, dev_shown, true);
}
int gms_pf_rollout(gms_pf *pf, const gms_rollout *r, const gms_rollout_step *arcs, int32_t K, int32_t T, const float *points, int32_t F, gms_rollout_risk *out) {
    return pf_rollout(pf, r, arcs, K, T, points, F, out, false);
}
int gms_pf_rollout_dev(gms_pf *pf, const gms_rollout *r, const gms_rollout_step *dev_arcs, int32_t K, int32_t T, const float *dev_points, int32_t F,
                       gms_rollout_risk *dev_out) {
    return pf_rollout(pf, r, dev_arcs, K, T, dev_points, F, dev_out, true);
}

}  // extern "C"
