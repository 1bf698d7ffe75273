// gms_route.hip -- routes (gridmapslam.h "routes"): for P start cells over a whole-map cost-to-go field, the cheapest 8-connected path
// down to a seed and that path pulled taut to waypoints by line of sight through the cost-to-go fields' blocked plane.
//
// A translation unit of its own, kernel and C-ABI, layered on the query base and on reach's blocked plane (gms_reach_inflate) as
// gms_rollout.hip is: nothing here is on the scan step's path, and no kernel of the other units is compiled differently for it.
//
//   k_route            one wavefront per start, four per workgroup of 256 lanes; no barrier, no workgroup waits on another.
//     the descent      a chain of dependent loads, one round trip per step: lane k < 8 loads the k-th neighbour of the current cell in
//                      the definition's order E, N, W, S, NE, NW, SW, SE, lane 8 the cell itself (off the map reads as FAR); a diagonal
//                      lane takes its two side cells from the axis lanes by cross-lane moves; the ballot's lowest bit is the next
//                      cell.  Lane n & 63 keeps cell n and the wavefront stores 64 cells at a time, off the chain.  At most
//                      min(max_cells, 13107) steps: the cost falls by at least 5 per step whatever the field holds, and a cell is
//                      entered only after it was found on the map, so no load leaves the field.
//     the clearance    one pass over the stored path, 64 cells at a time; the key d2 << 16 | index (index < 2^14) takes the smallest
//                      index among equal minima.
//     the pull         lanes own candidates: from path[i] lane l of pass p tests j = min(i + look, n - 1) - 64 p - l, walking the
//                      supercover of (path[i], path[j]) along its major axis from path[i] -- per column the cells v with
//                      2 |t * minor - v * major| <= major + minor, at most three, found by advancing a lower bound, no division --
//                      and leaves at its first blocked cell.  The ballot's lowest bit is the largest visible j; a pass without one
//                      goes on to the next 64.  Every cell walked lies in the bounding box of two path cells, so on the map.  At
//                      most ceil(look / 64) passes per waypoint and look + 1 columns per lane.
#undef GMS_STAMPS
#include "gms_device.h"

#define ROUTE_NT 256
#define ROUTE_WAVES (ROUTE_NT / 64)

static_assert(sizeof(gms_route_rec) == 32, "gms_route_rec is two 16-byte stores");
static_assert(sizeof(gms_route) == 24, "the header's size");
static_assert(GMS_ROUTE_MAX_CELLS <= (1 << 14), "the clearance key holds a path index in 14 bits beside 16 of d2");
static_assert((int64_t)GMS_ROUTE_MAX_LOOK * GMS_ROUTE_MAX_LOOK * 4 < (1ll << 31), "the supercover's products are formed in 32 bits");
static_assert(0xFFFE / GMS_REACH_AXIS + 1 <= GMS_ROUTE_MAX_CELLS, "max_cells can hold any descent");

// whose cells a launch starts from: cell blockIdx-th of `starts`, or -- n_per > 0, a gms_slam without starts -- the shown particle's own
struct RouteStart {
    const int32_t *starts;
    const float *poses;
    const PfStatsDev *stats;
    int32_t which, filter, n_per;
};

// lane k's offset from the current cell, as (d + 1) in two bits per lane: E, N, W, S, NE, NW, SW, SE, the cell itself
#define ROUTE_DX_CODES (2u | 1u << 2 | 0u << 4 | 1u << 6 | 2u << 8 | 0u << 10 | 0u << 12 | 2u << 14 | 1u << 16)
#define ROUTE_DY_CODES (1u | 2u << 2 | 1u << 4 | 0u << 6 | 2u << 8 | 2u << 10 | 0u << 12 | 0u << 14 | 1u << 16)
__device__ __forceinline__ int32_t route_dx(int32_t k) { return (int32_t)((ROUTE_DX_CODES >> (2 * k)) & 3u) - 1; }
__device__ __forceinline__ int32_t route_dy(int32_t k) { return (int32_t)((ROUTE_DY_CODES >> (2 * k)) & 3u) - 1; }

__device__ __forceinline__ bool route_blocked(const uint32_t *__restrict__ plane, int32_t wpr, int32_t x, int32_t y) {
    return (plane[(size_t)y * (size_t)wpr + (size_t)(x >> 5)] >> (x & 31)) & 1u;
}

// VISIBLE(a, b) for two cells on the map at most GMS_ROUTE_MAX_LOOK apart per axis
__device__ __forceinline__ bool route_visible(const uint32_t *__restrict__ plane, int32_t wpr, int32_t ax, int32_t ay, int32_t bx, int32_t by) {
    const int32_t dx = bx - ax, dy = by - ay, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const int32_t sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
    const bool xmajor = adx >= ady;
    const int32_t am = xmajor ? adx : ady, an = xmajor ? ady : adx, half = am + an;
    int32_t lo = 0;                                                             // the first minor offset of column t that is not below the band
    for (int32_t t = 0; t <= am; t++) {
        const int32_t c = t * an;
        while (2 * (c - lo * am) > half) lo++;                                  // (never past an: cell (t, round(t an / am)) is in the band)
        for (int32_t v = lo; v <= an && 2 * (v * am - c) <= half; v++) {
            const int32_t x = ax + sx * (xmajor ? t : v), y = ay + sy * (xmajor ? v : t);
            if (route_blocked(plane, wpr, x, y)) return false;
        }
    }
    return true;
}

// plane: ONE map's blocked plane; cost, clear: [H][W] (clear may be NULL); out [gridDim.x * ROUTE_WAVES >= P]; waypoints [P][max_wp][2];
// path [P][max_cells][2]: the caller's cells or the handle's scratch
__global__ void __launch_bounds__(ROUTE_NT)
k_route(GridDev g, const uint32_t *__restrict__ plane, int32_t wpr, RouteStart start, int32_t P, const uint16_t *__restrict__ cost,
        const uint16_t *__restrict__ clear, int32_t max_cells, int32_t max_wp, int32_t look, gms_route_rec *__restrict__ out, int32_t *__restrict__ waypoints,
        int32_t *__restrict__ path_all) {
    const int32_t lane = (int32_t)(threadIdx.x & 63), pi = (int32_t)blockIdx.x * ROUTE_WAVES + (int32_t)(threadIdx.x >> 6);
    if (pi >= P) return;                                                        // (uniform per wavefront; no barrier follows)
    int32_t cx, cy;
    if (start.n_per > 0) {
        const int32_t p = start.which >= 0 ? start.which : start.filter * start.n_per + start.stats[start.filter].strongest;
        cx = j_cell_exact((double)start.poses[3 * (size_t)p] - g.posx, g.res);                  // GridMap.java:273
        cy = j_cell_exact((double)start.poses[3 * (size_t)p + 1] - g.posy, g.res);              // :274
    } else {
        cx = start.starts[2 * (size_t)pi];
        cy = start.starts[2 * (size_t)pi + 1];
    }
    int2 *__restrict__ path = reinterpret_cast<int2 *>(path_all) + (size_t)pi * (size_t)max_cells;
    int2 *__restrict__ wp = reinterpret_cast<int2 *>(waypoints) + (size_t)pi * (size_t)max_wp;
    const uint32_t FAR = GMS_REACH_FAR;
    const int32_t kx = route_dx(min(lane, 8)), ky = route_dy(min(lane, 8));     // lanes 9 .. 63 idle on the cell itself
    const bool diag = lane >= 4 && lane < 8;
    const uint32_t step = diag ? GMS_REACH_DIAG : GMS_REACH_AXIS;
    const int32_t side_a = kx > 0 ? 0 : 2, side_b = ky > 0 ? 1 : 3;            // a diagonal's side cells: E or W, N or S

    // ---- the descent ----
    uint32_t flags = 0u, start_cost = FAR, end_cost = FAR;
    int32_t n = 0, keep_x = 0, keep_y = 0;
    const int32_t sx0 = cx, sy0 = cy;
    if (cx < 0 || cy < 0 || cx >= g.W || cy >= g.H) {
        flags = GMS_ROUTE_NO_PATH;
    } else {
        for (;;) {                                                              // (cx, cy) is on the map
            const int32_t nx = cx + kx, ny = cy + ky;
            uint32_t v = FAR;
            if (lane < 9 && nx >= 0 && ny >= 0 && nx < g.W && ny < g.H) v = cost[(size_t)ny * (size_t)g.W + (size_t)nx];
            const uint32_t cur = (uint32_t)__shfl((int)v, 8);
            const uint32_t sa = (uint32_t)__shfl((int)v, side_a), sb = (uint32_t)__shfl((int)v, side_b);
            if (n == 0) {
                start_cost = cur;
                if (cur == FAR) { flags = GMS_ROUTE_NO_PATH; break; }
            }
            if (lane == (n & 63)) { keep_x = cx; keep_y = cy; }
            n++;
            if ((n & 63) == 0) path[n - 64 + lane] = make_int2(keep_x, keep_y);
            end_cost = cur;
            if (cur == 0u) break;
            const bool ok = lane < 8 && v != FAR && v + step == cur && (!diag || (sa != FAR && sb != FAR));
            const uint64_t oks = __ballot(ok);
            if (!oks) { flags |= GMS_ROUTE_BROKEN; break; }
            if (n == max_cells) { flags |= GMS_ROUTE_CELLS_CUT; break; }
            const int32_t k = __ffsll((unsigned long long)oks) - 1;
            cx += route_dx(k);
            cy += route_dy(k);
        }
        if (lane < (n & 63)) path[(n & ~63) + lane] = make_int2(keep_x, keep_y);
    }
    __threadfence_block();                                                      // the cells the other lanes stored, before this lane reads them

    // ---- the clearance along the path ----
    uint32_t key = 0xffffffffu;
    if (clear)
        for (int32_t base = 0; base < n; base += 64) {
            const int32_t i = base + lane;
            if (i < n) {
                const int2 c = path[i];
                key = min(key, ((uint32_t)clear[(size_t)c.y * (size_t)g.W + (size_t)c.x] << 16) | (uint32_t)i);
            }
        }
#define GMS_STEP_(O) key = min(key, wave_xor<O>(key));
    GMS_BUTTERFLY(GMS_STEP_)
#undef GMS_STEP_
    const bool have_min = clear && n > 0;
    const uint32_t min_d2 = have_min ? key >> 16 : (uint32_t)GMS_CLEAR_FAR, min_at = have_min ? key & 0xffffu : 0u;

    // ---- the pull ----
    int32_t nw = 0;
    if (n > 0) {
        int32_t i = 0, ax = sx0, ay = sy0;
        if (lane == 0) wp[0] = make_int2(ax, ay);
        nw = 1;
        while (i < n - 1) {
            if (nw == max_wp) { flags |= GMS_ROUTE_WAYPOINTS_CUT; break; }
            const int32_t hi = min(i + look, n - 1);
            int32_t j = -1, jx = 0, jy = 0;
            for (int32_t top = hi; top > i && j < 0; top -= 64) {
                const int32_t mine = top - lane;
                bool vis = false;
                int2 b = make_int2(0, 0);
                if (mine > i) {
                    b = path[mine];
                    vis = route_visible(plane, wpr, ax, ay, b.x, b.y);
                }
                const uint64_t seen = __ballot(vis);
                if (seen) {
                    const int32_t l = __ffsll((unsigned long long)seen) - 1;
                    j = top - l;
                    jx = __shfl(b.x, l);
                    jy = __shfl(b.y, l);
                }
            }
            if (j < 0) {
                flags |= GMS_ROUTE_MISMATCH;
                j = i + 1;
                const int2 b = path[j];
                jx = b.x; jy = b.y;
            }
            if (lane == 0) wp[nw] = make_int2(jx, jy);
            nw++;
            i = j; ax = jx; ay = jy;
        }
    }
    if (lane == 0) {
        int4 *dst = reinterpret_cast<int4 *>(out + pi);
        dst[0] = make_int4(n, nw, (int32_t)(start_cost | (end_cost << 16)), (int32_t)(min_d2 | (flags << 16)));
        dst[1] = make_int4((int32_t)min_at, cx, cy, 0);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int route_check(const gms_route *r, const char *who) {
    if (!r) return gms_fail(GMS_ERR_INVALID, "%s: null request", who);
    if (r->max_cells < 1 || r->max_cells > GMS_ROUTE_MAX_CELLS) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= gms_route.max_cells <= GMS_ROUTE_MAX_CELLS", who);
    if (r->max_waypoints < 1 || r->max_waypoints > r->max_cells) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= gms_route.max_waypoints <= max_cells", who);
    if (r->look < 1 || r->look > GMS_ROUTE_MAX_LOOK) return gms_fail(GMS_ERR_INVALID, "%s: 1 <= gms_route.look <= GMS_ROUTE_MAX_LOOK path indices", who);
    if (r->inflate < 0 || r->inflate > 255) return gms_fail(GMS_ERR_INVALID, "%s: 0 <= gms_route.inflate <= 255 cells", who);
    if (r->mode != GMS_CLEAR_OCCUPIED && r->mode != GMS_CLEAR_NOT_FREE)
        return gms_fail(GMS_ERR_INVALID, "%s: gms_route.mode must be GMS_CLEAR_OCCUPIED or GMS_CLEAR_NOT_FREE", who);
    return GMS_OK;
}

// the routes of P starts in one map of a shared handle, or of P starts (P == 0 and no starts: its own cell) in the shown particle's map of
// a per-particle one; `shown` exists for a particle only
static int route(QuerySource src, const char *what, const gms_route *r, const int32_t *starts, int32_t P, const uint16_t *cost, const uint16_t *clear,
                 gms_route_rec *out, int32_t *waypoints, int32_t *cells, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !r || !cost || !out || !waypoints || (!src.s && !starts))
        return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request, the cost-to-go field, the records, the waypoints and -- for a map -- the starts are required)",
                        what);
    gms_map *m = src.m;
    int rc = route_check(r, what);
    if (rc) return rc;
    const bool own = src.s && P == 0 && !starts;
    if (!own && (!starts || P < 1 || P > GMS_ROUTE_MAX_P))
        return gms_fail(GMS_ERR_INVALID, "%s: 1 <= P <= GMS_ROUTE_MAX_P starts%s", what, src.s ? ", or P = 0 and no starts (the shown particle's own cell)" : "");
    if (on_device && (((uintptr_t)out & 15) != 0 || (((uintptr_t)waypoints | (uintptr_t)cells) & 7) != 0 || ((uintptr_t)starts & 3) != 0 ||
                      (((uintptr_t)clear | (uintptr_t)cost) & 1) != 0))
        return gms_fail(GMS_ERR_INVALID, "%s: the records must be 16-byte aligned, the waypoints and cells 8-byte, the starts 4-byte, the fields 2-byte", what);
    src.filter = r->filter;
    rc = query_check(src, what, "gms_route.filter");                            // the map's index, or the shown particle
    if (rc) return rc;
    HIPCHK(hipSetDevice(m->device));
    const int32_t n_starts = own ? 1 : P;
    if (!cells) {
        rc = gms_dev_grow(&m->d_route_path, &m->route_cap, (int64_t)n_starts * r->max_cells, 65536, &m->stream, [](size_t c) { return c * 2 * sizeof(int32_t); }, what,
                          "the descended paths");
        if (rc) return rc;
    }
    HostStage st(m, on_device);
    const size_t field_bytes = (size_t)m->gd.cells * sizeof(uint16_t), out_bytes = (size_t)n_starts * sizeof(gms_route_rec);
    const size_t wp_bytes = (size_t)n_starts * (size_t)r->max_waypoints * 2 * sizeof(int32_t);
    const size_t cell_bytes = cells ? (size_t)n_starts * (size_t)r->max_cells * 2 * sizeof(int32_t) : 0, start_bytes = own ? 0 : (size_t)P * 2 * sizeof(int32_t);
    const size_t p_out = st.part(out_bytes), p_wp = st.part(wp_bytes), p_cells = st.part(cell_bytes), p_starts = st.part(start_bytes);
    const size_t p_cost = st.part(field_bytes), p_clear = st.part(clear ? field_bytes : 0);
    rc = st.open();
    if (!rc && !own) rc = st.up(p_starts, starts, start_bytes);
    if (!rc) rc = st.up(p_cost, cost, field_bytes);
    if (!rc && clear) rc = st.up(p_clear, clear, field_bytes);
    if (!rc) rc = st.up(p_wp, waypoints, wp_bytes);                             // what lies behind the counts comes back as it went
    if (!rc && cells) rc = st.up(p_cells, cells, cell_bytes);
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(src, r->mode, st.shown(shown), nullptr, &plane);
    if (!rc && r->inflate > 0) rc = gms_reach_inflate(m, plane, r->inflate, r->mode, &plane);
    if (rc) return rc;
    RouteStart start = {own ? nullptr : st.at(p_starts, starts), nullptr, nullptr, 0, 0, 0};
    if (own) start = {nullptr, src.s->pf->d_pose, src.s->pf->d_stats, src.index, src.filter, src.s->n_per};
    hipLaunchKernelGGL(k_route, dim3((unsigned)((n_starts + ROUTE_WAVES - 1) / ROUTE_WAVES)), dim3(ROUTE_NT), 0, m->stream, m->gd, plane, gms_plane_wpr(m), start, n_starts,
                       st.at(p_cost, cost), clear ? st.at(p_clear, clear) : nullptr, r->max_cells, r->max_waypoints, r->look, st.at(p_out, out), st.at(p_wp, waypoints),
                       cells ? st.at(p_cells, cells) : m->d_route_path);
    HIPCHK(hipGetLastError());
    st.fetch(out, p_out, out_bytes);
    st.fetch(waypoints, p_wp, wp_bytes);
    if (cells) st.fetch(cells, p_cells, cell_bytes);
    return st.finish(shown);
}

extern "C" {

int gms_route_check(const gms_route *r) { return route_check(r, "gms_route"); }

int gms_map_route(gms_map *m, int32_t mi, const gms_route *r, const int32_t *starts, int32_t P, const uint16_t *cost, const uint16_t *clear, gms_route_rec *out,
                  int32_t *waypoints, int32_t *cells) {
    return route(query_map(m, mi), "gms_map_route", r, starts, P, cost, clear, out, waypoints, cells, nullptr, false);
}
int gms_map_route_dev(gms_map *m, int32_t mi, const gms_route *r, const int32_t *dev_starts, int32_t P, const uint16_t *dev_cost, const uint16_t *dev_clear,
                      gms_route_rec *dev_out, int32_t *dev_waypoints, int32_t *dev_cells) {
    return route(query_map(m, mi), "gms_map_route_dev", r, dev_starts, P, dev_cost, dev_clear, dev_out, dev_waypoints, dev_cells, nullptr, true);
}
int gms_slam_route(gms_slam *s, int32_t which, const gms_route *r, const int32_t *starts, int32_t P, const uint16_t *cost, const uint16_t *clear, gms_route_rec *out,
                   int32_t *waypoints, int32_t *cells, int32_t *shown) {
    return route(query_slam(s, which), "gms_slam_route", r, starts, P, cost, clear, out, waypoints, cells, shown, false);
}
int gms_slam_route_dev(gms_slam *s, int32_t which, const gms_route *r, const int32_t *dev_starts, int32_t P, const uint16_t *dev_cost, const uint16_t *dev_clear,
                       gms_route_rec *dev_out, int32_t *dev_waypoints, int32_t *dev_cells, int32_t *dev_shown) {
    return route(query_slam(s, which), "gms_slam_route_dev", r, dev_starts, P, dev_cost, dev_clear, dev_out, dev_waypoints, dev_cells, dev_shown, true);
}

}  // extern "C"
