// gms_clearance.hip -- clearance fields (gridmapslam.h "clearance fields"): the squared distance, in cells, from every cell of a rectangle
// to the nearest obstacle cell of the whole map, capped at max_radius.  All integer arithmetic.
//
// A translation unit of its own, kernels and C-ABI: nothing here is on the scan step's path, and no kernel of the other units is
// compiled differently for it.
//
//   the planes       one bit per cell, rows of gms_plane_wpr 32-bit words (padded to 64 cells, the padding zero): the map's plane of the
//                    request's mode, or the shown particle's, packed per request (query_plane, gms_query.hip).
//   k_clear_field    the separable nearest-obstacle transform (gms_nearest_device.h: the stages, the tile, the LDS) keeping the DISTANCE
//                    alone: g = the horizontal distance to the nearest set bit of the row as uint16, 0xFFFF beyond R, per staged cell;
//                    the minimum over dy of g(x, y + dy)^2 + dy^2, left once dy^2 >= the best so far.
//   k_clear_poses    the same rows under a wavefront per pose, wave_min(uint32_t) takes the minimum.  No field is made.
#undef GMS_STAMPS
#include <stdlib.h>
#include <string.h>

#include "gms_nearest_device.h"

constexpr auto k_clear_field = k_nearest_field<KeepDistance>;
constexpr auto k_clear_poses = k_nearest_poses<KeepDistance>;

// ---- host ----------------------------------------------------------------------------------------------------------------------
// the field of rectangle c of ONE map's plane into d_out
int gms_clear_launch(gms_map *m, const uint32_t *d_plane, const gms_clearance *c, uint16_t *d_out) {
    return nearest_launch<k_clear_field>(m, d_plane, c->x0, c->y0, c->w, c->h, c->max_radius, d_out, "gms_clearance");
}

// the field of one map of a shared handle or of the shown particle of a per-particle one; `shown` exists for a particle only
static int clearance(QuerySource src, const char *what, const gms_clearance *c, uint16_t *out, int32_t *shown, bool on_device) {
    if ((!src.m && !src.s) || !c || !out) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the handle, the request and the output are required)", what);
    gms_map *m = src.m;
    int64_t bytes = 0;
    int rc = src.s ? GMS_OK : query_check(src, what, nullptr);                  // (a map's index: ahead of the request, the shown particle behind it)
    if (!rc) rc = gms_clearance_size(c, nullptr, nullptr, &bytes);
    if (!rc) rc = gms_rect_check(c->x0, c->y0, c->w, c->h, m->gd.W, m->gd.H, what);
    if (rc) return rc;
    if (on_device && ((uintptr_t)out & 1) != 0) return gms_fail(GMS_ERR_INVALID, "%s_dev: the output must be 2-byte aligned", what);
    src.filter = c->filter;
    if (src.s && (rc = query_check(src, what, "gms_clearance.filter")) != 0) return rc;
    HIPCHK(hipSetDevice(m->device));
    HostStage st(m, on_device);
    const size_t p_out = st.part((size_t)bytes);
    rc = st.open();
    if (rc) return rc;
    const uint32_t *plane = nullptr;
    rc = query_plane(src, c->mode, st.shown(shown), nullptr, &plane);
    if (!rc) rc = gms_clear_launch(m, plane, c, st.at(p_out, out));
    if (rc) return rc;
    st.fetch(out, p_out, (size_t)bytes);
    return st.finish(shown);
}

extern "C" {

int gms_clearance_size(const gms_clearance *c, int32_t *out_w, int32_t *out_h, int64_t *bytes) {
    REQUIRE(c, "gms_clearance: null request");
    const int rc = nearest_request_check(c->x0, c->y0, c->w, c->h, c->max_radius, c->mode, "gms_clearance");
    if (rc) return rc;
    if (out_w) *out_w = c->w;
    if (out_h) *out_h = c->h;
    if (bytes) *bytes = (int64_t)c->w * c->h * (int64_t)sizeof(uint16_t);
    return GMS_OK;
}
int gms_map_clearance(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *out) { return clearance(query_map(m, mi), "gms_map_clearance", c, out, nullptr, false); }
int gms_map_clearance_dev(gms_map *m, int32_t mi, const gms_clearance *c, uint16_t *dev_out) { return clearance(query_map(m, mi), "gms_map_clearance", c, dev_out, nullptr, true); }
int gms_map_clearance_poses(gms_map *m, int32_t mi, const float *poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *out) {
    return nearest_poses<k_clear_poses>(m, mi, poses, P, max_radius, mode, out, false, "gms_map_clearance_poses", nullptr);
}
int gms_map_clearance_poses_dev(gms_map *m, int32_t mi, const float *dev_poses, int32_t P, int32_t max_radius, int32_t mode, uint16_t *dev_out) {
    return nearest_poses<k_clear_poses>(m, mi, dev_poses, P, max_radius, mode, dev_out, true, "gms_map_clearance_poses", nullptr);
}
int gms_slam_clearance(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *out, int32_t *shown) {
    return clearance(query_slam(s, which), "gms_slam_clearance", c, out, shown, false);
}
int gms_slam_clearance_dev(gms_slam *s, int32_t which, const gms_clearance *c, uint16_t *dev_out, int32_t *dev_shown) {
    return clearance(query_slam(s, which), "gms_slam_clearance", c, dev_out, dev_shown, true);
}

}  // extern "C"
