// gridmapslam.hpp -- C++ host-side mirror of the reference's Java class surface over the C-ABI of
// include/gridmapslam.h.  Header-only, C++17; link with -lgridmapslam (and the HIP runtime it needs).
//
// The reference is compiled Java and no JVM exists in this image, so the host side above the C-ABI is
// written in C++ with the reference's names, argument meaning and error behaviour
// (J/ = java/GridMapGL/src/main/java/com/fmsz/gridmapgl/ in the reference tree):
//
//   gms::Pose             J/slam/Pose.java:21-35
//   gms::Observation      J/slam/Observation.java:29-106   (Measurement = gms_beam)
//   gms::GridMap          J/slam/GridMap.java:47-432       (one object = GridMap + its GridMapData)
//   gms::ParticleFilter   J/slam/ParticleFilter.java:19-84 (resample semantics of SLAM.resample)
//   gms::SLAM             J/slam/SLAM.java:26-204          (one shared map, N poses: SURVEY.md fact 3)
//   gms::SlamParticleMaps J/slam/SLAM.java:26-204          (the reference's own shape: every Particle owns a GridMapData)
//
// Java signals nothing on this path except ArrayIndexOutOfBounds from getRawAt; here every failing
// C-ABI call throws gms::Error carrying gms_last_error().
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <array>
#include <vector>

#include "gridmapslam.h"

namespace gms {

struct Error : std::runtime_error {
    int code;
    Error(int c, const char *msg) : std::runtime_error(std::string("libgridmapslam: ") + msg), code(c) {}
};

inline void check(int rc) {
    if (rc != GMS_OK) throw Error(rc, gms_last_error());
}

/** Pose{float x, y, theta} (J/slam/Pose.java:21-35) */
struct Pose {
    float x = 0, y = 0, theta = 0;
    Pose() = default;
    Pose(float x_, float y_, float theta_) : x(x_), y(y_), theta(theta_) {}
};

/** One LIDAR revolution (J/slam/Observation.java) */
class Observation {
public:
    using Measurement = gms_beam;

    /** addMeasurement(angle, distance, wasHit): localX = distance * cos(angle) (Observation.java:44-51,87-89) */
    void addMeasurement(float angle, float distance, bool wasHit) {
        Measurement m{};
        m.distance = (double)distance;
        m.local_x = (double)distance * std::cos((double)angle);
        m.local_y = (double)distance * std::sin((double)angle);
        m.hit = wasHit ? 1 : 0;
        measurements_.push_back(m);
    }
    /** Measurement(x, y, wasHit, dummy) in the robot frame (Observation.java:69-76) */
    void addLocal(double x, double y, bool wasHit) {
        Measurement m{};
        m.local_x = x; m.local_y = y; m.distance = std::sqrt(x * x + y * y); m.hit = wasHit ? 1 : 0;
        measurements_.push_back(m);
    }
    void addMeasurement(const Measurement &m) { measurements_.push_back(m); }
    const std::vector<Measurement> &getMeasurements() const { return measurements_; }
    int getNumberOfMeasurements() const { return (int)measurements_.size(); }
    void reset() { measurements_.clear(); }

private:
    std::vector<Measurement> measurements_;
};

class ParticleFilter;

/** GridMap(width, height, resolution, position) + createMapData(null) (GridMap.java:80-132) */
class GridMap {
public:
    GridMap(float width, float height, float resolution, float posX, float posY, int device = 0) {
        check(gms_params_default(&params_, width, height, resolution, posX, posY));
        params_.device = device;
        check(gms_map_create(&params_, &h_));
        check(gms_map_get_size(h_, &w_, &hgt_, nullptr));
    }
    explicit GridMap(const gms_params &p) : params_(p) {
        check(gms_map_create(&params_, &h_));
        check(gms_map_get_size(h_, &w_, &hgt_, nullptr));
    }
    ~GridMap() { gms_map_destroy(h_); }
    GridMap(const GridMap &) = delete;
    GridMap &operator=(const GridMap &) = delete;

    /** createMapData(other): a new map with the same geometry holding a copy of both arrays (GridMap.java:106-124) */
    GridMap *createMapData() const {
        GridMap *m = new GridMap(params_);
        check(gms_map_copy(m->h_, h_));
        return m;
    }
    void reset() { check(gms_map_reset(h_)); }                                               // :129-132
    double getRawAt(int x, int y) { double v; check(gms_map_get_raw_at(h_, 0, x, y, &v, nullptr)); return v; }   // :134
    double getProbAt(int x, int y) { double v; check(gms_map_get_raw_at(h_, 0, x, y, nullptr, &v)); return v; }  // :138
    double getRawAt(float px, float py) { double v; check(gms_map_get_at_point(h_, 0, px, py, &v, nullptr)); return v; }      // :142 (Vec2 point)
    double getLikelihood(float px, float py) { double v; check(gms_map_get_at_point(h_, 0, px, py, nullptr, &v)); return v; } // :150
    bool pointInMap(float px, float py) const {                                              // :164-170
        const float tx = (px - params_.pos_x) / params_.resolution, ty = (py - params_.pos_y) / params_.resolution;
        return !(tx < 0 || ty < 0 || tx >= (float)w_ || ty >= (float)hgt_);
    }
    /** integrateObservation(map, obs, pose) (:173-191) */
    void integrateObservation(const Observation &obs, const Pose &p) {
        const float pose[3] = {p.x, p.y, p.theta};
        check(gms_map_integrate(h_, obs.getMeasurements().data(), obs.getNumberOfMeasurements(), pose));
    }
    /** applyMeasurement(map, startX, startY, endX, endY, measuredDistance, wasHit) (:194-228) */
    void applyMeasurement(float startX, float startY, float endX, float endY, float measuredDistance, bool wasHit) {
        check(gms_map_apply_ray(h_, startX, startY, endX, endY, measuredDistance, wasHit ? 1 : 0));
    }
    /** computeLikelihoodMap(map) (:233-250) */
    void computeLikelihoodMap() { check(gms_map_build_likelihood(h_)); }
    /** integrateObservation + computeLikelihoodMap, rebuilding only what the scan changed */
    void update(const Observation &obs, const Pose &p) {
        const float pose[3] = {p.x, p.y, p.theta};
        check(gms_map_update(h_, obs.getMeasurements().data(), obs.getNumberOfMeasurements(), pose));
    }
    /** probabilityOf(map, obs, pose) (:261-294) */
    double probabilityOf(const Observation &obs, const Pose &p);
    /** findBestPose(map, obs, startPose) (:319-346) */
    Pose findBestPose(const Observation &obs, const Pose &start);

    /** what the dirty-tile rebuilds of computeLikelihoodMap did since the last call: 64 x 32-cell tiles {left alone, constants
     *  kept, constants written, blurred}; keepCounting = false stops the census (gms_map_tile_stats) */
    std::array<int64_t, 4> tileStats(bool keepCounting = true) {
        std::array<int64_t, 4> o{};
        check(gms_map_tile_stats(h_, keepCounting ? 1 : 0, o.data()));
        return o;
    }

    std::vector<double> logData() { std::vector<double> v((size_t)w_ * hgt_); check(gms_map_download_log(h_, v.data())); return v; }
    std::vector<double> likelihoodData() { std::vector<double> v((size_t)w_ * hgt_); check(gms_map_download_likelihood(h_, v.data())); return v; }
    void setLogData(const std::vector<double> &v) { check(gms_map_upload_log(h_, v.data())); }
    /** GridMap.render's grey levels (:371-388) of map mi, made on the device: one byte per pixel (GMS_VIEW_GREY8) or one packed colour
     *  word (GMS_VIEW_PACKED32) of the view's rectangle, ceil(w / d) x ceil(h / d) pixels row-major (gridmapslam.h "map views") */
    std::vector<uint8_t> render(const gms_view &v, int mi = 0) {
        int64_t bytes = 0;
        check(gms_view_size(&v, nullptr, nullptr, &bytes));
        std::vector<uint8_t> out((size_t)bytes);
        check(gms_map_view(h_, mi, &v, out.data()));
        return out;
    }
    /** The predicted scan (gridmapslam.h "predicted scans"): for every pose, the first occupied cell on the walk integrateObservation
     *  would make for every probe (local_x, local_y, distance of the measurements are read); records [poses][probes].  The walk includes
     *  the extra_steps cells past a probe's end point. */
    std::vector<gms_cast_hit> cast(const std::vector<Pose> &poses, const Observation &probes, int mi = 0) {
        const auto &ms = probes.getMeasurements();
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        std::vector<gms_cast_hit> out(poses.size() * ms.size());
        check(gms_map_cast(h_, mi, p.data(), (int32_t)poses.size(), ms.data(), (int32_t)ms.size(), out.data()));
        return out;
    }
    /** The view gain (gridmapslam.h "view gain"): for every candidate pose the distinct cells the probes' walks would see from it in
     *  map mi, by class -- walks cut at maxRange cells (1 .. 255) from the start cell and ended by their first occupied cell. */
    std::vector<gms_gain_rec> gain(const std::vector<Pose> &poses, const Observation &probes, int maxRange, int mi = 0) {
        const auto &ms = probes.getMeasurements();
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        const gms_gain g{maxRange, 0};
        std::vector<gms_gain_rec> out(poses.size());
        check(gms_map_gain(h_, mi, &g, p.data(), (int32_t)poses.size(), ms.data(), (int32_t)ms.size(), out.data()));
        return out;
    }
    /** Map srcMi of src read through the rigid transform w -- the pose of src's world frame in this map's world -- and compared with,
     *  copied into, added to or filled into the rectangle of map mi (gridmapslam.h "map warps"; w.op: GMS_WARP_*).  Returns the
     *  class-pair counts, taken from this map's values before the call. */
    gms_warp_stats warpFrom(GridMap &src, const gms_warp &w, int mi = 0, int srcMi = 0) {
        gms_warp_stats st{};
        check(gms_map_warp(h_, mi, src.h_, srcMi, &w, &st));
        return st;
    }
    /** Trajectory rollouts (gridmapslam.h "trajectory rollouts") from every start pose in map mi: arcs [K][T] (gms_rollout_arcs makes
     *  unicycle arcs), points [F][2] the footprint, clear / cost whole-map fields or null; records [poses.size()][K], row-major. */
    std::vector<gms_rollout_rec> rollout(const std::vector<Pose> &poses, const gms_rollout &req, const std::vector<gms_rollout_step> &arcs, int K, int T,
                                         const std::vector<float> &points, const uint16_t *clear = nullptr, const uint16_t *cost = nullptr, int mi = 0) {
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        std::vector<gms_rollout_rec> out(poses.size() * (size_t)(K > 0 ? K : 0));
        check(gms_map_rollout(h_, mi, &req, p.data(), (int32_t)poses.size(), arcs.data(), K, T, points.empty() ? nullptr : points.data(),
                              (int32_t)(points.size() / 2), clear, cost, out.data()));
        return out;
    }
    /** Routes (gridmapslam.h "routes") from every start cell -- starts = x0, y0, x1, y1, ... -- in map mi over cost, a whole-map
     *  cost-to-go field for req's inflate and mode; clear a whole-map clearance field or null.  One record per start; waypoints becomes
     *  [starts][req.max_waypoints][2] and, where wanted, *cells [starts][req.max_cells][2], both zero behind a record's counts. */
    std::vector<gms_route_rec> route(const std::vector<int32_t> &starts, const gms_route &req, const uint16_t *cost, std::vector<int32_t> &waypoints,
                                     const uint16_t *clear = nullptr, std::vector<int32_t> *cells = nullptr, int mi = 0) {
        const size_t n = starts.size() / 2;
        std::vector<gms_route_rec> out(n);
        waypoints.assign(n * (size_t)(req.max_waypoints > 0 ? req.max_waypoints : 0) * 2, 0);
        if (cells) cells->assign(n * (size_t)(req.max_cells > 0 ? req.max_cells : 0) * 2, 0);
        check(gms_map_route(h_, mi, &req, starts.data(), (int32_t)n, cost, clear, out.data(), waypoints.data(), cells ? cells->data() : nullptr));
        return out;
    }
    /** The clearance field (gridmapslam.h "clearance fields") of map mi: per cell of c's rectangle the squared distance in cells to the
     *  nearest obstacle cell of the whole map, GMS_CLEAR_FAR beyond c.max_radius; [h][w] row-major */
    std::vector<uint16_t> clearance(const gms_clearance &c, int mi = 0) {
        int64_t bytes = 0;
        check(gms_clearance_size(&c, nullptr, nullptr, &bytes));
        std::vector<uint16_t> out((size_t)bytes / sizeof(uint16_t));
        check(gms_map_clearance(h_, mi, &c, out.data()));
        return out;
    }
    /** Sites and skeleton (gridmapslam.h "sites and skeleton") of map mi over q's rectangle, each [h][w] row-major: site (may be null)
     *  the nearest obstacle cell oy * W + ox of every cell, GMS_SITE_NONE beyond q.max_radius; skel (may be null) d2 on the skeleton
     *  cells, else 0.  Returns the totals over the rectangle. */
    gms_skeleton_totals skeleton(const gms_skeleton &q, std::vector<uint32_t> *site, std::vector<uint16_t> *skel = nullptr, int mi = 0) {
        int64_t siteBytes = 0, skelBytes = 0;
        check(gms_skeleton_size(&q, nullptr, nullptr, &siteBytes, &skelBytes));
        if (site) site->resize((size_t)siteBytes / sizeof(uint32_t));
        if (skel) skel->resize((size_t)skelBytes / sizeof(uint16_t));
        gms_skeleton_totals totals{};
        check(gms_map_skeleton(h_, mi, &q, site ? site->data() : nullptr, skel ? skel->data() : nullptr, &totals));
        return totals;
    }
    /** the whole map's skeleton request */
    gms_skeleton fullSkeleton(int maxRadius, bool notFree = false, int minClear = 1, int minGap = 2) const {
        return gms_skeleton{0, 0, w_, hgt_, maxRadius, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, minClear, minGap, 0, {0, 0, 0}};
    }
    /** the nearest obstacle cell under every pose's cell and its squared distance, without making a field; {GMS_SITE_OUTSIDE,
     *  GMS_CLEAR_OUTSIDE} for a pose off the map, {GMS_SITE_NONE, GMS_CLEAR_FAR} with nothing within maxRadius */
    std::vector<gms_nearest> nearest_poses(const std::vector<Pose> &poses, int maxRadius, bool notFree = false, int mi = 0) {
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        std::vector<gms_nearest> out(poses.size());
        check(gms_map_nearest_poses(h_, mi, p.data(), (int32_t)poses.size(), maxRadius, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, out.data()));
        return out;
    }
    /** The cost-to-go field (gridmapslam.h "cost-to-go fields") of map mi: per cell of r's rectangle the cost of the cheapest path from
     *  any of seeds ({x, y} pairs) through the cells that are not blocked, GMS_REACH_FAR beyond r.max_cost; [h][w] row-major */
    std::vector<uint16_t> reach(const gms_reach &r, const std::vector<int32_t> &seeds, int mi = 0) {
        int64_t bytes = 0;
        check(gms_reach_size(&r, nullptr, nullptr, &bytes));
        std::vector<uint16_t> out((size_t)bytes / sizeof(uint16_t));
        check(gms_map_reach(h_, mi, &r, seeds.data(), (int32_t)(seeds.size() / 2), out.data()));
        return out;
    }
    /** the whole map's cost-to-go request */
    gms_reach fullReach(int maxCost = 0xFFFE, int inflate = 0, bool notFree = true) const {
        return gms_reach{0, 0, w_, hgt_, maxCost, inflate, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, 0};
    }
    /** The frontier regions (gridmapslam.h "frontier regions") of map mi: the records of the regions with count >= f.min_size in
     *  ascending anchor order, at most cap of them; *found (may be null) how many qualify.  cost (may be null): the whole map's
     *  cost-to-go field, [H][W]; labels (may be null) receives f's rectangle of the label field, [h][w] */
    std::vector<gms_frontier> frontiers(const gms_frontiers &f, int cap = 4096, const std::vector<uint16_t> *cost = nullptr,
                                        std::vector<uint32_t> *labels = nullptr, int *found = nullptr, int mi = 0) {
        int64_t bytes = 0;
        check(gms_frontiers_size(&f, nullptr, nullptr, &bytes));
        if (labels) labels->resize((size_t)bytes / sizeof(uint32_t));
        std::vector<gms_frontier> rec((size_t)cap);
        int32_t n = 0;
        check(gms_map_frontiers(h_, mi, &f, cost ? cost->data() : nullptr, labels ? labels->data() : nullptr, cap ? rec.data() : nullptr, cap, &n));
        rec.resize((size_t)(n < cap ? n : cap));
        if (found) *found = n;
        return rec;
    }
    /** the whole map's frontier request */
    gms_frontiers fullFrontiers(int minSize = 1, int inflate = 0) const { return gms_frontiers{0, 0, w_, hgt_, minSize, inflate, 0, 0}; }
    /** rounds launched and tile relaxations run for the last cost-to-go field of this handle */
    void reachStats(int32_t *rounds, int64_t *tileRuns) const { check(gms_map_reach_stats(h_, rounds, tileRuns)); }
    /** Rooms and doors of map mi (gridmapslam.h "rooms and doors"): the room records in rank order (at most capRooms); *doors (may be
     *  null) receives the door records in ascending (a, b) order (at most capDoors), *labels / *depth (may be null) the two fields of
     *  q's rectangle, *found (may be null) the true numbers {rooms, doors}. */
    std::vector<gms_room> rooms(const gms_rooms &q, int capRooms = 1024, std::vector<gms_door> *doors = nullptr, int capDoors = 4096,
                                std::vector<uint32_t> *labels = nullptr, std::vector<uint16_t> *depth = nullptr, int *found = nullptr, int mi = 0) {
        int64_t lb = 0, db = 0;
        check(gms_rooms_size(&q, nullptr, nullptr, &lb, &db));
        if (labels) labels->resize((size_t)lb / sizeof(uint32_t));
        if (depth) depth->resize((size_t)db / sizeof(uint16_t));
        std::vector<gms_room> rec((size_t)capRooms);
        if (doors) doors->resize((size_t)capDoors);
        const int cd = doors ? capDoors : 0;
        int32_t nr = 0, nd = 0;
        check(gms_map_rooms(h_, mi, &q, labels ? labels->data() : nullptr, depth ? depth->data() : nullptr, capRooms ? rec.data() : nullptr, capRooms, &nr,
                            cd ? doors->data() : nullptr, cd, &nd));
        rec.resize((size_t)(nr < capRooms ? nr : capRooms));
        if (doors) doors->resize((size_t)(nd < cd ? nd : cd));
        if (found) { found[0] = nr; found[1] = nd; }
        return rec;
    }
    /** the whole map's rooms request */
    gms_rooms fullRooms(int core = 15, int inflate = 5, int mode = GMS_CLEAR_NOT_FREE, int minCore = 1, int maxCost = 0xFFFE) const {
        return gms_rooms{0, 0, w_, hgt_, core, inflate, mode, minCore, maxCost, 0, {0, 0}};
    }
    /** The offset table of a scan for locate() (gridmapslam.h "global scan matching"; pure host code): [nTheta][B][2] end cells
     *  relative to the pose's cell under the headings theta0 + k * dtheta; misses and beams beyond 4095 cells become SKIP pairs. */
    std::vector<int16_t> locateOffsets(const Observation &z, double theta0, double dtheta, int nTheta) const {
        const auto &ms = z.getMeasurements();
        std::vector<int16_t> off((size_t)nTheta * ms.size() * 2);
        check(gms_locate_offsets(ms.data(), (int32_t)ms.size(), theta0, dtheta, nTheta, (double)params_.resolution, off.data()));
        return off;
    }
    /** Global scan matching in map mi: the best lc.cap candidates (heading index, cell) of lc's rectangle whose score -- the beams
     *  of `offsets` [lc.n_theta][B][2] that end within lc.tol cells of an obstacle -- is at least lc.min_score, score descending,
     *  then k, y, x ascending: the exhaustive search's result, found by a pruned multi-resolution one. */
    std::vector<gms_locate_rec> locate(const gms_locate &lc, const std::vector<int16_t> &offsets, int mi = 0) {
        std::vector<gms_locate_rec> rec((size_t)lc.cap);
        int32_t n = 0;
        check(gms_map_locate(h_, mi, &lc, offsets.data(), (int32_t)(offsets.size() / 2 / (size_t)(lc.n_theta > 0 ? lc.n_theta : 1)), rec.data(), &n));
        rec.resize((size_t)n);
        return rec;
    }
    /** the whole map's scan-matching request */
    gms_locate fullLocate(int nTheta, int tol, int minScore, int cap = 64, bool freeOnly = true, bool notFree = false) const {
        return gms_locate{0, 0, w_, hgt_, nTheta, tol, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, minScore, cap, freeOnly ? 1 : 0, 0, 0};
    }
    /** the top level of this handle's last locate() and the candidates it evaluated per level, evaluated[8] */
    void locateStats(int32_t *levels, int64_t *evaluated) const { check(gms_map_locate_stats(h_, levels, evaluated)); }
    /** the clearance under every pose's cell, without making a field; GMS_CLEAR_OUTSIDE for a pose off the map */
    std::vector<uint16_t> clearanceOf(const std::vector<Pose> &poses, int maxRadius, bool notFree = false, int mi = 0) {
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        std::vector<uint16_t> out(poses.size());
        check(gms_map_clearance_poses(h_, mi, p.data(), (int32_t)poses.size(), maxRadius, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, out.data()));
        return out;
    }
    /** the whole map's clearance request */
    gms_clearance fullClearance(int maxRadius, bool notFree = false) const {
        return gms_clearance{0, 0, w_, hgt_, maxRadius, notFree ? GMS_CLEAR_NOT_FREE : GMS_CLEAR_OCCUPIED, 0};
    }
    /** the whole map at one cell per pixel */
    gms_view fullView(bool likelihood = false, bool packed = false, int decimate = 1) const {
        return gms_view{0, 0, w_, hgt_, decimate, likelihood ? GMS_VIEW_LIKELIHOOD : GMS_VIEW_LOG, packed ? GMS_VIEW_PACKED32 : GMS_VIEW_GREY8, 0};
    }

    float getResolution() const { return params_.resolution; }                               // :426-428
    std::pair<float, float> getPosition() const { return {params_.pos_x, params_.pos_y}; }   // :430-432
    std::pair<float, float> getWorldSize() const { return {(float)w_ * params_.resolution, (float)hgt_ * params_.resolution}; }   // :88,422
    int getGridWidth() const { return w_; }
    int getGridHeight() const { return hgt_; }
    gms_map *handle() { return h_; }

private:
    gms_params params_{};
    gms_map *h_ = nullptr;
    int32_t w_ = 0, hgt_ = 0;
};

/** ParticleFilter(numberOfParticles) (J/slam/ParticleFilter.java:43), bound to the map it scores against */
class ParticleFilter {
public:
    struct Particle {               // ParticleFilter.Particle (ParticleFilter.java:21-38)
        double weight;
        Pose pose;
    };

    ParticleFilter(GridMap &map, int numberOfParticles) : n_(numberOfParticles) {
        check(gms_pf_create(map.handle(), numberOfParticles, &h_));
    }
    ~ParticleFilter() { gms_pf_destroy(h_); }
    ParticleFilter(const ParticleFilter &) = delete;
    ParticleFilter &operator=(const ParticleFilter &) = delete;

    /** getParticles() (ParticleFilter.java:50): a snapshot */
    std::vector<Particle> getParticles() {
        std::vector<float> p((size_t)n_ * 3);
        std::vector<double> w(n_);
        check(gms_pf_get_poses(h_, p.data()));
        check(gms_pf_get_weights(h_, w.data()));
        std::vector<Particle> out(n_);
        for (int i = 0; i < n_; i++) out[i] = Particle{w[i], Pose(p[3 * i], p[3 * i + 1], p[3 * i + 2])};
        return out;
    }
    void setPoses(const std::vector<Pose> &poses) {
        if (poses.size() < (size_t)n_) throw Error(GMS_ERR_INVALID, "SlamParticleMaps::setPoses: fewer poses than particles");
        std::vector<float> p((size_t)n_ * 3);
        for (int i = 0; i < n_; i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        check(gms_pf_set_poses(h_, p.data()));
    }
    /** weight[i] = probabilityOf(map, obs, pose[i]) (SLAM.java:99) */
    void score(const Observation &obs) { check(gms_pf_score(h_, obs.getMeasurements().data(), obs.getNumberOfMeasurements())); }
    /** weightSum, strongest, weight /= weightSum, Neff (SLAM.java:87-129) */
    gms_pf_stats normalize() { gms_pf_stats s{}; check(gms_pf_normalize(h_, &s)); return s; }
    /** resample() (ParticleFilter.java:59-82 surface, SLAM.java:133-153 semantics); r01 stands for Math.random() */
    void resample(double r01) { check(gms_pf_resample(h_, &r01, nullptr, nullptr)); }
    void refinePoses(const Observation &obs) { check(gms_pf_refine_poses(h_, obs.getMeasurements().data(), obs.getNumberOfMeasurements())); }
    /** opt-in, not in the reference: normalise from the log-weights (exp(logw - max logw)) instead of the plain product of up to
     *  720 factors, which underflows for nearly every particle of a wide cloud (gms_pf_set_log_normalize) */
    void setLogNormalize(bool on) { check(gms_pf_set_log_normalize(h_, on ? 1 : 0)); }
    Pose getWeightedPose() { float o[3]; check(gms_pf_weighted_pose(h_, o)); return Pose(o[0], o[1], o[2]); }
    /** Particle seeding (gridmapslam.h "particle seeding"): the slots [sc.first, sc.first + sc.count) receive poses drawn uniformly
     *  over the eligible cells of the map -- free, inside sc's rectangle, no obstacle within sc.inflate cells -- with uniform headings
     *  and the weight 1 / nGlobal.  nEligible (may be null): the number of eligible cells, read back with one synchronise; without it
     *  nothing is synchronised.  A single-map filter, as the rest of this class. */
    void scatter(const gms_scatter &sc, uint64_t seed, uint64_t sequence, int64_t *nEligible = nullptr) {
        check(gms_pf_scatter(h_, &sc, seed, sequence, nEligible));
    }
    /** The pose modes of the filter (gridmapslam.h "pose modes"): the particles binned in (x, y, theta) per q, the occupied bins grouped
     *  into maximal 26-connected sets with the heading wrapping.  labels [size()] and records [cap] are host memory, either may be
     *  null (records exactly when cap == 0); returns the number of modes with count >= q.min_count, of which the first cap are
     *  stored in ascending anchor order.  nOutside (may be null): the particles off the map or with a non-finite heading.  Waits on
     *  the stream.  A single-map filter, as the rest of this class. */
    int32_t modes(const gms_modes &q, uint32_t *labels, gms_mode *records, int32_t cap, int32_t *nOutside = nullptr) {
        int32_t found = 0;
        check(gms_pf_modes(h_, 0, &q, labels, records, cap, &found, nOutside));
        return found;
    }
    /** modes() into device memory (labels 4-byte, records 8-byte aligned), written on the handle's stream; complete on return */
    int32_t modesDev(const gms_modes &q, uint32_t *devLabels, gms_mode *devRecords, int32_t cap, int32_t *nOutside = nullptr) {
        int32_t found = 0;
        check(gms_pf_modes_dev(h_, 0, &q, devLabels, devRecords, cap, &found, nOutside));
        return found;
    }
    /** GridMap::rollout from every particle's pose, counted per candidate (gms_pf_rollout): one gms_rollout_risk per candidate; after
     *  a resample n_hit / size() is the collision probability of the command.  The filter is not changed. */
    std::vector<gms_rollout_risk> rolloutRisk(const gms_rollout &req, const std::vector<gms_rollout_step> &arcs, int K, int T, const std::vector<float> &points) {
        std::vector<gms_rollout_risk> out((size_t)(K > 0 ? K : 0));
        check(gms_pf_rollout(h_, &req, arcs.data(), K, T, points.empty() ? nullptr : points.data(), (int32_t)(points.size() / 2), out.data()));
        return out;
    }
    /** The beam sensor model (gridmapslam.h "beam sensor model"): every particle weighted by where the map's first wall lies on each
     *  beam's walk relative to the measured end point.  factors [2][behind + ahead + 2] host doubles (row 0: beams that missed, row 1:
     *  beams that hit), every entry finite and > 0; residuals (may be null) [size()][B] receives the table index per particle and
     *  beam, and only then does the call wait on the stream.  Leaves the filter as score() does. */
    void scoreBeams(const Observation &obs, int32_t behind, int32_t ahead, const double *factors, uint16_t *residuals = nullptr) {
        check(gms_pf_score_beams(h_, obs.getMeasurements().data(), obs.getNumberOfMeasurements(), behind, ahead, factors, residuals));
    }
    /** scoreBeams() on device-resident beams [B] (devResiduals: device memory, 2-byte aligned, or null); factors stay host memory.
     *  Runs on the handle's stream and synchronises nothing. */
    void scoreBeamsDev(const gms_beam *devBeams, int32_t B, int32_t behind, int32_t ahead, const double *factors, uint16_t *devResiduals = nullptr) {
        check(gms_pf_score_beams_dev(h_, devBeams, B, behind, ahead, factors, devResiduals));
    }
    int size() const { return n_; }
    gms_pf *handle() { return h_; }

    /** multi-GPU: this rank holds particles [offset, offset + size()) of nGlobal (equal shards in rank order) */
    void setShard(int64_t offset, int64_t nGlobal) { check(gms_pf_set_shard(h_, offset, nGlobal)); }

private:
    gms_pf *h_ = nullptr;
    int n_;
};

/** One rank's RCCL communicator (one process per GPU).  `id` is the 128-byte token of uniqueId(), made by one
 *  rank and handed to the others by whatever channel the host has (a file, a socket, MPI ...). */
class Comm {
public:
    static std::vector<char> uniqueId() { std::vector<char> id(128); check(gms_comm_unique_id(id.data())); return id; }
    Comm(const std::vector<char> &id, int rank, int world, int device) { check(gms_comm_create(&h_, id.data(), rank, world, device)); }
    ~Comm() { gms_comm_destroy(h_); }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    gms_comm *handle() { return h_; }
    /** SLAM.update (SLAM.java:80-131) + `if (neff < fraction * N) resample()` (GridMapApp.java:185-186) for a sharded
     *  filter with device-resident inputs; both exchanges happen inside. */
    void slamUpdate(ParticleFilter &pf, const float *devPoses, const gms_beam *devBeams, int B, double r01,
                    double fraction = 0.5, bool integrate = true) {
        check(gms_slam_update_sharded_dev(pf.handle(), h_, devPoses, devBeams, B, &r01, fraction, integrate ? 1 : 0));
    }

private:
    gms_comm *h_ = nullptr;
};

inline double GridMap::probabilityOf(const Observation &obs, const Pose &p) {
    ParticleFilter pf(*this, 1);
    pf.setPoses({p});
    pf.score(obs);
    return pf.getParticles()[0].weight;
}

inline Pose GridMap::findBestPose(const Observation &obs, const Pose &start) {
    ParticleFilter pf(*this, 1);
    pf.setPoses({start});
    pf.refinePoses(obs);
    return pf.getParticles()[0].pose;
}

/** The particle filter the reference runs (J/slam/SLAM.java), pose proposals being an input */
class SLAM {
public:
    explicit SLAM(int numParticles = 500, float width = 6.0f, float height = 6.0f, float resolution = 0.05f,
                  float posX = -3.0f, float posY = -3.0f)                                   // SLAM.java:50,57
        : gridMap_(width, height, resolution, posX, posY), pf_(gridMap_, numParticles) {
        gridMap_.computeLikelihoodMap();
    }
    /** update(z, u) (SLAM.java:80-131); `poses` are the motion-model samples, dTheta is u.dTheta */
    double update(const Observation &z, const std::vector<Pose> *poses = nullptr, double dTheta = 0.0) {
        const bool skipUpdate = std::fabs(dTheta) > (3.141592653589793 / 180.0) * 30;       // :82
        std::vector<float> p;
        if (poses) {                                                                        // :90
            p.resize(poses->size() * 3);
            for (size_t i = 0; i < poses->size(); i++) { p[3 * i] = (*poses)[i].x; p[3 * i + 1] = (*poses)[i].y; p[3 * i + 2] = (*poses)[i].theta; }
        }
        const double unused_r01 = 0.0;
        gms_pf_stats st{};
        // one call: score (:99), bookkeeping (:100-124), map update at the weighted pose (:102-105, :93); no resample here
        check(gms_slam_update(pf_.handle(), poses ? p.data() : nullptr, z.getMeasurements().data(), z.getNumberOfMeasurements(),
                              &unused_r01, -1.0, skipUpdate ? 0 : 1, &st));
        strongest_ = st.strongest;
        return st.neff;
    }
    void resample(double r01) { pf_.resample(r01); }                                        // :133-153
    Pose getWeightedPose() { return pf_.getWeightedPose(); }                                // :165-178
    double calculateNeff() { gms_pf_stats s{}; check(gms_pf_get_stats(pf_.handle(), &s)); return s.neff; }   // :180-190
    std::vector<ParticleFilter::Particle> getParticles() { return pf_.getParticles(); }     // :192
    int getStrongestParticle() const { return strongest_; }                                 // :196
    GridMap &getGridMap() { return gridMap_; }                                              // :200

private:
    GridMap gridMap_;
    ParticleFilter pf_;
    int strongest_ = 0;
};

/** SLAM as the reference has it (J/slam/SLAM.java:26-204): every Particle owns a pose, a weight AND a GridMapData.  update() scores a
 *  particle against its own likelihood field and integrates the scan into its own map at its own pose (:88-107); resample()
 *  deep-copies the surviving particles' maps (:41-45 -> GridMap.createMapData(other), GridMap.java:106-124).  findBestPoseOptim (:97)
 *  is left out; the motion-model draw of Odometry.apply is Philox(seed; particle slot, sequence). */
class SlamParticleMaps {
public:
    struct Odometry { double dCenter = 0, dTheta = 0; };                                   // J/slam/Odometry.java:31
    struct Particle { double weight; Pose pose; };                                          // SLAM.Particle without its map: mapOf(i)

    explicit SlamParticleMaps(int numParticles = 500, float width = 6.0f, float height = 6.0f, float resolution = 0.05f,
                              float posX = -3.0f, float posY = -3.0f, int maxBeams = 0) : n_(numParticles) {   // SLAM.java:50,57
        gms_params p{};
        check(gms_params_default(&p, width, height, resolution, posX, posY));
        p.max_beams = maxBeams;
        check(gms_slam_create(&p, numParticles, &h_));
        check(gms_slam_handles(h_, &map_, &pf_));
        check(gms_slam_count(h_, nullptr, &w_, &hgt_));
    }
    /** One rank's block [offset, offset + numParticlesLocal) of a filter of numParticlesGlobal particles sharded WITH their maps over
     *  the GPUs of a node (gms_slam_create_shard; blocks of a multiple of 256 particles in rank order): updateSharded / resampleSharded */
    SlamParticleMaps(int numParticlesLocal, long long offset, long long numParticlesGlobal, float width, float height, float resolution,
                     float posX, float posY, int maxBeams = 0, int device = 0) : n_(numParticlesLocal) {
        gms_params p{};
        check(gms_params_default(&p, width, height, resolution, posX, posY));
        p.max_beams = maxBeams;
        p.device = device;
        check(gms_slam_create_shard(&p, numParticlesLocal, offset, numParticlesGlobal, &h_));
        check(gms_slam_handles(h_, &map_, &pf_));
        check(gms_slam_count(h_, nullptr, &w_, &hgt_));
    }
    ~SlamParticleMaps() { gms_slam_destroy(h_); }
    SlamParticleMaps(const SlamParticleMaps &) = delete;
    SlamParticleMaps &operator=(const SlamParticleMaps &) = delete;

    void reset() { check(gms_slam_reset(h_)); }                                             // :65-77
    /** update() refines every particle's pose with GridMap.findBestPose against the particle's own field before weighting it (:96) */
    void setRefine(bool on) { check(gms_slam_set_refine(h_, on ? 1 : 0)); }
    /** update() aligns every particle against its own field between computeLikelihoodMap and the weighting -- the stand-in for
     *  findBestPoseOptim (:97; gridmapslam.h "per-particle scan alignment"); params null: off.  With setRefine: lattice first. */
    void setAlign(const gms_align_params *params) { check(gms_slam_set_align(h_, params)); }
    /** the same alignment as a call of its own: every particle in place, no map and no weight changes; records [n] or null */
    void align(const Observation &z, const gms_align_params &params, gms_align_record *records = nullptr) {
        check(gms_slam_align(h_, z.getMeasurements().data(), z.getNumberOfMeasurements(), &params, records));
    }
    /** the records [n] of the last aligned update (throws before there is one); waits for the stream */
    void lastAlign(gms_align_record *records) { check(gms_slam_last_align(h_, records)); }
    /** the beam sensor model of every particle through ITS OWN map (gridmapslam.h "per-particle beam sensor model"): raw weights and
     *  log-weights as update_local leaves them, no pose and no map changes; factors [2][behind + ahead + 2] host doubles, residuals [n][B] or null */
    void score_beams(const Observation &z, const double *factors, int32_t behind, int32_t ahead, uint16_t *residuals = nullptr) {
        check(gms_slam_score_beams(h_, z.getMeasurements().data(), z.getNumberOfMeasurements(), behind, ahead, factors, residuals));
    }
    /** every update weighs each particle by that model as well, through its map as it stands before the scan goes into it; combine:
     *  GMS_SLAM_BEAMS_MULTIPLY or GMS_SLAM_BEAMS_REPLACE; factors null: off */
    void set_beam_model(const double *factors, int32_t behind = 0, int32_t ahead = 0, int32_t combine = GMS_SLAM_BEAMS_MULTIPLY) {
        check(gms_slam_set_beam_model(h_, behind, ahead, factors, combine));
    }
    /** update(z, u) (:80-131); returns Neff. seed / sequence select the motion model's variates (one sequence per frame). */
    double update(const Observation &z, const Odometry &u, uint64_t seed, uint64_t sequence, bool sampleMotion = true) {
        gms_pf_stats st{};
        check(gms_slam_update_per_particle(h_, z.getMeasurements().data(), z.getNumberOfMeasurements(), sampleMotion ? 1 : 0, u.dCenter, u.dTheta,
                                           seed, sequence, &st));
        strongest_ = st.strongest;
        return st.neff;
    }
    /** GridMapApp.onHandleData for one raw revolution (J/app/GridMapApp.java:133-192) as one call: the de-skew (:143-175), update(z, u)
     *  (:178) and `if (neff < fraction * n) resample()` (:185-186; fraction < 0: no resampling).  angle / distance / hit: `length`
     *  measurements.  Nothing is read back and the stream is not synchronised; onHandleDataNeff is the form that returns update()'s Neff. */
    void onHandleData(const double *angle, const double *distance, const uint8_t *hit, int length, const Odometry &u, uint64_t seed,
                      uint64_t sequence, double r01, double fraction = 0.5) {
        check(gms_slam_frame_per_particle(h_, angle, distance, hit, length, u.dCenter, u.dTheta, seed, sequence, r01, fraction, nullptr));
    }
    double onHandleDataNeff(const double *angle, const double *distance, const uint8_t *hit, int length, const Odometry &u, uint64_t seed,
                            uint64_t sequence, double r01, double fraction = 0.5) {
        gms_pf_stats st{};
        check(gms_slam_frame_per_particle(h_, angle, distance, hit, length, u.dCenter, u.dTheta, seed, sequence, r01, fraction, &st));
        strongest_ = st.strongest;
        return st.neff;
    }
    /** update(z, u) over all ranks of a sharded filter (every rank: the same scan, odometry, seed and sequence); returns Neff */
    double updateSharded(Comm &comm, const Observation &z, const Odometry &u, uint64_t seed, uint64_t sequence, bool sampleMotion = true) {
        gms_pf_stats st{};
        check(gms_slam_update_sharded_maps(h_, comm.handle(), z.getMeasurements().data(), z.getNumberOfMeasurements(), sampleMotion ? 1 : 0, u.dCenter,
                                           u.dTheta, seed, sequence, &st));
        strongest_ = st.strongest;
        return st.neff;
    }
    /** resample() over all ranks (every rank: the same r01; fraction < 0: unconditional); returns whether it drew */
    bool resampleSharded(Comm &comm, double r01, double fraction = -1.0) {
        int32_t did = 0;
        check(gms_slam_resample_sharded_maps(h_, comm.handle(), r01, fraction, &did));
        return did != 0;
    }
    /** resample() (:133-153); r01 stands for Math.random() */
    void resample(double r01) { check(gms_slam_resample_maps(h_, r01, nullptr, nullptr)); }
    // `if (neff < fraction * n) resample()` (GridMapApp.java:185-186) decided on the device: update + this is a revolution without a host round trip
    void resampleIf(double r01, double fraction = 0.5) { check(gms_slam_resample_maps_if(h_, r01, fraction)); }
    Pose getWeightedPose() { float o[3]; check(gms_pf_weighted_pose(pf_, o)); return Pose(o[0], o[1], o[2]); }      // :165-178
    double calculateNeff() { gms_pf_stats s{}; check(gms_pf_get_stats(pf_, &s)); return s.neff; }                    // :180-190
    std::vector<Particle> getParticles() {                                                  // :192
        std::vector<float> p((size_t)n_ * 3);
        std::vector<double> w(n_);
        check(gms_pf_get_poses(pf_, p.data()));
        check(gms_pf_get_weights(pf_, w.data()));
        std::vector<Particle> out(n_);
        for (int i = 0; i < n_; i++) out[i] = Particle{w[i], Pose(p[3 * i], p[3 * i + 1], p[3 * i + 2])};
        return out;
    }
    void setPoses(const std::vector<Pose> &poses) {
        if (poses.size() < (size_t)n_) throw Error(GMS_ERR_INVALID, "SlamParticleMaps::setPoses: fewer poses than particles");
        std::vector<float> p((size_t)n_ * 3);
        for (int i = 0; i < n_; i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        check(gms_pf_set_poses(pf_, p.data()));
    }
    int getStrongestParticle() const { return strongest_; }                                 // :196
    /** Particle i's GridMapData.logData (or .likelihoodData), W * H doubles, row-major x + y * W (SLAM.java:33, GridMap.java:72-74) */
    std::vector<double> mapOf(int i, bool likelihood = false) {
        std::vector<double> out((size_t)w_ * hgt_);
        check(gms_slam_download_map(h_, i, likelihood ? nullptr : out.data(), likelihood ? out.data() : nullptr));
        return out;
    }
    /** GridMapApp.render's "strongest" / "chosen particle" cases (J/app/GridMapApp.java:374-393) through GridMap.render (GridMap.java:371-388):
     *  the grey levels of particle `which`'s map, or -- which == GMS_VIEW_STRONGEST -- of the strongest particle's, picked on the device;
     *  *shown (may be null) receives the particle that was drawn.  The combined map: calculateCombined(), then gms_map_view on the map of
     *  gms_slam_handles. */
    std::vector<uint8_t> render(const gms_view &v, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        int64_t bytes = 0;
        check(gms_view_size(&v, nullptr, nullptr, &bytes));
        std::vector<uint8_t> out((size_t)bytes);
        int32_t drawn = 0;
        check(gms_slam_view(h_, which, &v, out.data(), &drawn));
        if (shown) *shown = drawn;
        return out;
    }
    /** The frontier regions of particle `which`'s own map (GridMap::frontiers' values); *shown (may be null) receives the particle
     *  whose regions were made */
    std::vector<gms_frontier> frontiers(const gms_frontiers &f, int cap = 4096, const std::vector<uint16_t> *cost = nullptr,
                                        std::vector<uint32_t> *labels = nullptr, int *found = nullptr, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        int64_t bytes = 0;
        check(gms_frontiers_size(&f, nullptr, nullptr, &bytes));
        if (labels) labels->resize((size_t)bytes / sizeof(uint32_t));
        std::vector<gms_frontier> rec((size_t)cap);
        int32_t n = 0, picked = 0;
        check(gms_slam_frontiers(h_, which, &f, cost ? cost->data() : nullptr, labels ? labels->data() : nullptr, cap ? rec.data() : nullptr, cap, &n, &picked));
        rec.resize((size_t)(n < cap ? n : cap));
        if (found) *found = n;
        if (shown) *shown = picked;
        return rec;
    }
    /** Rooms and doors of particle `which`'s own map (GridMap::rooms' values); *shown (may be null) receives the particle that was read */
    std::vector<gms_room> rooms(const gms_rooms &q, int capRooms = 1024, std::vector<gms_door> *doors = nullptr, int capDoors = 4096,
                                std::vector<uint32_t> *labels = nullptr, std::vector<uint16_t> *depth = nullptr, int *found = nullptr,
                                int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        int64_t lb = 0, db = 0;
        check(gms_rooms_size(&q, nullptr, nullptr, &lb, &db));
        if (labels) labels->resize((size_t)lb / sizeof(uint32_t));
        if (depth) depth->resize((size_t)db / sizeof(uint16_t));
        std::vector<gms_room> rec((size_t)capRooms);
        if (doors) doors->resize((size_t)capDoors);
        const int cd = doors ? capDoors : 0;
        int32_t nr = 0, nd = 0, picked = 0;
        check(gms_slam_rooms(h_, which, &q, labels ? labels->data() : nullptr, depth ? depth->data() : nullptr, capRooms ? rec.data() : nullptr, capRooms, &nr,
                             cd ? doors->data() : nullptr, cd, &nd, &picked));
        rec.resize((size_t)(nr < capRooms ? nr : capRooms));
        if (doors) doors->resize((size_t)(nd < cd ? nd : cd));
        if (found) { found[0] = nr; found[1] = nd; }
        if (shown) *shown = picked;
        return rec;
    }
    /** The cost-to-go field of particle `which`'s own map (GridMap::reach's values); no seeds: the shown particle's own pose cell,
     *  picked on the device.  *shown (may be null) receives the particle whose field was made. */
    std::vector<uint16_t> reach(const gms_reach &r, const std::vector<int32_t> &seeds = {}, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        int64_t bytes = 0;
        check(gms_reach_size(&r, nullptr, nullptr, &bytes));
        std::vector<uint16_t> out((size_t)bytes / sizeof(uint16_t));
        int32_t picked = 0;
        check(gms_slam_reach(h_, which, &r, seeds.empty() ? nullptr : seeds.data(), (int32_t)(seeds.size() / 2), out.data(), &picked));
        if (shown) *shown = picked;
        return out;
    }
    /** The clearance field of particle `which`'s own map (GridMap::clearance's values) -- GMS_VIEW_STRONGEST: the strongest, as render()
     *  picks it; *shown (may be null) receives the particle whose field was made. */
    std::vector<uint16_t> clearance(const gms_clearance &c, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        int64_t bytes = 0;
        check(gms_clearance_size(&c, nullptr, nullptr, &bytes));
        std::vector<uint16_t> out((size_t)bytes / sizeof(uint16_t));
        int32_t picked = 0;
        check(gms_slam_clearance(h_, which, &c, out.data(), &picked));
        if (shown) *shown = picked;
        return out;
    }
    /** Sites and skeleton of particle `which`'s own map (GridMap::skeleton's values and totals); *shown (may be null) receives the
     *  particle whose map was read */
    gms_skeleton_totals skeleton(const gms_skeleton &q, std::vector<uint32_t> *site, std::vector<uint16_t> *skel = nullptr, int which = GMS_VIEW_STRONGEST,
                                 int *shown = nullptr) {
        int64_t siteBytes = 0, skelBytes = 0;
        check(gms_skeleton_size(&q, nullptr, nullptr, &siteBytes, &skelBytes));
        if (site) site->resize((size_t)siteBytes / sizeof(uint32_t));
        if (skel) skel->resize((size_t)skelBytes / sizeof(uint16_t));
        gms_skeleton_totals totals{};
        int32_t picked = 0;
        check(gms_slam_skeleton(h_, which, &q, site ? site->data() : nullptr, skel ? skel->data() : nullptr, &totals, &picked));
        if (shown) *shown = picked;
        return totals;
    }
    /** Global scan matching in particle `which`'s own map (GridMap::locate's records); *shown (may be null) receives the particle in
     *  whose map the scan was matched */
    std::vector<gms_locate_rec> locate(const gms_locate &lc, const std::vector<int16_t> &offsets, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        std::vector<gms_locate_rec> rec((size_t)lc.cap);
        int32_t n = 0, picked = 0;
        check(gms_slam_locate(h_, which, &lc, offsets.data(), (int32_t)(offsets.size() / 2 / (size_t)(lc.n_theta > 0 ? lc.n_theta : 1)), rec.data(), &n, &picked));
        rec.resize((size_t)n);
        if (shown) *shown = picked;
        return rec;
    }
    /** Particle `which`'s own map read through the rigid transform w into map mi of dst (GridMap::warpFrom's counts); the filter is
     *  only read.  *shown (may be null) receives the particle whose map was read */
    gms_warp_stats warpInto(GridMap &dst, const gms_warp &w, int which = GMS_VIEW_STRONGEST, int mi = 0, int *shown = nullptr) {
        gms_warp_stats st{};
        int32_t picked = 0;
        check(gms_slam_warp(h_, which, 0, dst.handle(), mi, &w, &st, &picked));
        if (shown) *shown = picked;
        return st;
    }
    /** The census of the particles' maps (gridmapslam.h "census of the particles' maps"): the totals, and -- each where non-null --
     *  counts resized to W * H * 2 {fr, oc}, consensus to W * H classes, agree to n * 10 words (pair[3][3] and a zero per particle).
     *  writeMap: the consensus also goes to the handle's own map as +1.0 / -1.0 / +0.0.  The filter is only read */
    gms_census_totals census(int minKnown = 1, std::vector<uint16_t> *counts = nullptr, std::vector<uint8_t> *consensus = nullptr,
                             std::vector<uint32_t> *agree = nullptr, bool writeMap = false, int filter = 0) {
        int32_t n = 0, W = 0, H = 0;
        check(gms_slam_count(h_, &n, &W, &H));
        const gms_census c{minKnown, filter, writeMap ? GMS_CENSUS_WRITE_MAP : 0, 0};
        if (counts) counts->assign((size_t)W * (size_t)H * 2, 0);
        if (consensus) consensus->assign((size_t)W * (size_t)H, 0);
        if (agree) agree->assign((size_t)n * 10, 0);
        gms_census_totals t{};
        check(gms_slam_census(h_, &c, counts ? counts->data() : nullptr, consensus ? consensus->data() : nullptr, agree ? agree->data() : nullptr, &t));
        return t;
    }
    /** Trajectory rollouts in particle `which`'s own map (GridMap::rollout's records); no poses: ONE start pose, the shown particle's
     *  own, read on the device.  *shown (may be null) receives the particle in whose map the arcs were rolled */
    std::vector<gms_rollout_rec> rollout(const std::vector<Pose> &poses, const gms_rollout &req, const std::vector<gms_rollout_step> &arcs, int K, int T,
                                         const std::vector<float> &points, const uint16_t *clear = nullptr, const uint16_t *cost = nullptr,
                                         int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        std::vector<gms_rollout_rec> out((poses.empty() ? 1 : poses.size()) * (size_t)(K > 0 ? K : 0));
        int32_t picked = 0;
        check(gms_slam_rollout(h_, which, &req, poses.empty() ? nullptr : p.data(), (int32_t)poses.size(), arcs.data(), K, T,
                               points.empty() ? nullptr : points.data(), (int32_t)(points.size() / 2), clear, cost, out.data(), &picked));
        if (shown) *shown = picked;
        return out;
    }
    /** Routes through particle `which`'s own map over that particle's field (GridMap::route's values); no starts: ONE start, the shown
     *  particle's own pose cell, read on the device.  *shown (may be null) receives the particle through whose map they were taken */
    std::vector<gms_route_rec> route(const std::vector<int32_t> &starts, const gms_route &req, const uint16_t *cost, std::vector<int32_t> &waypoints,
                                     const uint16_t *clear = nullptr, std::vector<int32_t> *cells = nullptr, int which = GMS_VIEW_STRONGEST,
                                     int *shown = nullptr) {
        const size_t n = starts.empty() ? 1 : starts.size() / 2;
        std::vector<gms_route_rec> out(n);
        waypoints.assign(n * (size_t)(req.max_waypoints > 0 ? req.max_waypoints : 0) * 2, 0);
        if (cells) cells->assign(n * (size_t)(req.max_cells > 0 ? req.max_cells : 0) * 2, 0);
        int32_t picked = 0;
        check(gms_slam_route(h_, which, &req, starts.empty() ? nullptr : starts.data(), (int32_t)(starts.size() / 2), cost, clear, out.data(), waypoints.data(),
                             cells ? cells->data() : nullptr, &picked));
        if (shown) *shown = picked;
        return out;
    }
    /** The view gain of the caller's candidate poses in particle `which`'s own map (GridMap::gain's records); *shown (may be null)
     *  receives the particle in whose map they were judged */
    std::vector<gms_gain_rec> gain(const std::vector<Pose> &poses, const Observation &probes, int maxRange, int which = GMS_VIEW_STRONGEST,
                                   int *shown = nullptr) {
        const auto &ms = probes.getMeasurements();
        std::vector<float> p(3 * poses.size());
        for (size_t i = 0; i < poses.size(); i++) { p[3 * i] = poses[i].x; p[3 * i + 1] = poses[i].y; p[3 * i + 2] = poses[i].theta; }
        const gms_gain g{maxRange, 0};
        std::vector<gms_gain_rec> out(poses.size());
        int32_t picked = 0;
        check(gms_slam_gain(h_, which, &g, p.data(), (int32_t)poses.size(), ms.data(), (int32_t)ms.size(), out.data(), &picked));
        if (shown) *shown = picked;
        return out;
    }
    /** The predicted scan of particle `which` -- GMS_VIEW_STRONGEST: the strongest, as render() picks it; GMS_CAST_ALL: every particle,
     *  records [size()][probes] -- at its own pose in its own map (gridmapslam.h "predicted scans"); *shown (may be null) receives the
     *  particle that was cast (not written for GMS_CAST_ALL). */
    std::vector<gms_cast_hit> cast(const Observation &probes, int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        const auto &ms = probes.getMeasurements();
        std::vector<gms_cast_hit> out((which == GMS_CAST_ALL ? (size_t)n_ : 1) * ms.size());
        int32_t picked = 0;
        check(gms_slam_cast(h_, which, 0, ms.data(), (int32_t)ms.size(), out.data(), &picked));
        if (shown && which != GMS_CAST_ALL) *shown = picked;
        return out;
    }
    /** GridMapApp.calculateCombined (J/app/GridMapApp.java:439-458): the combined logData */
    std::vector<double> calculateCombined() {
        check(gms_slam_combined(h_));
        std::vector<double> out((size_t)w_ * hgt_);
        check(gms_map_download_log(map_, out.data()));
        return out;
    }
    /** Keep every particle's path of the last `capacity` updates on the device, through resampling (gridmapslam.h "trajectories"); 0: off */
    void setHistory(int capacity) { check(gms_slam_set_history(h_, capacity)); }
    /** updates kept = min(updates recorded, capacity); *total (may be null): the updates recorded */
    int historyLength(int64_t *total = nullptr) {
        int32_t kept = 0;
        check(gms_slam_history_len(h_, total, &kept));
        return kept;
    }
    /** The path particle `which` -- or, GMS_VIEW_STRONGEST, the strongest particle as render() picks it -- descends along, oldest first
     *  over the kept updates: the path its map was built along.  *shown (may be null) receives the particle that was followed. */
    std::vector<Pose> trajectory(int which = GMS_VIEW_STRONGEST, int *shown = nullptr) {
        const int kept = historyLength();
        std::vector<float> p((size_t)3 * kept + 1);
        int32_t count = 0, followed = 0;
        check(gms_slam_trajectory(h_, which, 0, p.data(), kept, &count, &followed));
        if (shown) *shown = followed;
        std::vector<Pose> out((size_t)count);
        for (int j = 0; j < count; j++) out[j] = Pose(p[3 * j], p[3 * j + 1], p[3 * j + 2]);
        return out;
    }
    int size() const { return n_; }
    int width() const { return w_; }
    int height() const { return hgt_; }
    gms_slam *handle() { return h_; }

private:
    gms_slam *h_ = nullptr;
    gms_map *map_ = nullptr;     // owned by h_
    gms_pf *pf_ = nullptr;       // owned by h_
    int n_;
    int32_t w_ = 0, hgt_ = 0;
    int strongest_ = 0;
};

}  // namespace gms
