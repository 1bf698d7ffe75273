"""Times the map warps (GridMap.warp_from, SLAMParticleMaps.warp_into; gridmapslam.h "map warps") with op REPLACE and COMPARE, both
with the class-pair counts, in five cases -- 2048^2 -> 2048^2 cells at the identity and under a 0.3 rad turn, 2048^2 at 2 cm ->
1024^2 at 4 cm, 120^2 -> 2048^2, and 500 successive particles of a gms_slam of 120^2 cells into one 2048^2 map (the rectangle their
maps cover) -- beside gms_map_copy on the same 2048^2 handle as the yardstick: the copy moves logData AND likelihoodData, four arrays'
worth of traffic, a REPLACE with counts reads the source and the destination and writes the destination, three.  Prints one JSON line
per figure and writes them all to the file given as the first argument (default profiles/warp_probe.json).  Needs a GPU; there is no
fallback.

Every figure is a host clock around calls that end in a wait on the stream: the median and the spread (min, max) of 7 timed calls
after two untimed ones, as tools/slam_align_probe.py takes them.  No time is a pass criterion."""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, synth  # noqa: E402

RESULTS = []


def timed(name, fn, reps=7, **extra):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    r = dict(figure=name, median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts), reps=reps, **extra)
    RESULTS.append(r)
    print(json.dumps(r), flush=True)
    return r


def grid(cells, res, pos):
    m = GridMap(cells * res - 0.4 * res, cells * res - 0.4 * res, res, pos)
    assert (m.W, m.H) == (cells, cells), (m.W, m.H)
    return m


def fill(m, seed):
    rng = np.random.default_rng(seed)
    m.upload_log(rng.choice([0.0, -0.4054651081081643, 0.8472978603872037], size=(m.H, m.W), p=[0.3, 0.5, 0.2]))


def pair(name, dst, src, pose, cells):
    for op in ("replace", "compare"):
        timed(f"{name}: {op}", lambda: dst.warp_from(src, pose[:2], c=pose[2], s=pose[3], op=op), cells=cells)


def about(theta, p):
    """a turn by theta that keeps the world point p where it is"""
    c, s = math.cos(theta), math.sin(theta)
    return (p[0] - (c * p[0] - s * p[1]), p[1] - (s * p[0] + c * p[1]), c, s)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warp_probe.json")
    big, twin = grid(2048, 0.05, (-51.2, -51.2)), grid(2048, 0.05, (-51.2, -51.2))
    fill(big, 1); fill(twin, 2)
    big.compute_likelihood_map(); twin.compute_likelihood_map()

    def copy():
        big.copy_from(twin)
        big.synchronize()
    yard = timed("2048^2: gms_map_copy (logData and likelihoodData)", copy, cells=2048 * 2048)
    pair("2048^2 -> 2048^2, identity", big, twin, (0.0, 0.0, 1.0, 0.0), 2048 * 2048)
    pair("2048^2 -> 2048^2, 0.3 rad about the middle", big, twin, about(0.3, (0.0, 0.0)), 2048 * 2048)
    fine, coarse = grid(2048, 0.02, (-20.48, -20.48)), grid(1024, 0.04, (-20.48, -20.48))
    fill(fine, 3)
    pair("2048^2 at 2 cm -> 1024^2 at 4 cm", coarse, fine, (0.0, 0.0, 1.0, 0.0), 1024 * 1024)
    small = grid(120, 0.05, (-3.0, -3.0))
    fill(small, 4)
    pair("120^2 -> 2048^2, whole destination", big, small, about(0.3, (0.0, 0.0)), 2048 * 2048)
    n = 500
    tr = synth.make_trace(6.0, 0.05, 90, T=8, seed=7)
    s = SLAMParticleMaps(6.0, 6.0, 0.05, (-3.0, -3.0), num_particles=n, max_beams=128)
    for t in range(3):
        s.set_poses(synth.make_particles(tr.poses[t], n, seed=4 + t, sigma_xy=0.05, sigma_theta_deg=3.0))
        s.update(tr.scans[t], None)
    pose = about(0.3, (0.0, 0.0))
    rect = (1024 - 90, 1024 - 90, 180, 180)                                    # what a 120^2 map turned by 0.3 rad covers around the middle
    where = "500 particles of 120^2 -> one 2048^2 map, rectangle 180 x 180"

    def replace_all():
        for k in range(n):
            s.warp_into_dev(big, None, k, pose[:2], c=pose[2], s=pose[3], op="replace", rect=rect)
        big.synchronize()

    def compare_all():
        for k in range(n):
            s.warp_into(big, k, pose[:2], c=pose[2], s=pose[3], op="compare", rect=rect)
    timed(f"{where}: replace, device form without counts, all 500 and one wait", replace_all, cells=n * 180 * 180)
    timed(f"{where}: compare, host form with counts, all 500, a wait each", compare_all, cells=n * 180 * 180)
    for r in RESULTS[1:5]:
        r["ratio_to_copy"] = r["median_us"] / yard["median_us"]
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
    s.close(); small.close(); fine.close(); coarse.close(); big.close(); twin.close()
