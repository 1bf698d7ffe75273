"""Times sites and skeleton (gms_map_skeleton, gms_map_nearest_poses, gms_slam_skeleton) against the clearance field of the same
request and against the first step of the route a caller had before them: download_log of the same map, before any threshold, feature
transform or ridge test on the host.  Prints one JSON line per figure and writes them all to the file given as the first argument
(default profiles/skeleton_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around stream-ordered work that ends in a device synchronise: the median and the spread (min, max) of
`reps` timed batches after two untimed ones, the device forms in batches of `inner` launches per synchronise.  The last entry holds
the one condition the feature has: with the plane current, the full R = 25 call on 2048 x 2048 cells takes less time than download_log.
NOT measured here: R = 255, small rectangles, and the LDS bank-conflict counters."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import _skeleton_expect as xs  # noqa: E402
from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, _lib, synth  # noqa: E402

RESULTS = []


def timed(name, fn, reps=11, inner=1, sync=None, **extra):
    for _ in range(2):
        fn()
    if sync:
        sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) / inner * 1e6)
    r = dict(figure=name, median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts), reps=reps, inner=inner, **extra)
    RESULTS.append(r)
    print(json.dumps(r), flush=True)
    return r


def shared_map():
    """C3: 2048 x 2048 cells at 2 cm after four scans of the synthetic room (the clearance probe's map)"""
    cfg = synth.CONFIGS["C3"]
    ext, res, B = cfg["extent"], cfg["resolution"], cfg["beams"]
    m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    log = m.download_log()
    site = torch.empty(m.W * m.H, dtype=torch.int32, device="cuda")
    skel = torch.empty(m.W * m.H, dtype=torch.int16, device="cuda")
    tot = torch.empty(4, dtype=torch.int64, device="cuda")
    clear = torch.empty(m.W * m.H, dtype=torch.int16, device="cuda")
    sync = m.synchronize
    full = {}
    for R in (8, 25, 64):
        for not_free in (False, True):
            mode = "not free" if not_free else "occupied"
            kw = dict(max_radius=R, not_free=not_free)
            c = timed(f"2048^2 clearance_dev, R = {R}, {mode}, plane current", lambda: m.clearance_dev(clear, **kw), inner=20, sync=sync)
            s = timed(f"2048^2 skeleton_dev, site only, R = {R}, {mode}, plane current", lambda: m.skeleton_dev(site, **kw), inner=20, sync=sync)
            a = timed(f"2048^2 skeleton_dev, site + skel + totals, R = {R}, {mode}, plane current", lambda: m.skeleton_dev(site, skel, tot, **kw),
                      inner=20, sync=sync)
            s["ratio_to_clearance"] = s["median_us"] / c["median_us"]
            a["ratio_to_clearance"] = a["median_us"] / c["median_us"]
            full[R, not_free] = a
    sync()
    rect = (928, 960, 96, 64)                               # (the last request: R = 64, not free)
    got_site = site.cpu().numpy().view(np.uint32).reshape(m.H, m.W)
    got_skel = skel.cpu().numpy().view(np.uint16).reshape(m.H, m.W)
    assert np.array_equal(xs.cut(got_site, rect), xs.cut(xs.sites(log, 64, True, rect=rect), rect)), "the timed sites and the brute-force expectation disagree"
    assert np.array_equal(got_skel, xs.skeleton(got_site)), "the timed skeleton and the three rules on the timed sites disagree"
    assert xs.totals_of(tot.cpu().numpy().view(_lib.SKELETON_TOTALS_DTYPE)[0]) == xs.totals(got_site, got_skel), "the timed totals"
    assert np.array_equal(xs.clearance_of(got_site), clear.cpu().numpy().view(np.uint16).reshape(m.H, m.W)), "sites against the clearance field"
    P = 16384
    rng = np.random.default_rng(1)
    poses = np.column_stack([rng.uniform(-ext / 2, ext / 2, (P, 2)), np.zeros(P)]).astype(np.float32)
    d_poses = torch.from_numpy(poses).to("cuda")
    out_p = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    for R in (8, 25, 64):
        timed(f"2048^2 nearest under {P} poses, R = {R} (device form)", lambda: m.nearest_poses_dev(d_poses.data_ptr(), P, out_p, max_radius=R),
              inner=20, sync=sync)
    sync()
    s64, d64 = xs.expect_poses(m.skeleton(max_radius=64, skel=False, totals=False)[0], poses, -ext / 2, -ext / 2, res)
    got_p = out_p.cpu().numpy().view(np.uint32).reshape(P, 2)
    assert np.array_equal(got_p[:, 0], s64) and np.array_equal(got_p[:, 1], d64), "poses against the field"
    down = timed("2048^2 download_log alone (32 MiB): the parent commit's route before any host transform", lambda: m.download_log(), reps=7)
    f25 = full[25, False]
    cond = dict(figure="condition: full R = 25 call with the plane current < download_log alone", skeleton_us=f25["median_us"], download_us=down["median_us"],
                holds=bool(f25["max_us"] < down["min_us"]), ratio=down["median_us"] / f25["median_us"])
    RESULTS.append(cond)
    print(json.dumps(cond), flush=True)
    m.close()


def per_particle(n=500, ext=6.0, B=90):
    res = 0.05
    s = SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    for k in range(3):
        s.update(tr.scans[k], (0.02, 0.1), seed=3, sequence=k)
    site = torch.empty(s.W * s.H, dtype=torch.int32, device="cuda")
    skel = torch.empty(s.W * s.H, dtype=torch.int16, device="cuda")
    tot = torch.empty(4, dtype=torch.int64, device="cuda")
    for R in (8, 25):
        for not_free in (False, True):
            timed(f"strongest of {n} x {s.W}^2, R = {R}, {'not free' if not_free else 'occupied'} (device form: pre-pass + sites + ridge)",
                  lambda: s.skeleton("strongest", max_radius=R, not_free=not_free, dev=(site, skel, tot)), inner=20, sync=s.grid_map.synchronize)
    timed(f"map_of(0) alone ({s.W}^2 doubles): the parent commit's route before any host transform", lambda: s.map_of(0))
    got = s.skeleton("strongest", max_radius=8)
    want = xs.sites(s.map_of(got[3]), 8)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], xs.skeleton(want)), "the timed call and the brute-force expectation disagree"
    s.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "skeleton_probe.json")
    shared_map()
    per_particle()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
