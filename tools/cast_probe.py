"""Times the predicted scans (gms_map_cast, gms_slam_cast) against the route that existed before them: download the map's doubles and
walk the rays on the host.  Prints one JSON line per figure and writes them all to the file given as the first argument (default
cast_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around work that ends in a device synchronise: the median and the spread (min, max) of `reps` timed
calls after two untimed ones, the device forms in batches of `inner` launches per synchronise.  The host route is download_log (or
map_of) plus the oracle's C walk driven per ray from Python, first occupied cell picked in numpy -- it is what a caller of the parent
commit can do with the package, not a tuned host implementation; its download part is reported separately."""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import _cast_expect as ce  # noqa: E402
from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

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


def dev_bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def fan(B, reach):
    ang = np.arange(B) * (2 * math.pi / B)
    return ce.probes_from(reach * np.cos(ang), reach * np.sin(ang))


def shared_map(form):
    """C3: 2048 x 2048 cells at 2 cm, probes of 10 m"""
    cfg = synth.CONFIGS["C3"]
    ext, res, B = cfg["extent"], cfg["resolution"], cfg["beams"]
    if form == "mem":
        os.environ["GMS_CAST_WALK"] = "mem"
    m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    os.environ.pop("GMS_CAST_WALK", None)
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    probes = fan(B, 10.0)
    pose = tr.poses[4]
    d_probes, d_pose = dev_bytes(probes), dev_bytes(np.asarray(pose, np.float32))
    out = torch.empty(B * 16, dtype=torch.uint8, device="cuda")
    sync = m.synchronize
    timed(f"C3 1 pose x {B} probes, {form} form, plane kept (device form)", lambda: m.cast_dev(d_pose.data_ptr(), 1, d_probes.data_ptr(), B, out),
          inner=50, sync=sync)
    def rebuilt():
        m.upload_log(log)                      # (marks the plane stale; the upload itself is timed below and subtracted by the reader)
        m.cast_dev(d_pose.data_ptr(), 1, d_probes.data_ptr(), B, out)
    log = m.download_log()
    timed(f"C3 upload_log alone (the plane's invalidation in the next figure)", lambda: m.upload_log(log), reps=5, sync=sync)
    timed(f"C3 upload_log + 1 pose x {B} probes, {form} form, plane rebuilt", rebuilt, reps=5, sync=sync)
    timed(f"C3 1 pose x {B} probes, {form} form, host form (stages, reads back, synchronises)", lambda: m.cast(pose, probes))
    if form == "lds":
        P = cfg["particles"]
        poses = synth.make_particles(pose, P, sigma_xy=0.1, sigma_theta_deg=5.0)
        d_poses = dev_bytes(poses)
        big = torch.empty(P * B * 16, dtype=torch.uint8, device="cuda")
        timed(f"C3 {P} poses x {B} probes (device form)", lambda: m.cast_dev(d_poses.data_ptr(), P, d_probes.data_ptr(), B, big), reps=7, inner=3, sync=sync)
        # the route of the parent commit: W * H doubles to the host, then the walk there
        g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
        timed("C3 download_log alone (32 MiB)", lambda: m.download_log(), reps=5)
        host = timed(f"C3 download_log + host walk of 1 pose x {B} probes", lambda: ce.expect(g, m.download_log(), probes, pose), reps=3)
        got = m.cast(pose, probes)[0]
        assert np.array_equal(got, ce.expect(g, m.download_log(), probes, pose)), "the timed cast and the host route disagree"
        host["equal_to_device"] = True
    m.close()


def per_particle(n, ext, B, reps):
    res = 0.05
    s = SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=max(B, 64))
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    s.set_poses(np.tile(tr.poses[0], (n, 1)))
    for k in range(3):
        s.update(tr.scans[k], (0.02, 0.1), seed=3, sequence=k)
    probes = fan(B, 0.4 * ext)
    d_probes = dev_bytes(probes)
    out = torch.empty(n * B * 16, dtype=torch.uint8, device="cuda")
    W = s.W
    timed(f"GMS_CAST_ALL {n} x {W}^2 x {B} (device form)", lambda: s.cast((d_probes.data_ptr(), B), "all", out=out), reps=reps, inner=5,
          sync=s.grid_map.synchronize)
    timed(f"strongest of {n} x {W}^2 x {B} (device form)", lambda: s.cast((d_probes.data_ptr(), B), "strongest", out=out), reps=reps, inner=20,
          sync=s.grid_map.synchronize)
    g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
    timed(f"map_of(0) + host walk of ONE particle x {B} probes ({n} x {W}^2; all particles: x {n}, {n * W * W * 8 / 1e6:.0f} MB of downloads)",
          lambda: ce.expect(g, s.map_of(0), probes, s.get_particles()[0][0]), reps=3)
    s.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else "cast_probe.json"
    shared_map("lds")
    shared_map("mem")
    per_particle(500, 6.0, 90, 7)
    per_particle(4096, 12.8, 180, 5)
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
