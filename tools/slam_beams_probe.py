"""Times the per-particle beam sensor model (gms_slam_score_beams, gms_slam_set_beam_model): the update of a per-particle-map filter
(SLAMParticleMaps.update_dev) with the model off, with MULTIPLY and with REPLACE, and the stand-alone call in its device form with the
window packed into LDS and with every bit read from memory (GMS_CAST_WALK=mem), at 500 particles x 120^2 cells x 90 beams (the
reference's operating point) and 4096 x 256^2 x 180.  Prints one JSON line per figure and writes them all to the file given as the
first argument (default profiles/slam_beams_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around a call that ends in a wait on the stream: the median and the spread (min, max) of 9 timed calls
after three untimed ones.  Every update integrates its scan, so the timed calls are consecutive frames of the filter (sample_motion
off, the same scan); the stand-alone call changes nothing and is simply repeated.  staged_bytes: what the staging of one particle
reads for this scan at the filter's mean pose, rows x 64-cell units x 512 bytes."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from gridmap_slam_robot_amd import SLAMParticleMaps, beam_model_factors, synth  # noqa: E402

RESULTS = []
BEHIND, AHEAD = 6, 4


def timed(name, fn, reps=9, **extra):
    for _ in range(3):
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


def staged_bytes(s, scan, pose):
    """the window of one particle at `pose` (the box of the scan's end points and the pose, padded by AHEAD + 1, clipped to the map)
    in 64-cell units of 512 bytes"""
    c, sn = np.cos(pose[2]), np.sin(pose[2])
    px, py = s.grid_map.position
    x = np.append((pose[0] + c * scan["local_x"] - sn * scan["local_y"] - px) / 0.05, (pose[0] - px) / 0.05)
    y = np.append((pose[1] + sn * scan["local_x"] + c * scan["local_y"] - py) / 0.05, (pose[1] - py) / 0.05)
    x0, x1 = max(0, int(np.floor(x.min())) - AHEAD - 1), min(s.W - 1, int(np.floor(x.max())) + AHEAD + 1)
    y0, y1 = max(0, int(np.floor(y.min())) - AHEAD - 1), min(s.H - 1, int(np.floor(y.max())) + AHEAD + 1)
    words = (x1 >> 5) - (x0 >> 5) + 1
    return int((y1 - y0 + 1) * ((words + 1) // 2) * 512)


def shape(n, ext, B):
    where = f"{n} x {int(round(ext / 0.05))}^2 x {B} beams"
    tr = synth.make_trace(min(ext, 6.4), 0.05, B, T=8, seed=7)
    factors = beam_model_factors(0.05, BEHIND, AHEAD, 0.05)
    scan = tr.scans[3]
    d_scan = torch.from_numpy(scan.view(np.uint8).copy()).to("cuda")
    start = synth.make_particles(tr.poses[3], n, seed=9, sigma_xy=0.05, sigma_theta_deg=3.0)
    for walk in ("lds", "mem"):
        os.environ.pop("GMS_CAST_WALK", None)
        if walk == "mem":
            os.environ["GMS_CAST_WALK"] = "mem"
        s = SLAMParticleMaps(ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=max(128, B))
        os.environ.pop("GMS_CAST_WALK", None)
        for t in range(3):
            s.set_poses(synth.make_particles(tr.poses[t], n, seed=4 + t, sigma_xy=0.05, sigma_theta_deg=3.0))
            s.update(tr.scans[t], None)
        s.set_poses(start)
        per = staged_bytes(s, scan, tr.poses[3])

        def call():
            s.score_beams_dev(d_scan.data_ptr(), len(scan), factors, BEHIND, AHEAD)
            s.grid_map.synchronize()
        timed(f"{where}: stand-alone call, bits from {'the LDS window' if walk == 'lds' else 'memory'}", call, staged_bytes=per if walk == "lds" else 0)
        if walk == "mem":
            s.close()
            continue

        def step():
            s.update_dev(d_scan.data_ptr(), len(scan), None)
            s.grid_map.synchronize()
        timed(f"{where}: update, model off", step)
        for combine in ("multiply", "replace"):
            s.set_beam_model(factors, BEHIND, AHEAD, combine=combine); s.set_poses(start)
            timed(f"{where}: update, model {combine}", step, staged_bytes=per)
        s.set_beam_model(None); s.set_poses(start)
        timed(f"{where}: update, model off again", step)
        s.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slam_beams_probe.json")
    shape(500, 6.0, 90)
    shape(4096, 12.8, 180)
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
