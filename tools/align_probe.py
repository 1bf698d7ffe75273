"""Times continuous scan alignment (gms_pf_align_dev) on a filter of 16 384 particles on a 2048 x 2048 map at 2 cm after a few scans of
the synthetic room, 720 beams (config C3's shape), for iters = 1, 4 and 8, next to gms_pf_refine_poses (findBestPose's 1210 poses per
particle) and gms_pf_score_dev on the same filter.  Prints one JSON line per figure and writes them all to the file given as the first
argument (default profiles/align_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around a call that ends in a wait on the stream: the median and the spread (min, max) of 7 timed calls
after two untimed ones, as tools/beams_probe.py takes them.  The poses are set again in front of every call (inside the timed window:
gms_pf_set_poses_dev, one small launch, the same for all three), so every call starts from the same cloud; eps_t = eps_r = 0, so no
pose stops early and every figure is iters + 1 evaluations.  `lookups_per_pose`: 4 x B x (iters + 1) field values for the alignment
against 1210 x B for the lattice search."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _align_expect as ax  # noqa: E402
from gridmap_slam_robot_amd import AlignParams, GridMap, ParticleFilter, synth  # noqa: E402

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


def main():
    cfg = synth.CONFIGS["C3"]
    ext, res, B, n = cfg["extent"], cfg["resolution"], cfg["beams"], cfg["particles"]
    m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=16, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    scan = tr.scans[4]
    d_scan = torch.from_numpy(scan.view(np.uint8).copy()).to("cuda")
    start = synth.make_particles(tr.poses[4], n, seed=3, sigma_xy=0.03, sigma_theta_deg=1.5)
    d_start = torch.from_numpy(start).to("cuda")
    pf = ParticleFilter(m, n)
    where = f"2048^2 at 2 cm, {B} beams, {n} particles"

    def reset():
        pf.set_poses_dev(d_start.data_ptr())
    timed(f"{where}: set_poses_dev alone (inside every figure below)", lambda: (reset(), m.synchronize()))
    for iters in (1, 4, 8):
        prm = AlignParams(iters=iters, eps_t=0.0, eps_r=0.0)
        timed(f"{where}: gms_pf_align_dev, iters = {iters}", lambda: (reset(), pf.align_dev(d_scan.data_ptr(), B, prm), m.synchronize()),
              lookups_per_pose=4 * B * (iters + 1))
    timed(f"{where}: gms_pf_refine_poses (1210 poses per particle)", lambda: (reset(), pf.refine_poses(scan), m.synchronize()), lookups_per_pose=1210 * B)
    timed(f"{where}: gms_pf_score_dev", lambda: (reset(), pf.score_dev(d_scan.data_ptr(), B), m.synchronize()), lookups_per_pose=B)
    # the timed code is the tested code: the first particles against the restatement of the header's text
    prm = dict(ax.default_params(), iters=4, eps_t=0.0, eps_r=0.0)
    reset()
    rec = pf.align(scan, AlignParams(iters=4, eps_t=0.0, eps_r=0.0), records=True)
    want_p, want_r = ax.align(m.download_likelihood(), m.W, m.H, res, -ext / 2, -ext / 2, scan, start[:4], prm)
    assert np.array_equal(pf.get_poses()[:4].view(np.uint32), want_p.view(np.uint32)), "the device and the restatement disagree"
    assert np.array_equal(rec["score"][:4], want_r["score"]) and np.array_equal(rec["H"][:4], want_r["H"])
    reset()
    status, count = np.unique(pf.align(scan, AlignParams(iters=4), records=True)["status"], return_counts=True)
    RESULTS.append(dict(figure=f"{where}: statuses after iters = 4 with the default eps", **{str(k): int(v) for k, v in zip(status, count)}))
    print(json.dumps(RESULTS[-1]), flush=True)
    pf.close()
    m.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "align_probe.json")
    main()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
