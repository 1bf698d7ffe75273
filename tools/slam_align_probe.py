"""Times the update of a per-particle-map filter (SLAMParticleMaps.update_dev) with the per-particle scan alignment on
(gms_slam_set_align) at iters = 1, 4 and 8 in both forms of the field (GMS_SLAM_ALIGN_FIELD=planes|memory), beside the plain and the
lattice-refined update (gms_slam_set_refine) from the same run, at 500 particles x 120^2 cells x 90 beams (the reference's operating
point) and 4096 x 256^2 x 90.  Prints one JSON line per figure and writes them all to the file given as the first argument (default
profiles/slam_align_probe.json).  A library without gms_slam_set_align (the parent commit) gives the plain and the refined figures
alone, so the same script measures both sides.  Needs a GPU; there is no fallback.

Every figure is a host clock around a call that ends in a wait on the stream: the median and the spread (min, max) of 7 timed calls
after two untimed ones, as tools/align_probe.py takes them.  Every call updates the maps, so the seven calls are seven consecutive
frames of the filter (sample_motion off, the same scan); eps_t = eps_r = 0, so no pose stops early: iters + 1 evaluations each."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from gridmap_slam_robot_amd import AlignParams, SLAMParticleMaps, synth  # noqa: E402

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


def shape(n, ext, B):
    where = f"{n} x {int(round(ext / 0.05))}^2 x {B} beams"
    tr = synth.make_trace(min(ext, 6.4), 0.05, B, T=8, seed=7)
    have_align = hasattr(SLAMParticleMaps, "set_align")
    for form in ("planes", "memory") if have_align else ("none",):
        os.environ["GMS_SLAM_ALIGN_FIELD"] = form
        s = SLAMParticleMaps(ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
        for t in range(3):
            s.set_poses(synth.make_particles(tr.poses[t], n, seed=4 + t, sigma_xy=0.05, sigma_theta_deg=3.0))
            s.update(tr.scans[t], None)
        scan = tr.scans[3]
        d_scan = torch.from_numpy(scan.view(np.uint8).copy()).to("cuda")
        start = synth.make_particles(tr.poses[3], n, seed=9, sigma_xy=0.05, sigma_theta_deg=3.0)

        def step():
            s.update_dev(d_scan.data_ptr(), len(scan), None)
            s.grid_map.synchronize()
        if form != "memory":                                                   # (the plain and the refined update do not depend on the form)
            s.set_poses(start)
            timed(f"{where}: update, plain", step)
            s.set_refine(True); s.set_poses(start)
            timed(f"{where}: update, lattice refinement (1210 poses per particle)", step)
            s.set_refine(False)
        for iters in (1, 4, 8) if have_align else ():
            s.set_align(AlignParams(iters=iters, eps_t=0.0, eps_r=0.0)); s.set_poses(start)
            r = timed(f"{where}: update, alignment iters = {iters}, field form {form}", step)
            r["form_ran"] = s.align_form()                                     # (read behind the launches; the printed line does not carry it)
        s.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slam_align_probe.json")
    shape(500, 6.0, 90)
    shape(4096, 12.8, 90)
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
