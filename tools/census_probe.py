"""Times the census of the particles' maps (SLAMParticleMaps.census_dev; gridmapslam.h "census of the particles' maps") at 500 x 120^2
and 4096 x 256^2 in three configurations -- the counts alone, with the consensus and the totals, and with the agreement as well --
beside two yardsticks.  Prints one JSON line per figure and writes them all to the file given as the first argument (default
profiles/census_probe.json).  Needs a GPU; there is no fallback.

  the census       host clock around census_dev + a wait on the stream: the median and the spread of 7 timed calls after two untimed ones
  a streaming read the time of n * cells * 8 bytes at the rate gms_slam_resample_maps' copy of logData reaches on the same handle in
                   the same run (its kernel, one array, bracketed by events: GMS_K_MAPCOPY; read + write = twice the bytes), the median
                   of 3 draws, an update between them
  what came before download_maps + the numpy expectation of tests/_census_expect.py at 500 x 120^2: ONE run, host clock; at 4096 x 256^2
                   the same figure scaled by the bytes, not run
No time is a pass criterion."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from gridmap_slam_robot_amd import SLAMParticleMaps, _lib, synth  # noqa: E402

RESULTS = []


def put(**r):
    RESULTS.append(r)
    print(json.dumps(r), flush=True)
    return r


def timed(name, fn, reps=7, **extra):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return put(figure=name, median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts), reps=reps, how="median of 7, host clock", **extra)


def case(n, cells_side, before):
    import torch
    ext = cells_side * 0.05
    tr = synth.make_trace(ext, 0.05, 90, T=8, seed=7)
    s = SLAMParticleMaps(ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=128)
    assert (s.W, s.H) == (cells_side, cells_side)
    cells = s.W * s.H
    nbytes = n * cells * 8
    where = f"{n} x {cells_side}^2"
    copy_us = []
    for t in range(3):
        s.set_poses(synth.make_particles(tr.poses[t], n, seed=4 + t, sigma_xy=0.05, sigma_theta_deg=3.0))
        s.update(tr.scans[t], None)
        s.grid_map.profile(1 << _lib.K_MAPCOPY)
        s.grid_map.profile_reset()
        s.resample(0.37)
        s.grid_map.synchronize()
        ms, launches = s.grid_map.profile_get()["mapcopy"]
        s.grid_map.profile(False)
        copy_us.append(ms * 1e3 / max(launches, 1))
    copy = statistics.median(copy_us)
    assert copy > 0, "the copy was not bracketed"
    rate = 2 * nbytes / (copy * 1e-6)
    yard = put(figure=f"{where}: a streaming read of the maps at the resampling copy's rate", us=copy / 2, copy_us=copy, copy_runs_us=copy_us,
               copy_bytes_per_s=rate, map_bytes=nbytes, how="median of 3 bracketed launches of the copy, one array")
    counts = torch.empty(cells, dtype=torch.int32, device="cuda")
    cons = torch.empty(cells, dtype=torch.uint8, device="cuda")
    agree = torch.empty(10 * n, dtype=torch.int32, device="cuda")
    totals = torch.empty(4, dtype=torch.int64, device="cuda")
    min_known = max(1, n // 10)

    def run(**kw):
        s.census_dev(min_known=min_known, **kw)
        s.grid_map.synchronize()
    for name, kw, passes in (("counts alone", dict(counts=counts), 1), ("counts, consensus and totals", dict(counts=counts, consensus=cons, totals=totals), 1),
                             ("with the agreement", dict(counts=counts, consensus=cons, totals=totals, agree=agree), 2)):
        r = timed(f"{where}: census, {name}", lambda: run(**kw), passes_over_the_maps=passes)
        r["ratio_to_streaming_read_per_pass"] = r["median_us"] / passes / yard["us"]
    if before:
        import _census_expect as cx
        t0 = time.perf_counter()
        want = cx.expect(s.maps(), min_known)
        us = (time.perf_counter() - t0) * 1e6
        put(figure=f"{where}: download_maps + numpy, every output", us=us, how="one run, host clock")
        put(figure="4096 x 256^2: download_maps + numpy, every output", us=us * (4096 * 256 * 256) / (n * cells), how="extrapolated by bytes from the run above, not run")
        run(counts=counts, consensus=cons, totals=totals, agree=agree)
        got = {"counts": counts.cpu().numpy().view(np.uint16).reshape(s.H, s.W, 2), "consensus": cons.cpu().numpy().reshape(s.H, s.W),
               "agree": agree.cpu().numpy().view(_lib.CENSUS_AGREE_DTYPE), "totals": totals.cpu().numpy().view(_lib.CENSUS_TOTALS_DTYPE)[0]}
        assert cx.same(got, want), "the timed call computes the expectation"
    s.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "census_probe.json")
    case(500, 120, True)
    case(4096, 256, False)
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
