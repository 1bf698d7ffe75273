"""Times the beam sensor model (gms_pf_score_beams_dev) on filters of 16 384 and 65 536 particles on a 2048 x 2048 map at 2 cm after a
few scans of the synthetic room, 720 beams, behind = ahead = 10 -- the cloud scattered over the whole map, and again after ten fused
scan steps -- next to gms_pf_score_dev at the same shape (the end-point model, for context) and to what a caller could do before:
gms_map_cast_dev over the same poses plus the read-back of its 16-byte records.  Prints one JSON line per figure and writes them all to
the file given as the first argument (default profiles/beams_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around a call that ends in a wait on the stream: the median and the spread (min, max) of 7 timed calls
after two untimed ones, as tools/modes_probe.py takes them.  `window_fits` is the share of 256 sampled particles whose plane window fits
the LDS the launch asks for; the others walk the plane in memory."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _beams_expect as bx  # noqa: E402
from gridmap_slam_robot_amd import GridMap, ParticleFilter, beam_model_factors, synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

RESULTS = []
BEHIND = AHEAD = 10


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
    ext, res, B = cfg["extent"], cfg["resolution"], cfg["beams"]
    m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    g = orc.Grid(ext, ext, res, -ext / 2, -ext / 2)
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=16, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    beams = [torch.from_numpy(tr.scans[t].view(np.uint8).copy()).to("cuda") for t in range(4, 15)]
    scan, d_scan = tr.scans[14], beams[10]
    factors = beam_model_factors(res, BEHIND, AHEAD, 0.04)
    asked = min(64 * 1024 // 4, 2048 * 64)
    rng = np.random.default_rng(2048)
    for n in (16384, 65536):
        pf = ParticleFilter(m, n)
        pf.scatter(seed=1, sequence=1 << 32)
        d_hits = torch.zeros(n * B * 2, dtype=torch.int64, device="cuda")          # n * B gms_cast_hit records of 16 bytes
        d_res = torch.zeros(n * B, dtype=torch.int16, device="cuda")
        for state in ("scattered whole", "after ten steps"):
            if state == "after ten steps":
                for k, t in enumerate(range(4, 14)):
                    d = tr.poses[t] - tr.poses[t - 1]
                    pf.slam_update_u_dev(float(np.hypot(d[0], d[1])), float(d[2]), 3, k, beams[k].data_ptr(), B, rng.random(), 0.5, False)
                m.synchronize()
            poses = pf.get_poses()
            d_poses = torch.from_numpy(poses).to("cuda")
            sample = poses[:: n // 256]
            fits = float(np.mean([0 < bx.window_words(g, scan, p, AHEAD) <= asked for p in sample]))
            where = f"2048^2, {B} beams, {n} particles, {state}"
            dev = timed(f"{where}: score_beams_dev, behind = ahead = {AHEAD}",
                        lambda: (pf.score_beams_dev(d_scan.data_ptr(), B, factors, BEHIND, AHEAD), m.synchronize()), window_fits=fits)
            timed(f"{where}: score_beams_dev with the residuals", lambda: (pf.score_beams_dev(d_scan.data_ptr(), B, factors, BEHIND, AHEAD, residuals_out=d_res), m.synchronize()))
            timed(f"{where}: gms_pf_score_dev (the end-point model)", lambda: (pf.score_dev(d_scan.data_ptr(), B), m.synchronize()))
            c = timed(f"{where}: gms_map_cast_dev over the same poses + the read-back of its records",
                      lambda: (m.cast_dev(d_poses.data_ptr(), n, d_scan.data_ptr(), B, d_hits), d_hits.cpu()))
            c["over_score_beams_dev"] = c["median_us"] / dev["median_us"]
            timed(f"{where}: gms_map_cast_dev alone (records left on the device)", lambda: (m.cast_dev(d_poses.data_ptr(), n, d_scan.data_ptr(), B, d_hits), m.synchronize()))
            if n == 16384:
                # the timed code is the tested code: the first particles against the expectation
                pf.score_beams_dev(d_scan.data_ptr(), B, factors, BEHIND, AHEAD, residuals_out=d_res)
                m.synchronize()
                w, lw, idx = bx.expect(g, m.download_log(), scan, poses[:8], factors, BEHIND, AHEAD)
                got = d_res[:8 * B].cpu().numpy().view(np.uint16).reshape(8, B)
                assert np.array_equal(got, idx) and bx.same_bits(pf.get_weights()[:8], w) and bx.same_bits(pf.get_log_weights()[:8], lw), "the device and the expectation disagree"
        pf.close()
    m.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "beams_probe.json")
    main()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
