"""Batched reference-shape filters (SLAMParticleMapsBatch: S filters in one gms_slam handle) against S stand-alone handles run back to
back on one stream, per filter: one update, and one update + resample_if, at 500 x 120^2 x 90 beams (refinement off and on) and at
100 x 64^2 x 90, for S in {1, 4, 16, 64}.  The S = 1 rows compare the batch entry points with the scalar ones.  Device inputs on both
sides (update_dev: the scans are staged once), every figure the median of REGIONS regions of STEPS steps between device
synchronisations.  Prints one JSON document (and writes it to the path given as the first argument)."""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gridmap_slam_robot_amd import SLAMParticleMaps, SLAMParticleMapsBatch, synth  # noqa: E402
from gridmap_slam_robot_amd._lib import check, load  # noqa: E402

STEPS, REGIONS, WARMUP = 20, 5, 3
CONFIGS = [("500x120^2x90", 500, 6.0, 90, False), ("500x120^2x90_refine", 500, 6.0, 90, True), ("100x64^2x90", 100, 3.2, 90, False)]
SIZES = [1, 4, 16, 64]


def _region(step, sync):
    for _ in range(WARMUP):
        step(0)
    sync()
    out = []
    for _ in range(REGIONS):
        sync()
        t0 = time.perf_counter()
        for k in range(STEPS):
            step(k)
        sync()
        out.append((time.perf_counter() - t0) / STEPS * 1e6)
    return statistics.median(out)


def run_config(name, n, ext, B, refine, S, stream):
    res = 0.05
    L = load()
    tr = synth.make_trace(ext, res, B, T=4, seed=21)
    beams = torch.from_numpy(np.ascontiguousarray(np.stack([tr.scans[1]] * S)).view(np.uint8)).cuda()
    odo = np.tile([0.02, 0.01], (S, 1))
    seeds = np.arange(1, S + 1, dtype=np.uint64)
    P0 = synth.make_particles(tr.poses[1], n * S, seed=4, sigma_xy=0.03, sigma_theta_deg=1.0)
    sync = torch.cuda.synchronize
    r01 = np.full(S, 0.37)

    bat = SLAMParticleMapsBatch(S, ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=B)
    check(L.gms_map_set_stream(bat.grid_map._h, stream))
    bat.set_refine(refine)

    def setup_b():
        bat.reset(); bat.set_poses(P0)
    setup_b()
    upd_b = _region(lambda k: bat.update_dev(beams.data_ptr(), B, None, odo, seeds, k), sync)
    setup_b()
    res_b = _region(lambda k: (bat.update_dev(beams.data_ptr(), B, None, odo, seeds, k), bat.resample_if(r01, 0.5)), sync)
    bat.close()

    alone = [SLAMParticleMaps(ext, ext, res, (-ext / 2, -ext / 2), num_particles=n, max_beams=B) for _ in range(S)]
    for f, a in enumerate(alone):
        check(L.gms_map_set_stream(a.grid_map._h, stream))
        a.set_refine(refine)
        a.reset(); a.set_poses(P0[f * n:(f + 1) * n])
    row = beams.data_ptr()

    def upd_a(k):
        for f, a in enumerate(alone):
            a.update_dev(row, B, (0.02, 0.01), seed=f + 1, sequence=k)

    def both_a(k):
        for f, a in enumerate(alone):
            a.update_dev(row, B, (0.02, 0.01), seed=f + 1, sequence=k)
            a.resample_if(0.37, 0.5)
    upd_s = _region(upd_a, sync)
    for f, a in enumerate(alone):
        a.reset(); a.set_poses(P0[f * n:(f + 1) * n])
    res_s = _region(both_a, sync)
    for a in alone:
        a.close()
    return {"config": name, "S": S, "particles_per_filter": n, "beams": B, "refine": refine,
            "batched_update_us": round(upd_b, 2), "batched_update_resample_if_us": round(res_b, 2),
            "standalone_update_us": round(upd_s, 2), "standalone_update_resample_if_us": round(res_s, 2),
            "batched_update_us_per_filter": round(upd_b / S, 2), "standalone_update_us_per_filter": round(upd_s / S, 2),
            "batched_update_resample_if_us_per_filter": round(res_b / S, 2),
            "standalone_update_resample_if_us_per_filter": round(res_s / S, 2),
            "update_speedup": round(upd_s / upd_b, 3), "update_resample_if_speedup": round(res_s / res_b, 3)}


def main():
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for name, n, ext, B, refine in CONFIGS:
        for S in SIZES:
            r = run_config(name, n, ext, B, refine, S, stream)
            rows.append(r)
            print(json.dumps(r), flush=True)
    doc = {"tool": "tools/pm_batch_probe.py", "device": torch.cuda.get_device_name(0), "steps_per_region": STEPS, "regions": REGIONS,
           "statistic": "median of the regions, device-synchronised wall clock, microseconds per step (all S filters)",
           "note": "standalone = S SLAMParticleMaps handles on one stream, called back to back; S = 1 rows: batch entry points vs scalar ones",
           "rows": rows}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps({"rows": len(rows)}))


if __name__ == "__main__":
    main()
