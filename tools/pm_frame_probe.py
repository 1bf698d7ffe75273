"""What one frame call costs against the calls it stands for, for the filter with a map per particle.

  (a) SLAMParticleMaps.frame (gms_slam_frame_per_particle): de-skew, update(z, u), resample_if as ONE call, against
  (b) the three calls gms_map_deskew -> gms_slam_update_per_particle_dev -> gms_slam_resample_maps_if,
      on ONE handle, regions of (a) and (b) alternating in the same process, at 500 x 120^2 x 90 beams and 4096 x 256^2 x 180;
  (c) SLAMParticleMapsBatch.frame (gms_slam_frame_batch) for S = 4 and 16 filters of 500 x 120^2 x 90, against what a caller had to
      write before it: S gms_map_deskew calls on a scratch map, each de-skewed revolution copied device-to-device into its row of an
      [S][B] block, then gms_slam_update_batch_dev and gms_slam_resample_maps_if_batch -- again alternating on one handle.

Raw revolutions from host memory every step on both sides (a synthetic recording, cycled), nothing read back inside a region; every
figure is microseconds per step, the median of REGIONS regions of STEPS steps between device synchronisations, with the regions' min
and max beside it.  Prints one JSON document and writes it to the path given as the first argument."""
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

from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, SLAMParticleMapsBatch, synth  # noqa: E402
from gridmap_slam_robot_amd._lib import check, load  # noqa: E402

STEPS, REGIONS, WARMUP = 40, 7, 5
SCALAR = [("500x120^2x90", 500, 6.0, 90), ("4096x256^2x180", 4096, 12.8, 180)]
BATCH = [4, 16]
SEED, FRACTION, R01 = 2024, 0.5, 0.37


class _DeviceBytes:
    """a device address as something torch.as_tensor takes"""

    def __init__(self, address: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (address, False), "version": 2}


def _alternate(step_a, step_b, sync):
    """regions of step_a and step_b in turn; returns the two lists of microseconds per step"""
    for k in range(WARMUP):
        step_a(k); step_b(k)
    a, b = [], []
    for _ in range(REGIONS):
        for step, out in ((step_a, a), (step_b, b)):
            sync()
            t0 = time.perf_counter()
            for k in range(STEPS):
                step(k)
            sync()
            out.append((time.perf_counter() - t0) / STEPS * 1e6)
    return a, b


def _summary(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def scalar_row(name, n, ext, B, stream, sync):
    frames, _ = synth.make_recording(ext, B, T=48, seed=77, n_frames=8)
    start = synth.true_pose(synth.make_world(ext, 77), -1, 48)
    dev = SLAMParticleMaps(ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=B)
    check(load().gms_map_set_stream(dev.grid_map._h, stream))
    dev.set_poses(np.tile(start.astype(np.float32), (n, 1)))
    seq = [0]

    def one_call(k):
        f = frames[k % len(frames)]
        dev.frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, seed=SEED, sequence=seq[0], r01=R01, fraction=FRACTION)
        seq[0] += 1

    def three_calls(k):
        f = frames[k % len(frames)]
        d, nb = dev.grid_map.deskew_dev(f.angle, f.distance, f.hit, f.d_center, f.d_theta)
        dev.update_dev(d, nb, (f.d_center, f.d_theta), seed=SEED, sequence=seq[0])
        dev.resample_if(R01, FRACTION)
        seq[0] += 1

    a, b = _alternate(one_call, three_calls, sync)
    dev.close()
    return {"config": name, "particles": n, "beams": B, "one_call_frame": _summary(a), "three_calls": _summary(b),
            "one_call_over_three_calls": round(statistics.median(a) / statistics.median(b), 4)}


def batch_row(S, stream, sync):
    n, ext, B = 500, 6.0, 90
    recs = [synth.make_recording(ext, B, T=48, seed=77 + 13 * f, n_frames=8)[0] for f in range(S)]
    starts = np.stack([synth.true_pose(synth.make_world(ext, 77 + 13 * f), -1, 48) for f in range(S)]).astype(np.float32)
    bat = SLAMParticleMapsBatch(S, ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=B)
    scratch = GridMap(ext, ext, 0.05, (-ext / 2, -ext / 2), max_beams=B)
    L = load()
    check(L.gms_map_set_stream(bat.grid_map._h, stream))
    check(L.gms_map_set_stream(scratch._h, stream))
    bat.set_poses(np.ascontiguousarray(np.broadcast_to(starts[:, None, :], (S, n, 3))))
    seeds = np.arange(1, S + 1, dtype=np.uint64)
    r01 = np.full(S, R01)
    T = len(recs[0])
    raw = [(np.stack([recs[f][k].angle for f in range(S)]), np.stack([recs[f][k].distance for f in range(S)]),
            np.stack([recs[f][k].hit for f in range(S)]), np.array([(recs[f][k].d_center, recs[f][k].d_theta) for f in range(S)])) for k in range(T)]
    block = torch.zeros((S, B * 32), dtype=torch.uint8, device="cuda")
    seq = [0]

    def one_call(k):
        a, d, h, odo = raw[k % T]
        bat.frame(a, d, h, odo, seeds=seeds, sequence=seq[0], r01=r01, fraction=FRACTION)
        seq[0] += 1

    def glue(k):
        a, d, h, odo = raw[k % T]
        for f in range(S):
            ptr, nb = scratch.deskew_dev(a[f], d[f], h[f], odo[f, 0], odo[f, 1])
            block[f].copy_(torch.as_tensor(_DeviceBytes(ptr, nb * 32), device="cuda"), non_blocking=True)
        bat.update_dev(block.data_ptr(), B, None, odo, seeds, seq[0])
        bat.resample_if(r01, FRACTION)
        seq[0] += 1

    a, b = _alternate(one_call, glue, sync)
    bat.close(); scratch.close()
    return {"config": f"{S} x 500x120^2x90", "S": S, "particles_per_filter": n, "beams": B, "frame_batch": _summary(a),
            "deskew_per_filter_then_batch_calls": _summary(b), "frame_batch_over_glue": round(statistics.median(a) / statistics.median(b), 4),
            "frame_batch_us_per_filter": round(statistics.median(a) / S, 2)}


def main():
    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    sync = torch.cuda.synchronize
    doc = {"tool": "tools/pm_frame_probe.py", "device": torch.cuda.get_device_name(0), "steps_per_region": STEPS, "regions": REGIONS,
           "statistic": "microseconds per step (host clock around STEPS steps ending in a device synchronise): median, min and max of the regions; "
                        "the two sides' regions alternate on one handle in one process; raw revolutions from host memory every step",
           "resample_fraction": FRACTION, "scalar": [], "batch": []}
    for name, n, ext, B in SCALAR:
        r = scalar_row(name, n, ext, B, stream, sync)
        doc["scalar"].append(r)
        print(json.dumps(r), flush=True)
    for S in BATCH:
        r = batch_row(S, stream, sync)
        doc["batch"].append(r)
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
