"""Times the pose modes (gms_pf_modes_dev) of filters of 16 384 / 65 536 / 2^20 particles on a 2048 x 2048 map -- scattered over the whole
map, and again after ten fused scan steps -- next to the cheapest path a caller had before it: get_poses + get_weights with their
synchronise alone, no clustering at all.  bin_cells = 25, n_theta = 36, cap = 64 records.  Prints one JSON line per figure and writes
them all to the file given as the first argument (default profiles/modes_probe.json).  Needs a GPU; there is no fallback.

Every figure is a host clock around a call that ends in its own wait on the stream: the median and the spread (min, max) of 7 timed
calls after two untimed ones, as tools/scatter_probe.py takes them."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _modes_expect as mx  # noqa: E402
from gridmap_slam_robot_amd import GridMap, ParticleFilter, synth  # noqa: E402
from gridmap_slam_robot_amd._lib import MODE_DTYPE  # noqa: E402

RESULTS = []
BIN_CELLS, N_THETA, CAP = 25, 36, 64


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
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=16, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    beams = [torch.from_numpy(tr.scans[t].view(np.uint8).copy()).to("cuda") for t in range(4, 14)]
    rng = np.random.default_rng(2048)
    for n in (16384, 65536, 1 << 20):
        pf = ParticleFilter(m, n)
        pf.scatter(seed=1, sequence=1 << 32)
        d_rec = torch.zeros(CAP * MODE_DTYPE.itemsize // 8, dtype=torch.int64, device="cuda")
        d_lab = torch.zeros(n, dtype=torch.int32, device="cuda")
        for state in ("scattered whole", "after ten steps"):
            if state == "after ten steps":
                for k, t in enumerate(range(4, 14)):
                    d = tr.poses[t] - tr.poses[t - 1]
                    pf.slam_update_u_dev(float(np.hypot(d[0], d[1])), float(d[2]), 3, k, beams[k].data_ptr(), B, rng.random(), 0.5, False)
                m.synchronize()
            found = pf.modes(BIN_CELLS, N_THETA, records_out=d_rec, labels_out=d_lab)
            dev = timed(f"2048^2 modes_dev, {n} particles, {state}: labels and {CAP} records",
                        lambda: pf.modes(BIN_CELLS, N_THETA, records_out=d_rec, labels_out=d_lab), n_found=found[0], n_outside=found[1])
            timed(f"2048^2 modes_dev, {n} particles, {state}: labels alone (no sums)",
                  lambda: pf.modes(BIN_CELLS, N_THETA, labels_out=d_lab))
            h = timed(f"2048^2 bare download, {n} particles, {state}: get_poses + get_weights, no clustering",
                      lambda: (pf.get_poses(), pf.get_weights()))
            h["over_modes_dev"] = h["median_us"] / dev["median_us"]
            if n == 16384:
                # the timed code is the tested code: the first records against the expectation
                poses = pf.get_poses()
                th = np.ascontiguousarray(poses[:, 2])
                trig = np.stack([m.debug_f32(1, th), m.debug_f32(2, th)], axis=-1)
                want, want_lab, _ = mx.expect(poses, pf.get_weights(), trig, m.position, res, m.W, m.H, BIN_CELLS, N_THETA, cap=4)
                got = d_rec.cpu().numpy().view(MODE_DTYPE)
                assert found[0] == len(want) and np.array_equal(d_lab.cpu().numpy().view(np.uint32), want_lab), "labels and the expectation disagree"
                assert got[:min(4, len(want))].tobytes() == want[:min(4, len(want))].tobytes(), "records and the expectation disagree"
        pf.close()
    m.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "modes_probe.json")
    main()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
