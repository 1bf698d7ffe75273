"""Times global scan matching (gms_map_locate) on the flagship map: 2048 x 2048 cells at 2 cm after four scans of the synthetic room, the
fifth scan (720 beams) as the offset table at n_theta = 72 and 360, tol 2, cap 64, min_score half the beams that hit.  Three things
are timed per n_theta: the pruned search over the whole map, the pruned search over a 256 x 256 crop around the true pose, and the
same crop on a handle created with GMS_LOCATE_LEVELS=0 -- the exhaustive search on the device, the only like-for-like baseline that
exists.  At n_theta = 72 the numpy brute force of tests/_locate_expect.py runs on that crop too (once; its hit cells are handed to it,
dilated here with array shifts, so only the scoring and the ranking are timed), and all three must return the same records.
Prints one JSON line per figure and writes them all to the file given as the first argument (default profiles/locate_probe.json).
Needs a GPU; there is no fallback.

Every device figure is a host clock around a host-form call, which ends in a device synchronise: the median and the spread (min, max)
of 7 timed calls after two untimed ones, as tools/gain_probe.py takes them; levels and candidates evaluated per level come from
gms_map_locate_stats of the last call."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _locate_expect as lx  # noqa: E402
from gridmap_slam_robot_amd import GridMap, locate_offsets, synth  # noqa: E402

RESULTS = []
TOL, CAP, B = 2, 64, 720


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


def note(**kw):
    RESULTS.append(kw)
    print(json.dumps(kw), flush=True)


def handle(levels):
    cfg = synth.CONFIGS["C3"]
    ext, res = cfg["extent"], cfg["resolution"]
    old = os.environ.pop("GMS_LOCATE_LEVELS", None)
    if levels is not None:
        os.environ["GMS_LOCATE_LEVELS"] = str(levels)
    try:
        m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    finally:
        os.environ.pop("GMS_LOCATE_LEVELS", None)
        if old is not None:
            os.environ["GMS_LOCATE_LEVELS"] = old
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    return m, tr, ext, res


def dilate(obstacles, tol):
    """the cells within tol of an obstacle cell, by array shifts (the probe's own; the tests use the brute force)"""
    H, W = obstacles.shape
    out = np.zeros_like(obstacles)
    for dy in range(-tol, tol + 1):
        for dx in range(-tol, tol + 1):
            if dx * dx + dy * dy <= tol * tol:
                out[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= obstacles[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
    return out


def main():
    m, tr, ext, res = handle(None)
    m0, _, _, _ = handle(0)
    scan, pose = tr.scans[4], tr.poses[4]
    n_hit = int(scan["hit"].sum())
    min_score = max(1, n_hit // 2)
    cx, cy = int((float(pose[0]) + ext / 2) / res), int((float(pose[1]) + ext / 2) / res)
    crop = (min(max(cx - 128, 0), 2048 - 256), min(max(cy - 128, 0), 2048 - 256), 256, 256)
    note(figure="setup", map="2048^2 after four scans", beams=B, hit_beams=n_hit, tol=TOL, cap=CAP, min_score=min_score, true_cell=[cx, cy], crop=list(crop))
    log = m.download_log()
    for n_theta in (72, 360):
        off = locate_offsets(scan, n_theta, res)
        kw = dict(tol=TOL, min_score=min_score, cap=CAP, free_only=True)
        whole = timed(f"2048^2 pruned, n_theta {n_theta}, the whole map", lambda: m.locate(off, **kw))
        rec = m.locate(off, **kw)
        whole.update(m.locate_stats(), n_out=len(rec), best=[int(v) for v in rec[0]] if len(rec) else None)
        print(json.dumps(whole), flush=True)
        pruned = timed(f"256^2 crop pruned, n_theta {n_theta}", lambda: m.locate(off, rect=crop, **kw))
        got = m.locate(off, rect=crop, full=True, **kw)
        pruned.update(m.locate_stats())
        exhaustive = timed(f"256^2 crop exhaustive on the device (GMS_LOCATE_LEVELS=0), n_theta {n_theta}", lambda: m0.locate(off, rect=crop, **kw))
        got0 = m0.locate(off, rect=crop, full=True, **kw)
        exhaustive.update(m0.locate_stats())
        assert got[1] == got0[1] and np.array_equal(got[0], got0[0]), "the pruned and the exhaustive search disagree"
        pruned["over_exhaustive"] = pruned["median_us"] / exhaustive["median_us"]
        print(json.dumps(pruned), flush=True)
        print(json.dumps(exhaustive), flush=True)
        if n_theta == 72:
            with np.errstate(invalid="ignore"):
                hit = dilate(log > 0, TOL)
            t0 = time.perf_counter()
            want = lx.expect(log, off, rect=crop, hit=hit, **kw)
            dt = (time.perf_counter() - t0) * 1e6
            note(figure=f"256^2 crop numpy brute force (tests/_locate_expect.py; hit cells given), n_theta {n_theta}", once_us=dt, N=want[2])
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), "the device records and the expectation disagree"
    m.close(); m0.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "locate_probe.json")
    main()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
