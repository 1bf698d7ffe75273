#!/usr/bin/env python3
"""Host count for the scoring kernel: how many 128-byte lines of the factor table one look-up instruction touches, by lane order.

  python tools/score_segment_order_count.py [--sets 8] [--threads 1024] [--json out.json]

numpy only, no GPU.  The bench's C3 cloud and scans (synth.make_trace(..., seed=1234), make_particles(poses[T/2 + s], 16384, seed=99 + s)),
k_score_c's geometry (16 segments of 45 beams, workgroups of `threads` particles in caller order, a look-up instruction = 64 consecutive
lanes x one hit beam) and its cell arithmetic (float-rounded trig, double transform, truncation; the table's rows are W + 16 entries of
8 bytes, so a line is a row and a group of 16 columns).  For every look-up instruction it counts the distinct lines per aligned quad of
lanes, per instruction, and the runs of equal lines along the lanes, with the workgroup's lanes
  (a) in the caller's order,
  (b) ordered by the row / 16-cell group of the end point of the segment's middle hit beam (several folds of that key), and
  (c) ordered by heading (DESIGN section 9's rejected prologue sort),
and predicts the look-up phase from the lines per quad: the committed micro-benchmark gives 47.8 clocks per instruction at four lines
per quad and 25.1 at one (32.6 at two: the line through the end points says 32.7), calibrated on (a) against the measured 15 us."""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gridmap_slam_robot_amd import synth                                       # noqa: E402

CLK_INDEPENDENT, CLK_QUAD = 47.8, 25.1         # profiles/r06/microbench.json: gather_coalesce modes 0 and 2 (quads), clocks per wave instruction
MEASURED_LOOKUP_US = 15.0                      # per-workgroup look-up phase at C3 (median 15.2, 14.4-16.7)
SEG = 45
KEPT = "row6.grp2 (256)"                       # the key k_score_c<1, true> uses: the per-beam and buckets-in-use tables are its


def cells(P, lx, ly, cfg):
    """End-point cells [n][len(lx)] as k_score_c forms them (beam_cell_fast without its guard: the guard changes 4e-6 of them by one)."""
    W = int(round(cfg["extent"] / cfg["resolution"]))
    pos = -cfg["extent"] / 2
    th = P[:, 2].astype(np.float64)
    c = np.cos(th).astype(np.float32).astype(np.float64)[:, None]
    s = np.sin(th).astype(np.float32).astype(np.float64)[:, None]
    px, py = P[:, 0].astype(np.float64)[:, None], P[:, 1].astype(np.float64)[:, None]
    rinv = 1.0 / cfg["resolution"]
    gx = np.trunc((lx[None, :] * c - ly[None, :] * s + px - pos) * rinv).astype(np.int64)
    gy = np.trunc((lx[None, :] * s + ly[None, :] * c + py - pos) * rinv).astype(np.int64)
    gx = np.where(gx < 0, W, np.minimum(gx, W))       # fac_index: clamped onto the neutral border (column W, row H)
    gy = np.where(gy < 0, W, np.minimum(gy, W))
    return gx, gy, W


def distinct(a, axis):
    a = np.sort(a, axis=axis)
    return 1 + (np.diff(a, axis=axis) != 0).sum(axis=axis)


def count(line):
    """line: [groups][threads][beams] -> (lines per quad, lines per instruction, runs per instruction), sums over the instructions"""
    g, t, nb = line.shape
    quad = distinct(line.reshape(g, t // 4, 4, nb), 2).sum()
    inst = distinct(line.reshape(g, t // 64, 64, nb), 2).sum()
    w = line.reshape(g, t // 64, 64, nb)
    runs = (1 + (np.diff(w, axis=2) != 0).sum(axis=2)).sum()
    return int(quad), int(inst), int(runs), g * (t // 64) * nb


KEYS = {                                                                        # name -> (key of (cx, cy), bucket count)
    "row7.grp3 (1024)": (lambda cx, cy: ((cy & 127) << 3) | ((cx >> 4) & 7), 1024),
    "row6.grp4 (1024)": (lambda cx, cy: ((cy & 63) << 4) | ((cx >> 4) & 15), 1024),
    "row8.grp2 (1024)": (lambda cx, cy: ((cy & 255) << 2) | ((cx >> 4) & 3), 1024),
    "row7.grp2 (512)": (lambda cx, cy: ((cy & 127) << 2) | ((cx >> 4) & 3), 512),
    "row6.grp2 (256)": (lambda cx, cy: ((cy & 63) << 2) | ((cx >> 4) & 3), 256),
    "row8.grp3 (2048)": (lambda cx, cy: ((cy & 255) << 3) | ((cx >> 4) & 7), 2048),
    "row, grp unfolded": (lambda cx, cy: (cy << 8) | (cx >> 4), 0),
    "row2 (half rows).grp": (lambda cx, cy: (((cy >> 1) & 127) << 3) | ((cx >> 4) & 7), 1024),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8, help="pose sets / scans of the bench counted (it cycles through 8)")
    ap.add_argument("--threads", type=int, default=1024, help="lanes per workgroup (1024 at C3; 512 / 256 for shards and small populations)")
    ap.add_argument("--particles", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cfg = synth.CONFIGS["C3"]
    n, B, T = a.particles or cfg["particles"], cfg["beams"], 64
    tr = synth.make_trace(cfg["extent"], cfg["resolution"], B, T=T, seed=1234)
    orders = ["caller", "heading"] + list(KEYS)
    tot = {o: np.zeros(4, dtype=np.int64) for o in orders}
    per_beam = {o: np.zeros((SEG, 2), dtype=np.int64) for o in ("caller", KEPT)}    # by distance from the middle hit beam
    occupancy = []
    for s in range(a.sets):
        P = synth.make_particles(tr.poses[T // 2 + s], n, seed=99 + s)
        scan = tr.scans[T // 2 + s]
        groups = n // a.threads
        for seg in range(B // SEG):
            bm = scan[seg * SEG:(seg + 1) * SEG]
            bm = bm[bm["hit"] != 0]
            nb = len(bm)
            if nb == 0:
                continue
            gx, gy, W = cells(P, bm["local_x"].astype(np.float64), bm["local_y"].astype(np.float64), cfg)
            line = (gy * ((W + 16) // 16) + (gx >> 4)).reshape(groups, a.threads, nb)
            mid = nb // 2
            cx, cy = gx[:, mid].reshape(groups, a.threads), gy[:, mid].reshape(groups, a.threads)
            outside = (cx >= W) | (cy >= W)
            for o in orders:
                if o == "caller":
                    L = line
                else:
                    if o == "heading":
                        key = P[:, 2].reshape(groups, a.threads)
                    else:
                        f, nbk = KEYS[o]
                        key = f(cx, cy)
                        if nbk:
                            key = np.where(outside, nbk - 1, key)
                            if o == KEPT:
                                occupancy += [np.unique(k).size for k in key]
                    perm = np.argsort(key, axis=1, kind="stable")       # (inside a bucket: caller order; the device's is the atomics' arrival order)
                    L = np.take_along_axis(line, perm[:, :, None], axis=1)
                tot[o] += count(L)
                if o in per_beam:
                    for j in range(nb):
                        q, i, r, k = count(L[:, :, j:j + 1])
                        per_beam[o][abs(j - mid)] += (q, k)
    res = {"config": "C3", "particles": n, "threads": a.threads, "sets": a.sets, "orders": {}}
    base_q = tot["caller"][0] / (tot["caller"][3] * 16)
    clk = lambda q: CLK_QUAD + (CLK_INDEPENDENT - CLK_QUAD) * (q - 1.0) / 3.0
    print(f"C3 cloud, {n} particles, workgroups of {a.threads}, {a.sets} scans: {tot['caller'][3]} look-up instructions")
    print(f"{'lane order':24s} {'lines/quad':>10s} {'lines/instr':>11s} {'runs/instr':>10s} {'clk/instr':>9s} {'look-up phase, us':>18s}")
    for o in orders:
        q, i, r, k = tot[o]
        lq, li, lr = q / (k * 16), i / k, r / k
        us = MEASURED_LOOKUP_US * clk(lq) / clk(base_q)
        print(f"{o:24s} {lq:10.3f} {li:11.2f} {lr:10.2f} {clk(lq):9.1f} {us:18.2f}")
        res["orders"][o] = {"lines_per_quad": lq, "lines_per_instruction": li, "runs_per_instruction": lr, "clocks_per_instruction_model": clk(lq),
                            "lookup_phase_us_model": us}
    print("lines per quad by distance (in hit beams) from the segment's middle hit beam: caller / " + KEPT)
    rows = []
    for d in range(SEG):
        if per_beam["caller"][d, 1]:
            qa = per_beam["caller"][d, 0] / (per_beam["caller"][d, 1] * 16)
            qb = per_beam[KEPT][d, 0] / (per_beam[KEPT][d, 1] * 16)
            rows.append((d, qa, qb))
            print(f"  {d:2d}: {qa:5.2f} {qb:5.2f}")
    res["lines_per_quad_by_beam_distance"] = rows
    if occupancy:
        print(f"{KEPT}: buckets in use per workgroup: median {int(np.median(occupancy))}, min {min(occupancy)}, max {max(occupancy)}")
        res["buckets_in_use"] = {"median": int(np.median(occupancy)), "min": int(min(occupancy)), "max": int(max(occupancy))}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
