"""Times rooms and doors (gms_map_rooms_dev) on the C3 map -- 2048 x 2048 cells, the bench's -- at inflate = 5, core = 15, against
the two calls of the same handle it is built from: gms_map_reach_dev seeded at one cell with the same inflate and max_cost (the
yardstick of k_rooms_round is k_reach_round: twice the bytes per cell, many seeds instead of one) and gms_map_frontiers_dev, and against
download_log alone, the first step of the route a caller had before.  Prints one JSON line per figure and writes them all to the file
given as the first argument (default profiles/rooms_probe.json).  Needs a GPU; there is no fallback.

Every figure is the host clock around one call that ends in a stream synchronise: the median and the spread (min, max) of 7 warm calls
after two untimed ones.  Rounds and tile runs come from gms_map_rooms_stats / gms_map_reach_stats.  The call's parts -- planes, cores,
rounds, fields and records, doors -- come from a second series of calls with GMS_ROOMS_STAGES set, in which the library waits on the
stream after each part and keeps the host clock (gms_map_rooms_stage_us): their sum exceeds the untimed call by those waits.  The
rounds' part per tile run stands against the WHOLE reach call per tile run, an upper bound for k_reach_round's, whose unit carries no
stage clock.  NOT measured here: the LDS bank-conflict counters of k_rooms_round."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gridmap_slam_robot_amd import GridMap, _lib, synth  # noqa: E402

RESULTS = []


def timed(name, fn, sync, reps=7, **extra):
    for _ in range(2):
        fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e6)
    r = dict(figure=name, median_us=statistics.median(ts), min_us=min(ts), max_us=max(ts), reps=reps, **extra)
    RESULTS.append(r)
    print(json.dumps(r), flush=True)
    return r


def shared_map(inflate=5, core=15, max_cost=0xFFFE):
    cfg = synth.CONFIGS["C3"]
    ext, res, B = cfg["extent"], cfg["resolution"], cfg["beams"]
    m = GridMap(ext, ext, res, (-ext / 2, -ext / 2), max_beams=B)
    assert (m.W, m.H) == (2048, 2048)
    tr = synth.make_trace(ext, res, B, T=8, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    cells = m.W * m.H
    lab = torch.empty(cells, dtype=torch.int32, device="cuda")
    dep = torch.empty(cells, dtype=torch.int16, device="cuda")
    rooms = torch.empty(7 * 1024, dtype=torch.int64, device="cuda")
    doors = torch.empty(6 * 4096, dtype=torch.int64, device="cuda")
    cost = torch.empty(cells, dtype=torch.int16, device="cuda")
    flab = torch.empty(cells, dtype=torch.int32, device="cuda")
    frec = torch.empty(7 * 4096, dtype=torch.int64, device="cuda")
    seed = torch.tensor([[m.W // 2, m.H // 2]], dtype=torch.int32, device="cuda")
    sync = m.synchronize
    for not_free in (True, False):
        mode = "not free" if not_free else "occupied"
        kw = dict(core=core, inflate=inflate, not_free=not_free, max_cost=max_cost)
        counts = {}

        def call():
            counts["n"] = m.rooms_dev(lab, dep, rooms, doors, **kw)

        a = timed(f"2048^2 rooms_dev, all outputs, core = {core}, inflate = {inflate}, {mode}", call, sync)
        a.update(n_rooms=counts["n"][0], n_doors=counts["n"][1], **m.rooms_stats())
        b = timed(f"2048^2 rooms_dev, records alone (no fields), {mode}", lambda: m.rooms_dev(None, None, rooms, doors, **kw), sync)
        r = timed(f"2048^2 reach_dev, one seed at the centre, inflate = {inflate}, {mode}", lambda: m.reach_dev(cost, seed, max_cost, inflate, not_free), sync)
        r.update(**m.reach_stats())
        f = timed(f"2048^2 frontiers_dev, records and labels, inflate = {inflate}", lambda: m.frontiers_dev(frec, flab, inflate=inflate), sync)
        os.environ["GMS_ROOMS_STAGES"] = "1"
        parts = []
        for k in range(9):                                                      # (two untimed, seven kept)
            call()
            parts.append(m.rooms_stats()["stage_us"])
        del os.environ["GMS_ROOMS_STAGES"]
        med = [statistics.median(p[i] for p in parts[2:]) for i in range(5)]
        st = dict(figure=f"2048^2 rooms_dev, the parts with a stream wait after each, {mode}", planes_us=med[0], cores_us=med[1], rounds_us=med[2],
                  fields_and_records_us=med[3], doors_us=med[4], sum_us=sum(med), rounds_us_per_tile_run=med[2] / max(a["tile_runs"], 1),
                  reach_whole_call_us_per_tile_run=r["median_us"] / max(r["tile_runs"], 1))
        RESULTS.append(st)
        print(json.dumps(st), flush=True)
        a["ratio_to_reach"], a["ratio_to_frontiers"] = a["median_us"] / r["median_us"], a["median_us"] / f["median_us"]
        b["ratio_to_reach"], b["ratio_to_frontiers"] = b["median_us"] / r["median_us"], b["median_us"] / f["median_us"]
        print(json.dumps(dict(figure=f"ratios, {mode}", to_reach=a["ratio_to_reach"], to_frontiers=a["ratio_to_frontiers"])), flush=True)
    down = timed("2048^2 download_log alone (32 MiB): the route before, ahead of any segmentation on the host", lambda: m.download_log(), lambda: None)
    RESULTS.append(dict(figure="rooms_dev (not free) against download_log alone", ratio=RESULTS[0]["median_us"] / down["median_us"]))
    # the last timed call against the host form, the whole map (the restatement on 2048^2 is not run here)
    host = m.rooms(core=core, inflate=inflate, not_free=False, max_cost=max_cost, depth=True, cap_rooms=1024, cap_doors=4096)
    sync()
    assert np.array_equal(lab.cpu().numpy().view(np.uint32).reshape(m.H, m.W), host["labels"]), "the device form and the host form disagree"
    stored = min(host["n_rooms"], 1024)
    assert np.array_equal(rooms.cpu().numpy()[:7 * stored].view(_lib.ROOM_DTYPE), host["rooms"][:stored])
    m.close()


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rooms_probe.json")
    shared_map()
    with open(path, "w") as f:
        json.dump(RESULTS, f, indent=1)
