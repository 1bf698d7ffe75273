"""What a map view costs (gms_map_view / gms_slam_view, include/gridmapslam.h "map views") against the route a caller had before it.

  shared map, 2048 x 2048 cells (BASELINE C3's grid): the full view at d = 1 and d = 4 and a 512 x 512 window, log view, grey bytes;
  per-particle filter, 500 x 120^2 and 4096 x 256^2: the same three views of the STRONGEST particle's map (picked on the device),
      log view and likelihood view (the field computed from the shown particle's class plane);
  each in the _dev form (device output, no synchronise) and the host form (host output, synchronises);
  the previous route: gms_map_download_log / (statistics read-back +) gms_slam_download_map, then the grey chain in numpy.

_dev form: hipEvents around every single call (`bracketed`: includes what the two event markers cost on the stream, a few
microseconds) and around runs of CALLS_PER_RUN calls back to back (`back_to_back`: per call; the launch rate of the host binds it when
the kernel is shorter than a launch); bytes/s = the cells' 8 bytes + the output's bytes over the back-to-back time.  Host form:
hipEvents around every call and the host clock around it (it ends in a synchronise).  Medians of CALLS calls after WARMUP.
Prints one JSON document and writes it to the path given as the first argument."""
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

from gridmap_slam_robot_amd import GridMap, SLAMParticleMaps, synth  # noqa: E402
from gridmap_slam_robot_amd._lib import check, load  # noqa: E402

CALLS, WARMUP, CALLS_PER_RUN, OLD_ROUTE_CALLS = 240, 20, 40, 12


def _events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def _bracketed(call, n=CALLS):
    """median microseconds between events recorded right before and right after one call"""
    for _ in range(WARMUP):
        call()
    a, b = _events(n), _events(n)
    for i in range(n):
        a[i].record(); call(); b[i].record()
    torch.cuda.synchronize()
    return statistics.median(x.elapsed_time(y) * 1e3 for x, y in zip(a, b))


def _back_to_back(call, runs=CALLS // CALLS_PER_RUN):
    a, b = _events(runs), _events(runs)
    for i in range(runs):
        a[i].record()
        for _ in range(CALLS_PER_RUN):
            call()
        b[i].record()
    torch.cuda.synchronize()
    return statistics.median(x.elapsed_time(y) * 1e3 / CALLS_PER_RUN for x, y in zip(a, b))


def _host_clock(call, n):
    for _ in range(3):
        call()
    t = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def _grey_numpy(log):
    """the grey chain on the host, as a caller of the download route writes it"""
    value = 1.0 - (1.0 - 1.0 / (1.0 + np.exp(log)))
    t = value.astype(np.float32) * np.float32(255)
    idx = np.clip(np.nan_to_num(t, nan=0.0), 0, 255).astype(np.int32)
    return ((idx * 255) >> 8).astype(np.uint8)


def _views(side):
    win = min(512, side)
    return [("full_d1", None, 1), ("full_d4", None, 4), (f"window_{win}", ((side - win) // 2, (side - win) // 2, win, win), 1)]


def _row(name, side, rect, d, view_dev, view_host, likelihood):
    w, h = (side, side) if rect is None else rect[2:]
    ow, oh = -(-w // d), -(-h // d)
    out = torch.empty(ow * oh, dtype=torch.uint8, device="cuda")
    dev = lambda: view_dev(rect, d, likelihood, out)                       # noqa: E731
    host = lambda: view_host(rect, d, likelihood)                          # noqa: E731
    br, bb = _bracketed(dev), _back_to_back(dev)
    moved = w * h * 8 + ow * oh
    return {"view": name, "source": "likelihood" if likelihood else "log", "cells": w * h, "pixels": ow * oh,
            "dev_bracketed_us": round(br, 2), "dev_back_to_back_us": round(bb, 2), "bytes_moved": moved,
            "dev_bytes_per_s_back_to_back": round(moved / (bb * 1e-6), 0),
            "host_events_us": round(_bracketed(host), 2), "host_clock_us": round(_host_clock(host, CALLS), 2)}


def shared_map(stream):
    m = GridMap(40.96, 40.96, 0.02, (-20.48, -20.48), max_beams=2048)
    assert (m.W, m.H) == (2048, 2048)
    check(load().gms_map_set_stream(m._h, stream))
    tr = synth.make_trace(40.96, 0.02, 720, T=8, seed=7)
    for t in range(4):
        m.update(tr.scans[t], tr.poses[t])
    rows = [_row(n, 2048, r, d, lambda r, d, l, o: m.view(r, d, l, out=o), lambda r, d, l: m.view(r, d, l), False) for n, r, d in _views(2048)]
    old = _host_clock(lambda: _grey_numpy(m.download_log()), OLD_ROUTE_CALLS)
    dl = _host_clock(lambda: m.download_log(), OLD_ROUTE_CALLS)
    m.close()
    return {"config": "shared map 2048^2", "views": rows, "download_log_then_numpy_us": round(old, 1), "download_log_alone_us": round(dl, 1)}


def particle_maps(name, n, ext, B, stream):
    s = SLAMParticleMaps(ext, ext, 0.05, (-ext / 2, -ext / 2), num_particles=n, max_beams=B)
    check(load().gms_map_set_stream(s.grid_map._h, stream))
    tr = synth.make_trace(ext, 0.05, B, T=8, seed=7)
    s.set_poses(synth.make_particles(tr.poses[0], n, seed=3, sigma_xy=0.03, sigma_theta_deg=2.0))
    s.update(tr.scans[0], None)
    s.update(tr.scans[1], (0.02, 0.05), seed=5, sequence=1)
    side = s.W
    rows = []
    for likelihood in (False, True):
        rows += [_row(nm, side, r, d, lambda r, d, l, o: s.view("strongest", r, d, l, out=o), lambda r, d, l: s.view("strongest", r, d, l), likelihood)
                 for nm, r, d in _views(side)]

    def old_route():
        return _grey_numpy(s.map_of(s.pf.stats()["strongest"]))            # the read-back in front of the download

    old = _host_clock(old_route, OLD_ROUTE_CALLS)
    s.close()
    return {"config": name, "particles": n, "side": side, "views": rows, "stats_download_map_then_numpy_us": round(old, 1)}


def main():
    torch.cuda.init()
    side_stream = torch.cuda.Stream()                  # a real stream: the default stream's handle is NULL, which a gms_map takes for "my own"
    torch.cuda.set_stream(side_stream)                 # the events below are recorded on it, the handles run on it
    stream = side_stream.cuda_stream
    doc = {"tool": "tools/view_probe.py", "device": torch.cuda.get_device_name(0), "calls": CALLS, "calls_per_run": CALLS_PER_RUN,
           "statistic": "medians; microseconds; see the tool's docstring for what each column brackets", "rows": []}
    for make in (lambda: shared_map(stream), lambda: particle_maps("500 x 120^2", 500, 6.0, 90, stream),
                 lambda: particle_maps("4096 x 256^2", 4096, 12.8, 180, stream)):
        r = make()
        doc["rows"].append(r)
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
