"""A plain `bench.py --gpus 1` run: one timed region of exactly --steps steps, the contract's fields on the line (no roofline, no CPU
baseline: those are --full's), and --dump-outputs writing the same arrays in two processes with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(tmp_path, tag):
    out_dir, rep = str(tmp_path / tag), str(tmp_path / f"{tag}_report.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                          "--dump-outputs", out_dir, "--report", rep], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), out_dir


def test_plain_run_times_its_steps_once_and_dumps_the_same_outputs_every_time(tmp_path):
    d, a = _plain_run(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 3 and d["timed_regions"] == 1 and d["unit"] == "particle-scan evals/s" and d["dtype"] == "f64"
    assert d["roofline"] is None and d["cpu_baseline"] is None and "secondary_ms_per_step" not in d
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(d["config"]["particles_total"] / (d["ms_per_step"] * 1e-3), rel=1e-4)
    _, b = _plain_run(tmp_path, "b")
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "poses.npy" in names and "map_log_odds.npy" in names
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64_000_000
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.array_equal(x, y), n
    assert np.load(os.path.join(a, "poses.npy")).shape == (d["config"]["particles_total"], 3)
