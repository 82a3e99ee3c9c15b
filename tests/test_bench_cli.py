"""bench.py's single-rank options on CPU (gloo + the stub workload): --steps sets the timed steps, a plain run carries no --full
sections, --dump-outputs writes the last timed step's outputs as float .npy files, the same ones from run to run."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*extra):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "stub", "--backend", "gloo"] + list(extra),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only():
    line = _bench("--steps", "7", "--warmup", "2")
    assert line["steps"] == 7 and line["warmup"] == 2
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 4 * 7 / (line["ms_per_step"] * 7e-3)) / line["value"] < 1e-3
    assert "cpu_baseline" not in line and "secondary" not in line


def test_full_adds_the_cpu_baseline_section():
    line = _bench("--steps", "3", "--warmup", "1", "--full")
    assert "cpu_baseline" in line


def test_dump_outputs_writes_the_last_step_the_same_every_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    _bench("--steps", "5", "--warmup", "1", "--dump-outputs", str(a))
    _bench("--steps", "5", "--warmup", "1", "--dump-outputs", str(b))
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) == ["stub.npy"]
    x, y = np.load(a / "stub.npy"), np.load(b / "stub.npy")
    assert x.dtype in (np.float32, np.float64)
    assert (x == y).all()
    assert (x[0] == np.arange(64) + 4).all()            # step 4 is the last of 5
    total = sum(os.path.getsize(a / f) for f in files)
    assert total <= 64e6
