"""bench.py as a command, on the tiny architecture: a plain run prints the headline line and nothing that takes runs of its own;
--full adds the roofline table and the CPU baseline to the same line (the north-star and parity legs exist at the full size only)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")
FULL_ONLY = ("roofline", "north_star", "parity", "cpu_baseline")


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--tiny", *extra],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines            # one JSON result line on stdout
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    line, err = _run("--dump-outputs", str(tmp_path / "dump"))
    for k in HEADLINE:
        assert k in line, k
    assert not any(k in line for k in FULL_ONLY), sorted(line)
    assert line["metric"] == "views/sec" and line["unit"] == "views/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 2 and line["warmup"] == 1
    assert abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert "cpu_baseline" not in err and "north-star" not in err and "parity leg" not in err
    names = sorted(p.name for p in (tmp_path / "dump").iterdir())
    assert {"pts3d.npy", "depth.npy", "normals.npy", "camera_params.npy"} <= set(names), names


@pytest.mark.gpu
def test_full_run_adds_roofline_and_cpu_baseline():
    line, err = _run("--full")
    for k in HEADLINE + ("roofline", "cpu_baseline"):
        assert k in line, k
    assert line["roofline"]["kernels"] and line["roofline"]["forward_ms_events"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "views/s"
    line2, _ = _run("--full", "--no-cpu-baseline")        # the options that drop single legs still do
    assert "roofline" in line2 and "cpu_baseline" not in line2
