"""GPU: what a plain `bench.py` run reports and what only `--full` adds.  A plain run sets up, warms up, times the steps and
prints the line (the roofline entries come from the timed steps' own launches); the passes that take runs of their own
(candidates_100, exact_f32, clip_by_clip, roofline_tracker, stages_ms, cpu_baseline, configs) run only under --full."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("candidates_100", "exact_f32", "clip_by_clip", "roofline_tracker", "stages_ms", "cpu_baseline", "configs")


def _bench_line(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "6", *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    assert r.returncode == 0, tail
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, tail
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_nothing_that_takes_a_run_of_its_own(tmp_path):
    d = _bench_line("--dump-outputs", str(tmp_path / "out"))
    assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert d["metric"].startswith("frames/sec DVIS++ R50 offline, 720p T=6") and d["unit"] == "frames/s"
    assert d["roofline"]["launches_timed"] > 0 and d["latency_ms"]["n"] == 2
    assert not [k for k in FULL_ONLY if k in d]
    assert d["dump_outputs"]["step"] == 1 and os.listdir(tmp_path / "out")


def test_full_run_adds_the_extra_passes():
    d = _bench_line("--full", "--no-cpu-baseline")
    assert all(k in d for k in HEADLINE) and d["value"] > 0
    for k in ("candidates_100", "exact_f32", "clip_by_clip", "roofline_tracker", "stages_ms"):
        assert k in d, k
    assert d["candidates_100"]["value"] > 0 and d["exact_f32"]["value"] > 0 and d["clip_by_clip"]["value"] > 0
    assert "cpu_baseline" not in d and "configs" not in d      # --no-cpu-baseline; configs need T = 30
