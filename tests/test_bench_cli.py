"""bench.py's command line: a plain run ends after its timed steps; what takes runs of its own (the CPU baseline, the
eager roofline steps of --graph) is behind --full, which is off by default."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--T", "4", "--size", "32"]


def _bench(*args):
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_full_is_an_option():
    out = _bench("--help")
    assert "--full" in out and "--no-cpu-baseline" in out


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_plain_run_is_lean(graph):
    lines = _bench(*TINY, *(["--graph"] if graph else [])).splitlines()
    assert len(lines) == 1, lines                                   # stdout carries the JSON line and nothing else
    out = json.loads(lines[0])
    assert out["unit"] == "patches/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) <= 1e-9 * out["value"]     # B / step time
    assert "cpu_baseline" not in out                                # a run of its own: --full
    if graph:
        assert out["roofline"] is None                              # a graph carries no events; the eager steps are --full's
    else:
        assert out["roofline"]["launches_timed"] > 0                # timed inside the steps: no run of its own
