"""bench.py's plain run prints the headline and nothing that needs runs of its own; --full adds the other blocks after the same timed
steps, so both runs return the same results for the same arguments."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FULL_ONLY = ("roofline", "filter", "candidates_per_query", "fallback_steps", "exact_fp32", "one_query", "f16_stored", "f16_queries",
             "recall_at_100", "cpu_baseline", "configs", "raglite_shaped", "rank_split")


def _bench(tmp_path: Path, name: str, *extra: str) -> dict:
    out = tmp_path / name
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", "125000",
           "--dump-outputs", str(out), *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench(tmp_path, "plain")
    assert plain["full"] is False and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["unit"] == "queries/s" and plain["higher_is_better"] is True and plain["value"] > 0
    assert plain["ms_per_step"] == pytest.approx(1e3 * plain["config"]["queries_per_step"] / plain["value"], rel=1e-9)
    assert plain["metric"].startswith("queries/sec, MaxSim") and isinstance(plain["dtype"], str)
    assert not [key for key in FULL_ONLY if key in plain]
    assert plain["fraction_check"].startswith("ok")

    # (no CPU baseline or vendor GEMM: the other --full blocks are what this checks; configs only run at the metric's own 1 M rows)
    full = _bench(tmp_path, "full", "--full", "--no-cpu-baseline", "--no-vendor-gemm")
    assert full["full"] is True
    for key in ("roofline", "filter", "fallback_steps", "exact_fp32", "one_query", "f16_stored", "f16_queries"):
        assert key in full, key
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "index_memory"):
        assert full[key] == plain[key], key
    assert full["config"]["workload"] == plain["config"]["workload"]
    for name in ("scores.npy", "chunk_ids.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)), name
