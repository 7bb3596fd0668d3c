"""bench.py's two kinds of run on one MI355X: a plain run times the steps and prints the line with the driver contract and
nothing else; `--full` adds the other arithmetic modes, launches alone, the CPU baselines, the report sections and the side
file of the whole report."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

SHORT = ["--steps", "1", "--warmup", "1", "--batches-per-step", "4"]
EXTRAS = ("cpu_baseline", "cpu_native", "esdf_build", "esdf_kernel", "cfg1", "value_parity_mode", "single_batch_traj_per_s",
          "host_visible_traj_per_s", "accepted_after_retries_traj_per_s", "single_batch_budget")


def _bench(args, timeout=900):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NEO_BENCH_FORCE_DIST"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only():
    out = _bench(SHORT)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in out, k
    assert out["value"] > 1e4 and out["unit"] == "traj/s" and out["dtype"] == "f32x" and out["steps"] == 1
    assert abs(out["value"] - 4 * 4096 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert set(out["modes"]) == {"f32x"} and out["details"] is None
    for k in EXTRAS:
        assert k not in out, k


def test_full_run_adds_the_modes_the_cpu_baselines_and_the_side_file(tmp_path):
    details = tmp_path / "details.json"
    out = _bench(SHORT + ["--full", "--cpu-seconds", "1", "--native-seconds", "1", "--report-sections", "cfg1",
                          "--details", str(details)])
    assert set(out["modes"]) == {"f32x", "f32", "f64"} and out["value_parity_mode"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_native"]["value"] > 0
    assert out["single_batch_traj_per_s"] > 0 and out["host_visible_traj_per_s"] > 0
    assert out["esdf_build"]["ms"] > 0 and "plan_ms_gpu" in out["cfg1"] and "plan_ms_cpu_native" in out["cfg1"]
    assert out["details"] == str(details)
    full = json.load(open(details))
    assert full["value"] == pytest.approx(out["value"], rel=1e-5) and full["modes"]["f64"]["single_batch_ms"] > 0
