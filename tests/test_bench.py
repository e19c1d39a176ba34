"""bench.py's two modes: a plain run prints the headline line only; --full adds the per-kernel, roofline, eager-module and slice
figures (the CPU baseline and the train-step harness are switched off here to keep the run short).  Each run is a child process."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "step_roofline", "kernels", "cpu_baseline", "eager_module_ms_per_step", "eager_module_ms_per_step_engine_inline",
             "layer_loop_slice", "train_harness", "eager_module_note")


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "1"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def run_bench(*args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py")] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(built_lib):
    d = run_bench("--steps", "5", "--warmup", "2")
    for k in HEADLINE:
        assert k in d, k
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["batch_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]


@pytest.mark.gpu
def test_full_run_keeps_the_extra_figures(built_lib):
    d = run_bench("--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-harness", "--kernel-reps", "3")
    for k in HEADLINE + FULL_ONLY:
        assert k in d, k
    assert d["full"] is True
    assert d["kernels"] and all(v["us"] > 0 for v in d["kernels"].values())
    assert d["roofline"]["kernel"] in {v["symbol"] for v in d["kernels"].values()}
    assert d["eager_module_ms_per_step"] > 0 and d["layer_loop_slice"]["ms_per_step"] > 0
    assert d["cpu_baseline"] is None and d["train_harness"] is None
