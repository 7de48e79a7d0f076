"""bench.py's two modes: a plain run measures only the headline (set-up, warm-up, the timed steps, the line); --full adds
the secondary figures, the per-dispatch kernel time, the CPU baseline and the kernel-only figures of the other workloads."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "other_configs_kernel_only", "optimized_pattern_kernel_only", "csr_order_kernel_only",
             "large_grid_kernel_only", "hessian_kernel_only", "same_workload_other_callbacks", "csr_order_same_workload")


def _bench(*args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", *args],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_help_lists_full():
    """(no GPU: argparse answers --help before torch is imported)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "--full" in p.stdout + p.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_only():
    line = _bench()
    assert all(k in line for k in HEADLINE), sorted(line)
    assert line["unit"] == "evals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["full"] is False
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 1.0) < 1e-9
    assert not [k for k in FULL_ONLY if k in line]
    assert line["roofline"]["kernel_ms"] > 0 and "kernel_ms_per_dispatch_events" not in line["roofline"]


@pytest.mark.gpu
def test_full_run_keeps_the_secondary_figures():
    line = _bench("--full", "--no-extras")
    assert all(k in line for k in HEADLINE) and line["full"] is True
    assert line["roofline"]["kernel_ms_per_dispatch_events"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "evals/s"
