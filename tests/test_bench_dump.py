"""bench.py --dump-outputs: what the last timed step computed, written as DIR/<name>.npy (float64, at most 64 MB, a fixed seeded
sample of the larger arrays beyond that) so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

from helpers import TOL, bench_inputs, describe, relerr  # noqa: E402


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_under_the_limit_writes_whole_arrays(tmp_path):
    c, v = np.linspace(-1.0, 1.0, 1001), np.arange(5000, dtype=np.float32)
    w = bench.dump_outputs(str(tmp_path), {"constraints": c, "jacobian_values": v})
    assert w == {"constraints": {"entries": 1001, "of": 1001}, "jacobian_values": {"entries": 5000, "of": 5000}}
    assert sorted(os.listdir(tmp_path)) == ["constraints.npy", "jacobian_values.npy"]
    c2, v2 = np.load(tmp_path / "constraints.npy"), np.load(tmp_path / "jacobian_values.npy")
    assert c2.dtype == np.float64 and v2.dtype == np.float64
    assert np.array_equal(c2, c) and np.array_equal(v2, v.astype(np.float64))


def test_dump_over_the_limit_is_a_fixed_sample_within_the_limit(tmp_path):
    rng = np.random.default_rng(7)
    small, big = rng.standard_normal(300), rng.standard_normal(400_000)
    limit = 1 << 20
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        w = bench.dump_outputs(str(d), {"jacobian_values": big, "constraints": small}, limit=limit)
        assert _sizes(d) <= limit
        assert w["constraints"] == {"entries": 300, "of": 300}           # the small array stays whole
        assert 0 < w["jacobian_values"]["entries"] < 400_000
        runs.append((np.load(d / "constraints.npy"), np.load(d / "jacobian_values.npy")))
    assert np.array_equal(runs[0][0], small)
    assert np.array_equal(runs[0][1], runs[1][1])                        # the same positions every time
    assert np.isin(runs[0][1], big).all()
    pos = np.searchsorted(np.sort(big), runs[0][1])
    assert len(np.unique(pos)) == len(pos)                               # no entry twice


@pytest.mark.gpu
def test_bench_dump_is_the_timed_steps_output(tmp_path):
    """the dumped c and Jacobian values of the bench workload (Goddard, Gauss-Legendre 2, 10 000 steps) against the CPU oracle"""
    from oracle.oracle import OracleDOCP
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 5 and line["ms_per_step"] > 0
    assert set(line["dumped_outputs"]["arrays"]) == {"constraints", "jacobian_values"}
    assert _sizes(d) <= 64 << 20
    ora = OracleDOCP("goddard", "gauss_legendre_2", 10000)
    x = bench_inputs(describe(ora, "goddard", "gauss_legendre_2"), perturb=1e-3)
    c, v = np.load(d / "constraints.npy"), np.load(d / "jacobian_values.npy")
    assert c.shape == (ora.dim_NLP_constraints,)
    assert relerr(c, ora.constraints(x)) <= TOL and relerr(v, ora.jac_coord(x)) <= TOL
