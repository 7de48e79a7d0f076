"""The two variants of the constraint / Jacobian kernel (run with -m gpu on an MI355X).

Every registry instantiation is compiled twice (csrc/ctd_kernels.hpp): the GENERAL variant, and the LEAN variant for launches
that read the whole iterate from one buffer and emit everything behind the barrier -- no shard table, no early emission, block
sizes and Butcher tables from the static layout of the instantiation.  `launch_cons_jac` picks the variant per launch;
`CTD_LEAN=0`, read at `ctd_create`, forces the general one.  (The staged tiles of the one-point schemes -- trapeze here -- have
no lean instantiation: their two evaluations run the same kernel and only the oracle comparison says something.)

Here: the two variants give bit-identical constraints and Jacobian values, the lean result matches the CPU oracle with the
comparison and tolerance of tests/test_gpu_parity.py, and one handle switches variants when a shard table is set and removed.

Grids: T is the tile the sizing rule settles on for a long grid (a host-only handle tells it); the handles under test are
pinned to it (CTD_TILE) and run N in {1, 2, T, T + 1, 2T + 1}: an edge block alone, one full tile, a one-step last tile,
two tiles and a ragged one.
"""
import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import TOL, bench_inputs, describe, relerr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def user_grid(N):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(N))])
    return tg / tg[-1]


def default_tile(prob, sch, **kw):
    d = ct.DOCP(prob, 100000, sch, device=-1, **kw)
    T = d.launch_info()["steps_per_tile"]
    d.close()
    return T


def evaluate(torch, monkeypatch, lean, prob, N, sch, x, **kw):
    """c and the Jacobian values of one evaluation with the lean (default selection) or the general (forced) variant"""
    if lean:
        monkeypatch.delenv("CTD_LEAN", raising=False)
    else:
        monkeypatch.setenv("CTD_LEAN", "0")
    d = ct.DOCP(prob, N, sch, device=0, **kw)
    c, v = d.cons_jac(torch.from_numpy(x).cuda())
    c, v = c.cpu().numpy(), v.cpu().numpy()
    rows, cols = d.jac_structure()
    d.close()
    monkeypatch.delenv("CTD_LEAN", raising=False)
    return c, v, rows, cols


# (id, problem, scheme, handle keywords, user grid, oracle pattern mode)
CASES = [("goddard-" + s, "goddard", s, {}, False, 0)
         for s in ("gauss_legendre_1", "gauss_legendre_2", "gauss_legendre_3", "midpoint", "trapeze", "euler", "euler_implicit")]
CASES += [(f"{p}-{s}", p, s, {}, False, 0)
          for p in ("double_integrator_freet0tf", "double_integrator_path") for s in ("gauss_legendre_2", "midpoint")]
CASES += [("goddard-gl2-user-grid", "goddard", "gauss_legendre_2", {}, True, 0),
          ("goddard-gl2-optimized", "goddard", "gauss_legendre_2", {"pattern": "optimized"}, False, 2),
          ("goddard-gl2-csr", "goddard", "gauss_legendre_2", {"value_order": "csr"}, False, 0),
          ("goddard-midpoint-cs2", "goddard", "midpoint", {"control_steps": 2}, False, 0),
          ("quadrotor-gl3", "quadrotor", "gauss_legendre_3", {}, False, 0)]      # staged driver, split evaluation


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_lean_equals_general_and_oracle(oracle_lib, torch_cuda, monkeypatch, case):
    _, prob, sch, kw, grid, mode = case
    T = default_tile(prob, sch, **kw)
    monkeypatch.setenv("CTD_TILE", str(T))
    sizes = (T + 1,) if prob == "quadrotor" else (1, 2, T, T + 1, 2 * T + 1)
    for N in sizes:
        tg = user_grid(N) if grid else None
        o = oracle_lib.OracleDOCP(prob, sch, None if grid else N, time_grid=tg, control_steps=kw.get("control_steps", 1))
        o.set_pattern_mode(mode)
        x = bench_inputs(describe(o, prob, sch), perturb=1e-3)
        hk = dict(kw, time_grid=tg)
        cl, vl, rows, cols = evaluate(torch_cuda, monkeypatch, True, prob, N, sch, x, **hk)
        cg, vg, _, _ = evaluate(torch_cuda, monkeypatch, False, prob, N, sch, x, **hk)
        assert np.array_equal(cl, cg), (N, "c")
        assert np.array_equal(vl, vg), (N, "Jacobian values")
        assert relerr(cl, o.constraints(x)) <= TOL, N
        if kw.get("value_order") == "csr":      # the oracle's values are in CSC order: columns, rows ascending inside a column
            vl = vl[np.lexsort((rows, cols))]
        assert relerr(vl, o.jac_coord(x)) <= TOL, N


def test_one_handle_switches_variants(torch_cuda):
    """A shard table whose every entry is the handle's own buffer (one GPU) sends the launches to the general variant; removing
    it sends them back to the lean one: three bit-identical results.  A whole-grid handle (a table of one shard) and the middle
    shard of three."""
    torch = torch_cuda
    for prob, sch, N in (("goddard", "gauss_legendre_2", 300), ("double_integrator_path", "midpoint", 300)):
        cuts = [0, N // 3, 2 * N // 3 + 1, N]
        for steps, table, me in ((None, [0, N], 0), ((cuts[1], cuts[2]), cuts, 1)):
            d = ct.DOCP(prob, N, sch, device=0, steps=steps)
            x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()

            def run():      # (a shard writes its own rows and entries only: the rest keeps the fill value)
                c = torch.full((d.dim_NLP_constraints,), 666.666, dtype=torch.float64, device="cuda")
                v = torch.full((d.nnzj,), 666.666, dtype=torch.float64, device="cuda")
                return d.cons_jac(x, c, v)

            c0, v0 = run()
            d.set_x_shards(table, [x.data_ptr()] * (len(table) - 1), me)
            c1, v1 = run()
            d.set_x_shards(None, None, 0)
            c2, v2 = run()
            assert torch.equal(c0, c1) and torch.equal(v0, v1), (prob, steps)
            assert torch.equal(c0, c2) and torch.equal(v0, v2), (prob, steps)
            d.close()
