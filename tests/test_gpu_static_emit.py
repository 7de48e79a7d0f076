"""The static-emit form of the lean constraint / Jacobian kernel against the two kernels it stands in for (run with -m gpu).

`launch_variant` (csrc/ctd_kernels.hpp) sends a launch to `cons_jac_static_kernel` when the handle's emit geometry is the static one
of its instantiation (csrc/ctd_emit_static.hpp): manual pattern, CSC order, the whole grid, 256 or 320 lanes.  `CTD_STATIC_EMIT=0`
at `ctd_create` forces the lean kernel, `CTD_LEAN=0` the general one.  All three must give the same bits in c and in the Jacobian
values -- also where the static form must NOT be taken (optimized pattern, CSR order, a shard, a period longer than the workgroup),
so that a wrong dispatch shows.

Grids: T is the tile the sizing rule settles on for a long grid, pinned with CTD_TILE; par = lanes / CSC period replicas walk the
steps of a tile.  N runs over 1, 2, par - 1, par, par + 1, T - 1, T, T + 1, 2 T + 1 and T + 1 + q for every residue q modulo par,
with the default workgroup size and with CTD_BLOCK=256; both store flavours (CTD_WT_STORE) on the sizes with a ragged last pass.
"""
import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe

pytestmark = pytest.mark.gpu

KNOBS = ("CTD_STATIC_EMIT", "CTD_LEAN", "CTD_BLOCK", "CTD_WT_STORE", "CTD_TILE")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def user_grid(N):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(N))])
    return tg / tg[-1]


def three_ways(torch, monkeypatch, prob, N, sch, env, **kw):
    """c and the values by the default selection, with CTD_STATIC_EMIT=0 and with CTD_LEAN=0; returns the launch info too"""
    out, li = [], None
    for knob in ({}, {"CTD_STATIC_EMIT": "0"}, {"CTD_LEAN": "0"}):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(env, **knob).items():
            monkeypatch.setenv(k, v)
        d = ct.DOCP(prob, N, sch, device=0, **kw)
        if li is None:
            li = d.launch_info()
            x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
        c = torch.full((d.dim_NLP_constraints,), 666.666, dtype=torch.float64, device="cuda")
        v = torch.full((d.nnzj,), 666.666, dtype=torch.float64, device="cuda")
        d.cons_jac(x, c, v)
        torch.cuda.synchronize()
        out.append((c, v))
        d.close()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return out, li


def check(torch, monkeypatch, prob, N, sch, env, **kw):
    (s, l, g), li = three_ways(torch, monkeypatch, prob, N, sch, env, **kw)
    steps = kw.get("steps")
    if steps is None:
        assert not (g[0] == 666.666).any() and not (g[1] == 666.666).any(), (prob, sch, N, env)
    assert torch.equal(s[0], l[0]) and torch.equal(s[1], l[1]), (prob, sch, N, env, "static vs lean")
    assert torch.equal(s[0], g[0]) and torch.equal(s[1], g[1]), (prob, sch, N, env, "static vs general")
    return li


def geometry(prob, sch, block, **kw):
    """(T, par) of a long grid's handle with `block` lanes (0: the default rule's size on a one-round grid)"""
    d = ct.DOCP(prob, 100000, sch, device=-1, **kw)
    li = d.launch_info()
    d.close()
    lanes = block or 256
    return li["steps_per_tile"], max(1, lanes // max(1, li["csc_period"])), li["csc_period"]


CASES = [(p, s) for p in ("goddard", "double_integrator_path", "quadrotor") for s in ("midpoint", "gauss_legendre_2", "gauss_legendre_3")]


@pytest.mark.parametrize("prob,sch", CASES, ids=[f"{p}-{s}" for p, s in CASES])
def test_static_equals_lean_equals_general(torch_cuda, monkeypatch, prob, sch):
    for block in (0, 256):
        T, par, period = geometry(prob, sch, block)
        if block == 0 and period > 0 and 320 // period > 256 // period:      # (the default rule may take a fifth wave: its par)
            par = 320 // period
        T = min(T, 48)          # (the long-grid tiles of the light steps are hundreds of steps: the same passes, shorter)
        env = {"CTD_TILE": str(T)}
        if block:
            env["CTD_BLOCK"] = str(block)
        sizes = {1, 2, par - 1, par, par + 1, T - 1, T, T + 1, 2 * T + 1} | {T + 1 + q for q in range(par)}
        for N in sorted(n for n in sizes if n >= 1):
            li = check(torch_cuda, monkeypatch, prob, N, sch, env)
            assert li["steps_per_tile"] <= T and (block == 0 or li["block"] == block)
        for wt in ("0", "1"):
            for N in (par + 1, T + 1, 2 * T + 1):
                check(torch_cuda, monkeypatch, prob, N, sch, dict(env, CTD_WT_STORE=wt))


def test_user_grid_and_the_flagship_geometry(torch_cuda, monkeypatch):
    for N in (37, 10000):         # (10 000 steps of Goddard / Gauss-Legendre 2: the benchmark's grid -- 21-step tiles, 320 lanes)
        li = check(torch_cuda, monkeypatch, "goddard", N, "gauss_legendre_2", {})
        check(torch_cuda, monkeypatch, "goddard", N, "gauss_legendre_2", {}, time_grid=user_grid(N))
    assert li["block"] == 320 and li["steps_per_tile"] == 21
    check(torch_cuda, monkeypatch, "double_integrator_path", 500, "midpoint", {}, time_grid=user_grid(500))


NOT_STATIC = [("optimized", "goddard", "gauss_legendre_2", {"pattern": "optimized"}),
              ("csr", "goddard", "gauss_legendre_2", {"value_order": "csr"}),
              ("csr-no-v", "double_integrator_path", "midpoint", {"value_order": "csr"}),
              ("shard", "goddard", "gauss_legendre_2", {"steps": (40, 91)}),
              ("long-period", "quadrotor12", "gauss_legendre_3", {}),
              ("constant-control", "goddard", "gauss_legendre_2_constant_control", {}),
              ("trapeze", "goddard", "trapeze", {})]


@pytest.mark.parametrize("case", NOT_STATIC, ids=[c[0] for c in NOT_STATIC])
def test_cases_the_static_form_must_not_take(torch_cuda, monkeypatch, case):
    _, prob, sch, kw = case
    for N in ((130, 300) if "steps" in kw else (7, 130)):
        for block in ("256", "320"):
            check(torch_cuda, monkeypatch, prob, N, sch, {"CTD_BLOCK": block}, **kw)
