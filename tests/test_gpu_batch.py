"""Batched callbacks on the MI355X (ctd_*_batch_dev_async, DOCP.*_batch): K iterates of one transcription per launch.  The
contract is BIT-IDENTITY: member b of a batched call equals one single call on member b alone (np.array_equal), for the
constraints, the Jacobian values, the objective, the gradient and the Hessian values -- every registry problem x every scheme
on small grids (edge-only, single- and multi-tile launches, a ragged grid) in both patterns and value orders, the full-size
bench workloads (checked against the oracle too), strided buffers, a run-time OCP and the refusals."""
import ctypes as C

import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import TOL, bench_inputs, describe, relerr
from jit_defs import twin

pytestmark = pytest.mark.gpu
SENT = 666.666


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def members(torch, d, prob, sch, K):
    """K perturbed iterates of d as the rows of a (K, nvar) device tensor (and the host copy)"""
    X = np.stack([bench_inputs(describe(d, prob, sch), perturb=1e-3, seed=0x9E3779B97F4A7C15 + 7919 * b) for b in range(K)])
    return torch.from_numpy(X).cuda(), X


def multipliers(torch, d, K):
    r = np.arange(d.dim_NLP_constraints)
    return torch.from_numpy(np.stack([np.cos(0.37 * r + 0.9 * b) for b in range(K)])).cuda()


def check_members(torch, d, Xd, Y=None, w=0.7, first_order=True):
    """batched results == single calls, member by member, bit for bit"""
    K = Xd.shape[0]
    Cb, Vb = d.cons_jac_batch(Xd)
    if first_order:
        fb = d.obj_batch(Xd).cpu().numpy()
        Gb = d.grad_batch(Xd).cpu().numpy()
    if Y is not None:
        Hb = d.hess_coord_batch(Xd, Y, w).cpu().numpy()
    Cb, Vb = Cb.cpu().numpy(), Vb.cpu().numpy()
    for b in range(K):
        c, v = d.cons_jac(Xd[b])
        assert np.array_equal(Cb[b], c.cpu().numpy()), ("c", b)
        assert np.array_equal(Vb[b], v.cpu().numpy()), ("vals", b)
        if first_order:
            assert fb[b] == d.obj(Xd[b]), ("f", b)
            assert np.array_equal(Gb[b], d.grad(Xd[b]).cpu().numpy()), ("g", b)
        if Y is not None:
            assert np.array_equal(Hb[b], d.hess_coord(Xd[b], Y[b], w).cpu().numpy()), ("hess", b)
    return Cb, Vb


PAIRS = [(p, s) for p in ct.PROBLEMS for s in ct.SCHEMES]


@pytest.mark.parametrize("prob", list(ct.PROBLEMS))
def test_batch_equals_single_calls_every_problem_and_scheme(torch_cuda, prob):
    """K = 3 members, N in {1, 5, 64} and a ragged grid; patterns manual / optimized, value orders CSC / CSR (the Hessian and the
    first-order callbacks on the first handle of each grid: their values do not depend on the Jacobian's pattern or order)"""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    for sch in ct.SCHEMES:
        for N, tg in ((1, None), (5, None), (64, None), (23, np.cumsum(rng.uniform(0.2, 1.8, 24)))):
            first = True
            for pattern in ("manual", "optimized"):
                for order in ("csc", "csr"):
                    import warnings
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        d = ct.DOCP(prob, N, sch, time_grid=tg, pattern=pattern, value_order=order, device=0)
                    Xd, _ = members(torch, d, prob, sch, 3)
                    Y = multipliers(torch, d, 3) if first else None
                    check_members(torch, d, Xd, Y, first_order=first)
                    first = False
                    d.close()


@pytest.mark.parametrize("prob,sch,N,K", [("goddard", "gauss_legendre_2", 10000, 16), ("quadrotor12", "gauss_legendre_3", 20000, 2)],
                         ids=["cfg2-K16", "quadrotor12-gl3-K2"])
def test_batch_full_size(oracle_lib, torch_cuda, prob, sch, N, K):
    torch = torch_cuda
    d = ct.DOCP(prob, N, sch, device=0)
    Xd, X = members(torch, d, prob, sch, K)
    Cb, Vb = check_members(torch, d, Xd, multipliers(torch, d, K))
    o = oracle_lib.OracleDOCP(prob, sch, N)
    assert relerr(Cb[0], o.constraints(X[0])) <= TOL
    assert relerr(Vb[0], o.jac_coord(X[0])) <= TOL
    f0 = float(d.obj_batch(Xd)[0])
    assert abs(f0 - o.objective(X[0])) / max(1.0, abs(o.objective(X[0]))) <= TOL


def test_batch_strided_buffers(torch_cuda):
    """X a row slice of a (K, nvar + 7) tensor; outputs with padded rows filled with a sentinel: padding untouched, members exact"""
    torch = torch_cuda
    prob, sch, N, K, pad = "goddard", "gauss_legendre_2", 300, 4, 7
    d = ct.DOCP(prob, N, sch, device=0)
    Xc, _ = members(torch, d, prob, sch, K)
    Xw = torch.full((K, d.dim_NLP_variables + pad), SENT, dtype=torch.float64, device="cuda")
    Xw[:, :d.dim_NLP_variables] = Xc
    X = Xw[:, :d.dim_NLP_variables]
    assert X.stride(0) == d.dim_NLP_variables + pad
    Y = multipliers(torch, d, K)
    Yw = torch.full((K, d.dim_NLP_constraints + pad), SENT, dtype=torch.float64, device="cuda")
    Yw[:, :d.dim_NLP_constraints] = Y

    def wide(n):
        return torch.full((K, n + pad), SENT, dtype=torch.float64, device="cuda")

    Cw, Vw, Gw, Hw = wide(d.dim_NLP_constraints), wide(d.nnzj), wide(d.dim_NLP_variables), wide(d.nnzh)
    d.cons_jac_batch(X, Cw[:, :d.dim_NLP_constraints], Vw[:, :d.nnzj])
    d.grad_batch(X, Gw[:, :d.dim_NLP_variables])
    d.hess_coord_batch(X, Yw[:, :d.dim_NLP_constraints], 0.7, Hw[:, :d.nnzh])
    f = d.obj_batch(X).cpu().numpy()
    for T, n in ((Cw, d.dim_NLP_constraints), (Vw, d.nnzj), (Gw, d.dim_NLP_variables), (Hw, d.nnzh)):
        assert np.all(T[:, n:].cpu().numpy() == SENT)
    for b in range(K):
        c, v = d.cons_jac(Xc[b])
        assert np.array_equal(Cw[b, :d.dim_NLP_constraints].cpu().numpy(), c.cpu().numpy())
        assert np.array_equal(Vw[b, :d.nnzj].cpu().numpy(), v.cpu().numpy())
        assert np.array_equal(Gw[b, :d.dim_NLP_variables].cpu().numpy(), d.grad(Xc[b]).cpu().numpy())
        assert np.array_equal(Hw[b, :d.nnzh].cpu().numpy(), d.hess_coord(Xc[b], Y[b], 0.7).cpu().numpy())
        assert f[b] == d.obj(Xc[b])


@pytest.mark.parametrize("sch", ["trapeze", "gauss_legendre_2"])
def test_batch_runtime_ocp(torch_cuda, sch):
    """a run-time OCP (hiprtc): the expression twin of a registry problem, K = 4"""
    torch = torch_cuda
    name = twin("goddard")
    d = ct.DOCP(name, 40, sch, device=0)
    Xd, _ = members(torch, d, "goddard", sch, 4)
    check_members(torch, d, Xd, multipliers(torch, d, 4))


def test_batch_of_one_is_the_single_call(torch_cuda):
    torch = torch_cuda
    d = ct.DOCP("quadrotor", 100, "gauss_legendre_3", device=0)
    Xd, _ = members(torch, d, "quadrotor", "gauss_legendre_3", 1)
    check_members(torch, d, Xd, multipliers(torch, d, 1), w=1.0)


def test_batch_members_with_their_own_multipliers(torch_cuda):
    """different multipliers per member, a shared obj_weight != 1: each member's Hessian is its own"""
    torch = torch_cuda
    d = ct.DOCP("goddard", 200, "midpoint", device=0)
    Xd, _ = members(torch, d, "goddard", "midpoint", 3)
    Xs = Xd[0].repeat(3, 1).contiguous()            # same iterate, different multipliers: only Y tells the members apart
    Y = multipliers(torch, d, 3)
    H = d.hess_coord_batch(Xs, Y, 2.5).cpu().numpy()
    assert not np.array_equal(H[0], H[1])
    for b in range(3):
        assert np.array_equal(H[b], d.hess_coord(Xs[b], Y[b], 2.5).cpu().numpy())


def test_batch_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    d = ct.DOCP("goddard", 50, "gauss_legendre_2", device=0)
    nvar, ncon, nnzj = d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzj
    X = torch.zeros((2, nvar), dtype=torch.float64, device="cuda")
    Cb = torch.zeros((2, ncon), dtype=torch.float64, device="cuda")
    Vb = torch.zeros((2, nnzj), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for batch in (0, 65536):
        assert L.ctd_cons_jac_batch_dev_async(d._h, batch, p(X), nvar, p(Cb), ncon, p(Vb), nnzj) == ct._lib.CTD_EINVAL
        assert b"batch" in L.ctd_last_error(d._h)
    assert L.ctd_cons_jac_batch_dev_async(d._h, 2, p(X), nvar, p(Cb), ncon - 1, p(Vb), nnzj) == ct._lib.CTD_EINVAL
    assert b"ldc" in L.ctd_last_error(d._h)
    shard = ct.DOCP("goddard", 50, "gauss_legendre_2", steps=(0, 25), device=0)
    assert L.ctd_cons_jac_batch_dev_async(shard._h, 2, p(X), nvar, p(Cb), ncon, p(Vb), nnzj) == ct._lib.CTD_EINVAL
    assert b"shard" in L.ctd_last_error(shard._h)
    d.sync()
