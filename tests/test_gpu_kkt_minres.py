"""The device-resident preconditioned MINRES solve of K z = r on the MI355X (ctd_kkt_minres*; DOCP.kkt_minres, kkt_minres_start,
kkt_minres_iters, kkt_minres_info), K = [[H + Sx, J'], [J, -Sc]] the operator of ctd_kktprod.

The reference is scipy.sparse.linalg.minres on K_asm, assembled on the CPU from the oracle in structural mode (minres_case, the
helper of test_gpu_diag.py with the transcription as parameters), preconditioned with vectors computed on the CPU from K_asm's own
blocks (asm_precond): no code under test is involved.

BARS
  first iterates   |z_k - z_k(scipy on K_asm)| / |z_k(scipy on K_asm)| <= 10 D_REF, k in {1, 2, 5}.  d_ref is the largest such
                   difference between scipy on K_asm and scipy with the GPU kktprod as its operator, over all cases; the factor 10
                   covers the different summation order of the inner products (a tree per workgroup against NumPy's sums),
                   compounding over five iterations.  D_REF is d_ref as measured on the MI355X (the test prints it): 2.28e-12
                   (goddard, trapeze, N = 7, preconditioned, k = 5); the largest device difference measured there is 3.92e-12.
                   Both were measured again with the N = 75 000 case included and did not move: that case's own largest
                   figures are 1.78e-12 through the GPU operator and 1.78e-12 on the device (preconditioned, k = 2), both
                   halves (plain and preconditioned) run -- assembling K_asm and the scipy runs take about 2 s at that size.
  the solve        N = 20 Goddard trapeze, seed 21, rtol 1e-10, cap 10 n: converged; iterations within +-2 of scipy's on K_asm
                   with the same M (the margin the project grants for last-bit differences of the operator); at most half those
                   of the unpreconditioned device solve; true residual |K_asm z - r| / |r| at most rho^2 times that of scipy's
                   run, rho the mean per-iteration reduction of scipy's true residual over its last five iterations (the two runs
                   may stop two iterations apart; rho is not allowed below 1: the solve is not asked to beat the reference).
                   Measured on the MI355X: 72 iterations (scipy on K_asm: 72; precond="diag": 72; unpreconditioned device
                   solve: 310), residual 2.2915e-6 against scipy's 2.2916e-6, rho = 1.58 (rho^2 = 2.50).
Everything else is exact: bit equality (freeze, reproducibility, capture), statuses, iteration counts, refusals.

Workgroups: the vector kernels give a workgroup 1024 elements, up to 512 workgroups, then longer chunks (krylov_geom of
ctd_krylov_kernels.hpp; `krylov_geom` below restates the rule and reads its constants from that header).  Of the cases below
N = 300 (n = 2109) spans 3 workgroups and N = 2000 (n = 14009) spans 14: the partial-sum path and its order are exercised.
N = 75 000 (n = 525 009) is the capped geometry: 512 workgroups with a chunk of 1280 elements, so a thread makes five passes, one
past the four unrolled ones, every thread adds 512 partial sums, and the workgroups 411 to 511 own nothing (asserted next to
CASES, without a GPU).  Every other case is one workgroup, N = 1 (n = 16) less than one wave."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe
from jit_defs import twin
from oracle.oracle import OracleDOCP

pytestmark = pytest.mark.gpu

D_REF = 2.281364561561445e-12            # d_ref on the MI355X over all CASES, N = 75 000 included (goddard, trapeze, N = 7, preconditioned, k = 5)
BAR = 10.0 * D_REF
KS = (1, 2, 5)
# (problem, scheme, N, run-time twin)
CASES = [("goddard", "trapeze", N, False) for N in (1, 2, 7, 20, 300, 2000)] + \
        [("double_integrator_path", "midpoint", 7, False), ("goddard", "gauss_legendre_2", 7, False), ("goddard", "midpoint", 7, True)] + \
        [("goddard", "trapeze", 75000, False)]
CAPPED = CASES[-1]                       # the case of the capped workgroup count; n = 7 N + 9 (4 N + 5 variables, 3 N + 4 constraints)
CAPPED_N = 7 * CAPPED[2] + 9


def krylov_constants():
    """kKrylovBlock, kKrylovSpan, kKrylovMaxWg as csrc/ctd_krylov_kernels.hpp has them"""
    hpp = os.path.join(os.path.dirname(os.path.abspath(ct.__file__)), "csrc", "ctd_krylov_kernels.hpp")
    with open(hpp) as f:
        text = f.read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) for name in ("kKrylovBlock", "kKrylovSpan", "kKrylovMaxWg"))


def krylov_geom(n):
    """(nwg, chunk) by the rule stated in ctd_krylov_kernels.hpp: min(kKrylovMaxWg, ceil(n / kKrylovSpan)) workgroups, at least one;
    chunk = ceil(n / nwg) rounded up to a multiple of kKrylovBlock"""
    block, span, max_wg = krylov_constants()
    nwg = max(1, min(max_wg, -(-n // span)))
    chunk = -(-(-(-n // nwg)) // block) * block
    return nwg, chunk


def capped_geometry():
    """what the N = 75 000 case is there for: the workgroup count at its cap, more passes per thread than the four unrolled ones
    (chunk > 1024), trailing workgroups that own nothing ((nwg - 1) chunk >= n).  Returns (nwg, chunk, first empty workgroup)"""
    nwg, chunk = krylov_geom(CAPPED_N)
    assert nwg == 512, (nwg, chunk)
    assert chunk > 1024, (nwg, chunk)
    assert (nwg - 1) * chunk >= CAPPED_N, (nwg, chunk, CAPPED_N)
    return nwg, chunk, -(-CAPPED_N // chunk)


assert capped_geometry() == (512, 1280, 411)                # (checked wherever this module is collected; tests/test_kkt_minres_cpu.py too)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def csc_coo(colptr, rowval):
    return np.asarray(rowval, dtype=np.int64), np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))


def dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@functools.lru_cache(maxsize=None)
def minres_case(prob="goddard", sch="trapeze", N=20):
    """structural pattern: the seeded inputs (seed 21), K_asm assembled from the oracle, its blocks H and J.  N = 20 only: sx is
    shifted by max(0, -lambda_min(H)) (a dense eigendecomposition) so that K is quasi-definite, as in test_gpu_diag.py; the
    fixed-k cases do not need definiteness.  Computed once per transcription and shared: nobody writes to the result"""
    import scipy.sparse as sp
    o = OracleDOCP(prob, sch, N)
    o.set_pattern_mode(1)
    x = bench_inputs(describe(o, prob, sch), perturb=1e-3)
    nvar = len(x)
    jr, jc = csc_coo(*o.jac_pattern())
    jv = o.jac_coord(x)
    ncon = int(jr.max()) + 1
    r = np.random.default_rng(21)
    y = 0.1 * r.uniform(-1.0, 1.0, ncon)
    hr, hc = csc_coo(*o.hess_pattern())
    vals, dropped = o.hess_coord(x, y, 1.0, return_dropped=True)
    assert dropped[1] == 0
    Hl = sp.csr_matrix((vals, (hr, hc)), shape=(nvar, nvar))
    H = (Hl + sp.tril(Hl, -1).T).tocsr()
    lam_min = float(np.linalg.eigvalsh(H.toarray())[0]) if N == 20 else 0.0
    sx = 10.0 ** r.uniform(-3.0, 5.0, nvar) + max(0.0, -lam_min)
    sc = 1e-2 * r.uniform(1.0, 2.0, ncon)
    rhs = r.uniform(-1.0, 1.0, nvar + ncon)
    J = sp.csr_matrix((jv, (jr, jc)), shape=(ncon, nvar))
    K_asm = sp.bmat([[H + sp.diags(sx), J.T], [J, -sp.diags(sc)]]).tocsr()
    return dict(prob=prob, sch=sch, N=N, x=x, y=y, sx=sx, sc=sc, rhs=rhs, H=H, J=J, K_asm=K_asm, nvar=nvar, ncon=ncon)


def asm_precond(c, floor=1e-8):
    """the preconditioner of DOCP.kkt_diag_precond from K_asm's own blocks"""
    px = np.maximum(np.abs(c["H"].diagonal() + c["sx"]), floor)
    pc = np.asarray(c["J"].multiply(c["J"]) @ (1.0 / px)).ravel() + c["sc"]
    return px, pc


def diag_op(px, pc):
    m = 1.0 / np.r_[px, pc]
    return LinearOperator((len(m), len(m)), matvec=lambda v: m * np.asarray(v).ravel(), dtype=np.float64)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Solve:
    """the N = 20 case on a handle, its inputs on the device"""
    def __init__(self, torch, c=None, **kw):
        self.c = c = c or minres_case()
        self.n = c["nvar"] + c["ncon"]
        self.d = ct.DOCP(c["prob"], c["N"], c["sch"], device=0, **{"pattern": "structural", **kw})
        assert (self.d.dim_NLP_variables, self.d.dim_NLP_constraints) == (c["nvar"], c["ncon"])
        self.px, self.pc = asm_precond(c)
        self.x, self.y, self.sx, self.sc, self.rhs, self.pxd, self.pcd = dev(torch, c["x"], c["y"], c["sx"], c["sc"], c["rhs"], self.px, self.pc)

    def run(self, pre=True, rhs=None, **kw):
        precond = (self.pxd, self.pcd) if pre is True else (pre or None)
        return self.d.kkt_minres(self.x, self.y, self.rhs if rhs is None else rhs, sx=self.sx, sc=self.sc, precond=precond, **kw)

    def res(self, z):
        z = z if isinstance(z, np.ndarray) else z.cpu().numpy()
        return float(np.linalg.norm(self.c["K_asm"] @ z - self.c["rhs"]) / np.linalg.norm(self.c["rhs"]))


@pytest.fixture(scope="module")
def solve20(torch_cuda):
    return Solve(torch_cuda)


# ---- 1. first iterates -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_iterates(torch_cuda):
    """per case, preconditioner and k: (|z_dev - z_asm| / |z_asm|, |z_op - z_asm| / |z_asm|, iterations the device reports)"""
    torch = torch_cuda
    out = {}
    for prob, sch, N, rt in CASES:
        c = minres_case(prob, sch, N)
        nvar, ncon, n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
        d = ct.DOCP(twin(prob) if rt else prob, N, sch, device=0, pattern="structural")
        assert (d.dim_NLP_variables, d.dim_NLP_constraints) == (nvar, ncon)
        xd, yd, sxd, scd, rhsd = dev(torch, c["x"], c["y"], c["sx"], c["sc"], c["rhs"])
        zin = torch.empty(n, dtype=torch.float64, device="cuda")
        zout = torch.empty(n, dtype=torch.float64, device="cuda")
        z = torch.empty(n, dtype=torch.float64, device="cuda")

        def matvec(v):
            zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
            d.kktprod(xd, yd, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=sxd, sc=scd, out=(zout[:nvar], zout[nvar:]))
            return zout.cpu().numpy()

        K_op = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
        px, pc = asm_precond(c)
        assert (px > 0).all() and (pc > 0).all()
        for pre in (False, True):
            M = diag_op(px, pc) if pre else None
            precond = tuple(dev(torch, px, pc)) if pre else None
            for k in KS:
                z_asm, _ = minres(c["K_asm"], c["rhs"], M=M, rtol=0.0, maxiter=k)
                z_op, _ = minres(K_op, c["rhs"], M=M, rtol=0.0, maxiter=k)
                z.fill_(7.0)
                d.kkt_minres_start(xd, yd, rhsd, z, sx=sxd, sc=scd, precond=precond, rtol=0.0)
                d.kkt_minres_iters(xd, yd, z, k, sx=sxd, sc=scd)
                info = d.kkt_minres_info()
                out[(prob, sch, N, rt, pre, k)] = (rel(z.cpu().numpy(), z_asm), rel(z_op, z_asm), info)
    return out


def test_first_iterates_reference_spread(first_iterates):
    """d_ref, the largest difference between scipy on K_asm and scipy through the GPU operator: what D_REF records"""
    d_ref = max(v[1] for v in first_iterates.values())
    worst = max(first_iterates, key=lambda key: first_iterates[key][1])
    print("d_ref", d_ref, "at", worst, "| D_REF", D_REF, "| largest device difference", max(v[0] for v in first_iterates.values()))
    assert np.isfinite(d_ref)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-N{c[2]}" + ("-rt" if c[3] else ""))
def test_first_iterates(first_iterates, case):
    for pre in (False, True):
        for k in KS:
            err, ref, info = first_iterates[case + (pre, k)]
            print(case, "preconditioned" if pre else "plain", "k", k, "device vs K_asm", err, "GPU operator vs K_asm", ref, info)
            assert info.iterations == k and info.status == "running", info
            assert err <= BAR, (case, pre, k, err, BAR)


# ---- 2. the solve ------------------------------------------------------------------------------------------------------------------
def scipy_solve(c, M, cap):
    """scipy's run on K_asm: (z, info, iterations, true residuals of its iterates)"""
    nrm = np.linalg.norm(c["rhs"])
    res = []
    z, info = minres(c["K_asm"], c["rhs"], M=M, rtol=1e-10, maxiter=cap,
                     callback=lambda zk: res.append(float(np.linalg.norm(c["K_asm"] @ zk - c["rhs"]) / nrm)))
    return z, info, len(res), res


def test_solve(solve20):
    s = solve20
    cap = 10 * s.n
    z_ref, info_ref, it_ref, res = scipy_solve(s.c, diag_op(s.px, s.pc), cap)
    assert info_ref == 0
    rho = max(1.0, (res[-6] / res[-1]) ** 0.2)
    z, info = s.run(rtol=1e-10, max_iter=cap)
    z0, info0 = s.run(pre=False, rtol=1e-10, max_iter=cap)
    zd, infod = s.run(pre="diag", rtol=1e-10, max_iter=cap)
    it0 = info0.iterations if info0.status == "converged" else cap
    print("scipy on K_asm: iterations", it_ref, "residual", res[-1], "rho", rho, "| device:", info, "residual", s.res(z),
          "| plain device:", info0, "residual", s.res(z0), "| precond='diag':", infod, "residual", s.res(zd))
    assert info.status == "converged", info
    assert abs(info.iterations - it_ref) <= 2, (info.iterations, it_ref)
    assert 2 * info.iterations <= it0, (info.iterations, it0)
    assert s.res(z) <= rho * rho * res[-1], (s.res(z), res[-1], rho)
    assert infod.status == "converged" and abs(infod.iterations - it_ref) <= 2, (infod, it_ref)
    assert info.beta1 > 0 and info.phibar < info.beta1 and info.Anorm > 0 and info.ynorm > 0, info
    assert abs(info.ynorm - float(np.linalg.norm(z.cpu().numpy()))) <= 1e-12 * info.ynorm, info      # (the sums it is formed from)


# ---- 3. freeze ---------------------------------------------------------------------------------------------------------------------
def test_freeze(solve20):
    s = solve20
    cap = 10 * s.n
    z1, info1 = s.run(rtol=1e-10, max_iter=cap, check_every=1)
    z16, info16 = s.run(rtol=1e-10, max_iter=cap, check_every=16)
    assert info1.status == "converged" and info1 == info16, (info1, info16)
    assert info1.iterations % 16 != 0            # (the second run overshoots: frozen iterations ran)
    assert np.array_equal(z1.cpu().numpy(), z16.cpu().numpy())
    # further iterations after convergence: no bit of z or of the state changes
    before = z16.clone()
    s.d.kkt_minres_iters(s.x, s.y, z16, 8, sx=s.sx, sc=s.sc)
    assert s.d.kkt_minres_info() == info16
    assert np.array_equal(z16.cpu().numpy(), before.cpu().numpy())


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------------
def test_reproducible_host_device_offset(torch_cuda, solve20):
    """two calls, host entry == device entry, and rhs / z as views at an odd multiple of 8 bytes"""
    torch = torch_cuda
    s, c = solve20, solve20.c
    za, ia = s.run(rtol=0.0, max_iter=12)
    zb, ib = s.run(rtol=0.0, max_iter=12)
    assert ia.status == "max_iter" and ia.iterations == 12 and ia == ib
    assert np.array_equal(za.cpu().numpy(), zb.cpu().numpy())
    zh, ih = s.d.kkt_minres(c["x"], c["y"], c["rhs"], sx=c["sx"], sc=c["sc"], precond=(s.px, s.pc), rtol=0.0, max_iter=12)
    assert ih == ia and np.array_equal(zh, za.cpu().numpy())
    zh0, ih0 = s.d.kkt_minres(c["x"], None, c["rhs"], rtol=0.0, max_iter=12)             # every optional argument left out
    zd0, id0 = s.d.kkt_minres(s.x, None, s.rhs, rtol=0.0, max_iter=12)
    assert ih0 == id0 and np.array_equal(zh0, zd0.cpu().numpy())
    odd_offset_equals_aligned(torch, s, za, ia, 12)
    # the same at the capped workgroup count (CAPPED: five passes per thread, 512 partial sums, empty trailing workgroups)
    big = Solve(torch, minres_case(*CAPPED[:3]))
    assert krylov_geom(big.n)[0] == 512 and big.n == CAPPED_N
    zA, iA = big.run(rtol=0.0, max_iter=6)
    assert iA.status == "max_iter" and iA.iterations == 6, iA
    odd_offset_equals_aligned(torch, big, zA, iA, 6)
    big.d.close()


def odd_offset_equals_aligned(torch, s, za, ia, max_iter):
    """rhs and z as views at an odd multiple of 8 bytes, z between guards: the bits and the info of the aligned run (za, ia)"""
    buf_r = torch.zeros(s.n + 1, dtype=torch.float64, device="cuda")
    buf_z = torch.full((s.n + 3,), 7.0, dtype=torch.float64, device="cuda")
    buf_r[1:].copy_(s.rhs)
    assert buf_r[1:].data_ptr() % 16 == 8 and buf_z[1:s.n + 1].data_ptr() % 16 == 8
    zo, io = s.run(rhs=buf_r[1:], rtol=0.0, max_iter=max_iter, out=buf_z[1:s.n + 1])
    assert io == ia and np.array_equal(zo.cpu().numpy(), za.cpu().numpy())
    assert float(buf_z[0]) == 7.0 and bool((buf_z[s.n + 1:] == 7.0).all())


def test_pattern_independence(torch_cuda):
    """every pattern mode / value order of one transcription: the same bits"""
    c = minres_case("goddard", "trapeze", 7)
    results = []
    for kw in (dict(pattern="manual"), dict(pattern="structural"), dict(pattern="optimized"), dict(pattern="structural", value_order="csr"),
               dict(pattern="manual", value_order="csr")):
        z, info = Solve(torch_cuda, c, **kw).run(rtol=0.0, max_iter=9)
        results.append((z.cpu().numpy(), info))
    for z, info in results[1:]:
        assert info == results[0][1] and np.array_equal(z, results[0][0])


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------
def test_graph_capture(torch_cuda, solve20):
    torch = torch_cuda
    s = Solve(torch, solve20.c)
    d, nvar = s.d, s.c["nvar"]
    pre = (s.pxd, s.pcd)
    z = torch.empty(s.n, dtype=torch.float64, device="cuda")
    kv = torch.empty(s.n, dtype=torch.float64, device="cuda")

    def kktprod():
        d.kktprod(s.x, s.y, s.rhs[:nvar], s.rhs[nvar:], sx=s.sx, sc=s.sc, out=(kv[:nvar], kv[nvar:]), sync=False)

    def three():
        d.kkt_minres_start(s.x, s.y, s.rhs, z, sx=s.sx, sc=s.sc, precond=pre, rtol=0.0)
        d.kkt_minres_iters(s.x, s.y, z, 3, sx=s.sx, sc=s.sc)

    side = torch.cuda.Stream()
    d.set_stream(side)
    with torch.cuda.stream(side):
        kktprod()
        three()                         # the warm call: workspace, partial sums
    side.synchronize()
    z_eager, kv_eager, info_eager = z.cpu().numpy(), kv.cpu().numpy(), d.kkt_minres_info()
    assert info_eager.iterations == 3
    gk = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gk, stream=side):
        kktprod()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        three()
    z.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy(), z_eager) and d.kkt_minres_info() == info_eager
    g.replay()                          # a replay after a replay: nothing of the arguments depends on the launches before
    torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy(), z_eager) and d.kkt_minres_info() == info_eager
    kv.fill_(0.0)
    gk.replay()
    torch.cuda.synchronize()
    assert np.array_equal(kv.cpu().numpy(), kv_eager)


# ---- 6. status paths ---------------------------------------------------------------------------------------------------------------
def test_status_paths(torch_cuda, solve20):
    torch = torch_cuda
    s = solve20
    # M not positive definite.  MINRES sees M only through r' M r: an entry of pc is negative and small, so its term decides the sign
    pc = s.pcd.clone()
    pc[3] = -1e-12
    z, info = s.run(pre=(s.pxd, pc), rtol=1e-10, max_iter=50)
    assert info.status == "breakdown" and info.iterations == 0, info
    assert bool(torch.isfinite(z).all()) and not bool(z.any())
    # rhs = 0
    z, info = s.run(rhs=torch.zeros_like(s.rhs), rtol=1e-10, max_iter=50)
    assert info.status == "converged" and info.iterations == 0 and not bool(z.any()), info
    # the iteration cap
    z, info = s.run(rtol=1e-10, max_iter=3)
    assert info.status == "max_iter" and info.iterations == 3, info
    z3, info3 = s.run(rtol=1e-10, max_iter=3, check_every=1)
    assert info3 == info and np.array_equal(z3.cpu().numpy(), z.cpu().numpy())
    # a NaN in rhs: breakdown within the first chunk
    rhs = s.rhs.clone()
    rhs[5] = float("nan")
    z, info = s.run(rhs=rhs, rtol=1e-10, max_iter=50, check_every=4)
    assert info.status == "breakdown" and info.iterations <= 4, info


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    L, lib = ct._lib.lib(), ct._lib
    E = lib.CTD_EINVAL
    d = ct.DOCP("goddard", 20, "midpoint", device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    n = nvar + ncon
    t = lambda k, v: torch.full((k,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    x, y, sx, sc, px, pc, rhs, z = t(nvar, 1.0), t(ncon, 0.1), t(nvar, 1.0), t(ncon, 1.0), t(nvar, 2.0), t(ncon, 2.0), t(n, 1.0), t(n, 7.0)
    P = lambda a: None if a is None else a.data_ptr()        # noqa: E731
    V = lambda a: None if a is None else C.c_void_p(a.data_ptr())        # noqa: E731

    def system(**kw):
        a = {"x": x, "y": y, "sx": sx, "sc": sc, "px": px, "pc": pc, **kw}
        return lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, **{k: P(v) for k, v in a.items()})

    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    calls = {
        "ctd_kkt_minres_start_dev_async": lambda h, ks, r, zz, rtol=1e-10, mi=10, ce=2: L.ctd_kkt_minres_start_dev_async(h, C.byref(ks), V(r), V(zz), rtol),
        "ctd_kkt_minres_dev": lambda h, ks, r, zz, rtol=1e-10, mi=10, ce=2: L.ctd_kkt_minres_dev(h, C.byref(ks), V(r), V(zz), rtol, mi, ce, C.byref(info)),
    }

    def refused(h, name, what):
        err = L.ctd_last_error(h._h)
        assert err.startswith(name.encode() + b": ") and what in err, (name, what, err)
        d.sync()
        assert bool((z == 7.0).all()), name

    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(0, 10))
    sh = ct.DOCP("goddard", 20, "midpoint", device=0)
    sh.set_x_shards([0, 20], [x.data_ptr()], 0)
    iters = lambda h, ks, zz, k: L.ctd_kkt_minres_iters_dev_async(h, C.byref(ks), V(zz), k)        # noqa: E731
    # iterations before any start
    assert iters(d._h, system(), z, 1) == E
    refused(d, "ctd_kkt_minres_iters_dev_async", b"no solve has been started")
    for name, call in calls.items():
        for ks, r, zz in ((system(x=None), rhs, z), (system(), None, z), (system(), rhs, None)):
            assert call(d._h, ks, r, zz) == E, name
            refused(d, name, b"null")
        for ks, r, zz, keep in ((system(), rhs, x, x), (system(), rhs, rhs, rhs), (system(), rhs, sc, sc), (system(), rhs, pc, pc)):
            before = keep.clone()
            assert call(d._h, ks, r, zz) == E, name
            refused(d, name, b"input")
            assert torch.equal(keep, before), name
        for ks in (system(px=None), system(pc=None)):
            assert call(d._h, ks, rhs, z) == E, name
            refused(d, name, b"px and pc")
        assert call(d._h, system(), rhs, z, -1.0) == E and call(d._h, system(), rhs, z, float("nan")) == E, name
        refused(d, name, b"rtol")
        for h in (s, sh):
            assert call(h._h, system(), rhs, z) == E, name
            refused(h, name, b"shard")
            assert b"no shard form" in L.ctd_last_error(h._h), name
    for mi, ce, what in ((0, 2, b"max_iter"), (-3, 2, b"max_iter"), (10, 0, b"check_every")):
        assert calls["ctd_kkt_minres_dev"](d._h, system(), rhs, z, 1e-10, mi, ce) == E
        refused(d, "ctd_kkt_minres_dev", what)
    assert iters(d._h, system(), z, 1) == E          # (still no start: every start above was refused)
    # after a start: k < 1, another z, the same refusals of pointers
    zz = t(n, 0.0)
    assert calls["ctd_kkt_minres_start_dev_async"](d._h, system(), rhs, zz) == 0
    for k in (0, -1):
        assert iters(d._h, system(), zz, k) == E
        refused(d, "ctd_kkt_minres_iters_dev_async", b"k = ")
    assert iters(d._h, system(), z, 1) == E
    refused(d, "ctd_kkt_minres_iters_dev_async", b"not the iterate")
    assert iters(d._h, system(x=None), zz, 1) == E and iters(d._h, system(), None, 1) == E
    refused(d, "ctd_kkt_minres_iters_dev_async", b"null")
    assert iters(s._h, system(), zz, 1) == E
    refused(s, "ctd_kkt_minres_iters_dev_async", b"shard")
    # the optional inputs may be NULL, and the refused calls left the solve usable
    assert iters(d._h, system(y=None, sx=None, sc=None, px=None, pc=None), zz, 2) == 0
    assert L.ctd_kkt_minres_info(d._h, C.byref(info)) == 0 and info.iterations == 2
    # the host entry
    xs, rs, zs = np.ones(nvar), np.ones(n), np.full(n, 7.0)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    hs = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, x=xs.ctypes.data)
    for r, zz_, what in ((None, zs, b"null"), (rs, None, b"null"), (rs, rs, b"input")):
        assert L.ctd_kkt_minres(d._h, C.byref(hs), dp(r), dp(zz_), 1e-10, 10, 2, C.byref(info)) == E
        assert L.ctd_last_error(d._h).startswith(b"ctd_kkt_minres: ") and what in L.ctd_last_error(d._h)
    assert (zs == 7.0).all()
