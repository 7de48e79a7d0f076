"""The chunked block-tridiagonal Schur preconditioner on the MI355X (ctd_kkt_schur_*, ctd_kkt_minres_schur_*; DOCP.kkt_schur_precond,
kkt_schur_factor, kkt_schur_solve, kkt_schur_info, kkt_minres(precond=P)).

The reference is the dense NumPy / scipy statement of the contract in tests/schur_ref.py on K_asm's own blocks (minres_case and
asm_precond of test_gpu_kkt_minres.py): no code under test is involved.  The preconditioner's (px, pc) are asm_precond's, uploaded,
and the Jacobian values are the handle's own cons_jac (CSR handles, structural pattern).

BARS
  factor + solve   backward error eta = |T y - r|_inf / (|T|_inf |y|_inf + |r|_inf) of kkt_schur_solve against the dense T at most
                   max(10 eta_ref, 64 eps), eta_ref that of scipy.linalg.cho_solve on the same T and r (per chunk): the factor 10
                   covers the different elimination order.  Measured on the MI355X: eta at most 6.7e-17 (goddard, trapeze, N = 20,
                   L = 1; cho_solve there: 1.1e-17), on every case below 64 eps.
  symmetry         |u . (M v) - (M u) . v| <= 1e-13 max(|u . (M v)|, |(M u) . v|) for random u, v; and, the scale backward stability
                   gives (each product is the exact one of a matrix within c eps |M^-1| of M^-1, so the two sides differ by
                   (M u) . (dM1 - dM2) (M v)), <= 1e-13 |M^-1|_inf |M u| |M v|.  Measured on the MI355X: at most 5.2e-16 of the
                   inner product.
  first iterates   |z_k - z_k(scipy on K_asm with the CPU-built M)| / |...| <= 10 d_ref, k in {1, 2, 5}; d_ref the same distance for
                   scipy driven by the GPU kktprod and the GPU kkt_schur_solve, the maximum over all cases of the same run.
                   Measured on the MI355X: d_ref = 1.19e-11 (goddard, trapeze, N = 7, L = 3, k = 5), the largest device difference
                   1.32e-11.
  the solve        N = 20 (minres_case), L in {20, 8}: converged, iterations within +-2 of scipy's with the same M, at most half of
                   the device solve with precond="diag", true residual within rho^2 of scipy's (the rule of test_gpu_kkt_minres.py).
  the point        Goddard trapeze N = 300, sc = 1e-8 U(1, 2), one chunk: converged in at most a tenth of the iterations scipy needs
                   with the diagonal M on K_asm.
Everything else is exact: bit equality, statuses, refusals, write sets.

Beyond the issue's transcriptions the factor / solve test runs quadrotor Gauss-Legendre 2 (m = 25) and quadrotor12 Gauss-Legendre 3
(m = 49): the kernels are instantiated for blocks of up to 8, 16, 32 and 64 rows, and m = 3 and 9 reach only the first two."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from guarded import guarded
from jit_defs import twin
from schur_ref import SchurRef, small_sc_case
from test_gpu_kkt_minres import asm_precond, dev, diag_op, minres_case, rel, scipy_solve

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KS = (1, 2, 5)
# (problem, scheme, N, run-time twin)
CASES = [("goddard", "trapeze", N, False) for N in (1, 2, 7, 20, 300)] + \
        [("goddard", "gauss_legendre_2", 7, False), ("double_integrator_path", "midpoint", 7, False), ("goddard", "midpoint", 7, True)]
BIG_BLOCKS = [("quadrotor", "gauss_legendre_2", 3, False), ("quadrotor12", "gauss_legendre_3", 3, False)]
case_id = lambda c: f"{c[0]}-{c[1]}-N{c[2]}" + ("-rt" if c[3] else "")      # noqa: E731


def chunk_lengths(N):
    return sorted({1, min(3, N), N})


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class Case:
    """one transcription on a CSR handle: the inputs and asm_precond's (px, pc) on the device, the handle's Jacobian values"""
    def __init__(self, torch, case, c=None):
        prob, sch, N, rt = case
        self.torch, self.c = torch, c or minres_case(prob, sch, N)
        c = self.c
        self.nvar, self.ncon, self.n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
        self.d = ct.DOCP(twin(prob) if rt else prob, N, sch, device=0, pattern="structural", value_order="csr")
        assert (self.d.dim_NLP_variables, self.d.dim_NLP_constraints) == (self.nvar, self.ncon)
        self.lay = self.d.kkt_schur_layout()
        self.m, self.N, self.nv, self.nb = self.lay.block_rows, self.lay.N, self.lay.tail_cols, self.lay.first_tail_row
        self.px, self.pc = asm_precond(c)
        assert (self.px > 0).all() and (self.pc > 0).all()
        self.x, self.y, self.sx, self.sc, self.rhs, self.pxd, self.pcd = dev(torch, c["x"], c["y"], c["sx"], c["sc"], c["rhs"], self.px, self.pc)
        self.jvals = self.d.cons_jac(self.x)[1]

    def factor(self, L, px=None, ws=None):
        lay = self.d.kkt_schur_layout(L)
        ws = torch_empty(self.torch, lay.workspace) if ws is None else ws
        return self.d.kkt_schur_factor(self.jvals, self.pxd if px is None else px, self.pcd, self.sc, L, ws)

    def ref(self, L):
        return SchurRef(self.c, self.px, self.pc, self.m, self.N, self.nv, L)

    def apply_M(self, P, v):
        """M v on the device: variables / px, the block rows through kkt_schur_solve, the tail rows / pc"""
        out = self.torch.empty(self.n, dtype=self.torch.float64, device="cuda")
        out[:self.nvar] = v[:self.nvar] / P.px
        out[self.nvar + self.nb:] = v[self.nvar + self.nb:] / P.pc[self.nb:]
        self.d.kkt_schur_solve(P, v[self.nvar:].contiguous(), out=out[self.nvar:])
        return out

    def minres(self, P, **kw):
        return self.d.kkt_minres(self.x, self.y, self.rhs, sx=self.sx, sc=self.sc, precond=P, **kw)

    def res(self, z):
        return float(np.linalg.norm(self.c["K_asm"] @ z.cpu().numpy() - self.c["rhs"]) / np.linalg.norm(self.c["rhs"]))


def torch_empty(torch, n):
    return torch.empty(n, dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def cases(torch_cuda):
    return {case: Case(torch_cuda, case) for case in CASES + BIG_BLOCKS}


# ---- 1. factor and solve against the dense reference ---------------------------------------------------------------------------------
def backward_error(T, y, r):
    return float(np.abs(T @ y - r).max() / (np.abs(T).sum(axis=1).max() * np.abs(y).max() + np.abs(r).max()))


@pytest.mark.parametrize("case", CASES + BIG_BLOCKS, ids=case_id)
def test_factor_solve(torch_cuda, cases, case):
    s = cases[case]
    r = np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon)
    rd, = dev(torch_cuda, r)
    for L in chunk_lengths(s.N):
        P = s.factor(L)
        assert s.d.kkt_schur_info(P) == -1
        out = torch_cuda.full((s.ncon,), 7.0, dtype=torch_cuda.float64, device="cuda")
        s.d.kkt_schur_solve(P, rd, out=out)
        y = out.cpu().numpy()
        assert (y[s.nb:] == 7.0).all(), "the tail rows of out are left untouched"
        R = s.ref(L)
        eta = backward_error(R.T, y[:s.nb], r[:s.nb])
        eta_ref = backward_error(R.T, R.solve_rows(r[:s.nb]), r[:s.nb])
        print(case_id(case), "L", L, "eta", eta, "eta_ref (cho_solve)", eta_ref, "forward difference", rel(y[:s.nb], R.solve_rows(r[:s.nb])))
        assert eta <= max(10.0 * eta_ref, 64.0 * EPS), (case, L, eta, eta_ref)


# ---- 2. symmetry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_symmetry(torch_cuda, cases, case):
    s = cases[case]
    g = np.random.default_rng(9)
    u, v = dev(torch_cuda, g.uniform(-1.0, 1.0, s.n), g.uniform(-1.0, 1.0, s.n))
    for L in chunk_lengths(s.N):
        P = s.factor(L)
        Mu, Mv = s.apply_M(P, u), s.apply_M(P, v)
        a, b = float(u @ Mv), float(Mu @ v)
        R = s.ref(L)
        norm_minv = max(float(s.px.max()), float(np.abs(R.T).sum(axis=1).max()), float(s.pc[s.nb:].max()) if s.nb < s.ncon else 0.0)
        scale = norm_minv * float(Mu.norm()) * float(Mv.norm())
        print(case_id(case), "L", L, "u.Mv", a, "Mu.v", b, "difference / scale", abs(a - b) / scale, "difference / |u.Mv|", abs(a - b) / abs(a))
        assert abs(a - b) <= 1e-13 * max(abs(a), abs(b)), (case, L, a, b)
        assert abs(a - b) <= 1e-13 * scale, (case, L, a, b, scale)


# ---- 3. chunk lengths past N are one chunk -------------------------------------------------------------------------------------------
def test_one_chunk_is_one_chunk(torch_cuda, cases):
    s = cases[("goddard", "trapeze", 7, False)]
    Pa, Pb = s.factor(s.N), s.factor(s.N + 5)
    assert Pa.layout.n_chunks == Pb.layout.n_chunks == 1
    s.d.sync()
    assert torch_cuda.equal(Pa.ws.view(torch_cuda.int64), Pb.ws.view(torch_cuda.int64))
    r, = dev(torch_cuda, np.random.default_rng(2).uniform(-1.0, 1.0, s.ncon))
    assert torch_cuda.equal(s.d.kkt_schur_solve(Pa, r), s.d.kkt_schur_solve(Pb, r))


# ---- 4. first iterates ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_iterates(torch_cuda, cases):
    """per case, chunk length and k: (|z_dev - z_asm| / |z_asm|, |z_op - z_asm| / |z_asm|, the device's info)"""
    torch = torch_cuda
    out = {}
    for case in CASES:
        s = cases[case]
        c, d, nvar, n = s.c, s.d, s.nvar, s.n
        zin, zout, z, rc, yc = (torch_empty(torch, k) for k in (n, n, n, s.ncon, s.ncon))

        def matvec(v):
            zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
            d.kktprod(s.x, s.y, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=s.sx, sc=s.sc, out=(zout[:nvar], zout[nvar:]))
            return zout.cpu().numpy()

        K_op = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
        for L in chunk_lengths(s.N):
            P = s.factor(L)
            R = s.ref(L)

            def gpu_M(v):
                v = np.asarray(v, dtype=np.float64).ravel()
                rc.copy_(torch.from_numpy(np.ascontiguousarray(v[nvar:])))
                d.kkt_schur_solve(P, rc, out=yc)
                return np.r_[v[:nvar] / s.px, yc[:s.nb].cpu().numpy(), v[nvar + s.nb:] / s.pc[s.nb:]]

            M_op = LinearOperator((n, n), matvec=gpu_M, dtype=np.float64)
            for k in KS:
                z_asm, _ = minres(c["K_asm"], c["rhs"], M=R.operator(), rtol=0.0, maxiter=k)
                z_op, _ = minres(K_op, c["rhs"], M=M_op, rtol=0.0, maxiter=k)
                z.fill_(7.0)
                d.kkt_minres_start(s.x, s.y, s.rhs, z, sx=s.sx, sc=s.sc, precond=P, rtol=0.0)
                d.kkt_minres_iters(s.x, s.y, z, k, sx=s.sx, sc=s.sc)
                info = d.kkt_minres_info()
                out[(case, L, k)] = (rel(z.cpu().numpy(), z_asm), rel(z_op, z_asm), info)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_first_iterates(first_iterates, case):
    d_ref = max(v[1] for v in first_iterates.values())
    worst = max(first_iterates, key=lambda key: first_iterates[key][1])
    print("d_ref", d_ref, "at", worst, "| largest device difference", max(v[0] for v in first_iterates.values()))
    assert np.isfinite(d_ref) and d_ref > 0.0
    for (cs, L, k), (err, ref, info) in first_iterates.items():
        if cs != case:
            continue
        print(case_id(case), "L", L, "k", k, "device vs K_asm", err, "GPU operator and solve vs K_asm", ref, info)
        assert info.iterations == k and info.status == "running", info
        assert err <= 10.0 * d_ref, (case, L, k, err, d_ref)


# ---- 5. the solve ---------------------------------------------------------------------------------------------------------------------
def test_solve(cases):
    s = cases[("goddard", "trapeze", 20, False)]
    cap = 10 * s.n
    zd, infod = s.minres("diag", rtol=1e-10, max_iter=cap)
    assert infod.status == "converged", infod
    for L in (20, 8):
        z_ref, info_ref, it_ref, res = scipy_solve(s.c, s.ref(L).operator(), cap)
        assert info_ref == 0
        rho = max(1.0, (res[-6] / res[-1]) ** 0.2)
        z, info = s.minres(s.factor(L), rtol=1e-10, max_iter=cap)
        print("L", L, "scipy with the same M: iterations", it_ref, "residual", res[-1], "rho", rho, "| device:", info, "residual", s.res(z),
              "| precond='diag':", infod)
        assert info.status == "converged", info
        assert abs(info.iterations - it_ref) <= 2, (info.iterations, it_ref)
        assert 2 * info.iterations <= infod.iterations, (info.iterations, infod.iterations)
        assert s.res(z) <= rho * rho * res[-1], (s.res(z), res[-1], rho)
    # precond="schur": built with the defaults (kkt_diag_precond's pair, one chunk)
    zs, infos = s.minres("schur", rtol=1e-10, max_iter=cap)
    assert infos.status == "converged" and 2 * infos.iterations <= infod.iterations, infos


# ---- 6. the point of the feature -----------------------------------------------------------------------------------------------------
def test_small_sc_long_grid(torch_cuda):
    case = ("goddard", "trapeze", 300, False)
    s = Case(torch_cuda, case, small_sc_case(minres_case(*case[:3])))
    it = [0]
    _, info_ref = minres(s.c["K_asm"], s.c["rhs"], M=diag_op(s.px, s.pc), rtol=1e-10, maxiter=20 * s.n, callback=lambda zk: it.__setitem__(0, it[0] + 1))
    assert info_ref == 0
    P = s.factor(s.N)
    z, info = s.minres(P, rtol=1e-10, max_iter=10 * s.n)
    print("scipy, diagonal M:", it[0], "iterations | device, one chunk:", info, "residual", s.res(z))
    assert info.status == "converged", info
    assert 10 * info.iterations <= it[0], (info.iterations, it[0])
    assert s.d.kkt_schur_info(P) == -1


# ---- 7. exactness ----------------------------------------------------------------------------------------------------------------------
def test_exactness(torch_cuda, cases):
    torch = torch_cuda
    s = cases[("goddard", "trapeze", 20, False)]
    cap = 10 * s.n
    P = s.factor(8)
    z1, info1 = s.minres(P, rtol=1e-10, max_iter=cap, check_every=1)
    z16, info16 = s.minres(s.factor(8), rtol=1e-10, max_iter=cap, check_every=16)
    assert info1.status == "converged" and info1 == info16, (info1, info16)
    assert info1.iterations % 16 != 0            # (the second run overshoots: frozen iterations ran)
    assert torch.equal(z1, z16)
    before = z16.clone()
    s.d.kkt_minres_iters(s.x, s.y, z16, 8, sx=s.sx, sc=s.sc)
    assert s.d.kkt_minres_info() == info16
    assert torch.equal(z16, before)


def test_graph_capture(torch_cuda, cases):
    torch = torch_cuda
    s = Case(torch, ("goddard", "trapeze", 20, False))
    d = s.d
    P = s.factor(8)
    z = torch_empty(torch, s.n)

    def three():
        d.kkt_minres_start(s.x, s.y, s.rhs, z, sx=s.sx, sc=s.sc, precond=P, rtol=0.0)
        d.kkt_minres_iters(s.x, s.y, z, 3, sx=s.sx, sc=s.sc)

    side = torch.cuda.Stream()
    d.sync()
    d.set_stream(side)
    with torch.cuda.stream(side):
        three()                         # the warm call: workspace, partial sums
    side.synchronize()
    z_eager, info_eager = z.cpu().numpy(), d.kkt_minres_info()
    assert info_eager.iterations == 3
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        three()
    for _ in range(2):                  # a replay, and a replay after a replay
        z.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(z.cpu().numpy(), z_eager) and d.kkt_minres_info() == info_eager


# ---- 8. breakdown ----------------------------------------------------------------------------------------------------------------------
def test_breakdown(torch_cuda, cases):
    s = cases[("goddard", "trapeze", 7, False)]
    px = s.pxd.clone()
    px[2 * s.d.discretization._step_variables_block] = -1e-9          # the first state of step 2: w = -1e9 on its column
    for L in (3, s.N):
        P = s.factor(L, px=px)
        bad = s.d.kkt_schur_info(P)
        print("L", L, "first bad block", bad)
        assert 0 <= bad <= 2, bad
        z, info = s.minres(P, rtol=1e-10, max_iter=50)
        assert info.status == "breakdown", info
        assert not bool(z.any()) and bool(torch_cuda.isfinite(z).all())


# ---- 9. write sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (0, 1))
def test_write_sets(torch_cuda, cases, shift):
    torch = torch_cuda
    s = cases[("goddard", "gauss_legendre_2", 7, False)]
    d, L = s.d, 3
    lay = d.kkt_schur_layout(L)
    G = lambda n, like=None: guarded(torch, n, shift, "cuda", like)      # noqa: E731
    # the run on ordinary tensors
    P0 = s.factor(L)
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    out0 = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    d.kkt_schur_solve(P0, r, out=out0)
    z0 = torch_empty(torch, s.n)
    d.kkt_minres_start(s.x, s.y, s.rhs, z0, sx=s.sx, sc=s.sc, precond=P0, rtol=0.0)
    d.kkt_minres_iters(s.x, s.y, z0, 1, sx=s.sx, sc=s.sc)
    d.sync()
    # ... and on guarded views
    ins = {nm: G(t.numel(), t).snapshot() for nm, t in (("jvals", s.jvals), ("px", s.pxd), ("pc", s.pcd), ("sc", s.sc), ("r", r), ("x", s.x),
                                                       ("y", s.y), ("sx", s.sx), ("rhs", s.rhs))}
    ws, out, z = G(lay.workspace), G(s.ncon, out0.new_full((s.ncon,), 7.0)), G(s.n)
    P = d.kkt_schur_factor(ins["jvals"].view, ins["px"].view, ins["pc"].view, ins["sc"].view, L, ws.view)
    d.sync()
    assert ws.guards_intact("factor") and ws.unwritten() == [], "the factor writes the whole workspace"
    fac = ws.bits().clone()
    d.kkt_schur_solve(P, ins["r"].view, out=out.view)
    assert out.guards_intact("solve") and torch.equal(ws.bits(), fac)
    assert torch.equal(out.bits(), out0.view(torch.int64))
    d.kkt_minres_start(ins["x"].view, ins["y"].view, ins["rhs"].view, z.view, sx=ins["sx"].view, sc=ins["sc"].view, precond=P, rtol=0.0)
    d.kkt_minres_iters(ins["x"].view, ins["y"].view, z.view, 1, sx=ins["sx"].view, sc=ins["sc"].view)
    d.sync()
    assert z.guards_intact("start + iteration") and ws.guards_intact("start + iteration")
    assert torch.equal(z.bits(), z0.view(torch.int64))
    # the solve inside MINRES writes its partial sums into the fixed part of the workspace and nothing else of it
    fixed = ct._lib.KKT_SCHUR_FIXED
    assert torch.equal(ws.bits()[fixed:], fac[fixed:]) and torch.equal(ws.bits()[:16], fac[:16])
    assert torch.equal(ws.bits(), P0.ws.view(torch.int64))
    for nm, g in ins.items():
        assert g.unchanged(nm)


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda, cases):
    torch = torch_cuda
    L, lib = ct._lib.lib(), ct._lib
    E = lib.CTD_EINVAL
    s = cases[("goddard", "trapeze", 7, False)]
    d = s.d
    P = s.factor(3)
    z = torch.full((s.n,), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    V = lambda a: None if a is None else C.c_void_p(a.data_ptr())        # noqa: E731
    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    bad = C.c_int64(0)

    def system(size=None, **kw):
        a = {"x": s.x, "y": s.y, "sx": s.sx, "sc": s.sc, "px": s.pxd, "pc": s.pcd, **kw}
        return lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system) if size is None else size, obj_weight=1.0,
                                  **{k: None if v is None else v.data_ptr() for k, v in a.items()})

    def refused(h, name, what):
        err = L.ctd_last_error(h._h)
        assert err.startswith(name.encode() + b": ") and what in err, (name, what, err)
        d.sync()
        assert bool((z == 7.0).all()) and bool((out == 7.0).all()), name

    factor = lambda h, jv, px, sc, cs, ws: L.ctd_kkt_schur_factor_dev_async(h, V(jv), V(px), V(sc), cs, V(ws))        # noqa: E731
    solve = lambda h, ws, r, o: L.ctd_kkt_schur_solve_dev_async(h, V(ws), V(r), V(o))        # noqa: E731
    start = lambda h, ks, ws, r, zz, rtol=1e-10: L.ctd_kkt_minres_schur_start_dev_async(h, C.byref(ks), V(ws), V(r), V(zz), rtol)        # noqa: E731
    drive = lambda h, ks, ws, r, zz, rtol=1e-10, mi=10, ce=2: L.ctd_kkt_minres_schur_dev(h, C.byref(ks), V(ws), V(r), V(zz), rtol, mi, ce, C.byref(info))        # noqa: E731
    # NULL handle
    assert factor(None, s.jvals, s.pxd, s.sc, 3, P.ws) == E and solve(None, P.ws, s.sc, out) == E
    assert start(None, system(), P.ws, s.rhs, z) == E and drive(None, system(), P.ws, s.rhs, z) == E
    # struct sizes
    for name, call in (("ctd_kkt_minres_schur_start_dev_async", start), ("ctd_kkt_minres_schur_dev", drive)):
        assert call(d._h, system(size=8), P.ws, s.rhs, z) == E
        refused(d, name, b"struct_size")
    # shard handles, CSC handles: before the pointers
    kw = dict(device=0, pattern="structural")
    shard = ct.DOCP("goddard", 7, "trapeze", steps=(0, 4), value_order="csr", **kw)
    csc = ct.DOCP("goddard", 7, "trapeze", **kw)
    for h, what in ((shard, b"no shard form"), (csc, b"CTD_ORDER_CSR")):
        assert factor(h._h, None, None, None, 3, None) == E
        refused(h, "ctd_kkt_schur_factor_dev_async", what)
        assert solve(h._h, None, None, None) == E
        refused(h, "ctd_kkt_schur_solve_dev_async", what)
        assert L.ctd_kkt_schur_info(h._h, None, None) == E
        refused(h, "ctd_kkt_schur_info", what)
        assert start(h._h, system(x=None), None, None, None) == E
        refused(h, "ctd_kkt_minres_schur_start_dev_async", what)
        assert drive(h._h, system(x=None), None, None, None) == E
        refused(h, "ctd_kkt_minres_schur_dev", what)
    # chunk_steps
    assert factor(d._h, s.jvals, s.pxd, s.sc, 0, P.ws) == E
    refused(d, "ctd_kkt_schur_factor_dev_async", b"chunk_steps")
    # null pointers
    for jv, px, ws in ((None, s.pxd, P.ws), (s.jvals, None, P.ws), (s.jvals, s.pxd, None)):
        assert factor(d._h, jv, px, s.sc, 3, ws) == E
        refused(d, "ctd_kkt_schur_factor_dev_async", b"null")
    for ws, r, o in ((None, s.sc, out), (P.ws, None, out), (P.ws, s.sc, None)):
        assert solve(d._h, ws, r, o) == E
        refused(d, "ctd_kkt_schur_solve_dev_async", b"null")
    assert L.ctd_kkt_schur_info(d._h, None, C.byref(bad)) == E and L.ctd_kkt_schur_info(d._h, V(P.ws), None) == E
    refused(d, "ctd_kkt_schur_info", b"null")
    for name, call in (("ctd_kkt_minres_schur_start_dev_async", start), ("ctd_kkt_minres_schur_dev", drive)):
        for ks, ws, r, zz in ((system(x=None), P.ws, s.rhs, z), (system(), P.ws, None, z), (system(), P.ws, s.rhs, None), (system(), None, s.rhs, z),
                              (system(px=None, pc=None), P.ws, s.rhs, z)):
            assert call(d._h, ks, ws, r, zz) == E, name
            refused(d, name, b"null")
        # aliasing
        assert call(d._h, system(), P.ws, s.rhs, s.rhs) == E
        refused(d, name, b"input")
        assert call(d._h, system(), s.rhs, s.rhs, z) == E
        refused(d, name, b"workspace")
        assert call(d._h, system(), P.ws, s.rhs, z, -1.0) == E
        refused(d, name, b"rtol")
    # aliasing of factor and solve
    assert factor(d._h, s.jvals, s.pxd, s.sc, 3, s.pxd) == E
    refused(d, "ctd_kkt_schur_factor_dev_async", b"input")
    assert solve(d._h, P.ws, s.sc, s.sc) == E
    refused(d, "ctd_kkt_schur_solve_dev_async", b"input")
    # a workspace that holds no factor: the solve stores nothing, the status query says so
    blank = torch.zeros(P.layout.workspace, dtype=torch.float64, device="cuda")
    assert solve(d._h, blank, s.sc, out) == 0
    d.sync()
    assert bool((out == 7.0).all())
    assert L.ctd_kkt_schur_info(d._h, V(blank), C.byref(bad)) == E
    refused(d, "ctd_kkt_schur_info", b"no factor")
    # the refused calls left the factor usable
    assert L.ctd_kkt_schur_info(d._h, V(P.ws), C.byref(bad)) == 0 and bad.value == -1
    # the first factor on a handle inside a capture
    fresh = ct.DOCP("goddard", 7, "trapeze", value_order="csr", **kw)
    ws = torch_empty(torch, P.layout.workspace)
    side = torch.cuda.Stream()
    fresh.set_stream(side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ws.zero_()                      # (so that the capture is not empty)
        st = factor(fresh._h, s.jvals, s.pxd, s.sc, 3, ws)
    assert st == E and b"capturing" in L.ctd_last_error(fresh._h)
