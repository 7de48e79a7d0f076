"""The log-depth exact block-tridiagonal Schur preconditioner on the MI355X (ctd_kkt_schur_cr_*, ctd_kkt_minres_schur_cr_*;
DOCP.kkt_schur_cr_precond, kkt_schur_cr_factor, kkt_schur_cr_solve, kkt_schur_cr_info, kkt_minres(precond=P)).

The reference throughout is the dense one-chunk T of tests/schur_ref.py (SchurRef with L = N) on K_asm's own blocks; the elimination
order itself is stated in tests/schur_cr_ref.py, which tests/test_kkt_schur_cr_cpu.py pins against the same dense T.  Case, and the
inputs (asm_precond's (px, pc), the handle's own cons_jac values), are those of tests/test_gpu_kkt_schur.py.

BARS (those of tests/test_gpu_kkt_schur.py, with the one-chunk matrix as the reference)
  factor + solve   eta = |T y - r|_inf / (|T|_inf |y|_inf + |r|_inf) <= max(10 eta_ref, 64 eps), eta_ref that of scipy.linalg.cho_solve
                   on the same T and r; info gives -1.
  symmetry         |u . (M v) - (M u) . v| <= 1e-13 max(|u . (M v)|, |(M u) . v|) and <= 1e-13 |M^-1|_inf |M u| |M v|.
  first iterates   |z_k - z_k(scipy on K_asm with the CPU-built dense M)| / |...| <= 10 d_ref, k in {1, 2, 5}; d_ref the same distance
                   for scipy driven by the GPU kktprod and the GPU kkt_schur_cr_solve, the maximum over the cases of the same run.
  the solve        N = 20: converged, iterations within +-2 of scipy's with the same M, true residual within rho^2 of scipy's.
  the point        Goddard trapeze N = 300, sc = 1e-8 U(1, 2): converged, iterations within +-2 of scipy's with the dense one-chunk M and
                   at most a tenth of scipy's with the diagonal M.
Everything else is exact: bit equality, statuses, refusals, write sets.  The Krylov workspace lives inside the handle: its state is
compared through kkt_minres_info, its vectors through z."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from guarded import guarded
from schur_cr_ref import SchurCrRef
from schur_ref import schur_T, small_sc_case
from test_gpu_kkt_minres import dev, diag_op, minres_case, rel, scipy_solve
from test_gpu_kkt_schur import Case, backward_error, case_id, torch_empty

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KS = (1, 2, 5)
FIXED = 512
# (problem, scheme, N, run-time twin)
CASES = [("goddard", "trapeze", N, False) for N in (1, 2, 3, 4, 5, 7, 8, 9, 20, 33, 300)] + \
        [("goddard", "gauss_legendre_2", 7, False), ("double_integrator_path", "midpoint", 7, False), ("goddard", "midpoint", 7, True)]
BIG_BLOCKS = [(p, s, N, False) for p, s in (("quadrotor", "gauss_legendre_2"), ("quadrotor12", "gauss_legendre_3")) for N in (3, 5)]
G7 = ("goddard", "trapeze", 7, False)
G20 = ("goddard", "trapeze", 20, False)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


@pytest.fixture(scope="module")
def cases(torch_cuda):
    return {case: Case(torch_cuda, case) for case in CASES + BIG_BLOCKS}


def factor(s, px=None, ws=None):
    lay = s.d.kkt_schur_cr_layout()
    assert (lay.N, lay.block_rows, lay.first_tail_row, lay.tail_cols) == (s.N, s.m, s.nb, s.nv)
    ws = torch_empty(s.torch, lay.workspace) if ws is None else ws
    return s.d.kkt_schur_cr_factor(s.jvals, s.pxd if px is None else px, s.pcd, s.sc, ws)


def factor_part(P):
    """the bits of the workspace that the factor owns: everything but the partial sums and the solve's scratch"""
    import torch
    lay = P.layout
    w = P.ws.view(torch.int64)
    return w[:16].clone(), w[FIXED:FIXED + lay.N + 3 * lay.N * lay.block_rows ** 2].clone()


def same_factor(torch, a, b):
    return all(torch.equal(x, y) for x, y in zip(factor_part(a), factor_part(b)))


def apply_M(s, P, v):
    """M v on the device: variables / px, the block rows through kkt_schur_cr_solve, the tail rows / pc"""
    out = s.torch.empty(s.n, dtype=s.torch.float64, device="cuda")
    out[:s.nvar] = v[:s.nvar] / P.px
    out[s.nvar + s.nb:] = v[s.nvar + s.nb:] / P.pc[s.nb:]
    s.d.kkt_schur_cr_solve(P, v[s.nvar:].contiguous(), out=out[s.nvar:])
    return out


# ---- 1. factor and solve against the dense reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + BIG_BLOCKS, ids=case_id)
def test_factor_solve(torch_cuda, cases, case):
    s = cases[case]
    r = np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon)
    rd, = dev(torch_cuda, r)
    keep = rd.clone()
    P = factor(s)
    assert s.d.kkt_schur_cr_info(P) == -1
    assert P.layout.n_levels == (s.N - 1).bit_length() and P.layout.solve_launches == 2 * P.layout.n_levels + 1
    out = torch_cuda.full((s.ncon,), 7.0, dtype=torch_cuda.float64, device="cuda")
    s.d.kkt_schur_cr_solve(P, rd, out=out)
    y = out.cpu().numpy()
    assert (y[s.nb:] == 7.0).all(), "the tail rows of out are left untouched"
    assert torch_cuda.equal(rd, keep), "r is not modified"
    R = s.ref(s.N)
    y_ref = R.solve_rows(r[:s.nb])
    eta = backward_error(R.T, y[:s.nb], r[:s.nb])
    eta_ref = backward_error(R.T, y_ref, r[:s.nb])
    print(case_id(case), "m", s.m, "levels", P.layout.n_levels, "eta", eta, "eta_ref (cho_solve)", eta_ref, "forward difference", rel(y[:s.nb], y_ref))
    assert eta <= max(10.0 * eta_ref, 64.0 * EPS), (case, eta, eta_ref)


# ---- 2. symmetry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_symmetry(torch_cuda, cases, case):
    s = cases[case]
    g = np.random.default_rng(9)
    u, v = dev(torch_cuda, g.uniform(-1.0, 1.0, s.n), g.uniform(-1.0, 1.0, s.n))
    P = factor(s)
    Mu, Mv = apply_M(s, P, u), apply_M(s, P, v)
    a, b = float(u @ Mv), float(Mu @ v)
    R = s.ref(s.N)
    norm_minv = max(float(s.px.max()), float(np.abs(R.T).sum(axis=1).max()), float(s.pc[s.nb:].max()) if s.nb < s.ncon else 0.0)
    scale = norm_minv * float(Mu.norm()) * float(Mv.norm())
    print(case_id(case), "u.Mv", a, "Mu.v", b, "difference / scale", abs(a - b) / scale, "difference / |u.Mv|", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b)), (case, a, b)
    assert abs(a - b) <= 1e-13 * scale, (case, a, b, scale)


# ---- 3. first iterates ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_iterates(torch_cuda, cases):
    """per case and k: (|z_dev - z_asm| / |z_asm|, |z_op - z_asm| / |z_asm|, the device's info)"""
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
        P = factor(s)
        M_ref = s.ref(s.N).operator()

        def gpu_M(v):
            v = np.asarray(v, dtype=np.float64).ravel()
            rc.copy_(torch.from_numpy(np.ascontiguousarray(v[nvar:])))
            d.kkt_schur_cr_solve(P, rc, out=yc)
            return np.r_[v[:nvar] / s.px, yc[:s.nb].cpu().numpy(), v[nvar + s.nb:] / s.pc[s.nb:]]

        M_op = LinearOperator((n, n), matvec=gpu_M, dtype=np.float64)
        for k in KS:
            z_asm, _ = minres(c["K_asm"], c["rhs"], M=M_ref, rtol=0.0, maxiter=k)
            z_op, _ = minres(K_op, c["rhs"], M=M_op, rtol=0.0, maxiter=k)
            z.fill_(7.0)
            d.kkt_minres_start(s.x, s.y, s.rhs, z, sx=s.sx, sc=s.sc, precond=P, rtol=0.0)
            d.kkt_minres_iters(s.x, s.y, z, k, sx=s.sx, sc=s.sc)
            info = d.kkt_minres_info()
            out[(case, k)] = (rel(z.cpu().numpy(), z_asm), rel(z_op, z_asm), info)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_first_iterates(first_iterates, case):
    d_ref = max(v[1] for v in first_iterates.values())
    worst = max(first_iterates, key=lambda key: first_iterates[key][1])
    print("d_ref", d_ref, "at", worst, "| largest device difference", max(v[0] for v in first_iterates.values()))
    assert np.isfinite(d_ref) and d_ref > 0.0
    for (cs, k), (err, ref, info) in first_iterates.items():
        if cs != case:
            continue
        print(case_id(case), "k", k, "device vs K_asm", err, "GPU operator and solve vs K_asm", ref, info)
        assert info.iterations == k and info.status == "running", info
        assert err <= 10.0 * d_ref, (case, k, err, d_ref)


# ---- 4. the solve ---------------------------------------------------------------------------------------------------------------------
def test_solve(cases):
    s = cases[G20]
    cap = 10 * s.n
    z_ref, info_ref, it_ref, res = scipy_solve(s.c, s.ref(s.N).operator(), cap)
    assert info_ref == 0
    rho = max(1.0, (res[-6] / res[-1]) ** 0.2)
    z, info = s.minres(factor(s), rtol=1e-10, max_iter=cap)
    print("scipy with the same M: iterations", it_ref, "residual", res[-1], "rho", rho, "| device:", info, "residual", s.res(z))
    assert info.status == "converged", info
    assert abs(info.iterations - it_ref) <= 2, (info.iterations, it_ref)
    assert s.res(z) <= rho * rho * res[-1], (s.res(z), res[-1], rho)
    # precond="schur_cr": built with the defaults (kkt_diag_precond's pair); "schur" stays the chunked one
    zs, infos = s.minres("schur_cr", rtol=1e-10, max_iter=cap)
    zc, infoc = s.minres("schur", rtol=1e-10, max_iter=cap)
    print("precond='schur_cr':", infos, "| precond='schur':", infoc)
    assert infos.status == "converged" and abs(infos.iterations - infoc.iterations) <= 2, (infos, infoc)


# ---- 5. the point of the feature -----------------------------------------------------------------------------------------------------
def test_small_sc_long_grid(torch_cuda):
    case = ("goddard", "trapeze", 300, False)
    s = Case(torch_cuda, case, small_sc_case(minres_case(*case[:3])))
    it = [0]
    count = lambda zk: it.__setitem__(0, it[0] + 1)      # noqa: E731
    _, info_ref = minres(s.c["K_asm"], s.c["rhs"], M=s.ref(s.N).operator(), rtol=1e-10, maxiter=10 * s.n, callback=count)
    it_dense, it[0] = it[0], 0
    _, info_diag = minres(s.c["K_asm"], s.c["rhs"], M=diag_op(s.px, s.pc), rtol=1e-10, maxiter=20 * s.n, callback=count)
    it_diag = it[0]
    assert info_ref == 0 and info_diag == 0
    P = factor(s)
    z, info = s.minres(P, rtol=1e-10, max_iter=10 * s.n)
    print("scipy, dense one-chunk M:", it_dense, "| scipy, diagonal M:", it_diag, "| device:", info, "residual", s.res(z))
    assert info.status == "converged", info
    assert abs(info.iterations - it_dense) <= 2, (info.iterations, it_dense)
    assert 10 * info.iterations <= it_diag, (info.iterations, it_diag)
    assert s.d.kkt_schur_cr_info(P) == -1


# ---- 6. exactness ----------------------------------------------------------------------------------------------------------------------
def test_exactness(torch_cuda, cases):
    torch = torch_cuda
    s = cases[G20]
    cap = 10 * s.n
    Pa, Pb = factor(s), factor(s)
    s.d.sync()
    assert same_factor(torch, Pa, Pb), "two factors of the same inputs"
    fac = factor_part(Pa)
    # two runs; check_every 1 and 7
    za, ia = s.minres(Pa, rtol=1e-10, max_iter=cap, check_every=1)
    zb, ib = s.minres(Pb, rtol=1e-10, max_iter=cap, check_every=1)
    z7, i7 = s.minres(Pb, rtol=1e-10, max_iter=cap, check_every=7)
    assert ia.status == "converged" and ia == ib == i7, (ia, ib, i7)
    assert torch.equal(za, zb) and torch.equal(za, z7)
    assert all(torch.equal(x, y) for x, y in zip(factor_part(Pa), fac)), "the solve leaves the factor part alone"
    assert same_factor(torch, Pa, Pb)
    # 20 iterations enqueued past convergence change nothing: not z, not the state, not one word of the Schur workspace
    before, ws_before = z7.clone(), Pb.ws.view(torch.int64).clone()
    s.d.kkt_minres_iters(s.x, s.y, z7, 20, sx=s.sx, sc=s.sc)
    assert s.d.kkt_minres_info() == i7
    assert torch.equal(z7, before) and torch.equal(Pb.ws.view(torch.int64), ws_before)
    # the plain solve twice: the same bits
    r, = dev(torch, np.random.default_rng(2).uniform(-1.0, 1.0, s.ncon))
    assert torch.equal(s.d.kkt_schur_cr_solve(Pa, r), s.d.kkt_schur_cr_solve(Pb, r))


def test_graph_capture(torch_cuda):
    torch = torch_cuda
    s = Case(torch, G20)
    d = s.d
    P = factor(s)
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
    z_eager, info_eager, ws_eager = z.cpu().numpy(), d.kkt_minres_info(), P.ws.view(torch.int64).clone()
    assert info_eager.iterations == 3
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        three()
    for _ in range(2):                  # a replay, and a replay after a replay
        z.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(z.cpu().numpy(), z_eager) and d.kkt_minres_info() == info_eager
        assert torch.equal(P.ws.view(torch.int64), ws_eager)


# ---- 7. breakdown ----------------------------------------------------------------------------------------------------------------------
def test_breakdown(torch_cuda, cases):
    s = cases[G7]
    col = 2 * s.d.discretization._step_variables_block          # the first state of step 2: w = -1e9 on its column
    px = s.pxd.clone()
    px[col] = -1e-9
    pxh = s.px.copy()
    pxh[col] = -1e-9
    F = SchurCrRef(schur_T(s.c, pxh, s.m, s.N, s.nv, s.N), s.N, s.m)
    P = factor(s, px=px)
    bad = s.d.kkt_schur_cr_info(P)
    status = P.ws.view(torch_cuda.int64)[FIXED:FIXED + s.N].cpu().numpy()
    print("first bad block", bad, "status words", status, "reference", F.status)
    # block 1 holds the column and is eliminated at level 0; its NaN reaches block 2 and, like every failure, the root
    assert status[1] >= 0 and ((status >= 0) == (F.status >= 0)).all()
    assert bad == F.info() == 0
    out = torch_cuda.full((s.ncon,), 7.0, dtype=torch_cuda.float64, device="cuda")
    s.d.kkt_schur_cr_solve(P, s.sc, out=out)
    assert bool(torch_cuda.isnan(out[:s.nb]).all()) and bool((out[s.nb:] == 7.0).all())
    z, info = s.minres(P, rtol=1e-10, max_iter=50)
    assert info.status == "breakdown", info
    assert not bool(z.any()) and bool(torch_cuda.isfinite(z).all())


# ---- 8. write sets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (0, 1))
def test_write_sets(torch_cuda, cases, shift):
    torch = torch_cuda
    s = cases[("goddard", "gauss_legendre_2", 7, False)]
    d = s.d
    lay = d.kkt_schur_cr_layout()
    nfac = FIXED + lay.N + 3 * lay.N * lay.block_rows ** 2          # the scratch of the solve begins here
    G = lambda n, like=None: guarded(torch, n, shift, "cuda", like)      # noqa: E731
    # the run on ordinary tensors
    P0 = factor(s)
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    out0 = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    d.kkt_schur_cr_solve(P0, r, out=out0)
    z0 = torch_empty(torch, s.n)
    d.kkt_minres_start(s.x, s.y, s.rhs, z0, sx=s.sx, sc=s.sc, precond=P0, rtol=0.0)
    d.kkt_minres_iters(s.x, s.y, z0, 1, sx=s.sx, sc=s.sc)
    d.sync()
    # ... and on guarded views
    ins = {nm: G(t.numel(), t).snapshot() for nm, t in (("jvals", s.jvals), ("px", s.pxd), ("pc", s.pcd), ("sc", s.sc), ("r", r), ("x", s.x),
                                                       ("y", s.y), ("sx", s.sx), ("rhs", s.rhs))}
    ws, out, z = G(lay.workspace), G(s.ncon, out0.new_full((s.ncon,), 7.0)), G(s.n)
    P = d.kkt_schur_cr_factor(ins["jvals"].view, ins["px"].view, ins["pc"].view, ins["sc"].view, ws.view)
    d.sync()
    assert ws.guards_intact("factor") and ws.unwritten() == [], "the factor writes the whole workspace"
    fac = ws.bits().clone()
    d.kkt_schur_cr_solve(P, ins["r"].view, out=out.view)
    assert out.guards_intact("solve") and ws.guards_intact("solve")
    assert torch.equal(ws.bits()[:nfac], fac[:nfac]), "the plain solve writes its scratch region only"
    assert torch.equal(out.bits(), out0.view(torch.int64))
    assert bool((out.view[s.nb:] == 7.0).all()), "the tail rows of out keep their fill"
    d.kkt_minres_start(ins["x"].view, ins["y"].view, ins["rhs"].view, z.view, sx=ins["sx"].view, sc=ins["sc"].view, precond=P, rtol=0.0)
    d.kkt_minres_iters(ins["x"].view, ins["y"].view, z.view, 1, sx=ins["sx"].view, sc=ins["sc"].view)
    d.sync()
    assert z.guards_intact("start + iteration") and ws.guards_intact("start + iteration")
    assert torch.equal(z.bits(), z0.view(torch.int64))
    # inside MINRES: the partial sums in the fixed part, the scratch, and nothing else of the workspace
    assert torch.equal(ws.bits()[FIXED:nfac], fac[FIXED:nfac]) and torch.equal(ws.bits()[:16], fac[:16])
    assert torch.equal(ws.bits()[16 + 256:FIXED], fac[16 + 256:FIXED])
    assert torch.equal(ws.bits(), P0.ws.view(torch.int64))
    for nm, g in ins.items():
        assert g.unchanged(nm)


# ---- 9. workspace mix-ups and device refusals ------------------------------------------------------------------------------------------
def test_mixups_and_refusals(torch_cuda, cases):
    torch = torch_cuda
    L, lib = ct._lib.lib(), ct._lib
    E = lib.CTD_EINVAL
    s = cases[G7]
    d = s.d
    P = factor(s)
    Pc = s.factor(3)                    # a chunked factor of the same handle
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

    fac = lambda h, jv, px, sc, ws: L.ctd_kkt_schur_cr_factor_dev_async(h, V(jv), V(px), V(sc), V(ws))        # noqa: E731
    solve = lambda h, ws, r, o: L.ctd_kkt_schur_cr_solve_dev_async(h, V(ws), V(r), V(o))        # noqa: E731
    start = lambda h, ks, ws, r, zz, rtol=1e-10: L.ctd_kkt_minres_schur_cr_start_dev_async(h, C.byref(ks), V(ws), V(r), V(zz), rtol)        # noqa: E731
    drive = lambda h, ks, ws, r, zz, rtol=1e-10, mi=10, ce=2: L.ctd_kkt_minres_schur_cr_dev(h, C.byref(ks), V(ws), V(r), V(zz), rtol, mi, ce, C.byref(info))        # noqa: E731
    # the other family's workspace: the solves store nothing, the status queries say so
    before_c, before = Pc.ws.clone(), P.ws.clone()
    assert solve(d._h, Pc.ws, s.sc, out) == 0
    assert L.ctd_kkt_schur_solve_dev_async(d._h, V(P.ws), V(s.sc), V(out)) == 0
    d.sync()
    assert bool((out == 7.0).all())
    assert torch.equal(Pc.ws.view(torch.int64), before_c.view(torch.int64)) and torch.equal(P.ws.view(torch.int64), before.view(torch.int64))
    assert L.ctd_kkt_schur_cr_info(d._h, V(Pc.ws), C.byref(bad)) == E
    refused(d, "ctd_kkt_schur_cr_info", b"no factor")
    assert L.ctd_kkt_schur_info(d._h, V(P.ws), C.byref(bad)) == E
    refused(d, "ctd_kkt_schur_info", b"no factor")
    blank = torch.zeros(P.layout.workspace, dtype=torch.float64, device="cuda")
    assert solve(d._h, blank, s.sc, out) == 0
    d.sync()
    assert bool((out == 7.0).all()) and not bool(blank.any())
    # NULL handle, struct sizes
    assert fac(None, s.jvals, s.pxd, s.sc, P.ws) == E and solve(None, P.ws, s.sc, out) == E
    assert start(None, system(), P.ws, s.rhs, z) == E and drive(None, system(), P.ws, s.rhs, z) == E
    for name, call in (("ctd_kkt_minres_schur_cr_start_dev_async", start), ("ctd_kkt_minres_schur_cr_dev", drive)):
        assert call(d._h, system(size=8), P.ws, s.rhs, z) == E
        refused(d, name, b"struct_size")
    # shard handles, CSC handles: before the pointers
    kw = dict(device=0, pattern="structural")
    shard = ct.DOCP("goddard", 7, "trapeze", steps=(0, 4), value_order="csr", **kw)
    csc = ct.DOCP("goddard", 7, "trapeze", **kw)
    for h, what in ((shard, b"no shard form"), (csc, b"CTD_ORDER_CSR")):
        assert fac(h._h, None, None, None, None) == E
        refused(h, "ctd_kkt_schur_cr_factor_dev_async", what)
        assert solve(h._h, None, None, None) == E
        refused(h, "ctd_kkt_schur_cr_solve_dev_async", what)
        assert L.ctd_kkt_schur_cr_info(h._h, None, None) == E
        refused(h, "ctd_kkt_schur_cr_info", what)
        assert start(h._h, system(x=None), None, None, None) == E
        refused(h, "ctd_kkt_minres_schur_cr_start_dev_async", what)
        assert drive(h._h, system(x=None), None, None, None) == E
        refused(h, "ctd_kkt_minres_schur_cr_dev", what)
    # null pointers
    for jv, px, ws in ((None, s.pxd, P.ws), (s.jvals, None, P.ws), (s.jvals, s.pxd, None)):
        assert fac(d._h, jv, px, s.sc, ws) == E
        refused(d, "ctd_kkt_schur_cr_factor_dev_async", b"null")
    for ws, r, o in ((None, s.sc, out), (P.ws, None, out), (P.ws, s.sc, None)):
        assert solve(d._h, ws, r, o) == E
        refused(d, "ctd_kkt_schur_cr_solve_dev_async", b"null")
    assert L.ctd_kkt_schur_cr_info(d._h, None, C.byref(bad)) == E and L.ctd_kkt_schur_cr_info(d._h, V(P.ws), None) == E
    refused(d, "ctd_kkt_schur_cr_info", b"null")
    for name, call in (("ctd_kkt_minres_schur_cr_start_dev_async", start), ("ctd_kkt_minres_schur_cr_dev", drive)):
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
    assert fac(d._h, s.jvals, s.pxd, s.sc, s.pxd) == E
    refused(d, "ctd_kkt_schur_cr_factor_dev_async", b"input")
    assert solve(d._h, P.ws, s.sc, s.sc) == E
    refused(d, "ctd_kkt_schur_cr_solve_dev_async", b"input")
    # the refused calls left the factor usable
    assert torch.equal(P.ws.view(torch.int64), before.view(torch.int64))
    assert L.ctd_kkt_schur_cr_info(d._h, V(P.ws), C.byref(bad)) == 0 and bad.value == -1
    # the first factor on a handle inside a capture
    fresh = ct.DOCP("goddard", 7, "trapeze", value_order="csr", **kw)
    ws = torch_empty(torch, P.layout.workspace)
    side = torch.cuda.Stream()
    fresh.set_stream(side)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ws.zero_()                      # (so that the capture is not empty)
        st = fac(fresh._h, s.jvals, s.pxd, s.sc, ws)
    assert st == E and b"capturing" in L.ctd_last_error(fresh._h)
