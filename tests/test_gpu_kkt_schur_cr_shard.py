"""The shard form of the log-depth Schur preconditioner on the MI355X (ctd_kkt_schur_cr_shard_*, ctd_kkt_minres_schur_cr_shard_*;
DOCP.kkt_schur_cr_shard_factor / _solve / _info, the kkt_minres_schur_shard_* phases, dist.kkt_minres_shards with one
SchurCrShardPrecond per shard).  Shards are handles of one process on device 0, as in tests/test_gpu_kkt_minres_shard.py.

The reference throughout is the dense cut matrix of tests/schur_shard_ref.py on K_asm's own blocks (SchurCutRef); the inputs are
those of tests/test_gpu_kkt_schur_cr.py: minres_case, asm_precond's (px, pc), the whole-grid handle's own cons_jac values.

BARS (those of tests/test_gpu_kkt_schur_cr.py, with the dense cut matrix as the reference)
  factor + solve   per rank, eta = |T_r y - r|_inf / (|T_r|_inf |y|_inf + |r|_inf) <= max(10 eta_ref, 64 eps), eta_ref that of
                   scipy.linalg.cho_solve on the same T_r and r; info gives -1.
  symmetry         |u . (M v) - (M u) . v| <= 1e-13 max(|u . (M v)|, |(M u) . v|) and <= 1e-13 |M^-1|_inf |M u| |M v|.
  first iterates   |z_k - z_k(scipy on K_asm with the dense cut M)| / |...| <= 10 d_ref, k in {1, 2, 5}; d_ref the same distance for
                   scipy driven by the GPU kktprod and the GPU shard solves, the maximum over the cases of the same run.
  the solves       N = 20, three shards: converged, iterations within +-2 of scipy's with the same M.  Goddard trapeze N = 300 with
                   sc = 1e-8 U(1, 2), three shards: converged, iterations within +-2 of scipy's with the dense cut M and at most a
                   tenth of scipy's with the diagonal M (7151: pinned by tests/test_kkt_schur_cr_shard_cpu.py).
Everything else is exact: bit equality, statuses, refusals, read and write sets."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import dist as cdist
from guarded import guarded
from jit_defs import twin
from schur_ref import small_sc_case
from schur_shard_ref import SchurCutRef, cross_rank_sum, shard_cuts, solve_partial_sums
from test_gpu_kkt_minres import asm_precond, dev, minres_case, rel
from test_kkt_schur_cr_shard_cpu import COUNTS, wide_ocp

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KS = (1, 2, 5)
FIXED = 512
# a slot of the Schur form (csrc/ctd_krylov_shard_kernels.hpp): the count of the phase's own partial sums, the solve's partial sums,
# their count
SLOT_COUNT, SLOT_SCHUR, SLOT_SCHUR_COUNT = 2064, 2080, 2080 + 256
# 1. one shard: (problem, scheme, N)
ONE = [("goddard", "trapeze", N) for N in (1, 2, 7, 20)] + [("goddard", "gauss_legendre_2", 7)]
# 2. factor + solve per rank: (problem, scheme, N, cuts, run-time twin) -- the smallest shapes at which the level logic can go wrong
RANKS = [("goddard", "trapeze", 7, (0, 3, 5, 7), False),                # levels 2 and 1, with and without a right neighbour
         ("goddard", "trapeze", 5, (0, 1, 2, 3, 4, 5), False),          # five ranks of one block: no level, the root only
         ("goddard", "trapeze", 20, (0, 7, 14, 20), False),
         ("goddard", "trapeze", 33, (0, 17, 33), False),
         ("goddard", "trapeze", 20, (0, 1, 8, 20), False),              # explicit uneven cuts
         ("goddard", "gauss_legendre_2", 7, (0, 4, 7), False),          # m = 9
         ("double_integrator_path", "midpoint", 7, (0, 3, 5, 7), False),
         ("goddard", "midpoint", 7, (0, 3, 5, 7), True),
         ("quadrotor12", "gauss_legendre_3", 5, (0, 3, 5), False)]      # m = 49
G7 = RANKS[0]
G20 = RANKS[2]
THREE = [G7, G20, RANKS[6]]
case_id = lambda c: f"{c[0]}-{c[1]}-N{c[2]}-" + "_".join(map(str, c[3])) + ("-rt" if c[4] else "")      # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class Case:
    """one transcription cut into shards: CSR shard handles beside a CSR handle of the whole grid, the inputs of minres_case and
    asm_precond's (px, pc) on the device, the whole-grid handle's Jacobian values, the dense cut reference"""

    def __init__(self, torch, case, c=None):
        prob, sch, N, cuts, rt = case
        self.torch, self.c, self.cuts, self.G = torch, c or minres_case(prob, sch, N), list(cuts), len(cuts) - 1
        c = self.c
        self.nvar, self.ncon, self.n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
        kw = dict(device=0, pattern="structural", value_order="csr")
        name = twin(prob) if rt else prob
        self.full = ct.DOCP(name, N, sch, **kw)
        assert (self.full.dim_NLP_variables, self.full.dim_NLP_constraints) == (self.nvar, self.ncon)
        self.hs = [self.full] if self.G == 1 else [ct.DOCP(name, N, sch, steps=(cuts[k], cuts[k + 1]), **kw) for k in range(self.G)]
        lay = self.full.kkt_schur_cr_layout()
        self.m, self.N, self.nv, self.nb = lay.block_rows, lay.N, lay.tail_cols, lay.first_tail_row
        self.px, self.pc = asm_precond(c)
        assert (self.px > 0).all() and (self.pc > 0).all()
        self.x, self.y, self.sx, self.sc, self.rhs, self.pxd, self.pcd = dev(torch, c["x"], c["y"], c["sx"], c["sc"], c["rhs"], self.px, self.pc)
        self.jvals = self.full.cons_jac(self.x)[1]
        self.lays = [h.kkt_minres_schur_shard_layout(self.G) for h in self.hs]
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = SchurCutRef(self.c, self.px, self.pc, self.m, self.N, self.nv, self.cuts)
        return self._ref

    def rows(self, k):
        return slice(self.cuts[k] * self.m, self.cuts[k + 1] * self.m)

    def factors(self, px=None, jvals=None, sc=None):
        per = lambda a, k: a[k] if isinstance(a, list) else a      # noqa: E731
        return [h.kkt_schur_cr_shard_factor(per(self.jvals if jvals is None else jvals, k), per(self.pxd if px is None else px, k), self.pcd,
                                            per(self.sc if sc is None else sc, k)) for k, h in enumerate(self.hs)]

    def shards(self, Ps, **kw):
        return cdist.kkt_minres_shards(self.hs, [self.x] * self.G, self.y, self.rhs, sx=self.sx, sc=self.sc, precond=list(Ps), **kw)

    def phases(self, Ps, **kw):
        return cdist.minres_shards(self.hs, [self.x] * self.G, self.y, self.rhs, sx=self.sx, sc=self.sc, precond=list(Ps), **kw)

    def apply_M(self, Ps, v):
        """M v on the device: variables / px, every rank's block rows through its own solve, the tail rows / pc"""
        out = self.torch.empty(self.n, dtype=self.torch.float64, device="cuda")
        out[:self.nvar] = v[:self.nvar] / self.pxd
        out[self.nvar + self.nb:] = v[self.nvar + self.nb:] / self.pcd[self.nb:]
        r = v[self.nvar:].contiguous()
        for h, P in zip(self.hs, Ps):
            h.kkt_schur_cr_shard_solve(P, r, out=out[self.nvar:])
        return out

    def own_mask(self, k):
        lay, m = self.lays[k], np.zeros(self.n, dtype=bool)
        for a, b in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            m[a:b] = True
        return m

    def compose(self, zs):
        z, seen = np.full(self.n, 777.0), np.zeros(self.n, dtype=int)
        for k, zk in enumerate(zs):
            m = self.own_mask(k)
            z[m] = zk.cpu().numpy()[m]
            seen += m
        lay = self.lays[0]
        tail = np.zeros(self.n, dtype=bool)
        tail[lay.tail_begin:lay.tail_end] = True
        assert (seen[~tail] == 1).all() and (seen[tail] == len(zs)).all()
        return z

    def same(self, za, zb):
        masks = [self.torch.from_numpy(self.own_mask(k)).cuda() for k in range(self.G)]
        return all(self.torch.equal(a[m], b[m]) for a, b, m in zip(za, zb, masks))

    def res(self, z):
        return float(np.linalg.norm(self.c["K_asm"] @ z - self.c["rhs"]) / np.linalg.norm(self.c["rhs"]))

    def close(self):
        for h in {id(h): h for h in [self.full] + self.hs}.values():
            h.close()


@pytest.fixture(scope="module")
def cases(torch_cuda):
    made = {}

    def get(case):
        if case not in made:
            made[case] = Case(torch_cuda, case)
        return made[case]

    yield get
    for s in made.values():
        s.close()


def factor_part(P):
    """the bits of the workspace that the factor owns: the header, the status words, the blocks"""
    import torch
    lay = P.layout
    w = P.ws.view(torch.int64)
    return w[:16].clone(), w[FIXED:FIXED + lay.n_blocks + 3 * lay.n_blocks * lay.block_rows ** 2].clone()


def state_bytes(torch, w):
    return w.ws[w.layout.off_state:w.layout.off_state + 16].view(torch.int64).cpu().numpy().copy()


def backward_error(T, y, r):
    return float(np.abs(T @ y - r).max() / (np.abs(T).sum(axis=1).max() * np.abs(y).max() + np.abs(r).max()))


# ---- 1. one shard is the whole grid --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch,N", ONE, ids=[f"{p}-{s}-N{N}" for p, s, N in ONE])
def test_one_shard_is_the_whole_grid(torch_cuda, prob, sch, N):
    torch = torch_cuda
    s = Case(torch, (prob, sch, N, (0, N), False))
    d = s.full
    lay = d.kkt_schur_cr_layout()
    Pw = d.kkt_schur_cr_factor(s.jvals, s.pxd, s.pcd, s.sc, torch.empty(lay.workspace, dtype=torch.float64, device="cuda"))
    Ps, = s.factors()
    d.sync()
    assert Ps.layout.workspace == lay.workspace and (Ps.layout.step_begin, Ps.layout.n_blocks) == (0, N)
    fw = (Pw.ws.view(torch.int64)[:16], Pw.ws.view(torch.int64)[FIXED:FIXED + N + 3 * N * s.m ** 2])
    assert all(torch.equal(a, b) for a, b in zip(factor_part(Ps), fw)), "the factor part: not the bits of ctd_kkt_schur_cr_factor_dev_async"
    assert d.kkt_schur_cr_shard_info(Ps) == d.kkt_schur_cr_info(Pw) == -1
    r, = dev(torch, np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon))
    ow = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    os_ = ow.clone()
    d.kkt_schur_cr_solve(Pw, r, out=ow)
    d.kkt_schur_cr_shard_solve(Ps, r, out=os_)
    assert torch.equal(ow, os_), "out: not the bits of ctd_kkt_schur_cr_solve_dev_async"
    # the whole-grid solve accepts the single shard's workspace and the other way round: the same header
    assert torch.equal(d.kkt_schur_cr_solve(Ps, r), d.kkt_schur_cr_shard_solve(Pw, r))
    for kw in [dict(rtol=0.0, max_iter=k) for k in KS] + [dict(rtol=1e-10, max_iter=10 * s.n)]:
        zw, iw = d.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=Pw, **kw)
        (z,), (info,) = s.shards([Ps], **kw)
        assert info == iw, (kw, info, iw)
        assert torch.equal(z, zw), (kw, "z: not the bits of ctd_kkt_minres_schur_cr_dev")
        assert iw.status != "running" and (kw["rtol"] or iw.iterations == kw["max_iter"]), iw
    s.close()


# ---- 2. factor + solve per rank against the dense T_r ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RANKS, ids=case_id)
def test_factor_solve_per_rank(torch_cuda, cases, case):
    torch = torch_cuda
    s = cases(case)
    r = np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon)
    rd, = dev(torch, r)
    keep = rd.clone()
    Ps = s.factors()
    for k, (h, P) in enumerate(zip(s.hs, Ps)):
        n_r = s.cuts[k + 1] - s.cuts[k]
        lay = P.layout
        assert (lay.step_begin, lay.n_blocks, lay.n_levels) == (s.cuts[k], n_r, (n_r - 1).bit_length())
        assert lay.solve_launches == 2 * lay.n_levels + 1 and lay.factor_launches == 2 * lay.n_levels + 2
        assert h.kkt_schur_cr_shard_info(P) == -1
        out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
        h.kkt_schur_cr_shard_solve(P, rd, out=out)
        y = out.cpu().numpy()
        rows = s.rows(k)
        mask = np.ones(s.ncon, dtype=bool)
        mask[rows] = False
        assert (y[mask] == 7.0).all(), (k, "out is written on the rank's block rows only")
        assert torch.equal(rd, keep), "r is not modified"
        T = s.ref.T_r(k)
        y_ref = s.ref.solve_rank(k, r[:s.nb])
        eta, eta_ref = backward_error(T, y[rows], r[rows]), backward_error(T, y_ref, r[rows])
        print(case_id(case), "rank", k, "blocks", n_r, "m", s.m, "levels", lay.n_levels, "eta", eta, "eta_ref (cho_solve)", eta_ref,
              "forward difference", rel(y[rows], y_ref))
        assert eta <= max(10.0 * eta_ref, 64.0 * EPS), (case, k, eta, eta_ref)


# ---- 3. read sets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [G7, RANKS[5]], ids=case_id)
def test_read_sets(torch_cuda, cases, case):
    """NaN everywhere outside the documented read set of jvals, px, sc and r: the factor part and out keep their bits"""
    torch = torch_cuda
    s = cases(case)
    nan = float("nan")
    r, = dev(torch, np.random.default_rng(6).uniform(-1.0, 1.0, s.ncon))
    want = s.factors()
    for k, (h, P0) in enumerate(zip(s.hs, want)):
        lay = P0.layout
        rows = s.rows(k)
        jv, px, sc, rr = (torch.full_like(a, nan) for a in (s.jvals, s.pxd, s.sc, r))
        jv[lay.jvals_begin:lay.jvals_end] = s.jvals[lay.jvals_begin:lay.jvals_end]
        px[lay.px_begin:lay.px_end] = s.pxd[lay.px_begin:lay.px_end]
        sc[rows] = s.sc[rows]
        rr[rows] = r[rows]
        assert lay.px_end <= s.nvar - s.nv and lay.jvals_end - lay.jvals_begin < s.jvals.numel()
        P = h.kkt_schur_cr_shard_factor(jv, px, s.pcd, sc)
        assert h.kkt_schur_cr_shard_info(P) == -1
        assert all(torch.equal(a, b) for a, b in zip(factor_part(P), factor_part(P0))), (k, "the factor read outside its read set")
        out0 = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
        out = out0.clone()
        h.kkt_schur_cr_shard_solve(P0, r, out=out0)
        h.kkt_schur_cr_shard_solve(P, rr, out=out)
        assert torch.equal(out, out0), (k, "the solve read r outside the rank's block rows")


# ---- 4. write sets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (0, 1))
def test_write_sets(torch_cuda, cases, shift):
    torch = torch_cuda
    s = cases(G7)
    Gd = lambda n, like=None: guarded(torch, n, shift, "cuda", like)      # noqa: E731
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    # the run on ordinary tensors
    P0 = s.factors()
    out0 = [torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda") for _ in s.hs]
    for h, P, o in zip(s.hs, P0, out0):
        h.kkt_schur_cr_shard_solve(P, r, out=o)
    z0, i0 = s.shards(P0, rtol=0.0, max_iter=2)
    z0 = [z.clone() for z in z0]
    # ... and on guarded views
    ins = {nm: Gd(t.numel(), t).snapshot() for nm, t in (("jvals", s.jvals), ("px", s.pxd), ("pc", s.pcd), ("sc", s.sc), ("r", r), ("x", s.x),
                                                       ("y", s.y), ("sx", s.sx), ("rhs", s.rhs))}
    gws = [Gd(P.layout.workspace) for P in P0]
    Ps = [h.kkt_schur_cr_shard_factor(ins["jvals"].view, ins["px"].view, ins["pc"].view, ins["sc"].view, g.view) for h, g in zip(s.hs, gws)]
    for h in s.hs:
        h.sync()
    fac = []
    for k, (g, P) in enumerate(zip(gws, Ps)):
        assert g.guards_intact(f"factor of rank {k}") and g.unwritten() == [], "the factor writes the whole workspace"
        assert all(torch.equal(a, b) for a, b in zip(factor_part(P), factor_part(P0[k])))
        fac.append(g.bits().clone())
    for k, (h, P, g) in enumerate(zip(s.hs, Ps, gws)):
        out = Gd(s.ncon)
        h.kkt_schur_cr_shard_solve(P, ins["r"].view, out=out.view)
        rows = s.rows(k)
        assert out.guards_intact(f"solve of rank {k}") and g.guards_intact(f"solve of rank {k}")
        assert out.unwritten() == [i for i in range(s.ncon) if not rows.start <= i < rows.stop], (k, "out is written on the rank's block rows only")
        assert torch.equal(out.bits()[rows], out0[k].view(torch.int64)[rows])
        nfac = FIXED + P.layout.n_blocks + 3 * P.layout.n_blocks * s.m ** 2
        assert torch.equal(g.bits()[:nfac], fac[k][:nfac]), "the plain solve writes its scratch region only"
    # the solve: z and the Krylov vectors on owned entries only
    gz = [Gd(s.n) for _ in s.hs]
    gw = [Gd(lay.workspace) for lay in s.lays]
    ws = [h.kkt_minres_schur_shard_workspace(s.G, ws=g.view) for h, g in zip(s.hs, gw)]
    zs, infos = cdist.kkt_minres_shards(s.hs, [ins["x"].view] * s.G, ins["y"].view, ins["rhs"].view, sx=ins["sx"].view, sc=ins["sc"].view,
                                        precond=Ps, rtol=0.0, max_iter=2, out=[g.view for g in gz], workspaces=ws)
    assert infos == i0
    for k in range(s.G):
        assert gz[k].guards_intact(f"z of rank {k}") and gw[k].guards_intact(f"workspace of rank {k}") and gws[k].guards_intact(f"factor of rank {k}")
        m = s.own_mask(k)
        assert gz[k].unwritten() == np.nonzero(~m)[0].tolist(), (k, "z is written on owned entries only")
        assert torch.equal(zs[k][torch.from_numpy(m).cuda()], z0[k][torch.from_numpy(m).cuda()]), (k, "not the bits of the run on ordinary tensors")
        untouched = torch.from_numpy(np.array(gw[k].unwritten(), dtype=np.int64))
        for j in (0, 1, 2, 5, 6, 7):           # r1, r2, y, w, w2, minv: owned entries only (v and kv also receive halos / K v)
            inside = untouched[(untouched >= j * s.n) & (untouched < (j + 1) * s.n)] - j * s.n
            assert inside.tolist() == np.nonzero(~m)[0].tolist(), (k, j, "a workspace vector written outside the owned entries")
        nfac = FIXED + Ps[k].layout.n_blocks + 3 * Ps[k].layout.n_blocks * s.m ** 2
        assert torch.equal(gws[k].bits()[:nfac], fac[k][:nfac]), "inside MINRES the factor part is only read"
    for nm, g in ins.items():
        assert g.unchanged(nm)


# ---- 5. symmetry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", THREE, ids=case_id)
def test_symmetry(torch_cuda, cases, case):
    s = cases(case)
    g = np.random.default_rng(9)
    u, v = dev(torch_cuda, g.uniform(-1.0, 1.0, s.n), g.uniform(-1.0, 1.0, s.n))
    Ps = s.factors()
    Mu, Mv = s.apply_M(Ps, u), s.apply_M(Ps, v)
    a, b = float(u @ Mv), float(Mu @ v)
    norm_minv = max(float(s.px.max()), float(np.abs(s.ref.T).sum(axis=1).max()), float(s.pc[s.nb:].max()) if s.nb < s.ncon else 0.0)
    scale = norm_minv * float(Mu.norm()) * float(Mv.norm())
    print(case_id(case), "u.Mv", a, "Mu.v", b, "difference / scale", abs(a - b) / scale, "difference / |u.Mv|", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b)), (case, a, b)
    assert abs(a - b) <= 1e-13 * scale, (case, a, b, scale)


# ---- 6. first iterates -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_iterates(torch_cuda, cases):
    """per case and k: (|z_dev - z_asm| / |z_asm|, |z_op - z_asm| / |z_asm|, the ranks' infos)"""
    torch = torch_cuda
    out = {}
    for case in THREE:
        s = cases(case)
        c, d, nvar, n = s.c, s.full, s.nvar, s.n
        zin, zout, rc, yc = (torch.empty(k, dtype=torch.float64, device="cuda") for k in (n, n, s.ncon, s.ncon))

        def matvec(v):
            zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
            d.kktprod(s.x, s.y, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=s.sx, sc=s.sc, out=(zout[:nvar], zout[nvar:]))
            return zout.cpu().numpy()

        K_op = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
        Ps = s.factors()
        M_ref = s.ref.operator()

        def gpu_M(v):
            v = np.asarray(v, dtype=np.float64).ravel()
            rc.copy_(torch.from_numpy(np.ascontiguousarray(v[nvar:])))
            for h, P in zip(s.hs, Ps):
                h.kkt_schur_cr_shard_solve(P, rc, out=yc)
            return np.r_[v[:nvar] / s.px, yc[:s.nb].cpu().numpy(), v[nvar + s.nb:] / s.pc[s.nb:]]

        M_op = LinearOperator((n, n), matvec=gpu_M, dtype=np.float64)
        for k in KS:
            z_asm, _ = minres(c["K_asm"], c["rhs"], M=M_ref, rtol=0.0, maxiter=k)
            z_op, _ = minres(K_op, c["rhs"], M=M_op, rtol=0.0, maxiter=k)
            zs, infos = s.shards(Ps, rtol=0.0, max_iter=k)
            out[(case, k)] = (rel(s.compose(zs), z_asm), rel(z_op, z_asm), infos)
    return out


@pytest.mark.parametrize("case", THREE, ids=case_id)
def test_first_iterates(first_iterates, case):
    d_ref = max(v[1] for v in first_iterates.values())
    worst = max(first_iterates, key=lambda key: first_iterates[key][1])
    print("d_ref", d_ref, "at", worst, "| largest device difference", max(v[0] for v in first_iterates.values()))
    assert np.isfinite(d_ref) and d_ref > 0.0
    for (cs, k), (err, ref, infos) in first_iterates.items():
        if cs != case:
            continue
        print(case_id(case), "k", k, "three shards vs K_asm", err, "GPU operator and solves vs K_asm", ref, infos[0])
        assert all(i == infos[0] for i in infos), infos
        assert infos[0].iterations == k and infos[0].status == "max_iter", infos[0]
        assert err <= 10.0 * d_ref, (case, k, err, d_ref)


# ---- 7. the solves -----------------------------------------------------------------------------------------------------------------------
def count_iterations(c, M, cap):
    it = [0]
    _, info = minres(c["K_asm"], c["rhs"], M=M, rtol=1e-10, maxiter=cap, callback=lambda zk: it.__setitem__(0, it[0] + 1))
    assert info == 0
    return it[0]


def test_solve_three_shards(cases):
    s = cases(G20)
    assert s.cuts == shard_cuts(20, 3)
    cap = 10 * s.n
    it_ref = count_iterations(s.c, s.ref.operator(), cap)
    assert it_ref == COUNTS[("goddard", "trapeze", 20, False)][3]
    zs, infos = s.shards(s.factors(), rtol=1e-10, max_iter=cap)
    z = s.compose(zs)
    print("scipy with the dense cut M: iterations", it_ref, "| three shards:", infos[0], "residual", s.res(z))
    assert all(i == infos[0] for i in infos) and infos[0].status == "converged", infos
    assert abs(infos[0].iterations - it_ref) <= 2, (infos[0].iterations, it_ref)


def test_small_sc_long_grid_three_shards(torch_cuda):
    key = ("goddard", "trapeze", 300, True)
    s = Case(torch_cuda, ("goddard", "trapeze", 300, tuple(shard_cuts(300, 3)), False), small_sc_case(minres_case("goddard", "trapeze", 300)))
    it_dense = count_iterations(s.c, s.ref.operator(), 10 * s.n)
    it_diag = COUNTS[key]["diag"]                   # scipy with the diagonal M: pinned on the CPU by tests/test_kkt_schur_cr_shard_cpu.py
    assert it_dense == COUNTS[key][3]
    Ps = s.factors()
    zs, infos = s.shards(Ps, rtol=1e-10, max_iter=10 * s.n)
    print("scipy, dense cut M:", it_dense, "| scipy, diagonal M:", it_diag, "| three shards:", infos[0], "residual", s.res(s.compose(zs)))
    assert all(i == infos[0] for i in infos) and infos[0].status == "converged", infos
    assert abs(infos[0].iterations - it_dense) <= 2, (infos[0].iterations, it_dense)
    assert 10 * infos[0].iterations <= it_diag, (infos[0].iterations, it_diag)
    assert [h.kkt_schur_cr_shard_info(P) for h, P in zip(s.hs, Ps)] == [-1, -1, -1]
    s.close()


# ---- 8. state and reproducibility ----------------------------------------------------------------------------------------------------
def test_state_and_reproducibility(torch_cuda, cases):
    torch, s = torch_cuda, cases(G20)
    cap = 10 * s.n
    Ps = s.factors()
    runs = {}
    for ce in (1, 7, 1):
        chunks = [0]
        keep = []

        def on_chunk(ph, infos):
            chunks[0] += 1
            keep.append(ph)
            st = [state_bytes(torch, r.w) for r in ph.ranks]
            assert all(np.array_equal(b, st[0]) for b in st), (ce, chunks[0], "the ranks' KrylovState bytes differ")
            assert all(i == infos[0] for i in infos)

        zs, infos = s.shards(Ps, rtol=1e-10, max_iter=cap, check_every=ce, on_chunk=on_chunk)
        assert infos[0].status == "converged" and chunks[0] == -(-infos[0].iterations // ce), (ce, infos[0], chunks[0])
        if ce in runs:                  # the second run with check_every = 1: reproducible across runs
            assert runs[ce][1] == infos and s.same(runs[ce][0], zs)
        runs[ce] = ([z.clone() for z in zs], infos, keep[-1])
    assert runs[7][1] == runs[1][1] and s.same(runs[7][0], runs[1][0]), "the result depends on check_every"
    # iterations enqueued after convergence change no bit: not z, not the state, not a word of a factor's workspace
    zs, infos, ph = runs[7]
    before = [state_bytes(torch, r.w) for r in ph.ranks]
    fac = [P.ws.view(torch.int64).clone() for P in Ps]
    ph.iterate(9)
    assert ph.infos() == infos
    for r, z0, b0, P, f0 in zip(ph.ranks, zs, before, Ps, fac):
        assert torch.equal(r.z, z0) and np.array_equal(state_bytes(torch, r.w), b0), r.rank
        assert torch.equal(P.ws.view(torch.int64), f0), r.rank


def test_graph_capture_of_a_chunk(torch_cuda):
    torch = torch_cuda
    s = Case(torch, G20)
    Ps = s.factors()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ph = s.phases(Ps)
        ph.start(0.0, 1000)
        ph.iterate(3)                   # the warm solve
    side.synchronize()
    z_eager, info_eager = [r.z.clone() for r in ph.ranks], ph.infos()
    assert info_eager[0].iterations == 3 and all(i == info_eager[0] for i in info_eager)
    with torch.cuda.stream(side):
        ph.start(0.0, 1000)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ph.iterate(3)
    g.replay()
    torch.cuda.synchronize()
    assert ph.infos() == info_eager and s.same([r.z for r in ph.ranks], z_eager)
    for h in s.hs + [s.full]:
        h.set_stream(torch.cuda.current_stream())
    s.close()


# ---- 9. breakdown ------------------------------------------------------------------------------------------------------------------------
def test_breakdown_on_every_rank(torch_cuda, cases):
    """a negative entry of px on a column that only the middle rank's factor reads (the first state of the step behind its first
    one): that rank's T_r fails a pivot, the others do not; the NaN of its partial sums reaches beta1^2 on every rank"""
    torch, s = torch_cuda, cases(G20)
    blk = s.full.discretization._step_variables_block
    col = (s.cuts[1] + 2) * blk
    lays = [h.kkt_schur_cr_shard_layout() for h in s.hs]
    assert lays[1].px_begin <= col < lays[1].px_end and not lays[0].px_begin <= col < lays[0].px_end and not lays[2].px_begin <= col < lays[2].px_end
    px = s.pxd.clone()
    px[col] = -1e-9
    Ps = [h.kkt_schur_cr_shard_factor(s.jvals, px if k == 1 else s.pxd, s.pcd, s.sc) for k, h in enumerate(s.hs)]
    bad = [h.kkt_schur_cr_shard_info(P) for h, P in zip(s.hs, Ps)]
    print("first bad block per rank", bad)
    assert bad[0] == -1 and bad[2] == -1 and s.cuts[1] <= bad[1] < s.cuts[2], bad
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    s.hs[1].kkt_schur_cr_shard_solve(Ps[1], s.sc, out=out)
    rows = s.rows(1)
    assert bool(torch.isnan(out[rows]).all()) and bool((out[:rows.start] == 7.0).all()) and bool((out[rows.stop:] == 7.0).all())
    chunks = [0]
    zs, infos = s.shards(Ps, rtol=1e-10, max_iter=50, check_every=4, on_chunk=lambda ph, i: chunks.__setitem__(0, chunks[0] + 1))
    assert all(i == infos[0] for i in infos) and infos[0].status == "breakdown" and infos[0].iterations == 0, infos
    assert chunks[0] == 1, "every rank ends after the same chunk"
    for k, z in enumerate(zs):
        m = torch.from_numpy(s.own_mask(k)).cuda()
        assert not bool(z[m].any()) and bool(torch.isfinite(z[m]).all()), (k, "z = 0")


# ---- 10. refusals and mix-ups ------------------------------------------------------------------------------------------------------------
def test_refusals_and_mixups(torch_cuda, cases):
    torch, s = torch_cuda, cases(G20)
    L, lib = ct._lib.lib(), ct._lib
    E = lib.CTD_EINVAL
    h, k = s.hs[1], 1
    Ps = s.factors()
    P = Ps[1]
    w = h.kkt_minres_schur_shard_workspace(3)
    z = torch.full((s.n,), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    V = lambda a, off=0: None if a is None else C.c_void_p(a.data_ptr() + off)        # noqa: E731
    ks = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, px=s.pxd.data_ptr(), pc=s.pcd.data_ptr())
    bad = C.c_int64(0)

    def refused(name, what, hh=h):
        err = L.ctd_last_error(hh._h)
        assert err.startswith(name.encode() + b": ") and what in err, (name, what, err)
        hh.sync()
        assert bool((z == 7.0).all()) and bool((out == 7.0).all()) and not bool(w.ws.any()), name

    fac = lambda hh, jv, px, sc, ws: L.ctd_kkt_schur_cr_shard_factor_dev_async(hh._h, V(jv), V(px), V(sc), V(ws))        # noqa: E731
    solve = lambda hh, ws, r, o: L.ctd_kkt_schur_cr_shard_solve_dev_async(hh._h, V(ws), V(r), V(o))        # noqa: E731
    start = lambda hh=h, sy=ks, sw=V(P.ws), r=V(s.rhs), zz=V(z), ww=V(w.ws), G=3, rk=1, rtol=1e-10, mi=10: \
        L.ctd_kkt_minres_schur_cr_shard_start_dev_async(hh._h, C.byref(sy), sw, r, zz, ww, G, rk, rtol, mi)        # noqa: E731
    lanczos = lambda sw=V(P.ws), zz=V(z), ww=V(w.ws), G=3, rk=1: L.ctd_kkt_minres_schur_cr_shard_lanczos_dev_async(h._h, sw, zz, ww, G, rk)        # noqa: E731
    phases = {p: getattr(L, f"ctd_kkt_minres_schur_cr_shard_{p}_dev_async") for p in ("alfa", "update")}
    pre = "ctd_kkt_minres_schur_cr_shard_"
    # CSC handles: before the pointers
    csc = ct.DOCP("goddard", 20, "trapeze", device=0, pattern="structural", steps=(7, 14))
    assert fac(csc, None, None, None, None) == E
    refused("ctd_kkt_schur_cr_shard_factor_dev_async", b"CTD_ORDER_CSR", csc)
    assert solve(csc, None, None, None) == E
    refused("ctd_kkt_schur_cr_shard_solve_dev_async", b"CTD_ORDER_CSR", csc)
    assert L.ctd_kkt_schur_cr_shard_info(csc._h, None, None) == E
    refused("ctd_kkt_schur_cr_shard_info", b"CTD_ORDER_CSR", csc)
    assert start(hh=csc) == E
    refused(pre + "start_dev_async", b"CTD_ORDER_CSR", csc)
    csc.close()
    # null pointers, aliasing
    for jv, px, ws in ((None, s.pxd, P.ws), (s.jvals, None, P.ws), (s.jvals, s.pxd, None)):
        assert fac(h, jv, px, s.sc, ws) == E
        refused("ctd_kkt_schur_cr_shard_factor_dev_async", b"null")
    for ws, r, o in ((None, s.sc, out), (P.ws, None, out), (P.ws, s.sc, None)):
        assert solve(h, ws, r, o) == E
        refused("ctd_kkt_schur_cr_shard_solve_dev_async", b"null")
    assert L.ctd_kkt_schur_cr_shard_info(h._h, None, C.byref(bad)) == E and L.ctd_kkt_schur_cr_shard_info(h._h, V(P.ws), None) == E
    refused("ctd_kkt_schur_cr_shard_info", b"null")
    assert fac(h, s.jvals, s.pxd, s.sc, s.pxd) == E
    refused("ctd_kkt_schur_cr_shard_factor_dev_async", b"input")
    assert solve(h, P.ws, s.sc, s.sc) == E
    refused("ctd_kkt_schur_cr_shard_solve_dev_async", b"input")
    # n_ranks / rank that do not fit the handle
    for G, rk, what in ((0, 0, b"n_ranks"), (21, 1, b"n_ranks"), (3, -1, b"rank"), (3, 3, b"rank"), (3, 0, b"cannot be block rank"),
                        (3, 2, b"cannot be block rank"), (2, 1, b"cannot be block rank")):
        assert start(G=G, rk=rk) == E, (G, rk)
        refused(pre + "start_dev_async", what)
        assert lanczos(G=G, rk=rk) == E
        refused(pre + "lanczos_dev_async", what)
        for p, fn in phases.items():
            assert fn(h._h, V(z), V(w.ws), G, rk) == E, (p, G, rk)
            refused(pre + p + "_dev_async", what)
        assert L.ctd_kkt_minres_schur_cr_shard_begin_dev_async(h._h, V(w.ws), G, rk) == E
        refused(pre + "begin_dev_async", what)
    # pointers: null and misaligned, by name; overlapping ranges
    for kw, what in ((dict(r=None), b"rhs"), (dict(zz=None), b"z is"), (dict(ww=None), b"ws"), (dict(sw=None), b"schur_ws"),
                     (dict(r=V(s.rhs, 4)), b"rhs is not aligned"), (dict(zz=V(z, 4)), b"z is not aligned"), (dict(ww=V(w.ws, 4)), b"ws is not aligned"),
                     (dict(sw=V(P.ws, 4)), b"schur_ws is not aligned"), (dict(zz=V(w.ws, 8 * 16)), b"z overlaps the workspace"),
                     (dict(sw=V(w.ws, 8 * 16)), b"schur_ws must not overlap"), (dict(sw=V(z)), b"schur_ws must not overlap"),
                     (dict(zz=V(s.rhs)), b"input"), (dict(sw=V(s.rhs)), b"input"), (dict(rtol=-1.0), b"rtol"), (dict(mi=0), b"max_iter")):
        assert start(**kw) == E, kw
        refused(pre + "start_dev_async", what)
    none = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0)
    assert start(sy=none) == E
    refused(pre + "start_dev_async", b"px")
    for bad_sys in (lib.ctd_kkt_system(struct_size=0), lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system) + 8)):
        assert start(sy=bad_sys) == E
        refused(pre + "start_dev_async", b"struct_size")
    for kw, what in ((dict(sw=None), b"schur_ws"), (dict(zz=None), b"z is"), (dict(ww=None), b"ws"), (dict(sw=V(P.ws, 4)), b"schur_ws is not aligned"),
                     (dict(zz=V(w.ws, 8 * 64)), b"z overlaps the workspace"), (dict(sw=V(w.ws, 8 * 64)), b"schur_ws must not overlap")):
        assert lanczos(**kw) == E, kw
        refused(pre + "lanczos_dev_async", what)
    for p, fn in phases.items():
        for zz, ww, what in ((None, V(w.ws), b"z is"), (V(z), None, b"ws"), (V(z, 4), V(w.ws), b"z is not aligned"), (V(z), V(w.ws, 4), b"ws is not aligned"),
                             (V(w.ws, 8 * 64), V(w.ws), b"z overlaps the workspace")):
            assert fn(h._h, zz, ww, 3, 1) == E
            refused(pre + p + "_dev_async", what)
    assert L.ctd_kkt_minres_schur_cr_shard_begin_dev_async(h._h, None, 3, 1) == E
    refused(pre + "begin_dev_async", b"ws")
    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    assert L.ctd_kkt_minres_schur_cr_shard_info(h._h, None, 3, C.byref(info)) == E
    refused(pre + "info", b"ws")
    # mix-ups: a workspace factored for another range, by the whole grid, or by the chunked family, given to this range's solve:
    # recognised on the device, nothing is stored; the status query says so
    lay = s.full.kkt_schur_cr_layout()
    Pw = s.full.kkt_schur_cr_factor(s.jvals, s.pxd, s.pcd, s.sc, torch.empty(lay.workspace, dtype=torch.float64, device="cuda"))
    Pc = s.full.kkt_schur_factor(s.jvals, s.pxd, s.pcd, s.sc, 7, torch.empty(s.full.kkt_schur_layout(7).workspace, dtype=torch.float64, device="cuda"))
    assert Ps[0].layout.n_blocks == P.layout.n_blocks == 7, "ranks 0 and 1 have the same N_r and m: only the step range tells them apart"
    for other in (Ps[0], Ps[2], Pw, Pc):
        before = other.ws.view(torch.int64).clone()
        assert solve(h, other.ws, s.sc, out) == 0
        h.sync()
        assert bool((out == 7.0).all()), "a foreign workspace: nothing is stored"
        assert torch.equal(other.ws.view(torch.int64), before)
        assert L.ctd_kkt_schur_cr_shard_info(h._h, V(other.ws), C.byref(bad)) == E
        refused("ctd_kkt_schur_cr_shard_info", b"no factor")
    # ... and inside the solve: the start's launches of the solve store nothing into y, so beta1^2 lacks the block rows' terms but
    # nothing of the foreign workspace is written
    before = Ps[0].ws.view(torch.int64).clone()
    z2 = torch.empty_like(z)
    assert start(sw=V(Ps[0].ws), zz=V(z2)) == 0
    h.sync()
    assert torch.equal(Ps[0].ws.view(torch.int64), before)
    # the shard's workspace given to the whole-grid solve of a whole-grid handle: nothing is stored
    assert L.ctd_kkt_schur_cr_solve_dev_async(s.full._h, V(P.ws), V(s.sc), V(out)) == 0
    s.full.sync()
    assert bool((out == 7.0).all())
    # the whole-grid entry points go on refusing the shard handle
    assert L.ctd_kkt_schur_cr_solve_dev_async(h._h, V(P.ws), V(s.sc), V(out)) == E
    assert b"no shard form" in L.ctd_last_error(h._h) and L.ctd_last_error(h._h).startswith(b"ctd_kkt_schur_cr_solve_dev_async: ")
    # the refused calls left the factor usable, and the good calls go through
    assert L.ctd_kkt_schur_cr_shard_info(h._h, V(P.ws), C.byref(bad)) == 0 and bad.value == -1
    assert solve(h, P.ws, s.sc, out) == 0 and start() == 0
    h.sync()
    assert not bool((out == 7.0).all()) and not bool((z == 7.0).all())


def test_wide_blocks_are_refused_on_the_device(torch_cuda):
    """block_rows = 65 (a run-time OCP: no registry problem has more than 64): every device entry point of both families refuses
    the handle with CTD_EINVAL, by name, before it looks at its pointers"""
    L, lib = ct._lib.lib(), ct._lib
    name, sch, m = wide_ocp()
    h = ct.DOCP(name, 6, sch, device=0, pattern="structural", value_order="csr", steps=(2, 4))
    ks = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0)
    pre = "ctd_kkt_minres_schur_cr_shard_"
    calls = {"ctd_kkt_schur_cr_shard_factor_dev_async": lambda: L.ctd_kkt_schur_cr_shard_factor_dev_async(h._h, None, None, None, None),
             "ctd_kkt_schur_cr_shard_solve_dev_async": lambda: L.ctd_kkt_schur_cr_shard_solve_dev_async(h._h, None, None, None),
             "ctd_kkt_schur_cr_shard_info": lambda: L.ctd_kkt_schur_cr_shard_info(h._h, None, None),
             pre + "start_dev_async": lambda: L.ctd_kkt_minres_schur_cr_shard_start_dev_async(h._h, C.byref(ks), None, None, None, None, 3, 1, 1e-10, 10),
             pre + "begin_dev_async": lambda: L.ctd_kkt_minres_schur_cr_shard_begin_dev_async(h._h, None, 3, 1),
             pre + "alfa_dev_async": lambda: L.ctd_kkt_minres_schur_cr_shard_alfa_dev_async(h._h, None, None, 3, 1),
             pre + "lanczos_dev_async": lambda: L.ctd_kkt_minres_schur_cr_shard_lanczos_dev_async(h._h, None, None, None, 3, 1),
             pre + "update_dev_async": lambda: L.ctd_kkt_minres_schur_cr_shard_update_dev_async(h._h, None, None, 3, 1)}
    for fn, call in calls.items():
        assert call() == lib.CTD_EINVAL, fn
        err = L.ctd_last_error(h._h)
        assert err.startswith(fn.encode() + b": ") and f"block_rows = {m} exceeds 64".encode() in err, (fn, err)
    h.close()


# ---- 11. the order of the cross-rank sum, from the slots -------------------------------------------------------------------------
def test_cross_rank_sum_order(torch_cuda, cases):
    """begin adds the gathered slots in the order of tests/schur_shard_ref.py's cross_rank_sum: the ranks' own partial sums, ranks
    ascending, THEN the ranks ascending again with the solves' partial sums.  The gathered areas are overwritten with numbers whose
    sum depends on the order (1e16 absorbs every 1.0 added before -1e16 cancels it): this order gives 6, rank-interleaved 8.
    beta1 = sqrt of the sum, to one ulp of the square root.  (C) adds beta^2 through the same device function."""
    torch, s = torch_cuda, cases(G7)
    ph = s.phases(s.factors())
    ph.start(0.0, 10)
    torch.cuda.synchronize()
    own, solve = [[1e16], [1.0], [1.0]], [[-1e16, 1.0, 1.0], [1.0, 1.0], [1.0, 1.0]]
    want = cross_rank_sum(own, solve)
    assert want == 6.0
    for r in ph.ranks:
        slot, ga = r.w.layout.slot, r.w.gathered_a
        for q in range(s.G):
            base = q * slot
            assert float(ga[base + SLOT_COUNT]) == len(own[q]) and float(ga[base + SLOT_SCHUR_COUNT]) == len(solve[q]) == s.cuts[q + 1] - s.cuts[q]
            ga[base:base + len(own[q])] = torch.tensor(own[q], dtype=torch.float64, device="cuda")
            ga[base + SLOT_SCHUR:base + SLOT_SCHUR + len(solve[q])] = torch.tensor(solve[q], dtype=torch.float64, device="cuda")
    for r in ph.ranks:
        r.docp.kkt_minres_schur_shard_begin(r.w, r.rank)
    infos = ph.infos()
    root = float(np.sqrt(want))
    print("beta1 per rank", [i.beta1 for i in infos], "sqrt(6)", root)
    assert all(i == infos[0] for i in infos) and infos[0].status == "running"
    assert abs(infos[0].beta1 - root) <= float(np.spacing(root)), (infos[0].beta1, root)


def test_solve_partial_sums_from_the_slots(torch_cuda):
    """the partial sums of r2 . y that a rank's solve leaves in its send slot are those of solve_partial_sums (workgroup g: the
    local blocks g, g + G_r, ..; lanes from 0.0; the shuffle tree), bit for bit -- 290 blocks on rank 0, so that a workgroup adds
    more than one block, 10 on rank 1 -- and beta1 is the square root of cross_rank_sum over the gathered slots, to one ulp"""
    torch = torch_cuda
    s = Case(torch, ("goddard", "trapeze", 300, (0, 290, 300), False))
    ph = s.phases(s.factors())
    ph.start(0.0, 10)
    torch.cuda.synchronize()
    own, solve = [], []
    for k, r in enumerate(ph.ranks):
        n_r = s.cuts[k + 1] - s.cuts[k]
        G_r = min(n_r, 256)
        send = r.w.send_a.cpu().numpy()
        assert send[SLOT_SCHUR_COUNT] == G_r and (send[SLOT_SCHUR + G_r:SLOT_SCHUR_COUNT] == 0.0).all() and not np.signbit(send[SLOT_SCHUR + G_r:SLOT_SCHUR_COUNT]).any()
        vec = r.w.ws[:3 * s.n].cpu().numpy().reshape(3, s.n)                # r1, r2, y
        rows = slice(s.nvar + s.cuts[k] * s.m, s.nvar + s.cuts[k + 1] * s.m)
        got, ref = send[SLOT_SCHUR:SLOT_SCHUR + G_r], np.array(solve_partial_sums(vec[1][rows], vec[2][rows], s.m, n_r))
        assert np.array_equal(got, ref), (k, "the solve's partial sums: not the order of solve_partial_sums", np.abs(got - ref).max())
        own.append(list(send[:int(send[SLOT_COUNT])]))
        solve.append(list(got))
        ga = r.w.gathered_a.cpu().numpy()
        assert all(np.array_equal(ga[q * r.w.layout.slot:(q + 1) * r.w.layout.slot], ph.ranks[q].w.send_a.cpu().numpy()) for q in range(s.G))
    infos = ph.infos()
    root = float(np.sqrt(cross_rank_sum(own, solve)))
    print("beta1", infos[0].beta1, "sqrt(cross_rank_sum)", root, "own terms", [len(o) for o in own], "solve terms", [len(o) for o in solve])
    assert all(i == infos[0] for i in infos) and abs(infos[0].beta1 - root) <= float(np.spacing(root)), (infos[0].beta1, root)
    s.close()


# ---- 12. ShardedDOCP with one rank ----------------------------------------------------------------------------------------------------
def test_sharded_docp_with_one_rank(torch_cuda):
    """ShardedDOCP.kkt_schur_cr_precond and kkt_minres(precond="schur_cr") with world = 1: the matrix of DOCP.kkt_minres with
    "schur_cr" on the whole grid (px comes from the shard form of the diagonals: the iteration counts agree, not the bits)"""
    torch = torch_cuda
    prob, sch, N = "goddard", "trapeze", 7
    s = Case(torch, (prob, sch, N, (0, N), False))
    kw = dict(device=0, pattern="structural", value_order="csr")
    sd = cdist.ShardedDOCP(lambda steps: ct.DOCP(prob, N, sch, steps=steps, **kw), N, world=1, rank=0)
    zw, iw = s.full.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond="schur_cr", rtol=1e-10, max_iter=10 * s.n)
    P = sd.kkt_schur_cr_precond(s.x, s.y, 1.0, s.sx, s.sc)
    assert isinstance(P, ct.SchurCrShardPrecond) and sd.docp.kkt_schur_cr_shard_info(P) == -1
    za, ia = sd.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=P, rtol=1e-10, max_iter=10 * s.n)
    za = za.clone()
    zb, ib = sd.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond="schur_cr", rtol=1e-10, max_iter=10 * s.n)
    assert ia == ib and ia.status == "converged" and torch.equal(za, zb)
    assert iw.status == "converged" and abs(ia.iterations - iw.iterations) <= 2, (ia, iw)
    with pytest.raises(ValueError, match="schur_cr"):
        sd.kkt_minres(s.x, s.y, s.rhs, precond="schur")
    sd.close()
    s.close()
