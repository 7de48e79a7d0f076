"""The joined form of the log-depth Schur preconditioner on the MI355X (ctd_kkt_schur_cr_joint_*; DOCP.kkt_schur_cr_joint_*,
dist.kkt_schur_cr_joint_shards / kkt_schur_cr_joint_apply_shards).  Shards are handles of one process on device 0, as in
tests/test_gpu_kkt_schur_cr_shard.py, whose Case (handles, inputs of minres_case, asm_precond's pair, the whole-grid handle's own
Jacobian values) is used here.

The reference is tests/schur_joint_ref.py: the separator elimination stated densely on K_asm's own blocks.

BARS
  backward error   eta = |T y - r|_inf / (|T|_inf |y|_inf + |r|_inf) against the dense T of the WHOLE grid (no coupling dropped)
                   <= max(10 eta_ref, 64 eps), eta_ref that of the reference on the same case and right-hand side: the bar of
                   tests/test_gpu_kkt_schur_cr.py and tests/test_gpu_kkt_schur_cr_shard.py.
  symmetry         |u . (M v) - (M u) . v| <= 1e-13 max(|u . (M v)|, |(M u) . v|) and <= 1e-13 |M^-1|_inf |M u| |M v|: the margins of
                   tests/test_gpu_kkt_schur_cr_shard.py.
  identity         |(sum_r r_I . g_r + sigma) - r . y| / |r . y| <= max(10 defect_ref, 64 eps), defect_ref the same figure of the
                   reference; g_r read from out between the local solve and the join, sigma from the workspace.
Everything else is exact: bit equality (the spikes against single solves, one rank against the shard form, the reduced factor, x_s
and sigma across the ranks), statuses, refusals, read and write sets."""
import numpy as np
import pytest

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from ctdirect_jl_amd import dist as cdist
from guarded import guarded
from jit_defs import twin
from schur_joint_ref import SchurJointRef, backward_error
from schur_ref import small_sc_case
from schur_shard_ref import shard_cuts
from test_gpu_kkt_minres import dev, minres_case
from test_gpu_kkt_schur_cr_shard import Case

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
FIXED = 512
# (problem, scheme, N, cuts, run-time twin, sc = 1e-8 U(1, 2)): the smallest shapes that take each branch
CASES = [("goddard", "trapeze", 5, (0, 1, 3, 5), False, False),      # every interior is one block (no level); both spikes on one block
         ("goddard", "trapeze", 7, (0, 2, 5, 7), False, False),      # interiors of 2, 2 and 1 blocks
         ("goddard", "trapeze", 7, (0, 3, 5, 7), False, False),      # ... of 3, 1 and 1
         ("goddard", "trapeze", 20, (0, 7, 13, 20), False, False),
         ("goddard", "trapeze", 20, tuple(shard_cuts(20, 8)), False, False),      # more ranks than levels
         ("goddard", "gauss_legendre_2", 20, tuple(shard_cuts(20, 8)), False, True),      # m = 9, cond(T) about 1e10
         ("quadrotor", "gauss_legendre_2", 6, (0, 2, 4, 6), False, False),      # m = 25: the 32-row instantiation
         ("goddard", "midpoint", 7, (0, 3, 5, 7), True, False)]      # a run-time OCP
G5, G7, G20x8, GL2 = CASES[0], CASES[2], CASES[4], CASES[5]
M9 = ("goddard", "gauss_legendre_2", 7, (0, 3, 7), False, False)       # m = 9 with minres_case's own sc
case_id = lambda c: f"{c[0]}-{c[1]}-N{c[2]}-" + "_".join(map(str, c[3])) + ("-rt" if c[4] else "") + ("-small_sc" if c[5] else "")      # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class JointCase(Case):
    def __init__(self, torch, case, c=None):
        prob, sch, N, cuts, rt, small = case
        if c is None:
            c = minres_case(prob, sch, N)
            c = small_sc_case(c) if small else c
        super().__init__(torch, (prob, sch, N, cuts, rt), c)
        self.name = twin(prob) if rt else prob
        self.sch = sch
        self._jref = None

    @property
    def jref(self):
        if self._jref is None:
            self._jref = SchurJointRef(self.c, self.px, self.pc, self.m, self.N, self.nv, self.cuts)
        return self._jref

    def joint(self, **kw):
        return cdist.kkt_schur_cr_joint_shards(self.hs, kw.get("jvals", self.jvals), kw.get("px", self.pxd), self.pcd, kw.get("sc", self.sc))

    def region(self, P, off, n):
        return P.ws[off:off + n]


@pytest.fixture(scope="module")
def cases(torch_cuda):
    made = {}

    def get(case):
        if case not in made:
            made[case] = JointCase(torch_cuda, case)
        return made[case]

    yield get
    for s in made.values():
        s.close()


def bits(t):
    import torch
    return t.view(torch.int64)


def factor_bits(lay, w):
    """the words of a workspace (as int64) that the factor owns and no solve writes: the interior's status words and blocks, the
    interface blocks and the spikes, the reduced factor"""
    import torch
    n_fac = FIXED + lay.n_int + 3 * lay.n_int * lay.block_rows ** 2
    return torch.cat([w[1:9], w[FIXED:n_fac], w[lay.off_es:lay.off_scratch], w[lay.off_reduced:lay.off_rs]])


# ---- 1. the application against the dense T, the identity, equal decisions ---------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_error_and_identity(torch_cuda, cases, case):
    torch = torch_cuda
    s = cases(case)
    m, G = s.m, s.G
    r = np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon)
    rd, = dev(torch, r)
    keep = rd.clone()
    Ps = s.joint()
    for k, (h, P) in enumerate(zip(s.hs, Ps)):
        lay = P.layout
        n_int = s.cuts[k + 1] - s.cuts[k] - (1 if k else 0)
        assert (lay.n_ranks, lay.rank, lay.step_begin, lay.step_end, lay.n_int) == (G, k, s.cuts[k], s.cuts[k + 1], n_int)
        assert (lay.separator, lay.int_begin, lay.n_levels) == (s.cuts[k] if k else -1, s.cuts[k] + (1 if k else 0), (n_int - 1).bit_length())
        assert h.kkt_schur_cr_joint_info(P) == -1
    # local solves, the gather, the joins -- g is read in between
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    for h, P in zip(s.hs, Ps):
        h.kkt_schur_cr_joint_solve_local(P, rd, out)
    s.hs[0].sync()
    g = out.cpu().numpy().copy()
    gathered = torch.cat([P.xsend for P in Ps])
    for h, P in zip(s.hs, Ps):
        h.kkt_schur_cr_joint_solve_join(P, gathered, out)
    y = out.cpu().numpy()
    assert (y[s.nb:] == 7.0).all(), "the tail rows of out are left untouched"
    assert torch.equal(rd, keep), "r is not modified"
    assert torch.equal(out, cdist.kkt_schur_cr_joint_apply_shards(s.hs, Ps, rd, torch.full_like(out, 7.0))), "the driver gives the same bits"
    y_ref, inner_ref, sigma_ref, _, _ = s.jref.solve_parts(r[:s.nb])
    T = s.jref.T
    eta, eta_ref = backward_error(T, y[:s.nb], r[:s.nb]), backward_error(T, y_ref, r[:s.nb])
    print(case_id(case), "m", m, "eta", eta, "eta_ref", eta_ref, "forward difference", np.linalg.norm(y[:s.nb] - y_ref) / np.linalg.norm(y_ref))
    assert eta <= max(10.0 * eta_ref, 64.0 * EPS), (case, eta, eta_ref)
    # equal decisions: the reduced factor, rs~, x_s and sigma have the same bits on every rank
    lay0 = Ps[0].layout
    red = lambda P: bits(P.ws[P.layout.off_reduced:P.layout.off_sigma + 1])      # noqa: E731
    for P in Ps[1:]:
        assert P.layout.off_sigma - P.layout.off_reduced == lay0.off_sigma - lay0.off_reduced
        assert torch.equal(red(P), red(Ps[0])), "the reduced factor, rs~, x_s or sigma differ between ranks"
    # the identity: r . y = sum_r r_I . g_r + sigma
    sigma = float(Ps[0].ws[lay0.off_sigma])
    inner = sum(float(r[P.layout.int_begin * m:P.layout.step_end * m] @ g[P.layout.int_begin * m:P.layout.step_end * m]) for P in Ps)
    ry, ry_ref = float(r[:s.nb] @ y[:s.nb]), float(r[:s.nb] @ y_ref)
    defect, defect_ref = abs(inner + sigma - ry) / abs(ry), abs(sum(inner_ref) + sigma_ref - ry_ref) / abs(ry_ref)
    print(case_id(case), "r.y", ry, "sum r_I.g", inner, "sigma", sigma, "defect", defect, "defect_ref", defect_ref)
    assert sigma >= 0.0 and inner >= 0.0
    assert defect <= max(10.0 * defect_ref, 64.0 * EPS), (case, defect, defect_ref)


# ---- 2. symmetry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [G5, G7, M9], ids=case_id)
def test_symmetry(torch_cuda, cases, case):
    """on systems with minres_case's own sc, as in tests/test_gpu_kkt_schur_cr_shard.py: the margin relative to |u . M v| presumes
    eps cond(T) well below 1e-13 |u . M v| / (|M u| |v|), which sc = 1e-8 (cond(T) about 1e10) does not give"""
    torch = torch_cuda
    s = cases(case)
    g = np.random.default_rng(9)
    u, v = dev(torch, g.uniform(-1.0, 1.0, s.n), g.uniform(-1.0, 1.0, s.n))
    Ps = s.joint()

    def apply_M(w):
        out = torch.empty(s.n, dtype=torch.float64, device="cuda")
        out[:s.nvar] = w[:s.nvar] / s.pxd
        out[s.nvar + s.nb:] = w[s.nvar + s.nb:] / s.pcd[s.nb:]
        cdist.kkt_schur_cr_joint_apply_shards(s.hs, Ps, w[s.nvar:].contiguous(), out[s.nvar:])
        s.hs[0].sync()
        return out

    Mu, Mv = apply_M(u), apply_M(v)
    a, b = float(u @ Mv), float(Mu @ v)
    norm_minv = max(float(s.px.max()), float(np.abs(s.jref.T).sum(axis=1).max()), float(s.pc[s.nb:].max()) if s.nb < s.ncon else 0.0)
    scale = norm_minv * float(Mu.norm()) * float(Mv.norm())
    print(case_id(case), "u.Mv", a, "Mu.v", b, "difference / scale", abs(a - b) / scale, "difference / |u.Mv|", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b)), (case, a, b)
    assert abs(a - b) <= 1e-13 * scale, (case, a, b, scale)


# ---- 3. the spikes pin the multi-column sum order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [G5, CASES[1], M9], ids=case_id)
def test_spikes_are_single_solves(torch_cuda, cases, case):
    """every column of Wl / Wr has the bits of ctd_kkt_schur_cr_shard_solve on a shard handle of the interior's steps, with the
    column of the stored E[s] / E[b]' in the first / last block as the right-hand side"""
    torch = torch_cuda
    s = cases(case)
    m, mm = s.m, s.m * s.m
    Ps = s.joint()
    for k, P in enumerate(Ps):
        lay = P.layout
        a, se, n_int = lay.int_begin, lay.step_end, lay.n_int
        d = ct.DOCP(s.name, s.N, s.sch, steps=(a, se), device=0, pattern="structural", value_order="csr")
        Q = d.kkt_schur_cr_shard_factor(s.jvals, s.pxd, s.pcd, s.sc)
        Es = s.region(P, lay.off_es, mm).view(m, m)
        Eb = s.region(P, lay.off_eb, mm).view(m, m)
        Wl = s.region(P, lay.off_wl, n_int * mm).view(n_int * m, m)
        Wr = s.region(P, lay.off_wr, n_int * mm).view(n_int * m, m)
        sides = ([("Wl", Wl, a, Es)] if k > 0 else []) + ([("Wr", Wr, se - 1, Eb.t())] if k < s.G - 1 else [])
        assert sides, "more than one rank: every rank has a spike"
        for name, W, blk, cols in sides:
            assert bool(cols.abs().sum() > 0), (k, name, "the interface block is not zero")
            for j in range(m):
                rhs = torch.zeros(s.ncon, dtype=torch.float64, device="cuda")
                rhs[blk * m:(blk + 1) * m] = cols[:, j]
                x = d.kkt_schur_cr_shard_solve(Q, rhs)
                assert torch.equal(bits(W[:, j].contiguous()), bits(x[a * m:se * m].contiguous())), (k, name, j, "not the bits of a single solve")
        if k == 0:
            assert not bool(Wl.any()) and not bool(Es.any()), "rank 0 has no left spike: zero"
        if k == s.G - 1:
            assert not bool(Wr.any()) and not bool(Eb.any()), "the last rank has no right spike: zero"
        d.close()


# ---- 4. one rank: the bits of the shard form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 7))
def test_one_rank_is_the_shard_form(torch_cuda, N):
    torch = torch_cuda
    s = JointCase(torch, ("goddard", "trapeze", N, (0, N), False, False))
    d = s.full
    P, = s.joint()
    Q = d.kkt_schur_cr_shard_factor(s.jvals, s.pxd, s.pcd, s.sc)
    lay = P.layout
    assert (lay.n_sep, lay.separator, lay.int_begin, lay.n_int) == (1, -1, 0, N)
    assert (lay.factor_join_launches, lay.solve_join_launches, lay.solve_local_launches) == (0, 0, Q.layout.solve_launches)
    assert lay.factor_local_launches == Q.layout.factor_launches and lay.off_es == Q.layout.workspace
    nfac = FIXED + N + 3 * N * s.m ** 2
    assert torch.equal(bits(P.ws[FIXED:nfac]), bits(Q.ws[FIXED:nfac])), "the interior's factor: the bits of the shard form"
    assert d.kkt_schur_cr_joint_info(P) == -1
    r, = dev(torch, np.random.default_rng(5).uniform(-1.0, 1.0, s.ncon))
    out = cdist.kkt_schur_cr_joint_apply_shards([d], [P], r, torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda"))
    d.sync()
    want = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    d.kkt_schur_cr_shard_solve(Q, r, out=want)
    assert torch.equal(bits(out), bits(want)), "out: not the bits of ctd_kkt_schur_cr_shard_solve_dev_async"
    s.close()


# ---- 5. read and write sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (0, 1))
def test_read_and_write_sets(torch_cuda, cases, shift):
    torch = torch_cuda
    s = cases(G7)
    m = s.m
    Gd = lambda n, like=None: guarded(torch, n, shift, "cuda", like)      # noqa: E731
    nan = float("nan")
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    P0 = s.joint()
    out0 = cdist.kkt_schur_cr_joint_apply_shards(s.hs, P0, r, torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda"))
    s.hs[0].sync()
    ins = {nm: Gd(t.numel(), t).snapshot() for nm, t in (("px", s.pxd), ("pc", s.pcd), ("sc", s.sc))}
    gws, gsend, Ps = [], [], []
    for k, h in enumerate(s.hs):
        lay = P0[k].layout
        # NaN everywhere outside the stated read set of jvals: the rank's own range and the halo behind it
        jv = torch.full_like(s.jvals, nan)
        jv[lay.jvals_begin:lay.jvals_end] = s.jvals[lay.jvals_begin:lay.jvals_end]
        jv[lay.jvals_halo_begin:lay.jvals_halo_end] = s.jvals[lay.jvals_halo_begin:lay.jvals_halo_end]
        assert lay.jvals_halo_begin == lay.jvals_end and (lay.jvals_halo_end > lay.jvals_halo_begin) == (k < s.G - 1)
        assert lay.jvals_halo_end - lay.jvals_begin < s.jvals.numel()
        gj = Gd(jv.numel(), jv).snapshot()
        gws.append(Gd(lay.workspace))
        gsend.append(Gd(lay.factor_slot))
        Ps.append(h.kkt_schur_cr_joint_factor_local(gj.view, ins["px"].view, ins["pc"].view, ins["sc"].view, s.G, k, ws=gws[k].view,
                                                    send=gsend[k].view))
        h.sync()
        assert gj.unchanged("jvals") and gws[k].guards_intact(f"factor_local of rank {k}") and gsend[k].guards_intact(f"record of rank {k}")
        assert gws[k].unwritten() == [] and gsend[k].unwritten() == [], "factor_local writes the whole workspace and the whole record"
        assert torch.equal(gsend[k].bits(), bits(P0[k].send)), (k, "the factor read outside its read set")
    gathered = Gd(s.G * Ps[0].layout.factor_slot, torch.cat([P.send for P in Ps])).snapshot()
    for k, (h, P) in enumerate(zip(s.hs, Ps)):
        h.kkt_schur_cr_joint_factor_join(P, gathered.view)
        h.sync()
        assert gws[k].guards_intact(f"factor_join of rank {k}") and gathered.unchanged("gathered")
        assert torch.equal(factor_bits(P.layout, gws[k].bits()), factor_bits(P.layout, bits(P0[k].ws))), (k, "not the bits of the run on ordinary tensors")
    # the application: r is read on the rank's block rows only; out is written there only
    fac = [factor_bits(P.layout, g.bits()).clone() for g, P in zip(gws, Ps)]
    gout = [Gd(s.ncon) for _ in s.hs]
    gx = [Gd(P.layout.solve_slot) for P in Ps]
    for k, (h, P) in enumerate(zip(s.hs, Ps)):
        rr = torch.full_like(r, nan)
        rr[s.rows(k)] = r[s.rows(k)]
        gr = Gd(s.ncon, rr).snapshot()
        h.kkt_schur_cr_joint_solve_local(P, gr.view, gout[k].view, send=gx[k].view)
        h.sync()
        assert gr.unchanged("r") and gout[k].guards_intact(f"solve_local of rank {k}") and gx[k].guards_intact(f"solve record of rank {k}")
        assert gx[k].unwritten() == [], "the whole solve record is written"
        lay = P.layout
        assert gout[k].unwritten() == [i for i in range(s.ncon) if not lay.int_begin * m <= i < lay.step_end * m], \
            (k, "solve_local writes the interior rows only")
    gxs = Gd(s.G * Ps[0].layout.solve_slot, torch.cat([g.view for g in gx])).snapshot()
    for k, (h, P) in enumerate(zip(s.hs, Ps)):
        h.kkt_schur_cr_joint_solve_join(P, gxs.view, gout[k].view)
        rows = s.rows(k)
        assert gout[k].guards_intact(f"solve_join of rank {k}") and gws[k].guards_intact(f"solve of rank {k}") and gxs.unchanged("gathered")
        assert gout[k].unwritten() == [i for i in range(s.ncon) if not rows.start <= i < rows.stop], (k, "out is written on the rank's block rows only")
        assert torch.equal(gout[k].bits()[rows], bits(out0)[rows]), (k, "not the bits of the run on ordinary tensors")
        assert torch.equal(factor_bits(P.layout, gws[k].bits()), fac[k]), "the solve only reads the factors"
    for nm, g in ins.items():
        assert g.unchanged(nm)


# ---- 6. foreign workspaces ---------------------------------------------------------------------------------------------------------------
def test_foreign_workspaces(torch_cuda, cases):
    """a workspace of the whole-grid family or of the shard form given to this family, one of this family given to them, and one
    factored for another split: nothing is stored, info returns CTD_EINVAL"""
    torch = torch_cuda
    s = cases(G7)
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    Ps = s.joint()
    k, h, P = 1, s.hs[1], Ps[1]
    lay = P.layout
    gathered = torch.cat([Q.xsend for Q in Ps]).clone()
    fgath = torch.cat([Q.send for Q in Ps]).clone()
    sh = h.kkt_schur_cr_shard_layout()
    big = lambda: torch.zeros(max(lay.workspace, sh.workspace, s.full.kkt_schur_cr_layout().workspace), dtype=torch.float64, device="cuda")      # noqa: E731
    # (a) the shard form's factor of the same handle, (b) the whole grid's factor, (c) this family's for the same steps as rank 1 of 2
    wa, wb = big(), big()
    h.kkt_schur_cr_shard_factor(s.jvals, s.pxd, s.pcd, s.sc, ws=wa[:sh.workspace])
    s.full.kkt_schur_cr_factor(s.jvals, s.pxd, s.pcd, s.sc, wb[:s.full.kkt_schur_cr_layout().workspace])
    h.sync()
    s.full.sync()
    foreign = [("shard form", wa), ("whole grid", wb)]
    for name, w in foreign:
        F = ct.SchurCrJointPrecond(s.pxd, s.pcd, w[:lay.workspace], lay, P.send, torch.full_like(P.xsend, 3.0))
        before = w.clone()
        out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
        h.kkt_schur_cr_joint_factor_join(F, fgath)
        h.kkt_schur_cr_joint_solve_local(F, r, out)
        h.kkt_schur_cr_joint_solve_join(F, gathered, out)
        assert torch.equal(bits(w), bits(before)), (name, "the workspace was written")
        assert bool((out == 7.0).all()) and bool((F.xsend == 3.0).all()), (name, "out or the record was written")
        with pytest.raises(ct.CTDirectError) as e:
            h.kkt_schur_cr_joint_info(F)
        assert e.value.status == _lib.CTD_EINVAL
    # this family's workspace in the hands of the shard form and of the whole-grid form
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    before = P.ws.clone()
    padded = big()
    padded[:lay.workspace] = P.ws
    h.kkt_schur_cr_shard_solve(ct.SchurCrShardPrecond(s.pxd, s.pcd, padded[:sh.workspace], sh), r, out=out)
    assert bool((out == 7.0).all()) and torch.equal(bits(padded[:lay.workspace]), bits(before)), "the shard form stored something"
    with pytest.raises(ct.CTDirectError) as e:
        h.kkt_schur_cr_shard_info(ct.SchurCrShardPrecond(s.pxd, s.pcd, padded[:sh.workspace], sh))
    assert e.value.status == _lib.CTD_EINVAL
    # another split of the same steps: the last handle [5, 7) factored as rank 1 of 2, used as rank 2 of 3
    hl = s.hs[2]
    Q = hl.kkt_schur_cr_joint_factor_local(s.jvals, s.pxd, s.pcd, s.sc, 2, 1)
    l3 = Ps[2].layout
    w = torch.zeros(max(Q.layout.workspace, l3.workspace), dtype=torch.float64, device="cuda")
    w[:Q.layout.workspace] = Q.ws
    before = w.clone()
    F = ct.SchurCrJointPrecond(s.pxd, s.pcd, w[:l3.workspace], l3, Ps[2].send, torch.full_like(P.xsend, 3.0))
    out = torch.full((s.ncon,), 7.0, dtype=torch.float64, device="cuda")
    hl.kkt_schur_cr_joint_factor_join(F, fgath)
    hl.kkt_schur_cr_joint_solve_local(F, r, out)
    hl.kkt_schur_cr_joint_solve_join(F, gathered, out)
    assert torch.equal(bits(w), bits(before)) and bool((out == 7.0).all()) and bool((F.xsend == 3.0).all()), "another split: something was stored"
    with pytest.raises(ct.CTDirectError) as e:
        hl.kkt_schur_cr_joint_info(F)
    assert e.value.status == _lib.CTD_EINVAL


# ---- 7. records that do not cover the grid, a failed pivot -------------------------------------------------------------------------------
def test_bad_records_and_pivots(torch_cuda, cases):
    torch = torch_cuda
    s = cases(G7)
    m = s.m
    r, = dev(torch, np.random.default_rng(4).uniform(-1.0, 1.0, s.ncon))
    # the records of ranks 1 and 2 swapped: not an ascending cover -> the reduced factor is NaN on every rank
    Ps = s.joint()
    slot = Ps[0].layout.factor_slot
    swapped = torch.cat([Ps[0].send, Ps[2].send, Ps[1].send])
    assert swapped.numel() == 3 * slot
    for h, P in zip(s.hs, Ps):
        h.kkt_schur_cr_joint_factor_join(P, swapped)
        assert h.kkt_schur_cr_joint_info(P) == 0
    y = cdist.kkt_schur_cr_joint_apply_shards(s.hs, Ps, r)
    s.hs[0].sync()
    assert bool(torch.isnan(y[:s.nb]).all()), "every block row is NaN"
    # a non-positive pivot on one interior block of one rank (sc < 0 there): an arithmetic outcome that reaches every rank
    bad_block = 4           # the interior of rank 1 of (0, 3, 5, 7)
    sc = s.sc.clone()
    sc[bad_block * m:(bad_block + 1) * m] = -1e6
    Ps = s.joint(sc=sc)
    infos = [h.kkt_schur_cr_joint_info(P) for h, P in zip(s.hs, Ps)]
    print("first bad blocks", infos)
    assert int(bits(Ps[1].ws)[FIXED]) >= 0 and Ps[1].layout.int_begin == bad_block, "the rank that owns the block records the pivot"
    assert infos == [3, 3, 3], "every rank sees the first separator whose reduced pivot is NaN: the smallest block with a record"
    y = cdist.kkt_schur_cr_joint_apply_shards(s.hs, Ps, r)
    s.hs[0].sync()
    assert bool(torch.isnan(y[:s.nb]).all()), "x_s is NaN on every rank, hence every block row"
    sig = [float(P.ws[P.layout.off_sigma]) for P in Ps]
    assert all(np.isnan(v) for v in sig), "sigma is NaN on every rank: beta^2 would be NaN everywhere"
