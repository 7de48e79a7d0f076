"""The sharded MINRES solve with the joined form of the log-depth Schur preconditioner on the MI355X
(ctd_kkt_minres_schur_cr_joint_*; DOCP.kkt_minres_schur_joint_*, dist.MinresPhases / kkt_minres_shards with one SchurCrJointPrecond
per shard).  Shards are handles of one process on device 0; JointCase and its inputs are those of
tests/test_gpu_kkt_schur_cr_joint.py, the reference is the dense statement of tests/schur_joint_ref.py.

BARS
  iteration counts   Goddard trapeze N = 300, sc = 1e-8 U(1, 2), at 3 and 8 shards: converged; within the spread of the reference's
                     pinned row (max - min over G of COUNTS of tests/test_kkt_schur_cr_joint_cpu.py) of the reference's count for
                     the same cuts, and strictly below the cut form's pinned count for those cuts (62 and 135).
  first iterates     |z_k - z_k(scipy on K_asm with the dense exact M)| / |...| <= 10 d_ref, k in {1, 2, 5}; d_ref the same distance
                     for scipy driven by the GPU kktprod and the GPU joined application, the maximum over the cases of the run.
  identity           on the device: the gathered partial sums of r_I . g_r + sigma against r2 . y formed from the corrected y,
                     relative, <= max(10 defect_ref, 64 eps), defect_ref the reference's figure for the same right-hand side.
Everything else is exact: bit equality (one shard against ctd_kkt_minres_schur_cr_dev, across runs, across check_every, frozen
iterations, a graph replay), the ranks' state bytes, statuses."""
import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

from ctdirect_jl_amd import dist as cdist
from schur_ref import small_sc_case
from schur_shard_ref import shard_cuts
from test_gpu_kkt_minres import minres_case, rel
from test_gpu_kkt_schur_cr_joint import CASES, G7, JointCase, case_id
from test_gpu_kkt_schur_cr_shard import state_bytes
from test_kkt_schur_cr_joint_cpu import COUNTS
from test_kkt_schur_cr_shard_cpu import COUNTS as CUT_COUNTS

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
KS = (1, 2, 5)
G20 = CASES[3]          # Goddard trapeze N = 20, cuts (0, 7, 13, 20)
G20x8 = CASES[4]
SLOT_SCHUR, SLOT_SCHUR_COUNT = 2080, 2080 + 256          # csrc/ctd_krylov_shard_kernels.hpp


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


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


# ---- 1. one shard: the bits of the whole-grid solve ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (2, 7))
def test_one_shard_is_the_whole_grid(torch_cuda, N):
    torch = torch_cuda
    s = JointCase(torch, ("goddard", "trapeze", N, (0, N), False, False))
    d = s.full
    lay = d.kkt_schur_cr_layout()
    Pw = d.kkt_schur_cr_factor(s.jvals, s.pxd, s.pcd, s.sc, torch.empty(lay.workspace, dtype=torch.float64, device="cuda"))
    Ps = s.joint()
    assert Ps[0].send is None and Ps[0].xsend is None, "one rank has no record"
    for kw in [dict(rtol=0.0, max_iter=k) for k in KS] + [dict(rtol=1e-10, max_iter=10 * s.n)]:
        zw, iw = d.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=Pw, **kw)
        (z,), (info,) = s.shards(Ps, **kw)
        assert info == iw, (kw, info, iw)
        assert torch.equal(z, zw), (kw, "z: not the bits of ctd_kkt_minres_schur_cr_dev")
    s.close()


# ---- 2. iteration counts: the assertion that fails without the feature -------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_grid():
    return small_sc_case(minres_case("goddard", "trapeze", 300))


@pytest.mark.parametrize("G", (3, 8))
def test_iteration_counts(torch_cuda, long_grid, G):
    key = ("goddard", "trapeze", 300, True)
    ref = COUNTS[key]
    spread = max(ref.values()) - min(ref.values())
    s = JointCase(torch_cuda, ("goddard", "trapeze", 300, tuple(shard_cuts(300, G)), False, True), long_grid)
    Ps = s.joint()
    assert [h.kkt_schur_cr_joint_info(P) for h, P in zip(s.hs, Ps)] == [-1] * G
    zs, infos = s.shards(Ps, rtol=1e-10, max_iter=10 * s.n)
    print("G", G, "reference", ref[G], "spread of its row", spread, "cut form", CUT_COUNTS[key][G], "| device:", infos[0], "residual", s.res(s.compose(zs)))
    assert all(i == infos[0] for i in infos) and infos[0].status == "converged", infos
    assert abs(infos[0].iterations - ref[G]) <= spread, (infos[0].iterations, ref[G], spread)
    assert infos[0].iterations < CUT_COUNTS[key][G], (infos[0].iterations, CUT_COUNTS[key][G])
    s.close()


# ---- 3. first iterates -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def first_iterates(torch_cuda, cases):
    torch = torch_cuda
    out = {}
    for case in (G7, G20, G20x8):
        s = cases(case)
        c, d, nvar, n = s.c, s.full, s.nvar, s.n
        zin, zout, rc, yc = (torch.empty(k, dtype=torch.float64, device="cuda") for k in (n, n, s.ncon, s.ncon))

        def matvec(v):
            zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
            d.kktprod(s.x, s.y, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=s.sx, sc=s.sc, out=(zout[:nvar], zout[nvar:]))
            return zout.cpu().numpy()

        K_op = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
        Ps = s.joint()
        M_ref = s.jref.operator()

        def gpu_M(v):
            v = np.asarray(v, dtype=np.float64).ravel()
            rc.copy_(torch.from_numpy(np.ascontiguousarray(v[nvar:])))
            cdist.kkt_schur_cr_joint_apply_shards(s.hs, Ps, rc, yc)
            return np.r_[v[:nvar] / s.px, yc[:s.nb].cpu().numpy(), v[nvar + s.nb:] / s.pc[s.nb:]]

        M_op = LinearOperator((n, n), matvec=gpu_M, dtype=np.float64)
        for k in KS:
            z_asm, _ = minres(c["K_asm"], c["rhs"], M=M_ref, rtol=0.0, maxiter=k)
            z_op, _ = minres(K_op, c["rhs"], M=M_op, rtol=0.0, maxiter=k)
            zs, infos = s.shards(Ps, rtol=0.0, max_iter=k)
            out[(case, k)] = (rel(s.compose(zs), z_asm), rel(z_op, z_asm), infos)
    return out


@pytest.mark.parametrize("case", (G7, G20, G20x8), ids=case_id)
def test_first_iterates(first_iterates, case):
    d_ref = max(v[1] for v in first_iterates.values())
    print("d_ref", d_ref, "| largest device difference", max(v[0] for v in first_iterates.values()))
    assert np.isfinite(d_ref) and d_ref > 0.0
    for (cs, k), (err, ref, infos) in first_iterates.items():
        if cs != case:
            continue
        print(case_id(case), "k", k, "shards vs K_asm", err, "GPU operator and application vs K_asm", ref, infos[0])
        assert all(i == infos[0] for i in infos), infos
        assert infos[0].iterations == k and infos[0].status == "max_iter", infos[0]
        assert err <= 10.0 * d_ref, (case, k, err, d_ref)


# ---- 4. the identity on the device: gathered partial sums + sigma ----------------------------------------------------------------------
@pytest.mark.parametrize("case", (G7, G20x8, CASES[5]), ids=case_id)
def test_identity_from_the_slots(torch_cuda, cases, case):
    """after start and the gather of slot A, begin's join launches leave the corrected y and sigma: the partial sums of r_I . g_r
    read from the gathered slots, added in the kernels' order, plus sigma, against r2 . y on the block rows"""
    torch = torch_cuda
    s = cases(case)
    Ps = s.joint()
    ph = s.phases(Ps)
    ph.start(1e-10, 100)
    s.hs[0].sync()
    nvar, nb, n = s.nvar, s.nb, s.n
    w = ph.ranks[0].w
    slot = w.layout.slot
    assert slot == 2080 + 256 + 16 + 3 * 64 + 16
    ga = w.gathered_a.cpu().numpy()
    part = np.float64(0.0)
    for r in range(s.G):
        cnt = int(ga[r * slot + SLOT_SCHUR_COUNT])
        assert cnt == min(Ps[r].layout.n_int, 256)
        for b in range(cnt):
            part = part + ga[r * slot + SLOT_SCHUR + b]
    sigma = float(Ps[0].ws[Ps[0].layout.off_sigma])
    r2 = s.c["rhs"][nvar:nvar + nb]
    y = np.zeros(nb)
    for k, rk in enumerate(ph.ranks):
        y[s.rows(k)] = rk.w.ws[2 * n + nvar:2 * n + nvar + nb].cpu().numpy()[s.rows(k)]        # (y is the third vector of the workspace)
    ry = float(r2 @ y)
    y_ref, inner_ref, sigma_ref, _, _ = s.jref.solve_parts(r2)
    ry_ref = float(r2 @ y_ref)
    defect, defect_ref = abs(float(part) + sigma - ry) / abs(ry), abs(sum(inner_ref) + sigma_ref - ry_ref) / abs(ry_ref)
    print(case_id(case), "partial sums", float(part), "sigma", sigma, "r2.y", ry, "defect", defect, "defect_ref", defect_ref)
    assert rel(y, y_ref) <= 1e-6, "y on the block rows is T^-1 r2"
    assert defect <= max(10.0 * defect_ref, 64.0 * EPS), (case, defect, defect_ref)


# ---- 5. state and reproducibility --------------------------------------------------------------------------------------------------------
def test_state_and_reproducibility(torch_cuda, cases):
    torch, s = torch_cuda, cases(G20)
    cap = 10 * s.n
    Ps = s.joint()
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
        if ce in runs:
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
    s = JointCase(torch, G20)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Ps = s.joint()
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


# ---- 6. breakdown ------------------------------------------------------------------------------------------------------------------------
def test_breakdown_on_every_rank(torch_cuda, cases):
    """a non-positive pivot on one interior block of the middle rank (sc < 0 there) reaches every rank's beta1^2 as NaN through the
    records: all ranks end with "breakdown" after the same chunk.  An arithmetic outcome, not a fault"""
    torch, s = torch_cuda, cases(G20)
    bad_block = s.cuts[1] + 2
    sc = s.sc.clone()
    sc[bad_block * s.m:(bad_block + 1) * s.m] = -1e6
    Ps = s.joint(sc=sc)
    infos = [h.kkt_schur_cr_joint_info(P) for h, P in zip(s.hs, Ps)]
    assert all(i >= 0 for i in infos), infos
    chunks = [0]
    zs, infos = s.shards(Ps, rtol=1e-10, max_iter=50, check_every=4, on_chunk=lambda ph, i: chunks.__setitem__(0, chunks[0] + 1))
    assert all(i == infos[0] for i in infos) and infos[0].status == "breakdown" and infos[0].iterations == 0, infos
    assert chunks[0] == 1, "every rank ends after the same chunk"
    for k, z in enumerate(zs):
        m = torch.from_numpy(s.own_mask(k)).cuda()
        assert not bool(z[m].any()) and bool(torch.isfinite(z[m]).all()), (k, "z = 0")


def test_cross_rank_sum_order(torch_cuda, cases):
    """begin adds the gathered slots in the order of joint_sum of tests/schur_joint_ref.py: the ranks' own partial sums, ranks
    ascending, then the ranks ascending again with the partial sums of r_I . g_r, then sigma, once.  The partial sums in the gathered
    areas are overwritten with numbers whose sum depends on the order (1e16 absorbs every 1.0 added before -1e16 cancels it); the
    records stay, so begin's join launches leave the sigma they left before.  This order gives 4 + sigma, sigma first or a
    rank-interleaved order another value.  beta1 = sqrt of the sum, to one ulp of the square root"""
    from schur_joint_ref import joint_sum
    torch, s = torch_cuda, cases(G7)
    Ps = s.joint()
    ph = s.phases(Ps)
    ph.start(0.0, 10)
    torch.cuda.synchronize()
    sigma = float(Ps[0].ws[Ps[0].layout.off_sigma])
    assert sigma > 1.0
    own, solve = [[1e16], [1.0], [1.0]], [[-1e16, 1.0, 1.0], [1.0], [1.0]]
    want = joint_sum(own, solve, sigma)
    assert want == 4.0 + sigma and joint_sum(own, solve, 0.0) == 4.0
    assert (((((((0.0 + sigma) + 1e16) + 1.0) + 1.0) - 1e16) + 1.0) + 1.0) + 1.0 + 1.0 != want, "sigma first would be another sum"
    for r in ph.ranks:
        slot, ga = r.w.layout.slot, r.w.gathered_a
        for q in range(s.G):
            base = q * slot
            assert float(ga[base + 2064]) == len(own[q]) and float(ga[base + SLOT_SCHUR_COUNT]) == len(solve[q]) == Ps[q].layout.n_int
            ga[base:base + len(own[q])] = torch.tensor(own[q], dtype=torch.float64, device="cuda")
            ga[base + SLOT_SCHUR:base + SLOT_SCHUR + len(solve[q])] = torch.tensor(solve[q], dtype=torch.float64, device="cuda")
    for r in ph.ranks:
        r.docp.kkt_minres_schur_joint_begin(r.precond, r.w, r.rank)
    infos = ph.infos()
    assert [float(P.ws[P.layout.off_sigma]) for P in Ps] == [sigma] * s.G, "the records did not change: the same sigma on every rank"
    root = float(np.sqrt(want))
    print("beta1 per rank", [i.beta1 for i in infos], "sqrt(4 + sigma)", root, "sigma", sigma)
    assert all(i == infos[0] for i in infos) and infos[0].status == "running"
    assert abs(infos[0].beta1 - root) <= float(np.spacing(root)), (infos[0].beta1, root)


def test_a_workspace_of_another_family_is_refused(torch_cuda, cases):
    """the phase methods check the slot length the workspace was cut with before the pointer reaches the library"""
    s = cases(G7)
    Ps, Qs = s.joint(), s.factors()
    h = s.hs[1]
    for w in (h.kkt_minres_shard_workspace(3), h.kkt_minres_schur_shard_workspace(3)):
        for call in (lambda: h.kkt_minres_schur_joint_begin(Ps[1], w, 1), lambda: h.kkt_minres_schur_joint_alfa(s.rhs, w, 1),
                     lambda: h.kkt_minres_schur_joint_update(Ps[1], s.rhs, w, 1), lambda: h.kkt_minres_schur_joint_info(w)):
            with pytest.raises(ValueError, match="slots of"):
                call()
        assert not bool(w.ws.any()), "nothing was written"
    wj = h.kkt_minres_schur_joint_workspace(3, 1)
    for call in (lambda: h.kkt_minres_schur_shard_begin(wj, 1), lambda: h.kkt_minres_shard_begin(wj, 1),
                 lambda: h.kkt_minres_schur_shard_lanczos(Qs[1], s.rhs, wj, 1)):
        with pytest.raises(ValueError, match="slots of"):
            call()
    assert not bool(wj.ws.any())


def test_a_mix_of_preconditioners_is_refused(torch_cuda, cases):
    s = cases(G20)
    Ps = s.joint()
    Qs = s.factors()
    with pytest.raises(ValueError, match="on every shard or on none"):
        s.phases([Ps[0], Qs[1], Ps[2]])
