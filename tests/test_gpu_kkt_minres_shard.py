"""The shard form of the device-resident MINRES solve on the MI355X (ctd_kkt_minres_shard_*; DOCP.kkt_minres_shard_*,
dist.kkt_minres_shards, ShardedDOCP.kkt_minres): three shard handles of one process on device 0 beside a handle of the whole grid,
in the manner of tests/test_gpu_kktprod_shard.py.  The inputs, K_asm and the preconditioner are those of tests/test_gpu_kkt_minres.py
(minres_case, asm_precond: assembled on the CPU from the oracle, no code under test involved).

BARS
  one shard          bit equality with DOCP.kkt_minres: z (torch.equal) and every field of MinresInfo.
  three shards       |z_k - z_k(scipy on K_asm)| / |z_k(scipy on K_asm)| <= 10 d_ref, k in {1, 2, 5}: the rule of
                     tests/test_gpu_kkt_minres.py, d_ref the largest such difference between scipy driven by the GPU kktprod
                     operator and scipy on K_asm over the cases of this file, measured in the same run on the reference side.
                     The full solve (Goddard trapeze N = 20, seed 21, rtol 1e-10, cuts (0, 7, 13, 20)): converged, iterations within
                     +-2 of the whole-grid device solve's, true residual within the rho^2 margin of scipy's run.
Everything else is exact: ownership, identical state bytes on every rank, freeze, reproducibility, capture, refusals."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import dist as cdist
from guarded import guarded
from helpers import bench_inputs, describe
from jit_defs import twin
from test_gpu_kkt_minres import KS, asm_precond, dev, diag_op, minres_case, rel, scipy_solve

pytestmark = pytest.mark.gpu

# one shard: (problem, scheme, N) -- nv = 1: the tail path; nv = 0 and a one-point scheme; a Gauss-Legendre scheme
ONE = [("goddard", "trapeze", 7), ("double_integrator_path", "midpoint", 20), ("goddard", "gauss_legendre_2", 5)]
# three shards: the same transcriptions with the cuts (0, 2, 5, 7), one-step shards (0, 1, 2, 3) and (0, 7, 13, 20)
THREE = [("goddard", "trapeze", 7, (0, 2, 5, 7)), ("goddard", "trapeze", 3, (0, 1, 2, 3)),
         ("double_integrator_path", "midpoint", 20, (0, 7, 13, 20)), ("double_integrator_path", "midpoint", 3, (0, 1, 2, 3)),
         ("goddard", "gauss_legendre_2", 7, (0, 2, 5, 7)), ("goddard", "gauss_legendre_2", 3, (0, 1, 2, 3))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class Case:
    """one transcription: the whole-grid handle, the shard handles of `cuts`, the inputs of minres_case on the device"""

    def __init__(self, torch, prob, sch, N, cuts=None):
        self.torch, self.c = torch, minres_case(prob, sch, N)
        c = self.c
        self.nvar, self.ncon, self.n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
        kw = dict(device=0, pattern="structural")
        self.full = ct.DOCP(prob, N, sch, **kw)
        self.hs = [ct.DOCP(prob, N, sch, steps=(cuts[k], cuts[k + 1]), **kw) for k in range(len(cuts) - 1)] if cuts else []
        self.px, self.pc = asm_precond(c)
        self.x, self.y, self.sx, self.sc, self.rhs, self.pxd, self.pcd = dev(torch, c["x"], c["y"], c["sx"], c["sc"], c["rhs"], self.px, self.pc)
        self.lays = [h.kkt_minres_shard_layout(len(self.hs)) for h in self.hs]

    def pre(self, on):
        return (self.pxd, self.pcd) if on else None

    def shards(self, handles, pre=True, **kw):
        precond = self.pre(pre) if isinstance(pre, bool) else pre
        return cdist.kkt_minres_shards(handles, [self.x] * len(handles), self.y, self.rhs, sx=self.sx, sc=self.sc, precond=precond, **kw)

    def whole(self, pre=True, **kw):
        return self.full.kkt_minres(self.x, self.y, self.rhs, sx=self.sx, sc=self.sc, precond=self.pre(pre), **kw)

    def own_mask(self, k):
        lay, m = self.lays[k], np.zeros(self.n, dtype=bool)
        for a, b in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            m[a:b] = True
        return m

    def compose(self, zs):
        """z from the ranks' owned entries (the tail from the last rank); the pieces cover everything"""
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
        """the ranks' iterates agree bit for bit on the owned entries (the others are not the solve's)"""
        masks = [self.torch.from_numpy(self.own_mask(k)).cuda() for k in range(len(self.hs))]
        return all(self.torch.equal(a[m], b[m]) for a, b, m in zip(za, zb, masks))

    def close(self):
        for h in [self.full] + self.hs:
            h.close()


def state_bytes(torch, w):
    return w.ws[w.layout.off_state:w.layout.off_state + 16].view(torch.int64).cpu().numpy().copy()


# ---- 1. one shard is the whole-grid solve, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch,N", ONE, ids=[f"{p}-{s}-N{N}" for p, s, N in ONE])
def test_one_shard_is_the_whole_grid_solve(torch_cuda, prob, sch, N):
    torch = torch_cuda
    s = Case(torch, prob, sch, N)
    for pre in (False, True):
        for kw in [dict(rtol=0.0, max_iter=k) for k in KS] + [dict(rtol=1e-10, max_iter=10 * s.n)]:
            zw, iw = s.whole(pre, **kw)
            (z,), (info,) = s.shards([s.full], pre, **kw)
            assert info == iw, (pre, kw, info, iw)
            assert torch.equal(z, zw), (pre, kw, "z: not the bits of DOCP.kkt_minres")
            assert iw.status != "running" and (kw["rtol"] or iw.iterations == kw["max_iter"]), iw
    s.close()


# ---- 2. three shards against the reference arithmetic -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_shard_iterates(torch_cuda):
    """per case, preconditioner, k: (|z_shards - z_asm| / |z_asm|, |z_op - z_asm| / |z_asm|, the ranks' infos)"""
    torch, out = torch_cuda, {}
    for prob, sch, N, cuts in THREE:
        s = Case(torch, prob, sch, N, cuts)
        c, nvar, n = s.c, s.nvar, s.n
        zin = torch.empty(n, dtype=torch.float64, device="cuda")
        zout = torch.empty(n, dtype=torch.float64, device="cuda")

        def matvec(v):
            zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
            s.full.kktprod(s.x, s.y, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=s.sx, sc=s.sc, out=(zout[:nvar], zout[nvar:]))
            return zout.cpu().numpy()

        K_op = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
        for pre in (False, True):
            M = diag_op(s.px, s.pc) if pre else None
            for k in KS:
                z_asm, _ = minres(c["K_asm"], c["rhs"], M=M, rtol=0.0, maxiter=k)
                z_op, _ = minres(K_op, c["rhs"], M=M, rtol=0.0, maxiter=k)
                zs, infos = s.shards(s.hs, pre, rtol=0.0, max_iter=k)
                out[(prob, sch, N, pre, k)] = (rel(s.compose(zs), z_asm), rel(z_op, z_asm), infos)
        s.close()
    return out


def test_three_shards_first_iterates(three_shard_iterates):
    res = three_shard_iterates
    d_ref = max(v[1] for v in res.values())
    worst = max(res, key=lambda key: res[key][0])
    print("d_ref", d_ref, "| bar", 10.0 * d_ref, "| largest sharded difference", res[worst][0], "at", worst)
    assert np.isfinite(d_ref) and d_ref > 0.0
    for key, (err, ref, infos) in res.items():
        print(key, "three shards vs K_asm", err, "GPU operator vs K_asm", ref)
        assert all(i == infos[0] for i in infos), (key, infos)
        assert infos[0].iterations == key[-1] and infos[0].status == "max_iter", (key, infos[0])
        assert err <= 10.0 * d_ref, (key, err, d_ref)


@pytest.fixture(scope="module")
def solve20(torch_cuda):
    return Case(torch_cuda, "goddard", "trapeze", 20, (0, 7, 13, 20))


def test_three_shards_full_solve(solve20):
    s = solve20
    cap = 10 * s.n
    _, info_ref, it_ref, res = scipy_solve(s.c, diag_op(s.px, s.pc), cap)
    assert info_ref == 0
    rho = max(1.0, (res[-6] / res[-1]) ** 0.2)
    _, iw = s.whole(rtol=1e-10, max_iter=cap)
    zs, infos = s.shards(s.hs, rtol=1e-10, max_iter=cap)
    z = s.compose(zs)
    r = float(np.linalg.norm(s.c["K_asm"] @ z - s.c["rhs"]) / np.linalg.norm(s.c["rhs"]))
    print("three shards:", infos[0], "residual", r, "| whole grid:", iw, "| scipy on K_asm: iterations", it_ref, "residual", res[-1], "rho", rho)
    assert all(i == infos[0] for i in infos) and infos[0].status == "converged", infos
    assert abs(infos[0].iterations - iw.iterations) <= 2, (infos[0], iw)
    assert r <= rho * rho * res[-1], (r, res[-1], rho)


# ---- 3. ownership -----------------------------------------------------------------------------------------------------------------
def test_a_rank_writes_its_owned_entries_only(torch_cuda, solve20):
    torch, s = torch_cuda, solve20
    G = len(s.hs)
    ws = [h.kkt_minres_shard_workspace(G) for h in s.hs]
    for w in ws:
        w.ws[:8 * s.n].fill_(777.0)
    zs = [torch.full((s.n,), 777.0, dtype=torch.float64, device="cuda") for _ in range(G)]
    _, infos = s.shards(s.hs, rtol=0.0, max_iter=5, out=zs, workspaces=ws)
    assert infos[0].iterations == 5
    lay = s.lays[0]
    for k in range(G):
        m = s.own_mask(k)
        zk = zs[k].cpu().numpy()
        assert (zk[~m] == 777.0).all(), (k, "z written outside the owned entries")
        assert not (zk[m] == 777.0).any(), k
        vec = ws[k].ws[:8 * s.n].cpu().numpy().reshape(8, s.n)
        for j in (0, 1, 2, 5, 6, 7):           # r1, r2, y, w, w2, minv: owned entries only (v and kv also receive halos / K v)
            assert (vec[j][~m] == 777.0).all(), (k, j, "a workspace vector written outside the owned entries")
        assert torch.equal(zs[k][lay.tail_begin:lay.tail_end], zs[0][lay.tail_begin:lay.tail_end]), (k, "the tails differ")
    assert not (s.compose(zs) == 777.0).any()


# ---- 4. identical decisions -------------------------------------------------------------------------------------------------------
def test_every_rank_takes_the_same_decisions(torch_cuda, solve20):
    torch, s = torch_cuda, solve20
    cap = 10 * s.n
    runs = {}
    for ce in (1, 3, 16):
        chunks = [0]

        def on_chunk(ph, infos):
            chunks[0] += 1
            st = [state_bytes(torch, r.w) for r in ph.ranks]
            assert all(np.array_equal(b, st[0]) for b in st), (ce, chunks[0], "the ranks' KrylovState bytes differ")
            assert all(i == infos[0] for i in infos)

        ph_keep = []
        zs, infos = s.shards(s.hs, rtol=1e-10, max_iter=cap, check_every=ce, on_chunk=lambda ph, i: (ph_keep.append(ph), on_chunk(ph, i)))
        assert infos[0].status == "converged" and chunks[0] == -(-infos[0].iterations // ce), (ce, infos[0], chunks[0])
        runs[ce] = ([z.clone() for z in zs], infos, ph_keep[-1])
    for ce in (3, 16):
        assert runs[ce][1] == runs[1][1], (ce, "MinresInfo depends on check_every")
        assert s.same(runs[ce][0], runs[1][0]), (ce, "z depends on check_every")
    # sixteen iterations enqueued after convergence: no bit of any rank's z or state changes
    zs, infos, ph = runs[16]
    before = [state_bytes(torch, r.w) for r in ph.ranks]
    ph.iterate(16)
    assert ph.infos() == infos
    for r, z0, b0 in zip(ph.ranks, zs, before):
        assert torch.equal(r.z, z0) and np.array_equal(state_bytes(torch, r.w), b0), r.rank


# ---- 5. reproducibility and modes -------------------------------------------------------------------------------------------------
def test_reproducible_and_x_modes(torch_cuda, solve20):
    torch, s = torch_cuda, solve20
    za, ia = s.shards(s.hs, rtol=0.0, max_iter=9)
    za = [z.clone() for z in za]
    zb, ib = s.shards(s.hs, rtol=0.0, max_iter=9)
    assert ia == ib and s.same(za, zb)
    # x read in place through the table: every shard's x holds its own variables and v, NaN elsewhere
    cuts = (0, 7, 13, 20)
    xs = []
    for k, lay in enumerate(s.lays):
        xk = torch.full_like(s.x, float("nan"))
        xk[lay.var_begin:lay.var_end] = s.x[lay.var_begin:lay.var_end]
        xk[lay.tail_begin:lay.tail_end] = s.x[lay.tail_begin:lay.tail_end]
        xs.append(xk)
    for k, h in enumerate(s.hs):
        h.set_x_shards(list(cuts), [t.data_ptr() for t in xs], k)
    zc, ic = cdist.kkt_minres_shards(s.hs, xs, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=s.pre(True), rtol=0.0, max_iter=9)
    for h in s.hs:
        h.set_x_shards(None, None, 0)
    assert ic == ia and s.same(za, zc), "in-place x differs from x with copied halos"


def test_run_time_ocp_gives_the_bits_of_its_registry_twin(torch_cuda):
    torch = torch_cuda
    prob, sch, N, cuts = "goddard_all", "midpoint", 7, (0, 2, 5, 7)
    results = []
    for name in (prob, twin(prob)):
        hs = [ct.DOCP(name, N, sch, device=0, pattern="structural", steps=(cuts[k], cuts[k + 1])) for k in range(3)]
        nvar, ncon = hs[0].dim_NLP_variables, hs[0].dim_NLP_constraints
        r = np.random.default_rng(11)
        x, y = bench_inputs(describe(hs[0], prob, sch), perturb=1e-3), 0.1 * r.uniform(-1.0, 1.0, ncon)
        sx, sc, rhs = 1.0 + r.uniform(0.0, 1.0, nvar), 1.0 + r.uniform(0.0, 1.0, ncon), r.uniform(-1.0, 1.0, nvar + ncon)
        xd, yd, sxd, scd, rhsd = dev(torch, x, y, sx, sc, rhs)
        zs, infos = cdist.kkt_minres_shards(hs, [xd] * 3, yd, rhsd, sx=sxd, sc=scd, rtol=0.0, max_iter=6)
        results.append(([z.clone() for z in zs], infos, [h.kkt_minres_shard_layout(3) for h in hs]))
        for h in hs:
            h.close()
    (za, ia, lays), (zb, ib, _) = results
    assert ia == ib and ia[0].iterations == 6
    for a, b, lay in zip(za, zb, lays):
        for lo, hi in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            assert torch.equal(a[lo:hi], b[lo:hi])


# ---- 6. breakdown and cap ---------------------------------------------------------------------------------------------------------
def test_breakdown_and_cap_on_every_rank(torch_cuda, solve20):
    torch, s = torch_cuda, solve20
    pc = s.pcd.clone()
    row = s.lays[1].row_begin - s.nvar + 1          # a row of the middle rank
    pc[row] = -1e-12
    pres = [(s.pxd, s.pcd), (s.pxd, pc), (s.pxd, s.pcd)]
    zs, infos = s.shards(s.hs, pres, rtol=1e-10, max_iter=50)
    assert all(i == infos[0] for i in infos) and infos[0].status == "breakdown" and infos[0].iterations == 0, infos
    for k, z in enumerate(zs):
        m = torch.from_numpy(s.own_mask(k)).cuda()
        assert not bool(z[m].any()), (k, "z touched by the iteration that broke down")
    zs, infos = s.shards(s.hs, rtol=1e-10, max_iter=3)
    assert all(i == infos[0] for i in infos) and infos[0].status == "max_iter" and infos[0].iterations == 3, infos


def test_breakdown_inside_the_iteration_on_every_rank(torch_cuda):
    """the breakdown branch of (C) with several ranks: rhs is a unit vector at the first variable (rank 0) and one entry of pc in the
    middle rank's rows is negative and tiny.  beta1^2 is positive; r2 is EXACTLY zero at that row until the Krylov space reaches it
    (the operator is block-banded: products with exact zeros are exact zeros), then r2' M r2 is negative: every rank reports the
    breakdown at the same iteration >= 1, and z is the iterate of the iterations completed -- the bits of a run capped there."""
    torch = torch_cuda
    s = Case(torch, "double_integrator_path", "midpoint", 20, (0, 7, 13, 20))
    assert s.full.dims.NLP_v == 0
    rhs = torch.zeros_like(s.rhs)
    rhs[0] = 1.0
    pc = s.pcd.clone()
    pc[s.lays[1].row_begin - s.nvar + 1] = -1e-12
    run = lambda **kw: cdist.kkt_minres_shards(s.hs, [s.x] * 3, s.y, rhs, sx=s.sx, sc=s.sc, precond=(s.pxd, pc), rtol=0.0, **kw)      # noqa: E731
    zs, infos = run(max_iter=60, check_every=4)
    print("breakdown inside the iteration:", infos[0])
    assert all(i == infos[0] for i in infos) and infos[0].status == "breakdown", infos
    it = infos[0].iterations
    assert 1 <= it < 60 and infos[0].beta1 > 0.0, infos[0]
    zs = [z.clone() for z in zs]
    zc, ic = run(max_iter=it, check_every=1)
    assert ic[0].status == "max_iter" and ic[0].iterations == it, ic
    assert s.same(zs, zc), "z was touched by the iteration that broke down"
    assert any(bool(z[torch.from_numpy(s.own_mask(k)).cuda()].any()) for k, z in enumerate(zs))
    s.close()


# ---- 7. guards --------------------------------------------------------------------------------------------------------------------
def test_between_guards_at_odd_and_even_offsets(torch_cuda):
    torch = torch_cuda
    s = Case(torch, "goddard", "trapeze", 7, (0, 2, 5, 7))
    want, iw = s.shards(s.hs, rtol=0.0, max_iter=5)
    want = [z.clone() for z in want]
    inputs = [guarded(torch, a.numel(), 1, "cuda", like=a).snapshot() for a in (s.rhs, s.pxd, s.pcd, s.x, s.y)]
    rhs, px, pc, x, y = (g.view for g in inputs)
    for shift in (1, 2):
        gz = [guarded(torch, s.n, shift, "cuda") for _ in s.hs]
        gw = [guarded(torch, lay.workspace, shift, "cuda") for lay in s.lays]
        ws = [h.kkt_minres_shard_workspace(3, ws=g.view) for h, g in zip(s.hs, gw)]
        zs, infos = cdist.kkt_minres_shards(s.hs, [x] * 3, y, rhs, sx=s.sx, sc=s.sc, precond=(px, pc), rtol=0.0, max_iter=5,
                                            out=[g.view for g in gz], workspaces=ws)
        assert infos == iw
        for k in range(3):
            gz[k].guards_intact(f"z of rank {k}, shift {shift}")
            gw[k].guards_intact(f"workspace of rank {k}, shift {shift}")
            m = torch.from_numpy(s.own_mask(k)).cuda()
            assert torch.equal(zs[k][m], want[k][m]), (k, shift, "not the bits of the run on ordinary tensors")
        for g, nm in zip(inputs, ("rhs", "px", "pc", "x", "y")):
            g.unchanged(nm)
    s.close()


# ---- 8. capture -------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_a_chunk(torch_cuda):
    torch = torch_cuda
    s = Case(torch, "goddard", "trapeze", 20)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ph = cdist.minres_shards([s.full], [s.x], s.y, s.rhs, sx=s.sx, sc=s.sc, precond=s.pre(True))
        ph.start(0.0, 1000)
        ph.iterate(4)                   # the warm solve
    side.synchronize()
    z_eager, info_eager = ph.ranks[0].z.clone(), ph.infos()
    assert info_eager[0].iterations == 4
    with torch.cuda.stream(side):
        ph.start(0.0, 1000)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ph.iterate(4)
    g.replay()
    torch.cuda.synchronize()
    assert ph.infos() == info_eager and torch.equal(ph.ranks[0].z, z_eager)
    s.full.set_stream(torch.cuda.current_stream())
    s.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda, solve20):
    torch, s = torch_cuda, solve20
    L, lib = ct._lib.lib(), ct._lib
    E = lib.CTD_EINVAL
    h = s.hs[1]
    w = h.kkt_minres_shard_workspace(3)
    z = torch.full((s.n,), 7.0, dtype=torch.float64, device="cuda")
    V = lambda a, off=0: None if a is None else C.c_void_p(a.data_ptr() + off)        # noqa: E731
    ks = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, px=s.pxd.data_ptr(), pc=s.pcd.data_ptr())
    start = lambda hh=h, sy=ks, r=V(s.rhs), zz=V(z), ww=V(w.ws), G=3, k=1, rtol=1e-10, mi=10: \
        L.ctd_kkt_minres_shard_start_dev_async(hh._h, C.byref(sy), r, zz, ww, G, k, rtol, mi)        # noqa: E731
    phases = {p: getattr(L, f"ctd_kkt_minres_shard_{p}_dev_async") for p in ("alfa", "lanczos", "update")}

    def refused(name, what, hh=h):
        err = L.ctd_last_error(hh._h)
        assert err.startswith(b"ctd_kkt_minres_shard_" + name + b": ") and what in err, (name, what, err)
        hh.sync()
        assert bool((z == 7.0).all()) and not bool(w.ws.any()), name

    for G, k, what in ((0, 0, b"n_ranks"), (-2, 0, b"n_ranks"), (21, 1, b"n_ranks"), (3, -1, b"rank"), (3, 3, b"rank"),
                       (3, 0, b"cannot be block rank"), (3, 2, b"cannot be block rank"), (2, 1, b"cannot be block rank")):
        assert start(G=G, k=k) == E, (G, k)
        refused(b"start_dev_async", what)
        for p, fn in phases.items():
            assert fn(h._h, V(z), V(w.ws), G, k) == E, (p, G, k)
            refused(p.encode() + b"_dev_async", what)
        assert L.ctd_kkt_minres_shard_begin_dev_async(h._h, V(w.ws), G, k) == E
        refused(b"begin_dev_async", what)
    # the whole-grid handle is rank 0 of 1 and nothing else; the first shard is not a middle rank
    assert start(hh=s.full, G=3, k=1) == E and b"cannot be block rank" in L.ctd_last_error(s.full._h)
    assert start(hh=s.hs[0], G=3, k=1) == E and b"cannot be block rank" in L.ctd_last_error(s.hs[0]._h)
    # pointers: null and misaligned, by name
    for kw, what in ((dict(r=None), b"rhs"), (dict(zz=None), b"z is"), (dict(ww=None), b"ws"), (dict(r=V(s.rhs, 4)), b"rhs is not aligned"),
                     (dict(zz=V(z, 4)), b"z is not aligned"), (dict(ww=V(w.ws, 4)), b"ws is not aligned")):
        assert start(**kw) == E, kw
        refused(b"start_dev_async", what)
    for p, fn in phases.items():
        for zz, ww, what in ((None, V(w.ws), b"z is"), (V(z), None, b"ws"), (V(z, 4), V(w.ws), b"z is not aligned"), (V(z), V(w.ws, 4), b"ws is not aligned")):
            assert fn(h._h, zz, ww, 3, 1) == E
            refused(p.encode() + b"_dev_async", what)
    assert L.ctd_kkt_minres_shard_begin_dev_async(h._h, None, 3, 1) == E
    refused(b"begin_dev_async", b"ws")
    # start's own: px without pc, a misaligned px, z an input, rtol, max_iter
    one = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, px=s.pxd.data_ptr())
    assert start(sy=one) == E
    refused(b"start_dev_async", b"px and pc")
    odd = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, px=s.pxd.data_ptr() + 4, pc=s.pcd.data_ptr())
    assert start(sy=odd) == E
    refused(b"start_dev_async", b"px is not aligned")
    for bad in (lib.ctd_kkt_system(struct_size=0), lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system) + 8)):
        assert start(sy=bad) == E
        refused(b"start_dev_async", b"struct_size")
    before = s.rhs.clone()
    assert start(zz=V(s.rhs)) == E
    refused(b"start_dev_async", b"input")
    assert torch.equal(s.rhs, before)
    # ranges, not addresses: z inside the workspace, rhs a view into it
    assert start(zz=V(w.ws, 8 * 16)) == E
    refused(b"start_dev_async", b"z overlaps the workspace")
    assert start(zz=V(w.ws, 8 * (w.layout.workspace - 1))) == E
    refused(b"start_dev_async", b"z overlaps the workspace")
    assert start(r=V(w.ws, 8 * 8)) == E
    refused(b"start_dev_async", b"input")
    for p, fn in phases.items():
        assert fn(h._h, V(w.ws, 8 * 64), V(w.ws), 3, 1) == E
        refused(p.encode() + b"_dev_async", b"z overlaps the workspace")
    assert start(rtol=-1.0) == E and start(rtol=float("nan")) == E
    refused(b"start_dev_async", b"rtol")
    assert start(mi=0) == E
    refused(b"start_dev_async", b"max_iter")
    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    assert L.ctd_kkt_minres_shard_info(h._h, None, 3, C.byref(info)) == E
    refused(b"info", b"ws")
    # the whole-grid solve on a shard handle: refused as before
    full = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, x=s.x.data_ptr())
    assert L.ctd_kkt_minres_dev(h._h, C.byref(full), V(s.rhs), V(z), 1e-10, 10, 2, C.byref(info)) == E
    assert b"no shard form" in L.ctd_last_error(h._h)
    # and the good call goes through
    assert start() == 0
    h.sync()
    assert not bool((z == 7.0).all())


# ---- 10. ShardedDOCP.kkt_minres with world = 1 ------------------------------------------------------------------------------------
def test_sharded_docp_with_one_rank(torch_cuda):
    torch = torch_cuda
    prob, sch, N = "goddard", "trapeze", 7
    s = Case(torch, prob, sch, N)
    sd = cdist.ShardedDOCP(lambda steps: ct.DOCP(prob, N, sch, device=0, pattern="structural", steps=steps), N, world=1, rank=0)
    for kw in (dict(rtol=0.0, max_iter=5), dict(rtol=1e-10, max_iter=10 * s.n)):
        zw, iw = s.whole(True, **kw)
        z, info = sd.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=s.pre(True), **kw)
        assert info == iw and torch.equal(z, zw), kw
    pair = sd.kkt_diag_precond(s.x, s.y, 1.0, s.sx, s.sc)
    za, ia = sd.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond=pair, rtol=1e-10, max_iter=10 * s.n)
    za = za.clone()
    zb, ib = sd.kkt_minres(s.x, s.y, s.rhs, sx=s.sx, sc=s.sc, precond="diag", rtol=1e-10, max_iter=10 * s.n)
    assert ia == ib and ia.status == "converged" and torch.equal(za, zb)
    sd.close()
    s.close()
