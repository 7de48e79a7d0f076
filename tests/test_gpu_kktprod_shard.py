"""The fused KKT product on time-step shards on the MI355X (ctd_kktprod_shard_dev_async, DOCP.kktprod_shard).

In the manner of test_gpu_products_shard.py, whose cases, sizes and Shards helper this file uses: three shard handles of one process
on device 0 beside a handle of the whole grid.  Every input a shard is given holds exactly the read set include/ctdirect_hip.h
documents and NaN everywhere else -- x, dx the variable-layout set, y, dy the constraint-layout set, sx the shard's own variable
entries (the nv tail on the last shard only), sc its own rows -- and the outputs are pre-filled with 777.0.  Checked: no NaN comes out
and a shard writes its write set only; the composed rc and the composed rx below v_off are BIT-IDENTICAL to DOCP.kktprod on the
whole-grid handle; the composed vectors, the v entries summed over the shards, meet the rx / rc bars of test_gpu_kktprod.py against
the oracle (a run-time OCP: against its own handle's assembled blocks; where the oracle's Hessian pattern drops nonzeros: the top
block against hprod + jtprod + sx o dx of the whole-grid handle); a second call gives the same bits; the halo-copied mode gives the
bits of the in-place mode; and all of it again with y, sx and sc None.  Also: a whole-grid handle, graph capture, the refusals, and
scipy's minres through three shard calls."""
import ctypes as C
import types

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe
from jit_defs import twin
from oracle.oracle import OracleDOCP
from test_gpu_kktprod import Inputs, assert_block, csc_coo, handle_blocks, oracle_blocks
from test_gpu_products_shard import CASES, SIZES, Shards

pytestmark = pytest.mark.gpu
SIGMA = 0.7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class KktShards(Shards):
    """Shards with the inputs, the read / write sets and the references of the KKT product"""

    def __init__(self, *a):
        super().__init__(*a)
        self.k = Inputs(self.nvar, self.ncon)
        # sx: own variable entries, the nv tail on the last shard only; sc: own rows
        self.sx_set = []
        for j in range(3):
            m = self.var[j][0].copy()
            m[self.v_off:] = j == 2
            self.sx_set.append(m)

    def run_kkt(self, full_args):
        """the three shard calls: [(rx_k, rc_k)]; full_args False: y, sx and sc are None"""
        torch, w, outs = self.torch, self.k, []
        for j, h in enumerate(self.hs):
            rx = torch.full((self.nvar,), 777.0, dtype=torch.float64, device="cuda")
            rc = torch.full((self.ncon,), 777.0, dtype=torch.float64, device="cuda")
            y = self.masked(w.y, self.con[j][1]) if full_args else None
            sx = self.masked(w.sx, self.sx_set[j]) if full_args else None
            sc = self.masked(w.sc, self.con[j][0]) if full_args else None
            h.kktprod_shard(self.xs[j], y, self.masked(w.dx, self.var[j][1]), self.masked(w.dy, self.con[j][1]), obj_weight=SIGMA,
                            sx=sx, sc=sc, out=(rx, rc), sync=True)
            outs.append((rx, rc))
        return outs

    def compose_kkt(self, outs):
        """write sets only; the pieces cover everything; the v entries of rx are the sum of the three partials"""
        rx, rc = np.full(self.nvar, 777.0), np.full(self.ncon, 777.0)
        tail = np.zeros(self.nv)
        for j in range(3):
            ox, oc = outs[j][0].cpu().numpy(), outs[j][1].cpu().numpy()
            assert not np.isnan(ox).any() and not np.isnan(oc).any(), (j, "NaN")
            assert (ox[~self.var[j][0]] == 777.0).all(), (j, "rx written outside its write set")
            assert (oc[~self.con[j][0]] == 777.0).all(), (j, "rc written outside its write set")
            body = self.var[j][0].copy()
            body[self.v_off:] = False
            rx[body] = ox[body]
            tail += ox[self.v_off:]
            rc[self.con[j][0]] = oc[self.con[j][0]]
        rx[self.v_off:] = tail
        assert not (rx == 777.0).any() and not (rc == 777.0).any()
        return rx, rc

    def whole_kkt(self, full_args):
        torch, w = self.torch, self.k
        t = lambda a: torch.from_numpy(a).cuda()        # noqa: E731
        rx, rc = self.full.kktprod(self.xd, t(w.y) if full_args else None, t(w.dx), t(w.dy), obj_weight=SIGMA,
                                   sx=t(w.sx) if full_args else None, sc=t(w.sc) if full_args else None)
        return rx.cpu().numpy(), rc.cpu().numpy()

    def reference(self, full_args):
        """(rx_ref, rx_bar, rc_ref, rc_bar) by the rules of test_gpu_kktprod.py"""
        w, d = self.k, self.full
        y, sx, sc = (w.y, w.sx, w.sc) if full_args else (None, None, None)
        if self.rt:
            wk = types.SimpleNamespace(dx=w.dx, dy=w.dy, sx=sx, sc=sc)
            return handle_blocks(self.torch, d, self.x, np.zeros(self.ncon) if y is None else y, SIGMA, wk)
        rx_ref, rx_bar, rc_ref, rc_bar, dropped = oracle_blocks(self.o, self.x, y, SIGMA, w.dx, w.dy, sx, sc)
        if dropped:
            z = np.zeros(self.nvar) if sx is None else sx
            rx_ref = d.hprod(self.x, y, w.dx, obj_weight=SIGMA) + d.jtprod(self.x, w.dy) + z * w.dx
        return rx_ref, rx_bar, rc_ref, rc_bar


@pytest.mark.parametrize("N,cuts", SIZES, ids=["one_step_shards", "N700"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_shards_compose_the_whole_grid_kkt_product(torch_cuda, case, N, cuts):
    _, prob, sch, cs, grid, rt = case
    s = KktShards(torch_cuda, prob, sch, cs, grid, rt, N, cuts)
    for full_args in (True, False):
        what = (case[0], N, "all arguments" if full_args else "y, sx, sc None")
        s.bind(in_place=True)
        in_place = s.run_kkt(full_args)
        for j, (rx, rc) in enumerate(s.run_kkt(full_args)):
            assert torch_cuda.equal(rx, in_place[j][0]) and torch_cuda.equal(rc, in_place[j][1]), what + (j, "a second call differs")
        rx, rc = s.compose_kkt(in_place)
        wx, wc = s.whole_kkt(full_args)
        assert np.array_equal(rc, wc), what + ("rc: not the bits of the whole-grid call",)
        assert np.array_equal(rx[:s.v_off], wx[:s.v_off]), what + ("rx: not the bits of the whole-grid call",)
        rx_ref, rx_bar, rc_ref, rc_bar = s.reference(full_args)
        assert_block(rc, rc_ref, rc_bar, what + ("rc",))
        assert_block(rx, rx_ref, rx_bar, what + ("rx",))
        s.bind(in_place=False)
        for j, (rx, rc) in enumerate(s.run_kkt(full_args)):
            assert torch_cuda.equal(rx, in_place[j][0]) and torch_cuda.equal(rc, in_place[j][1]), \
                what + (j, "halo-copied mode differs from the in-place mode")
    s.close()


@pytest.mark.parametrize("prob,sch,rt", [("goddard_all", "trapeze", False), ("quadrotor12", "gauss_legendre_3", False),
                                         ("double_integrator_path", "euler_implicit", False), ("goddard_all", "midpoint", True)])
def test_whole_grid_handle_and_reproducibility(torch_cuda, prob, sch, rt):
    """on a handle of the whole grid the shard call gives the bits of ctd_kktprod_dev_async, the v entries included; twice"""
    torch = torch_cuda
    d = ct.DOCP(twin(prob) if rt else prob, 300, sch, device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    w = Inputs(nvar, ncon)
    y, dx, dy, sx, sc = (torch.from_numpy(a).cuda() for a in (w.y, w.dx, w.dy, w.sx, w.sc))
    new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")      # noqa: E731
    for _ in range(2):
        for yy, sxx, scc in ((y, sx, sc), (None, None, None)):
            rx, rc = d.kktprod_shard(x, yy, dx, dy, obj_weight=SIGMA, sx=sxx, sc=scc, out=(new(nvar), new(ncon)), sync=True)
            wx, wc = d.kktprod(x, yy, dx, dy, obj_weight=SIGMA, sx=sxx, sc=scc)
            assert torch.equal(rx, wx) and torch.equal(rc, wc)
    d.close()


def test_graph_capture_of_the_shard_call(torch_cuda):
    """the middle shard of three, its iterate read in place: one warm call on the capturing stream, then captured and replayed"""
    torch = torch_cuda
    s = KktShards(torch, "goddard_all", "trapeze", 1, False, False, 200, (0, 66, 135, 200))
    s.bind(in_place=True)
    want = s.run_kkt(True)[1]
    h, w = s.hs[1], s.k
    args = (s.xs[1], s.masked(w.y, s.con[1][1]), s.masked(w.dx, s.var[1][1]), s.masked(w.dy, s.con[1][1]))
    sx, sc = s.masked(w.sx, s.sx_set[1]), s.masked(w.sc, s.con[1][0])
    rx = torch.full((s.nvar,), 777.0, dtype=torch.float64, device="cuda")
    rc = torch.full((s.ncon,), 777.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    h.set_stream(st)
    with torch.cuda.stream(st):
        h.kktprod_shard(*args, obj_weight=SIGMA, sx=sx, sc=sc, out=(rx, rc))
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        h.kktprod_shard(*args, obj_weight=SIGMA, sx=sx, sc=sc, out=(rx, rc))
    rx.fill_(777.0)
    rc.fill_(777.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rx, want[0]) and torch.equal(rc, want[1])
    s.close()


def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    E = ct._lib.CTD_EINVAL
    d = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(5, 12))
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    x, dx, sx, rx = t(nvar, 1.0), t(nvar, 0.5), t(nvar, 0.25), t(nvar, 7.0)
    y, dy, sc, rc = t(ncon, 1.0), t(ncon, 0.5), t(ncon, 0.25), t(ncon, 7.0)
    P = lambda a: C.c_void_p(a.data_ptr())        # noqa: E731
    good = dict(x=x, y=y, dx=dx, dy=dy, sx=sx, sc=sc, rx=rx, rc=rc)

    def call(fn, **kw):
        a = dict(good)
        a.update(kw)
        p = {k: (None if v is None else P(v)) for k, v in a.items()}
        return fn(d._h, p["x"], p["y"], 1.0, p["dx"], p["dy"], p["sx"], p["sc"], p["rx"], p["rc"])

    def untouched():
        d.sync()
        return bool((rx == 7.0).all()) and bool((rc == 7.0).all())

    fn = L.ctd_kktprod_shard_dev_async
    for name in ("x", "dx", "dy", "rx", "rc"):
        assert call(fn, **{name: None}) == E, name
        assert b"null" in L.ctd_last_error(d._h), name
        assert untouched(), name
    for out in ("rx", "rc"):
        for inp in ("x", "y", "dx", "dy", "sx", "sc"):
            before = good[inp].clone()
            assert call(fn, **{out: good[inp]}) == E, (out, inp)
            assert b"input" in L.ctd_last_error(d._h), (out, inp)
            d.sync()
            assert torch.equal(good[inp], before) and untouched(), (out, inp)
    assert call(fn, rc=rx) == E
    assert b"rx and rc" in L.ctd_last_error(d._h)
    assert untouched()
    # the whole-grid entry point still refuses the shard handle, and names the shard call
    assert call(L.ctd_kktprod_dev_async) == E
    assert b"ctd_kktprod_shard_dev_async" in L.ctd_last_error(d._h)
    assert untouched()
    # the optional ones may be NULL
    assert call(fn, y=None, sx=None, sc=None) == 0
    d.sync()
    assert not untouched()
    d.close()


def test_minres_through_three_shard_calls(torch_cuda):
    """test_gpu_kktprod.py::test_minres_through_the_operator with the operator applied as three kktprod_shard calls, cuts
    (0, 7, 13, 20), composed on the host: the same transcription (double integrator with a path constraint, midpoint, N = 20), the
    same data (seed 21) and the same bars -- info == 0, at most 10 (nvar + ncon) iterations, |K_asm z - r| <= 1e-8 |r|.  The
    margin that docstring records was established on the CPU with K_asm itself: 47 iterations, true residual 8.7e-10 |r|.  The
    problem has nv = 0: no entry is a partial sum, and the composed operator has the bits of the whole-grid one."""
    import scipy.sparse as sp
    torch = torch_cuda
    prob, sch, N, cuts = "double_integrator_path", "midpoint", 20, (0, 7, 13, 20)
    hs = [ct.DOCP(prob, N, sch, device=0, pattern="structural", steps=(cuts[j], cuts[j + 1])) for j in range(3)]
    d = hs[0]
    assert d.dims.NLP_v == 0
    o = OracleDOCP(prob, sch, N)
    o.set_pattern_mode(1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    disc = d.discretization
    blk, cb = disc._step_variables_block, disc._state_stage_eqs_block + disc._step_pathcons_block
    own_x = [slice(cuts[j] * blk, cuts[j + 1] * blk if j < 2 else nvar) for j in range(3)]
    own_c = [slice(cuts[j] * cb, cuts[j + 1] * cb if j < 2 else ncon) for j in range(3)]
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    r = np.random.default_rng(21)
    y = r.uniform(-1.0, 1.0, ncon)
    sx, sc = 1.0 + r.uniform(0.0, 1.0, nvar), 1.0 + r.uniform(0.0, 1.0, ncon)
    rhs = r.uniform(-1.0, 1.0, nvar + ncon)
    hr, hc = csc_coo(*o.hess_pattern())
    vals, dropped = o.hess_coord(x, y, 1.0, return_dropped=True)
    assert dropped[1] == 0
    Hl = sp.csr_matrix((vals, (hr, hc)), shape=(nvar, nvar))
    jr, jc = csc_coo(*o.jac_pattern())
    J = sp.csr_matrix((o.jac_coord(x), (jr, jc)), shape=(ncon, nvar))
    K_asm = sp.bmat([[Hl + sp.tril(Hl, -1).T + sp.diags(sx), J.T], [J, -sp.diags(sc)]]).tocsr()
    xd, yd, sxd, scd = (torch.from_numpy(a).cuda() for a in (x, y, sx, sc))
    zin = torch.empty(nvar + ncon, dtype=torch.float64, device="cuda")
    zout = [torch.empty(nvar + ncon, dtype=torch.float64, device="cuda") for _ in range(3)]
    calls = [0]

    def matvec(z):
        calls[0] += 1
        zin.copy_(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64).ravel()))
        out = np.empty(nvar + ncon)
        for j, h in enumerate(hs):
            h.kktprod_shard(xd, yd, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=sxd, sc=scd, out=(zout[j][:nvar], zout[j][nvar:]),
                            sync=True)
            piece = zout[j].cpu().numpy()
            out[:nvar][own_x[j]] = piece[:nvar][own_x[j]]
            out[nvar:][own_c[j]] = piece[nvar:][own_c[j]]
        return out

    # the composed operator has the bits of the whole-grid one
    full = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    zt = torch.from_numpy(rhs).cuda()
    wx, wc = full.kktprod(xd, yd, zt[:nvar], zt[nvar:], obj_weight=1.0, sx=sxd, sc=scd)
    assert np.array_equal(matvec(rhs), np.r_[wx.cpu().numpy(), wc.cpu().numpy()])
    calls[0] = 0
    cap = 10 * (nvar + ncon)
    its = [0]
    K = LinearOperator((nvar + ncon, nvar + ncon), matvec=matvec, rmatvec=matvec, dtype=np.float64)
    z, info = minres(K, rhs, rtol=1e-10, maxiter=cap, callback=lambda zk: its.__setitem__(0, its[0] + 1))
    res = float(np.linalg.norm(K_asm @ z - rhs) / np.linalg.norm(rhs))
    print("minres info", info, "iterations", its[0], "operator calls", calls[0], "residual under K_asm", res)
    assert info == 0 and 0 < its[0] <= cap, (info, its[0], cap)
    assert res <= 1e-8, res
