"""The matrix-free KKT diagonals on time-step shards on the MI355X (ctd_hdiag_shard_dev_async, ctd_jsq_rows_shard_dev_async,
ctd_jsq_cols_shard_dev_async; DOCP.hdiag_shard / jsq_rows_shard / jsq_cols_shard; ShardedDOCP.hdiag / jsq_rows / jsq_cols /
kkt_diag_precond).

In the manner of test_gpu_kktprod_shard.py, with the cases, sizes and Shards helper of test_gpu_products_shard.py: three shard handles
of one process on device 0 beside a handle of the whole grid.  Every input a shard is given holds exactly the read set
include/ctdirect_hip.h documents and NaN everywhere else -- x the variable-layout set (in place: its own entries and v), y and wc the
constraint-layout set, wx the variable-layout set -- and the outputs are pre-filled with 777.0.  Checked: no NaN comes out and a shard
writes its write set only; the composed jsq_rows and the composed hdiag / jsq_cols below v_off are BIT-IDENTICAL to the whole-grid
handle's; the composed vectors, the v entries summed over the shards, meet the bars of test_gpu_diag.py (hdiag_ref, jsq_ref) against
the oracle (a run-time OCP: against its own handle's assembled blocks; where the oracle's Hessian pattern drops nonzeros: hdiag against
hprod of the whole-grid handle, as check_hdiag does); a second call gives the same bits; the halo-copied mode gives the bits of the
in-place mode; and all of it again with y / the weights None.  No tolerance of its own: the bars are those helpers'.  Also: a
whole-grid handle, graph capture, the refusals, the sharded preconditioner through scipy's minres in one process, and two ranks on one
GPU over gloo."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe
from jit_defs import twin
from test_gpu_diag import (Inputs, asm_precond, assert_block, dev, handle_refs, hdiag_ref, jsq_ref, minres_case, oracle_refs,
                           run_minres)
from test_gpu_products_shard import CASES, SIZES, Shards

pytestmark = pytest.mark.gpu
SIGMA = 0.7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class DiagShards(Shards):
    """Shards with the inputs, the calls and the references of the three diagonals.  The iterate of a run-time OCP is the one
    test_gpu_diag.py gives the expression twins (bench_inputs), not Shards' uniform one: at r = 0.2 Goddard's drag exp(-500 (r - 1))
    puts entries of 1e174 into J, fine for a product but inf once squared, in the result and in the reference alike."""
    OPS = ("hdiag", "jsq_rows", "jsq_cols")

    def __init__(self, torch, prob, sch, *a):
        super().__init__(torch, prob, sch, *a)
        if self.rt:
            self.x = bench_inputs(describe(self.full, prob, sch), perturb=1e-3)
            self.xd = torch.from_numpy(self.x).cuda()
        self.k = Inputs(self.nvar, self.ncon)
        self._refs = {}

    def new(self, op):
        return self.torch.full((self.ncon if op == "jsq_rows" else self.nvar,), 777.0, dtype=self.torch.float64, device="cuda")

    def call(self, j, op, full_args, out, sync=True):
        """shard j's call of `op`; full_args False: y / the weights are None"""
        h, w = self.hs[j], self.k
        if op == "hdiag":
            return h.hdiag_shard(self.xs[j], self.masked(w.y, self.con[j][1]) if full_args else None, SIGMA, out=out, sync=sync)
        if op == "jsq_rows":
            return h.jsq_rows_shard(self.xs[j], self.masked(w.wx, self.var[j][1]) if full_args else None, out=out, sync=sync)
        return h.jsq_cols_shard(self.xs[j], self.masked(w.wc, self.con[j][1]) if full_args else None, out=out, sync=sync)

    def run_diag(self, full_args, ops=OPS):
        """{op: [out_0, out_1, out_2]}"""
        return {op: [self.call(j, op, full_args, self.new(op)) for j in range(3)] for op in ops}

    def compose_diag(self, op, outs):
        """write sets only; the pieces cover everything; the v entries of hdiag / jsq_cols are the sum of the three partials"""
        rows = op == "jsq_rows"
        own = [(self.con if rows else self.var)[j][0] for j in range(3)]
        comp = np.full(self.ncon if rows else self.nvar, 777.0)
        tail = np.zeros(self.nv)
        for j in range(3):
            o = outs[j].cpu().numpy()
            assert not np.isnan(o).any(), (op, j, "NaN")
            assert (o[~own[j]] == 777.0).all(), (op, j, "written outside its write set")
            body = own[j].copy()
            if not rows:
                body[self.v_off:] = False
                tail += o[self.v_off:]
            comp[body] = o[body]
        if not rows:
            comp[self.v_off:] = tail
        assert not (comp == 777.0).any(), op
        return comp

    def whole_diag(self, op, full_args):
        d, w = self.full, self.k
        y, wx, wc = dev(self.torch, *((w.y, w.wx, w.wc) if full_args else (None, None, None)))
        if op == "hdiag":
            return d.hdiag(self.xd, y, obj_weight=SIGMA).cpu().numpy()
        return (d.jsq_rows(self.xd, wx) if op == "jsq_rows" else d.jsq_cols(self.xd, wc)).cpu().numpy()

    def refs(self, full_args):
        """(H, J) by the rules of test_gpu_diag.py, computed once per argument set"""
        if full_args not in self._refs:
            y = self.k.y if full_args else np.zeros(self.ncon)
            self._refs[full_args] = (handle_refs(self.torch, self.full, self.x, y, SIGMA) if self.rt
                                     else oracle_refs(self.o, self.x, y, SIGMA))
        return self._refs[full_args]

    def check_reference(self, op, comp, full_args, what):
        H, J = self.refs(full_args)
        w = self.k
        if op != "hdiag":
            rref, rbar, cref, cbar = jsq_ref(*J, w.wx if full_args else None, w.wc if full_args else None, self.nvar, self.ncon)
            ref, bar = (rref, rbar) if op == "jsq_rows" else (cref, cbar)
            assert_block(comp, ref, bar, what)
            return
        hr, hc, vals, mag, dropped = H
        ref, bar = hdiag_ref(hr, hc, vals, mag, self.nvar)
        if not dropped:
            assert_block(comp, ref, bar, what)
            return
        # the hprod-based check of test_gpu_diag.check_hdiag on the composed vector
        torch, d, nvar = self.torch, self.full, self.nvar
        if self.N <= 7:
            idx = np.arange(nvar)
        else:
            n, blk = d.dims.NLP_x, d.discretization._step_variables_block
            cand = np.r_[np.arange(min(blk, 20)), np.arange(nvar - self.nv - n, nvar), np.random.default_rng(9).integers(0, nvar, 64)]
            idx = np.array(list(dict.fromkeys(int(j) for j in cand))[:64])
        yd = dev(torch, w.y if full_args else None)[0]
        vd = torch.zeros(nvar, dtype=torch.float64, device="cuda")
        ref = np.zeros(nvar)
        for j in idx:
            vd.zero_()
            vd[j] = 1.0
            ref[j] = float(d.hprod(self.xd, yd, vd, obj_weight=SIGMA)[j])
        mask = np.zeros(nvar, dtype=bool)
        mask[idx] = True
        assert_block(comp, ref, bar, what + ("vs hprod",), mask)


def compose_checks(torch, s, case_id, ops):
    """everything test 1 asserts, for the calls `ops`"""
    for full_args in (True, False):
        what = (case_id, s.N, "all arguments" if full_args else "y / weights None")
        s.bind(in_place=True)
        in_place = s.run_diag(full_args, ops)
        again = s.run_diag(full_args, ops)
        for op in ops:
            for j in range(3):
                assert torch.equal(again[op][j], in_place[op][j]), what + (op, j, "a second call differs")
        for op in ops:
            comp = s.compose_diag(op, in_place[op])
            whole = s.whole_diag(op, full_args)
            body = s.ncon if op == "jsq_rows" else s.v_off
            assert np.array_equal(comp[:body], whole[:body]), what + (op, "not the bits of the whole-grid call")
            s.check_reference(op, comp, full_args, what + (op,))
        s.bind(in_place=False)
        copied = s.run_diag(full_args, ops)
        for op in ops:
            for j in range(3):
                assert torch.equal(copied[op][j], in_place[op][j]), what + (op, j, "halo-copied mode differs from the in-place mode")


# ---- 1. three shards compose the whole grid --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,cuts", SIZES, ids=["one_step_shards", "N700"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_shards_compose_the_whole_grid_diagonals(torch_cuda, case, N, cuts):
    _, prob, sch, cs, grid, rt = case
    s = DiagShards(torch_cuda, prob, sch, cs, grid, rt, N, cuts)
    compose_checks(torch_cuda, s, case[0], DiagShards.OPS)
    s.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_jsq_rows_two_workgroups_and_a_one_step_shard_between(torch_cuda, case):
    """N = 700, cuts (0, 300, 301, 700): at one lane per node the smallest shape where a shard spans two workgroups and a one-step
    shard sits between two others (the thirds of 700 all fit in one 256-lane workgroup)"""
    _, prob, sch, cs, grid, rt = case
    s = DiagShards(torch_cuda, prob, sch, cs, grid, rt, 700, (0, 300, 301, 700))
    compose_checks(torch_cuda, s, case[0], ("jsq_rows",))
    s.close()


# ---- 2. a whole-grid handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch,rt", [("goddard_all", "trapeze", False), ("quadrotor12", "gauss_legendre_3", False),
                                         ("double_integrator_path", "euler_implicit", False), ("goddard_all", "midpoint", True)])
def test_whole_grid_handle_and_reproducibility(torch_cuda, prob, sch, rt):
    """on a handle of the whole grid every shard call gives the bits of its *_dev_async counterpart, the v entries included; twice"""
    torch = torch_cuda
    d = ct.DOCP(twin(prob) if rt else prob, 300, sch, device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    w = Inputs(nvar, ncon)
    y, wx, wc = dev(torch, w.y, w.wx, w.wc)
    new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")      # noqa: E731
    for _ in range(2):
        for yy, wxx, wcc in ((y, wx, wc), (None, None, None)):
            assert torch.equal(d.hdiag_shard(x, yy, SIGMA, out=new(nvar), sync=True), d.hdiag(x, yy, obj_weight=SIGMA))
            assert torch.equal(d.jsq_rows_shard(x, wxx, out=new(ncon), sync=True), d.jsq_rows(x, wxx))
            assert torch.equal(d.jsq_cols_shard(x, wcc, out=new(nvar), sync=True), d.jsq_cols(x, wcc))
    d.close()


# ---- 3. graph capture ------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_shard_calls(torch_cuda):
    """the middle shard of three, its iterate read in place: one warm call of each on the capturing stream, then the three captured
    together and replayed"""
    torch = torch_cuda
    s = DiagShards(torch, "goddard_all", "trapeze", 1, False, False, 200, (0, 66, 135, 200))
    s.bind(in_place=True)
    want = {op: outs[1] for op, outs in s.run_diag(True).items()}
    h, w = s.hs[1], s.k
    yk, wxk, wck = s.masked(w.y, s.con[1][1]), s.masked(w.wx, s.var[1][1]), s.masked(w.wc, s.con[1][1])
    outs = {op: s.new(op) for op in DiagShards.OPS}

    def enqueue():
        h.hdiag_shard(s.xs[1], yk, SIGMA, out=outs["hdiag"])
        h.jsq_rows_shard(s.xs[1], wxk, out=outs["jsq_rows"])
        h.jsq_cols_shard(s.xs[1], wck, out=outs["jsq_cols"])

    st = torch.cuda.Stream()
    h.set_stream(st)
    with torch.cuda.stream(st):
        enqueue()
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        enqueue()
    for o in outs.values():
        o.fill_(777.0)
    g.replay()
    torch.cuda.synchronize()
    for op, o in outs.items():
        assert torch.equal(o, want[op]), op
    s.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    E = ct._lib.CTD_EINVAL
    d = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(5, 12))
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    x, wx, ov = t(nvar, 1.0), t(nvar, 0.5), t(nvar, 7.0)
    y, oc = t(ncon, 1.0), t(ncon, 7.0)
    P = lambda a: None if a is None else C.c_void_p(a.data_ptr())        # noqa: E731
    # name: (the shard call, its whole-grid counterpart, the optional input, the output)
    calls = {"hdiag": (lambda x_, a, o: L.ctd_hdiag_shard_dev_async(d._h, P(x_), P(a), 1.0, P(o)),
                       lambda x_, a, o: L.ctd_hdiag_dev_async(d._h, P(x_), P(a), 1.0, P(o)), y, ov),
             "jsq_rows": (lambda x_, a, o: L.ctd_jsq_rows_shard_dev_async(d._h, P(x_), P(a), P(o)),
                          lambda x_, a, o: L.ctd_jsq_rows_dev_async(d._h, P(x_), P(a), P(o)), wx, oc),
             "jsq_cols": (lambda x_, a, o: L.ctd_jsq_cols_shard_dev_async(d._h, P(x_), P(a), P(o)),
                          lambda x_, a, o: L.ctd_jsq_cols_dev_async(d._h, P(x_), P(a), P(o)), y, ov)}

    def untouched():
        d.sync()
        return bool((ov == 7.0).all()) and bool((oc == 7.0).all())

    for name, (fn, whole, a, o) in calls.items():
        for args in ((None, a, o), (x, a, None)):
            assert fn(*args) == E, name
            assert b"null" in L.ctd_last_error(d._h), name
            assert untouched(), name
        for args, keep in (((x, a, x), x), ((x, a, a), a)):
            before = keep.clone()
            assert fn(*args) == E, name
            assert b"input" in L.ctd_last_error(d._h), name
            d.sync()
            assert torch.equal(keep, before) and untouched(), name
        # the whole-grid entry point still refuses the shard handle
        assert whole(x, a, o) == E, name
        err = L.ctd_last_error(d._h)
        assert b"shard" in err and b"out of scope" in err, name
        assert untouched(), name
    # the optional input may be NULL
    for name, (fn, whole, a, o) in calls.items():
        assert fn(x, None, o) == 0, name
    d.sync()
    assert not untouched()
    d.close()


# ---- 5. the sharded preconditioner, one process ----------------------------------------------------------------------------------
def test_sharded_preconditioner_through_minres(torch_cuda):
    """test_gpu_diag.py::test_preconditioned_minres_through_the_operators on three shard handles, cuts (0, 7, 13, 20): the same
    transcription and inputs (minres_case(): Goddard, trapeze, N = 20, seed 21).  K is applied as three kktprod_shard calls; (px, pc)
    comes from three hdiag_shard and three jsq_rows_shard calls composed on the host by the recipe of
    ShardedDOCP.kkt_diag_precond, a plain sum standing in for the all-reduce.  Asserted: px has the bits of DOCP.kkt_diag_precond
    below v_off, its v entry and all of pc agree within the hdiag_ref / jsq_ref bars; and the conditions of that test -- info == 0,
    at most half the plain run's iterations, a true residual under K_asm no larger than the plain run's, the iteration count (+-2)
    of the run whose M comes from K_asm's own diagonals.  The CPU-established margin on these inputs, from that test's docstring:
    plain 313 iterations, preconditioned 72 -- a factor of 4.3 where 2 is asked."""
    torch = torch_cuda
    c = minres_case()
    nvar, ncon, n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
    cuts, floor = (0, 7, 13, 20), 1e-8
    hs = [ct.DOCP(c["prob"], c["N"], c["sch"], device=0, pattern="structural", steps=(cuts[j], cuts[j + 1])) for j in range(3)]
    full = ct.DOCP(c["prob"], c["N"], c["sch"], device=0, pattern="structural")
    assert (full.dim_NLP_variables, full.dim_NLP_constraints) == (nvar, ncon)
    nv = full.dims.NLP_v
    v_off = nvar - nv
    assert nv > 0
    disc = full.discretization
    blk, cb = disc._step_variables_block, disc._state_stage_eqs_block + disc._step_pathcons_block
    own_x = [slice(cuts[j] * blk, cuts[j + 1] * blk if j < 2 else v_off) for j in range(3)]
    own_c = [slice(cuts[j] * cb, cuts[j + 1] * cb if j < 2 else ncon) for j in range(3)]
    xd, yd, sxd, scd = dev(torch, c["x"], c["y"], c["sx"], c["sc"])
    zin = torch.empty(n, dtype=torch.float64, device="cuda")
    zout = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3)]

    def matvec(z):
        zin.copy_(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64).ravel()))
        out = np.zeros(n)
        for j, h in enumerate(hs):
            h.kktprod_shard(xd, yd, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=sxd, sc=scd, out=(zout[j][:nvar], zout[j][nvar:]),
                            sync=True)
            piece = zout[j].cpu().numpy()
            out[:nvar][own_x[j]] = piece[:nvar][own_x[j]]
            out[v_off:nvar] += piece[v_off:nvar]
            out[nvar:][own_c[j]] = piece[nvar:][own_c[j]]
        return out

    # the recipe of ShardedDOCP.kkt_diag_precond on the host
    px = np.zeros(nvar)
    for j, h in enumerate(hs):
        hd = h.hdiag_shard(xd, yd, 1.0, sync=True).cpu().numpy()
        px[own_x[j]] = hd[own_x[j]] + c["sx"][own_x[j]]
        part = hd[v_off:]
        if j == 2:
            part = part + c["sx"][v_off:]
        px[v_off:] += part
    px = np.maximum(np.abs(px), floor)
    wxd = torch.from_numpy(1.0 / px).cuda()
    pc = np.zeros(ncon)
    for j, h in enumerate(hs):
        pc[own_c[j]] = h.jsq_rows_shard(xd, wxd, sync=True).cpu().numpy()[own_c[j]] + c["sc"][own_c[j]]
    wpx, wpc = (t.cpu().numpy() for t in full.kkt_diag_precond(xd, yd, obj_weight=1.0, sx=sxd, sc=scd))
    assert np.array_equal(px[:v_off], wpx[:v_off]), "px: not the bits of DOCP.kkt_diag_precond"
    H, J = oracle_refs(_oracle(c), c["x"], c["y"], 1.0)
    _, hbar = hdiag_ref(H[0], H[1], H[2], H[3], nvar)
    assert_block(px, wpx, hbar, ("px", "v entries"), np.arange(nvar) >= v_off)
    _, rbar, _, _ = jsq_ref(*J, 1.0 / wpx, None, nvar, ncon)
    assert_block(pc, wpc, rbar, ("pc",))
    assert (px > 0).all() and (pc > 0).all()

    def diag_op(qx, qc):
        m = 1.0 / np.r_[qx, qc]
        return LinearOperator((n, n), matvec=lambda v: m * np.asarray(v).ravel(), dtype=np.float64)

    K = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
    cap = 10 * n
    nrm = np.linalg.norm(c["rhs"])
    z0, info0, it0 = run_minres(K, c["rhs"], None, cap)
    z1, info1, it1 = run_minres(K, c["rhs"], diag_op(px, pc), cap)
    _, info2, it2 = run_minres(K, c["rhs"], diag_op(*asm_precond(c)), cap)
    res0 = float(np.linalg.norm(c["K_asm"] @ z0 - c["rhs"]) / nrm)
    res1 = float(np.linalg.norm(c["K_asm"] @ z1 - c["rhs"]) / nrm)
    print("plain: info", info0, "iterations", it0, "residual", res0, "| preconditioned: info", info1, "iterations", it1,
          "residual", res1, "| M from K_asm: info", info2, "iterations", it2)
    assert info1 == 0, info1
    assert 2 * it1 <= it0, (it1, it0)
    assert res1 <= res0, (res1, res0)
    assert abs(it1 - it2) <= 2, (it1, it2)
    for h in hs + [full]:
        h.close()


def _oracle(c):
    from oracle.oracle import OracleDOCP
    o = OracleDOCP(c["prob"], c["sch"], c["N"])
    o.set_pattern_mode(1)
    return o


# ---- 6. two ranks on one GPU over gloo -------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    """every input holds this rank's own entries (x, wx: + the nv tail; sx: the tail on the last rank only), NaN elsewhere; the
    iterate's halo is copied in by the calls themselves.  Reports a list of failures (empty: all held)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        import ctdirect_jl_amd as ct_
        from ctdirect_jl_amd import dist as ctdist
        from oracle.oracle import OracleDOCP
        torch.cuda.set_device(0)
        prob, sch, N = "goddard_all", "trapeze", 20
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(o, prob, sch), perturb=1e-3)
        make = lambda steps=None: ct_.DOCP(prob, N, sch, device=0, steps=steps, pattern="structural")     # noqa: E731
        sh = ctdist.ShardedDOCP(make, N, world=world, rank=rank)
        full = make()
        d = sh.docp
        nvar, ncon, nv = d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v
        v_off = nvar - nv
        last = rank == world - 1
        w = Inputs(nvar, ncon)
        r = np.random.default_rng(21)
        sx, sc = 10.0 ** r.uniform(-3.0, 5.0, nvar) + 50.0, 1e-2 * r.uniform(1.0, 2.0, ncon)
        a, b = sh.owned_variables()
        r0, r1 = sh.owned_constraints()
        own_x = np.zeros(nvar, dtype=bool)
        own_x[a:b] = True
        own_c = np.zeros(ncon, dtype=bool)
        own_c[r0:r1] = True
        tail = np.arange(nvar) >= v_off
        mine = lambda full_, mask: torch.from_numpy(np.where(mask, full_, np.nan)).cuda()        # noqa: E731
        new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")              # noqa: E731
        xd, yd, wxd, wcd, sxd, scd = dev(torch, x, w.y, w.wx, w.wc, sx, sc)
        H, J = oracle_refs(o, x, w.y, SIGMA)
        _, hbar = hdiag_ref(H[0], H[1], H[2], H[3], nvar)
        _, _, _, cbar = jsq_ref(*J, w.wx, w.wc, nvar, ncon)
        bad = []

        def check(name, got, ref, own, bar=None):
            """own entries: the whole-grid handle's bits; the tail (bar given): within the bar"""
            got, ref = got.cpu().numpy(), ref.cpu().numpy()
            if not np.array_equal(got[own], ref[own]):
                j = int(np.flatnonzero(own & ~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0])
                bad.append((name, "own entries differ from the whole-grid handle's", j, float(got[j]), float(ref[j])))
            if bar is not None:
                err = np.abs(got[tail] - ref[tail])
                if not (np.isfinite(err).all() and (err <= bar[tail]).all()):
                    bad.append((name, "v entries", err.tolist(), bar[tail].tolist()))

        # the whole-grid handle's references first; the device is idle before and after every sharded call, so a failure below is
        # a value, never an ordering between the two handles
        ref = dict(hdiag=full.hdiag(xd, yd, obj_weight=SIGMA), jsq_cols=full.jsq_cols(xd, wcd), jsq_rows=full.jsq_rows(xd, wxd))
        wpx, wpc = full.kkt_diag_precond(xd, yd, obj_weight=SIGMA, sx=sxd, sc=scd)
        torch.cuda.synchronize()

        def done(out):
            torch.cuda.synchronize()
            return out

        xs = mine(x, own_x | tail)
        check("hdiag", done(sh.hdiag(xs, mine(w.y, own_c), SIGMA, new(nvar))), ref["hdiag"], own_x, hbar)
        # (x's halo is in xs now: it does not change between the calls of one outer iteration)
        check("jsq_cols", done(sh.jsq_cols(xs, mine(w.wc, own_c), new(nvar), x_halo_valid=True)), ref["jsq_cols"], own_x, cbar)
        check("jsq_rows", done(sh.jsq_rows(xs, mine(w.wx, own_x | tail), new(ncon), x_halo_valid=True)), ref["jsq_rows"], own_c)
        xs = mine(x, own_x | tail)
        px, pc = done(sh.kkt_diag_precond(xs, mine(w.y, own_c), obj_weight=SIGMA, sx=mine(sx, own_x | (tail & last)),
                                          sc=mine(sc, own_c)))
        check("px", px, wpx, own_x, hbar)
        _, rbar, _, _ = jsq_ref(*J, 1.0 / wpx.cpu().numpy(), None, nvar, ncon)
        gpc, rpc = pc.cpu().numpy(), wpc.cpu().numpy()
        err = np.where(own_c, np.abs(gpc - rpc), 0.0)
        if not (np.isfinite(err).all() and (err <= rbar).all()):
            j = int(np.argmax(~(err <= rbar)))
            bad.append(("pc", j, float(gpc[j]), float(rpc[j]), float(rbar[j])))
        torch.cuda.synchronize()
        q.put((rank, bad))
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_sharded_diagonals_and_preconditioner(torch_cuda):
    """Goddard-all, trapeze, N = 20, two ranks on one GPU over gloo, the iterate halo-copied: ShardedDOCP.hdiag / jsq_cols / jsq_rows
    and kkt_diag_precond give, on each rank's own entries and the replicated tail, the whole-grid handle's values -- bit-identical
    where no v partial enters (own entries of hdiag, jsq_cols, jsq_rows and px), within the hdiag_ref / jsq_ref bars otherwise (the
    v entries; pc, which reads 1 / px of the v entries)"""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(bad == [] for _, bad in res), res
