"""Matrix-free products on time-step shards on the MI355X (ctd_jprod_shard_dev_async, ctd_jtprod_shard_dev_async,
ctd_hprod_shard_dev_async; DOCP.jprod_shard / jtprod_shard / hprod_shard).

In the manner of test_sharded_gradient_three_shards_through_the_c_abi: three shard handles of one process on device 0 beside a
handle of the whole grid.  Every buffer a shard is given holds exactly the read set include/ctdirect_hip.h documents and NaN
everywhere else; the outputs are pre-filled with 777.0.  Checked: a shard writes its own entries only; the three pieces compose to a
vector without 777.0 whose rows (jprod) / entries below v_off (jtprod, hprod) are BIT-IDENTICAL to the whole-grid *_dev_async result;
the composed vector, the d/dv entries summed over the shards, meets the criteria of test_gpu_products.py (|got - ref| <= 1e-12
(|J_s| |v|)_i against the oracle's structural Jacobian) and of test_gpu_hprod.py::check_against_oracle; and the halo-copied mode
(no table, x holding its read set) gives the bits of the in-place mode.  A run-time OCP is checked against its own handle's
assembled structural Jacobian / Hessian, as the run-time cases of those two files are.  Also: reproducibility, a whole-grid handle,
graph capture, the refusals."""
import ctypes as C

import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe
from jit_defs import twin
from oracle.oracle import OracleDOCP
from test_gpu_hprod import assert_close as h_assert_close
from test_gpu_hprod import RTOL as H_RTOL
from test_gpu_hprod import fd_hprod, handle_product, oracle_product, rand
from test_gpu_products import assert_close as j_assert_close
from test_gpu_products import coo_products, csc_products, directions
from shard_read_sets import constraint_read_set, variable_read_set

pytestmark = pytest.mark.gpu
SIGMA = 0.7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def user_grid(N):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(N))])
    return tg / tg[-1]


# (id, problem, scheme, control_steps, user grid, run-time OCP)
CASES = [
    ("goddard_all-trapeze", "goddard_all", "trapeze", 1, False, False),                  # final control, path rows, free tf
    ("dipath-midpoint", "double_integrator_path", "midpoint", 1, False, False),
    ("dipath-euler_implicit", "double_integrator_path", "euler_implicit", 1, False, False),
    ("difreet0tf-euler", "double_integrator_freet0tf", "euler", 1, False, False),
    ("quadrotor-gl2", "quadrotor", "gauss_legendre_2", 1, False, False),
    ("goddard-gl3", "goddard", "gauss_legendre_3", 1, False, False),
    ("goddard_all-gl2cc", "goddard_all", "gauss_legendre_2_constant_control", 1, False, False),
    ("lsq-midpoint", "least_squares_with_constraint", "midpoint", 1, False, False),
    ("goddard_all-midpoint-cs2", "goddard_all", "midpoint", 2, False, False),
    ("goddard_all-gl2-usergrid", "goddard_all", "gauss_legendre_2", 1, True, False),     # non-uniform grid, free final time
    ("goddard_all_rt-midpoint", "goddard_all", "midpoint", 1, False, True),
]
# one-step shards (both halos meet in one lane), and shards of several workgroups
SIZES = [(5, (0, 1, 2, 5)), (700, (0, 700 // 3, 2 * 700 // 3 + 1, 700))]


class Shards:
    """the whole-grid handle, three shard handles, the inputs, the references and the read / write sets of one case"""

    def __init__(self, torch, prob, sch, cs, grid, rt, N, cuts):
        self.torch, self.N, self.cuts, self.rt = torch, N, cuts, rt
        name = twin(prob) if rt else prob
        tg = user_grid(N) if grid else None
        kw = dict(time_grid=tg, device=0, pattern="structural", control_steps=cs)
        self.full = d = ct.DOCP(name, N, sch, **kw)
        self.hs = [ct.DOCP(name, N, sch, steps=(cuts[k], cuts[k + 1]), **kw) for k in range(3)]
        disc = d.discretization
        self.nvar, self.ncon, self.nv = d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v
        self.v_off = self.nvar - self.nv
        blk, eqs = disc._step_variables_block, disc._state_stage_eqs_block
        cb = eqs + disc._step_pathcons_block
        if rt:
            self.x = 0.5 + 0.3 * np.random.default_rng(11).uniform(-1.0, 1.0, self.nvar)
        else:
            self.x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        self.v, self.w = directions(self.nvar, self.ncon)
        self.y = rand(self.ncon, 4)
        self.var = [variable_read_set(cuts[k], cuts[k + 1], N, d.dims.NLP_x, d.dims.NLP_u, blk, self.nvar, self.nv, sch == "trapeze")
                    for k in range(3)]
        self.con = [constraint_read_set(cuts[k], cuts[k + 1], N, cb, eqs, self.ncon) for k in range(3)]
        self.xd, self.vd, self.wd, self.yd = (torch.from_numpy(a).cuda() for a in (self.x, self.v, self.w, self.y))
        if not rt:
            self.o = OracleDOCP(prob, sch, None if grid else N, time_grid=tg, control_steps=cs)
            self.o.set_pattern_mode(1)

    def masked(self, a, mask):
        return self.torch.from_numpy(np.where(mask, a, np.nan)).cuda()

    def bind(self, in_place):
        """in place: every x buffer holds its shard's own variables + v and the table is set; halo-copied: no table, x holds its
        read set.  NaN everywhere else in both."""
        self.xs = [self.masked(self.x, self.var[k][0 if in_place else 1]) for k in range(3)]
        for k, h in enumerate(self.hs):
            if in_place:
                h.set_x_shards(list(self.cuts), [t.data_ptr() for t in self.xs], k)
            else:
                h.set_x_shards(None, None, 0)

    def run(self, op):
        """the three shard calls of `op`: [out_k]; every direction holds exactly its read set"""
        torch, outs = self.torch, []
        for k, h in enumerate(self.hs):
            vk = self.masked(self.v, self.var[k][1])
            if op == "jprod":
                out = torch.full((self.ncon,), 777.0, dtype=torch.float64, device="cuda")
                h.jprod_shard(self.xs[k], vk, out, sync=True)
            elif op == "jtprod":
                out = torch.full((self.nvar,), 777.0, dtype=torch.float64, device="cuda")
                h.jtprod_shard(self.xs[k], self.masked(self.w, self.con[k][1]), out, sync=True)
            else:
                out = torch.full((self.nvar,), 777.0, dtype=torch.float64, device="cuda")
                yk = self.masked(self.y, self.con[k][1]) if op == "hprod" else None
                h.hprod_shard(self.xs[k], yk, vk, obj_weight=SIGMA, out=out, sync=True)
            outs.append(out)
        return outs

    def compose(self, op, outs):
        """own entries only; the pieces cover everything; the d/dv entries are the sum of the three partials"""
        own = [(self.con if op == "jprod" else self.var)[k][0] for k in range(3)]
        comp = np.full(self.ncon if op == "jprod" else self.nvar, 777.0)
        tail = np.zeros(self.nv)
        for k in range(3):
            o = outs[k].cpu().numpy()
            assert not np.isnan(o).any(), (op, k)
            assert (o[~own[k]] == 777.0).all(), (op, k, "wrote outside its own entries")
            body = own[k].copy()
            if op != "jprod":
                body[self.v_off:] = False
                tail += o[self.v_off:]
            comp[body] = o[body]
        if op != "jprod":
            comp[self.v_off:] = tail
        assert not (comp == 777.0).any(), op
        return comp

    def whole(self, op):
        d = self.full
        if op == "jprod":
            return d.jprod(self.xd, self.vd).cpu().numpy()
        if op == "jtprod":
            return d.jtprod(self.xd, self.wd).cpu().numpy()
        return d.hprod(self.xd, self.yd if op == "hprod" else None, self.vd, obj_weight=SIGMA).cpu().numpy()

    def check_reference(self, op, comp, what):
        d, x, v, w, torch = self.full, self.x, self.v, self.w, self.torch
        if op in ("jprod", "jtprod"):
            if self.rt:         # its own handle's structural Jacobian assembled on the host (test_gpu_products.rt_check)
                rows, cols = d.jac_structure()
                vals = d.cons_jac(self.xd)[1].cpu().numpy()
                jv, sv, jtw, sw = coo_products(rows - 1, cols - 1, vals, v, w, self.nvar, self.ncon)
            else:
                colptr, rowval = self.o.jac_pattern()
                jv, sv, jtw, sw = csc_products(colptr, rowval, self.o.jac_coord(x), v, w, self.ncon)
            ref, scale = (jv, sv) if op == "jprod" else (jtw, sw)
            j_assert_close(comp, ref, scale, what)
            return
        y = self.y if op == "hprod" else None
        if self.rt:             # (test_gpu_hprod.rt_check)
            yd = self.yd if y is not None else torch.zeros_like(self.yd)
            ref, scale = handle_product(d, self.xd, yd, SIGMA, v)
            h_assert_close(comp, ref, scale, what)
            return
        # test_gpu_hprod.check_against_oracle on the composed vector
        ref, scale, dropped = oracle_product(self.o, x, np.zeros(self.ncon) if y is None else y, SIGMA, v)
        if not dropped:
            h_assert_close(comp, ref, scale, what)
            return
        off = np.abs(comp - ref) > H_RTOL * np.maximum(1.0, scale)
        assert 0 < off.sum() <= 2 * dropped, (what, int(off.sum()), dropped)
        fd = fd_hprod(d, x, y, SIGMA, v)
        h_assert_close(comp, fd, scale + np.abs(fd), what + ("fd",), rtol=1e-6, mask=off)

    def close(self):
        for h in self.hs:
            h.close()
        self.full.close()


@pytest.mark.parametrize("N,cuts", SIZES, ids=["one_step_shards", "N700"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_three_shards_compose_the_whole_grid_products(torch_cuda, case, N, cuts):
    _, prob, sch, cs, grid, rt = case
    s = Shards(torch_cuda, prob, sch, cs, grid, rt, N, cuts)
    ops = ("jprod", "jtprod", "hprod", "hprod_objective")
    s.bind(in_place=True)
    in_place = {op: s.run(op) for op in ops}
    for op in ops:                                          # two calls give identical bits
        for k, out in enumerate(s.run(op)):
            assert torch_cuda.equal(out, in_place[op][k]), (case[0], op, k, "a second call differs")
    for op in ops:
        comp = s.compose(op, in_place[op])
        ref = s.whole(op)
        body = s.ncon if op == "jprod" else s.v_off
        assert np.array_equal(comp[:body], ref[:body]), (case[0], op, "not the bits of the whole-grid call")
        s.check_reference(op, comp, (case[0], N, op))
    s.bind(in_place=False)
    for op in ops:
        for k, out in enumerate(s.run(op)):
            assert torch_cuda.equal(out, in_place[op][k]), (case[0], op, k, "halo-copied mode differs from the in-place mode")
    s.close()


@pytest.mark.parametrize("prob,sch,rt", [("goddard_all", "trapeze", False), ("quadrotor12", "gauss_legendre_3", False),
                                         ("double_integrator_path", "euler_implicit", False), ("goddard_all", "midpoint", True)])
def test_whole_grid_handle_and_reproducibility(torch_cuda, prob, sch, rt):
    """on a handle of the whole grid every shard call gives the bits of its *_dev_async counterpart, d/dv entries included; two
    calls give identical bits"""
    torch = torch_cuda
    d = ct.DOCP(twin(prob) if rt else prob, 300, sch, device=0)
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    v, w = (torch.from_numpy(a).cuda() for a in directions(d.dim_NLP_variables, d.dim_NLP_constraints))
    new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")      # noqa: E731
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    for _ in range(2):
        assert torch.equal(d.jprod_shard(x, v, new(ncon), sync=True), d.jprod(x, v))
        assert torch.equal(d.jtprod_shard(x, w, new(nvar), sync=True), d.jtprod(x, w))
        assert torch.equal(d.hprod_shard(x, w, v, 0.7, new(nvar), sync=True), d.hprod(x, w, v, obj_weight=0.7))
        assert torch.equal(d.hprod_shard(x, None, v, 1.3, new(nvar), sync=True), d.hprod(x, None, v, obj_weight=1.3))
    d.close()


def test_graph_capture_of_the_shard_calls(torch_cuda):
    """the middle shard of three, its iterate read in place: one warm call of each product on the capturing stream, then the three
    captured together and replayed"""
    torch = torch_cuda
    s = Shards(torch, "goddard_all", "trapeze", 1, False, False, 200, (0, 66, 135, 200))
    s.bind(in_place=True)
    want = {op: s.run(op)[1] for op in ("jprod", "jtprod", "hprod")}
    h = s.hs[1]
    vk, wk, yk = s.masked(s.v, s.var[1][1]), s.masked(s.w, s.con[1][1]), s.masked(s.y, s.con[1][1])
    outs = {"jprod": torch.full((s.ncon,), 777.0, dtype=torch.float64, device="cuda"),
            "jtprod": torch.full((s.nvar,), 777.0, dtype=torch.float64, device="cuda"),
            "hprod": torch.full((s.nvar,), 777.0, dtype=torch.float64, device="cuda")}

    def enqueue():
        h.jprod_shard(s.xs[1], vk, outs["jprod"])
        h.jtprod_shard(s.xs[1], wk, outs["jtprod"])
        h.hprod_shard(s.xs[1], yk, vk, SIGMA, outs["hprod"])

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


def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    E = ct._lib.CTD_EINVAL
    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(5, 12))
    x, v, ov = (torch.zeros(s.dim_NLP_variables, dtype=torch.float64, device="cuda") for _ in range(3))
    w, oc = (torch.zeros(s.dim_NLP_constraints, dtype=torch.float64, device="cuda") for _ in range(2))
    P = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    # null pointers (y may be null), then an output that equals an input
    assert L.ctd_jprod_shard_dev_async(s._h, P(x), None, P(oc)) == E
    assert L.ctd_jprod_shard_dev_async(s._h, None, P(v), P(oc)) == E
    assert L.ctd_jtprod_shard_dev_async(s._h, P(x), P(w), None) == E
    assert L.ctd_hprod_shard_dev_async(s._h, P(x), P(w), 1.0, None, P(ov)) == E
    assert b"null" in L.ctd_last_error(s._h)
    assert L.ctd_jprod_shard_dev_async(s._h, P(x), P(w), P(w)) == E
    assert b"input" in L.ctd_last_error(s._h)
    assert L.ctd_jtprod_shard_dev_async(s._h, P(x), P(w), P(x)) == E
    assert L.ctd_hprod_shard_dev_async(s._h, P(x), P(w), 1.0, P(v), P(v)) == E
    assert L.ctd_hprod_shard_dev_async(s._h, P(x), P(ov), 1.0, P(v), P(ov)) == E          # Hv == y
    assert b"input" in L.ctd_last_error(s._h)
    assert L.ctd_hprod_shard_dev_async(s._h, P(x), None, 1.0, P(v), P(ov)) == 0
    assert L.ctd_jprod_shard_dev_async(s._h, P(x), P(v), P(oc)) == 0
    assert L.ctd_jtprod_shard_dev_async(s._h, P(x), P(w), P(ov)) == 0
    s.sync()
    # the whole-grid entry points still refuse the shard handle, and name the shard calls
    assert L.ctd_jprod_dev_async(s._h, P(x), P(v), P(oc)) == E
    assert b"ctd_jprod_shard_dev_async" in L.ctd_last_error(s._h)
    assert L.ctd_hprod_dev_async(s._h, P(x), P(w), 1.0, P(v), P(ov)) == E
    assert b"shard" in L.ctd_last_error(s._h)
    s.close()
