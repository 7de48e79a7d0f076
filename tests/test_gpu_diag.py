"""The matrix-free KKT diagonals on the MI355X (ctd_hdiag, ctd_jsq_rows, ctd_jsq_cols; DOCP.hdiag / jsq_rows / jsq_cols /
kkt_diag_precond):

    Hd_j = (obj_weight d2 f + sum_r y_r d2 c_r)_jj,    rows_r = sum_j wx_j J_rj^2,    cols_j = sum_r wc_r J_rj^2.

Bars, derived from those of the products (test_gpu_hprod.py, test_gpu_products.py):
  hdiag   |Hd_j - H_jj| <= 1e-10 max(1, |H_jj|, |H^{|y|,|obj_weight|}_jj|): hprod's bar for v = e_j; a diagonal entry absent from
          the oracle's pattern has reference 0;
  jsq_*   |out - ref| <= 3e-12 sum |w| J^2 + 1e-300: jprod's bar with v = e_j is 1e-12 |J_rj| entrywise, squaring doubles the
          relative error, and the third 1e-12 covers the summation (at most ~1e4 terms x 2^-53: the longest sum is a v column at
          N = 300).
References: H and J assembled on the CPU from the oracle in structural mode (where the reference's Euler Hessian pattern leaves true
nonzeros out: hprod(x, y, e_j)[j] of the same handle), the 50-digit Hessian goldens, the structural hess_coord / jac_coord of
run-time OCPs' own handles.  Also: the cross-family identity wx . cols(wc) = wc . rows(wx), bit reproducibility (two calls, host ==
device, every pattern mode / value order), graph capture, the refusals, and scipy's minres on K z = r preconditioned with
DOCP.kkt_diag_precond."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
import jit_defs
from helpers import bench_inputs, describe, hess_golden_files, load_hess_golden
from jit_defs import twin
from oracle.oracle import OracleDOCP

pytestmark = pytest.mark.gpu
HTOL, JTOL = 1e-10, 3e-12
GRIDS = (1, 2, 7, 300)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class Inputs:
    """seeded inputs of one transcription: multipliers uniform(-1, 1), weights uniform(0, 2)"""
    def __init__(self, nvar, ncon, seed=3):
        r = np.random.default_rng(seed)
        self.y = r.uniform(-1.0, 1.0, ncon)
        self.wx, self.wc = r.uniform(0.0, 2.0, nvar), r.uniform(0.0, 2.0, ncon)


def csc_coo(colptr, rowval):
    return np.asarray(rowval, dtype=np.int64), np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))


def dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def coo_diag(rows, cols, vals, n):
    """the diagonal of a COO matrix; entries absent from the pattern are 0"""
    on = rows == cols
    return np.bincount(rows[on], weights=vals[on], minlength=n)


def hdiag_ref(rows, cols, vals, mag, n):
    """reference and bar from the lower triangle (rows, cols, vals) and its magnitude values"""
    on = rows == cols
    scale = np.ones(n)
    np.maximum.at(scale, rows[on], np.maximum(np.abs(vals[on]), np.abs(mag[on])))
    return coo_diag(rows, cols, vals, n), HTOL * scale


def jsq_ref(jr, jc, jv, wx, wc, nvar, ncon):
    """(rows reference, rows bar, cols reference, cols bar) from J = (jr, jc, jv); None weights: ones"""
    wx = np.ones(nvar) if wx is None else wx
    wc = np.ones(ncon) if wc is None else wc
    sq = jv * jv
    rows = np.bincount(jr, weights=wx[jc] * sq, minlength=ncon)
    cols = np.bincount(jc, weights=wc[jr] * sq, minlength=nvar)
    rbar = JTOL * np.bincount(jr, weights=np.abs(wx[jc]) * sq, minlength=ncon) + 1e-300
    cbar = JTOL * np.bincount(jc, weights=np.abs(wc[jr]) * sq, minlength=nvar) + 1e-300
    return rows, rbar, cols, cbar


def assert_block(got, ref, bar, what, mask=None):
    assert np.isfinite(got).all() and np.isfinite(ref).all() and np.isfinite(bar).all(), what
    err = np.abs(got - ref)
    if mask is not None:
        err, bar = err[mask], bar[mask]
    print(what, "max err / bar", float(np.max(err / bar)) if err.size else 0.0)
    bad = err > bar
    assert not bad.any(), (what, int(np.argmax(bad)), float(err[bad].max()), int(bad.sum()))


def oracle_refs(o, x, y, sigma):
    """structural H (lower triangle, with its magnitude values and the count of nonzeros the pattern leaves out) and J of the oracle"""
    hr, hc = csc_coo(*o.hess_pattern())
    vals, dropped = o.hess_coord(x, y, sigma, return_dropped=True)
    mag = o.hess_coord(x, np.abs(y), abs(sigma))
    jr, jc = csc_coo(*o.jac_pattern())
    return (hr, hc, vals, mag, dropped[1]), (jr, jc, o.jac_coord(x))


def check_hdiag(torch, d, H, x, y, sigma, what):
    """hdiag on device tensors against the oracle's diagonal, or -- where its pattern leaves nonzeros out -- against hprod"""
    hr, hc, vals, mag, dropped = H
    nvar = d.dim_NLP_variables
    xd, yd = dev(torch, x, y)
    got = d.hdiag(xd, yd, obj_weight=sigma).cpu().numpy()
    ref, bar = hdiag_ref(hr, hc, vals, mag, nvar)
    if not dropped:
        assert_block(got, ref, bar, what + ("hdiag",))
        return got
    N, blk = d.time.steps, d.discretization._step_variables_block
    if N <= 7:
        idx = np.arange(nvar)
    else:       # 64 indices: entries of node 0, X of node N and v first, then seeded random ones
        n, nv = d.dims.NLP_x, d.dims.NLP_v
        cand = np.r_[np.arange(min(blk, 20)), np.arange(nvar - nv - n, nvar), np.random.default_rng(9).integers(0, nvar, 64)]
        idx = np.array(list(dict.fromkeys(int(j) for j in cand))[:64])
    vd = torch.zeros(nvar, dtype=torch.float64, device="cuda")
    ref = np.zeros(nvar)
    for j in idx:
        vd.zero_()
        vd[j] = 1.0
        ref[j] = float(d.hprod(xd, yd, vd, obj_weight=sigma)[j])
    mask = np.zeros(nvar, dtype=bool)
    mask[idx] = True
    assert_block(got, ref, bar, what + ("hdiag vs hprod",), mask)
    return got


def check_jsq(torch, d, J, x, wx, wc, what):
    jr, jc, jv = J
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    xd, wxd, wcd = dev(torch, x, wx, wc)
    rows, cols = d.jsq_rows(xd, wxd).cpu().numpy(), d.jsq_cols(xd, wcd).cpu().numpy()
    rref, rbar, cref, cbar = jsq_ref(jr, jc, jv, wx, wc, nvar, ncon)
    assert_block(rows, rref, rbar, what + ("jsq_rows",))
    assert_block(cols, cref, cbar, what + ("jsq_cols",))
    return rows, cols


REGISTRY = [p for p, pid in ct.PROBLEMS.items() if pid < 1000]      # the compiled registry (run-time OCPs: ids from 1000)
PAIRS = [(p, s) for p in REGISTRY for s in ct.SCHEMES]


# ---- 1. every registry problem x every scheme against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", PAIRS)
def test_registry_against_oracle(torch_cuda, prob, sch):
    """N = 1 (one step), 2 (first and last node adjacent), 7 (odd interior grid), 300 (several 256-lane workgroups: the partial
    sums and the ordered finish take part); at N = 7 also obj_weight = 0, y = None (bit-identical to a zero y) and NULL weights
    (bit-identical to ones)"""
    torch = torch_cuda
    for N in GRIDS:
        d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
        x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        w = Inputs(nvar, ncon)
        H, J = oracle_refs(o, x, w.y, 0.7)
        check_hdiag(torch, d, H, x, w.y, 0.7, (prob, sch, N))
        check_jsq(torch, d, J, x, w.wx, w.wc, (prob, sch, N))
        if N == 7:
            H0, _ = oracle_refs(o, x, w.y, 0.0)
            check_hdiag(torch, d, H0, x, w.y, 0.0, (prob, sch, N, "obj_weight 0"))
            Hf, _ = oracle_refs(o, x, np.zeros(ncon), 1.3)
            hf = check_hdiag(torch, d, Hf, x, None, 1.3, (prob, sch, N, "y None"))
            assert np.array_equal(hf, d.hdiag(dev(torch, x)[0], torch.zeros(ncon, dtype=torch.float64, device="cuda"), 1.3).cpu().numpy())
            r1, c1 = check_jsq(torch, d, J, x, None, None, (prob, sch, N, "NULL weights"))
            rows, cols = check_jsq(torch, d, J, x, np.ones(nvar), np.ones(ncon), (prob, sch, N, "ones"))
            assert np.array_equal(r1, rows) and np.array_equal(c1, cols)


# ---- 2. 50-digit goldens -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", hess_golden_files(), ids=lambda p: p.split("/")[-1][:-5])
def test_golden_hessians(torch_cuda, path):
    """the diagonal of the fixture's exact Hessian; the bar takes the larger of the fixture's and the oracle's entry scales, as the
    golden test of test_gpu_hprod.py does"""
    g = load_hess_golden(path)
    cs = g.get("control_steps", 1)
    prob = twin(g["problem"]) if cs > 3 else g["problem"]
    d = ct.DOCP(prob, g["grid_size"], g["scheme"], time_grid=g["time_grid"], device=0, control_steps=cs)
    nvar = d.dim_NLP_variables
    keys = list(g["H"])
    rows = np.array([k[0] for k in keys], dtype=np.int64)
    cols = np.array([k[1] for k in keys], dtype=np.int64)
    vals = np.array([g["H"][k] for k in keys])
    ref, bar = hdiag_ref(rows, cols, vals, vals, nvar)
    o = OracleDOCP(g["problem"], g["scheme"], g["grid_size"], time_grid=g["time_grid"], control_steps=cs)
    o.set_pattern_mode(1)
    hr, hc = csc_coo(*o.hess_pattern())
    _, obar = hdiag_ref(hr, hc, o.hess_coord(g["xu"], g["y"], g["obj_weight"]),
                        o.hess_coord(g["xu"], np.abs(g["y"]), abs(g["obj_weight"])), nvar)
    got = d.hdiag(g["xu"], g["y"], obj_weight=g["obj_weight"])
    assert_block(got, ref, np.maximum(bar, obar), (path, "hdiag"))


# ---- 3. cross-family identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("double_integrator_freet0tf", "trapeze"),
                                      ("quadrotor12", "gauss_legendre_2"), ("quadrotor", "euler_implicit"),
                                      ("least_squares_with_constraint", "midpoint"), ("double_integrator_path", "euler")])
def test_rows_and_columns_agree(torch_cuda, prob, sch):
    """wx . jsq_cols(x, wc) and wc . jsq_rows(x, wx) are the same double sum sum_rj wx_j wc_r J_rj^2, computed by two lane
    families: they agree to the two entry bars summed against the other weight vector"""
    for N in (7, 300):
        d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
        x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        w = Inputs(nvar, ncon, seed=8)
        jr, jc = csc_coo(*o.jac_pattern())
        _, rbar, _, cbar = jsq_ref(jr, jc, o.jac_coord(x), w.wx, w.wc, nvar, ncon)
        xd, wxd, wcd = dev(torch_cuda, x, w.wx, w.wc)
        lhs = float(w.wx @ d.jsq_cols(xd, wcd).cpu().numpy())
        rhs = float(w.wc @ d.jsq_rows(xd, wxd).cpu().numpy())
        bar = float(np.abs(w.wx) @ cbar + np.abs(w.wc) @ rbar)
        print((prob, sch, N), "difference / bar", abs(lhs - rhs) / bar)
        assert abs(lhs - rhs) <= bar, (lhs, rhs, bar)


# ---- 4. run-time OCPs ----------------------------------------------------------------------------------------------------------
def handle_refs(torch, d, x, y, sigma):
    """H and J from the handle's own structural hess_coord / jac_coord"""
    xd, yd = dev(torch, x, y)
    hr, hc = d.hess_structure()
    vals = d.hess_coord(xd, yd, sigma).cpu().numpy()
    mag = d.hess_coord(xd, torch.abs(yd), abs(sigma)).cpu().numpy()
    jr, jc = d.jac_structure()
    return (hr - 1, hc - 1, vals, mag, 0), (jr - 1, jc - 1, d.cons_jac(xd)[1].cpu().numpy())


def rt_case(name, sch, N, control_steps=1):
    d = ct.DOCP(name, N, sch, device=0, pattern="structural", control_steps=control_steps)
    x = 0.5 + 0.3 * np.random.default_rng(11).uniform(-1.0, 1.0, d.dim_NLP_variables)
    return d, x, Inputs(d.dim_NLP_variables, d.dim_NLP_constraints, seed=5)


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control", "euler"])
@pytest.mark.parametrize("prob", ["goddard_all", "double_integrator_path"])
def test_runtime_twins(torch_cuda, prob, sch):
    """the expression twin of a registry problem gives the registry handle's values (both within their bars) and the values of its
    own assembled H and J.  Explicit Euler: the twin against the registry handle only -- the handle's Hessian pattern leaves true
    nonzeros out there (test_gpu_hprod.py), so its hess_coord is no reference for the diagonal"""
    torch = torch_cuda
    N = 40
    reg = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    rt = ct.DOCP(twin(prob), N, sch, device=0, pattern="structural")
    nvar, ncon = reg.dim_NLP_variables, reg.dim_NLP_constraints
    assert (rt.dim_NLP_variables, rt.dim_NLP_constraints) == (nvar, ncon)
    x = bench_inputs(describe(reg, prob, sch), perturb=1e-3)
    w = Inputs(nvar, ncon, seed=5)
    H, J = handle_refs(torch, rt, x, w.y, 0.6)
    xd, yd, wxd, wcd = dev(torch, x, w.y, w.wx, w.wc)
    if sch == "euler":
        hd = rt.hdiag(xd, yd, obj_weight=0.6).cpu().numpy()
    else:
        hd = check_hdiag(torch, rt, H, x, w.y, 0.6, (prob, sch, "twin"))
    rows, cols = check_jsq(torch, rt, J, x, w.wx, w.wc, (prob, sch, "twin"))
    _, hbar = hdiag_ref(H[0], H[1], H[2], H[3], nvar)
    _, rbar, _, cbar = jsq_ref(*J, w.wx, w.wc, nvar, ncon)
    assert_block(reg.hdiag(xd, yd, obj_weight=0.6).cpu().numpy(), hd, 2 * hbar, (prob, sch, "registry hdiag"))
    assert_block(reg.jsq_rows(xd, wxd).cpu().numpy(), rows, 2 * rbar, (prob, sch, "registry jsq_rows"))
    assert_block(reg.jsq_cols(xd, wcd).cpu().numpy(), cols, 2 * cbar, (prob, sch, "registry jsq_cols"))


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control", "euler_implicit"])
def test_runtime_only_problem(torch_cuda, sch):
    """a problem that exists only as expressions (free tf, Bolza cost, path and boundary rows that read v)"""
    name = "vdp_rt" if "vdp_rt" in ct.PROBLEMS else ct.register_ocp("vdp_rt", **jit_defs.VDP)
    d, x, w = rt_case(name, sch, 40)
    x[-1] = 2.0 + 0.1 * x[-1]           # tf > t0 = 0.25
    H, J = handle_refs(torch_cuda, d, x, w.y, 0.6)
    check_hdiag(torch_cuda, d, H, x, w.y, 0.6, (name, sch))
    check_jsq(torch_cuda, d, J, x, w.wx, w.wc, (name, sch))


def test_runtime_four_controls_per_step(torch_cuda):
    """control_steps = 4: beyond what the registry compiles in"""
    d, _, w = rt_case(twin("goddard_all"), "midpoint", 30, control_steps=4)
    x = bench_inputs(describe(d, "goddard_all", "midpoint"), perturb=1e-3)
    H, J = handle_refs(torch_cuda, d, x, w.y, 0.6)
    check_hdiag(torch_cuda, d, H, x, w.y, 0.6, ("cs4",))
    check_jsq(torch_cuda, d, J, x, w.wx, w.wc, ("cs4",))


# ---- 5. bits -------------------------------------------------------------------------------------------------------------------
def all_three(torch, d, x, w, sigma=0.7):
    xd, yd, wxd, wcd = dev(torch, x, w.y, w.wx, w.wc)
    return [t.cpu().numpy() for t in (d.hdiag(xd, yd, obj_weight=sigma), d.jsq_rows(xd, wxd), d.jsq_cols(xd, wcd))]


@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("quadrotor12", "gauss_legendre_2"),
                                      ("double_integrator_freet0tf", "trapeze"), ("estimate_rotation_rate", "euler_implicit"),
                                      ("double_integrator_path", "midpoint")])
def test_reproducible_host_device(torch_cuda, prob, sch):
    """two calls, and the host form == the device form (NULL optional arguments included)"""
    d = ct.DOCP(prob, 300, sch, device=0)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints)
    a, b = all_three(torch_cuda, d, x, w), all_three(torch_cuda, d, x, w)
    host = [d.hdiag(x, w.y, obj_weight=0.7), d.jsq_rows(x, w.wx), d.jsq_cols(x, w.wc)]
    for u, v, h in zip(a, b, host):
        assert np.array_equal(u, v) and np.array_equal(u, h)
    xd = dev(torch_cuda, x)[0]
    for hostv, devv in ((d.hdiag(x, None, obj_weight=0.7), d.hdiag(xd, None, obj_weight=0.7)), (d.jsq_rows(x), d.jsq_rows(xd)),
                        (d.jsq_cols(x), d.jsq_cols(xd))):
        assert np.array_equal(hostv, devv.cpu().numpy())


@pytest.mark.parametrize("prob,sch", [("double_integrator_freet0tf", "trapeze"), ("goddard_all", "euler_implicit")])
def test_pattern_independence(torch_cuda, prob, sch):
    """manual, structural, optimized and CSR handles of one transcription whose manual pattern drops nonzeros: identical bits"""
    results = []
    for kw in (dict(pattern="manual"), dict(pattern="structural"), dict(pattern="optimized"),
               dict(pattern="structural", value_order="csr"), dict(pattern="manual", value_order="csr")):
        d = ct.DOCP(prob, 40, sch, device=0, **kw)
        if not results:
            assert d.dropped_nonzeros() > 0
            x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
            w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints)
        results.append(all_three(torch_cuda, d, x, w))
    for r in results[1:]:
        assert all(np.array_equal(u, v) for u, v in zip(r, results[0]))


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------
def capture_case(torch, d, x, w):
    """a warm call of everything, an hprod graph captured first, then the three calls captured and replayed: the eager bits; and the
    hprod graph, replayed after the new calls have run, still gives its own (separate partial-sum buffers)"""
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    xd, yd, wxd, wcd = dev(torch, x, w.y, w.wx, w.wc)
    eager = all_three(torch, d, x, w)
    hv_eager = d.hprod(xd, yd, wxd, obj_weight=0.7).cpu().numpy()
    s = torch.cuda.Stream()
    d.set_stream(s)
    hv = torch.empty(nvar, dtype=torch.float64, device="cuda")
    outs = [torch.empty(n, dtype=torch.float64, device="cuda") for n in (nvar, ncon, nvar)]

    def three():
        d.hdiag(xd, yd, obj_weight=0.7, out=outs[0], sync=False)
        d.jsq_rows(xd, wxd, out=outs[1], sync=False)
        d.jsq_cols(xd, wcd, out=outs[2], sync=False)

    with torch.cuda.stream(s):
        d.hprod(xd, yd, wxd, obj_weight=0.7, out=hv, sync=False)
        three()
    s.synchronize()
    gh = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gh, stream=s):
        d.hprod(xd, yd, wxd, obj_weight=0.7, out=hv, sync=False)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        three()
    for o in outs:
        o.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert np.array_equal(o.cpu().numpy(), e)
    hv.fill_(0.0)
    gh.replay()
    torch.cuda.synchronize()
    assert np.array_equal(hv.cpu().numpy(), hv_eager)


def test_graph_capture(torch_cuda):
    prob, sch = "goddard_all", "gauss_legendre_2"
    d = ct.DOCP(prob, 300, sch, device=0)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    capture_case(torch_cuda, d, x, Inputs(d.dim_NLP_variables, d.dim_NLP_constraints))


def test_graph_capture_runtime_ocp(torch_cuda):
    d, _, w = rt_case(twin("goddard_all"), "midpoint", 40)
    capture_case(torch_cuda, d, bench_inputs(describe(d, "goddard_all", "midpoint"), perturb=1e-3), w)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    E = ct._lib.CTD_EINVAL
    d = ct.DOCP("goddard", 20, "midpoint", device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    x, wx, ov = t(nvar, 1.0), t(nvar, 0.5), t(nvar, 7.0)
    y, oc = t(ncon, 1.0), t(ncon, 7.0)
    P = lambda a: None if a is None else C.c_void_p(a.data_ptr())        # noqa: E731
    calls = {"hdiag": (lambda h, x_, a, o: L.ctd_hdiag_dev_async(h, P(x_), P(a), 1.0, P(o)), y, ov),
             "jsq_rows": (lambda h, x_, a, o: L.ctd_jsq_rows_dev_async(h, P(x_), P(a), P(o)), wx, oc),
             "jsq_cols": (lambda h, x_, a, o: L.ctd_jsq_cols_dev_async(h, P(x_), P(a), P(o)), y, ov)}

    def untouched():
        d.sync()
        return bool((ov == 7.0).all()) and bool((oc == 7.0).all())

    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(0, 10))
    sh = ct.DOCP("goddard", 20, "midpoint", device=0)
    sh.set_x_shards([0, 20], [x.data_ptr()], 0)
    for name, (fn, a, o) in calls.items():
        for args in ((None, a, o), (x, a, None)):
            assert fn(d._h, *args) == E, name
            assert b"null" in L.ctd_last_error(d._h), name
            assert L.ctd_last_error(d._h).startswith(b"ctd_" + name.encode() + b"_dev_async: "), name
            assert untouched(), name
        for args, keep in (((x, a, x), x), ((x, a, a), a)):
            before = keep.clone()
            assert fn(d._h, *args) == E, name
            assert b"input" in L.ctd_last_error(d._h), name
            assert L.ctd_last_error(d._h).startswith(b"ctd_" + name.encode() + b"_dev_async: "), name
            d.sync()
            assert torch.equal(keep, before) and untouched(), name
        # shard handles: a range of steps, and a whole-grid handle with an x-shard table
        assert fn(s._h, x, a, o) == E, name
        assert b"shard" in L.ctd_last_error(s._h) and b"out of scope" in L.ctd_last_error(s._h), name
        assert L.ctd_last_error(s._h).startswith(b"ctd_" + name.encode() + b"_dev_async: "), name
        assert b"ctd_" + name.encode() + b"_shard_dev_async" in L.ctd_last_error(s._h), name
        assert fn(sh._h, x, a, o) == E, name
        assert b"shard" in L.ctd_last_error(sh._h), name
        assert untouched(), name
    # the optional input may be NULL
    for name, (fn, a, o) in calls.items():
        assert fn(d._h, x, None, o) == 0, name
    d.sync()
    assert not bool((ov == 7.0).any()) and not bool((oc == 7.0).any())


# ---- 8. preconditioned MINRES through the operators alone --------------------------------------------------------------------------
def minres_case():
    """Goddard, trapeze, N = 20, structural pattern: the seeded inputs, K_asm assembled from the oracle, its blocks H and J"""
    import scipy.sparse as sp
    prob, sch, N = "goddard", "trapeze", 20
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
    lam_min = float(np.linalg.eigvalsh(H.toarray())[0])
    sx = 10.0 ** r.uniform(-3.0, 5.0, nvar) + max(0.0, -lam_min)
    sc = 1e-2 * r.uniform(1.0, 2.0, ncon)
    rhs = r.uniform(-1.0, 1.0, nvar + ncon)
    J = sp.csr_matrix((jv, (jr, jc)), shape=(ncon, nvar))
    K_asm = sp.bmat([[H + sp.diags(sx), J.T], [J, -sp.diags(sc)]]).tocsr()
    return dict(prob=prob, sch=sch, N=N, x=x, y=y, sx=sx, sc=sc, rhs=rhs, H=H, J=J, K_asm=K_asm, nvar=nvar, ncon=ncon)


def run_minres(K, rhs, M, cap):
    """(solution, info, iterations); a run that does not reach info == 0 within the cap counts the cap"""
    its = [0]
    z, info = minres(K, rhs, M=M, rtol=1e-10, maxiter=cap, callback=lambda zk: its.__setitem__(0, its[0] + 1))
    return z, info, (its[0] if info == 0 else cap)


def asm_precond(c, floor=1e-8):
    """the preconditioner of DOCP.kkt_diag_precond from K_asm's own blocks"""
    px = np.maximum(np.abs(c["H"].diagonal() + c["sx"]), floor)
    pc = np.asarray(c["J"].multiply(c["J"]) @ (1.0 / px)).ravel() + c["sc"]
    return px, pc


def test_preconditioned_minres_through_the_operators(torch_cuda):
    """scipy's minres on K z = r with K given only as DOCP.kktprod and M = diag(1 / px, 1 / pc) from DOCP.kkt_diag_precond, against
    the same solve without M; both residuals measured under K_asm assembled from the oracle.  Goddard, trapeze, N = 20 (149
    unknowns), y = 0.1 U(-1, 1), sx = 10^U(-3, 5) + max(0, -lambda_min(H_asm)), sc = 1e-2 U(1, 2), seed 21.
    Asserted: the preconditioned run returns info == 0, needs at most half the plain run's iterations (a plain run that does not
    converge within the cap of 10 (nvar + ncon) counts the cap), leaves a true residual no larger than the plain run's, and takes
    the iteration count (+-2) of a run whose M is built from K_asm's own diagonals.
    On the CPU, with K_asm and its diagonals only and these exact inputs: plain 313 iterations (true residual 1.6e-3 |r|),
    preconditioned 72 (2.3e-6 |r|): a factor of 4.3 where 2 is asked; counts move with last-bit differences of the operator."""
    torch = torch_cuda
    c = minres_case()
    nvar, ncon, n = c["nvar"], c["ncon"], c["nvar"] + c["ncon"]
    d = ct.DOCP(c["prob"], c["N"], c["sch"], device=0, pattern="structural")
    assert (d.dim_NLP_variables, d.dim_NLP_constraints) == (nvar, ncon)
    xd, yd, sxd, scd = dev(torch, c["x"], c["y"], c["sx"], c["sc"])
    zin = torch.empty(n, dtype=torch.float64, device="cuda")
    zout = torch.empty(n, dtype=torch.float64, device="cuda")

    def matvec(z):
        zin.copy_(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64).ravel()))
        d.kktprod(xd, yd, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=sxd, sc=scd, out=(zout[:nvar], zout[nvar:]))
        return zout.cpu().numpy()

    def diag_op(px, pc):
        m = 1.0 / np.r_[px, pc]
        return LinearOperator((n, n), matvec=lambda v: m * np.asarray(v).ravel(), dtype=np.float64)

    K = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
    px, pc = d.kkt_diag_precond(xd, yd, obj_weight=1.0, sx=sxd, sc=scd)
    px, pc = px.cpu().numpy(), pc.cpu().numpy()
    assert (px > 0).all() and (pc > 0).all()
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
