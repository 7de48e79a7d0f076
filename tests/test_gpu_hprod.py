"""Matrix-free Hessian-of-the-Lagrangian products on the MI355X (ctd_hprod / ctd_hprod_dev_async, DOCP.hprod).

H = obj_weight d2 f + sum_r y_r d2 c_r is the exact second derivative of the objective and the constraints.  Each product is checked
entry by entry against the symmetric matrix rebuilt from a lower triangle, with the bar of helpers.hess_err applied to a product:
every Hessian entry may be off by 1e-10 max(1, |H_ij|, |H_ij| with |y| and |obj_weight|), so
|got - ref|_i <= 1e-10 sum_j max(1, |H_ij|, |H^{|y|,|obj_weight|}_ij|) |v_j|  (Goddard's drag terms cancel inside single entries:
two double-precision evaluations of the product agree to this bar, not to 1e-10 of (|H| |v|)_i).  References: the 50-digit goldens (every hess_*.json), the oracle's
hess_coord for every registry problem x every scheme, the structural hess_coord of run-time OCPs and of the full-size workloads.
Where a Hessian pattern leaves true nonzeros out (the reference's Euler patterns), the product holds them: those entries are checked
against central differences of the engine's own first-order callbacks.  Also: objective only (y = None) and constraints only
(obj_weight = 0), pattern independence, symmetry, linearity, bit reproducibility, graph capture, a 2^22-step grid without any
nnzh-sized array, the refusals, and scipy's trust-constr driven by hprod alone."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import Bounds, NonlinearConstraint, minimize
from scipy.sparse.linalg import LinearOperator

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe, hess_golden_files, load_hess_golden
from jit_defs import FUNCS, catalogue, twin
from oracle.oracle import OracleDOCP

pytestmark = pytest.mark.gpu
RTOL = 1e-10


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def rand(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def sym_product(rows, cols, vals, v, n):
    """H v of the symmetric matrix whose lower triangle is the 0-based COO (rows >= cols, vals)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    off = rows != cols
    return (np.bincount(rows, weights=vals * v[cols], minlength=n) +
            np.bincount(cols[off], weights=vals[off] * v[rows[off]], minlength=n))


def csc_coo(colptr, rowval):
    return np.asarray(rowval, dtype=np.int64), np.repeat(np.arange(len(colptr) - 1), np.diff(colptr))


def entry_scale(vals, mag):
    """per-entry bar of helpers.hess_err: max(1, |H_ij|, |H^{|y|,|obj_weight|}_ij|)"""
    return np.maximum(1.0, np.maximum(np.abs(vals), np.abs(mag)))


def assert_close(got, ref, scale, what, rtol=RTOL, mask=None):
    err = np.abs(got - ref)
    bad = err > rtol * np.maximum(1.0, scale)
    if mask is not None:
        bad &= mask
    assert not bad.any(), (what, int(np.argmax(bad)), float(err[bad].max()), int(bad.sum()))


def lagrangian_gradient(d, x, y, sigma):
    g = sigma * d.grad(x)
    return g if y is None else g + d.jtprod(x, y)


def fd_hprod(d, x, y, sigma, v, eps=1e-6):
    """central difference of sigma grad f + J' y along v (first-order callbacks only)"""
    return (lagrangian_gradient(d, x + eps * v, y, sigma) - lagrangian_gradient(d, x - eps * v, y, sigma)) / (2 * eps)


# ---- 50-digit goldens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", hess_golden_files(), ids=lambda p: p.split("/")[-1][:-5])
def test_golden_hessians(torch_cuda, path):
    """H of the fixture (exact, 50 digits, with the nonzeros a pattern may leave out) times a seeded random v"""
    g = load_hess_golden(path)
    cs = g.get("control_steps", 1)
    prob = twin(g["problem"]) if cs > 3 else g["problem"]
    d = ct.DOCP(prob, g["grid_size"], g["scheme"], time_grid=g["time_grid"], device=0, control_steps=cs)
    n = d.dim_NLP_variables
    v = rand(n, 17)
    keys = list(g["H"])
    rows = np.array([k[0] for k in keys], dtype=np.int64)
    cols = np.array([k[1] for k in keys], dtype=np.int64)
    vals = np.array([g["H"][k] for k in keys])
    ref = sym_product(rows, cols, vals, v, n)
    scale = sym_product(rows, cols, np.maximum(1.0, np.abs(vals)), np.abs(v), n)
    o = OracleDOCP(g["problem"], g["scheme"], g["grid_size"], time_grid=g["time_grid"], control_steps=cs)
    o.set_pattern_mode(1)
    r, c = csc_coo(*o.hess_pattern())
    mag = entry_scale(o.hess_coord(g["xu"], g["y"], g["obj_weight"]), o.hess_coord(g["xu"], np.abs(g["y"]), abs(g["obj_weight"])))
    scale = np.maximum(scale, sym_product(r, c, mag, np.abs(v), n))
    got = d.hprod(g["xu"], g["y"], v, obj_weight=g["obj_weight"])
    assert_close(got, ref, scale, path)


# ---- oracle: every registry problem x every scheme -------------------------------------------------------------------------
def oracle_product(o, x, y, sigma, v):
    """the oracle's pattern product, its magnitude (|y|, |sigma|, |v|) and the nonzeros its pattern leaves out"""
    n = len(x)
    r, c = csc_coo(*o.hess_pattern())
    vals, dropped = o.hess_coord(x, y, sigma, return_dropped=True)
    mag = o.hess_coord(x, np.abs(y), abs(sigma))
    return sym_product(r, c, vals, v, n), sym_product(r, c, entry_scale(vals, mag), np.abs(v), n), dropped[1]


def check_against_oracle(torch, d, o, x, y, sigma, v, what):
    yo = np.zeros(d.dim_NLP_constraints) if y is None else y
    ref, scale, dropped = oracle_product(o, x, yo, sigma, v)
    xd, vd = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    yd = None if y is None else torch.from_numpy(y).cuda()
    got = d.hprod(xd, yd, vd, obj_weight=sigma).cpu().numpy()
    assert np.array_equal(got, d.hprod(x, y, v, obj_weight=sigma)), what        # host == device, bit for bit
    if not dropped:
        assert_close(got, ref, scale, what)
        return got
    # the pattern leaves true nonzeros out: every entry they touch differs; those match the derivative of the gradient
    off = np.abs(got - ref) > RTOL * np.maximum(1.0, scale)
    assert 0 < off.sum() <= 2 * dropped, (what, int(off.sum()), dropped)
    fd = fd_hprod(d, x, y, sigma, v)
    assert_close(got, fd, scale + np.abs(fd), what + ("fd",), rtol=1e-6, mask=off)
    return got


REGISTRY = [p for p, pid in ct.PROBLEMS.items() if pid < 1000]      # the compiled registry (run-time OCPs: ids from 1000)
PAIRS = [(p, s) for p in REGISTRY for s in ct.SCHEMES]


@pytest.mark.parametrize("prob,sch", PAIRS)
def test_registry_against_oracle(torch_cuda, prob, sch):
    """N = 1, 7 and a grid of several workgroups; at N = 7 also the objective alone (y = None: bit-identical to y = 0) and the
    constraints alone (obj_weight = 0)"""
    for N in (1, 7, 300):
        d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        v, y = rand(d.dim_NLP_variables, 3), rand(d.dim_NLP_constraints, 4)
        check_against_oracle(torch_cuda, d, o, x, y, 0.7, v, (prob, sch, N))
        if N == 7:
            h0 = check_against_oracle(torch_cuda, d, o, x, None, 1.3, v, (prob, sch, N, "objective"))
            assert np.array_equal(h0, d.hprod(x, np.zeros(d.dim_NLP_constraints), v, obj_weight=1.3))
            check_against_oracle(torch_cuda, d, o, x, y, 0.0, v, (prob, sch, N, "constraints"))


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control"])
@pytest.mark.parametrize("prob", ["goddard_all", "double_integrator_freet0tf"])
def test_nonuniform_grid(torch_cuda, prob, sch):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(23))])
    tg = tg / tg[-1]
    d = ct.DOCP(prob, len(tg) - 1, sch, time_grid=tg, device=0)
    o = OracleDOCP(prob, sch, None, time_grid=tg)
    o.set_pattern_mode(1)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    check_against_oracle(torch_cuda, d, o, x, rand(d.dim_NLP_constraints, 4), 0.7, rand(d.dim_NLP_variables, 3), (prob, sch))


@pytest.mark.parametrize("prob", ["goddard_all", "quadrotor12"])
@pytest.mark.parametrize("cs", [2, 3])
def test_direct_shooting(torch_cuda, prob, cs):
    for N in (1, 9, 200):
        d = ct.DOCP(prob, N, "midpoint", device=0, control_steps=cs)
        o = OracleDOCP(prob, "midpoint", N, control_steps=cs)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(d, prob, "midpoint"), perturb=1e-3)
        check_against_oracle(torch_cuda, d, o, x, rand(d.dim_NLP_constraints, 4), 0.7, rand(d.dim_NLP_variables, 3),
                             (prob, cs, N))


# ---- run-time OCPs ---------------------------------------------------------------------------------------------------------
def handle_product(d, xd, yd, sigma, v):
    """the handle's own assembled product (hess_structure + hess_coord) and its magnitude"""
    import torch
    hr, hc = d.hess_structure()
    vals = d.hess_coord(xd, yd, sigma).cpu().numpy()
    mag = d.hess_coord(xd, torch.abs(yd), abs(sigma)).cpu().numpy()
    n = d.dim_NLP_variables
    return sym_product(hr - 1, hc - 1, vals, v, n), sym_product(hr - 1, hc - 1, entry_scale(vals, mag), np.abs(v), n)


def rt_check(torch, name, sch, N=40, control_steps=1):
    d = ct.DOCP(name, N, sch, device=0, pattern="structural", control_steps=control_steps)
    r = np.random.default_rng(11)
    x = 0.5 + 0.3 * r.uniform(-1.0, 1.0, d.dim_NLP_variables)
    v, y = rand(d.dim_NLP_variables, 5), rand(d.dim_NLP_constraints, 6)
    xd, yd, vd = (torch.from_numpy(a).cuda() for a in (x, y, v))
    ref, scale = handle_product(d, xd, yd, 0.6, v)
    assert_close(d.hprod(xd, yd, vd, obj_weight=0.6).cpu().numpy(), ref, scale, (name, sch))


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control"])
@pytest.mark.parametrize("which", ["beam", "bolza_freetf", "funcs"])
def test_runtime_ocps(torch_cuda, which, sch):
    if which == "funcs":
        name = "funcs_rt" if "funcs_rt" in ct.PROBLEMS else ct.register_ocp("funcs_rt", **FUNCS)
    else:
        name = catalogue(which)[0]
    rt_check(torch_cuda, name, sch)


def test_runtime_twins(torch_cuda):
    rt_check(torch_cuda, twin("quadrotor12"), "gauss_legendre_2")
    rt_check(torch_cuda, twin("goddard_all"), "midpoint", N=30, control_steps=4)


# ---- pattern independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("double_integrator_freet0tf", "trapeze"), ("goddard_all", "euler_implicit"),
                                      ("estimate_rotation_rate", "euler"), ("double_integrator_path", "euler")])
def test_pattern_independence(torch_cuda, prob, sch):
    """bit-identical across manual / structural / optimized patterns and CSC / CSR value orders; where the Hessian pattern leaves
    true nonzeros out (the reference's explicit Euler pattern), the product differs from the assembled one and matches the
    derivative of the gradient of the Lagrangian"""
    torch = torch_cuda
    N = 40
    x = None
    results = []
    for kw in (dict(pattern="manual"), dict(pattern="structural"), dict(pattern="optimized"),
               dict(pattern="structural", value_order="csr"), dict(pattern="manual", value_order="csr")):
        d = ct.DOCP(prob, N, sch, device=0, **kw)
        if x is None:
            x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
            v, y = rand(d.dim_NLP_variables, 3), rand(d.dim_NLP_constraints, 4)
            xd, yd, vd = (torch.from_numpy(a).cuda() for a in (x, y, v))
        results.append(d.hprod(xd, yd, vd, obj_weight=0.7).cpu().numpy())
        if kw == dict(pattern="manual"):
            ref, scale = handle_product(d, xd, yd, 0.7, v)
            manual_diff = np.abs(results[-1] - ref) > RTOL * np.maximum(1.0, scale)
            fd = fd_hprod(d, x, y, 0.7, v)
            assert_close(results[-1], fd, scale + np.abs(fd), (prob, sch, "fd"), rtol=1e-6)
    for r in results[1:]:
        assert np.array_equal(r, results[0])
    o = OracleDOCP(prob, sch, N)
    o.set_pattern_mode(1)
    _, _, dropped = oracle_product(o, x, y, 0.7, v)
    assert manual_diff.any() == (dropped > 0), (prob, sch, dropped)


# ---- identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("quadrotor12", "gauss_legendre_2"),
                                      ("double_integrator_freet0tf", "gauss_legendre_2"), ("estimate_rotation_rate", "euler_implicit"),
                                      ("goddard", "midpoint")])
def test_identities_reproducibility_capture(torch_cuda, prob, sch):
    """symmetry, linearity in (y, obj_weight), central differences of the first-order callbacks, two calls bit-identical, replay
    of a captured graph"""
    torch = torch_cuda
    d = ct.DOCP(prob, 500, sch, device=0)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    n = d.dim_NLP_variables
    v, w, y = rand(n, 3), rand(n, 8), rand(d.dim_NLP_constraints, 4)
    xd, vd, wd, yd = (torch.from_numpy(a).cuda() for a in (x, v, w, y))
    hv = d.hprod(xd, yd, vd, obj_weight=0.7).cpu().numpy()
    hw = d.hprod(xd, yd, wd, obj_weight=0.7).cpu().numpy()
    a, b = float(w @ hv), float(v @ hw)
    assert abs(a - b) <= 1e-10 * max(np.abs(w) @ np.abs(hv), np.abs(v) @ np.abs(hw), 1.0), (a, b)
    hc = d.hprod(xd, yd, vd, obj_weight=0.0).cpu().numpy()
    ho = d.hprod(xd, None, vd, obj_weight=0.7).cpu().numpy()
    assert np.max(np.abs(hc + ho - hv)) <= 1e-10 * max(1.0, np.abs(hv).max(), np.abs(hc).max(), np.abs(ho).max())
    fd = fd_hprod(d, x, y, 0.7, v)
    assert np.linalg.norm(fd - hv) <= 1e-6 * max(1.0, np.linalg.norm(hv)), np.linalg.norm(fd - hv)
    assert np.array_equal(d.hprod(xd, yd, vd, obj_weight=0.7).cpu().numpy(), hv)
    # graph capture after one warm call on the capturing stream
    s = torch.cuda.Stream()
    d.set_stream(s)
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    with torch.cuda.stream(s):
        d.hprod(xd, yd, vd, obj_weight=0.7, out=out, sync=False)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        d.hprod(xd, yd, vd, obj_weight=0.7, out=out, sync=False)
    out.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), hv)


# ---- full size and long grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch,N", [("goddard", "gauss_legendre_2", 10_000), ("double_integrator_path", "midpoint", 100_000),
                                        ("quadrotor12", "gauss_legendre_3", 20_000)])
def test_full_size_workloads(torch_cuda, prob, sch, N):
    """bench configs 2, 3 and 5 against the structural hess_coord of the same transcription and a host matvec"""
    torch = torch_cuda
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    v, y = rand(d.dim_NLP_variables, 3), rand(d.dim_NLP_constraints, 4)
    xd, yd, vd = (torch.from_numpy(a).cuda() for a in (x, y, v))
    ref, scale = handle_product(d, xd, yd, 0.7, v)
    assert_close(d.hprod(xd, yd, vd, obj_weight=0.7).cpu().numpy(), ref, scale, (prob, sch, N))


def test_large_grid_without_hessian(torch_cuda):
    """Goddard, midpoint, N = 2^22: no nnzh-sized array anywhere; symmetry and a central difference of grad + jtprod"""
    torch = torch_cuda
    N = 1 << 22
    d = ct.DOCP("goddard", N, "midpoint", device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, "goddard", "midpoint"), perturb=1e-3)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    v = torch.rand(nvar, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    w = torch.rand(nvar, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    y = torch.rand(ncon, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    hv = d.hprod(x, y, v, obj_weight=0.7)
    hw = d.hprod(x, y, w, obj_weight=0.7)
    a, b = float(torch.dot(w, hv)), float(torch.dot(v, hw))
    assert abs(a - b) <= 1e-10 * max(float(torch.dot(w.abs(), hv.abs())), float(torch.dot(v.abs(), hw.abs()))), (a, b)
    eps = 1e-6
    gp = 0.7 * d.grad(x + eps * v) + d.jtprod(x + eps * v, y)
    gm = 0.7 * d.grad(x - eps * v) + d.jtprod(x - eps * v, y)
    fd = (gp - gm) / (2 * eps)
    rel = float(torch.linalg.norm(fd - hv) / torch.linalg.norm(hv))
    assert rel <= 1e-6, rel


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    d = ct.DOCP("goddard", 20, "midpoint", device=0)
    x = torch.zeros(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    v = torch.zeros(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    o = torch.zeros(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    y = torch.zeros(d.dim_NLP_constraints, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    fn = L.ctd_hprod_dev_async
    assert fn(d._h, None, P(y), 1.0, P(v), P(o)) == ct._lib.CTD_EINVAL
    assert fn(d._h, P(x), P(y), 1.0, None, P(o)) == ct._lib.CTD_EINVAL
    assert fn(d._h, P(x), P(y), 1.0, P(v), None) == ct._lib.CTD_EINVAL
    assert b"null" in L.ctd_last_error(d._h)
    assert L.ctd_last_error(d._h).startswith(b"ctd_hprod_dev_async: ")
    for alias in (x, v):
        assert fn(d._h, P(x), P(y), 1.0, P(v), P(alias)) == ct._lib.CTD_EINVAL
        assert b"input" in L.ctd_last_error(d._h)
        assert L.ctd_last_error(d._h).startswith(b"ctd_hprod_dev_async: ")
    assert fn(d._h, P(x), P(y), 1.0, P(v), P(y)) == ct._lib.CTD_EINVAL
    assert b"input" in L.ctd_last_error(d._h)
    assert fn(d._h, P(x), None, 1.0, P(v), P(o)) == 0
    d.sync()
    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(0, 10))
    assert fn(s._h, P(x), P(y), 1.0, P(v), P(o)) == ct._lib.CTD_EINVAL
    assert b"shard" in L.ctd_last_error(s._h)
    assert L.ctd_last_error(s._h).startswith(b"ctd_hprod_dev_async: ") and b"ctd_hprod_shard_dev_async" in L.ctd_last_error(s._h)


# ---- end to end: trust-constr with Hessians given only as products ------------------------------------------------------------
def _trust_constr_hprod(prob, scheme, N):
    import scipy.sparse as sp
    d = ct.DOCP(prob, N, scheme, pattern="structural", device=0)
    n = d.dim_NLP_variables
    lc, uc = ct.constraints_bounds(d)
    lv, uv = ct.variables_bounds(d)
    x0 = np.clip(ct.initial_guess(d), lv, uv)
    sign = -1.0 if d.flags.max else 1.0

    def no_assembly(*a, **k):
        raise AssertionError("hess_coord called")
    d.hess_coord = no_assembly

    def op(x, y, sigma):
        x = np.array(x, dtype=np.float64)
        y = None if y is None else np.array(y, dtype=np.float64)
        mv = lambda p: d.hprod(x, y, np.ravel(p), obj_weight=sigma)       # noqa: E731
        return LinearOperator((n, n), matvec=mv, rmatvec=mv, dtype=np.float64)

    def jac(x):
        jr, jc = d.jac_structure()
        return sp.csr_matrix((d.jac_coord(x), (jr - 1, jc - 1)), shape=(d.dim_NLP_constraints, n))
    con = NonlinearConstraint(lambda x: d.cons(x), lc, uc, jac=jac, hess=lambda x, y: op(x, y, 0.0))
    res = minimize(lambda x: sign * d.obj(x), x0, jac=lambda x: sign * d.grad(x), hess=lambda x: op(x, None, sign),
                   constraints=[con], bounds=Bounds(lv, uv), method="trust-constr",
                   options={"maxiter": 500, "gtol": 1e-8, "xtol": 1e-10})
    c = d.cons(res.x)
    viol = max(float(np.max(np.maximum(lc - c, 0.0))), float(np.max(np.maximum(c - uc, 0.0))))
    return res, sign * res.fun, viol


def test_trust_constr_with_hessian_products():
    res, obj, viol = _trust_constr_hprod("double_integrator_path", "midpoint", 50)
    assert res.status in (1, 2) and viol <= 1e-8 and abs(obj - 1.5) <= 1e-2 * 1.5, (res.status, obj, viol)
    res, obj, viol = _trust_constr_hprod("stagewise_scalar", "gauss_legendre_2", 20)
    assert res.status in (1, 2) and viol <= 1e-8 and abs(obj - 1.0) <= 1e-2, (res.status, obj, viol)
