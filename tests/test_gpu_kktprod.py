"""The fused matrix-free KKT product on the MI355X (ctd_kktprod / ctd_kktprod_dev_async, DOCP.kktprod):

    rx = (obj_weight d2 f + sum_r y_r d2 c_r) dx + J' dy + sx o dx,        rc = J dx - sc o dy.

The bars are those of the separate products, entry by entry:
  bottom block  |rc - ref| <= 1e-12 (|J_s| |dx| + |sc| |dy|)                                         (test_gpu_products.py)
  top block     |rx - ref| <= 1e-10 max(1, sum_j max(1, |H_ij|, |H^{|y|,|obj_weight|}_ij|) |dx_j|)     (test_gpu_hprod.py)
                              + 1e-12 (|J_s|' |dy| + |sx| |dx|)
References: H and J assembled on the CPU from the oracle in structural mode (where the reference's Euler Hessian pattern leaves
true nonzeros out, the top block is checked against hprod + jtprod + sx o dx of the same handle), the 50-digit Hessian goldens, the
structural hess_coord / jac_coord of run-time OCPs' own handles.  Also: optional arguments, bit reproducibility (two calls, host ==
device, every pattern mode / value order, halves of one buffer), symmetry of the operator, graph capture, the refusals, and scipy's
minres solving K z = r through the operator alone.  Bit equality with hprod / jprod is not required: the fused sink rounds
differently."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import LinearOperator, minres

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe, hess_golden_files, load_hess_golden
from jit_defs import twin
from oracle.oracle import OracleDOCP

pytestmark = pytest.mark.gpu
HTOL, JTOL = 1e-10, 1e-12


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


class Inputs:
    """seeded inputs of one transcription: directions uniform(-1, 1), sx uniform(0, 1), sc uniform(0, 1e-2)"""
    def __init__(self, nvar, ncon, seed=3):
        r = np.random.default_rng(seed)
        self.dx, self.dy, self.y = r.uniform(-1.0, 1.0, nvar), r.uniform(-1.0, 1.0, ncon), r.uniform(-1.0, 1.0, ncon)
        self.sx, self.sc = r.uniform(0.0, 1.0, nvar), r.uniform(0.0, 1e-2, ncon)


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


def assemble(H, Hs, J, dx, dy, sx, sc):
    """reference blocks and their bars from H = (rows, cols, vals) lower triangle, Hs = its entry scales, J = (rows, cols, vals)"""
    nvar, ncon = len(dx), len(dy)
    sx = np.zeros(nvar) if sx is None else sx
    sc = np.zeros(ncon) if sc is None else sc
    hr, hc, hv = H
    jr, jc, jv = J
    hdx = sym_product(hr, hc, hv, dx, nvar)
    hbar = HTOL * np.maximum(1.0, sym_product(hr, hc, Hs, np.abs(dx), nvar))
    jdx = np.bincount(jr, weights=jv * dx[jc], minlength=ncon)
    jtdy = np.bincount(jc, weights=jv * dy[jr], minlength=nvar)
    jbar_c = JTOL * (np.bincount(jr, weights=np.abs(jv) * np.abs(dx[jc]), minlength=ncon) + np.abs(sc) * np.abs(dy))
    jbar_x = JTOL * (np.bincount(jc, weights=np.abs(jv) * np.abs(dy[jr]), minlength=nvar) + np.abs(sx) * np.abs(dx))
    return hdx + jtdy + sx * dx, hbar + jbar_x, jdx - sc * dy, jbar_c + 1e-300


def oracle_blocks(o, x, y, sigma, dx, dy, sx, sc):
    """reference and bars from the oracle in structural mode; + the number of true nonzeros its Hessian pattern leaves out"""
    yo = np.zeros(len(dy)) if y is None else y
    hr, hc = csc_coo(*o.hess_pattern())
    vals, dropped = o.hess_coord(x, yo, sigma, return_dropped=True)
    mag = o.hess_coord(x, np.abs(yo), abs(sigma))
    jr, jc = csc_coo(*o.jac_pattern())
    return assemble((hr, hc, vals), entry_scale(vals, mag), (jr, jc, o.jac_coord(x)), dx, dy, sx, sc) + (dropped[1],)


def assert_block(got, ref, bar, what):
    err = np.abs(got - ref)
    bad = err > bar
    print(what, "max err / bar", float(np.max(err / bar)))
    assert not bad.any(), (what, int(np.argmax(bad)), float(err[bad].max()), int(bad.sum()))


def dev(torch, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def fused(torch, d, x, y, sigma, dx, dy, sx, sc):
    xd, yd, dxd, dyd, sxd, scd = dev(torch, x, y, dx, dy, sx, sc)
    rx, rc = d.kktprod(xd, yd, dxd, dyd, obj_weight=sigma, sx=sxd, sc=scd)
    return rx.cpu().numpy(), rc.cpu().numpy()


def check_against_oracle(torch, d, o, x, y, sigma, w, what, sx=True, sc=True):
    sx, sc = (w.sx if sx else None), (w.sc if sc else None)
    rx_ref, rx_bar, rc_ref, rc_bar, dropped = oracle_blocks(o, x, y, sigma, w.dx, w.dy, sx, sc)
    rx, rc = fused(torch, d, x, y, sigma, w.dx, w.dy, sx, sc)
    assert_block(rc, rc_ref, rc_bar, what + ("rc",))
    if dropped:
        # the reference's pattern leaves true nonzeros of H out: the top block against the unchanged products of the same handle
        z = np.zeros(len(w.dx)) if sx is None else sx
        rx_ref = d.hprod(x, y, w.dx, obj_weight=sigma) + d.jtprod(x, w.dy) + z * w.dx
    assert_block(rx, rx_ref, rx_bar, what + ("rx",))
    return rx, rc


REGISTRY = [p for p, pid in ct.PROBLEMS.items() if pid < 1000]      # the compiled registry (run-time OCPs: ids from 1000)
PAIRS = [(p, s) for p in REGISTRY for s in ct.SCHEMES]


# ---- 1. every registry problem x every scheme against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", PAIRS)
def test_registry_against_oracle(torch_cuda, prob, sch):
    """N = 1 (one step), 2 (first and last node adjacent), 7 (odd interior grid), 300 (several 256-lane workgroups: the partial
    sums and the ordered finish take part); at N = 7 also obj_weight = 0 and y = None"""
    for N in (1, 2, 7, 300):
        d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints)
        check_against_oracle(torch_cuda, d, o, x, w.y, 0.7, w, (prob, sch, N))
        if N == 7:
            check_against_oracle(torch_cuda, d, o, x, w.y, 0.0, w, (prob, sch, N, "obj_weight 0"))
            check_against_oracle(torch_cuda, d, o, x, None, 1.3, w, (prob, sch, N, "y None"))


# ---- 2. 50-digit goldens -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", hess_golden_files(), ids=lambda p: p.split("/")[-1][:-5])
def test_golden_hessians(torch_cuda, path):
    """H of the fixture (exact, 50 digits, with the nonzeros a pattern may leave out), J of the oracle"""
    g = load_hess_golden(path)
    cs = g.get("control_steps", 1)
    prob = twin(g["problem"]) if cs > 3 else g["problem"]
    d = ct.DOCP(prob, g["grid_size"], g["scheme"], time_grid=g["time_grid"], device=0, control_steps=cs)
    w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints, seed=17)
    keys = list(g["H"])
    rows = np.array([k[0] for k in keys], dtype=np.int64)
    cols = np.array([k[1] for k in keys], dtype=np.int64)
    vals = np.array([g["H"][k] for k in keys])
    o = OracleDOCP(g["problem"], g["scheme"], g["grid_size"], time_grid=g["time_grid"], control_steps=cs)
    o.set_pattern_mode(1)
    x, y, sigma = g["xu"], g["y"], g["obj_weight"]
    jr, jc = csc_coo(*o.jac_pattern())
    rx_ref, rx_bar, rc_ref, rc_bar = assemble((rows, cols, vals), np.maximum(1.0, np.abs(vals)), (jr, jc, o.jac_coord(x)),
                                              w.dx, w.dy, w.sx, w.sc)
    # the bar of test_gpu_hprod.py's golden test: the larger of the fixture's and the oracle's entry scales
    _, obar, _, _, _ = oracle_blocks(o, x, y, sigma, w.dx, w.dy, w.sx, w.sc)
    rx, rc = fused(torch_cuda, d, x, y, sigma, w.dx, w.dy, w.sx, w.sc)
    assert_block(rc, rc_ref, rc_bar, (path, "rc"))
    assert_block(rx, rx_ref, np.maximum(rx_bar, obar), (path, "rx"))


# ---- 3. free times, path rows, non-uniform grid, several controls per step ---------------------------------------------------------
@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control"])
@pytest.mark.parametrize("prob", ["goddard_all", "double_integrator_freet0tf"])
def test_nonuniform_grid(torch_cuda, prob, sch):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(23))])
    tg = tg / tg[-1]
    d = ct.DOCP(prob, len(tg) - 1, sch, time_grid=tg, device=0)
    o = OracleDOCP(prob, sch, None, time_grid=tg)
    o.set_pattern_mode(1)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints)
    check_against_oracle(torch_cuda, d, o, x, w.y, 0.7, w, (prob, sch))


CS_FIXTURES = [p for p in hess_golden_files() if load_hess_golden(p).get("control_steps", 1) in (2, 3)]


@pytest.mark.parametrize("path", CS_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_direct_shooting(torch_cuda, path):
    """the transcriptions of the cs* fixtures with 2 and 3 controls per step, at seeded inputs"""
    g = load_hess_golden(path)
    cs = g["control_steps"]
    d = ct.DOCP(g["problem"], g["grid_size"], g["scheme"], time_grid=g["time_grid"], device=0, control_steps=cs)
    o = OracleDOCP(g["problem"], g["scheme"], g["grid_size"], time_grid=g["time_grid"], control_steps=cs)
    o.set_pattern_mode(1)
    x = bench_inputs(describe(d, g["problem"], g["scheme"]), perturb=1e-3)
    w = Inputs(d.dim_NLP_variables, d.dim_NLP_constraints)
    check_against_oracle(torch_cuda, d, o, x, w.y, 0.7, w, (path,))


# ---- 4. run-time OCPs ----------------------------------------------------------------------------------------------------------
def handle_blocks(torch, d, x, y, sigma, w):
    """reference and bars from the handle's own structural hess_coord / jac_coord"""
    xd, yd = dev(torch, x, y)
    hr, hc = d.hess_structure()
    vals = d.hess_coord(xd, yd, sigma).cpu().numpy()
    mag = d.hess_coord(xd, torch.abs(yd), abs(sigma)).cpu().numpy()
    jr, jc = d.jac_structure()
    jv = d.cons_jac(xd)[1].cpu().numpy()
    return assemble((hr - 1, hc - 1, vals), entry_scale(vals, mag), (jr - 1, jc - 1, jv), w.dx, w.dy, w.sx, w.sc)


def rt_case(name, sch, N, control_steps=1):
    d = ct.DOCP(name, N, sch, device=0, pattern="structural", control_steps=control_steps)
    x = 0.5 + 0.3 * np.random.default_rng(11).uniform(-1.0, 1.0, d.dim_NLP_variables)
    return d, x, Inputs(d.dim_NLP_variables, d.dim_NLP_constraints, seed=5)


def rt_check(torch, name, sch, N=40, control_steps=1):
    d, x, w = rt_case(name, sch, N, control_steps)
    rx_ref, rx_bar, rc_ref, rc_bar = handle_blocks(torch, d, x, w.y, 0.6, w)
    rx, rc = fused(torch, d, x, w.y, 0.6, w.dx, w.dy, w.sx, w.sc)
    assert_block(rc, rc_ref, rc_bar, (name, sch, "rc"))
    assert_block(rx, rx_ref, rx_bar, (name, sch, "rx"))


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2"])
@pytest.mark.parametrize("prob", ["goddard", "goddard_all"])
def test_runtime_twins(torch_cuda, prob, sch):
    rt_check(torch_cuda, twin(prob), sch)


def test_runtime_four_controls_per_step(torch_cuda):
    """control_steps = 4: beyond what the registry compiles in"""
    rt_check(torch_cuda, twin("goddard_all"), "midpoint", N=30, control_steps=4)


# ---- 5. optional arguments -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard_all", "trapeze"), ("double_integrator_freet0tf", "gauss_legendre_2"),
                                      ("least_squares_with_constraint", "euler")])
def test_optional_arguments(torch_cuda, prob, sch):
    d = ct.DOCP(prob, 300, sch, device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    w = Inputs(nvar, ncon)
    full = fused(torch_cuda, d, x, w.y, 0.7, w.dx, w.dy, w.sx, w.sc)
    for none, zero in ((dict(sx=None), dict(sx=np.zeros(nvar))), (dict(sc=None), dict(sc=np.zeros(ncon))),
                       (dict(y=None), dict(y=np.zeros(ncon)))):
        a = dict(y=w.y, sx=w.sx, sc=w.sc)
        b = dict(a)
        a.update(none)
        b.update(zero)
        ra = fused(torch_cuda, d, x, a["y"], 0.7, w.dx, w.dy, a["sx"], a["sc"])
        rb = fused(torch_cuda, d, x, b["y"], 0.7, w.dx, w.dy, b["sx"], b["sc"])
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), none
        assert not (np.array_equal(ra[0], full[0]) and np.array_equal(ra[1], full[1])), none     # (the argument has an effect)
        ha = d.kktprod(x, a["y"], w.dx, w.dy, obj_weight=0.7, sx=a["sx"], sc=a["sc"])             # host entry point, NULL pointers
        assert np.array_equal(ha[0], ra[0]) and np.array_equal(ha[1], ra[1]), none


# ---- 6. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("quadrotor12", "gauss_legendre_2"),
                                      ("double_integrator_freet0tf", "trapeze"), ("estimate_rotation_rate", "euler_implicit"),
                                      ("double_integrator_path", "midpoint")])
def test_reproducible_host_device_one_buffer(torch_cuda, prob, sch):
    """two calls, host == device, and dx|dy, rx|rc as halves of one tensor whose second half is only 8-byte aligned"""
    torch = torch_cuda
    N = 300
    d = ct.DOCP(prob, N, sch, device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    if nvar % 2 == 0:       # an odd nvar puts the second half of a 16-byte aligned buffer at 8 bytes
        N += 1
        d = ct.DOCP(prob, N, sch, device=0)
        nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    w = Inputs(nvar, ncon)
    rx, rc = fused(torch, d, x, w.y, 0.7, w.dx, w.dy, w.sx, w.sc)
    rx2, rc2 = fused(torch, d, x, w.y, 0.7, w.dx, w.dy, w.sx, w.sc)
    assert np.array_equal(rx, rx2) and np.array_equal(rc, rc2)
    hx, hc = d.kktprod(x, w.y, w.dx, w.dy, obj_weight=0.7, sx=w.sx, sc=w.sc)
    assert np.array_equal(rx, hx) and np.array_equal(rc, hc)
    assert nvar % 2 == 1
    xd, yd, sxd, scd = dev(torch, x, w.y, w.sx, w.sc)
    z = torch.from_numpy(np.r_[w.dx, w.dy]).cuda()
    r = torch.zeros(nvar + ncon, dtype=torch.float64, device="cuda")
    assert z.data_ptr() % 16 == 0 and z[nvar:].data_ptr() % 16 == 8
    d.kktprod(xd, yd, z[:nvar], z[nvar:], obj_weight=0.7, sx=sxd, sc=scd, out=(r[:nvar], r[nvar:]))
    r = r.cpu().numpy()
    assert np.array_equal(r[:nvar], rx) and np.array_equal(r[nvar:], rc)


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
        results.append(fused(torch_cuda, d, x, w.y, 0.7, w.dx, w.dy, w.sx, w.sc))
    for rx, rc in results[1:]:
        assert np.array_equal(rx, results[0][0]) and np.array_equal(rc, results[0][1])


# ---- 7. symmetry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("double_integrator_freet0tf", "trapeze"),
                                      ("quadrotor", "euler_implicit"), ("least_squares_with_constraint", "midpoint")])
def test_symmetry(torch_cuda, prob, sch):
    """K = [[H + Sx, J'], [J, -Sc]] is symmetric: <K a, b> = <a, K b> for two random vectors a = (dx, dy), b, to the entry bars of
    the two products summed against the other vector"""
    N = 300
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    o = OracleDOCP(prob, sch, N)
    o.set_pattern_mode(1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    a, b = Inputs(nvar, ncon, seed=3), Inputs(nvar, ncon, seed=8)
    ka = fused(torch_cuda, d, x, a.y, 0.7, a.dx, a.dy, a.sx, a.sc)
    kb = fused(torch_cuda, d, x, a.y, 0.7, b.dx, b.dy, a.sx, a.sc)
    _, bax, _, bac, _ = oracle_blocks(o, x, a.y, 0.7, a.dx, a.dy, a.sx, a.sc)
    _, bbx, _, bbc, _ = oracle_blocks(o, x, a.y, 0.7, b.dx, b.dy, a.sx, a.sc)
    lhs = float(ka[0] @ b.dx + ka[1] @ b.dy)
    rhs = float(a.dx @ kb[0] + a.dy @ kb[1])
    bar = float(bax @ np.abs(b.dx) + bac @ np.abs(b.dy) + bbx @ np.abs(a.dx) + bbc @ np.abs(a.dy))
    print((prob, sch), "asymmetry / bar", abs(lhs - rhs) / bar)
    assert abs(lhs - rhs) <= bar, (lhs, rhs, bar)


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------------
def capture_case(torch, d, x, w):
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    xd, yd, dxd, dyd, sxd, scd = dev(torch, x, w.y, w.dx, w.dy, w.sx, w.sc)
    rx, rc = d.kktprod(xd, yd, dxd, dyd, obj_weight=0.7, sx=sxd, sc=scd)          # eager, and the warm call
    rx, rc = rx.cpu().numpy(), rc.cpu().numpy()
    s = torch.cuda.Stream()
    d.set_stream(s)
    ox = torch.empty(nvar, dtype=torch.float64, device="cuda")
    oc = torch.empty(ncon, dtype=torch.float64, device="cuda")
    with torch.cuda.stream(s):
        d.kktprod(xd, yd, dxd, dyd, obj_weight=0.7, sx=sxd, sc=scd, out=(ox, oc), sync=False)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        d.kktprod(xd, yd, dxd, dyd, obj_weight=0.7, sx=sxd, sc=scd, out=(ox, oc), sync=False)
    ox.fill_(0.0)
    oc.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ox.cpu().numpy(), rx) and np.array_equal(oc.cpu().numpy(), rc)


def test_graph_capture(torch_cuda):
    prob, sch = "goddard_all", "gauss_legendre_2"
    d = ct.DOCP(prob, 300, sch, device=0)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    capture_case(torch_cuda, d, x, Inputs(d.dim_NLP_variables, d.dim_NLP_constraints))


def test_graph_capture_runtime_ocp(torch_cuda):
    d, x, w = rt_case(twin("goddard_all"), "midpoint", 40)
    capture_case(torch_cuda, d, x, w)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    E = ct._lib.CTD_EINVAL
    d = ct.DOCP("goddard", 20, "midpoint", device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda")        # noqa: E731
    x, dx, sx, rx = t(nvar, 1.0), t(nvar, 0.5), t(nvar, 0.25), t(nvar, 7.0)
    y, dy, sc, rc = t(ncon, 1.0), t(ncon, 0.5), t(ncon, 0.25), t(ncon, 7.0)
    P = lambda a: C.c_void_p(a.data_ptr())        # noqa: E731
    fn = L.ctd_kktprod_dev_async
    good = dict(x=x, y=y, dx=dx, dy=dy, sx=sx, sc=sc, rx=rx, rc=rc)

    def call(h, **kw):
        a = dict(good)
        a.update(kw)
        p = {k: (None if v is None else P(v)) for k, v in a.items()}
        return fn(h, p["x"], p["y"], 1.0, p["dx"], p["dy"], p["sx"], p["sc"], p["rx"], p["rc"])

    def untouched():
        d.sync()
        return bool((rx == 7.0).all()) and bool((rc == 7.0).all())

    for name in ("x", "dx", "dy", "rx", "rc"):
        assert call(d._h, **{name: None}) == E, name
        assert b"null" in L.ctd_last_error(d._h), name
        assert L.ctd_last_error(d._h).startswith(b"ctd_kktprod_dev_async: "), name
        assert untouched(), name
    # every output against every input (same-length pairs and, through raw pointers, the others too), and rx == rc
    for out in ("rx", "rc"):
        for inp in ("x", "y", "dx", "dy", "sx", "sc"):
            before = good[inp].clone()
            assert call(d._h, **{out: good[inp]}) == E, (out, inp)
            assert b"input" in L.ctd_last_error(d._h), (out, inp)
            assert L.ctd_last_error(d._h).startswith(b"ctd_kktprod_dev_async: "), (out, inp)
            d.sync()
            assert torch.equal(good[inp], before) and untouched(), (out, inp)
    assert call(d._h, rc=rx) == E
    assert b"rx and rc" in L.ctd_last_error(d._h)
    assert L.ctd_last_error(d._h).startswith(b"ctd_kktprod_dev_async: ")
    assert untouched()
    # shard handles: a range of steps, and a whole-grid handle with an x-shard table
    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(0, 10))
    assert call(s._h) == E
    assert b"shard" in L.ctd_last_error(s._h) and b"out of scope" in L.ctd_last_error(s._h)
    assert L.ctd_last_error(s._h).startswith(b"ctd_kktprod_dev_async: ") and b"ctd_kktprod_shard_dev_async" in L.ctd_last_error(s._h)
    assert untouched()
    sh = ct.DOCP("goddard", 20, "midpoint", device=0)
    sh.set_x_shards([0, 20], [x.data_ptr()], 0)
    assert call(sh._h) == E
    assert b"shard" in L.ctd_last_error(sh._h)
    assert untouched()
    # the optional ones may be NULL
    assert call(d._h, y=None, sx=None, sc=None) == 0
    d.sync()
    assert not untouched()


# ---- 10. a Krylov solve through the operator alone -----------------------------------------------------------------------------------
def test_minres_through_the_operator(torch_cuda):
    """scipy's minres on K z = r with K given only as DOCP.kktprod (device tensors); accepted on the residual under the matrix
    assembled independently from the oracle's H and J and the diagonals: |K_asm z - r| <= 1e-8 |r| (the solver's rtol 1e-10 with
    two orders of margin; operator and matrix differ at the 1e-12 level).  The transcription (double integrator with a path
    constraint, midpoint, N = 20: 127 unknowns) and the diagonals (uniform(1, 2)) were chosen on the CPU: minres on K_asm itself
    reaches rtol 1e-10 in 47 iterations (cond(K_asm) = 2.6, true residual 8.7e-10 |r|), within the cap of 10 (nvar + ncon)
    asserted here; with sc of order 1e-2 the same solve stops at a true residual of 6e-8 |r|, above the acceptance."""
    import scipy.sparse as sp
    torch = torch_cuda
    prob, sch, N = "double_integrator_path", "midpoint", 20
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    o = OracleDOCP(prob, sch, N)
    o.set_pattern_mode(1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
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
    xd, yd, sxd, scd = dev(torch, x, y, sx, sc)
    zin = torch.empty(nvar + ncon, dtype=torch.float64, device="cuda")
    zout = torch.empty(nvar + ncon, dtype=torch.float64, device="cuda")
    calls = [0]

    def matvec(z):
        calls[0] += 1
        zin.copy_(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64).ravel()))
        d.kktprod(xd, yd, zin[:nvar], zin[nvar:], obj_weight=1.0, sx=sxd, sc=scd, out=(zout[:nvar], zout[nvar:]))
        return zout.cpu().numpy()

    cap = 10 * (nvar + ncon)
    its = [0]
    K = LinearOperator((nvar + ncon, nvar + ncon), matvec=matvec, rmatvec=matvec, dtype=np.float64)
    z, info = minres(K, rhs, rtol=1e-10, maxiter=cap, callback=lambda zk: its.__setitem__(0, its[0] + 1))
    res = float(np.linalg.norm(K_asm @ z - rhs) / np.linalg.norm(rhs))
    print("minres info", info, "iterations", its[0], "operator calls", calls[0], "residual under K_asm", res)
    assert info == 0 and 0 < its[0] <= cap, (info, its[0], cap)
    assert res <= 1e-8, res
