"""Matrix-free Jacobian products on the MI355X (ctd_jprod / ctd_jtprod, DOCP.jprod / DOCP.jtprod).

J is the STRUCTURAL Jacobian of the constraints: the products are checked entry by entry against J_s v and J_s' w assembled
from the oracle's structural pattern (|got - ref| <= 1e-12 (|J_s| |v|)_i), for every registry problem x every scheme, run-time
OCPs against their own handle's structural Jacobian, the pattern independence (bit-identical across pattern modes and value
orders, and different from the assembled manual-pattern product where that pattern drops entries), bit reproducibility, the
adjoint identity, graph capture, the full-size workloads, a 2^24-step grid without any nnzj-sized array, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe
from jit_defs import FUNCS, catalogue, twin
from oracle.oracle import OracleDOCP

pytestmark = pytest.mark.gpu
RTOL = 1e-12


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def directions(nvar, ncon, seed=3):
    r = np.random.default_rng(seed)
    return r.uniform(-1.0, 1.0, nvar), r.uniform(-1.0, 1.0, ncon)


def csc_products(colptr, rowval, vals, v, w, ncon):
    """J v, J' w and the scales |J| |v|, |J'| |w| of a CSC matrix"""
    nvar = len(colptr) - 1
    cols = np.repeat(np.arange(nvar), np.diff(colptr))
    jv = np.bincount(rowval, weights=vals * v[cols], minlength=ncon)
    sv = np.bincount(rowval, weights=np.abs(vals) * np.abs(v[cols]), minlength=ncon)
    jtw = np.bincount(cols, weights=vals * w[rowval], minlength=nvar)
    sw = np.bincount(cols, weights=np.abs(vals) * np.abs(w[rowval]), minlength=nvar)
    return jv, sv, jtw, sw


def coo_products(rows, cols, vals, v, w, nvar, ncon):
    """the same from the 0-based COO of a handle (jac_structure)"""
    jv = np.bincount(rows, weights=vals * v[cols], minlength=ncon)
    sv = np.bincount(rows, weights=np.abs(vals) * np.abs(v[cols]), minlength=ncon)
    jtw = np.bincount(cols, weights=vals * w[rows], minlength=nvar)
    sw = np.bincount(cols, weights=np.abs(vals) * np.abs(w[rows]), minlength=nvar)
    return jv, sv, jtw, sw


def assert_close(got, ref, scale, what):
    err = np.abs(got - ref)
    bad = err > RTOL * scale + 1e-300
    assert not bad.any(), (what, int(np.argmax(bad)), float(err[bad].max()), int(bad.sum()))


def oracle_ref(prob, sch, N=None, time_grid=None, control_steps=1):
    o = OracleDOCP(prob, sch, N, time_grid=time_grid, control_steps=control_steps)
    o.set_pattern_mode(1)
    return o


def check_against_oracle(torch, prob, sch, N=None, time_grid=None, control_steps=1, pattern="structural"):
    d = ct.DOCP(prob, N if N is not None else len(time_grid) - 1, sch, time_grid=time_grid, device=0, pattern=pattern,
                control_steps=control_steps)
    o = oracle_ref(prob, sch, N, time_grid, control_steps)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    v, w = directions(d.dim_NLP_variables, d.dim_NLP_constraints)
    colptr, rowval = o.jac_pattern()
    jv, sv, jtw, sw = csc_products(colptr, rowval, o.jac_coord(x), v, w, d.dim_NLP_constraints)
    xd, vd, wd = (torch.from_numpy(a).cuda() for a in (x, v, w))
    got_v = d.jprod(xd, vd).cpu().numpy()
    got_t = d.jtprod(xd, wd).cpu().numpy()
    assert_close(got_v, jv, sv, (prob, sch, N, "jprod"))
    assert_close(got_t, jtw, sw, (prob, sch, N, "jtprod"))
    return d, x, v, w, got_v, got_t


REGISTRY = [p for p, pid in ct.PROBLEMS.items() if pid < 1000]      # the compiled registry (run-time OCPs: ids from 1000)
PAIRS = [(p, s) for p in REGISTRY for s in ct.SCHEMES]


@pytest.mark.parametrize("prob,sch", PAIRS)
def test_registry_against_structural_oracle(torch_cuda, prob, sch):
    """every registry problem x every scheme: N = 1, 2, 7 and a grid of several workgroups (jtprod: 256 lanes each)"""
    for N in (1, 2, 7, 300):
        check_against_oracle(torch_cuda, prob, sch, N)


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control", "euler_implicit"])
@pytest.mark.parametrize("prob", ["goddard_all", "double_integrator_freet0tf", "least_squares_with_constraint"])
def test_nonuniform_grid(torch_cuda, prob, sch):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(23))])
    check_against_oracle(torch_cuda, prob, sch, time_grid=tg / tg[-1])


@pytest.mark.parametrize("prob,sch", [("double_integrator_freet0tf", "trapeze"), ("goddard", "trapeze"),
                                      ("goddard_all", "euler_implicit")])
def test_pattern_independence(torch_cuda, prob, sch):
    """REFERENCE_MANUAL handles that drop structural entries (hazard H1; implicit Euler's path rows reading U_{i-1}): their
    products are the structural ones, differ from the assembled manual-pattern product and are bit-identical to the products of
    the STRUCTURAL / OPTIMIZED / CSR handles of the same transcription"""
    torch = torch_cuda
    N = 40
    d, x, v, w, jv, jtw = check_against_oracle(torch, prob, sch, N, pattern="manual")
    assert d.dropped_nonzeros() > 0
    xd, vd, wd = (torch.from_numpy(a).cuda() for a in (x, v, w))
    rows, cols = d.jac_structure()
    vals = d.cons_jac(xd)[1].cpu().numpy()
    mv, _, mt, _ = coo_products(rows - 1, cols - 1, vals, v, w, d.dim_NLP_variables, d.dim_NLP_constraints)
    assert np.abs(mv - jv).max() > 1e-8 * max(1.0, np.abs(jv).max())
    assert np.abs(mt - jtw).max() > 1e-8 * max(1.0, np.abs(jtw).max())
    for kw in (dict(pattern="structural"), dict(pattern="optimized"), dict(pattern="structural", value_order="csr"),
               dict(pattern="manual", value_order="csr")):
        e = ct.DOCP(prob, N, sch, device=0, **kw)
        assert np.array_equal(e.jprod(xd, vd).cpu().numpy(), jv), kw
        assert np.array_equal(e.jtprod(xd, wd).cpu().numpy(), jtw), kw


@pytest.mark.parametrize("prob", ["goddard_all", "double_integrator_path", "quadrotor12"])
@pytest.mark.parametrize("cs", [2, 3])
def test_direct_shooting(torch_cuda, prob, cs):
    for N in (1, 9, 200):
        check_against_oracle(torch_cuda, prob, "midpoint", N, control_steps=cs)


def rt_check(torch, name, sch, N=60, control_steps=1):
    """a run-time OCP against its own handle's structural Jacobian assembled on the host"""
    d = ct.DOCP(name, N, sch, device=0, pattern="structural", control_steps=control_steps)
    r = np.random.default_rng(11)
    x = 0.5 + 0.3 * r.uniform(-1.0, 1.0, d.dim_NLP_variables)
    v, w = directions(d.dim_NLP_variables, d.dim_NLP_constraints, seed=5)
    xd, vd, wd = (torch.from_numpy(a).cuda() for a in (x, v, w))
    rows, cols = d.jac_structure()
    vals = d.cons_jac(xd)[1].cpu().numpy()
    jv, sv, jtw, sw = coo_products(rows - 1, cols - 1, vals, v, w, d.dim_NLP_variables, d.dim_NLP_constraints)
    assert_close(d.jprod(xd, vd).cpu().numpy(), jv, sv, (name, sch, "jprod"))
    assert_close(d.jtprod(xd, wd).cpu().numpy(), jtw, sw, (name, sch, "jtprod"))


@pytest.mark.parametrize("sch", ["trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3_constant_control", "euler",
                                 "euler_implicit"])
@pytest.mark.parametrize("which", ["beam", "bolza_freetf", "double_integrator_tf", "funcs", "quadrotor12_twin"])
def test_runtime_ocps(torch_cuda, which, sch):
    if which == "funcs":
        name = "funcs_rt" if "funcs_rt" in ct.PROBLEMS else ct.register_ocp("funcs_rt", **FUNCS)
    elif which == "quadrotor12_twin":
        name = twin("quadrotor12")
    else:
        name = catalogue(which)[0]
    rt_check(torch_cuda, name, sch)


def test_runtime_direct_shooting(torch_cuda):
    rt_check(torch_cuda, catalogue("beam")[0], "midpoint", N=30, control_steps=4)
    rt_check(torch_cuda, twin("goddard_all"), "midpoint", N=30, control_steps=4)


@pytest.mark.parametrize("prob,sch", [("goddard_all", "gauss_legendre_3"), ("quadrotor12", "gauss_legendre_2"),
                                      ("double_integrator_freet0tf", "trapeze"), ("estimate_rotation_rate", "euler_implicit")])
def test_consistency(torch_cuda, prob, sch):
    """host == device bit for bit, two calls bit-identical, adjoint identity, replay of a captured graph"""
    torch = torch_cuda
    d = ct.DOCP(prob, 500, sch, device=0)
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    v, w = directions(d.dim_NLP_variables, d.dim_NLP_constraints)
    xd, vd, wd = (torch.from_numpy(a).cuda() for a in (x, v, w))
    jv, jtw = d.jprod(xd, vd).cpu().numpy(), d.jtprod(xd, wd).cpu().numpy()
    assert np.array_equal(d.jprod(x, v), jv) and np.array_equal(d.jtprod(x, w), jtw)
    assert np.array_equal(d.jprod(xd, vd).cpu().numpy(), jv) and np.array_equal(d.jtprod(xd, wd).cpu().numpy(), jtw)
    a, b = float(w @ jv), float(jtw @ v)
    assert abs(a - b) <= 1e-12 * max(np.abs(w) @ np.abs(jv), np.abs(jtw) @ np.abs(v)), (a, b)
    # graph capture after one warm call on the capturing stream
    s = torch.cuda.Stream()
    d.set_stream(s)
    ov = torch.empty(d.dim_NLP_constraints, dtype=torch.float64, device="cuda")
    ot = torch.empty(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    with torch.cuda.stream(s):
        d.jprod(xd, vd, out=ov, sync=False)
        d.jtprod(xd, wd, out=ot, sync=False)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        d.jprod(xd, vd, out=ov, sync=False)
        d.jtprod(xd, wd, out=ot, sync=False)
    ov.fill_(0.0)
    ot.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ov.cpu().numpy(), jv) and np.array_equal(ot.cpu().numpy(), jtw)


@pytest.mark.parametrize("prob,sch,N", [("goddard", "gauss_legendre_2", 10_000), ("double_integrator_path", "midpoint", 100_000),
                                        ("quadrotor12", "gauss_legendre_3", 20_000)])
def test_full_size_workloads(torch_cuda, prob, sch, N):
    """bench configs 2, 3 and 5 against the assembled structural product of the same transcription"""
    torch = torch_cuda
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural")
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    v, w = directions(d.dim_NLP_variables, d.dim_NLP_constraints)
    xd, vd, wd = (torch.from_numpy(a).cuda() for a in (x, v, w))
    rows, cols = d.jac_structure()
    vals = d.cons_jac(xd)[1].cpu().numpy()
    jv, sv, jtw, sw = coo_products(rows - 1, cols - 1, vals, v, w, d.dim_NLP_variables, d.dim_NLP_constraints)
    del vals, rows, cols
    assert_close(d.jprod(xd, vd).cpu().numpy(), jv, sv, (prob, sch, N, "jprod"))
    assert_close(d.jtprod(xd, wd).cpu().numpy(), jtw, sw, (prob, sch, N, "jtprod"))


def test_large_grid_without_jacobian(torch_cuda):
    """Goddard, midpoint, N = 2^24: no nnzj-sized array anywhere; c from ctd_cons_jac_dev_async with vals NULL; the adjoint
    identity and a central difference of c against Jv"""
    torch = torch_cuda
    N = 1 << 24
    d = ct.DOCP("goddard", N, "midpoint", device=0)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, "goddard", "midpoint"), perturb=1e-3)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    v = torch.rand(nvar, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    w = torch.rand(ncon, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    jv = d.jprod(x, v)
    jtw = d.jtprod(x, w)
    a, b = float(torch.dot(w, jv)), float(torch.dot(jtw, v))
    assert abs(a - b) <= 1e-12 * max(float(torch.dot(w.abs(), jv.abs())), float(torch.dot(jtw.abs(), v.abs()))), (a, b)
    L = ct._lib.lib()
    eps = 1e-6
    cp = torch.empty(ncon, dtype=torch.float64, device="cuda")
    cm = torch.empty(ncon, dtype=torch.float64, device="cuda")
    for xs, c in ((x + eps * v, cp), (x - eps * v, cm)):
        assert L.ctd_cons_jac_dev_async(d._h, C.c_void_p(xs.data_ptr()), C.c_void_p(c.data_ptr()), None) == 0
        d.sync()
        del xs
    fd = (cp - cm) / (2 * eps)
    rel = float(torch.linalg.norm(fd - jv) / torch.linalg.norm(jv))
    assert rel <= 1e-6, rel


def test_refusals(torch_cuda):
    torch = torch_cuda
    L = ct._lib.lib()
    d = ct.DOCP("goddard", 20, "midpoint", device=0)
    x = torch.zeros(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    v = torch.zeros(d.dim_NLP_variables, dtype=torch.float64, device="cuda")
    o = torch.zeros(d.dim_NLP_constraints, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    assert L.ctd_jprod_dev_async(d._h, P(x), None, P(o)) == ct._lib.CTD_EINVAL
    assert L.ctd_last_error(d._h).startswith(b"ctd_jprod_dev_async: ")
    assert L.ctd_jtprod_dev_async(d._h, None, P(o), P(v)) == ct._lib.CTD_EINVAL
    assert L.ctd_last_error(d._h).startswith(b"ctd_jtprod_dev_async: ")
    assert L.ctd_jprod_dev_async(d._h, P(x), P(v), P(x)) == ct._lib.CTD_EINVAL
    assert b"input" in L.ctd_last_error(d._h)
    assert L.ctd_last_error(d._h).startswith(b"ctd_jprod_dev_async: ")
    # the methods on device tensors: a vector of wrong length is refused by its name
    for call, name in ((lambda: d.jprod(x, v[:-1]), "v"), (lambda: d.jtprod(x, o[:-1]), "w"), (lambda: d.jprod(x, v, out=o[:-1]), "out"),
                       (lambda: d.jprod(x[:-1], v), "x")):
        with pytest.raises(ValueError, match=f"^{name} "):
            call()
    s = ct.DOCP("goddard", 20, "midpoint", device=0, steps=(0, 10))
    assert L.ctd_jprod_dev_async(s._h, P(x), P(v), P(o)) == ct._lib.CTD_EINVAL
    assert b"shard" in L.ctd_last_error(s._h)
    assert L.ctd_last_error(s._h).startswith(b"ctd_jprod_dev_async: ") and b"ctd_jprod_shard_dev_async" in L.ctd_last_error(s._h)
    assert L.ctd_jtprod_dev_async(s._h, P(x), P(o), P(v)) == ct._lib.CTD_EINVAL
    assert L.ctd_last_error(s._h).startswith(b"ctd_jtprod_dev_async: ") and b"ctd_jtprod_shard_dev_async" in L.ctd_last_error(s._h)
