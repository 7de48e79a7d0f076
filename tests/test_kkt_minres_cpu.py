"""CPU test of the argument handling of the device-resident MINRES solve (DOCP.kkt_minres, kkt_minres_start, kkt_minres_iters,
kkt_minres_info; ctd_kkt_minres*), on a host-only handle and a host-only shard handle: every vector argument of wrong length raises
the ValueError that names it, a required argument left None raises, only one of px / pc raises, CPU tensors of the right lengths are
stopped only by "not on the handle's GPU", the host path returns CTD_ENODEVICE, and -- through ctypes -- a wrong struct_size returns
CTD_EINVAL before the device is looked at.  The values are checked on the GPU in tests/test_gpu_kkt_minres.py."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import ctdirect_jl_amd as ct

# the vector arguments of DOCP.kkt_minres by keyword: name -> (layout, required); "v": nvar, "c": ncon, "k": nvar + ncon entries
VECS = {"x": ("v", True), "y": ("c", False), "rhs": ("k", True), "sx": ("v", False), "sc": ("c", False), "px": ("v", False),
        "pc": ("c", False), "out": ("k", False)}


@pytest.fixture(scope="module", params=[False, True], ids=["whole", "shard"])
def handle(request):
    kw = {"steps": (3, 7)} if request.param else {}
    return ct.DOCP("goddard", 10, "midpoint", device=-1, **kw)


def sizes(d):
    s = {"v": d.dim_NLP_variables, "c": d.dim_NLP_constraints}
    s["k"] = s["v"] + s["c"]
    return {name: s[lay] for name, (lay, _) in VECS.items()}


def solve(d, a, **kw):
    pre = None if a["px"] is None and a["pc"] is None else (a["px"], a["pc"])
    return d.kkt_minres(a["x"], a["y"], a["rhs"], sx=a["sx"], sc=a["sc"], precond=pre, out=a["out"], **kw)


def test_kkt_minres_checks_its_arguments(handle):
    d = handle
    n = sizes(d)
    tensor = lambda k: torch.ones(k, dtype=torch.float64)      # noqa: E731
    for make in (tensor, np.ones):
        good = {name: make(k) for name, k in n.items()}
        for name, k in n.items():
            for wrong in (k + 1, k - 1):
                with pytest.raises(ValueError, match="^" + re.escape(name) + " ") as ei:
                    solve(d, {**good, name: make(wrong)})
                if not (name == "out" and make is np.ones):     # (a NumPy output: "must be a writeable ... array of n entries")
                    assert f"{name} has {wrong} entries, expected" in str(ei.value), ei.value
                    assert name == "x" or str(ei.value).endswith(f"expected {k}"), ei.value
        for name in ("x", "rhs"):
            with pytest.raises(ValueError, match=f"^{name} is required"):
                solve(d, {**good, name: None})
        for name in ("px", "pc"):
            with pytest.raises(ValueError, match="px and pc are given both"):
                solve(d, {**good, name: None})
        with pytest.raises(ValueError, match="precond is None, a pair"):
            d.kkt_minres(good["x"], good["y"], good["rhs"], precond="jacobi")
    # tensors of the right lengths pass these checks: what stops them here is that they are not on a GPU -- with every optional
    # argument, with none of them, and with the output left to the method
    good = {name: tensor(k) for name, k in n.items()}
    optional = {name: None for name, (_, required) in VECS.items() if not required}
    for args in (good, {**good, **optional}, {**good, "out": None}):
        with pytest.raises(ValueError, match="GPU"):
            solve(d, args)
    # ... and on the host path what stops them is the handle, which has no device
    host = {name: np.ones(k) for name, k in n.items()}
    for args in (host, {**host, **optional}, {**host, "out": None}):
        with pytest.raises(ct.CTDirectError) as ei:
            solve(d, args)
        assert ei.value.status == ct._lib.CTD_ENODEVICE
        assert "ctd_kkt_minres: " in str(ei.value)


def test_enqueue_only_pieces_check_their_arguments(handle):
    d = handle
    n = sizes(d)
    t = {name: torch.ones(k, dtype=torch.float64) for name, k in n.items()}
    z = torch.ones(n["out"], dtype=torch.float64)
    start = lambda a, zz=z: d.kkt_minres_start(a["x"], a["y"], a["rhs"], zz, sx=a["sx"], sc=a["sc"], precond=(a["px"], a["pc"]))  # noqa: E731
    iters = lambda a, zz=z, k=1: d.kkt_minres_iters(a["x"], a["y"], zz, k, sx=a["sx"], sc=a["sc"])                                   # noqa: E731
    for name in ("x", "y", "rhs", "sx", "sc", "px", "pc"):
        bad = {**t, name: torch.ones(n[name] + 1, dtype=torch.float64)}
        with pytest.raises(ValueError, match="^" + name + " has"):
            start(bad)
        if name not in ("rhs", "px", "pc"):
            with pytest.raises(ValueError, match="^" + name + " has"):
                iters(bad)
    for call in (start, iters):
        with pytest.raises(ValueError, match="^z has"):
            call(t, torch.ones(n["out"] - 1, dtype=torch.float64))
        with pytest.raises(ValueError, match="^z is required"):
            call(t, None)
        with pytest.raises(ValueError, match="^x is required"):
            call({**t, "x": None})
        with pytest.raises(ValueError, match="GPU"):
            call(t)
    with pytest.raises(ValueError, match="^rhs is required"):
        start({**t, "rhs": None})
    with pytest.raises(ValueError, match="px and pc are given both"):
        start({**t, "pc": None})
    # NumPy arrays: there is no host path
    with pytest.raises(TypeError, match="must be a device tensor"):
        start({**t, "rhs": np.ones(n["rhs"])})
    with pytest.raises(TypeError, match=re.escape("x must be a device tensor: kkt_minres_iters has no host path")):
        iters({name: (None if a is None else a.numpy()) for name, a in t.items()}, z.numpy())
    with pytest.raises(ct.CTDirectError) as ei:
        d.kkt_minres_info()
    assert ei.value.status == ct._lib.CTD_ENODEVICE


def test_struct_size_is_checked_before_the_device(handle):
    """through ctypes: a NULL handle, a NULL struct and a struct of another size are CTD_EINVAL on a handle without a device; the right
    size then reaches the device check (CTD_ENODEVICE), whose message begins with the entry point"""
    d = handle
    L, lib = ct._lib.lib(), ct._lib
    n = sizes(d)
    x, rhs, z = np.ones(n["x"]), np.ones(n["rhs"]), np.full(n["out"], 7.0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))     # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data)                    # noqa: E731
    ks = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), x=x.ctypes.data, obj_weight=1.0)
    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    calls = {
        "ctd_kkt_minres": lambda h, s, i: L.ctd_kkt_minres(h, s, p(rhs), p(z), 1e-10, 10, 2, i),
        "ctd_kkt_minres_dev": lambda h, s, i: L.ctd_kkt_minres_dev(h, s, vp(rhs), vp(z), 1e-10, 10, 2, i),
        "ctd_kkt_minres_start_dev_async": lambda h, s, i: L.ctd_kkt_minres_start_dev_async(h, s, vp(rhs), vp(z), 1e-10),
        "ctd_kkt_minres_iters_dev_async": lambda h, s, i: L.ctd_kkt_minres_iters_dev_async(h, s, vp(z), 1),
    }
    for name, call in calls.items():
        assert call(None, C.byref(ks), C.byref(info)) == lib.CTD_EINVAL, name
        assert call(d._h, None, C.byref(info)) == lib.CTD_EINVAL, name
        assert L.ctd_last_error(d._h).startswith(name.encode() + b": sys is null"), name
        for wrong in (0, C.sizeof(lib.ctd_kkt_system) - 8, C.sizeof(lib.ctd_kkt_system) + 8):
            bad = lib.ctd_kkt_system(struct_size=wrong, x=x.ctypes.data, obj_weight=1.0)
            assert call(d._h, C.byref(bad), C.byref(info)) == lib.CTD_EINVAL, (name, wrong)
            assert b"struct_size" in L.ctd_last_error(d._h) and L.ctd_last_error(d._h).startswith(name.encode() + b": "), name
        assert call(d._h, C.byref(ks), C.byref(info)) == lib.CTD_ENODEVICE, name
        assert L.ctd_last_error(d._h).startswith(name.encode() + b": "), name
    # the drivers and ctd_kkt_minres_info check the info struct the same way
    for wrong in (0, C.sizeof(lib.ctd_minres_info) + 8):
        bad = lib.ctd_minres_info(struct_size=wrong)
        for name in ("ctd_kkt_minres", "ctd_kkt_minres_dev"):
            assert calls[name](d._h, C.byref(ks), C.byref(bad)) == lib.CTD_EINVAL, name
            assert b"sizeof(ctd_minres_info)" in L.ctd_last_error(d._h), name
        assert L.ctd_kkt_minres_info(d._h, C.byref(bad)) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_info(d._h, None) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_info(None, C.byref(info)) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_info(d._h, C.byref(info)) == lib.CTD_ENODEVICE
    assert (z == 7.0).all()
    # the sizes the header states
    assert C.sizeof(lib.ctd_kkt_system) == 64 and C.sizeof(lib.ctd_minres_info) == 48


def test_the_capped_krylov_geometry_case_reaches_the_cap():
    """the N = 75 000 case of tests/test_gpu_kkt_minres.py is there for the geometry no other case has: 512 workgroups (the cap), a
    chunk above 1024 elements (more passes per thread than the four unrolled ones) and trailing workgroups that own nothing.  The
    rule is restated in Python with the constants read from csrc/ctd_krylov_kernels.hpp, so the case cannot stop exercising this
    unnoticed when the constants move; the handle's sizes are the ones the arithmetic assumes."""
    import test_gpu_kkt_minres as g
    prob, sch, N, rt = g.CAPPED
    assert g.CAPPED in g.CASES and not rt
    d = ct.DOCP(prob, N, sch, device=-1, pattern="structural")
    n = d.dim_NLP_variables + d.dim_NLP_constraints
    d.close()
    assert n == g.CAPPED_N == 525009
    block, span, max_wg = g.krylov_constants()
    nwg, chunk = g.krylov_geom(n)
    assert nwg == max_wg == 512
    assert chunk > 1024 and chunk % block == 0 and chunk > 4 * block           # five passes of 256 threads
    assert (nwg - 1) * chunk >= n                                              # the last workgroup owns nothing ...
    assert g.capped_geometry() == (512, 1280, 411)                             # ... nor do the workgroups 411 to 511
    assert nwg * chunk >= n                                                    # (and the chunks cover the vector)
    # every other case stays below the cap, the largest one spanning several workgroups
    others = [7 * c[2] + 9 for c in g.CASES if c[:2] == ("goddard", "trapeze") and c is not g.CAPPED]
    assert max(g.krylov_geom(k)[0] for k in others) == 14 and all(g.krylov_geom(k)[1] <= span for k in others)
