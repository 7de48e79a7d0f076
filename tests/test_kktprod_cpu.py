"""CPU tests of the fused matrix-free KKT product (ctd_kktprod and ctd_kktprod_dev_async, DOCP.kktprod): the header declares them,
the binding lists them and the library exports them; a host-only handle refuses them with CTD_ENODEVICE before any pointer check;
DOCP.kktprod checks lengths.  The products themselves are checked on the GPU in tests/test_gpu_kktprod.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctdirect_jl_amd as ct

KKT_SYMBOLS = ("ctd_kktprod", "ctd_kktprod_dev_async")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_kktprod_symbols_declared_listed_exported():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(ctd_\w+)\s*\(", f.read()))
    L = ct._lib.lib()
    for name in KKT_SYMBOLS:
        assert name in declared, name
        assert name in ct._lib.SYMBOLS, name
        assert len(ct._lib.SYMBOLS[name][1]) == 10, name
        assert hasattr(L, name), name


def test_host_only_handle_refuses_kktprod_first():
    """CTD_ENODEVICE with valid, with NULL and with aliased pointers; only the NULL handle is checked before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    L = ct._lib.lib()
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x, dx, sx, rx = np.zeros(nvar), np.ones(nvar), np.ones(nvar), np.zeros(nvar)
    y, dy, sc, rc = np.ones(ncon), np.ones(ncon), np.ones(ncon), np.zeros(ncon)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    for name, W in (("ctd_kktprod", P), ("ctd_kktprod_dev_async", V)):
        fn = getattr(L, name)
        valid = (W(x), W(y), 1.0, W(dx), W(dy), W(sx), W(sc), W(rx), W(rc))
        nulls = (None, None, 0.0, None, None, None, None, None, None)
        aliased = (W(x), None, 1.0, W(dx), W(dy), None, None, W(dx), W(dy))
        for a in (valid, nulls, aliased):
            assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, (name, a)
            assert b"host-only" in L.ctd_last_error(d._h), name
            assert L.ctd_last_error(d._h).startswith(name.encode() + b": "), name
        assert fn(None, *valid) == ct._lib.CTD_EINVAL, name
        assert fn(None, *nulls) == ct._lib.CTD_EINVAL, name
    assert not rx.any() and not rc.any()


def test_docp_kktprod_on_host_only_handle_raises():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x, dx, dy = np.zeros(nvar), np.ones(nvar), np.ones(ncon)
    for y, sx, sc in ((np.ones(ncon), np.ones(nvar), np.ones(ncon)), (None, None, None)):
        with pytest.raises(ct.CTDirectError) as ei:
            d.kktprod(x, y, dx, dy, obj_weight=0.5, sx=sx, sc=sc)
        assert ei.value.status == ct._lib.CTD_ENODEVICE


def test_docp_kktprod_checks_lengths():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x, y, dx, dy = np.zeros(nvar), np.ones(ncon), np.ones(nvar), np.ones(ncon)
    bad = [dict(x=np.zeros(nvar + 1)), dict(y=np.ones(ncon - 1)), dict(dx=np.ones(nvar + 1)), dict(dy=np.ones(ncon + 1)),
           dict(dy=None), dict(dx=None), dict(sx=np.ones(nvar - 1)), dict(sc=np.ones(ncon + 2)),
           dict(out=(np.zeros(nvar + 1), np.zeros(ncon))), dict(out=(np.zeros(nvar), np.zeros(ncon - 1)))]
    for kw in bad:
        a = dict(x=x, y=y, dx=dx, dy=dy)
        a.update(kw)
        with pytest.raises(ValueError):
            d.kktprod(a.pop("x"), a.pop("y"), a.pop("dx"), a.pop("dy"), **a)
