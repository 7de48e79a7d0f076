"""CPU tests of the matrix-free Jacobian products (ctd_jprod / ctd_jtprod and their _dev_async forms, DOCP.jprod / DOCP.jtprod):
the header declares them, the binding lists them and the library exports them; a host-only handle refuses them with CTD_ENODEVICE
before any other check.  The products themselves are checked on the GPU in tests/test_gpu_products.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctdirect_jl_amd as ct

PROD_SYMBOLS = ("ctd_jprod", "ctd_jtprod", "ctd_jprod_dev_async", "ctd_jtprod_dev_async")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_product_symbols_declared_listed_exported():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(ctd_\w+)\s*\(", f.read()))
    L = ct._lib.lib()
    for name in PROD_SYMBOLS:
        assert name in declared, name
        assert name in ct._lib.SYMBOLS, name
        assert hasattr(L, name), name


def test_host_only_handle_refuses_products_first():
    """CTD_ENODEVICE with valid and with NULL pointers; only the NULL handle is checked before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    L = ct._lib.lib()
    x = np.zeros(d.dim_NLP_variables)
    v = np.ones(d.dim_NLP_variables)
    w = np.ones(d.dim_NLP_constraints)
    outc = np.zeros(d.dim_NLP_constraints)
    outv = np.zeros(d.dim_NLP_variables)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    valid = {
        "ctd_jprod": (P(x), P(v), P(outc)),
        "ctd_jtprod": (P(x), P(w), P(outv)),
        "ctd_jprod_dev_async": (V(x), V(v), V(outc)),
        "ctd_jtprod_dev_async": (V(x), V(w), V(outv)),
    }
    for name, args in valid.items():
        fn = getattr(L, name)
        for a in (args, (None, None, None)):
            assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, (name, a)
            assert b"host-only" in L.ctd_last_error(d._h), name
            assert L.ctd_last_error(d._h).startswith(name.encode() + b": "), name
        assert fn(None, *args) == ct._lib.CTD_EINVAL, name
        assert fn(None, None, None, None) == ct._lib.CTD_EINVAL, name


def test_docp_products_on_host_only_handle_raise():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    x = np.zeros(d.dim_NLP_variables)
    for call in (lambda: d.jprod(x, np.ones(d.dim_NLP_variables)), lambda: d.jtprod(x, np.ones(d.dim_NLP_constraints))):
        with pytest.raises(ct.CTDirectError) as ei:
            call()
        assert ei.value.status == ct._lib.CTD_ENODEVICE
