"""CPU tests of the matrix-free Hessian products (ctd_hprod and ctd_hprod_dev_async, DOCP.hprod): the header declares them, the
binding lists them and the library exports them; a host-only handle refuses them with CTD_ENODEVICE before any other check.  The
products themselves are checked on the GPU in tests/test_gpu_hprod.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctdirect_jl_amd as ct

HPROD_SYMBOLS = ("ctd_hprod", "ctd_hprod_dev_async")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_hprod_symbols_declared_listed_exported():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(ctd_\w+)\s*\(", f.read()))
    L = ct._lib.lib()
    for name in HPROD_SYMBOLS:
        assert name in declared, name
        assert name in ct._lib.SYMBOLS, name
        assert hasattr(L, name), name


def test_host_only_handle_refuses_hprod_first():
    """CTD_ENODEVICE with valid and with NULL pointers; only the NULL handle is checked before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    L = ct._lib.lib()
    x = np.zeros(d.dim_NLP_variables)
    v = np.ones(d.dim_NLP_variables)
    y = np.ones(d.dim_NLP_constraints)
    out = np.zeros(d.dim_NLP_variables)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    valid = {
        "ctd_hprod": (P(x), P(y), 1.0, P(v), P(out)),
        "ctd_hprod_dev_async": (V(x), V(y), 1.0, V(v), V(out)),
    }
    for name, args in valid.items():
        fn = getattr(L, name)
        for a in (args, (None, None, 0.0, None, None), (args[0], None, 1.0, args[3], args[4])):
            assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, (name, a)
            assert b"host-only" in L.ctd_last_error(d._h), name
            assert L.ctd_last_error(d._h).startswith(name.encode() + b": "), name
        assert fn(None, *args) == ct._lib.CTD_EINVAL, name
        assert fn(None, None, None, 1.0, None, None) == ct._lib.CTD_EINVAL, name


def test_docp_hprod_on_host_only_handle_raises():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    x = np.zeros(d.dim_NLP_variables)
    v = np.ones(d.dim_NLP_variables)
    for y in (np.ones(d.dim_NLP_constraints), None):
        with pytest.raises(ct.CTDirectError) as ei:
            d.hprod(x, y, v, obj_weight=0.5)
        assert ei.value.status == ct._lib.CTD_ENODEVICE


def test_docp_hprod_checks_lengths():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    x = np.zeros(d.dim_NLP_variables)
    with pytest.raises(ValueError):
        d.hprod(x, None, np.ones(d.dim_NLP_variables + 1))
    with pytest.raises(ValueError):
        d.hprod(x, np.ones(d.dim_NLP_constraints - 1), np.ones(d.dim_NLP_variables))
