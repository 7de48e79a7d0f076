"""CPU tests of the matrix-free KKT diagonals (ctd_hdiag, ctd_jsq_rows, ctd_jsq_cols and their _dev_async forms; DOCP.hdiag,
DOCP.jsq_rows, DOCP.jsq_cols, DOCP.kkt_diag_precond): the header declares them, the binding lists them with the right arity and the
library exports them; a host-only handle refuses them with CTD_ENODEVICE before any pointer check; a null handle gives CTD_EINVAL;
the DOCP methods check lengths.  The values are checked on the GPU in tests/test_gpu_diag.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctdirect_jl_amd as ct

# name -> number of arguments
DIAG_SYMBOLS = {"ctd_hdiag": 5, "ctd_hdiag_dev_async": 5, "ctd_jsq_rows": 4, "ctd_jsq_rows_dev_async": 4, "ctd_jsq_cols": 4,
                "ctd_jsq_cols_dev_async": 4}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_diag_symbols_declared_listed_exported():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(ctd_\w+)\s*\(", f.read()))
    L = ct._lib.lib()
    for name, arity in DIAG_SYMBOLS.items():
        assert name in declared, name
        assert name in ct._lib.SYMBOLS, name
        assert len(ct._lib.SYMBOLS[name][1]) == arity, name
        assert hasattr(L, name), name


def test_host_only_handle_refuses_diag_first():
    """CTD_ENODEVICE with valid, with NULL and with aliased pointers; only the NULL handle is checked before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    L = ct._lib.lib()
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x, wx, ov = np.zeros(nvar), np.ones(nvar), np.zeros(nvar)
    y, oc = np.ones(ncon), np.zeros(ncon)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    for suffix, W in (("", P), ("_dev_async", V)):
        cases = {"ctd_hdiag": ((W(x), W(y), 1.0, W(ov)), (None, None, 0.0, None), (W(x), W(y), 1.0, W(x))),
                 "ctd_jsq_rows": ((W(x), W(wx), W(oc)), (None, None, None), (W(x), W(wx), W(wx))),
                 "ctd_jsq_cols": ((W(x), W(y), W(ov)), (None, None, None), (W(x), None, W(x)))}
        for base, (valid, nulls, aliased) in cases.items():
            fn = getattr(L, base + suffix)
            for a in (valid, nulls, aliased):
                assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, (base + suffix, a)
                assert b"host-only" in L.ctd_last_error(d._h), base + suffix
                assert L.ctd_last_error(d._h).startswith((base + suffix).encode() + b": "), base + suffix
            assert fn(None, *valid) == ct._lib.CTD_EINVAL, base + suffix
            assert fn(None, *nulls) == ct._lib.CTD_EINVAL, base + suffix
    assert not ov.any() and not oc.any() and not x.any() and (wx == 1.0).all()


def test_docp_diag_on_host_only_handle_raises():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = np.zeros(nvar)
    calls = [lambda: d.hdiag(x, np.ones(ncon), obj_weight=0.5), lambda: d.hdiag(x, None), lambda: d.jsq_rows(x, np.ones(nvar)),
             lambda: d.jsq_rows(x), lambda: d.jsq_cols(x, np.ones(ncon)), lambda: d.jsq_cols(x),
             lambda: d.kkt_diag_precond(x, np.ones(ncon), sx=np.ones(nvar), sc=np.ones(ncon)), lambda: d.kkt_diag_precond(x, None)]
    for call in calls:
        with pytest.raises(ct.CTDirectError) as ei:
            call()
        assert ei.value.status == ct._lib.CTD_ENODEVICE


def test_docp_diag_checks_lengths():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x, y, wx = np.zeros(nvar), np.ones(ncon), np.ones(nvar)
    bad = [lambda: d.hdiag(np.zeros(nvar + 1), y), lambda: d.hdiag(x, np.ones(ncon - 1)), lambda: d.hdiag(x, y, out=np.zeros(nvar + 1)),
           lambda: d.hdiag(x, None, out=np.zeros(ncon)),
           lambda: d.jsq_rows(np.zeros(nvar - 1)), lambda: d.jsq_rows(x, np.ones(nvar + 1)), lambda: d.jsq_rows(x, y),
           lambda: d.jsq_rows(x, wx, out=np.zeros(ncon + 1)), lambda: d.jsq_rows(x, out=np.zeros(nvar)),
           lambda: d.jsq_cols(np.zeros(nvar + 2)), lambda: d.jsq_cols(x, np.ones(ncon + 1)), lambda: d.jsq_cols(x, wx),
           lambda: d.jsq_cols(x, y, out=np.zeros(nvar - 1)), lambda: d.jsq_cols(x, out=np.zeros(ncon)),
           lambda: d.kkt_diag_precond(np.zeros(nvar + 1), y), lambda: d.kkt_diag_precond(x, np.ones(ncon + 1))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
