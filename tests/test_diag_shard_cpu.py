"""CPU tests of the matrix-free KKT diagonals on time-step shards (ctd_hdiag_shard_dev_async, ctd_jsq_rows_shard_dev_async,
ctd_jsq_cols_shard_dev_async; DOCP.hdiag_shard / jsq_rows_shard / jsq_cols_shard), in the manner of test_products_shard_cpu.py: the
header declares the three calls, the binding lists them and the library exports them; a host-only handle refuses them with
CTD_ENODEVICE before any other check; and the Python methods check lengths and refuse NumPy input.  The diagonals themselves are
checked on the GPU in tests/test_gpu_diag_shard.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ctdirect_jl_amd as ct

SHARD_SYMBOLS = {"ctd_hdiag_shard_dev_async": 5, "ctd_jsq_rows_shard_dev_async": 4, "ctd_jsq_cols_shard_dev_async": 4}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_shard_diag_symbols_declared_listed_exported():
    with open(HEADER) as f:
        text = f.read()
    declared = set(re.findall(r"\b(ctd_\w+)\s*\(", text))
    L = ct._lib.lib()
    for name, nargs in SHARD_SYMBOLS.items():
        assert name in declared, name
        decl = re.search(name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        res, args = ct._lib.SYMBOLS[name]
        assert res is C.c_int32 and len(args) == nargs, name
        assert hasattr(L, name), name
    # the diagonals' OUT OF SCOPE line no longer lists the shard form
    scope = re.search(r"OUT OF SCOPE: ([^\n]*row / column max-norms)", text)
    assert scope and "shard" not in scope.group(1), scope


@pytest.mark.parametrize("steps", [None, (3, 7)])
def test_host_only_handle_refuses_shard_diagonals_first(steps):
    """CTD_ENODEVICE with valid and with NULL pointers, on a whole-grid and on a shard handle, the message naming the function; only
    the NULL handle is checked before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1, steps=steps)
    L = ct._lib.lib()
    x, wx, ov = (np.zeros(d.dim_NLP_variables) for _ in range(3))
    y, oc = (np.zeros(d.dim_NLP_constraints) for _ in range(2))
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    valid = {
        "ctd_hdiag_shard_dev_async": (V(x), V(y), 1.0, V(ov)),
        "ctd_jsq_rows_shard_dev_async": (V(x), V(wx), V(oc)),
        "ctd_jsq_cols_shard_dev_async": (V(x), V(y), V(ov)),
    }
    for name, args in valid.items():
        fn = getattr(L, name)
        null = tuple(a if isinstance(a, float) else None for a in args)
        for a in (args, null):
            assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, (name, a)
            assert b"host-only" in L.ctd_last_error(d._h), name
            assert name.encode() in L.ctd_last_error(d._h), name
        assert fn(None, *args) == ct._lib.CTD_EINVAL, name
        assert fn(None, *null) == ct._lib.CTD_EINVAL, name


def test_shard_diagonals_check_lengths_and_refuse_numpy():
    d = ct.DOCP("goddard", 10, "midpoint", device=-1, steps=(3, 7))
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n: torch.zeros(n, dtype=torch.float64)          # noqa: E731
    # (method, name of the optional input, its length, the output's length)
    calls = ((lambda x, a, out: d.hdiag_shard(x, a, 0.7, out=out), "y", ncon, nvar),
             (lambda x, a, out: d.jsq_rows_shard(x, a, out=out), "wx", nvar, ncon),
             (lambda x, a, out: d.jsq_cols_shard(x, a, out=out), "wc", ncon, nvar))
    for fn, aname, na, nout in calls:
        with pytest.raises(ValueError, match=rf"x has {nvar + 1} entries, expected"):
            fn(t(nvar + 1), t(na), t(nout))
        with pytest.raises(ValueError, match=rf"{aname} has {na + 1} entries, expected {na}"):
            fn(t(nvar), t(na + 1), t(nout))
        with pytest.raises(ValueError, match=rf"out has {nout - 1} entries, expected {nout}"):
            fn(t(nvar), t(na), t(nout - 1))
        # NumPy input: there is no host path
        for args in ((np.zeros(nvar), t(na), t(nout)), (t(nvar), np.zeros(na), t(nout)), (t(nvar), t(na), np.zeros(nout))):
            with pytest.raises(TypeError, match="device tensor"):
                fn(*args)
        # vectors of the right lengths pass these checks: what stops them here is that they are not on a GPU
        for a in (t(na), None):
            with pytest.raises(ValueError, match="GPU"):
                fn(t(nvar), a, t(nout))
