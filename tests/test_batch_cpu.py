"""CPU tests of the batched callbacks (ctd_*_batch_dev_async, DOCP.*_batch): the library exports them, a host-only handle refuses
them with CTD_ENODEVICE before any other check, and the Python methods refuse host arrays before calling into the library.
The results themselves (bit-identical to single calls) are checked on the GPU in tests/test_gpu_batch.py."""
import ctypes as C

import numpy as np
import pytest

import ctdirect_jl_amd as ct

BATCH_SYMBOLS = ("ctd_cons_jac_batch_dev_async", "ctd_obj_batch_dev_async", "ctd_grad_batch_dev_async",
                 "ctd_hess_coord_batch_dev_async")


def test_batch_symbols_exported():
    L = ct._lib.lib()
    for name in BATCH_SYMBOLS:
        assert name in ct._lib.SYMBOLS
        assert hasattr(L, name), name


def _calls(L, h, batch, p, n):
    """every batched entry point on handle h with `batch` members; p: a non-null dummy pointer (never dereferenced: the handle
    has no device), leading dimensions exactly the vector lengths"""
    nvar, ncon, nnzj, nnzh = n
    return {
        "cons_jac": lambda: L.ctd_cons_jac_batch_dev_async(h, batch, p, nvar, p, ncon, p, nnzj),
        "obj": lambda: L.ctd_obj_batch_dev_async(h, batch, p, nvar, p),
        "grad": lambda: L.ctd_grad_batch_dev_async(h, batch, p, nvar, p, nvar),
        "hess": lambda: L.ctd_hess_coord_batch_dev_async(h, batch, p, nvar, p, ncon, 0.5, p, nnzh),
    }


@pytest.mark.parametrize("batch", [3, 0, 70000])
def test_host_only_handle_refuses_batched_calls_first(batch):
    """CTD_ENODEVICE comes before the batch-size, pointer and leading-dimension checks (as in ctd_hess_coord_dev_async): also
    with batch = 0, batch > 65535 and null pointers"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    L = ct._lib.lib()
    buf = np.zeros(8)
    sizes = (d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzj, d.nnzh)
    for p in (C.c_void_p(buf.ctypes.data), None):
        for name, call in _calls(L, d._h, batch, p, sizes).items():
            assert call() == ct._lib.CTD_ENODEVICE, (name, batch, p)
            assert b"host-only" in L.ctd_last_error(d._h), name
    # the null handle is the only thing checked before the device
    assert L.ctd_obj_batch_dev_async(None, 1, None, 0, None) == ct._lib.CTD_EINVAL


def test_docp_batch_methods_refuse_numpy():
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1)
    X = np.zeros((2, d.dim_NLP_variables))
    Y = np.zeros((2, d.dim_NLP_constraints))
    for call in (lambda: d.cons_jac_batch(X), lambda: d.obj_batch(X), lambda: d.grad_batch(X),
                 lambda: d.hess_coord_batch(X, Y, 0.5)):
        with pytest.raises(TypeError, match="no host batch path"):
            call()
