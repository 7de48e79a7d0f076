"""The chunked block-tridiagonal Schur preconditioner without a GPU: the layout query (ctd_kkt_schur_layout, DOCP.kkt_schur_layout)
on host-only handles, its refusals, and the iteration counts of the dense reference (tests/schur_ref.py) that the GPU test
leans on."""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse.linalg import minres

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from schur_ref import SchurRef, chunks
from test_gpu_kkt_minres import asm_precond, diag_op, minres_case

SCHEMES = ("trapeze", "midpoint", "gauss_legendre_1", "gauss_legendre_2_constant_control", "gauss_legendre_3_constant_control",
           "gauss_legendre_2", "gauss_legendre_3", "euler", "euler_implicit")
CASES = [(prob, sch, 3) for prob in ct.PROBLEMS for sch in SCHEMES] + [("goddard", "trapeze", 1)]


def host_handle(prob, sch, N, **kw):
    return ct.DOCP(prob, N, sch, device=-1, **{"pattern": "structural", "value_order": "csr", **kw})


def csr(d):
    rowptr = np.empty(d.dim_NLP_constraints + 1, dtype=np.int64)
    colind = np.empty(d.nnzj, dtype=np.int64)
    st = _lib.lib().ctd_jac_csr(d._h, rowptr.ctypes.data_as(C.POINTER(C.c_int64)), colind.ctypes.data_as(C.POINTER(C.c_int64)))
    assert st == _lib.CTD_OK
    return rowptr, colind


@pytest.mark.parametrize("prob,sch,N", CASES, ids=lambda v: str(v))
def test_layout(prob, sch, N):
    d = host_handle(prob, sch, N)
    lay = d.kkt_schur_layout()
    m, nv = lay.block_rows, d.dims.NLP_v
    assert lay.N == N and m >= 1
    assert m * N + lay.tail_rows == d.dim_NLP_constraints
    assert lay.first_tail_row == m * N and lay.tail_cols == nv
    assert (lay.n_chunks, lay.chunk_steps) == (1, N)
    # rows that share a non-tail column are at most one block apart, recomputed from ctd_jac_csr
    rowptr, colind = csr(d)
    rows = np.repeat(np.arange(d.dim_NLP_constraints), np.diff(rowptr))
    keep = (rows < lay.first_tail_row) & (colind < d.dim_NLP_variables - nv)
    blk = rows[keep] // m
    lo = np.full(d.dim_NLP_variables, N, dtype=np.int64)
    hi = np.full(d.dim_NLP_variables, -1, dtype=np.int64)
    np.minimum.at(lo, colind[keep], blk)
    np.maximum.at(hi, colind[keep], blk)
    used = hi >= 0
    assert (hi[used] - lo[used] <= 1).all()
    for L in (1, 2, N, N + 5):
        l = d.kkt_schur_layout(L)
        assert l.n_chunks == -(-N // min(L, N)) == len(chunks(N, L)) and l.chunk_steps == min(L, N), (L, l.n_chunks, l.chunk_steps)
        assert l.workspace == lay.workspace
    # the workspace as documented: CTD_KKT_SCHUR_FIXED + N + 2 N m^2
    assert lay.workspace == _lib.KKT_SCHUR_FIXED + N + 2 * N * m * m
    assert host_handle(prob, sch, 2 * N).kkt_schur_layout().workspace == _lib.KKT_SCHUR_FIXED + 2 * N + 4 * N * m * m


def test_layout_blocks_of_the_issue():
    for prob, sch, m, tail in (("goddard", "trapeze", 3, 4), ("goddard", "gauss_legendre_2", 9, 4), ("double_integrator_path", "midpoint", 3, 5)):
        lay = host_handle(prob, sch, 7).kkt_schur_layout()
        assert (lay.block_rows, lay.tail_rows) == (m, tail), (prob, sch)


def last_error(d):
    return _lib.lib().ctd_last_error(d._h).decode()


def test_refusals():
    d = host_handle("goddard", "trapeze", 3)
    for L in (0, -3):
        with pytest.raises(ct.CTDirectError) as e:
            d.kkt_schur_layout(L)
        assert e.value.status == _lib.CTD_EINVAL and last_error(d).startswith("ctd_kkt_schur_layout: chunk_steps")
    csc = host_handle("goddard", "trapeze", 3, value_order="csc")
    with pytest.raises(ct.CTDirectError) as e:
        csc.kkt_schur_layout()
    assert e.value.status == _lib.CTD_EINVAL and "CTD_ORDER_CSR" in last_error(csc) and last_error(csc).startswith("ctd_kkt_schur_layout")
    lay = _lib.ctd_schur_layout(struct_size=C.sizeof(_lib.ctd_schur_layout) - 8)
    assert _lib.lib().ctd_kkt_schur_layout(d._h, 1, C.byref(lay)) == _lib.CTD_EINVAL
    assert "struct_size" in last_error(d)
    assert _lib.lib().ctd_kkt_schur_layout(d._h, 1, None) == _lib.CTD_EINVAL
    assert _lib.lib().ctd_kkt_schur_layout(None, 1, C.byref(lay)) == _lib.CTD_EINVAL
    shard = host_handle("goddard", "trapeze", 8, steps=(0, 4))
    with pytest.raises(ct.CTDirectError) as e:
        shard.kkt_schur_layout()
    assert e.value.status == _lib.CTD_EINVAL and "no shard form" in last_error(shard)
    # the device entry points on a host-only handle: refused before anything else, by name
    assert _lib.lib().ctd_kkt_schur_factor_dev_async(d._h, None, None, None, 1, None) == _lib.CTD_ENODEVICE
    assert last_error(d).startswith("ctd_kkt_schur_factor_dev_async")
    assert _lib.lib().ctd_kkt_schur_solve_dev_async(d._h, None, None, None) == _lib.CTD_ENODEVICE
    assert _lib.lib().ctd_kkt_schur_info(d._h, None, None) == _lib.CTD_ENODEVICE


def test_numpy_inputs_are_refused():
    d = host_handle("goddard", "trapeze", 3)
    x = np.zeros(d.dim_NLP_variables)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_precond(x, None)
    P = ct.SchurPrecond(x, np.zeros(d.dim_NLP_constraints), np.zeros(8), d.kkt_schur_layout())
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_minres(x, None, np.zeros(d.dim_NLP_variables + d.dim_NLP_constraints), precond=P)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_solve(P, np.zeros(d.dim_NLP_constraints))


def iterations(c, M):
    it = [0]
    _, info = minres(c["K_asm"], c["rhs"], M=M, rtol=1e-10, maxiter=10 * len(c["rhs"]), callback=lambda z: it.__setitem__(0, it[0] + 1))
    assert info == 0
    return it[0]


def test_reference_counts():
    """scipy's MINRES on K_asm of minres_case("goddard", "trapeze", 20) with the dense statement of M: 29 iterations for chunk
    lengths 20, 8 and 3, 48 for 1; 72 with the diagonal M"""
    c = minres_case("goddard", "trapeze", 20)
    lay = host_handle("goddard", "trapeze", 20).kkt_schur_layout()
    px, pc = asm_precond(c)
    got = {L: iterations(c, SchurRef(c, px, pc, lay.block_rows, lay.N, lay.tail_cols, L).operator()) for L in (20, 8, 3, 1)}
    diag = iterations(c, diag_op(px, pc))
    print("reference counts", got, "diagonal", diag)
    assert got == {20: 29, 8: 29, 3: 29, 1: 48} and diag == 72
