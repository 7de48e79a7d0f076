"""The log-depth exact block-tridiagonal Schur preconditioner without a GPU: the layout query (ctd_kkt_schur_cr_layout,
DOCP.kkt_schur_cr_layout) on host-only handles, the level helper of the plan (a stand-alone program built with
-fsanitize=address,undefined: nothing is loaded into Python under a sanitizer), the refusals, and the NumPy statement of the
elimination (tests/schur_cr_ref.py) against scipy.linalg.cho_solve on the dense one-chunk T of tests/schur_ref.py -- which pins the
specification itself.

BAR of the reference against dense: backward error eta = |T y - r|_inf / (|T|_inf |y|_inf + |r|_inf) at most max(10 eta_ref, 64 eps),
eta_ref that of cho_solve on the same T and r: the bar of the GPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from schur_cr_ref import SchurCrRef, eliminated, levels
from schur_ref import SchurRef, schur_T, small_sc_case
from test_gpu_kkt_minres import asm_precond, minres_case
from test_kkt_schur_cpu import SCHEMES, host_handle, last_error

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float64).eps)
GRIDS = (1, 2, 3, 5, 8, 9)
# the cases of tests/test_gpu_kkt_schur_cr.py (the run-time twin shares its transcription with the registry problem)
DENSE = [("goddard", "trapeze", N) for N in (1, 2, 3, 4, 5, 7, 8, 9, 20, 33, 300)] + \
        [("goddard", "gauss_legendre_2", 7), ("double_integrator_path", "midpoint", 7), ("goddard", "midpoint", 7)] + \
        [(p, s, N) for p, s in (("quadrotor", "gauss_legendre_2"), ("quadrotor12", "gauss_legendre_3")) for N in (3, 5)]


def ceil_log2(N):
    l = 0
    while (1 << l) < N:
        l += 1
    return l


@pytest.mark.parametrize("prob", ct.PROBLEMS)
@pytest.mark.parametrize("sch", SCHEMES)
def test_layout(prob, sch):
    for N in GRIDS:
        d = host_handle(prob, sch, N)
        lay, old = d.kkt_schur_cr_layout(), d.kkt_schur_layout()
        m = lay.block_rows
        assert (lay.N, m, lay.tail_rows, lay.first_tail_row, lay.tail_cols) == \
               (old.N, old.block_rows, old.tail_rows, old.first_tail_row, old.tail_cols) and lay.N == N
        assert lay.n_levels == ceil_log2(N) == levels(N)
        # the launch counts: functions of N alone
        assert lay.factor_launches == 2 * lay.n_levels + 2 and lay.solve_launches == 2 * lay.n_levels + 1
        # the workspace: the macro of the header
        assert lay.workspace == _lib.kkt_schur_cr_workspace(N, m) == _lib.KKT_SCHUR_FIXED + N + 3 * N * m * m + 2 * N * m


def test_workspace_macro_of_the_header():
    """CTD_KKT_SCHUR_CR_WORKSPACE as include/ctdirect_hip.h spells it, evaluated by the C preprocessor's own arithmetic rules"""
    src = open(os.path.join(HERE, "..", "include", "ctdirect_hip.h")).read()
    at = src.index("#define CTD_KKT_SCHUR_CR_WORKSPACE(N, m)")
    body = src[at:src.index("\n/*", at)].split("\\\n", 1)[1]
    expr = body.replace("(int64_t)", "").replace("CTD_KKT_SCHUR_FIXED", str(_lib.KKT_SCHUR_FIXED))
    for N, m in ((1, 3), (9, 9), (1000, 49)):
        assert eval(expr, {"N": N, "m": m}) == _lib.kkt_schur_cr_workspace(N, m)


def test_level_helper(tmp_path):
    exe = str(tmp_path / "schur_cr_plan_main")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-o", exe, os.path.join(HERE, "schur_cr_plan_main.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTD_")}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == "ok: 10 grids", r.stdout


def test_index_sets_of_the_reference():
    """the reference's own index sets: the same properties, so that the two statements of the levels agree"""
    for N in (1, 2, 3, 4, 5, 7, 8, 9, 33, 1000):
        seen = np.zeros(N, dtype=int)
        for l in range(levels(N)):
            for i in eliminated(N, l):
                assert i % (1 << l) == 0 and (i >> l) & 1 and not seen[i - (1 << l)] and (i + (1 << l) >= N or not seen[i + (1 << l)])
                seen[i] += 1
        assert seen[0] == 0 and (seen[1:] == 1).all()


def test_refusals():
    L = _lib.lib()
    d = host_handle("goddard", "trapeze", 3)
    csc = host_handle("goddard", "trapeze", 3, value_order="csc")
    with pytest.raises(ct.CTDirectError) as e:
        csc.kkt_schur_cr_layout()
    assert e.value.status == _lib.CTD_EINVAL and "CTD_ORDER_CSR" in last_error(csc) and last_error(csc).startswith("ctd_kkt_schur_cr_layout: ")
    shard = host_handle("goddard", "trapeze", 8, steps=(0, 4))
    with pytest.raises(ct.CTDirectError) as e:
        shard.kkt_schur_cr_layout()
    assert e.value.status == _lib.CTD_EINVAL and "no shard form" in last_error(shard) and last_error(shard).startswith("ctd_kkt_schur_cr_layout: ")
    lay = _lib.ctd_schur_cr_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_layout) - 8)
    assert L.ctd_kkt_schur_cr_layout(d._h, C.byref(lay)) == _lib.CTD_EINVAL
    assert "struct_size" in last_error(d) and last_error(d).startswith("ctd_kkt_schur_cr_layout: ")
    assert L.ctd_kkt_schur_cr_layout(d._h, None) == _lib.CTD_EINVAL
    lay = _lib.ctd_schur_cr_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_layout))
    assert L.ctd_kkt_schur_cr_layout(None, C.byref(lay)) == _lib.CTD_EINVAL
    # the device entry points on a host-only handle: refused before anything else, by name
    info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
    sys = _lib.ctd_kkt_system(struct_size=C.sizeof(_lib.ctd_kkt_system), obj_weight=1.0)
    calls = {"ctd_kkt_schur_cr_factor_dev_async": lambda: L.ctd_kkt_schur_cr_factor_dev_async(d._h, None, None, None, None),
             "ctd_kkt_schur_cr_solve_dev_async": lambda: L.ctd_kkt_schur_cr_solve_dev_async(d._h, None, None, None),
             "ctd_kkt_schur_cr_info": lambda: L.ctd_kkt_schur_cr_info(d._h, None, None),
             "ctd_kkt_minres_schur_cr_start_dev_async": lambda: L.ctd_kkt_minres_schur_cr_start_dev_async(d._h, C.byref(sys), None, None, None, 1e-10),
             "ctd_kkt_minres_schur_cr_dev": lambda: L.ctd_kkt_minres_schur_cr_dev(d._h, C.byref(sys), None, None, None, 1e-10, 10, 2, C.byref(info))}
    for name, call in calls.items():
        assert call() == _lib.CTD_ENODEVICE, name
        assert last_error(d).startswith(name + ": "), (name, last_error(d))
    # struct sizes and the NULL handle come first
    small = _lib.ctd_kkt_system(struct_size=8, obj_weight=1.0)
    assert L.ctd_kkt_minres_schur_cr_start_dev_async(d._h, C.byref(small), None, None, None, 1e-10) == _lib.CTD_EINVAL
    assert last_error(d).startswith("ctd_kkt_minres_schur_cr_start_dev_async: ") and "struct_size" in last_error(d)
    assert L.ctd_kkt_minres_schur_cr_dev(None, C.byref(sys), None, None, None, 1e-10, 10, 2, C.byref(info)) == _lib.CTD_EINVAL


def test_numpy_inputs_are_refused():
    d = host_handle("goddard", "trapeze", 3)
    x = np.zeros(d.dim_NLP_variables)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_precond(x, None)
    P = ct.SchurCrPrecond(x, np.zeros(d.dim_NLP_constraints), np.zeros(8), d.kkt_schur_cr_layout())
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_minres(x, None, np.zeros(d.dim_NLP_variables + d.dim_NLP_constraints), precond=P)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_solve(P, np.zeros(d.dim_NLP_constraints))
    with pytest.raises(ValueError, match="schur_cr"):
        d.kkt_minres(x, None, np.zeros(d.dim_NLP_variables + d.dim_NLP_constraints), precond="cyclic")


def backward_error(T, y, r):
    return float(np.abs(T @ y - r).max() / (np.abs(T).sum(axis=1).max() * np.abs(y).max() + np.abs(r).max()))


def dense_T(c, prob, sch, N):
    lay = host_handle(prob, sch, N).kkt_schur_cr_layout()
    px, pc = asm_precond(c)
    R = SchurRef(c, px, pc, lay.block_rows, lay.N, lay.tail_cols, lay.N)
    return R, lay


@pytest.mark.parametrize("prob,sch,N", DENSE, ids=lambda v: str(v))
def test_reference_against_dense(prob, sch, N):
    cases = [minres_case(prob, sch, N)]
    if (prob, sch, N) == ("goddard", "trapeze", 300):
        cases.append(small_sc_case(cases[0]))          # the ill-conditioned T of the GPU test's "point"
    for c in cases:
        R, lay = dense_T(c, prob, sch, N)
        m, nb = lay.block_rows, lay.first_tail_row
        # T is block tridiagonal: the elimination sees all of it
        blocks = np.arange(nb) // m
        assert not R.T[np.abs(blocks[:, None] - blocks[None, :]) > 1].any()
        F = SchurCrRef(R.T, N, m)
        assert F.info() == -1 and F.n_levels == lay.n_levels
        r = np.random.default_rng(5).uniform(-1.0, 1.0, nb)
        y, y_ref = F.solve(r), sla.cho_solve(sla.cho_factor(R.T, lower=True), r)
        eta, eta_ref = backward_error(R.T, y, r), backward_error(R.T, y_ref, r)
        print(prob, sch, N, "m", m, "cond", np.linalg.cond(R.T), "eta", eta, "eta_ref (cho_solve)", eta_ref)
        assert eta <= max(10.0 * eta_ref, 64.0 * EPS), (eta, eta_ref)


def test_reference_records_a_failed_pivot():
    """a negative weight on the column of a state of step 2, which the rows of the blocks 1 and 2 hold: block 1 fails at level 0 on
    its own data; the NaN of its factors reaches block 2 and, as it reaches every later level, the root: the smallest block with a
    recorded pivot is 0 whenever any pivot fails, and the status words tell where it began"""
    c = minres_case("goddard", "trapeze", 7)
    d = host_handle("goddard", "trapeze", 7)
    lay = d.kkt_schur_cr_layout()
    px, pc = asm_precond(c)
    px = px.copy()
    px[2 * d.discretization._step_variables_block] = -1e-9
    T = schur_T(c, px, lay.block_rows, lay.N, lay.tail_cols, lay.N)
    F = SchurCrRef(T, lay.N, lay.block_rows)
    assert F.status[1] >= 0 and F.status[2] >= 0 and F.status[3] == F.status[5] == -1, F.status
    assert F.info() == 0
    assert np.isnan(F.solve(np.ones(lay.first_tail_row))).all()
