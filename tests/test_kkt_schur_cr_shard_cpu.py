"""The shard form of the log-depth Schur preconditioner without a GPU: the layout query (ctd_kkt_schur_cr_shard_layout,
DOCP.kkt_schur_cr_shard_layout) on host-only shard handles against the handle's own pattern, the two macros of the header, the
symbols and the refusals, the cut of the plan (a stand-alone program built with -fsanitize=address,undefined: nothing is loaded into
Python under a sanitizer), and the iteration counts of scipy's MINRES with the dense cut matrix of tests/schur_shard_ref.py -- the
yardstick of the GPU solves of tests/test_gpu_kkt_schur_cr_shard.py.  No code under test enters those counts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.sparse.linalg import minres

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from ctdirect_jl_amd.dist import shard_steps
from schur_ref import SchurRef, small_sc_case
from schur_shard_ref import SchurCutRef, cross_rank_sum, cut_T, full_T, shard_cuts, solve_partial_sums
from test_gpu_kkt_minres import asm_precond, diag_op, minres_case
from test_kkt_schur_cpu import SCHEMES, csr, host_handle, last_error

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "ctdirect_hip.h")
N_LAYOUT = 7
FAMILY = ["ctd_kkt_schur_cr_shard_layout", "ctd_kkt_schur_cr_shard_factor_dev_async", "ctd_kkt_schur_cr_shard_solve_dev_async",
          "ctd_kkt_schur_cr_shard_info", "ctd_kkt_minres_schur_cr_shard_layout", "ctd_kkt_minres_schur_cr_shard_start_dev_async",
          "ctd_kkt_minres_schur_cr_shard_begin_dev_async", "ctd_kkt_minres_schur_cr_shard_alfa_dev_async",
          "ctd_kkt_minres_schur_cr_shard_lanczos_dev_async", "ctd_kkt_minres_schur_cr_shard_update_dev_async",
          "ctd_kkt_minres_schur_cr_shard_info"]
# iterations of scipy's MINRES (rtol 1e-10) with the dense cut M, cuts from shard_steps: G -> count; "diag": the diagonal pair
COUNTS = {("goddard", "trapeze", 20, False): {1: 29, 2: 29, 3: 32, 4: 29, 8: 29, "diag": 72},
          ("goddard", "trapeze", 300, True): {1: 36, 2: 50, 3: 62, 4: 70, 8: 135, "diag": 7151}}


def ceil_log2(N):
    return (N - 1).bit_length()


def shard_info(d):
    o = (C.c_int64 * 8)()
    assert _lib.lib().ctd_shard_info(d._h, o) == _lib.CTD_OK
    return list(o)


@pytest.mark.parametrize("prob", ct.PROBLEMS)
@pytest.mark.parametrize("sch", SCHEMES)
def test_layout(prob, sch):
    N = N_LAYOUT
    whole = host_handle(prob, sch, N)
    rowptr, colind = csr(whole)
    cr = whole.kkt_schur_cr_layout()
    m, v_off = cr.block_rows, whole.dim_NLP_variables - cr.tail_cols
    for G in (1, 2, 3):
        blocks = []
        for r in range(G):
            sb, se = shard_steps(N, G, r)
            d = whole if G == 1 else host_handle(prob, sch, N, steps=(sb, se))
            lay = d.kkt_schur_cr_shard_layout()
            assert (lay.N, lay.step_begin, lay.step_end, lay.n_blocks, lay.block_rows) == (N, sb, se, se - sb, m)
            assert (lay.first_row, lay.tail_rows, lay.first_tail_row, lay.tail_cols) == (sb * m, cr.tail_rows, cr.first_tail_row, cr.tail_cols)
            assert lay.n_levels == ceil_log2(se - sb)
            assert lay.factor_launches == 2 * lay.n_levels + 2 and lay.solve_launches == 2 * lay.n_levels + 1
            assert lay.workspace == _lib.kkt_schur_cr_workspace(se - sb, m)
            if G == 1:
                assert (lay.n_levels, lay.factor_launches, lay.solve_launches, lay.workspace) == \
                       (cr.n_levels, cr.factor_launches, cr.solve_launches, cr.workspace)
            # the read set of the factor: the CSR range of the rank's block rows, inside ctd_shard_info's range ...
            assert (lay.jvals_begin, lay.jvals_end) == (rowptr[sb * m], rowptr[se * m])
            info = shard_info(d)
            assert info[4] <= lay.jvals_begin <= lay.jvals_end <= info[5]
            if se == N and cr.tail_rows:
                assert lay.jvals_end < info[5], "the last rank's factor does not read the tail rows behind its blocks"
            # ... and the span of the non-tail columns of those rows
            cols = colind[rowptr[sb * m]:rowptr[se * m]]
            cols = cols[cols < v_off]
            assert (lay.px_begin, lay.px_end) == (int(cols.min()), int(cols.max()) + 1)
            blocks += list(range(sb, se))
        assert blocks == list(range(N)), "the ranks' blocks partition [0, N)"


def test_macros_of_the_header():
    """CTD_KKT_MINRES_SCHUR_SHARD_SLOT and CTD_KKT_MINRES_SCHUR_SHARD_WORKSPACE as the header spells them, against the layouts"""
    src = open(HEADER).read()
    slot_expr = re.search(r"#define CTD_KKT_MINRES_SCHUR_SHARD_SLOT (.*)\n", src).group(1)
    old_slot = int(re.search(r"#define CTD_KKT_MINRES_SHARD_SLOT (\d+)\n", src).group(1))
    slot = eval(slot_expr, {"CTD_KKT_MINRES_SHARD_SLOT": old_slot})
    assert slot == old_slot + 256 + 16 == _lib.KKT_MINRES_SCHUR_SHARD_SLOT
    ws_expr = re.search(r"#define CTD_KKT_MINRES_SCHUR_SHARD_WORKSPACE\(n, n_ranks\) \\\n(.*)\n", src).group(1).replace("(int64_t)", "")
    for prob, sch, N in (("goddard", "trapeze", 7), ("goddard", "gauss_legendre_2", 5), ("double_integrator_path", "midpoint", 20)):
        for G in (1, 2, 3):
            for r in range(G):
                d = host_handle(prob, sch, N, steps=shard_steps(N, G, r))
                lay, old = d.kkt_minres_schur_shard_layout(G), d.kkt_minres_shard_layout(G)
                assert lay.slot == slot and old.slot == old_slot
                assert lay.workspace == eval(ws_expr, {"n": lay.n, "n_ranks": G, "CTD_KKT_MINRES_SCHUR_SHARD_SLOT": slot})
                # the same ownership and geometry; the areas of the larger slots do not overlap and fit the workspace
                for f in ("n", "var_begin", "var_end", "tail_begin", "tail_end", "row_begin", "row_end", "n_own", "n_dot", "nwg", "chunk", "off_v", "off_kv"):
                    assert getattr(lay, f) == getattr(old, f), f
                areas = [(lay.off_send_a, slot), (lay.off_send_b, slot)] + ([(lay.off_gathered_a, G * slot), (lay.off_gathered_b, G * slot)] if G > 1 else [])
                areas.sort()
                assert areas[0][0] == 8 * lay.n and all(a + k <= b for (a, k), (b, _) in zip(areas, areas[1:]))
                assert areas[-1][0] + areas[-1][1] <= lay.off_state and lay.off_state + 16 <= lay.workspace
                if G == 1:
                    assert (lay.off_gathered_a, lay.off_gathered_b) == (lay.off_send_a, lay.off_send_b)


def test_symbols():
    L = _lib.lib()
    src = open(HEADER).read()
    for name in FAMILY:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert re.search(r"int32_t " + name + r"\(", src), name
    assert "SchurCrShardPrecond" in ct.__all__


def test_refusals():
    L = _lib.lib()
    E = _lib.CTD_EINVAL
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    fn = "ctd_kkt_schur_cr_shard_layout"
    csc = host_handle("goddard", "trapeze", 8, steps=(2, 5), value_order="csc")
    with pytest.raises(ct.CTDirectError) as e:
        csc.kkt_schur_cr_shard_layout()
    assert e.value.status == E and "CTD_ORDER_CSR" in last_error(csc) and last_error(csc).startswith(fn + ": ")
    lay = _lib.ctd_schur_cr_shard_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_shard_layout) - 8)
    assert L.ctd_kkt_schur_cr_shard_layout(d._h, C.byref(lay)) == E
    assert "struct_size" in last_error(d) and last_error(d).startswith(fn + ": ")
    assert L.ctd_kkt_schur_cr_shard_layout(d._h, None) == E
    lay = _lib.ctd_schur_cr_shard_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_shard_layout))
    assert L.ctd_kkt_schur_cr_shard_layout(None, C.byref(lay)) == E
    # the whole-grid entry points go on refusing the shard handle, and say where the shard form is
    with pytest.raises(ct.CTDirectError):
        d.kkt_schur_cr_layout()
    assert "no shard form" in last_error(d) and "ctd_kkt_schur_cr_shard_" in last_error(d)
    # the layout of the solve: n_ranks that do not fit the grid, the struct size, the CSR order
    mlay = _lib.ctd_minres_shard_layout(struct_size=C.sizeof(_lib.ctd_minres_shard_layout))
    fn = "ctd_kkt_minres_schur_cr_shard_layout"
    for G in (0, 9):
        assert L.ctd_kkt_minres_schur_cr_shard_layout(d._h, G, C.byref(mlay)) == E
        assert last_error(d).startswith(fn + ": ") and "n_ranks" in last_error(d)
    assert L.ctd_kkt_minres_schur_cr_shard_layout(csc._h, 3, C.byref(mlay)) == E and "CTD_ORDER_CSR" in last_error(csc)
    mlay.struct_size -= 8
    assert L.ctd_kkt_minres_schur_cr_shard_layout(d._h, 3, C.byref(mlay)) == E and "struct_size" in last_error(d)
    # the device entry points on a host-only handle: refused by name; NULL handle and struct sizes first
    info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
    sys = _lib.ctd_kkt_system(struct_size=C.sizeof(_lib.ctd_kkt_system), obj_weight=1.0)
    calls = {"ctd_kkt_schur_cr_shard_factor_dev_async": lambda h: L.ctd_kkt_schur_cr_shard_factor_dev_async(h, None, None, None, None),
             "ctd_kkt_schur_cr_shard_solve_dev_async": lambda h: L.ctd_kkt_schur_cr_shard_solve_dev_async(h, None, None, None),
             "ctd_kkt_schur_cr_shard_info": lambda h: L.ctd_kkt_schur_cr_shard_info(h, None, None),
             "ctd_kkt_minres_schur_cr_shard_start_dev_async":
                 lambda h: L.ctd_kkt_minres_schur_cr_shard_start_dev_async(h, C.byref(sys), None, None, None, None, 3, 1, 1e-10, 10),
             "ctd_kkt_minres_schur_cr_shard_begin_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_shard_begin_dev_async(h, None, 3, 1),
             "ctd_kkt_minres_schur_cr_shard_alfa_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_shard_alfa_dev_async(h, None, None, 3, 1),
             "ctd_kkt_minres_schur_cr_shard_lanczos_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_shard_lanczos_dev_async(h, None, None, None, 3, 1),
             "ctd_kkt_minres_schur_cr_shard_update_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_shard_update_dev_async(h, None, None, 3, 1),
             "ctd_kkt_minres_schur_cr_shard_info": lambda h: L.ctd_kkt_minres_schur_cr_shard_info(h, None, 3, C.byref(info))}
    for name, call in calls.items():
        assert call(d._h) == _lib.CTD_ENODEVICE, name
        assert last_error(d).startswith(name + ": "), (name, last_error(d))
        assert call(None) == E, name
    small = _lib.ctd_kkt_system(struct_size=8, obj_weight=1.0)
    assert L.ctd_kkt_minres_schur_cr_shard_start_dev_async(d._h, C.byref(small), None, None, None, None, 3, 1, 1e-10, 10) == E
    assert last_error(d).startswith("ctd_kkt_minres_schur_cr_shard_start_dev_async: ") and "struct_size" in last_error(d)


def wide_ocp():
    """a run-time OCP whose blocks have more than 64 rows (no registry problem has): 15 states and 5 path rows, which with
    Gauss-Legendre 3 gives block_rows = 4 * 15 + 5 = 65"""
    name = "wide_blocks_rt"
    if name not in ct.PROBLEMS:
        name = ct.register_ocp(name, dynamics=["x2 + u1"] + [f"-x{i}" for i in range(1, 15)], m=1, path=[f"x{i}" for i in range(1, 6)])
    return name, "gauss_legendre_3", 65


def test_wide_blocks_are_refused():
    """block_rows > 64 on a handle cut to a step range: CTD_EINVAL from both layout queries, by name"""
    L = _lib.lib()
    name, sch, m = wide_ocp()
    d = host_handle(name, sch, 6, steps=(2, 4))
    mlay = d.kkt_minres_shard_layout(3)
    assert mlay.row_end - mlay.row_begin == 2 * m, "two steps of 65 rows"
    with pytest.raises(ct.CTDirectError) as e:
        d.kkt_schur_cr_shard_layout()
    assert e.value.status == _lib.CTD_EINVAL
    assert last_error(d).startswith("ctd_kkt_schur_cr_shard_layout: ") and f"block_rows = {m} exceeds 64" in last_error(d)
    lay = _lib.ctd_schur_cr_shard_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_shard_layout))
    assert L.ctd_kkt_schur_cr_shard_layout(d._h, C.byref(lay)) == _lib.CTD_EINVAL
    mlay = _lib.ctd_minres_shard_layout(struct_size=C.sizeof(_lib.ctd_minres_shard_layout))
    assert L.ctd_kkt_minres_schur_cr_shard_layout(d._h, 3, C.byref(mlay)) == _lib.CTD_EINVAL
    assert last_error(d).startswith("ctd_kkt_minres_schur_cr_shard_layout: ") and f"block_rows = {m} exceeds 64" in last_error(d)
    with pytest.raises(ct.CTDirectError):
        d.kkt_minres_schur_shard_layout(3)
    # the whole grid of the same OCP as the single shard: refused alike; the diagonal form's layout is not
    whole = host_handle(name, sch, 6)
    with pytest.raises(ct.CTDirectError) as e:
        whole.kkt_schur_cr_shard_layout()
    assert e.value.status == _lib.CTD_EINVAL and "exceeds 64" in last_error(whole)
    assert L.ctd_kkt_minres_shard_layout(d._h, 3, C.byref(mlay)) == _lib.CTD_OK


def test_layout_is_the_callers_copy():
    """DOCP keeps the layout of a handle (the read set is a walk of its rows); every caller gets a struct of its own"""
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    a, b = d.kkt_schur_cr_shard_layout(), d.kkt_schur_cr_shard_layout()
    assert a is not b and bytes(a) == bytes(b)
    a.n_blocks = -1
    assert d.kkt_schur_cr_shard_layout().n_blocks == 3


def test_numpy_inputs_are_refused():
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    a = np.zeros(d.dim_NLP_variables)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_shard_factor(np.zeros(d.nnzj), a, np.zeros(d.dim_NLP_constraints), None, np.zeros(8))
    P = ct.SchurCrShardPrecond(a, np.zeros(d.dim_NLP_constraints), np.zeros(8), d.kkt_schur_cr_shard_layout())
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_shard_solve(P, np.zeros(d.dim_NLP_constraints))


def test_plan_cut(tmp_path):
    exe = str(tmp_path / "schur_cr_shard_plan_main")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-o", exe, os.path.join(HERE, "schur_cr_shard_plan_main.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTD_")}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().startswith("ok: 11 grids, "), r.stdout


def test_reference_matrix_and_sum_order():
    """the reference's own statements agree: one rank is the one-chunk matrix of tests/schur_ref.py; a cut drops exactly the
    coupling blocks across it; the order of the cross-rank sum with one rank is the whole-grid order (own terms, then the solve's)"""
    c = minres_case("goddard", "trapeze", 7)
    lay = host_handle("goddard", "trapeze", 7).kkt_schur_cr_layout()
    px, pc = asm_precond(c)
    m, N, nv = lay.block_rows, lay.N, lay.tail_cols
    assert np.array_equal(cut_T(c, px, m, N, nv, [0, N]), SchurRef(c, px, pc, m, N, nv, N).T)
    S, T = full_T(c, px, m, N, nv), cut_T(c, px, m, N, nv, [0, 3, 5, 7])
    blocks = np.arange(N * m) // m
    rank = np.searchsorted([3, 5], blocks, side="right")
    same = rank[:, None] == rank[None, :]
    assert np.array_equal(T[same], S[same]) and not T[~same].any()
    dropped = {(int(a), int(b)) for a, b in zip(*np.nonzero(S * ~same)) for a, b in [(blocks[a], blocks[b])]}
    assert dropped == {(3, 2), (2, 3), (5, 4), (4, 5)}, dropped
    R = SchurCutRef(c, px, pc, m, N, nv, [0, 3, 5, 7])
    v = np.random.default_rng(3).uniform(-1.0, 1.0, c["nvar"] + c["ncon"])
    Minv = np.zeros((len(v), len(v)))
    nvar, nb = c["nvar"], N * m
    Minv[:nvar, :nvar] = np.diag(px)
    Minv[nvar:nvar + nb, nvar:nvar + nb] = T
    Minv[nvar + nb:, nvar + nb:] = np.diag(pc[nb:])
    assert np.allclose(Minv @ R.apply(v), v, rtol=1e-9, atol=1e-12)
    g = np.random.default_rng(4)
    own, solve = [list(g.uniform(0, 1, 3))], [list(g.uniform(0, 1, 5))]
    s = 0.0
    for t in own[0] + solve[0]:
        s += t
    assert cross_rank_sum(own, solve) == s
    own2, solve2 = [[1e16, 1.0], [1.0]], [[-1e16], [1.0]]
    assert cross_rank_sum(own2, solve2) == ((((0.0 + 1e16) + 1.0) + 1.0) + -1e16) + 1.0
    r, y = g.uniform(-1, 1, 5 * m), g.uniform(-1, 1, 5 * m)
    part = solve_partial_sums(r, y, m, 5)
    assert len(part) == 5 and np.isclose(sum(part), r @ y, rtol=1e-12)
    assert len(solve_partial_sums(np.ones(300 * 2), np.ones(300 * 2), 2, 300)) == 256


def count_iterations(c, M, cap):
    it = [0]
    _, info = minres(c["K_asm"], c["rhs"], M=M, rtol=1e-10, maxiter=cap, callback=lambda zk: it.__setitem__(0, it[0] + 1))
    assert info == 0
    return it[0]


@pytest.mark.parametrize("case", list(COUNTS), ids=lambda c: f"{c[0]}-{c[1]}-N{c[2]}" + ("-small_sc" if c[3] else ""))
def test_reference_counts(case):
    prob, sch, N, small = case
    c = minres_case(prob, sch, N)
    if small:
        c = small_sc_case(c)
    lay = host_handle(prob, sch, N).kkt_schur_cr_layout()
    px, pc = asm_precond(c)
    n = c["nvar"] + c["ncon"]
    got = {G: count_iterations(c, SchurCutRef(c, px, pc, lay.block_rows, N, lay.tail_cols, shard_cuts(N, G)).operator(), 10 * n)
           for G in (1, 2, 3, 4, 8)}
    got["diag"] = count_iterations(c, diag_op(px, pc), 20 * n)
    print(case, got)
    assert [shard_cuts(N, G)[r:r + 2] for G in (1, 2, 3, 4, 8) for r in range(G)] == \
           [list(shard_steps(N, G, r)) for G in (1, 2, 3, 4, 8) for r in range(G)]
    assert got == COUNTS[case], (got, COUNTS[case])
