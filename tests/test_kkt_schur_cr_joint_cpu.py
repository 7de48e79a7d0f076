"""The joined form of the log-depth Schur preconditioner without a GPU: the dense reference of tests/schur_joint_ref.py against the
dense T itself, against the cut reference with one rank, and its identity for r' T^-1 r; the iteration counts of scipy's MINRES with
that reference as M -- no code under test enters them --; the layout query (ctd_kkt_schur_cr_joint_layout) on host-only shard
handles against the handle's own pattern; the macros of the header, the symbols, the refusals; and the plan over every admissible
cut of small grids (a stand-alone program built with -fsanitize=address,undefined: nothing is loaded into Python under a
sanitizer)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla
from scipy.sparse.linalg import minres

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from ctdirect_jl_amd.dist import shard_steps
from schur_joint_ref import SchurJointRef, backward_error, joint_sum
from schur_ref import small_sc_case
from schur_shard_ref import SchurCutRef, cross_rank_sum, full_T, shard_cuts
from test_gpu_kkt_minres import asm_precond, minres_case
from test_kkt_schur_cpu import csr, host_handle, last_error
from test_kkt_schur_cr_shard_cpu import COUNTS as CUT_COUNTS, wide_ocp

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "ctdirect_hip.h")
EPS = float(np.finfo(np.float64).eps)
FAMILY = ["ctd_kkt_schur_cr_joint_layout", "ctd_kkt_schur_cr_joint_factor_local_dev_async", "ctd_kkt_schur_cr_joint_factor_join_dev_async",
          "ctd_kkt_schur_cr_joint_solve_local_dev_async", "ctd_kkt_schur_cr_joint_solve_join_dev_async", "ctd_kkt_schur_cr_joint_info",
          "ctd_kkt_minres_schur_cr_joint_layout", "ctd_kkt_minres_schur_cr_joint_start_dev_async", "ctd_kkt_minres_schur_cr_joint_begin_dev_async",
          "ctd_kkt_minres_schur_cr_joint_alfa_dev_async", "ctd_kkt_minres_schur_cr_joint_lanczos_dev_async",
          "ctd_kkt_minres_schur_cr_joint_update_dev_async", "ctd_kkt_minres_schur_cr_joint_info"]
GS = (1, 2, 3, 4, 8)
# (problem, scheme, N, sc = 1e-8 U(1, 2)) -> iterations of scipy's MINRES (rtol 1e-10) with the reference as M, cuts from shard_cuts
COUNTS = {("goddard", "trapeze", 20, False): {1: 29, 2: 29, 3: 29, 4: 29, 8: 29},
          ("goddard", "trapeze", 300, True): {1: 36, 2: 38, 3: 38, 4: 38, 8: 38},
          ("goddard", "gauss_legendre_2", 20, True): {1: 50, 2: 50, 3: 50, 4: 50, 8: 50}}
case_name = lambda c: f"{c[0]}-{c[1]}-N{c[2]}" + ("-small_sc" if c[3] else "")      # noqa: E731


def system(case):
    prob, sch, N, small = case
    c = minres_case(prob, sch, N)
    if small:
        c = small_sc_case(c)
    lay = host_handle(prob, sch, N).kkt_schur_cr_layout()
    px, pc = asm_precond(c)
    return c, px, pc, lay.block_rows, N, lay.tail_cols


@pytest.fixture(scope="module")
def systems():
    made = {}

    def get(case):
        if case not in made:
            made[case] = system(case)
        return made[case]

    return get


@pytest.mark.parametrize("case", list(COUNTS), ids=case_name)
def test_reference_against_the_dense_matrix(systems, case):
    """the application: backward error against the dense T at the level of cho_solve on the whole T; the identity r . y = sum_r
    r_I . g_r + sigma: both sides are r' T^-1 r formed through backward-stable solves, so they differ by at most c eps |T| |y|^2 (the
    quadratic form of two perturbations of T of relative size eps); c = 64 covers the m-term sums"""
    c, px, pc, m, N, nv = systems(case)
    T = full_T(c, px, m, N, nv)
    fac = sla.cho_factor(T, lower=True)
    r = np.random.default_rng(5).uniform(-1.0, 1.0, N * m)
    y_chol = sla.cho_solve(fac, r)
    eta_chol = backward_error(T, y_chol, r)
    norm_T = np.abs(T).sum(axis=1).max()
    for G in GS:
        R = SchurJointRef(c, px, pc, m, N, nv, shard_cuts(N, G))
        y, inner, sigma, rs, xs = R.solve_parts(r)
        eta = backward_error(T, y, r)
        lhs, rhs = float(r @ y), sum(inner) + sigma
        print(case_name(case), "G", G, "eta", eta, "eta(cho_solve)", eta_chol, "identity, relative", abs(lhs - rhs) / abs(lhs))
        assert eta <= max(10.0 * eta_chol, 64.0 * EPS), (case, G, eta, eta_chol)
        assert all(t >= 0.0 for t in inner) and sigma >= 0.0, "both terms of the identity are non-negative"
        assert abs(lhs - rhs) <= 64.0 * EPS * norm_T * float(y @ y), (case, G, lhs, rhs)
        if G > 1:
            assert np.linalg.eigvalsh(R.S)[0] > 0.0, "the reduced matrix is positive definite"
            assert len(rs) == len(xs) == (G - 1) * m


def test_one_rank_is_the_cut_reference(systems):
    """no separator: the operator of SchurCutRef with one rank, bit for bit (the same Cholesky factor of the same matrix)"""
    for case in list(COUNTS)[:1] + [("goddard", "trapeze", 7, False)]:
        c, px, pc, m, N, nv = systems(case)
        J, Cut = SchurJointRef(c, px, pc, m, N, nv, [0, N]), SchurCutRef(c, px, pc, m, N, nv, [0, N])
        v = np.random.default_rng(3).uniform(-1.0, 1.0, c["nvar"] + c["ncon"])
        assert np.array_equal(J.apply(v), Cut.apply(v))
        y, inner, sigma, rs, xs = J.solve_parts(v[c["nvar"]:c["nvar"] + N * m])
        assert sigma == 0.0 and len(inner) == 1 and len(rs) == 0


def test_uneven_cuts_and_refused_cuts(systems):
    c, px, pc, m, N, nv = systems(("goddard", "trapeze", 7, False))
    T = full_T(c, px, m, N, nv)
    r = np.random.default_rng(6).uniform(-1.0, 1.0, N * m)
    eta_chol = backward_error(T, sla.cho_solve(sla.cho_factor(T, lower=True), r), r)
    for cuts in ([0, 1, 3, 5, 7], [0, 2, 5, 7], [0, 3, 5, 7], [0, 5, 7], [0, 1, 7]):
        y = SchurJointRef(c, px, pc, m, N, nv, cuts).solve_rows(r)
        assert backward_error(T, y, r) <= max(10.0 * eta_chol, 64.0 * EPS), cuts
    with pytest.raises(AssertionError):
        SchurJointRef(c, px, pc, m, N, nv, [0, 3, 4, 7])        # rank 1 is its separator alone


@pytest.mark.parametrize("case", list(COUNTS), ids=case_name)
def test_reference_counts(systems, case):
    """the joined M gives the one-rank count at every split, up to the wobble of its own row; the cut form's counts grow with G"""
    c, px, pc, m, N, nv = systems(case)
    n = c["nvar"] + c["ncon"]
    got = {}
    for G in GS:
        it = [0]
        _, info = minres(c["K_asm"], c["rhs"], M=SchurJointRef(c, px, pc, m, N, nv, shard_cuts(N, G)).operator(), rtol=1e-10, maxiter=10 * n,
                         callback=lambda zk: it.__setitem__(0, it[0] + 1))
        assert info == 0
        got[G] = it[0]
    print(case_name(case), got)
    assert [shard_cuts(N, G)[r:r + 2] for G in GS for r in range(G)] == [list(shard_steps(N, G, r)) for G in GS for r in range(G)]
    assert got == COUNTS[case], (got, COUNTS[case])
    assert max(got.values()) - min(got.values()) <= 2, "the joined M gives the one-rank count at every split, up to a wobble of 2"
    cut = CUT_COUNTS.get(case)
    if cut:
        assert cut[1] == got[1] and all(got[G] <= cut[G] for G in GS)
        assert all(got[G] < cut[G] for G in GS if cut[G] > cut[1] + 3), "where the cuts cost iterations, the joined form wins them back"


def test_sum_order():
    """the cross-rank sum of beta^2 with sigma appended after the slots' partial sums: one rank gives the order of the shard form;
    a changed convention (sigma first, or added per rank) is seen"""
    g = np.random.default_rng(4)
    own, solve = [list(g.uniform(0, 1, 3))], [list(g.uniform(0, 1, 5))]
    assert joint_sum(own, solve, 123.0) == cross_rank_sum(own, solve), "one rank: no separator, sigma is not added"
    own2, solve2 = [[1e16, 1.0], [1.0]], [[-1e16], [1.0]]
    base = ((((0.0 + 1e16) + 1.0) + 1.0) + -1e16) + 1.0
    assert joint_sum(own2, solve2, 3.0) == base + 3.0
    assert joint_sum(own2, solve2, 3.0) != (((((0.0 + 3.0) + 1e16) + 1.0) + 1.0) + -1e16) + 1.0, "sigma first would be another sum"
    assert joint_sum([[1.0], [1e16]], [[-1e16], [0.0]], 1.0) == 1.0
    assert ((((0.0 + 1.0) + 1.0) + 1e16) + -1e16) + 0.0 != 1.0, "sigma behind the first rank's own terms would be another sum"


# ---- the layout on host-only handles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,sch", [("goddard", "trapeze"), ("goddard", "gauss_legendre_2"), ("double_integrator_path", "midpoint"),
                                      ("quadrotor", "gauss_legendre_2")])
def test_layout(prob, sch):
    N = 9
    whole = host_handle(prob, sch, N)
    rowptr, colind = csr(whole)
    cr = whole.kkt_schur_cr_layout()
    m, mm, v_off = cr.block_rows, cr.block_rows ** 2, whole.dim_NLP_variables - cr.tail_cols
    for cuts in ([0, N], [0, 4, N], [0, 1, 3, N], [0, 2, 4, 6, N]):
        G = len(cuts) - 1
        blocks = []
        for r in range(G):
            sb, se = cuts[r], cuts[r + 1]
            d = whole if G == 1 else host_handle(prob, sch, N, steps=(sb, se))
            lay, sh = d.kkt_schur_cr_joint_layout(G, r), d.kkt_schur_cr_shard_layout()
            a = sb + (1 if r else 0)
            assert (lay.N, lay.n_ranks, lay.rank, lay.step_begin, lay.step_end, lay.block_rows) == (N, G, r, sb, se, m)
            assert (lay.separator, lay.int_begin, lay.n_int, lay.n_sep) == (sb if r else -1, a, se - a, max(G - 1, 1))
            assert (lay.first_row, lay.tail_rows, lay.first_tail_row, lay.tail_cols) == (sb * m, cr.tail_rows, cr.first_tail_row, cr.tail_cols)
            L = (se - a - 1).bit_length()
            assert lay.n_levels == L
            assert (lay.factor_local_launches, lay.factor_join_launches, lay.solve_local_launches, lay.solve_join_launches) == \
                   ((2 * L + 2, 0, 2 * L + 1, 0) if G == 1 else (4 * L + 5, 1, 2 * L + 2, 2))
            assert lay.factor_slot == _lib.kkt_schur_cr_joint_factor_slot(m) and lay.solve_slot == _lib.KKT_SCHUR_CR_JOINT_SOLVE_SLOT
            n_int, n_sep = lay.n_int, lay.n_sep
            offs = [0, lay.off_es, lay.off_eb, lay.off_ds, lay.off_wl, lay.off_wr, lay.off_scratch, lay.off_reduced, lay.off_rs, lay.off_xs,
                    lay.off_sigma, lay.workspace]
            lens = [_lib.kkt_schur_cr_workspace(n_int, m), mm, mm, mm, n_int * mm, n_int * mm, 4 * n_int * mm, n_sep + 2 * n_sep * mm, n_sep * m,
                    n_sep * m, 16]
            assert [b - a_ for a_, b in zip(offs, offs[1:])] == lens
            # the read set: the shard form's, and the halo of jvals right behind it -- the rows of block se
            assert (lay.jvals_begin, lay.jvals_end, lay.px_begin, lay.px_end) == (sh.jvals_begin, sh.jvals_end, sh.px_begin, sh.px_end)
            assert lay.jvals_halo_begin == lay.jvals_end == rowptr[se * m]
            assert lay.jvals_halo_end == (rowptr[(se + 1) * m] if se < N else lay.jvals_halo_begin)
            if se < N:
                # px needs nothing more: the non-tail columns that block se shares with block se - 1 lie inside the span
                nxt = colind[rowptr[se * m]:rowptr[(se + 1) * m]]
                own = colind[rowptr[(se - 1) * m]:rowptr[se * m]]
                shared = np.intersect1d(nxt[nxt < v_off], own[own < v_off])
                assert shared.size and lay.px_begin <= shared.min() and shared.max() < lay.px_end
            blocks += ([sb] if r else []) + list(range(a, se))
        assert blocks == list(range(N)), "separators and interiors partition [0, N)"


def test_macros_and_symbols():
    L = _lib.lib()
    src = open(HEADER).read()
    for name in FAMILY:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert re.search(r"int32_t " + name + r"\(", src), name
    assert "SchurCrJointPrecond" in ct.__all__
    assert int(re.search(r"#define CTD_KKT_SCHUR_CR_JOINT_MAX_RANKS (\d+)\n", src).group(1)) == _lib.KKT_SCHUR_CR_JOINT_MAX_RANKS
    slot = re.search(r"#define CTD_KKT_SCHUR_CR_JOINT_FACTOR_SLOT\(m\) (.*)\n", src).group(1).replace("(int64_t)", "")
    assert all(eval(slot, {"m": m}) == _lib.kkt_schur_cr_joint_factor_slot(m) == 16 + 4 * m * m for m in (1, 3, 9, 64))
    assert eval(re.search(r"#define CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT (.*)\n", src).group(1)) == _lib.KKT_SCHUR_CR_JOINT_SOLVE_SLOT == 208


def test_minres_layout_and_macros():
    """CTD_KKT_MINRES_SCHUR_JOINT_SLOT and _WORKSPACE as the header spells them, against the layouts: the ownership and geometry of
    the shard form, areas of the larger slots that do not overlap and fit the workspace"""
    src = open(HEADER).read()
    shard_slot = _lib.KKT_MINRES_SCHUR_SHARD_SLOT
    slot = eval(re.search(r"#define CTD_KKT_MINRES_SCHUR_JOINT_SLOT (.*)\n", src).group(1), {"CTD_KKT_MINRES_SCHUR_SHARD_SLOT": shard_slot})
    assert slot == shard_slot + 3 * 64 + 16 == _lib.KKT_MINRES_SCHUR_JOINT_SLOT == shard_slot + _lib.KKT_SCHUR_CR_JOINT_SOLVE_SLOT
    ws_expr = re.search(r"#define CTD_KKT_MINRES_SCHUR_JOINT_WORKSPACE\(n, n_ranks\) \\\n(.*)\n", src).group(1).replace("(int64_t)", "")
    N = 9
    for cuts in ([0, N], [0, 4, N], [0, 1, 3, N]):
        G = len(cuts) - 1
        for r in range(G):
            d = host_handle("goddard", "gauss_legendre_2", N, steps=(cuts[r], cuts[r + 1]))
            lay, old = d.kkt_minres_schur_joint_layout(G, r), d.kkt_minres_schur_shard_layout(G)
            assert lay.slot == slot and lay.workspace == eval(ws_expr, {"n": lay.n, "n_ranks": G, "CTD_KKT_MINRES_SCHUR_JOINT_SLOT": slot})
            for f in ("n", "var_begin", "var_end", "tail_begin", "tail_end", "row_begin", "row_end", "n_own", "n_dot", "nwg", "chunk", "off_v", "off_kv"):
                assert getattr(lay, f) == getattr(old, f), f
            areas = [(lay.off_send_a, slot), (lay.off_send_b, slot)] + ([(lay.off_gathered_a, G * slot), (lay.off_gathered_b, G * slot)] if G > 1 else [])
            areas.sort()
            assert areas[0][0] == 8 * lay.n and all(a + k <= b for (a, k), (b, _) in zip(areas, areas[1:]))
            assert areas[-1][0] + areas[-1][1] <= lay.off_state and lay.off_state + 16 <= lay.workspace
    # refusals of the layout, by name
    L, E = _lib.lib(), _lib.CTD_EINVAL
    fn = "ctd_kkt_minres_schur_cr_joint_layout"
    d = host_handle("goddard", "trapeze", 8, steps=(2, 3))
    mlay = _lib.ctd_minres_shard_layout(struct_size=C.sizeof(_lib.ctd_minres_shard_layout))
    assert L.ctd_kkt_minres_schur_cr_joint_layout(d._h, 3, 1, C.byref(mlay)) == E
    assert last_error(d).startswith(fn + ": ") and "at least 2 steps" in last_error(d)
    assert L.ctd_kkt_minres_schur_cr_joint_layout(d._h, 0, 0, C.byref(mlay)) == E and "n_ranks" in last_error(d)
    mlay.struct_size -= 8
    assert L.ctd_kkt_minres_schur_cr_joint_layout(d._h, 3, 1, C.byref(mlay)) == E and "struct_size" in last_error(d)
    # the device entry points on a host-only handle: refused by name; NULL handle first
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
    sys = _lib.ctd_kkt_system(struct_size=C.sizeof(_lib.ctd_kkt_system), obj_weight=1.0)
    pre = "ctd_kkt_minres_schur_cr_joint_"
    calls = {pre + "start_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_joint_start_dev_async(h, C.byref(sys), None, None, None, None, 3, 1, 1e-10, 10),
             pre + "begin_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_joint_begin_dev_async(h, None, None, 3, 1),
             pre + "alfa_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_joint_alfa_dev_async(h, None, None, 3, 1),
             pre + "lanczos_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_joint_lanczos_dev_async(h, None, None, None, 3, 1),
             pre + "update_dev_async": lambda h: L.ctd_kkt_minres_schur_cr_joint_update_dev_async(h, None, None, None, 3, 1),
             pre + "info": lambda h: L.ctd_kkt_minres_schur_cr_joint_info(h, None, 3, C.byref(info))}
    for name, call in calls.items():
        assert call(d._h) == _lib.CTD_ENODEVICE, name
        assert last_error(d).startswith(name + ": "), (name, last_error(d))
        assert call(None) == E, name


def test_refusals():
    L = _lib.lib()
    E = _lib.CTD_EINVAL
    fn = "ctd_kkt_schur_cr_joint_layout"
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    lay = _lib.ctd_schur_cr_joint_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_joint_layout))

    def refused(h, G, r, *words):
        assert L.ctd_kkt_schur_cr_joint_layout(h._h, G, r, C.byref(lay)) == E, (G, r)
        assert last_error(h).startswith(fn + ": ") and all(w in last_error(h) for w in words), (G, r, last_error(h))

    assert L.ctd_kkt_schur_cr_joint_layout(d._h, 3, 1, C.byref(lay)) == _lib.CTD_OK
    refused(d, 0, 0, "n_ranks = 0")
    refused(d, 257, 1, "n_ranks = 257")
    refused(d, 3, 3, "rank = 3", "[0, n_ranks = 3)")
    refused(d, 3, -1, "rank = -1")
    refused(d, 3, 0, "cannot be block rank = 0 of n_ranks = 3")          # rank 0 starts at step 0
    refused(d, 3, 2, "cannot be block rank = 2 of n_ranks = 3")          # the last rank ends at N
    refused(d, 1, 0, "cannot be block rank = 0 of n_ranks = 1")
    one = host_handle("goddard", "trapeze", 8, steps=(2, 3))
    refused(one, 3, 1, "[2, 3)", "no interior block", "at least 2 steps")
    first = host_handle("goddard", "trapeze", 8, steps=(0, 1))
    assert L.ctd_kkt_schur_cr_joint_layout(first._h, 3, 0, C.byref(lay)) == _lib.CTD_OK and lay.n_int == 1      # rank 0 may hold one step
    csc = host_handle("goddard", "trapeze", 8, steps=(2, 5), value_order="csc")
    refused(csc, 3, 1, "CTD_ORDER_CSR")
    with pytest.raises(ct.CTDirectError) as e:
        csc.kkt_schur_cr_joint_layout(3, 1)
    assert e.value.status == E
    small = _lib.ctd_schur_cr_joint_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_joint_layout) - 8)
    assert L.ctd_kkt_schur_cr_joint_layout(d._h, 3, 1, C.byref(small)) == E and "struct_size" in last_error(d)
    assert L.ctd_kkt_schur_cr_joint_layout(d._h, 3, 1, None) == E
    assert L.ctd_kkt_schur_cr_joint_layout(None, 3, 1, C.byref(lay)) == E
    # block_rows > 64
    name, sch, m = wide_ocp()
    wide = host_handle(name, sch, 6, steps=(2, 4))
    assert L.ctd_kkt_schur_cr_joint_layout(wide._h, 3, 1, C.byref(lay)) == E
    assert last_error(wide).startswith(fn + ": ") and f"block_rows = {m} exceeds 64" in last_error(wide)
    # the device entry points on a host-only handle: refused by name; NULL handle first
    bad = C.c_int64(0)
    calls = {"ctd_kkt_schur_cr_joint_factor_local_dev_async": lambda h: L.ctd_kkt_schur_cr_joint_factor_local_dev_async(h, None, None, None, None, None, 3, 1),
             "ctd_kkt_schur_cr_joint_factor_join_dev_async": lambda h: L.ctd_kkt_schur_cr_joint_factor_join_dev_async(h, None, None, 3, 1),
             "ctd_kkt_schur_cr_joint_solve_local_dev_async": lambda h: L.ctd_kkt_schur_cr_joint_solve_local_dev_async(h, None, None, None, None, 3, 1),
             "ctd_kkt_schur_cr_joint_solve_join_dev_async": lambda h: L.ctd_kkt_schur_cr_joint_solve_join_dev_async(h, None, None, None, 3, 1),
             "ctd_kkt_schur_cr_joint_info": lambda h: L.ctd_kkt_schur_cr_joint_info(h, None, 3, 1, C.byref(bad))}
    for name, call in calls.items():
        assert call(d._h) == _lib.CTD_ENODEVICE, name
        assert last_error(d).startswith(name + ": "), (name, last_error(d))
        assert call(None) == E, name


def test_numpy_inputs_are_refused():
    d = host_handle("goddard", "trapeze", 8, steps=(2, 5))
    a, z = np.zeros(d.dim_NLP_variables), np.zeros(d.dim_NLP_constraints)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_joint_factor_local(np.zeros(d.nnzj), a, z, None, 3, 1)
    P = ct.SchurCrJointPrecond(a, z, np.zeros(8), d.kkt_schur_cr_joint_layout(3, 1), np.zeros(8), np.zeros(8))
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_joint_solve_local(P, z, z)
    with pytest.raises(ValueError, match="device tensor"):
        d.kkt_schur_cr_joint_solve_join(P, z, z)


def test_plan(tmp_path):
    exe = str(tmp_path / "schur_cr_joint_plan_main")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-o", exe, os.path.join(HERE, "schur_cr_joint_plan_main.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTD_")}
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().startswith("ok: 11 grids, "), r.stdout
