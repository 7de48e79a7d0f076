"""CPU tests of the STATIC emit phase (csrc/ctd_emit_static.hpp) against the generic one, without a GPU.

tests/static_emit_emu.cpp (test infrastructure only, compiled with g++ like tests/emu/) evaluates every workgroup's records once
and streams them out twice: phase_emit into (c, vals), phase_emit_static into (c2, vals2).  Both pairs start NaN-filled and must
come out equal at EVERY position, bit for bit -- for every registry problem x scheme whose tiles have a static emit, both workgroup
sizes the static variant is built for, uniform and non-uniform grids, and the grid sizes where the peeled passes can go wrong
(with T = steps per tile and par = lanes / CSC period: 1, 2, par - 1, par, par + 1, T - 1, T, T + 1, 2 T + 1 regular steps in a
tile and every residue of the step count modulo par).

Also here: the periods StaticEmit states are the model builder's for every registry problem x scheme x control_steps (what
ctd_create checks on every manual / CSC handle), and the check refuses periods that differ.
"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import ctdirect_jl_amd as ct
from helpers import bench_inputs, describe

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "static_emit_emu.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "ctdirect.jl_amd", "csrc")
LIB = os.path.join(HERE, "emu", "libctd_static_emit_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        with open(os.path.join(HERE, "emu", ".build.lock"), "w") as lock:          # (one builder at a time, as tests/emu/emu.py)
            fcntl.flock(lock, fcntl.LOCK_EX)
            deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".cpp"))]
            if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in deps):
                subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w", "-shared",
                                       "-o", LIB + ".tmp", SRC])
                os.replace(LIB + ".tmp", LIB)
        L = C.CDLL(LIB)
        L.se_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def both(prob, sch, N, nthr, tile=0, tg=None, cs=1, evaluate=True):
    """(info, c, vals, c2, vals2); info = dict(ran, Lseg, vr, sLseg, svr, T, nnzj, ncon)"""
    L = lib()
    tga = None if tg is None else np.ascontiguousarray(tg, dtype=np.float64)
    info = np.zeros(8, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
    args = lambda x, o: (ct.PROBLEMS[prob], ct.SCHEMES[sch], C.c_int64(N), p(tga), C.c_int64(0 if tga is None else len(tga)), cs, tile, nthr,      # noqa: E731
                         p(x), *[p(a) for a in o], p(info))
    st = L.se_cons_jac(*args(None, [None] * 4))          # sizes and periods
    assert st == 0, L.se_last_error().decode()
    keys = ("ran", "Lseg", "vr", "sLseg", "svr", "T", "nnzj", "ncon")
    if not evaluate:
        return dict(zip(keys, map(int, info))), None, None, None, None
    d = ct.DOCP(prob, N, sch, device=-1, time_grid=tg, control_steps=cs)
    x = np.ascontiguousarray(bench_inputs(describe(d, prob, sch), perturb=1e-3))
    d.close()
    out = [np.full(int(info[7]), np.nan), np.full(int(info[6]), np.nan), np.full(int(info[7]), np.nan), np.full(int(info[6]), np.nan)]
    st = L.se_cons_jac(*args(x, out))
    assert st == 0, L.se_last_error().decode()
    return (dict(zip(keys, map(int, info))), *out)


def grid_sizes(T, par):
    """N whose tiles hold the interesting counts of regular steps: the first tile loses step 0 to the edge block, so a grid of
    r + 1 steps has one tile of r regular steps (r < T); longer grids add full tiles and a short last one"""
    rs = {1, 2, par - 1, par, par + 1, T - 1, T, T + 1, 2 * T + 1} | {T + 1 + q for q in range(par)}
    return sorted({max(5, r + 1) for r in rs if r >= 1})


PAIRS = [(p, s) for p in ct.PROBLEMS for s in ct.SCHEMES if s.startswith("gauss_legendre")]


@pytest.mark.parametrize("prob,sch", PAIRS, ids=[f"{p}-{s}" for p, s in PAIRS])
def test_static_emit_equals_generic_emit(prob, sch):
    rng = np.random.default_rng(11)
    ran = 0
    for cs in (1,):
        for nthr in (256, 320):
            info, *_ = both(prob, sch, 7, nthr, cs=cs, evaluate=False)
            if info["Lseg"] != info["sLseg"] or info["Lseg"] > nthr:
                continue
            par = nthr // info["Lseg"]
            for tile in (4, 9):          # (9: more passes than one chunk holds for the short periods' small par; 4: several tiles)
                for N in grid_sizes(tile, par):
                    for tg in (None, np.cumsum(rng.uniform(0.5, 1.5, N + 1))) if N in (tile + 2, 2 * tile + 2) else (None,):
                        info, c, v, c2, v2 = both(prob, sch, N, nthr, tile=tile, tg=tg, cs=cs)
                        if not info["ran"]:
                            continue
                        ran += 1
                        assert not np.isnan(c).any() and not np.isnan(v).any()          # every output written ...
                        assert np.array_equal(c, c2) and np.array_equal(v, v2), (prob, sch, cs, nthr, tile, N)      # ... at the same place, the same bits
    # (ran == 0: no static emit for the tiles of this problem and scheme -- staged driver, constant control, or a period longer
    # than the workgroup; test_static_emit_is_offered_where_expected pins down that the flagship cases do run)


def test_static_emit_is_offered_where_expected():
    for prob, sch, nthr in (("goddard", "gauss_legendre_2", 320), ("goddard", "gauss_legendre_3", 256), ("goddard", "gauss_legendre_1", 320),
                            ("double_integrator_path", "gauss_legendre_2", 256)):
        info, *_ = both(prob, sch, 23, nthr, tile=4)
        assert info["ran"] == 1, (prob, sch, nthr, info)
    for prob, sch in (("quadrotor12", "gauss_legendre_3"), ("quadrotor", "gauss_legendre_2"), ("double_integrator_path", "midpoint"), ("goddard", "gauss_legendre_2_constant_control"), ("goddard", "trapeze")):
        info, *_ = both(prob, sch, 23, 256, tile=4)
        assert info["ran"] == 0, (prob, sch, info)


def test_static_emit_long_tiles():
    """tiles of many passes (the chunk loops behind the first chunk): the 40- and 48-step tiles of the long grids"""
    for prob, sch, tile in (("double_integrator_path", "gauss_legendre_2", 48), ("goddard", "gauss_legendre_2", 40), ("goddard", "gauss_legendre_3", 48)):
        for nthr in (256, 320):
            for N in (tile + 1, 2 * tile + 3, 3 * tile - 1):
                info, c, v, c2, v2 = both(prob, sch, N, nthr, tile=tile)
                assert info["ran"] == 1
                assert not np.isnan(c).any() and not np.isnan(v).any()
                assert np.array_equal(c, c2) and np.array_equal(v, v2), (prob, sch, nthr, N)


ALL = [(p, s) for p in ct.PROBLEMS for s in ct.SCHEMES]


@pytest.mark.parametrize("prob,sch", ALL, ids=[f"{p}-{s}" for p, s in ALL])
def test_static_periods_are_the_models(prob, sch):
    """every manual / CSC handle of the registry is accepted by ctd_create's period check, and where StaticEmit describes the
    scheme its periods are the built ones"""
    for cs in ((1, 2, 3) if sch == "midpoint" else (1,)):
        for N in (1, 4, 5, 7, 40):
            d = ct.DOCP(prob, N, sch, device=-1, control_steps=cs)          # (a refusal raises)
            period = d.launch_info()["csc_period"]
            d.close()
            info, *_ = both(prob, sch, N, 256, cs=cs, evaluate=False)
            assert info["Lseg"] == period
            stagewise = sch in ("gauss_legendre_2", "gauss_legendre_3")
            described = sch == "gauss_legendre_1" or stagewise
            if described and N >= 5:
                assert (info["sLseg"], info["svr"]) == (info["Lseg"], info["vr"]), (prob, sch, cs, N, info)


def test_period_check_refuses_other_periods():
    L = lib()
    for prob, sch in (("goddard", "gauss_legendre_2"), ("double_integrator_path", "gauss_legendre_1"), ("quadrotor", "gauss_legendre_3")):
        pid, sid = ct.PROBLEMS[prob], ct.SCHEMES[sch]
        assert L.se_mismatch(pid, sid, C.c_int64(9), 0, 0) == 0
        assert L.se_mismatch(pid, sid, C.c_int64(9), 1, 0) == 1 and L.se_last_error() == b"Lseg"
        assert L.se_mismatch(pid, sid, C.c_int64(9), -1, 0) == 1 and L.se_last_error() == b"Lseg"
        assert L.se_mismatch(pid, sid, C.c_int64(9), 0, 1) == 1 and L.se_last_error() == b"vr"
