"""The tile of the static-emit kernel reads its run-time inputs from TileArgs (csrc/ctd_layout.hpp): same bits as before (run with -m gpu).

`cons_jac_static_kernel` takes a packed block of the few values its tile workgroups read at run time as its first argument
(`make_tile_args`), reads the time grid from the device table only and selects a stage's row of K from registers.  None of that may
change a bit: c and the Jacobian values of a handle created normally are compared (`torch.equal`) with those of a handle created
with `CTD_STATIC_EMIT=0` (the lean kernel) and with `CTD_LEAN=0` (the general kernel), which read KParams as before.

Goddard on Gauss-Legendre 1, 2, 3, on the uniform grid and on a non-uniform user grid (a wrong index into the table shows there),
N in {2, 7, 22, 43, 100}: all-edge, one tile, one step more than a tile of 21, two tiles + 1, several tiles (CTD_TILE=21 pins the
tile of the benchmark's grid).  The double integrator with free t0 and tf (both times are optimisation variables) on
Gauss-Legendre 2, N in {7, 43}.  Per grid, the references are computed once; the default handle is then called with both outputs,
with c only, with the values only, with both outputs 8 bytes off their allocation (no 16-byte alignment), and into NaN-filled
buffers whose guard bands on both sides must come back untouched.
"""
import numpy as np
import pytest

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import _lib
from helpers import bench_inputs, describe

pytestmark = pytest.mark.gpu

KNOBS = ("CTD_STATIC_EMIT", "CTD_LEAN", "CTD_TILE")
GUARD = 96            # doubles on either side of a guarded payload
NAN_BITS = 0x7FF8_0000_0000_BEEF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def user_grid(N):
    tg = np.cumsum(np.r_[0.0, 1.0 + 0.5 * np.sin(np.arange(N))])
    return tg / tg[-1]


def handle(monkeypatch, prob, N, sch, knob, grid):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CTD_TILE", "21")
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    d = ct.DOCP(prob, N, sch, device=0, time_grid=user_grid(N) if grid == "user" else None)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return d


def nan_buffer(torch, n):
    return torch.full((n,), NAN_BITS, dtype=torch.int64, device="cuda").view(torch.float64)


def run_case(torch, monkeypatch, prob, N, sch, grid):
    what = (prob, sch, grid, N)
    refs, x = [], None
    for knob in ({"CTD_STATIC_EMIT": "0"}, {"CTD_LEAN": "0"}):
        d = handle(monkeypatch, prob, N, sch, knob, grid)
        if x is None:
            x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
        c, v = nan_buffer(torch, d.dim_NLP_constraints), nan_buffer(torch, d.nnzj)
        d.cons_jac(x, c, v)
        torch.cuda.synchronize()
        assert not torch.isnan(c).any() and not torch.isnan(v).any(), (what, knob, "the reference kernel left entries unwritten")
        refs.append((c, v))
        d.close()

    def same(c, v, variant):
        for (rc, rv), name in zip(refs, ("lean", "general")):
            if c is not None:
                assert torch.equal(c, rc), (what, variant, "c differs from the " + name + " kernel's")
            if v is not None:
                assert torch.equal(v, rv), (what, variant, "values differ from the " + name + " kernel's")

    d = handle(monkeypatch, prob, N, sch, {}, grid)
    nc, nv = d.dim_NLP_constraints, d.nnzj
    L = _lib.lib()
    # both outputs
    c, v = nan_buffer(torch, nc), nan_buffer(torch, nv)
    d.cons_jac(x, c, v)
    torch.cuda.synchronize()
    same(c, v, "both")
    # c only, values only: the other pointer is null, its buffer stays as it was
    c, v = nan_buffer(torch, nc), nan_buffer(torch, nv)
    d._ck(L.ctd_cons_jac_dev(d._h, d._dev_ptr(x, d.dim_NLP_variables, "x"), d._dev_ptr(c, nc, "c"), None))
    torch.cuda.synchronize()
    same(c, None, "c only")
    c = nan_buffer(torch, nc)
    d._ck(L.ctd_cons_jac_dev(d._h, d._dev_ptr(x, d.dim_NLP_variables, "x"), None, d._dev_ptr(v, nv, "vals")))
    torch.cuda.synchronize()
    same(None, v, "values only")
    assert (c.view(torch.int64) == NAN_BITS).all(), (what, "values only: c was written")
    # 8 bytes off the allocation: no 16-byte alignment
    cb, vb = nan_buffer(torch, nc + 2), nan_buffer(torch, nv + 2)
    c, v = cb[1:1 + nc], vb[1:1 + nv]
    assert c.data_ptr() % 16 == 8 and v.data_ptr() % 16 == 8
    d.cons_jac(x, c, v)
    torch.cuda.synchronize()
    same(c, v, "8 bytes off")
    for b, n in ((cb, nc), (vb, nv)):
        assert int(b.view(torch.int64)[0]) == NAN_BITS and int(b.view(torch.int64)[n + 1]) == NAN_BITS, (what, "8 bytes off: a neighbour was written")
    # NaN-filled outputs between guard bands
    cb, vb = nan_buffer(torch, nc + 2 * GUARD), nan_buffer(torch, nv + 2 * GUARD)
    c, v = cb[GUARD:GUARD + nc], vb[GUARD:GUARD + nv]
    d.cons_jac(x, c, v)
    torch.cuda.synchronize()
    same(c, v, "guarded")
    for b, n in ((cb, nc), (vb, nv)):
        bits = b.view(torch.int64)
        assert (bits[:GUARD] == NAN_BITS).all() and (bits[GUARD + n:] == NAN_BITS).all(), (what, "a guard band was written")
    d.close()


GODDARD = [(s, g) for s in ("gauss_legendre_1", "gauss_legendre_2", "gauss_legendre_3") for g in ("uniform", "user")]


@pytest.mark.parametrize("sch,grid", GODDARD, ids=[f"{s}-{g}" for s, g in GODDARD])
def test_goddard_bits_unchanged(torch_cuda, monkeypatch, sch, grid):
    for N in (2, 7, 22, 43, 100):
        run_case(torch_cuda, monkeypatch, "goddard", N, sch, grid)


@pytest.mark.parametrize("grid", ("uniform", "user"))
def test_free_t0_tf_bits_unchanged(torch_cuda, monkeypatch, grid):
    for N in (7, 43):
        run_case(torch_cuda, monkeypatch, "double_integrator_freet0tf", N, "gauss_legendre_2", grid)


def test_the_static_kernel_is_what_runs(torch_cuda, monkeypatch):
    """the geometry the cases above rely on: 21-step tiles, and a workgroup size the static form is built for"""
    d = handle(monkeypatch, "goddard", 100, "gauss_legendre_2", {}, "uniform")
    li = d.launch_info()
    d.close()
    assert li["steps_per_tile"] == 21 and li["block"] in (256, 320) and li["direct_tiles"] == 1, li
