"""CPU tests of the shard form of the device-resident MINRES solve (ctd_kkt_minres_shard_*; DOCP.kkt_minres_shard_*,
dist.kkt_minres_shards, ShardedDOCP.kkt_minres), without a GPU: the ownership planner (plan_krylov_shard of csrc/ctd_host.cpp through
ctd_kkt_minres_shard_layout, which needs no device), the workspace layout, the exported symbols and the refusals that come before
the device is looked at.  The values are checked on the GPU in tests/test_gpu_kkt_minres_shard.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ctdirect_jl_amd as ct
from test_gpu_kkt_minres import CAPPED, CAPPED_N, krylov_constants, krylov_geom

TRANSCRIPTIONS = [("goddard", "trapeze"), ("double_integrator_path", "midpoint"), ("goddard", "gauss_legendre_2")]
SLOT = 2080


def splits(N, G):
    """every split of N steps into G non-empty ascending blocks, as cut lists (0, .., N)"""
    return [(0,) + c + (N,) for c in itertools.combinations(range(1, N), G - 1)]


def layout(prob, sch, N, steps, G):
    d = ct.DOCP(prob, N, sch, device=-1, pattern="structural", steps=steps)
    lay = d.kkt_minres_shard_layout(G)
    dims = (d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v)
    d.close()
    return lay, dims


def owned(lay):
    return np.r_[np.arange(lay.var_begin, lay.var_end), np.arange(lay.tail_begin, lay.tail_end), np.arange(lay.row_begin, lay.row_end)]


@pytest.mark.parametrize("prob,sch", TRANSCRIPTIONS)
@pytest.mark.parametrize("N", [1, 3, 20])
def test_ownership_partitions_the_vector(prob, sch, N):
    for G in (1, 2, 3):
        if G > N:
            continue
        for cuts in splits(N, G):
            lays = [layout(prob, sch, N, (cuts[k], cuts[k + 1]), G) for k in range(G)]
            nvar, ncon, nv = lays[0][1]
            n = nvar + ncon
            tail = np.arange(nvar - nv, nvar)
            own_count, dot_count = np.zeros(n, dtype=int), np.zeros(n, dtype=int)
            for k, (lay, _) in enumerate(lays):
                idx = owned(lay)
                assert lay.n == n and lay.n_ranks == G and lay.slot == SLOT
                assert (np.diff(idx) > 0).all() and len(idx) == lay.n_own, (cuts, k)        # ascending global index, no repeats
                assert (lay.tail_begin, lay.tail_end) == (nvar - nv, nvar)
                assert (lay.nwg, lay.chunk) == krylov_geom(lay.n_own), (cuts, k)             # the geometry of the compacted list
                own_count[idx] += 1
                last = k == G - 1
                dot = idx if last else idx[~np.isin(idx, tail)]
                assert len(dot) == lay.n_dot, (cuts, k)
                dot_count[dot] += 1
            # the owned lists partition 0 .. n - 1 apart from the tail, which every rank holds; the summed ones partition it exactly
            body = np.ones(n, dtype=bool)
            body[tail] = False
            assert (own_count[body] == 1).all() and (own_count[tail] == G).all(), cuts
            assert (dot_count == 1).all(), cuts
            if G == 1:
                lay = lays[0][0]
                assert np.array_equal(owned(lay), np.arange(n))
                assert (lay.nwg, lay.chunk) == krylov_geom(n) and lay.n_own == lay.n_dot == n


def test_capped_size_three_ranks():
    """Goddard trapeze N = 75 000 (n = 525 009 = 7 N + 9: 4 N + 5 variables of which one is v, 3 N + 4 rows), ranks of 25 000 steps.
    By hand: ranks 0 and 1 own 4 * 25 000 variables + the tail entry + 3 * 25 000 rows = 175 001 entries and sum 175 000; the last
    rank owns 100 004 variables below v_off + 1 + 75 004 rows = 175 009 and sums them all.  ceil(175 001 / 1024) = 171 workgroups,
    chunk = ceil(175 001 / 171) = 1024 -> 1024; the last rank: ceil(175 009 / 1024) = 171, chunk 1024.  One rank of the whole grid:
    the capped geometry of tests/test_kkt_minres_cpu.py, (512, 1280)."""
    prob, sch, N, _ = CAPPED
    block, span, max_wg = krylov_constants()
    assert (block, span, max_wg) == (256, 1024, 512)
    want = [(175001, 175000, 171, 1024), (175001, 175000, 171, 1024), (175009, 175009, 171, 1024)]
    for k in range(3):
        lay, (nvar, ncon, nv) = layout(prob, sch, N, (25000 * k, 25000 * (k + 1)), 3)
        assert (nvar, ncon, nv) == (4 * N + 5, 3 * N + 4, 1) and lay.n == CAPPED_N
        assert (lay.n_own, lay.n_dot, lay.nwg, lay.chunk) == want[k], k
        assert lay.var_begin == 100000 * k and lay.row_begin == nvar + 75000 * k
        assert lay.var_end == (nvar - 1 if k == 2 else 100000 * (k + 1)) and lay.row_end == (nvar + ncon if k == 2 else nvar + 75000 * (k + 1))
    lay, _ = layout(prob, sch, N, None, 1)
    assert (lay.n_own, lay.nwg, lay.chunk) == (CAPPED_N, 512, 1280)


def test_workspace_layout():
    """the offsets the header states: v and kv are the fourth and fifth of eight n-vectors, the slots follow; with one rank the
    gathered areas are the send slots; the regions do not overlap and fit CTD_KKT_MINRES_SHARD_WORKSPACE"""
    for G, steps in ((1, None), (3, (2, 5))):
        lay, (nvar, ncon, _) = layout("goddard", "trapeze", 7, steps, G)
        n = nvar + ncon
        assert lay.workspace == 8 * n + (2 + 2 * G) * SLOT + 96
        assert (lay.off_v, lay.off_kv, lay.off_send_a, lay.off_send_b) == (3 * n, 4 * n, 8 * n, 8 * n + SLOT)
        if G == 1:
            assert (lay.off_gathered_a, lay.off_gathered_b) == (lay.off_send_a, lay.off_send_b)
        else:
            assert lay.off_gathered_a == lay.off_send_b + SLOT and lay.off_gathered_b == lay.off_gathered_a + G * SLOT
        assert max(lay.off_gathered_b + G * SLOT, lay.off_send_b + SLOT) <= lay.off_state and lay.off_state + 16 <= lay.workspace


def test_symbols_and_refusals_without_a_device():
    L, lib = ct._lib.lib(), ct._lib
    names = ["ctd_kkt_minres_shard_layout", "ctd_kkt_minres_shard_info"] + \
            [f"ctd_kkt_minres_shard_{p}_dev_async" for p in ("start", "begin", "alfa", "lanczos", "update")]
    for name in names:
        assert hasattr(L, name), name
    assert C.sizeof(lib.ctd_minres_shard_layout) == 8 + 21 * 8
    d = ct.DOCP("goddard", 10, "midpoint", device=-1, steps=(3, 7))
    n = d.dim_NLP_variables + d.dim_NLP_constraints
    err = lambda: L.ctd_last_error(d._h)        # noqa: E731
    # the layout query: NULL, struct_size, n_ranks -- and no device is needed for the answer
    lay = lib.ctd_minres_shard_layout(struct_size=C.sizeof(lib.ctd_minres_shard_layout))
    assert L.ctd_kkt_minres_shard_layout(None, 3, C.byref(lay)) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_shard_layout(d._h, 3, None) == lib.CTD_EINVAL
    for wrong in (0, C.sizeof(lay) - 8, C.sizeof(lay) + 8):
        bad = lib.ctd_minres_shard_layout(struct_size=wrong)
        assert L.ctd_kkt_minres_shard_layout(d._h, 3, C.byref(bad)) == lib.CTD_EINVAL
        assert err().startswith(b"ctd_kkt_minres_shard_layout: ") and b"struct_size" in err()
    for G in (0, -1, 11):
        assert L.ctd_kkt_minres_shard_layout(d._h, G, C.byref(lay)) == lib.CTD_EINVAL
        assert b"n_ranks" in err()
    assert L.ctd_kkt_minres_shard_layout(d._h, 3, C.byref(lay)) == 0 and lay.n == n
    # start: sys NULL or of another size is CTD_EINVAL before the device; the right size reaches CTD_ENODEVICE
    rhs, z, ws = np.ones(n), np.full(n, 7.0), np.zeros(lay.workspace)
    vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    ks = lib.ctd_kkt_system(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0)
    start = lambda h, s: L.ctd_kkt_minres_shard_start_dev_async(h, s, vp(rhs), vp(z), vp(ws), 3, 1, 1e-10, 10)        # noqa: E731
    assert start(None, C.byref(ks)) == lib.CTD_EINVAL
    assert start(d._h, None) == lib.CTD_EINVAL and err().startswith(b"ctd_kkt_minres_shard_start_dev_async: sys is null")
    for wrong in (0, C.sizeof(ks) - 8, C.sizeof(ks) + 8):
        bad = lib.ctd_kkt_system(struct_size=wrong, obj_weight=1.0)
        assert start(d._h, C.byref(bad)) == lib.CTD_EINVAL and b"struct_size" in err()
    assert start(d._h, C.byref(ks)) == lib.CTD_ENODEVICE and err().startswith(b"ctd_kkt_minres_shard_start_dev_async: ")
    # the phases and the info: NULL handle, then the device
    for p in ("alfa", "lanczos", "update"):
        fn = getattr(L, f"ctd_kkt_minres_shard_{p}_dev_async")
        assert fn(None, vp(z), vp(ws), 3, 1) == lib.CTD_EINVAL
        assert fn(d._h, vp(z), vp(ws), 3, 1) == lib.CTD_ENODEVICE and err().startswith(f"ctd_kkt_minres_shard_{p}_dev_async: ".encode())
    assert L.ctd_kkt_minres_shard_begin_dev_async(None, vp(ws), 3, 1) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_shard_begin_dev_async(d._h, vp(ws), 3, 1) == lib.CTD_ENODEVICE
    info = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info))
    assert L.ctd_kkt_minres_shard_info(None, vp(ws), 3, C.byref(info)) == lib.CTD_EINVAL
    assert L.ctd_kkt_minres_shard_info(d._h, vp(ws), 3, None) == lib.CTD_EINVAL
    bad = lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info) + 8)
    assert L.ctd_kkt_minres_shard_info(d._h, vp(ws), 3, C.byref(bad)) == lib.CTD_EINVAL and b"sizeof(ctd_minres_info)" in err()
    assert L.ctd_kkt_minres_shard_info(d._h, vp(ws), 3, C.byref(info)) == lib.CTD_ENODEVICE
    assert (z == 7.0).all() and not ws.any()
    # the whole-grid solve still refuses the shard handle, with the message it has always had
    ks.x = rhs.ctypes.data
    assert L.ctd_kkt_minres_dev(d._h, C.byref(ks), vp(rhs), vp(z), 1e-10, 10, 2, C.byref(info)) == lib.CTD_ENODEVICE
    d.close()
