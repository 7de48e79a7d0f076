"""CPU tests of the matrix-free products on time-step shards (ctd_jprod_shard_dev_async, ctd_jtprod_shard_dev_async,
ctd_hprod_shard_dev_async; ShardedDOCP.exchange_product_halo / exchange_product_rows): the header declares the three calls, the
binding lists them and the library exports them; a host-only handle refuses them with CTD_ENODEVICE before any other check; and
the two exchange helpers fill, over gloo, exactly the read sets the header documents -- restated from the header in
tests/shard_read_sets.py, not taken from dist.py.  The products themselves are checked on the GPU in tests/test_gpu_products_shard.py."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ctdirect_jl_amd as ct
from ctdirect_jl_amd import dist as ctdist
from shard_read_sets import constraint_read_set, variable_read_set

SHARD_SYMBOLS = ("ctd_jprod_shard_dev_async", "ctd_jtprod_shard_dev_async", "ctd_hprod_shard_dev_async")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_shard_product_symbols_declared_listed_exported():
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(ctd_\w+)\s*\(", f.read()))
    L = ct._lib.lib()
    for name in SHARD_SYMBOLS:
        assert name in declared, name
        assert name in ct._lib.SYMBOLS, name
        assert hasattr(L, name), name


@pytest.mark.parametrize("steps", [None, (3, 7)])
def test_host_only_handle_refuses_shard_products_first(steps):
    """CTD_ENODEVICE with valid and with NULL pointers, on a whole-grid and on a shard handle; only the NULL handle is checked
    before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1, steps=steps)
    L = ct._lib.lib()
    x, v, ov = (np.zeros(d.dim_NLP_variables) for _ in range(3))
    w, oc = (np.zeros(d.dim_NLP_constraints) for _ in range(2))
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    valid = {
        "ctd_jprod_shard_dev_async": (V(x), V(v), V(oc)),
        "ctd_jtprod_shard_dev_async": (V(x), V(w), V(ov)),
        "ctd_hprod_shard_dev_async": (V(x), V(w), 1.0, V(v), V(ov)),
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


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, prob, sch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = ctdist.ShardedDOCP(lambda steps=None: ct.DOCP(prob, N, sch, steps=steps, device=-1), N, world=world, rank=rank)
        d = sh.docp
        disc = d.discretization
        nvar, ncon, nv = d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v
        blk, eqs = disc._step_variables_block, disc._state_stage_eqs_block
        cb = eqs + disc._step_pathcons_block
        sb, se = ctdist.shard_steps(N, world, rank)
        g = np.random.default_rng(5).uniform(-1.0, 1.0, nvar)          # the same global vectors on every rank
        gw = np.random.default_rng(6).uniform(-1.0, 1.0, ncon)
        ok = True
        for full, (own, need), exchange in (
                (g, variable_read_set(sb, se, N, d.dims.NLP_x, d.dims.NLP_u, blk, nvar, nv, sch == "trapeze"), sh.exchange_product_halo),
                (gw, constraint_read_set(sb, se, N, cb, eqs, ncon), sh.exchange_product_rows)):
            mine = np.where(own, full, np.nan)
            for _ in range(2):                                          # (the second call runs on the cached index sets)
                t = torch.from_numpy(mine.copy())
                assert exchange(t) is t
                got = t.numpy()
                ok = ok and bool(np.array_equal(got[need], full[need])) and bool(np.isnan(got[~need]).all())
        ok = ok and (sh.owned_variables() == (sb * blk, se * blk if se < N else nvar - nv))
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("N,prob,sch", [(7, "goddard_all", "trapeze"), (8, "double_integrator_path", "midpoint"),
                                        (6, "goddard_all", "euler_implicit"), (10, "goddard_all", "gauss_legendre_2"),
                                        (3, "quadrotor", "trapeze")])
def test_exchange_helpers_fill_exactly_the_documented_read_sets(world, N, prob, sch):
    """every rank starts from its own entries (+ v) or its own rows, NaN elsewhere: after one exchange every index of the documented
    read set equals the global vector and every other index is still NaN (N = 3 on three ranks: one-step shards)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, N, prob, sch, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res), res
