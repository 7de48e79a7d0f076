"""CPU tests of the shard form of the fused KKT product (ctd_kktprod_shard_dev_async, DOCP.kktprod_shard,
ShardedDOCP.exchange_kkt_halo): the header declares the call, the binding lists it with its 10 arguments and the library exports it;
a host-only handle refuses it with CTD_ENODEVICE before any other check; DOCP.kktprod_shard checks the lengths of its vectors; and
exchange_kkt_halo fills, over gloo and with ONE collective call, exactly the read sets the header documents -- restated from the
header in tests/shard_read_sets.py, not taken from dist.py -- in both tensors.  The product itself is checked on the GPU in
tests/test_gpu_kktprod_shard.py."""
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

NAME = "ctd_kktprod_shard_dev_async"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctdirect_hip.h")


def test_symbol_declared_listed_exported():
    with open(HEADER) as f:
        text = f.read()
    assert NAME in set(re.findall(r"\b(ctd_\w+)\s*\(", text))
    decl = re.search(NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert decl and len(decl.group(1).split(",")) == 10, decl
    res, args = ct._lib.SYMBOLS[NAME]
    assert res is C.c_int32 and len(args) == 10 and args[3] is C.c_double
    assert hasattr(ct._lib.lib(), NAME)


@pytest.mark.parametrize("steps", [None, (3, 7)])
def test_host_only_handle_refuses_first(steps):
    """CTD_ENODEVICE with valid, NULL and aliased pointers, on a whole-grid and on a shard handle; only the NULL handle is checked
    before the device"""
    d = ct.DOCP("goddard", 10, "gauss_legendre_2", device=-1, steps=steps)
    L = ct._lib.lib()
    fn = getattr(L, NAME)
    x, dx, sx, rx = (np.zeros(d.dim_NLP_variables) for _ in range(4))
    y, dy, sc, rc = (np.zeros(d.dim_NLP_constraints) for _ in range(4))
    V = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
    valid = (V(x), V(y), 1.0, V(dx), V(dy), V(sx), V(sc), V(rx), V(rc))
    null = (None, None, 1.0, None, None, None, None, None, None)
    aliased = (V(x), V(y), 1.0, V(dx), V(dy), V(sx), V(sc), V(dx), V(dx))
    for a in (valid, null, aliased):
        assert fn(d._h, *a) == ct._lib.CTD_ENODEVICE, a
        assert b"host-only" in L.ctd_last_error(d._h)
        assert NAME.encode() in L.ctd_last_error(d._h)
        assert fn(None, *a) == ct._lib.CTD_EINVAL, a


def test_kktprod_shard_checks_lengths():
    d = ct.DOCP("goddard", 10, "midpoint", device=-1, steps=(3, 7))
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    t = lambda n: torch.zeros(n, dtype=torch.float64)          # noqa: E731
    good = dict(x=t(nvar), y=t(ncon), dx=t(nvar), dy=t(ncon), sx=t(nvar), sc=t(ncon))
    for name, n in (("x", nvar), ("y", ncon), ("dx", nvar), ("dy", ncon), ("sx", nvar), ("sc", ncon)):
        a = dict(good)
        a[name] = t(n + 1)
        with pytest.raises(ValueError, match=rf"{name} has {n + 1} entries, expected"):
            d.kktprod_shard(a["x"], a["y"], a["dx"], a["dy"], sx=a["sx"], sc=a["sc"], out=(t(nvar), t(ncon)))
    for k, out in enumerate(((t(nvar + 1), t(ncon)), (t(nvar), t(ncon - 1)))):
        with pytest.raises(ValueError, match=rf"out\[{k}\] has \d+ entries, expected"):
            d.kktprod_shard(good["x"], good["y"], good["dx"], good["dy"], sx=good["sx"], sc=good["sc"], out=out)
    for name in ("dx", "dy"):
        a = dict(good)
        a[name] = None
        with pytest.raises(ValueError, match=f"{name} is required"):
            d.kktprod_shard(a["x"], a["y"], a["dx"], a["dy"], out=(t(nvar), t(ncon)))
    # vectors of the right lengths pass these checks: what stops them here is that they are not on a GPU
    with pytest.raises(ValueError, match="GPU"):
        d.kktprod_shard(good["x"], None, good["dx"], good["dy"], out=(t(nvar), t(ncon)))


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
        own_v, need_v = variable_read_set(sb, se, N, d.dims.NLP_x, d.dims.NLP_u, blk, nvar, nv, sch == "trapeze")
        own_c, need_c = constraint_read_set(sb, se, N, cb, eqs, ncon)
        calls = [0]
        gather = ctdist._all_gather_into

        def counted(recv, send, group=None):
            calls[0] += 1
            return gather(recv, send, group)

        ctdist._all_gather_into = counted
        ok = True
        for it in range(2):                                             # (the second call runs on the cached index sets)
            tx = torch.from_numpy(np.where(own_v, g, np.nan))
            tc = torch.from_numpy(np.where(own_c, gw, np.nan))
            rx, rc = sh.exchange_kkt_halo(tx, tc)
            ok = ok and rx is tx and rc is tc and calls[0] == it + 1      # exactly one collective call per exchange
            gx, gc = tx.numpy(), tc.numpy()
            ok = ok and bool(np.array_equal(gx[need_v], g[need_v])) and bool(np.isnan(gx[~need_v]).all())
            ok = ok and bool(np.array_equal(gc[need_c], gw[need_c])) and bool(np.isnan(gc[~need_c]).all())
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("N,prob,sch", [(7, "goddard_all", "trapeze"), (8, "double_integrator_path", "midpoint"),
                                        (6, "goddard_all", "euler_implicit"), (10, "goddard_all", "gauss_legendre_2"),
                                        (3, "quadrotor", "trapeze")])
def test_exchange_kkt_halo_fills_exactly_the_documented_read_sets(world, N, prob, sch):
    """every rank starts from its own entries (+ v) and its own rows, NaN elsewhere: after one exchange -- one collective call --
    every index of the two documented read sets equals the global vector and every other index is still NaN (N = 3 on three
    ranks: one-step shards)"""
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
