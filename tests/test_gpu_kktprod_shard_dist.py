"""Two ranks on ONE GPU (gloo carries the collectives, as in test_gpu_products_shard_dist.py, on its two cases):
ShardedDOCP.kktprod with a sharded iterate, sharded multipliers, sharded directions and sharded diagonals -- every entry a rank
does not own is NaN until the exchanges fetch the few it reads -- with x exchanged by copy and with x read in place
(enable_peer_x).  On every rank the owned entries of rx and rc and the all-reduced v entries meet the bars of test_gpu_kktprod.py
against the oracle, everything else is still 777.0, the in-place x buffer is untouched, the two modes give the same bits, and
x_halo_valid / y_halo_valid reproduce them."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, prob, sch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, here)
        sys.path.insert(0, os.path.dirname(here))
        import ctdirect_jl_amd as ct
        from ctdirect_jl_amd import dist as ctdist
        from helpers import bench_inputs, describe
        from oracle.oracle import OracleDOCP
        from test_gpu_kktprod import Inputs, oracle_blocks
        torch.cuda.set_device(0)
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(o, prob, sch), perturb=1e-3)
        sh = ctdist.ShardedDOCP(lambda steps=None: ct.DOCP(prob, N, sch, device=0, steps=steps, pattern="structural"), N,
                                world=world, rank=rank)
        d = sh.docp
        nvar, ncon, nv = d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v
        w, sigma = Inputs(nvar, ncon), 0.7
        rx_ref, rx_bar, rc_ref, rc_bar, dropped = oracle_blocks(o, x, w.y, sigma, w.dx, w.dy, w.sx, w.sc)
        # (both cases were chosen so that the oracle's Hessian pattern leaves no true nonzero out)
        assert not dropped
        # what this rank holds: its own entries (+ the replicated nv tail) / its own rows, NaN everywhere else; of sx the nv tail
        # on the last rank only
        a, b = sh.owned_variables()
        ca, cz = sh.owned_constraints()
        own_v = np.zeros(nvar, dtype=bool)
        own_v[a:b] = True
        own_v[nvar - nv:] = True
        own_sx = own_v.copy()
        own_sx[nvar - nv:] = rank == world - 1
        own_c = np.zeros(ncon, dtype=bool)
        own_c[ca:cz] = True
        dev = lambda arr, own: torch.from_numpy(np.where(own, arr, np.nan)).cuda()        # noqa: E731
        new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")        # noqa: E731
        chk = {}

        def product(xd, yd, tag, **kw):
            rx, rc = sh.kktprod(xd, yd, dev(w.dx, own_v), dev(w.dy, own_c), sigma, dev(w.sx, own_sx), dev(w.sc, own_c),
                                (new(nvar), new(ncon)), **kw)
            torch.cuda.synchronize()
            gx, gc = rx.cpu().numpy(), rc.cpu().numpy()
            ex, ec = np.abs(gx - rx_ref), np.abs(gc - rc_ref)
            print(tag, "rank", rank, "max err / bar: rx", float(np.max((ex / rx_bar)[own_v])), "rc", float(np.max((ec / rc_bar)[own_c])))
            chk[tag + ' rx own + v'] = bool(np.all(ex[own_v] <= rx_bar[own_v]))
            chk[tag + ' rc own rows'] = bool(np.all(ec[own_c] <= rc_bar[own_c]))
            chk[tag + ' rx elsewhere untouched'] = bool(np.all(gx[~own_v] == 777.0))
            chk[tag + ' rc elsewhere untouched'] = bool(np.all(gc[~own_c] == 777.0))
            return gx, gc

        # x exchanged by copy: the halo entries of x and of y are fetched by the call itself
        xd, yd = dev(x, own_v), dev(w.y, own_c)
        copied = product(xd, yd, 'copy')
        # ... and left there: the inner iterations of one outer step skip those two all-gathers
        again = product(xd, yd, 'valid', x_halo_valid=True, y_halo_valid=True)
        chk['x_halo_valid, y_halo_valid'] = bool(np.array_equal(again[0], copied[0]) and np.array_equal(again[1], copied[1]))
        # x read in place: the local copy of everything the rank does not own stays NaN
        xp, yp = dev(x, own_v), dev(w.y, own_c)
        sh.enable_peer_x(xp)
        dist.barrier()
        peer = product(xp, yp, 'peer')
        again = product(xp, yp, 'peer valid', y_halo_valid=True)
        torch.cuda.synchronize()
        dist.barrier()                      # nobody frees its buffer while the other rank's kernel may still read it
        chk['peer x untouched'] = bool(np.array_equal(np.isnan(xp.cpu().numpy()), ~own_v))
        chk['peer == copy'] = bool(np.array_equal(peer[0], copied[0]) and np.array_equal(peer[1], copied[1]))
        chk['peer, y_halo_valid'] = bool(np.array_equal(again[0], peer[0]) and np.array_equal(again[1], peer[1]))
        sh.close()
        bad = [k for k, v_ in chk.items() if not v_]
        q.put((rank, True if not bad else bad))
    except Exception as e:      # noqa: BLE001 -- the parent reports it
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("N,prob,sch", [(301, "goddard_all", "trapeze"), (400, "goddard", "gauss_legendre_2")])
def test_two_ranks_one_gpu_sharded_kkt_product(N, prob, sch):
    assert torch.cuda.is_available()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, N, prob, sch, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok is True for _, ok in res), res
