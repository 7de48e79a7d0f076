"""Two ranks on ONE GPU (gloo carries the collectives, as in test_gpu_dist.py): ShardedDOCP.jprod / jtprod / hprod with a sharded
iterate and sharded directions -- every entry a rank does not own is NaN until the exchange helpers fetch the few it reads --
with x exchanged by copy and with x read in place (enable_peer_x).  On every rank the owned entries, the all-reduced d/dv entries
and the stitched Jv meet the criteria of test_gpu_products.py / test_gpu_hprod.py against the oracle's structural Jacobian and
Hessian, and the two modes give the same bits."""
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
        from test_gpu_hprod import RTOL as H_RTOL
        from test_gpu_hprod import oracle_product, rand
        from test_gpu_products import RTOL as J_RTOL
        from test_gpu_products import csc_products, directions
        torch.cuda.set_device(0)
        o = OracleDOCP(prob, sch, N)
        o.set_pattern_mode(1)
        x = bench_inputs(describe(o, prob, sch), perturb=1e-3)
        sh = ctdist.ShardedDOCP(lambda steps=None: ct.DOCP(prob, N, sch, device=0, steps=steps, pattern="structural"), N,
                                world=world, rank=rank)
        d = sh.docp
        nvar, ncon, nv = d.dim_NLP_variables, d.dim_NLP_constraints, d.dims.NLP_v
        v, w = directions(nvar, ncon)
        y, sigma = rand(ncon, 4), 0.7
        # references: the oracle's structural Jacobian and Hessian
        colptr, rowval = o.jac_pattern()
        jv, sv, jtw, sw = csc_products(colptr, rowval, o.jac_coord(x), v, w, ncon)
        hv, hs, dropped = oracle_product(o, x, y, sigma, v)
        h0, hs0, dropped0 = oracle_product(o, x, np.zeros(ncon), sigma, v)
        # both cases were chosen so that the oracle's Hessian pattern leaves no true nonzero out: every entry of the product
        # can then be held to the oracle's bound, with none set aside for a finite-difference check
        assert not dropped and not dropped0
        # what this rank holds: its own entries (+ the replicated nv tail) / its own rows, NaN everywhere else
        a, b = sh.owned_variables()
        ca, cz = sh.owned_constraints()
        own_v = np.zeros(nvar, dtype=bool)
        own_v[a:b] = True
        own_v[nvar - nv:] = True
        own_c = np.zeros(ncon, dtype=bool)
        own_c[ca:cz] = True
        dev = lambda arr, own: torch.from_numpy(np.where(own, arr, np.nan)).cuda()        # noqa: E731
        new = lambda n: torch.full((n,), 777.0, dtype=torch.float64, device="cuda")        # noqa: E731
        chk = {}

        def products(xd, tag):
            outs = {}
            out = sh.jprod(xd, dev(v, own_v), new(ncon), stitch=False)
            torch.cuda.synchronize()
            g = out.cpu().numpy()
            chk[tag + ' jprod own rows'] = bool(np.all(np.abs(g - jv)[own_c] <= (J_RTOL * sv + 1e-300)[own_c]))
            chk[tag + ' jprod elsewhere untouched'] = bool(np.all(g[~own_c] == 777.0))
            outs['jprod'] = g
            g = sh.jprod(xd, dev(v, own_v), new(ncon), stitch=True).cpu().numpy()
            chk[tag + ' jprod stitched'] = bool(np.all(np.abs(g - jv) <= J_RTOL * sv + 1e-300))
            outs['jprod stitched'] = g
            g = sh.jtprod(xd, dev(w, own_c), new(nvar)).cpu().numpy()
            chk[tag + ' jtprod own + d/dv'] = bool(np.all(np.abs(g - jtw)[own_v] <= (J_RTOL * sw + 1e-300)[own_v]))
            chk[tag + ' jtprod elsewhere untouched'] = bool(np.all(g[~own_v] == 777.0))
            outs['jtprod'] = g
            for name, yy, ref, scale in (('hprod', y, hv, hs), ('hprod objective', None, h0, hs0)):
                yd = None if yy is None else dev(yy, own_c)
                g = sh.hprod(xd, yd, dev(v, own_v), sigma, new(nvar)).cpu().numpy()
                chk[f'{tag} {name} own + d/dv'] = bool(np.all(np.abs(g - ref)[own_v] <= (H_RTOL * np.maximum(1.0, scale))[own_v]))
                chk[f'{tag} {name} elsewhere untouched'] = bool(np.all(g[~own_v] == 777.0))
                outs[name] = g
            return outs

        # x exchanged by copy: the halo entries of x are fetched by the product calls themselves
        xd = dev(x, own_v)
        copied = products(xd, 'copy')
        # ... and left there: a later product of the same outer iteration skips that all-gather
        g = sh.jtprod(xd, dev(w, own_c), new(nvar), x_halo_valid=True).cpu().numpy()
        chk['x_halo_valid'] = bool(np.array_equal(g, copied['jtprod']))
        # x read in place: the local copy of everything the rank does not own stays NaN
        xp = dev(x, own_v)
        sh.enable_peer_x(xp)
        dist.barrier()
        peer = products(xp, 'peer')
        torch.cuda.synchronize()
        dist.barrier()                      # nobody frees its buffer while the other rank's kernel may still read it
        chk['peer x untouched'] = bool(np.array_equal(np.isnan(xp.cpu().numpy()), ~own_v))
        for k in copied:
            chk['peer == copy: ' + k] = bool(np.array_equal(peer[k], copied[k]))
        sh.close()
        bad = [k for k, v_ in chk.items() if not v_]
        q.put((rank, True if not bad else bad))
    except Exception as e:      # noqa: BLE001 -- the parent reports it
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("N,prob,sch", [(301, "goddard_all", "trapeze"), (400, "goddard", "gauss_legendre_2")])
def test_two_ranks_one_gpu_sharded_products(N, prob, sch):
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
