"""The sharded MINRES solve with the joined form of the log-depth Schur preconditioner through a real process group, modelled on
tests/test_gpu_kkt_schur_cr_shard_dist.py: two ranks (fresh processes, gloo) sharing device 0 build
ShardedDOCP.kkt_schur_cr_joint_precond -- the diagonal pair, one halo exchange of px, one of the Jacobian values of the next rank's
first block, the local factor, the all-gather of the factor records, the join -- and run ShardedDOCP.kkt_minres with it: the halo of
the Lanczos vector and the two send slots, which also carry the solve records, go through the group's all-gathers.  On their owned
entries they give the BITS of dist.kkt_schur_cr_joint_shards + dist.kkt_minres_shards with the same two shards in one process, and
the same MinresInfo.  double_integrator_path, midpoint, N = 20,
cuts from shard_steps, rtol 1e-10.  The parent supervises: one time limit for both ranks, both are killed on the first failure,
nothing is retried."""
import os
import queue
import socket
import sys
import time
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
PROB, SCH, N, WORLD, LIMIT = "double_integrator_path", "midpoint", 20, 2, 150.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs():
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_gpu_kkt_minres import minres_case
    c = minres_case(PROB, SCH, N)
    return [torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("x", "y", "sx", "sc", "rhs")]


def _worker(rank, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        torch.cuda.set_device(0)
        x, y, sx, sc, rhs = _inputs()
        import ctdirect_jl_amd as ct
        from ctdirect_jl_amd import dist as cdist
        sd = cdist.ShardedDOCP(lambda steps=None: ct.DOCP(PROB, N, SCH, device=0, steps=steps, pattern="structural", value_order="csr"), N,
                               world=WORLD, rank=rank)
        P = sd.kkt_schur_cr_joint_precond(x, y, 1.0, sx, sc, x_halo_valid=True, y_halo_valid=True)
        bad = sd.docp.kkt_schur_cr_joint_info(P)
        z, info = sd.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond=P, rtol=1e-10, x_halo_valid=True, y_halo_valid=True)
        za = z.clone()
        zb, info_b = sd.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond="schur_cr_joint", rtol=1e-10, x_halo_valid=True, y_halo_valid=True)
        torch.cuda.synchronize()
        lay = sd.docp.kkt_minres_schur_joint_layout(WORLD, rank)
        own = torch.zeros(lay.n, dtype=torch.bool, device="cuda")
        for lo, hi in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            own[lo:hi] = True
        same = bool(torch.equal(za[own], zb[own])) and tuple(info) == tuple(info_b)
        # a workspace of another family never reaches the joined phases
        try:
            sd.docp.kkt_minres_schur_joint_begin(P, sd.docp.kkt_minres_shard_workspace(WORLD), rank)
            same = False
        except ValueError:
            pass
        q.put((rank, (za.cpu().numpy(), tuple(info), P.px.cpu().numpy(), P.pc.cpu().numpy(), bad, same)))
        dist.barrier()
        sd.close()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_two_processes_give_the_bits_of_one_process():
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()

    def stop(why):
        for p in procs:
            if p.is_alive():
                p.kill()
        for p in procs:
            p.join(timeout=10)
        pytest.fail(why)

    deadline, res = time.monotonic() + LIMIT, {}
    while len(res) < WORLD:
        try:
            rank, payload = q.get(timeout=1.0)
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                stop(f"a rank ended with exit codes {[p.exitcode for p in procs]}")
            if time.monotonic() > deadline:
                stop("the ranks did not finish within the time limit")
            continue
        if isinstance(payload, str):
            stop(f"rank {rank} failed:\n{payload}")
        res[rank] = payload
    for p in procs:
        p.join(timeout=30)
        if p.exitcode != 0:
            stop(f"exit codes {[p.exitcode for p in procs]}")
    # the same two shards in this process, each with the preconditioner its rank computed
    import ctdirect_jl_amd as ct
    from ctdirect_jl_amd import dist as cdist
    from ctdirect_jl_amd.docp import MinresInfo
    x, y, sx, sc, rhs = _inputs()
    hs = [ct.DOCP(PROB, N, SCH, device=0, pattern="structural", value_order="csr", steps=cdist.shard_steps(N, WORLD, r)) for r in range(WORLD)]
    # the joined factors from the (px, pc) each rank computed -- px with the halo its rank received -- and this process's Jacobian
    # values of the same x on the whole grid (a rank's own rows and the rows of the next rank's first block)
    full = ct.DOCP(PROB, N, SCH, device=0, pattern="structural", value_order="csr")
    jvals = full.cons_jac(x)[1]
    for r in range(WORLD):
        assert res[r][4] == -1 and res[r][5], (r, "a failed pivot, precond='schur_cr_joint' differs from the preconditioner built by hand, "
                                                  "or a foreign workspace was accepted")
    pxs, pcs = ([torch.from_numpy(res[r][k]).cuda() for r in range(WORLD)] for k in (2, 3))
    pres = cdist.kkt_schur_cr_joint_shards(hs, jvals, pxs, pcs, sc)
    zs, infos = cdist.kkt_minres_shards(hs, [x] * WORLD, y, rhs, sx=sx, sc=sc, precond=pres, rtol=1e-10)
    assert infos[0].status == "converged" and infos[0] == infos[1], infos
    for r in range(WORLD):
        lay = hs[r].kkt_minres_schur_joint_layout(WORLD, r)
        assert MinresInfo(*res[r][1]) == infos[r], (r, res[r][1], infos[r])
        got, want = res[r][0], zs[r].cpu().numpy()
        for lo, hi in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            assert np.array_equal(got[lo:hi], want[lo:hi]), (r, lo, hi, "not the bits of the in-process solve")
    for h in hs + [full]:
        h.close()
