"""The joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*) beside its shard form on one GPU, the shards being
handles of ONE process on ONE stream: their launches serialise, so the times for G > 1 are a rehearsal of the phase split and of
the copies that stand for the two all-gathers, NOT a multi-GPU figure.

  cfg2     Goddard, Gauss-Legendre 2, N = 10 000 (m = 9) on CSR handles, G in {1, 2, 4, 8} (cuts of dist.shard_steps): microseconds,
           summed over all ranks, for the four phases of the joined form -- factor_local, factor_join (with the copy of the
           records), solve_local, solve_join (with the copy of the records) -- and for the factor and the solve of the shard form
           (`cut_*`) in the same session.  All rows alternated over --rounds rounds after a warm-up; median, min / max as the spread.
           The entry points are called through ctypes on preallocated buffers: the timed region holds launches and device copies
           only.  In the same rounds: microseconds per MINRES iteration (64 iterations, rtol = 0, device events around MinresPhases.iterate) for the joined and the
           cut form.
  solve    Goddard trapeze N = 2000, sc = 1e-8 U(1, 2) (the system of bench/kkt_schur_cr_shard.py), rtol = 1e-10: iterations, and
           build (the factors of all ranks from the diagonal pair; the joined form with its gather and joins) and solve wall time
           for G in {1, 2, 4, 8}, joined against cut, alternated over --rounds rounds.

  join     cfg2 on 8 ranks: nothing but 200 applications (solve_local, the copies, solve_join), for a run under a kernel trace
           (rocprofv3 --kernel-trace --stats -- python bench/kkt_schur_cr_joint.py --only join), whose per-kernel statistics give
           the reduced solve and the correction separately; the script itself times nothing here.

Prints one JSON line (and writes it to --out when given).

    python bench/kkt_schur_cr_joint.py [--rounds 5] [--only cfg2,solve,join] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from ctdirect_jl_amd import _lib, dist  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from kkt_schur import ITERS, spread, up  # noqa: E402
from kkt_schur_cr_shard import RANKS, handles  # noqa: E402
from products import timed  # noqa: E402


def cfg2(rounds):
    prob, sch, N = "goddard", "gauss_legendre_2", 10_000
    L = _lib.lib()
    stream = torch.cuda.current_stream(0)
    full = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    full.set_stream(stream)
    nvar, ncon = full.dim_NLP_variables, full.dim_NLP_constraints
    r = np.random.default_rng(21)
    x = up(bench_inputs(describe(full, prob, sch), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, ncon))
    rhs_n = up(r.uniform(-1, 1, nvar + ncon))

    def iteration_us(ph):
        ph.start(0.0, 10 * ITERS)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        ph.iterate(ITERS)
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / ITERS

    px, pc = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
    jvals = full.cons_jac(x)[1]
    out = torch.zeros(ncon, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731  (one rank has no record)
    fns, meta = {}, {}
    for G in RANKS:
        hs = handles(prob, sch, N, G, full)
        for h in hs:
            h.set_stream(stream)
        Ps = dist.kkt_schur_cr_joint_shards(hs, jvals, px, pc, sc)
        Qs = [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc) for h in hs]
        torch.cuda.synchronize()
        assert all(h.kkt_schur_cr_joint_info(P) == -1 for h, P in zip(hs, Ps))
        fslot, xslot = int(Ps[0].layout.factor_slot), int(Ps[0].layout.solve_slot)
        fg = torch.zeros(G * fslot, dtype=torch.float64, device="cuda")
        xg = torch.zeros(G * xslot, dtype=torch.float64, device="cuda")

        def ok(st):
            assert st == _lib.CTD_OK, st

        def factor_local(hs=hs, Ps=Ps, G=G):
            for k, (h, P) in enumerate(zip(hs, Ps)):
                ok(L.ctd_kkt_schur_cr_joint_factor_local_dev_async(h._h, ptr(jvals), ptr(px), ptr(sc), ptr(P.ws), ptr(P.send), G, k))

        def factor_join(hs=hs, Ps=Ps, G=G, fg=fg, fslot=fslot):
            for k, P in enumerate(Ps):
                fg[k * fslot:(k + 1) * fslot].copy_(P.send)
            for k, (h, P) in enumerate(zip(hs, Ps)):
                ok(L.ctd_kkt_schur_cr_joint_factor_join_dev_async(h._h, ptr(P.ws), ptr(fg), G, k))

        def solve_local(hs=hs, Ps=Ps, G=G):
            for k, (h, P) in enumerate(zip(hs, Ps)):
                ok(L.ctd_kkt_schur_cr_joint_solve_local_dev_async(h._h, ptr(P.ws), ptr(rhs), ptr(out), ptr(P.xsend), G, k))

        def solve_join(hs=hs, Ps=Ps, G=G, xg=xg, xslot=xslot):
            for k, P in enumerate(Ps):
                xg[k * xslot:(k + 1) * xslot].copy_(P.xsend)
            for k, (h, P) in enumerate(zip(hs, Ps)):
                ok(L.ctd_kkt_schur_cr_joint_solve_join_dev_async(h._h, ptr(P.ws), ptr(xg), ptr(out), G, k))

        key = f"G{G}"
        us = lambda fn: (lambda: 1e3 * timed(fn, stream, 0.02))      # noqa: E731
        fns[(key, "factor_local_us")] = us(factor_local)
        fns[(key, "solve_local_us")] = us(solve_local)
        if G > 1:
            fns[(key, "factor_join_us")] = us(factor_join)
            fns[(key, "solve_join_us")] = us(solve_join)
        fns[(key, "cut_factor_us")] = us(lambda hs=hs, Qs=Qs: [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc, Q.ws) for h, Q in zip(hs, Qs)])
        fns[(key, "cut_solve_us")] = us(lambda hs=hs, Qs=Qs: [h.kkt_schur_cr_shard_solve(Q, rhs, out=out, sync=False) for h, Q in zip(hs, Qs)])
        phj = dist.minres_shards(hs, [x] * G, y, rhs_n, sx=sx, sc=sc, precond=Ps)
        phc = dist.minres_shards(hs, [x] * G, y, rhs_n, sx=sx, sc=sc, precond=Qs)
        fns[(key, "iteration_us")] = lambda ph=phj: iteration_us(ph)
        fns[(key, "cut_iteration_us")] = lambda ph=phc: iteration_us(ph)
        meta[key] = dict(n_ranks=G, interior_blocks_per_rank=[int(P.layout.n_int) for P in Ps], levels_per_rank=[int(P.layout.n_levels) for P in Ps],
                         launches_per_rank={w: [int(getattr(P.layout, w + "_launches")) for P in Ps]
                                            for w in ("factor_local", "factor_join", "solve_local", "solve_join")},
                         workspace_doubles_per_rank=[int(P.layout.workspace) for P in Ps],
                         cut_workspace_doubles_per_rank=[int(Q.layout.workspace) for Q in Qs])
    for fn in fns.values():
        fn()                                    # warm-up
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(fn())
    table = {}
    for (key, what), ts in res.items():
        table.setdefault(key, {})[what] = spread(ts)
    for key, m in meta.items():
        table[key].update(m)
    return dict(problem=prob, scheme=sch, N=N, nvar=nvar, ncon=ncon, block_rows=int(Ps[0].layout.block_rows), rounds=rounds, rows=table)


def solve(rounds):
    from scipy.sparse.linalg import eigsh
    from test_gpu_kkt_minres import minres_case
    prob, sch, N = "goddard", "trapeze", 2000
    c = minres_case(prob, sch, N)
    lam_min = float(eigsh(c["H"], k=1, which="SA", return_eigenvectors=False, tol=1e-8)[0])
    sx_h, sc_h = c["sx"] + max(0.0, -lam_min) * (1.0 + 1e-6), c["sc"] * 1e-6          # (minres_case's sc is 1e-2 U(1, 2))
    full = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    n = c["nvar"] + c["ncon"]
    x, y, sx, sc, rhs = up(c["x"]), up(c["y"]), up(sx_h), up(sc_h), up(c["rhs"])
    cap = 20 * n
    jvals = full.cons_jac(x)[1]
    hs = {G: handles(prob, sch, N, G, full) for G in RANKS}

    def build(G, joined):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        px, pc = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
        Ps = dist.kkt_schur_cr_joint_shards(hs[G], jvals, px, pc, sc) if joined else [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc) for h in hs[G]]
        torch.cuda.synchronize()
        return Ps, 1e3 * (time.perf_counter() - t0)

    def run(G, Ps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zs, infos = dist.kkt_minres_shards(hs[G], [x] * G, y, rhs, sx=sx, sc=sc, precond=Ps, rtol=1e-10, max_iter=cap, check_every=64)
        torch.cuda.synchronize()
        return infos[0], 1e3 * (time.perf_counter() - t0)

    rows, ts = {}, {}
    for rnd in range(rounds + 1):               # (round 0: the warm-up)
        for G in RANKS:
            for joined in (True, False):
                key = f"G{G}_" + ("joined" if joined else "cut")
                Ps, b = build(G, joined)
                info, s = run(G, Ps)
                if rnd == 0:
                    rows[key] = dict(status=info.status, iterations=info.iterations)
                    ts[key] = {"build_ms": [], "solve_ms": [], "total_ms": []}
                    continue
                assert info.iterations == rows[key]["iterations"]
                for what, v in (("build_ms", b), ("solve_ms", s), ("total_ms", b + s)):
                    ts[key][what].append(v)
    for key in rows:
        rows[key].update({what: spread(v) for what, v in ts[key].items()})
    return dict(problem=prob, scheme=sch, N=N, n=n, scv=1e-8, rtol=1e-10, cap=cap, rounds=rounds, rows=rows)


def join(reps=200, G=8):
    prob, sch, N = "goddard", "gauss_legendre_2", 10_000
    full = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    nvar, ncon = full.dim_NLP_variables, full.dim_NLP_constraints
    r = np.random.default_rng(21)
    x = up(bench_inputs(describe(full, prob, sch), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, ncon))
    px, pc = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
    hs = handles(prob, sch, N, G, full)
    Ps = dist.kkt_schur_cr_joint_shards(hs, full.cons_jac(x)[1], px, pc, sc)
    out = torch.zeros(ncon, dtype=torch.float64, device="cuda")
    for _ in range(reps):
        dist.kkt_schur_cr_joint_apply_shards(hs, Ps, rhs, out)
    torch.cuda.synchronize()
    return dict(problem=prob, scheme=sch, N=N, n_ranks=G, applications=reps, finite=bool(torch.isfinite(out).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="cfg2,solve")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_schur_cr_joint.py needs a GPU"
    only = set(args.only.split(","))
    res = {"bench": "kkt_schur_cr_joint", "device": torch.cuda.get_device_name(0)}
    if "cfg2" in only:
        res["cfg2"] = cfg2(args.rounds)
    if "solve" in only:
        res["solve"] = solve(args.rounds)
    if "join" in only:
        res["join"] = join()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
