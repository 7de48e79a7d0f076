"""The shard form of the log-depth Schur preconditioner (DOCP.kkt_schur_cr_shard_factor, dist.minres_shards with one
SchurCrShardPrecond per shard) on one GPU, the shards being handles of ONE process on ONE stream: their launches serialise, so the
times for G > 1 are a rehearsal of the phase split and of the copies that stand for the gathers, NOT a multi-GPU figure.  The
iteration counts do carry over.

  cfg2     Goddard, Gauss-Legendre 2, N = 10 000 (m = 9) on CSR handles, G in {1, 2, 4, 8} (cuts of dist.shard_steps): microseconds
           for the factor of all ranks, for the solve of all ranks, and per MINRES iteration (64 iterations, rtol = 0, device events
           around MinresPhases.iterate), with the levels per rank and the launches per rank and iteration.  In the same session: the
           whole-grid iteration with the log-depth preconditioner (`whole_cr`) and with the diagonal (`whole_diag`), and the
           diagonal shard form with one rank (`shard1_diag`), so that G = 1 can be set beside `whole_cr` as bench/kkt_minres_shard.py
           sets `shard1` beside `whole`.  All rows alternated over --rounds rounds after a warm-up; median, min / max as the spread.
  solve    Goddard trapeze N = 2000, sc = 1e-8 U(1, 2) (the system of bench/kkt_schur_cr.py), rtol = 1e-10: iterations, and build
           (the factors of all ranks from the diagonal pair) and solve wall time for G in {1, 2, 4, 8}, alternated over --rounds
           rounds; the diagonal shard solve (one rank) once, capped at 20 n iterations.

Prints one JSON line (and writes it to --out when given).

    python bench/kkt_schur_cr_shard.py [--rounds 5] [--only cfg2,solve] [--out FILE]
"""
import argparse
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
from ctdirect_jl_amd import dist  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from kkt_schur import ITERS, spread, up  # noqa: E402
from products import timed  # noqa: E402

RANKS = (1, 2, 4, 8)


def handles(prob, sch, N, G, full):
    kw = dict(device=0, pattern="structural", value_order="csr")
    return [full] if G == 1 else [ct.DOCP(prob, N, sch, steps=dist.shard_steps(N, G, k), **kw) for k in range(G)]


def cfg2(rounds):
    prob, sch, N = "goddard", "gauss_legendre_2", 10_000
    stream = torch.cuda.current_stream(0)
    full = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    full.set_stream(stream)
    nvar, ncon = full.dim_NLP_variables, full.dim_NLP_constraints
    n = nvar + ncon
    r = np.random.default_rng(21)
    x = up(bench_inputs(describe(full, prob, sch), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, n))
    px, pc = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
    jvals = full.cons_jac(x)[1]
    z, out = torch.empty(n, dtype=torch.float64, device="cuda"), torch.zeros(ncon, dtype=torch.float64, device="cuda")
    rc = rhs[nvar:].contiguous()
    Pw = full.kkt_schur_cr_factor(jvals, px, pc, sc, torch.empty(full.kkt_schur_cr_layout().workspace, dtype=torch.float64, device="cuda"))

    def event_us(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / per

    def whole(precond):
        full.kkt_minres_start(x, y, rhs, z, sx=sx, sc=sc, precond=precond, rtol=0.0)
        return event_us(lambda: full.kkt_minres_iters(x, y, z, ITERS, sx=sx, sc=sc), ITERS)

    def phases(ph):
        ph.start(0.0, 10 * ITERS)
        return event_us(lambda: ph.iterate(ITERS), ITERS)

    fns = {("whole_cr", "iteration_us"): lambda: whole(Pw), ("whole_diag", "iteration_us"): lambda: whole((px, pc))}
    ph_diag = dist.minres_shards([full], [x], y, rhs, sx=sx, sc=sc, precond=(px, pc))
    fns[("shard1_diag", "iteration_us")] = lambda: phases(ph_diag)
    meta = {}
    for G in RANKS:
        hs = handles(prob, sch, N, G, full)
        for h in hs:
            h.set_stream(stream)
        Ps = [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc) for h in hs]
        torch.cuda.synchronize()
        assert all(h.kkt_schur_cr_shard_info(P) == -1 for h, P in zip(hs, Ps))
        ph = dist.minres_shards(hs, [x] * G, y, rhs, sx=sx, sc=sc, precond=Ps)
        key = f"G{G}"
        fns[(key, "factor_us")] = lambda hs=hs, Ps=Ps: 1e3 * timed(lambda: [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc, P.ws) for h, P in zip(hs, Ps)], stream, 0.02)
        fns[(key, "solve_us")] = lambda hs=hs, Ps=Ps: 1e3 * timed(lambda: [h.kkt_schur_cr_shard_solve(P, rc, out=out, sync=False) for h, P in zip(hs, Ps)], stream, 0.02)
        fns[(key, "iteration_us")] = lambda ph=ph: phases(ph)
        lv = [int(P.layout.n_levels) for P in Ps]
        # per rank and iteration: K v (2), (A), (B), the solve, its partial sums, (C)
        meta[key] = dict(n_ranks=G, blocks_per_rank=[int(P.layout.n_blocks) for P in Ps], levels_per_rank=lv,
                         launches_per_rank_and_iteration=[2 + 3 + int(P.layout.solve_launches) + 1 for P in Ps],
                         factor_launches_per_rank=[int(P.layout.factor_launches) for P in Ps])
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
    med = lambda k: table[k]["iteration_us"]["median"]      # noqa: E731
    compare = dict(G1_minus_whole_cr_us=round(med("G1") - med("whole_cr"), 2), shard1_diag_minus_whole_diag_us=round(med("shard1_diag") - med("whole_diag"), 2),
                   whole_cr_levels=int(Pw.layout.n_levels), whole_cr_launches_per_iteration=2 + 3 + int(Pw.layout.solve_launches) + 1)
    return dict(problem=prob, scheme=sch, N=N, nvar=nvar, ncon=ncon, block_rows=int(Pw.layout.block_rows), iterations=ITERS, rounds=rounds,
                rows=table, compare=compare)


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

    def run(G, precond):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zs, infos = dist.kkt_minres_shards(hs[G], [x] * G, y, rhs, sx=sx, sc=sc, precond=precond, rtol=1e-10, max_iter=cap, check_every=64)
        torch.cuda.synchronize()
        return infos[0], 1e3 * (time.perf_counter() - t0)

    def build(G):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        px, pc = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
        Ps = [h.kkt_schur_cr_shard_factor(jvals, px, pc, sc) for h in hs[G]]
        torch.cuda.synchronize()
        return Ps, 1e3 * (time.perf_counter() - t0)

    pair = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
    dist.kkt_minres_shards(hs[1], [x], y, rhs, sx=sx, sc=sc, precond=pair, rtol=1e-10, max_iter=4)       # warm-up
    info, ms = run(1, pair)
    rows = {"diag_shard1": dict(status=info.status, iterations=info.iterations, capped=info.status == "max_iter", solve_ms=round(ms, 2))}
    ts = {G: {"build_ms": [], "solve_ms": [], "total_ms": []} for G in RANKS}
    for rnd in range(rounds + 1):               # (round 0: the warm-up)
        for G in RANKS:
            Ps, b = build(G)
            info, s = run(G, Ps)
            if rnd == 0:
                rows[f"G{G}"] = dict(status=info.status, iterations=info.iterations, levels_per_rank=[int(P.layout.n_levels) for P in Ps],
                                     first_bad_blocks=[h.kkt_schur_cr_shard_info(P) for h, P in zip(hs[G], Ps)])
                continue
            assert info.iterations == rows[f"G{G}"]["iterations"]
            for what, v in (("build_ms", b), ("solve_ms", s), ("total_ms", b + s)):
                ts[G][what].append(v)
    for G in RANKS:
        rows[f"G{G}"].update({what: spread(v) for what, v in ts[G].items()})
    return dict(problem=prob, scheme=sch, N=N, n=n, scv=1e-8, rtol=1e-10, cap=cap, rounds=rounds, lambda_min_H=lam_min, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="cfg2,solve")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_schur_cr_shard.py needs a GPU"
    only = set(args.only.split(","))
    res = {"bench": "kkt_schur_cr_shard", "device": torch.cuda.get_device_name(0)}
    if "cfg2" in only:
        res["cfg2"] = cfg2(args.rounds)
    if "solve" in only:
        res["solve"] = solve(args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
