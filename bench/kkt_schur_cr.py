"""The log-depth exact block-tridiagonal Schur preconditioner (DOCP.kkt_schur_cr_precond, kkt_minres(precond=P)) beside the chunked
one (bench/kkt_schur.py, whose workloads and timers these are) and the diagonal, measured in one session.

  chunks   workload cfg2 (Goddard, Gauss-Legendre 2, N = 10 000, m = 9) on a CSR handle: microseconds per call of the factor and of
           the solve, and per MINRES iteration (64 iterations, rtol = 0, device events around kkt_minres_iters) for `cr` (this
           preconditioner), the chunked one with chunk_steps in {N, 1024, 256, 64, 16} and `diag`.  All rows are alternated over
           --rounds rounds after a warm-up; median, and min / max as the spread.  `cr` also reports its launch counts and the
           microseconds per launch they amount to (the solve is a chain of dependent launches).
  solve    Goddard trapeze N = 2000, sc = 1e-8 U(1, 2) (the system of bench/kkt_schur.py), rtol = 1e-10: iterations, and build
           (diagonals + factor) and solve wall time for `cr` and every chunk length, alternated over --rounds rounds; `diag` once
           (capped at 20 n iterations).  `claim`: whether cr's iteration count is within +-2 of one chunk's, and whether the
           median of its build + solve lies below the best chunk length's by more than the larger of the two spreads (max - min).

Prints one JSON line (and writes it to --out when given).

    python bench/kkt_schur_cr.py [--rounds 5] [--only chunks,solve] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from kkt_schur import CHUNKS, ITERS, spread, up  # noqa: E402
from products import timed  # noqa: E402


def name(L):
    return "N" if L is None else str(L)


def chunk_table(rounds):
    prob, sch, N = "goddard", "gauss_legendre_2", 10_000
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    d.set_stream(stream)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    n = nvar + ncon
    r = np.random.default_rng(21)
    x = up(bench_inputs(describe(d, prob, sch), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, n))
    px, pc = d.kkt_diag_precond(x, y, sx=sx, sc=sc)
    jvals = d.cons_jac(x)[1]
    z, out = torch.empty(n, dtype=torch.float64, device="cuda"), torch.zeros(ncon, dtype=torch.float64, device="cuda")
    empty = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")      # noqa: E731
    lay, lay_cr = d.kkt_schur_layout(), d.kkt_schur_cr_layout()
    P = {L: d.kkt_schur_factor(jvals, px, pc, sc, N if L is None else L, empty(lay.workspace)) for L in CHUNKS}
    Pcr = d.kkt_schur_cr_factor(jvals, px, pc, sc, empty(lay_cr.workspace))
    torch.cuda.synchronize()
    assert all(d.kkt_schur_info(p) == -1 for p in P.values()) and d.kkt_schur_cr_info(Pcr) == -1
    # the two exact solves agree (they factor the same matrix in different orders)
    a, b = d.kkt_schur_solve(P[None], rhs[nvar:].contiguous()), d.kkt_schur_cr_solve(Pcr, rhs[nvar:].contiguous())
    agree = float((a - b).norm() / a.norm())

    def event_us(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / per

    def iteration(precond):
        d.kkt_minres_start(x, y, rhs, z, sx=sx, sc=sc, precond=precond, rtol=0.0)
        torch.cuda.synchronize()
        return event_us(lambda: d.kkt_minres_iters(x, y, z, ITERS, sx=sx, sc=sc), ITERS)

    rc = rhs[nvar:].contiguous()
    fns = {("diag", "iteration_us"): lambda: iteration((px, pc)),
           ("cr", "factor_us"): lambda: 1e3 * timed(lambda: d.kkt_schur_cr_factor(jvals, px, pc, sc, Pcr.ws), stream, 0.02),
           ("cr", "solve_us"): lambda: 1e3 * timed(lambda: d.kkt_schur_cr_solve(Pcr, rc, out=out, sync=False), stream, 0.02),
           ("cr", "iteration_us"): lambda: iteration(Pcr)}
    for L, p in P.items():
        fns[(name(L), "factor_us")] = lambda L=L, p=p: 1e3 * timed(lambda: d.kkt_schur_factor(jvals, px, pc, sc, N if L is None else L, p.ws), stream, 0.02)
        fns[(name(L), "solve_us")] = lambda p=p: 1e3 * timed(lambda: d.kkt_schur_solve(p, rc, out=out, sync=False), stream, 0.02)
        fns[(name(L), "iteration_us")] = lambda p=p: iteration(p)
    for fn in fns.values():
        fn()                                    # warm-up
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(fn())
    table = {}
    for (key, what), ts in res.items():
        table.setdefault(key, {})[what] = spread(ts)
    for L, p in P.items():
        table[name(L)]["n_chunks"] = int(p.layout.n_chunks)
    cr = table["cr"]
    cr.update(n_levels=int(lay_cr.n_levels), factor_launches=int(lay_cr.factor_launches), solve_launches=int(lay_cr.solve_launches),
              factor_us_per_launch=round(cr["factor_us"]["median"] / lay_cr.factor_launches, 2),
              solve_us_per_launch=round(cr["solve_us"]["median"] / lay_cr.solve_launches, 2),
              workspace_doubles=int(lay_cr.workspace), difference_from_one_chunk=agree)
    return dict(problem=prob, scheme=sch, N=N, nvar=nvar, ncon=ncon, block_rows=int(lay.block_rows), iterations=ITERS, rounds=rounds,
                precond=table)


def whole_solve(rounds):
    from scipy.sparse.linalg import eigsh
    from test_gpu_kkt_minres import minres_case
    prob, sch, N = "goddard", "trapeze", 2000
    c = minres_case(prob, sch, N)
    lam_min = float(eigsh(c["H"], k=1, which="SA", return_eigenvectors=False, tol=1e-8)[0])
    sx_h, sc_h = c["sx"] + max(0.0, -lam_min) * (1.0 + 1e-6), c["sc"] * 1e-6          # (minres_case's sc is 1e-2 U(1, 2))
    d = ct.DOCP(prob, N, sch, device=0, pattern="structural", value_order="csr")
    n = c["nvar"] + c["ncon"]
    x, y, sx, sc, rhs = up(c["x"]), up(c["y"]), up(sx_h), up(sc_h), up(c["rhs"])
    cap = 20 * n
    jvals = d.cons_jac(x)[1]

    def solve(precond):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, info = d.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond=precond, rtol=1e-10, max_iter=cap, check_every=64)
        torch.cuda.synchronize()
        return info, 1e3 * (time.perf_counter() - t0)

    def build(key):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = d.kkt_schur_cr_precond(x, y, sx=sx, sc=sc, jvals=jvals) if key == "cr" else \
            d.kkt_schur_precond(x, y, sx=sx, sc=sc, chunk_steps=None if key == "N" else int(key), jvals=jvals)
        torch.cuda.synchronize()
        return P, 1e3 * (time.perf_counter() - t0)

    px, pc = d.kkt_diag_precond(x, y, sx=sx, sc=sc)
    d.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond=(px, pc), rtol=1e-10, max_iter=4)       # warm-up
    info, ms = solve((px, pc))
    rows = {"diag": dict(status=info.status, iterations=info.iterations, capped=info.status == "max_iter", solve_ms=round(ms, 2))}
    keys = ["cr"] + [name(L) for L in CHUNKS]
    ts = {k: {"build_ms": [], "solve_ms": [], "total_ms": []} for k in keys}
    for rnd in range(rounds + 1):               # (round 0: the warm-up)
        for k in keys:
            P, b = build(k)
            info, s = solve(P)
            if rnd == 0:
                bad = d.kkt_schur_cr_info(P) if k == "cr" else d.kkt_schur_info(P)
                rows[k] = dict(status=info.status, iterations=info.iterations, capped=info.status == "max_iter", first_bad_block=bad)
                continue
            assert info.iterations == rows[k]["iterations"]
            for what, v in (("build_ms", b), ("solve_ms", s), ("total_ms", b + s)):
                ts[k][what].append(v)
    for k in keys:
        rows[k].update({what: spread(v) for what, v in ts[k].items()})
    best = min((k for k in keys if k != "cr"), key=lambda k: rows[k]["total_ms"]["median"])
    width = lambda k: rows[k]["total_ms"]["max"] - rows[k]["total_ms"]["min"]      # noqa: E731
    claim = dict(iterations_cr=rows["cr"]["iterations"], iterations_one_chunk=rows["N"]["iterations"],
                 iterations_match=abs(rows["cr"]["iterations"] - rows["N"]["iterations"]) <= 2, best_chunk_steps=best,
                 total_ms_cr=rows["cr"]["total_ms"]["median"], total_ms_best_chunk=rows[best]["total_ms"]["median"],
                 spread_ms=round(max(width("cr"), width(best)), 2))
    claim["faster_by_more_than_the_spread"] = claim["total_ms_best_chunk"] - claim["total_ms_cr"] > claim["spread_ms"]
    return dict(problem=prob, scheme=sch, N=N, n=n, scv=1e-8, rtol=1e-10, cap=cap, rounds=rounds, lambda_min_H=lam_min, precond=rows, claim=claim)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="chunks,solve")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_schur_cr.py needs a GPU"
    only = set(args.only.split(","))
    res = {"bench": "kkt_schur_cr", "device": torch.cuda.get_device_name(0)}
    if "chunks" in only:
        res["chunks"] = chunk_table(args.rounds)
    if "solve" in only:
        res["solve"] = whole_solve(args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
