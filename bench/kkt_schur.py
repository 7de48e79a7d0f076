"""The chunked block-tridiagonal Schur preconditioner of the KKT MINRES solve (DOCP.kkt_schur_precond, kkt_minres(precond=P)): what a
chunk length costs per call and per iteration, and what it buys in iterations and wall time.

  chunks   workload cfg2 (Goddard, Gauss-Legendre 2, N = 10 000) on a CSR handle, chunk_steps in {N, 1024, 256, 64, 16}: microseconds
           per call of the factor (two launches) and of the solve (one launch), and per MINRES iteration (64 iterations, rtol = 0,
           device events around kkt_minres_iters); `diag`: the iteration with the diagonal preconditioner on the same handle.  The
           chunk lengths and `diag` are alternated over --rounds rounds after a warm-up; median, and min / max as the spread.
  solve    Goddard trapeze N = 2000, sx = 10^U(-3, 5) shifted by max(0, -lambda_min(H)) so that H + Sx is positive definite,
           sc = 1e-8 U(1, 2), seed 21 (the system of tests/test_gpu_kkt_minres.py::minres_case with the small sc of an equality-
           constrained NLP): iterations and wall time to rtol = 1e-10 for precond="diag" -- capped at 20 n iterations and
           reported as capped when it gets there -- and for every chunk length (the factor's time is reported beside the solve's).

Prints one JSON line (and writes it to --out when given).

    python bench/kkt_schur.py [--rounds 5] [--only chunks,solve] [--out FILE]
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
from products import timed  # noqa: E402

ITERS = 64
CHUNKS = (None, 1024, 256, 64, 16)          # None: one chunk (N)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spread(ts):
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}


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
    lay = d.kkt_schur_layout()
    P = {L: d.kkt_schur_factor(jvals, px, pc, sc, N if L is None else L, torch.empty(lay.workspace, dtype=torch.float64, device="cuda"))
         for L in CHUNKS}
    torch.cuda.synchronize()
    assert all(d.kkt_schur_info(p) == -1 for p in P.values())

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

    fns = {("diag", "iteration_us"): lambda: iteration((px, pc))}
    for L, p in P.items():
        key = "N" if L is None else str(L)
        fns[(key, "factor_us")] = lambda L=L, p=p: 1e3 * timed(lambda: d.kkt_schur_factor(jvals, px, pc, sc, N if L is None else L, p.ws), stream, 0.02)
        fns[(key, "solve_us")] = lambda p=p: 1e3 * timed(lambda: d.kkt_schur_solve(p, rhs[nvar:], out=out, sync=False), stream, 0.02)
        fns[(key, "iteration_us")] = lambda p=p: iteration(p)
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
        table["N" if L is None else str(L)]["n_chunks"] = int(p.layout.n_chunks)
    return dict(problem=prob, scheme=sch, N=N, nvar=nvar, ncon=ncon, block_rows=int(lay.block_rows), iterations=ITERS, rounds=rounds,
                chunk_steps=table)


def whole_solve():
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
    rows = {}

    def run(key, precond):
        d.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond=precond, rtol=1e-10, max_iter=4)       # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z, info = d.kkt_minres(x, y, rhs, sx=sx, sc=sc, precond=precond, rtol=1e-10, max_iter=cap, check_every=64)
        torch.cuda.synchronize()
        rows[key] = dict(status=info.status, iterations=info.iterations, capped=info.status == "max_iter",
                         solve_ms=round(1e3 * (time.perf_counter() - t0), 2))

    px, pc = d.kkt_diag_precond(x, y, sx=sx, sc=sc)
    run("diag", (px, pc))
    jvals = d.cons_jac(x)[1]
    for L in CHUNKS:
        key = "N" if L is None else str(L)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = d.kkt_schur_precond(x, y, sx=sx, sc=sc, chunk_steps=L, jvals=jvals)
        torch.cuda.synchronize()
        build_ms = round(1e3 * (time.perf_counter() - t0), 2)
        run(key, P)
        rows[key].update(build_ms=build_ms, n_chunks=int(P.layout.n_chunks), first_bad_block=d.kkt_schur_info(P))
    return dict(problem=prob, scheme=sch, N=N, n=n, scv=1e-8, rtol=1e-10, cap=cap, lambda_min_H=lam_min, precond=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="chunks,solve")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_schur.py needs a GPU"
    only = set(args.only.split(","))
    res = {"bench": "kkt_schur", "device": torch.cuda.get_device_name(0)}
    if "chunks" in only:
        res["chunks"] = chunk_table(args.rounds)
    if "solve" in only:
        res["solve"] = whole_solve()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
