"""Batched constraint / Jacobian callback on cfg 2 (Goddard, Gauss-Legendre 2 stagewise, 10 000 steps): evaluations per second of
ONE launch of K members (ctd_cons_jac_batch_dev_async) against K back-to-back single launches (ctd_cons_jac_dev_async), for
K in 1 .. 64, in the same process, alternating the two.  Each side is timed with device events on the handle's stream over a
window of at least --window seconds after a warm-up.  Effective bandwidth: K x (bytes one evaluation moves: x in, c and vals
out) per batched launch divided by the batched launch time.  single_kernel_us: the single kernel's own duration (per-dispatch
events, ctd_time_cons_jac_dev) -- the floor K single launches cannot go below even without host overhead.  Prints one JSON line (and writes it to --out when
given).

    python bench/batch.py [--window 0.2] [--ks 1,2,4,8,16,32,64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402


def timed(fn, stream, window, reps0=8):
    """mean ms per call of fn over >= window seconds of device time (events on `stream`), after one warm call"""
    fn()
    torch.cuda.synchronize()
    reps, total_ms, calls = reps0, 0.0, 0
    while total_ms < window * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        total_ms += e0.elapsed_time(e1)
        calls += reps
        reps = min(reps * 2, 4096)
    return total_ms / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--ks", default="1,2,4,8,16,32,64")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of batched / single timing per K")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prob, sch, N = "goddard", "gauss_legendre_2", 10000
    assert torch.cuda.is_available(), "bench/batch.py needs a GPU"
    d = ct.DOCP(prob, N, sch, device=0)
    stream = torch.cuda.current_stream(0)
    nvar, ncon, nnzj = d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzj
    bytes_eval = 8 * (nvar + ncon + nnzj)    # one evaluation: reads x, writes c + the Jacobian values (10 480 288 B at cfg 2)
    L = ct._lib.lib()
    base = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    x1 = torch.from_numpy(base).cuda()
    c1 = torch.empty(ncon, dtype=torch.float64, device="cuda")
    v1 = torch.empty(nnzj, dtype=torch.float64, device="cuda")
    single_kernel_us = d.time_cons_jac(x1, c1, v1, iters=2000) * 1e3
    rows = []
    for K in [int(k) for k in args.ks.split(",")]:
        X = torch.from_numpy(np.stack([base + 1e-6 * b for b in range(K)])).cuda()
        Cb = torch.empty((K, ncon), dtype=torch.float64, device="cuda")
        Vb = torch.empty((K, nnzj), dtype=torch.float64, device="cuda")
        Cs = torch.empty_like(Cb)
        Vs = torch.empty_like(Vb)
        h = d._h
        bargs = (h, K, C.c_void_p(X.data_ptr()), X.stride(0), C.c_void_p(Cb.data_ptr()), Cb.stride(0), C.c_void_p(Vb.data_ptr()),
                 Vb.stride(0))
        fb = L.ctd_cons_jac_batch_dev_async

        def batched():
            st = fb(*bargs)
            if st:
                d._ck(st)
        singles = [d.bind_cons_jac(X[b], Cs[b], Vs[b]) for b in range(K)]

        def single_k():
            for s in singles:
                s()
        tb, ts = [], []
        for _ in range(args.rounds):           # alternate in one process: both sides see the same clocks / thermal state
            tb.append(timed(batched, stream, args.window))
            ts.append(timed(single_k, stream, args.window))
        torch.cuda.synchronize()
        same = bool(torch.equal(Cb, Cs) and torch.equal(Vb, Vs))
        mb, ms = min(tb), min(ts)
        rows.append(dict(K=K, batched_launch_us=round(mb * 1e3, 3), single_x_K_us=round(ms * 1e3, 3),
                         evals_per_s_batched=round(K / (mb * 1e-3), 1), evals_per_s_single=round(K / (ms * 1e-3), 1),
                         speedup=round(ms / mb, 3), effective_TBps=round(K * bytes_eval / (mb * 1e-3) / 1e12, 3),
                         rounds_batched_us=[round(t * 1e3, 3) for t in tb], rounds_single_us=[round(t * 1e3, 3) for t in ts],
                         bit_identical=same))
        print(json.dumps(rows[-1]), file=sys.stderr)
        del X, Cb, Vb, Cs, Vs
    out = dict(workload=f"{prob} / {sch}, {N} steps: cons_jac_batch (one launch of K members) vs K single launches",
               bytes_per_eval=bytes_eval, window_s=args.window, single_kernel_us=round(single_kernel_us, 3),
               device=torch.cuda.get_device_name(0),
               time=time.strftime("%Y-%m-%dT%H:%M:%S"), rows=rows)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
