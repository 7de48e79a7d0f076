"""Matrix-free Jacobian products (ctd_jprod_dev_async / ctd_jtprod_dev_async) against the assembled Jacobian, on one handle per
workload, in the same process:

    jprod, jtprod                  one call each (device events around the enqueue on the handle's stream)
    cons_jac                       the constraint / Jacobian kernel's own duration (per-dispatch events, ctd_time_cons_jac_dev)
    assemble + multiply            cons_jac on a CSR handle of the same transcription + a torch sparse CSR matvec (J v)

The four are alternated over --rounds rounds after a warm-up; each figure is the median over the rounds of the mean over a
window of at least --window seconds.  bytes: what a product must move (x, the direction, the result); roofline: those bytes
over the time, as a share of 8 TB/s.  Prints one JSON line (and writes it to --out when given).

    python bench/products.py [--window 0.2] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402

WORKLOADS = [  # (name, problem, scheme, N, pattern)
    ("cfg2", "goddard", "gauss_legendre_2", 10_000, "manual"),
    ("cfg3", "double_integrator_path", "midpoint", 100_000, "manual"),
    ("cfg5_manual", "quadrotor12", "gauss_legendre_3", 20_000, "manual"),
    ("cfg5_optimized", "quadrotor12", "gauss_legendre_3", 20_000, "optimized"),
]
ROOFLINE = 8e12


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


def workload(name, prob, sch, N, pattern, window, rounds):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern=pattern)
    d.set_stream(stream)
    nvar, ncon, nnzj = d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzj
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    r = np.random.default_rng(3)
    v = torch.from_numpy(r.uniform(-1, 1, nvar)).cuda()
    w = torch.from_numpy(r.uniform(-1, 1, ncon)).cuda()
    jv = torch.empty(ncon, dtype=torch.float64, device="cuda")
    jtw = torch.empty(nvar, dtype=torch.float64, device="cuda")
    c = torch.empty(ncon, dtype=torch.float64, device="cuda")
    vals = torch.empty(nnzj, dtype=torch.float64, device="cuda")
    # assemble-then-multiply: the CSR handle of the same transcription and a torch sparse CSR matrix over its value array
    e = ct.DOCP(prob, N, sch, device=0, pattern=pattern, value_order="csr")
    e.set_stream(stream)
    rows, cols = e.jac_structure()
    assert np.all(np.diff(rows) >= 0), "CSR handle: rows not sorted"
    crow = torch.from_numpy(np.searchsorted(rows - 1, np.arange(ncon + 1)).astype(np.int64)).cuda()
    col = torch.from_numpy((cols - 1).astype(np.int64)).cuda()
    evals = torch.empty(nnzj, dtype=torch.float64, device="cuda")
    ec = torch.empty(ncon, dtype=torch.float64, device="cuda")
    A = torch.sparse_csr_tensor(crow, col, evals, size=(ncon, nvar))
    del rows, cols

    def assemble_mul():
        e.cons_jac(x, ec, evals, sync=False)
        return torch.mv(A, v)

    fns = {
        "jprod_us": lambda: d.jprod(x, v, out=jv, sync=False),
        "jtprod_us": lambda: d.jtprod(x, w, out=jtw, sync=False),
        "assemble_multiply_us": assemble_mul,
    }
    res = {k: [] for k in list(fns) + ["cons_jac_kernel_us"]}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(1e3 * timed(fn, stream, window))
        res["cons_jac_kernel_us"].append(1e3 * d.time_cons_jac(x, c, vals, iters=50))
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    # the assembled product agrees with jprod (same transcription; manual patterns may drop entries: reported, not asserted)
    d.jprod(x, v, out=jv)
    ref = assemble_mul()
    torch.cuda.synchronize()
    out["assembled_vs_jprod_relerr"] = float(torch.linalg.norm(ref - jv) / torch.linalg.norm(jv))
    bj, bt = 8 * (2 * nvar + ncon), 8 * (nvar + 2 * ncon)
    out.update(name=name, problem=prob, scheme=sch, N=N, pattern=pattern, nvar=nvar, ncon=ncon, nnzj=nnzj,
               jprod_bytes=bj, jtprod_bytes=bt, cons_jac_store_bytes=8 * (ncon + nnzj),
               jprod_roofline=round(bj / (out["jprod_us"] * 1e-6) / ROOFLINE, 4),
               jtprod_roofline=round(bt / (out["jtprod_us"] * 1e-6) / ROOFLINE, 4),
               jprod_faster_than_cons_jac=out["jprod_us"] < out["cons_jac_kernel_us"],
               jtprod_faster_than_cons_jac=out["jtprod_us"] < out["cons_jac_kernel_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/products.py needs a GPU"
    only = set(args.only.split(",")) if args.only else None
    results = [workload(*wl, args.window, args.rounds) for wl in WORKLOADS if only is None or wl[0] in only]
    line = json.dumps({"bench": "products", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
