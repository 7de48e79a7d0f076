"""Matrix-free Hessian-of-the-Lagrangian products (ctd_hprod_dev_async) against the assembled Hessian, on one handle per workload,
in the same process:

    hprod                          one call (device events around the enqueue on the handle's stream)
    hprod_objective                the objective-only form (y = NULL)
    hess_kernel                    the Hessian kernel's own duration (per-dispatch events, ctd_time_hess_dev)
    assemble + multiply            hess_coord into the lower triangle, a gather into the full symmetric CSR value array and a
                                   torch sparse CSR matvec (H v)

The four are alternated over --rounds rounds after a warm-up; each figure is the median over the rounds of the mean over a
window of at least --window seconds.  bytes: what a product must move (x, y, v, the result); roofline: those bytes over the time,
as a share of 8 TB/s.  Prints one JSON line (and writes it to --out when given).

    python bench/hprod.py [--window 0.2] [--rounds 3] [--only cfg2,cfg5_manual] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "bench"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from products import ROOFLINE, timed  # noqa: E402

WORKLOADS = [  # (name, problem, scheme, N, pattern)
    ("cfg2", "goddard", "gauss_legendre_2", 10_000, "manual"),
    ("cfg3", "double_integrator_path", "midpoint", 100_000, "manual"),
    ("cfg5_manual", "quadrotor12", "gauss_legendre_3", 20_000, "manual"),
    ("cfg5_optimized", "quadrotor12", "gauss_legendre_3", 20_000, "optimized"),
]


def symmetric_csr(hr, hc, nvar):
    """full symmetric CSR (crow, col) of the lower triangle (1-based hr >= hc) and the gather index of its values"""
    r, c = hr - 1, hc - 1
    off = r != c
    rows = np.concatenate([r, c[off]])
    cols = np.concatenate([c, r[off]])
    src = np.concatenate([np.arange(len(r)), np.nonzero(off)[0]])
    order = np.lexsort((cols, rows))
    crow = np.searchsorted(rows[order], np.arange(nvar + 1)).astype(np.int64)
    return crow, cols[order].astype(np.int64), src[order].astype(np.int64)


def workload(name, prob, sch, N, pattern, window, rounds):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern=pattern)
    d.set_stream(stream)
    nvar, ncon, nnzh = d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzh
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    r = np.random.default_rng(3)
    v = torch.from_numpy(r.uniform(-1, 1, nvar)).cuda()
    y = torch.from_numpy(r.uniform(-1, 1, ncon)).cuda()
    hv = torch.empty(nvar, dtype=torch.float64, device="cuda")
    ho = torch.empty(nvar, dtype=torch.float64, device="cuda")
    hvals = torch.empty(nnzh, dtype=torch.float64, device="cuda")
    crow, col, src = symmetric_csr(*d.hess_structure(), nvar)
    crow, col, src = (torch.from_numpy(a).cuda() for a in (crow, col, src))
    full = torch.empty(len(src), dtype=torch.float64, device="cuda")
    A = torch.sparse_csr_tensor(crow, col, full, size=(nvar, nvar))

    def assemble_mul():
        d.hess_coord(x, y, 0.7, hvals, sync=False)
        torch.index_select(hvals, 0, src, out=full)
        return torch.mv(A, v)

    fns = {
        "hprod_us": lambda: d.hprod(x, y, v, obj_weight=0.7, out=hv, sync=False),
        "hprod_objective_us": lambda: d.hprod(x, None, v, obj_weight=0.7, out=ho, sync=False),
        "assemble_multiply_us": assemble_mul,
    }
    res = {k: [] for k in list(fns) + ["hess_kernel_us"]}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(1e3 * timed(fn, stream, window))
        res["hess_kernel_us"].append(1e3 * d.time_hess(x, y, hvals, 0.7, iters=50))
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    # the assembled product against hprod (manual patterns of the Euler schemes may drop entries: reported, not asserted)
    d.hprod(x, y, v, obj_weight=0.7, out=hv)
    ref = assemble_mul()
    torch.cuda.synchronize()
    out["assembled_vs_hprod_relerr"] = float(torch.linalg.norm(ref - hv) / torch.linalg.norm(hv))
    b = 8 * (3 * nvar + ncon)
    out.update(name=name, problem=prob, scheme=sch, N=N, pattern=pattern, nvar=nvar, ncon=ncon, nnzh=nnzh,
               hprod_bytes=b, hessian_output_bytes=8 * nnzh, hprod_roofline=round(b / (out["hprod_us"] * 1e-6) / ROOFLINE, 4),
               hprod_faster_than_hess_kernel=out["hprod_us"] < out["hess_kernel_us"],
               hprod_faster_than_assemble_multiply=out["hprod_us"] < out["assemble_multiply_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/hprod.py needs a GPU"
    only = set(args.only.split(",")) if args.only else None
    results = [workload(*wl, args.window, args.rounds) for wl in WORKLOADS if only is None or wl[0] in only]
    line = json.dumps({"bench": "hprod", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
