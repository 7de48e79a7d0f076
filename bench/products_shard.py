"""One shard call of the matrix-free products (ctd_*prod_shard_dev_async, the fused KKT product included) of a two-shard split next to the whole-grid call, on one
GPU: the first shard's handle (steps [0, N/2), halo entries copied: the buffers hold the whole vectors) against the handle of the
whole grid, for bench configs 2 and 5.  Context only -- one card says nothing about multi-GPU scaling: the figure to read is how
close a shard call comes to half the whole-grid time.  A library without ctd_kktprod_shard_dev_async (CTD_LIB_PATH: an A/B run
against an earlier build) gives no kktprod_shard_us.  Timing as in bench/products.py (median over --rounds of the mean over a
window of at least --window seconds).  Prints one JSON line (and writes it to --out when given).

    python bench/products_shard.py [--window 0.2] [--rounds 3] [--out FILE]
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
from products import timed  # noqa: E402

WORKLOADS = [  # (name, problem, scheme, N)
    ("cfg2", "goddard", "gauss_legendre_2", 10_000),
    ("cfg5", "quadrotor12", "gauss_legendre_3", 20_000),
]


def workload(name, prob, sch, N, window, rounds):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0)
    s = ct.DOCP(prob, N, sch, device=0, steps=(0, N // 2))
    for h in (d, s):
        h.set_stream(stream)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    r = np.random.default_rng(3)
    v = torch.from_numpy(r.uniform(-1, 1, nvar)).cuda()
    w = torch.from_numpy(r.uniform(-1, 1, ncon)).cuda()
    oc = torch.empty(ncon, dtype=torch.float64, device="cuda")
    ov = torch.empty(nvar, dtype=torch.float64, device="cuda")
    sx = torch.from_numpy(r.uniform(0, 1, nvar)).cuda()
    sc = torch.from_numpy(r.uniform(0, 1e-2, ncon)).cuda()
    dy = torch.from_numpy(r.uniform(-1, 1, ncon)).cuda()
    fns = {
        "jprod_us": lambda: d.jprod(x, v, out=oc, sync=False),
        "jprod_shard_us": lambda: s.jprod_shard(x, v, oc),
        "jtprod_us": lambda: d.jtprod(x, w, out=ov, sync=False),
        "jtprod_shard_us": lambda: s.jtprod_shard(x, w, ov),
        "hprod_us": lambda: d.hprod(x, w, v, 0.7, out=ov, sync=False),
        "hprod_shard_us": lambda: s.hprod_shard(x, w, v, 0.7, ov),
        "kktprod_us": lambda: d.kktprod(x, w, v, dy, obj_weight=0.7, sx=sx, sc=sc, out=(ov, oc), sync=False),
    }
    if hasattr(ct._lib.lib(), "ctd_kktprod_shard_dev_async"):
        fns["kktprod_shard_us"] = lambda: s.kktprod_shard(x, w, v, dy, obj_weight=0.7, sx=sx, sc=sc, out=(ov, oc))
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(1e3 * timed(fn, stream, window))
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    for op in ("jprod", "jtprod", "hprod", "kktprod"):
        out[op + "_half_us"] = round(out[op + "_us"] / 2, 2)
    out.update(name=name, problem=prob, scheme=sch, N=N, shard_steps=[0, N // 2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/products_shard.py needs a GPU"
    results = [workload(*wl, args.window, args.rounds) for wl in WORKLOADS]
    line = json.dumps({"bench": "products_shard", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
