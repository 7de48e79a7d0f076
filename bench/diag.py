"""The matrix-free KKT diagonals (ctd_hdiag_dev_async, ctd_jsq_rows_dev_async, ctd_jsq_cols_dev_async) beside the products they
are built from and the assembly kernels they replace, on one handle per workload, in the same process:

    hdiag, jsq_rows, jsq_cols     the three new calls (2, 1 and 2 launches)
    hprod, jtprod, jprod          their lane families' products (2, 2 and 1 launches)
    hess_coord, jac_coord         the assembly a consumer needed before to read the same diagonals off H and J
    --shard: hdiag_shard, jsq_rows_shard, jsq_cols_shard on the FIRST shard of a two-shard split of the same grid (a second handle,
                                  steps [0, N / 2), its halos copied: it reads the same full x), beside the whole-grid calls and half
                                  of them.  One card: context for the launch floor and the per-node cost, no multi-GPU rate.

The calls are alternated over --rounds rounds after a warm-up; each figure is the median over the rounds of the mean over a window
of at least --window seconds (device events around the enqueues on the handle's stream); the per-round figures are kept so the
run-to-run spread of each can be read (spread_us: max - min over the rounds).  --untouched-only times the calls that exist without
the diagonals (for a run on another commit).  Prints one JSON line (and writes it to --out when given).

    python bench/diag.py [--window 0.2] [--rounds 5] [--only cfg2,cfg3] [--untouched-only] [--shard] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from products import WORKLOADS, timed  # noqa: E402


def workload(name, prob, sch, N, pattern, window, rounds, untouched_only, shard=False):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern=pattern)
    d.set_stream(stream)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    r = np.random.default_rng(3)
    v, w, y = (torch.from_numpy(r.uniform(-1, 1, n)).cuda() for n in (nvar, ncon, ncon))
    wx, wc = (torch.from_numpy(r.uniform(0, 2, n)).cuda() for n in (nvar, ncon))
    new = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")      # noqa: E731
    ov, oc, ov2, c, jvals, hvals = new(nvar), new(ncon), new(nvar), new(ncon), new(d.nnzj), new(d.nnzh)
    fns = {}
    if not untouched_only:
        fns.update(hdiag_us=lambda: d.hdiag(x, y, obj_weight=0.7, out=ov, sync=False),
                   jsq_rows_us=lambda: d.jsq_rows(x, wx, out=oc, sync=False),
                   jsq_cols_us=lambda: d.jsq_cols(x, wc, out=ov2, sync=False))
    if shard and not untouched_only:
        ds = ct.DOCP(prob, N, sch, device=0, pattern=pattern, steps=(0, N // 2))
        ds.set_stream(stream)
        sv, sc_, sv2 = new(nvar), new(ncon), new(nvar)
        fns.update(hdiag_shard_us=lambda: ds.hdiag_shard(x, y, 0.7, out=sv),
                   jsq_rows_shard_us=lambda: ds.jsq_rows_shard(x, wx, out=sc_),
                   jsq_cols_shard_us=lambda: ds.jsq_cols_shard(x, wc, out=sv2))
    fns.update(hprod_us=lambda: d.hprod(x, y, v, obj_weight=0.7, out=ov, sync=False),
               jtprod_us=lambda: d.jtprod(x, w, out=ov2, sync=False),
               jprod_us=lambda: d.jprod(x, v, out=oc, sync=False),
               hess_coord_us=lambda: d.hess_coord(x, y, 0.7, hvals, sync=False),
               jac_coord_us=lambda: d.cons_jac(x, c, jvals, sync=False))
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(1e3 * timed(fn, stream, window))
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    out["rounds_us"] = {k: [round(t, 2) for t in ts] for k, ts in res.items()}
    out["spread_us"] = {k: round(max(ts) - min(ts), 2) for k, ts in res.items()}
    out.update(name=name, problem=prob, scheme=sch, N=N, pattern=pattern, nvar=nvar, ncon=ncon, nnzj=d.nnzj, nnzh=d.nnzh)
    if not untouched_only:
        out.update(hdiag_over_hprod=round(out["hdiag_us"] / out["hprod_us"], 3),
                   jsq_cols_over_jtprod=round(out["jsq_cols_us"] / out["jtprod_us"], 3),
                   jsq_rows_over_jprod=round(out["jsq_rows_us"] / out["jprod_us"], 3),
                   diagonals_over_assembly=round((out["hdiag_us"] + out["jsq_rows_us"] + out["jsq_cols_us"]) /
                                                 (out["hess_coord_us"] + out["jac_coord_us"]), 3))
        if shard:
            for k in ("hdiag", "jsq_rows", "jsq_cols"):
                out[f"{k}_shard_over_half"] = round(out[f"{k}_shard_us"] / (0.5 * out[f"{k}_us"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--untouched-only", action="store_true")
    ap.add_argument("--shard", action="store_true", help="also time the shard calls on the first of two shards")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/diag.py needs a GPU"
    only = set(args.only.split(",")) if args.only else None
    results = [workload(*wl, args.window, args.rounds, args.untouched_only, args.shard) for wl in WORKLOADS if only is None or wl[0] in only]
    line = json.dumps({"bench": "diag", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
