"""The fused matrix-free KKT product (ctd_kktprod_dev_async) against the composition a host writes from the separate products, on
one handle per workload, in the same process:

    fused        DOCP.kktprod: rx = H dx + J' dy + sx o dx, rc = J dx - sc o dy, two launches
    composed     hprod (2 launches) + jtprod (2) + jprod (1) and the two element-wise updates in torch with the fewest kernels torch
                 offers: rx = Hdx + Jtdy, then addcmul_(sx, dx) (2 kernels); rc = addcmul(Jdx, sc, dy, value=-1) (1 kernel) --
                 eight dispatches (seven for a host with a three-operand update kernel of its own)
    hprod        hprod alone: what the fused lanes cost before they also kept J' dy and J dx

The three are alternated over --rounds rounds after a warm-up; each figure is the median over the rounds of the mean over a
window of at least --window seconds (device events around the enqueues on the handle's stream); the per-round figures are kept
so the run-to-run spread of each can be read.  bytes: what a fused call must move with all operands present, 8 (4 nvar + 4 ncon);
roofline: those bytes over the fused time, as a share of 8 TB/s.  relerr: |fused - composed| / |composed| over both blocks.
Prints one JSON line (and writes it to --out when given).

    python bench/kktprod.py [--window 0.2] [--rounds 5] [--out FILE]
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
from products import ROOFLINE, WORKLOADS, timed  # noqa: E402


def workload(name, prob, sch, N, pattern, window, rounds):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern=pattern)
    d.set_stream(stream)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = torch.from_numpy(bench_inputs(describe(d, prob, sch), perturb=1e-3)).cuda()
    r = np.random.default_rng(3)
    dx, dy, y = (torch.from_numpy(r.uniform(-1, 1, n)).cuda() for n in (nvar, ncon, ncon))
    sx = torch.from_numpy(r.uniform(0, 1, nvar)).cuda()
    sc = torch.from_numpy(r.uniform(0, 1e-2, ncon)).cuda()
    new = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")      # noqa: E731
    rx, rc, hdx, jtdy, jdx, cx, cc = new(nvar), new(ncon), new(nvar), new(nvar), new(ncon), new(nvar), new(ncon)

    def fused():
        d.kktprod(x, y, dx, dy, obj_weight=0.7, sx=sx, sc=sc, out=(rx, rc), sync=False)

    def composed():
        d.hprod(x, y, dx, obj_weight=0.7, out=hdx, sync=False)
        d.jtprod(x, dy, out=jtdy, sync=False)
        d.jprod(x, dx, out=jdx, sync=False)
        torch.add(hdx, jtdy, out=cx)
        cx.addcmul_(sx, dx)
        torch.addcmul(jdx, sc, dy, value=-1.0, out=cc)

    fns = {"fused_us": fused, "composed_us": composed, "hprod_us": lambda: d.hprod(x, y, dx, obj_weight=0.7, out=hdx, sync=False)}
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(1e3 * timed(fn, stream, window))
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    out["rounds_us"] = {k: [round(t, 2) for t in ts] for k, ts in res.items()}
    fused()
    composed()
    torch.cuda.synchronize()
    num = torch.sqrt(torch.linalg.norm(rx - cx) ** 2 + torch.linalg.norm(rc - cc) ** 2)
    den = torch.sqrt(torch.linalg.norm(cx) ** 2 + torch.linalg.norm(cc) ** 2)
    spread = max(res["composed_us"]) - min(res["composed_us"])
    nbytes = 8 * (4 * nvar + 4 * ncon)
    out.update(name=name, problem=prob, scheme=sch, N=N, pattern=pattern, nvar=nvar, ncon=ncon,
               fused_vs_composed_relerr=float(num / den), fused_bytes=nbytes,
               fused_roofline=round(nbytes / (out["fused_us"] * 1e-6) / ROOFLINE, 4),
               composed_spread_us=round(spread, 2), composed_over_fused=round(out["composed_us"] / out["fused_us"], 3),
               fused_over_hprod=round(out["fused_us"] / out["hprod_us"], 3),
               fused_faster_by_more_than_spread=bool(max(res["fused_us"]) + spread < min(res["composed_us"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kktprod.py needs a GPU"
    only = set(args.only.split(",")) if args.only else None
    results = [workload(*wl, args.window, args.rounds) for wl in WORKLOADS if only is None or wl[0] in only]
    line = json.dumps({"bench": "kktprod", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
