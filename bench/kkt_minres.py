"""Per-iteration time of preconditioned MINRES on K z = r, K the matrix-free operator of DOCP.kktprod, for the three loops a user of
the matrix-free path can run, on one handle per workload, in the same process:

    device       DOCP.kkt_minres_start + kkt_minres_iters(64) with rtol = 0: per iteration the two launches of kktprod and three
                 vector kernels, no host synchronisation (ctd_kkt_minres_iters_dev_async)
    torch        the same recurrences written in torch ops on the device around DOCP.kktprod, the two inner products read back
                 with .item() (two host synchronisations per iteration; |z|, a third one, is left out: it favours this loop)
    scipy        scipy.sparse.linalg.minres(maxiter=64, rtol=0) with the operator as tests/test_gpu_diag.py gives it: the vector
                 copied host -> device, kktprod, the result copied back, the recurrences in NumPy
    kktprod      DOCP.kktprod alone: what one iteration cannot go below

The preconditioner is DOCP.kkt_diag_precond in all three.  The four are alternated over --rounds rounds after a warm-up; each figure
is the median over the rounds.  device, torch and kktprod: device events on the handle's stream around the whole run of 64
iterations (torch: the host waits inside the loop are part of what the events enclose).  scipy runs on the host: wall clock around
the call, which ends synchronised.  launch_gap_us: device minus kktprod, the cost of the three vector kernels and their launches.
Prints one JSON line (and writes it to --out when given).

    python bench/kkt_minres.py [--rounds 5] [--out FILE]
"""
import argparse
import json
import math
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
from scipy.sparse.linalg import LinearOperator, minres  # noqa: E402

import ctdirect_jl_amd as ct  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402
from products import WORKLOADS, timed  # noqa: E402

ITERS = 64
NAMES = ("cfg2", "cfg3", "cfg5_manual")


def torch_minres(d, x, y, sx, sc, rhs, minv, k, nvar, kv):
    """scipy's recurrences in torch ops; returns z"""
    eps = float(np.finfo(np.float64).eps)
    r1 = rhs.clone()
    yv = minv * r1
    beta1 = math.sqrt(torch.dot(r1, yv).item())
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w, w2, z, r2 = torch.zeros_like(rhs), torch.zeros_like(rhs), torch.zeros_like(rhs), r1
    for itn in range(1, k + 1):
        v = yv * (1.0 / beta)
        d.kktprod(x, y, v[:nvar], v[nvar:], sx=sx, sc=sc, out=(kv[:nvar], kv[nvar:]), sync=False)
        yv = torch.sub(kv, r1, alpha=beta / oldb) if itn >= 2 else kv.clone()
        alfa = torch.dot(v, yv).item()
        yv.sub_(r2, alpha=alfa / beta)
        r1, r2 = r2, yv
        yv = minv * r2
        oldb, beta = beta, math.sqrt(torch.dot(r2, yv).item())
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = max(math.hypot(gbar, beta), eps)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2 = w2, w
        w = (v - oldeps * w1 - delta * w2) * (1.0 / gamma)
        z.add_(w, alpha=phi)
    return z


def workload(name, prob, sch, N, pattern, rounds):
    stream = torch.cuda.current_stream(0)
    d = ct.DOCP(prob, N, sch, device=0, pattern=pattern)
    d.set_stream(stream)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    n = nvar + ncon
    r = np.random.default_rng(21)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    x = up(bench_inputs(describe(d, prob, sch), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, n))
    px, pc = d.kkt_diag_precond(x, y, sx=sx, sc=sc)
    minv = 1.0 / torch.cat([px, pc])
    minv_h, rhs_h = minv.cpu().numpy(), rhs.cpu().numpy()
    z, kv, zin, zout = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(4))

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def device():
        d.kkt_minres_start(x, y, rhs, z, sx=sx, sc=sc, precond=(px, pc), rtol=0.0)
        torch.cuda.synchronize()
        return 1e3 * event_ms(lambda: d.kkt_minres_iters(x, y, z, ITERS, sx=sx, sc=sc)) / ITERS

    def composed():
        return 1e3 * event_ms(lambda: torch_minres(d, x, y, sx, sc, rhs, minv, ITERS, nvar, kv)) / ITERS

    def matvec(v):
        zin.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).ravel()))
        d.kktprod(x, y, zin[:nvar], zin[nvar:], sx=sx, sc=sc, out=(zout[:nvar], zout[nvar:]))
        return zout.cpu().numpy()

    K = LinearOperator((n, n), matvec=matvec, rmatvec=matvec, dtype=np.float64)
    M = LinearOperator((n, n), matvec=lambda v: minv_h * np.asarray(v).ravel(), dtype=np.float64)

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        minres(K, rhs_h, M=M, rtol=0.0, maxiter=ITERS)
        return 1e6 * (time.perf_counter() - t0) / ITERS

    def kktprod():
        return 1e3 * timed(lambda: d.kktprod(x, y, rhs[:nvar], rhs[nvar:], sx=sx, sc=sc, out=(kv[:nvar], kv[nvar:]), sync=False), stream, 0.05)

    fns = {"device_us": device, "torch_us": composed, "scipy_us": host, "kktprod_us": kktprod}
    for fn in fns.values():
        fn()                                    # warm-up: workspace, partial sums, torch's allocator
    res = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            res[k].append(fn())
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    out["rounds_us"] = {k: [round(t, 2) for t in ts] for k, ts in res.items()}
    # the three loops compute the same iterate
    d.kkt_minres_start(x, y, rhs, z, sx=sx, sc=sc, precond=(px, pc), rtol=0.0)
    d.kkt_minres_iters(x, y, z, ITERS, sx=sx, sc=sc)
    info = d.kkt_minres_info()
    zt = torch_minres(d, x, y, sx, sc, rhs, minv, ITERS, nvar, kv)
    zs, _ = minres(K, rhs_h, M=M, rtol=0.0, maxiter=ITERS)
    rel = lambda a, b: float(torch.linalg.norm(a - b) / torch.linalg.norm(b))      # noqa: E731
    out.update(name=name, problem=prob, scheme=sch, N=N, pattern=pattern, nvar=nvar, ncon=ncon, iterations=ITERS,
               status=info.status, iterations_done=info.iterations,
               device_vs_torch_relerr=rel(z, zt), device_vs_scipy_relerr=rel(z, up(zs)),
               launch_gap_us=round(out["device_us"] - out["kktprod_us"], 2),
               device_over_kktprod=round(out["device_us"] / out["kktprod_us"], 3),
               torch_over_device=round(out["torch_us"] / out["device_us"], 3),
               scipy_over_device=round(out["scipy_us"] / out["device_us"], 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_minres.py needs a GPU"
    only = set(args.only.split(",")) if args.only else set(NAMES)
    results = [workload(*wl, args.rounds) for wl in WORKLOADS if wl[0] in only]
    line = json.dumps({"bench": "kkt_minres", "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
