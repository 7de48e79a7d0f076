"""Per-iteration time of the shard form of the device-resident MINRES solve (ctd_kkt_minres_shard_*, dist.minres_shards) beside the
whole-grid solve, on cfg 2 (Goddard, Gauss-Legendre 2, N = 10 000), in one process on one GPU:

    whole        DOCP.kkt_minres_start + kkt_minres_iters(64): the whole-grid solve (bench/kkt_minres.py's "device")
    shard1       the whole-grid handle as the single shard of a one-rank split, through MinresPhases: the same kernels' shard
                 variants, one Python call per phase, no gather
    shard3       three shard handles (the balanced split), the gathers as device copies of the slots, the halo of the Lanczos
                 vector copied from the owners: on ONE GPU the three shards serialise, so this shows the overhead of the phase
                 split and of the copies, NOT scaling

64 iterations with rtol = 0 after a start, device events on torch's current stream around the 64 iterations; the three are
alternated over --rounds rounds after a warm-up, each figure the median over the rounds.  Prints one JSON line (and writes it to
--out when given).

    python bench/kkt_minres_shard.py [--rounds 5] [--out FILE]
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
from ctdirect_jl_amd import dist  # noqa: E402
from helpers import bench_inputs, describe  # noqa: E402

ITERS = 64
PROB, SCH, N, PATTERN = "goddard", "gauss_legendre_2", 10_000, "manual"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench/kkt_minres_shard.py needs a GPU"
    stream = torch.cuda.current_stream(0)
    full = ct.DOCP(PROB, N, SCH, device=0, pattern=PATTERN)
    full.set_stream(stream)
    hs = [ct.DOCP(PROB, N, SCH, device=0, pattern=PATTERN, steps=dist.shard_steps(N, 3, k)) for k in range(3)]
    nvar, ncon = full.dim_NLP_variables, full.dim_NLP_constraints
    n = nvar + ncon
    r = np.random.default_rng(21)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    x = up(bench_inputs(describe(full, PROB, SCH), perturb=1e-3))
    y, sx, sc, rhs = up(0.1 * r.uniform(-1, 1, ncon)), up(10.0 ** r.uniform(-3, 5, nvar)), up(1e-2 * r.uniform(1, 2, ncon)), up(r.uniform(-1, 1, n))
    pre = full.kkt_diag_precond(x, y, sx=sx, sc=sc)
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    ph1 = dist.minres_shards([full], [x], y, rhs, sx=sx, sc=sc, precond=pre)
    ph3 = dist.minres_shards(hs, [x] * 3, y, rhs, sx=sx, sc=sc, precond=pre)

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / ITERS

    def whole():
        full.kkt_minres_start(x, y, rhs, z, sx=sx, sc=sc, precond=pre, rtol=0.0)
        return event_us(lambda: full.kkt_minres_iters(x, y, z, ITERS, sx=sx, sc=sc))

    def phases(ph):
        ph.start(0.0, 10 * ITERS)
        return event_us(lambda: ph.iterate(ITERS))

    fns = {"whole_us": whole, "shard1_us": lambda: phases(ph1), "shard3_us": lambda: phases(ph3)}
    for fn in fns.values():
        fn()                                    # warm-up: workspaces, partial sums, torch's allocator
    res = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            res[k].append(fn())
    out = {k: round(statistics.median(t), 2) for k, t in res.items()}
    out["rounds_us"] = {k: [round(t, 2) for t in ts] for k, ts in res.items()}
    # the three computed the same iterate: one shard the bits of the whole-grid solve, three shards its value
    info = full.kkt_minres_info()
    z1, z3 = ph1.ranks[0].z, torch.empty_like(z)
    for rk in ph3.ranks:
        lay = rk.w.layout
        for lo, hi in ((lay.var_begin, lay.var_end), (lay.tail_begin, lay.tail_end), (lay.row_begin, lay.row_end)):
            z3[lo:hi] = rk.z[lo:hi]
    out.update(problem=PROB, scheme=SCH, N=N, pattern=PATTERN, nvar=nvar, ncon=ncon, iterations=ITERS, iterations_done=info.iterations,
               shard1_equals_whole=bool(torch.equal(z1, z)), shard3_vs_whole_relerr=float(torch.linalg.norm(z3 - z) / torch.linalg.norm(z)),
               shard1_over_whole=round(out["shard1_us"] / out["whole_us"], 3), shard3_over_whole=round(out["shard3_us"] / out["whole_us"], 3))
    line = json.dumps({"bench": "kkt_minres_shard", "device": torch.cuda.get_device_name(0), "result": out})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
