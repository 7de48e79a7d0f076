"""Writes tests/golden/launch_plans.json: the launch plan of the constraint / Jacobian kernel on host-only handles, one case per line.

    python tests/golden/gen_launch_plans.py            # rewrites the file from the library that is built in this tree

Only `ct.DOCP(..., device=-1).launch_info()` and the CTD_* environment are used, so the script runs unchanged on any commit: the
committed file was written by the commit BEFORE the launch planner (plan_cons_jac, ctd_host.cpp) existed, and
tests/test_launch_plan_cpu.py asserts that the planner reproduces every line.  A host-only handle runs all of the plan except
the two rules that ask the device for its resident workgroups (those have tests of their own there).

The matrix is thinned to keep the file small, every rule of the plan still occurring in it: the ten registry problems x the
nine schemes on N = 1000 and 100 000 (the 480-workgroup rule, the one-round rule, the 320-lane rule, the tiles of the wide
OCPs), N = 7 on three schemes (one tile); on three problems (narrow, with path constraints, wide) x four schemes also N = 1, 2
(all steps in the edge blocks), 100 and 10 000, the optimized pattern and the CSR order, and the two half-grid shards; two and
three controls per step on midpoint; and the overrides of tile, block and kernel form.
"""
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PROBLEMS = ("goddard", "goddard_all", "double_integrator_path", "quadrotor", "quadrotor12", "stagewise_scalar",
            "estimate_initial_condition", "estimate_rotation_rate", "least_squares_with_constraint", "double_integrator_freet0tf")
SCHEMES = ("trapeze", "midpoint", "gauss_legendre_1", "gauss_legendre_2_constant_control", "gauss_legendre_3_constant_control",
           "gauss_legendre_2", "gauss_legendre_3", "euler", "euler_implicit")
NS = (1000, 100_000)
NS_SMALL = (1, 2, 100, 10_000)
SCHEMES_TINY = ("trapeze", "midpoint", "gauss_legendre_3")
PROBLEMS_THIN = ("goddard", "double_integrator_path", "quadrotor12")
SCHEMES_THIN = ("trapeze", "midpoint", "gauss_legendre_2", "gauss_legendre_3")
OVERRIDES = [{"CTD_TILE": str(t)} for t in (1, 7, 1000)] + [{"CTD_BLOCK": str(b)} for b in (64, 100, 128, 512)] + \
            [{"CTD_LEAN": "0"}, {"CTD_STATIC_EMIT": "0"}]
KNOBS = ("CTD_TILE", "CTD_BLOCK", "CTD_LEAN", "CTD_STATIC_EMIT", "CTD_LONG_GRID", "CTD_LONG_GRID_ROUNDS", "CTD_WT_STORE", "CTD_EARLY",
         "CTD_MULTI_TILE", "CTD_DEBUG_STOP", "CTD_EDGE_BLOCKS")
FIELDS = ("grid", "block", "lds_bytes", "steps_per_tile", "csc_period", "edge_entries", "direct_tiles")
OUT = os.path.join(HERE, "launch_plans.json")


def cases():
    """[problem, scheme, N, pattern, value order, control steps, shard or None, environment] of every case, in file order"""
    out = []
    for prob in PROBLEMS:
        for sch in SCHEMES:
            out.extend([prob, sch, N, "manual", "csc", 1, None, {}] for N in NS + ((7,) if sch in SCHEMES_TINY else ()))
    for prob in PROBLEMS_THIN:
        for sch in SCHEMES_THIN:
            out.extend([prob, sch, N, "manual", "csc", 1, None, {}] for N in NS_SMALL)
            for pattern, order in (("optimized", "csc"), ("manual", "csr"), ("optimized", "csr")):
                out.extend([prob, sch, N, pattern, order, 1, None, {}] for N in ((1000, 100_000) if prob == "goddard" else (100_000,)))
            for N in ((100, 100_000) if prob == "goddard" else (100_000,)):
                out.append([prob, sch, N, "manual", "csc", 1, [0, N // 2], {}])
                out.append([prob, sch, N, "manual", "csc", 1, [N // 2, N], {}])
        out.extend([prob, "midpoint", N, "manual", "csc", cs, None, {}] for cs in (2, 3) for N in (7, 10_000, 100_000))
        for sch, N in (("gauss_legendre_3", 1000), ("midpoint", 100_000)):
            out.extend([prob, sch, N, "manual", "csc", 1, None, env] for env in OVERRIDES)
    return out


def plan(case):
    """The FIELDS of launch_info() for one case, or the message of the refusal"""
    import ctdirect_jl_amd as ct
    prob, sch, N, pattern, order, cs, steps, env = case
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            docp = ct.DOCP(prob, N, sch, pattern=pattern, device=-1, steps=steps, control_steps=cs, value_order=order)
        info = docp.launch_info()
        docp.close()
        return [info[f] for f in FIELDS]
    except ct.CTDirectError as e:
        return str(e)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    lines = [json.dumps(c + [plan(c)], separators=(",", ":")) for c in cases()]
    with open(OUT, "w") as f:
        f.write('{"fields":' + json.dumps(FIELDS) + ',"cases":[\n' + ",\n".join(lines) + "\n]}\n")
    print(f"{len(lines)} cases -> {OUT}")


if __name__ == "__main__":
    main()
