"""What the device entry points write, and what they ask of a pointer's alignment (run with -m gpu).

Every other GPU test hands the engine freshly allocated, exactly sized tensors: a store past either end of an output lands in the
allocator's rounding, and every pointer is 256-byte aligned.  Here each call is made three times (check_call):

  run A   inputs as ordinary tensors, outputs exactly sized ordinary tensors prefilled with the sentinel of tests/guarded.py;
  run B   twice: every input and every output a `guarded` view -- once with every payload at an odd multiple of 8 bytes, once with
          the arguments alternating between 16-byte and odd 8-byte alignment by position, so that inputs and outputs sit at
          different alignments relative to each other.

After each run B: every guard of every buffer is intact; every input buffer is bit-unchanged; every output payload holds the bits
of run A over its WHOLE length (on a shard handle that includes the entries the shard leaves alone, which stay the sentinel, and
the partial sums in the nv tail / the V x V entries); on a handle of the whole grid no output entry still holds the sentinel.
Nothing has a tolerance: results are documented as independent of addresses.  Values against the oracle are checked elsewhere at
these shapes.

The batched forms get (K, n) arguments with the leading dimension n + 7 inside one guarded buffer: the padding between the rows
must keep the sentinel too.

Guards are max(65536, n) doubles on each side; a store further away is not seen (tests/guarded.py)."""
import numpy as np
import pytest

import ctdirect_jl_amd as ct
from guarded import SENTINEL, guarded
from helpers import bench_inputs, describe
from jit_defs import twin
from test_gpu_products_shard import SIZES as SHARD_SIZES
from test_gpu_static_emit import geometry, user_grid

pytestmark = pytest.mark.gpu

KNOBS = ("CTD_STATIC_EMIT", "CTD_LEAN", "CTD_BLOCK", "CTD_WT_STORE", "CTD_TILE", "CTD_LONG_GRID_ROUNDS", "CTD_HESS_STEP",
         "CTD_HESS_EDGE_BLOCKS", "CTD_HESS_TILE")
SIGMA = 0.7
DEV = "cuda"
PAD = 7         # leading dimension of the batched arguments: n + PAD


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return torch


def set_env(monkeypatch, env=None):
    """exactly the knobs of `env`; every other knob of this file cleared"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---- the check ---------------------------------------------------------------------------------------------------------------------
class Arg:
    """one guarded argument: a vector of n doubles, or K rows of n doubles with the leading dimension n + PAD"""
    def __init__(self, torch, shape, shift, like=None):
        self.rows = None if np.ndim(shape) == 0 else (int(shape[0]), int(shape[1]))
        if self.rows is None:
            self.g = guarded(torch, int(shape), shift, DEV, like=like)
            self.t = self.g.view
        else:
            K, n = self.rows
            self.g = guarded(torch, (K - 1) * (n + PAD) + n, shift, DEV)
            self.t = self.g.view.as_strided((K, n), (n + PAD, 1))
            if like is not None:
                self.t.copy_(torch.from_numpy(like))

    def bits(self, torch):
        """(the entries as int64 in the shape of run A's tensor, the padding between the rows as int64)"""
        b = self.g.bits()
        if self.rows is None:
            return b, b[:0]
        K, n = self.rows
        pad = torch.ones(b.numel(), dtype=torch.bool, device=b.device)
        rows = b.as_strided((K, n), (n + PAD, 1))
        pad.as_strided((K, n), (n + PAD, 1)).fill_(False)
        return rows, b[pad]


def check_call(torch, call, inputs, outputs, whole=True, what=()):
    """call(ins, outs) with dicts of tensors.  inputs: {name: host array (n,) or (K, n), or None for an optional argument left
    out}; outputs: {name: n or (K, n)}.  `whole`: a handle of the whole grid, whose outputs are written completely."""
    ins = {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for k, a in inputs.items()}
    outs = {k: torch.full(tuple(int(q) for q in np.atleast_1d(s)), SENTINEL, dtype=torch.int64, device=DEV).view(torch.float64) for k, s in outputs.items()}
    call(ins, outs)
    torch.cuda.synchronize()
    ref = {k: t.view(torch.int64) for k, t in outs.items()}
    for mode in ("odd", "alternating"):
        shift = (lambda i: 1) if mode == "odd" else (lambda i: i % 2)
        gin = {k: None if a is None else Arg(torch, a.shape if a.ndim == 2 else a.size, shift(i), like=a) for i, (k, a) in enumerate(inputs.items())}
        gout = {k: Arg(torch, s, shift(len(inputs) + j)) for j, (k, s) in enumerate(outputs.items())}
        for a in gin.values():
            if a is not None:
                a.g.snapshot()
        call({k: None if a is None else a.t for k, a in gin.items()}, {k: a.t for k, a in gout.items()})
        torch.cuda.synchronize()
        for k, a in list(gin.items()) + list(gout.items()):
            if a is not None:
                a.g.guards_intact(f"{what} {mode} shifts, argument {k}")
        for k, a in gin.items():
            if a is not None:
                a.g.unchanged(f"{what} {mode} shifts, input {k}")
        for k, a in gout.items():
            got, pad = a.bits(torch)
            if not bool((pad == SENTINEL).all()):
                raise AssertionError(f"{what} {mode} shifts, output {k}: the padding between the rows was written")
            if not torch.equal(got, ref[k]):
                diff = torch.nonzero((got != ref[k]).reshape(-1)).flatten().cpu().tolist()
                raise AssertionError(f"{what} {mode} shifts, output {k}: {len(diff)} of {got.numel()} entries differ in bits from the run on "
                                     f"ordinary tensors, positions {diff[0]} .. {diff[-1]}")
            if whole:
                left = torch.nonzero((got == SENTINEL).reshape(-1)).flatten().cpu().tolist()
                assert not left, f"{what} {mode} shifts, output {k}: {len(left)} entries not written, positions {left[0]} .. {left[-1]}"


# ---- handles and inputs ------------------------------------------------------------------------------------------------------------
def open_handle(prob, N, sch, grid=False, rt=False, **kw):
    return ct.DOCP(twin(prob) if rt else prob, N, sch, time_grid=user_grid(N) if grid else None, device=0, **kw)


def vectors(d, prob, sch):
    """deterministic inputs of every operator: the iterate, multipliers, directions, positive diagonals"""
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    i, r = np.arange(nvar), np.arange(ncon)
    return dict(x=bench_inputs(describe(d, prob, sch), perturb=1e-3), y=np.cos(0.37 * r), v=np.sin(0.7 * i + 0.3), w=np.cos(1.1 * r + 0.2),
                sx=1.0 + 0.5 * np.cos(0.3 * i) ** 2, sc=0.1 + 0.05 * np.sin(0.9 * r) ** 2, wx=0.5 + np.sin(0.4 * i) ** 2,
                wc=0.5 + np.cos(0.6 * r) ** 2)


def pick(V, *names, none=()):
    return {k: (None if k in none else V[k]) for k in names}


# ---- cons_jac, cons, jac_coord -----------------------------------------------------------------------------------------------------
def cons_jac_forms(torch, d, x, whole, what):
    nvar, ncon, nnzj = d.dim_NLP_variables, d.dim_NLP_constraints, d.nnzj
    check_call(torch, lambda i, o: d.cons_jac(i["x"], o["c"], o["vals"]), {"x": x}, {"c": ncon, "vals": nnzj}, whole, what + ("cons_jac",))
    if whole:                   # (the NULL-output forms)
        check_call(torch, lambda i, o: d.cons(i["x"], o["c"]), {"x": x}, {"c": ncon}, whole, what + ("cons",))
        check_call(torch, lambda i, o: d.jac_coord(i["x"], o["vals"]), {"x": x}, {"vals": nnzj}, whole, what + ("jac_coord",))


# (id, problem, scheme, handle arguments, user grid)
CJ_HANDLES = [
    ("goddard-gl2", "goddard", "gauss_legendre_2", {}, False),
    ("goddard-gl2-csr", "goddard", "gauss_legendre_2", {"value_order": "csr"}, False),
    ("goddard-gl2-optimized", "goddard", "gauss_legendre_2", {"pattern": "optimized"}, False),
    ("dipath-midpoint", "double_integrator_path", "midpoint", {}, False),                   # no v column
    ("goddard-midpoint-cs2", "goddard", "midpoint", {"control_steps": 2}, False),
    ("goddard-trapeze", "goddard", "trapeze", {}, False),                                   # staged tiles
    ("goddard_all-euler_implicit", "goddard_all", "euler_implicit", {}, False),             # staged tiles
    ("quadrotor-gl3", "quadrotor", "gauss_legendre_3", {}, False),
    ("goddard-gl2-usergrid", "goddard", "gauss_legendre_2", {}, True),
]
SELECT = [("default", {}), ("no-static", {"CTD_STATIC_EMIT": "0"}), ("general", {"CTD_LEAN": "0"})]


@pytest.mark.filterwarnings("ignore:pattern='manual'")
@pytest.mark.parametrize("sel", SELECT, ids=[s[0] for s in SELECT])
@pytest.mark.parametrize("case", CJ_HANDLES, ids=[c[0] for c in CJ_HANDLES])
def test_cons_jac(torch_cuda, monkeypatch, case, sel):
    cid, prob, sch, kw, grid = case
    T = min(geometry(prob, sch, 0, **kw)[0], 48)
    sizes = (T + 1,) if prob == "quadrotor" else sorted({1, 2, T, T + 1, 2 * T + 1})
    for N in sizes:
        for wt in ((None, "0", "1") if N == 2 * T + 1 else (None,)):
            env = dict(sel[1], CTD_TILE=str(T))
            if wt is not None:
                env["CTD_WT_STORE"] = wt
            set_env(monkeypatch, env)
            d = open_handle(prob, N, sch, grid=grid, **kw)
            set_env(monkeypatch)
            assert d.launch_info()["steps_per_tile"] <= T
            x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
            cons_jac_forms(torch_cuda, d, x, True, (cid, sel[0], N, "wt", wt))
            d.close()


def test_cons_jac_long_grid_geometry(torch_cuda, monkeypatch):
    """eight waves per workgroup and the largest tile whose records fit, forced with CTD_LONG_GRID_ROUNDS=0 on the smallest grid
    whose tile the sizing rule lets grow (16 steps per tile: 7202 steps and more)"""
    prob, sch, N = "goddard", "gauss_legendre_2", 7300
    set_env(monkeypatch, {"CTD_LONG_GRID_ROUNDS": "0"})
    d = open_handle(prob, N, sch)
    set_env(monkeypatch)
    li = d.launch_info()
    assert li["block"] == 512, li
    cons_jac_forms(torch_cuda, d, bench_inputs(describe(d, prob, sch), perturb=1e-3), True, ("long grid", li["steps_per_tile"]))
    d.close()


def test_cons_jac_middle_shard(torch_cuda, monkeypatch):
    prob, sch = "goddard", "gauss_legendre_2"
    set_env(monkeypatch)
    d = open_handle(prob, 130, sch, steps=(40, 91))
    cons_jac_forms(torch_cuda, d, bench_inputs(describe(d, prob, sch), perturb=1e-3), False, ("shard 40:91 of 130",))
    d.close()


# ---- objective and gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:pattern='manual'")
@pytest.mark.parametrize("prob,sch", [("goddard", "gauss_legendre_2"), ("goddard_all", "trapeze"), ("double_integrator_path", "midpoint"),
                                      ("double_integrator_freet0tf", "gauss_legendre_2")])
def test_obj_async_and_grad(torch_cuda, monkeypatch, prob, sch):
    set_env(monkeypatch)
    for N in (1, 2, 7, 130):
        d = open_handle(prob, N, sch)
        x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
        check_call(torch_cuda, lambda i, o: d.obj_async(i["x"], o["f"]), {"x": x}, {"f": 1}, True, (prob, sch, N, "obj_async"))
        check_call(torch_cuda, lambda i, o: d.grad(i["x"], o["g"]), {"x": x}, {"g": d.dim_NLP_variables}, True, (prob, sch, N, "grad"))
        check_call(torch_cuda, lambda i, o: d.grad(i["x"], o["g"], sync=False), {"x": x}, {"g": d.dim_NLP_variables}, True,
                   (prob, sch, N, "grad async"))
        d.close()


# ---- hess_coord --------------------------------------------------------------------------------------------------------------------
def hess_call(d):
    return lambda i, o: d.hess_coord(i["x"], i["y"], SIGMA, o["hvals"])


@pytest.mark.filterwarnings("ignore:pattern='manual'")
@pytest.mark.parametrize("step", ["0", "2"])
@pytest.mark.parametrize("prob,sch", [("goddard", "gauss_legendre_2"), ("goddard_all", "trapeze")])
def test_hess_coord(torch_cuda, monkeypatch, prob, sch, step):
    for N in (1, 2, 7, 130):
        for eb in (None, "3"):
            for tile in (None, "5"):
                env = {"CTD_HESS_STEP": step}
                if eb:
                    env["CTD_HESS_EDGE_BLOCKS"] = eb
                if tile:
                    env["CTD_HESS_TILE"] = tile
                set_env(monkeypatch, env)
                d = open_handle(prob, N, sch)
                V = vectors(d, prob, sch)
                check_call(torch_cuda, hess_call(d), pick(V, "x", "y"), {"hvals": d.nnzh}, True, (prob, sch, N, env))
                d.close()
                set_env(monkeypatch)


@pytest.mark.parametrize("step", ["0", "2"])
def test_hess_coord_middle_shard(torch_cuda, monkeypatch, step):
    """the shard's partial sums in the V x V entries are part of the compared bits"""
    prob, sch = "goddard", "gauss_legendre_2"
    set_env(monkeypatch, {"CTD_HESS_STEP": step})
    d = open_handle(prob, 130, sch, steps=(40, 91))
    V = vectors(d, prob, sch)
    check_call(torch_cuda, hess_call(d), pick(V, "x", "y"), {"hvals": d.nnzh}, False, ("shard 40:91 of 130", step))
    d.close()
    set_env(monkeypatch)


# ---- the fused iteration -----------------------------------------------------------------------------------------------------------
def test_eval_all(torch_cuda, monkeypatch):
    prob, sch = "goddard", "gauss_legendre_2"
    set_env(monkeypatch)
    d = open_handle(prob, 130, sch)
    V = vectors(d, prob, sch)
    sizes = {"f": 1, "g": d.dim_NLP_variables, "c": d.dim_NLP_constraints, "vals": d.nnzj, "hvals": d.nnzh}

    def call(i, o):
        d.eval_all(i["x"], i["y"], SIGMA, o.get("f"), o.get("g"), o.get("c"), o.get("vals"), o.get("hvals"), sync=True)

    check_call(torch_cuda, call, pick(V, "x", "y"), sizes, True, ("eval_all", "five outputs"))
    check_call(torch_cuda, call, pick(V, "x", "y"), {k: sizes[k] for k in ("f", "g", "vals")}, True, ("eval_all", "c and hvals left out"))
    d.close()


# ---- the matrix-free operators -----------------------------------------------------------------------------------------------------
def operator_calls(d, V, shard):
    """(name, call, inputs, outputs) of every matrix-free operator: every optional argument given, and every one left out; kktprod
    with separate outputs and with dx | dy and rx | rc as the halves of one buffer each"""
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    f = (lambda op: getattr(d, op + "_shard")) if shard else (lambda op: getattr(d, op))
    kw = {"sync": True}
    z = np.r_[V["v"], V["w"]]
    out = []
    out.append(("jprod", lambda i, o: f("jprod")(i["x"], i["v"], o["jv"], **kw), pick(V, "x", "v"), {"jv": ncon}))
    out.append(("jtprod", lambda i, o: f("jtprod")(i["x"], i["w"], o["jtw"], **kw), pick(V, "x", "w"), {"jtw": nvar}))
    for none in ((), ("y",)):
        out.append(("hprod", lambda i, o: f("hprod")(i["x"], i["y"], i["v"], SIGMA, o["hv"], **kw), pick(V, "x", "y", "v", none=none), {"hv": nvar}))
        out.append(("hdiag", lambda i, o: f("hdiag")(i["x"], i["y"], SIGMA, o["hd"], **kw), pick(V, "x", "y", none=none), {"hd": nvar}))
    for none in ((), ("wx",)):
        out.append(("jsq_rows", lambda i, o: f("jsq_rows")(i["x"], i["wx"], o["jr"], **kw), pick(V, "x", "wx", none=none), {"jr": ncon}))
    for none in ((), ("wc",)):
        out.append(("jsq_cols", lambda i, o: f("jsq_cols")(i["x"], i["wc"], o["jc"], **kw), pick(V, "x", "wc", none=none), {"jc": nvar}))
    for none in ((), ("y", "sx", "sc")):
        out.append(("kktprod", lambda i, o: f("kktprod")(i["x"], i["y"], i["v"], i["w"], SIGMA, i["sx"], i["sc"], out=(o["rx"], o["rc"]), **kw),
                    pick(V, "x", "y", "v", "w", "sx", "sc", none=none), {"rx": nvar, "rc": ncon}))
        out.append(("kktprod halves", lambda i, o: f("kktprod")(i["x"], i["y"], i["z"][:nvar], i["z"][nvar:], SIGMA, i["sx"], i["sc"],
                                                                 out=(o["r"][:nvar], o["r"][nvar:]), **kw),
                    pick(dict(V, z=z), "x", "y", "z", "sx", "sc", none=none), {"r": nvar + ncon}))
    if shard:
        out.append(("grad", lambda i, o: d.grad_shard(i["x"], o["g"], sync=True), pick(V, "x"), {"g": nvar}))
    return out


MF_HANDLES = [("goddard_all", "trapeze", (1, 2, 7, 300)),
              ("double_integrator_freet0tf", "gauss_legendre_2", (1, 2, 7, 300)),          # two free times: the nv tail
              ("double_integrator_path", "midpoint", (1, 2, 7, 300)),                      # nv = 0
              ("quadrotor12", "gauss_legendre_3", (2, 7))]
MF_CASES = [(p, s, N) for p, s, Ns in MF_HANDLES for N in Ns]


@pytest.mark.parametrize("prob,sch,N", MF_CASES, ids=[f"{p}-{s}-N{N}" for p, s, N in MF_CASES])
def test_matrix_free_operators(torch_cuda, monkeypatch, prob, sch, N):
    set_env(monkeypatch)
    d = open_handle(prob, N, sch, pattern="structural")
    V = vectors(d, prob, sch)
    for name, call, inputs, outputs in operator_calls(d, V, shard=False):
        check_call(torch_cuda, call, inputs, outputs, True, (prob, sch, N, name, [k for k, a in inputs.items() if a is None]))
    d.close()


SHARD_CUTS = [(SHARD_SIZES[0][0], SHARD_SIZES[0][1]), (300, (0, 100, 201, 300))]
SHARD_CASES = [(p, s, N, cuts, k) for p, s in (("goddard_all", "trapeze"), ("double_integrator_path", "midpoint"))
               for N, cuts in SHARD_CUTS for k in range(3)]


@pytest.mark.parametrize("prob,sch,N,cuts,k", SHARD_CASES, ids=[f"{p}-{s}-N{N}-shard{k}" for p, s, N, _, k in SHARD_CASES])
def test_shard_forms(torch_cuda, monkeypatch, prob, sch, N, cuts, k):
    """the eight *_shard_dev_async calls on one shard of three: no shard table, the iterate holds the halos"""
    set_env(monkeypatch)
    d = open_handle(prob, N, sch, pattern="structural", steps=(cuts[k], cuts[k + 1]))
    V = vectors(d, prob, sch)
    for name, call, inputs, outputs in operator_calls(d, V, shard=True):
        check_call(torch_cuda, call, inputs, outputs, False, (prob, sch, N, "shard", k, name, [q for q, a in inputs.items() if a is None]))
    d.close()


# ---- batched forms -----------------------------------------------------------------------------------------------------------------
def test_batched_forms(torch_cuda, monkeypatch):
    """K = 3 iterates; every matrix argument has the leading dimension n + 7 inside its guarded buffer"""
    prob, sch, N, K = "goddard", "gauss_legendre_2", 37, 3
    set_env(monkeypatch)
    d = open_handle(prob, N, sch)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    x = bench_inputs(describe(d, prob, sch), perturb=1e-3)
    X = np.stack([x * (1.0 + 0.01 * b) for b in range(K)])
    Y = np.stack([np.cos(0.37 * np.arange(ncon) + b) for b in range(K)])
    check_call(torch_cuda, lambda i, o: d.cons_jac_batch(i["X"], o["C"], o["V"]), {"X": X}, {"C": (K, ncon), "V": (K, d.nnzj)}, True, ("cons_jac_batch",))
    check_call(torch_cuda, lambda i, o: d.grad_batch(i["X"], o["G"]), {"X": X}, {"G": (K, nvar)}, True, ("grad_batch",))
    check_call(torch_cuda, lambda i, o: d.hess_coord_batch(i["X"], i["Y"], SIGMA, o["H"]), {"X": X, "Y": Y}, {"H": (K, d.nnzh)}, True,
               ("hess_coord_batch",))
    check_call(torch_cuda, lambda i, o: d.obj_batch(i["X"], o["f"]), {"X": X}, {"f": K}, True, ("obj_batch",))
    d.close()


# ---- run-time (hiprtc) kernels -----------------------------------------------------------------------------------------------------
def test_run_time_kernels(torch_cuda, monkeypatch):
    """the same bodies, compiled separately at run time: one warm call of each entry point first"""
    torch = torch_cuda
    prob, sch, N = "goddard", "midpoint", 7
    set_env(monkeypatch)
    d = open_handle(prob, N, sch, rt=True)
    V = vectors(d, prob, sch)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    xd, yd, vd, wd = (torch.from_numpy(V[k]).cuda() for k in ("x", "y", "v", "w"))
    d.cons_jac(xd)
    d.hess_coord(xd, yd, SIGMA)
    d.kktprod(xd, yd, vd, wd, SIGMA)
    d.hdiag(xd, yd, SIGMA)
    cons_jac_forms(torch, d, V["x"], True, ("run-time",))
    check_call(torch, hess_call(d), pick(V, "x", "y"), {"hvals": d.nnzh}, True, ("run-time", "hess_coord"))
    for name, call, inputs, outputs in operator_calls(d, V, shard=False):
        if name in ("kktprod", "kktprod halves", "hdiag"):
            check_call(torch, call, inputs, outputs, True, ("run-time", name, [k for k, a in inputs.items() if a is None]))
    d.close()
