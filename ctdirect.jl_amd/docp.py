"""Host-side mirror of the reference interface for the collocation hot path.

Names, argument meaning and error behaviour follow CTDirect.jl (the reference is Julia; Julia is not available in
this image, so the mirror above the C ABI is Python -- INTEGRATION.md holds the Julia `ccall` shim a maintainer
would add).  What is mirrored:

    CTDirect.DOCP(ocp, grid_size, control_steps, scheme, time_grid)          src/DOCP_data.jl:293-365
    docp.dims / docp.flags / docp.time / docp.bounds / dim_NLP_*             src/DOCP_data.jl:24-30,88-94,147-152,235-240
    CTDirect.__constraints!(c, xu, docp)                                     src/DOCP_functions.jl:80-115
    CTDirect.__objective(xu, docp)                                           src/DOCP_functions.jl:23-54
    CTDirect.__variables_bounds!(docp), __constraints_bounds!(docp)          src/DOCP_variables.jl:21-63, DOCP_functions.jl:163-191
    CTDirect.__initial_guess(docp, init)                                     src/DOCP_variables.jl:122-145
    CTDirect.DOCP_Jacobian_pattern(docp)                                     src/ode/{trapeze,midpoint,irk,irk_stagewise}.jl
    NLPModels: obj, cons!, jac_structure!, jac_coord!                        served by ADNLPModels in the reference
                                                                             (src/collocation.jl:137-149)

All arithmetic happens in the HIP library; this module only moves pointers.  NumPy arrays go through the
host-pointer entry points, torch CUDA(=HIP) tensors through the device-pointer ones.
"""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib

SCHEMES = {
    "trapeze": 0,
    "midpoint": 1,
    "gauss_legendre_1": 2,
    "gauss_legendre_2_constant_control": 3,
    "gauss_legendre_3_constant_control": 4,
    "gauss_legendre_2": 5,
    "gauss_legendre_3": 6,
    "euler": 7,
    "euler_implicit": 8,
}
# the reference's aliases (src/DOCP_data.jl:315-320)
SCHEME_ALIASES = {"euler_explicit": "euler", "euler_forward": "euler", "euler_backward": "euler_implicit"}
PROBLEMS = {
    "goddard": 0,
    "goddard_all": 1,
    "double_integrator_path": 2,
    "quadrotor": 3,
    "quadrotor12": 4,
    "stagewise_scalar": 5,
    "estimate_initial_condition": 6,
    "estimate_rotation_rate": 7,
    "least_squares_with_constraint": 8,
    "double_integrator_freet0tf": 9,
}
PATTERN_MODES = {"manual": 0, "reference_manual": 0, "structural": 1, "optimized": 2}
VALUE_ORDERS = {"csc": 0, "csr": 1}


class CTDirectError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"[ctd status {status}] {message}")
        self.status = status


def _raise(status, msg):
    # same exception kinds as the reference: ArgumentError for the grid (src/DOCP_data.jl:186-189) -> ValueError
    if status == _lib.CTD_EGRID:
        raise ValueError(msg)
    raise CTDirectError(status, msg)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _host_out(a, n, name):
    """A caller-supplied NumPy output of the host-pointer entry points: the library writes n doubles through the raw pointer,
    so anything but a C-contiguous float64 array of exactly n entries would corrupt host memory."""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"] and a.size == n):
        raise ValueError(f"{name} must be a writeable C-contiguous float64 NumPy array of {n} entries")
    return a


def _is_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


# The matrix-free operators, one row each (DOCP._mf): the vector inputs in the order of the C arguments, x first, as (name, layout,
# required) -- layout "v": dim_NLP_variables entries, "c": dim_NLP_constraints --; the number of them that the scalar arguments
# follow; the outputs as (name, layout).  The entry points are ctd_<op> (host pointers), ctd_<op>_dev_async and
# ctd_<op>_shard_dev_async
_MF_OPS = {
    "jprod": ((("x", "v", True), ("v", "v", True)), 2, (("out", "c"),)),
    "jtprod": ((("x", "v", True), ("w", "c", True)), 2, (("out", "v"),)),
    "hprod": ((("x", "v", True), ("y", "c", False), ("v", "v", True)), 2, (("out", "v"),)),
    "kktprod": ((("x", "v", True), ("y", "c", False), ("dx", "v", True), ("dy", "c", True), ("sx", "v", False), ("sc", "c", False)), 2,
                (("out[0]", "v"), ("out[1]", "c"))),
    "hdiag": ((("x", "v", True), ("y", "c", False)), 2, (("out", "v"),)),
    "jsq_rows": ((("x", "v", True), ("wx", "v", False)), 2, (("out", "c"),)),
    "jsq_cols": ((("x", "v", True), ("wc", "c", False)), 2, (("out", "v"),)),
}


# What DOCP.kkt_minres / kkt_minres_info return with the iterate: status is "running", "converged", "max_iter" or "breakdown";
# iterations: the completed ones; phibar: the estimate of the M-norm of the residual, beta1 its initial value; Anorm, ynorm: the
# estimates of |K| and |z| (ctd_minres_info)
MinresInfo = namedtuple("MinresInfo", "status iterations phibar Anorm ynorm beta1")
# The caller-owned workspace of a sharded solve (DOCP.kkt_minres_shard_workspace): the tensor, its layout (ctd_minres_shard_layout)
# and the views the caller exchanges or hands to kktprod_shard
# The chunked block-tridiagonal Schur preconditioner of DOCP.kkt_schur_precond: the pair (px, pc) of kkt_diag_precond it was built
# from, the factor's workspace (a device tensor of layout.workspace doubles) and the layout (ctd_schur_layout)
SchurPrecond = namedtuple("SchurPrecond", "px pc ws layout")
# ... and its log-depth exact form of DOCP.kkt_schur_cr_precond (layout: ctd_schur_cr_layout)
SchurCrPrecond = namedtuple("SchurCrPrecond", "px pc ws layout")
# ... and the shard form of that, of DOCP.kkt_schur_cr_shard_factor: the factor of the handle's own steps (layout:
# ctd_schur_cr_shard_layout); px, pc full-length, valid where the shard reads them
SchurCrShardPrecond = namedtuple("SchurCrShardPrecond", "px pc ws layout")
# ... and the joined form of that, of DOCP.kkt_schur_cr_joint_factor_local: the rank's local factor and, after the join, the reduced
# factor (layout: ctd_schur_cr_joint_layout); send, xsend: the rank's factor record and solve record
SchurCrJointPrecond = namedtuple("SchurCrJointPrecond", "px pc ws layout send xsend")
MinresShardWorkspace = namedtuple("MinresShardWorkspace", "ws layout n_ranks v_x v_c kv_x kv_c send_a send_b gathered_a gathered_b")
# A family of sharded MINRES phases (layout, start, begin, alfa, lanczos, update, info): the prefix of its C entry points, the slot
# length its workspaces are cut with, the class of the preconditioner it carries (None: none, or a pair (px, pc)), whether its
# layout query takes the rank, and the phases that take the factor's workspace.  DOCP._phase_* are the one implementation behind the
# public kkt_minres_*shard* / *joint* methods; dist.MinresPhases picks the family from the preconditioner (_phase_family).
_PhaseFamily = namedtuple("_PhaseFamily", "prefix slot precond layout_rank schur")
_PHASE_FAMILIES = (
    _PhaseFamily("ctd_kkt_minres_shard_", _lib.KKT_MINRES_SHARD_SLOT, None, False, ()),
    _PhaseFamily("ctd_kkt_minres_schur_cr_shard_", _lib.KKT_MINRES_SCHUR_SHARD_SLOT, SchurCrShardPrecond, False, ("start", "lanczos")),
    _PhaseFamily("ctd_kkt_minres_schur_cr_joint_", _lib.KKT_MINRES_SCHUR_JOINT_SLOT, SchurCrJointPrecond, True,
                ("start", "begin", "lanczos", "update")))
_PLAIN, _SCHUR_SHARD, _SCHUR_JOINT = _PHASE_FAMILIES


def _phase_family(precond):
    """the phase family of a sharded solve with `precond`: that of its class, the diagonal form's otherwise"""
    return next((f for f in _PHASE_FAMILIES if f.precond is not None and isinstance(precond, f.precond)), _PLAIN)


def _mf_rows(L, nvar, ncon):
    """_MF_OPS for one handle, per operator: the names and the lengths of its vectors, inputs then outputs; the number of inputs;
    the positions of the required inputs; the position of the scalars; the three entry points of the library L"""
    n = {"v": nvar, "c": ncon}
    return {op: (tuple(nm for nm, *_ in ins + outs), tuple(n[row[1]] for row in ins + outs), len(ins),
                 tuple(i for i, row in enumerate(ins) if row[2]), k,
                 (getattr(L, f"ctd_{op}"), getattr(L, f"ctd_{op}_dev_async"), getattr(L, f"ctd_{op}_shard_dev_async")))
            for op, (ins, k, outs) in _MF_OPS.items()}


def register_ocp(name, *, dynamics, n=None, m=0, nv=0, lagrange=None, mayer=None, path=(), boundary=(), constants=None,
                 t0=0.0, tf=1.0, it0=-1, itf=-1, maximize=False, state_box=None, control_box=None, variable_box=None,
                 path_bounds=None, boundary_bounds=None):
    """Defines an OCP at run time from arithmetic expressions (the stand-in for the Julia closures of a CTModels.Model,
    include/ctdirect_hip.h `ctd_ocp_def`) and returns `name`, usable as the `ocp` argument of DOCP.

    dynamics / path: expressions in t, x1..xn, u1..um, v1..vnv; mayer / boundary: in x0_k, xf_k, vk; `constants` a dict of
    numbers (constants) and strings (aliases: named sub-expressions, e.g. the `aux = ...` lines of a CTParser @def block).
    Functions: exp log sin cos tan atan tanh sqrt abs asin acos sinh cosh floor, max(a, b), min(a, b); `^` takes a constant exponent.
    Boxes and bounds are (lb, ub) pairs of sequences (None = free boxes / equality-with-zero rows); it0 / itf are the
    0-based positions of a free initial / final time inside v.  The kernels are compiled with hiprtc when a DOCP is built."""
    L = _lib.lib()
    dynamics = list(dynamics)
    n = len(dynamics) if n is None else int(n)
    path, boundary = list(path), list(boundary)
    d = _lib.ctd_ocp_def()
    keep = []

    def strs(items):
        arr = (C.c_char_p * max(len(items), 1))(*[s.encode() for s in items])
        keep.append(arr)
        return C.cast(arr, C.POINTER(C.c_char_p))

    def dbl(seq, dim, fill):
        a = np.full(dim, fill, dtype=np.float64) if seq is None else np.ascontiguousarray(seq, dtype=np.float64)
        if a.size != dim:
            raise ValueError(f"bound array has {a.size} entries, expected {dim}")
        keep.append(a)
        return _dp(a) if dim else None

    d.name = name.encode()
    d.n, d.m, d.nv, d.npath, d.nbc = n, int(m), int(nv), len(path), len(boundary)
    d.it0, d.itf, d.t0, d.tf, d.maximize = int(it0), int(itf), float(t0), float(tf), int(bool(maximize))
    d.dynamics, d.path, d.boundary = strs(dynamics), strs(path), strs(boundary)
    d.lagrange = lagrange.encode() if lagrange else None
    d.mayer = mayer.encode() if mayer else None
    # numbers are constants; strings are aliases: named sub-expressions ("aux = 543 + 186*cos(x4) + ...") substituted where used
    d.constants = "; ".join(f"{k}={v if isinstance(v, str) else repr(float(v))}" for k, v in constants.items()).encode() if constants else None
    inf = float("inf")
    for key, box, dim in (("state", state_box, n), ("control", control_box, int(m)), ("variable", variable_box, int(nv))):
        setattr(d, key + "_lb", dbl(None if box is None else box[0], dim, -inf))
        setattr(d, key + "_ub", dbl(None if box is None else box[1], dim, inf))
    for key, bnd, dim in (("path", path_bounds, len(path)), ("boundary", boundary_bounds, len(boundary))):
        setattr(d, key + "_lb", dbl(None if bnd is None else bnd[0], dim, 0.0))
        setattr(d, key + "_ub", dbl(None if bnd is None else bnd[1], dim, 0.0))
    pid = C.c_int32()
    st = L.ctd_register_ocp(C.byref(d), C.byref(pid))
    if st != _lib.CTD_OK:
        _raise(st, L.ctd_last_error(None).decode())
    PROBLEMS[name] = pid.value
    return name


def ocp_source(name):
    """The functor text generated for a run-time OCP (diagnostics)."""
    L = _lib.lib()
    cap = 1 << 16
    for _ in range(2):
        buf = C.create_string_buffer(cap)
        st = L.ctd_ocp_source(PROBLEMS[name], buf, len(buf))
        if st == _lib.CTD_OK:
            return buf.value.decode()
        msg = L.ctd_last_error(None).decode()
        if "needs" not in msg:
            _raise(st, msg)
        cap = int(msg.split("needs")[1].split()[0])
    _raise(st, msg)


def jit_check(name, scheme):
    """Compile-only check (no GPU needed): the kernels of `scheme` build for gfx950 for a run-time OCP."""
    L = _lib.lib()
    st = L.ctd_jit_check(PROBLEMS[name], SCHEMES[scheme] if isinstance(scheme, str) else int(scheme))
    if st != _lib.CTD_OK:
        _raise(st, L.ctd_last_error(None).decode())


class DOCP:
    """Discretised OCP handle; mirrors `CTDirect.DOCP(ocp, grid_size, control_steps, scheme, time_grid)` (src/DOCP_data.jl:293).

    `ocp` is the name (or id) of a problem of the compiled registry (include/ctdirect_hip.h) -- the reference takes
    a CTModels.Model with Julia closures, which cannot cross the C ABI to the GPU.
    `device` is the HIP device ordinal; -1 builds a host-only handle (sizes, bounds, patterns, initial guess).
    `steps=(begin, end)` restricts the handle to a shard of the time grid (multi-GPU).
    `stream`: "torch" (default) launches on torch's current stream of `device` when torch sees that GPU, so the
    callbacks are ordered with the caller's tensor work; "own" gives the handle a private stream; an integer is a raw
    hipStream_t.
    `control_steps` > 1: the direct-shooting layout (src/direct_shooting.jl:55-71; :midpoint only): `control_steps` controls per
    time step, dynamics summed over the control sub-steps (midpoint.jl:137-155).
    `value_order`: "csc" (default: the reference's SparseArrays.sparse order, what jac_coord! fills) or "csr" (the same entries by
    rows: `jac_structure`, `jac_coord`, `cons_jac` follow it; `DOCP_Jacobian_csr` gives rowptr / colind).
    """

    def __init__(self, ocp, grid_size=250, scheme="midpoint", time_grid=None, *, pattern="manual", device=0,
                 steps=None, stream="torch", control_steps=1, value_order="csc"):
        L = _lib.lib()
        self.problem_name = ocp if isinstance(ocp, str) else {v: k for k, v in PROBLEMS.items()}.get(int(ocp), str(ocp))
        pid = PROBLEMS[ocp] if isinstance(ocp, str) else int(ocp)
        if isinstance(scheme, str):
            scheme = SCHEME_ALIASES.get(scheme, scheme)
            if scheme not in SCHEMES:
                _raise(_lib.CTD_ESCHEME, f"Unknown discretization method: {scheme}")    # src/DOCP_data.jl:342-349
            sid = SCHEMES[scheme]
        else:
            sid = int(scheme)
        self.scheme = scheme
        d = _lib.ctd_desc()
        d.problem, d.scheme = pid, sid
        d.pattern_mode = PATTERN_MODES[pattern] if isinstance(pattern, str) else int(pattern)
        d.device = int(device)
        self._tg = None
        if time_grid is not None:
            self._tg = np.ascontiguousarray(time_grid, dtype=np.float64)
            d.time_grid = _dp(self._tg)
            d.time_grid_len = len(self._tg)
            d.grid_size = len(self._tg) - 1
        else:
            d.time_grid = None
            d.time_grid_len = 0
            d.grid_size = int(grid_size)
        if steps is not None:
            d.step_begin, d.step_end = int(steps[0]), int(steps[1])
        d.stream, d.stream_mode = None, 0
        d.control_steps = int(control_steps)
        d.value_order = VALUE_ORDERS[value_order] if isinstance(value_order, str) else int(value_order)
        d.reserved0 = 0
        self.value_order = {0: "csc", 1: "csr"}.get(d.value_order, str(d.value_order))
        self.control_steps = max(1, int(control_steps))
        if int(device) >= 0 and stream != "own":
            if stream == "torch":
                try:
                    import torch
                    if torch.cuda.is_available():
                        d.stream = C.c_void_p(torch.cuda.current_stream(int(device)).cuda_stream)
                        d.stream_mode = 1
                except ImportError:
                    pass
            elif stream is not None:
                d.stream, d.stream_mode = C.c_void_p(int(stream)), 1
        self._stream_raw = int(d.stream or 0) if d.stream_mode == 1 else None      # the handle's stream when Python knows it
        h = C.c_void_p()
        st = L.ctd_create(C.byref(d), C.byref(h))
        if st != _lib.CTD_OK:
            _raise(st, L.ctd_last_error(None).decode())
        self._h = h
        self._schur_cr_shard_layout = None      # kkt_schur_cr_shard_layout's answer, kept: the handle's steps never change
        self.device = int(device)
        self._load_static()
        if d.pattern_mode == 0 and self.dropped_nonzeros() > 0:
            # the reference's :manual pattern leaves structural nonzeros out here (trapeze.jl:203: dynamics rows x variables;
            # euler.jl:231: implicit Euler's path rows x previous control): values at the pattern's positions are exact, but
            # a solver fed this Jacobian misses those entries
            import warnings
            warnings.warn(f"pattern='manual' reproduces the reference's DOCP_Jacobian_pattern, which omits {self.dropped_nonzeros()} "
                          f"structural nonzeros for {self.problem_name} / {self.scheme}; pass pattern='structural' (or 'optimized') "
                          "to solve with a complete Jacobian", stacklevel=2)

    # ---- static data ------------------------------------------------------------------------------------
    def _load_static(self):
        L = _lib.lib()
        nvar, ncon, nnzj, nnzh = (C.c_int64() for _ in range(4))
        self._ck(L.ctd_sizes(self._h, C.byref(nvar), C.byref(ncon), C.byref(nnzj), C.byref(nnzh)))
        self.dim_NLP_variables, self.dim_NLP_constraints = nvar.value, ncon.value
        self._mf_rows = _mf_rows(L, nvar.value, ncon.value)
        self._f64 = None
        self.nnzj, self.nnzh = nnzj.value, nnzh.value
        o = np.zeros(16, dtype=np.int64)
        self._ck(L.ctd_dims(self._h, _ip(o)))
        self.dims = SimpleNamespace(NLP_x=int(o[0]), NLP_u=int(o[1]), NLP_v=int(o[2]), path_cons=int(o[3]),
                                    boundary_cons=int(o[4]))
        self.flags = SimpleNamespace(freet0=bool(o[11]), freetf=bool(o[12]), lagrange=bool(o[13]), mayer=bool(o[14]),
                                     max=bool(o[15]))
        stage = int(o[9])
        self.discretization = SimpleNamespace(_step_variables_block=int(o[6]), _state_stage_eqs_block=int(o[7]),
                                              _step_pathcons_block=int(o[8]), stage=stage, _final_control=bool(o[10]))
        steps = int(o[5])
        nrm = np.zeros(steps + 1)
        fx = np.zeros(steps + 1)
        self._ck(L.ctd_time_grid(self._h, _dp(nrm), _dp(fx)))
        self.time = SimpleNamespace(steps=steps, control_steps=getattr(self, "control_steps", 1), normalized_grid=nrm, fixed_grid=fx)
        if stage > 0:
            a = np.zeros(stage * stage); b = np.zeros(stage); c = np.zeros(stage)
            self._ck(L.ctd_butcher(self._h, _dp(a), _dp(b), _dp(c)))
            self.discretization.butcher_a = a.reshape(stage, stage)
            self.discretization.butcher_b, self.discretization.butcher_c = b, c
        sh = np.zeros(8, dtype=np.int64)
        self._ck(L.ctd_shard_info(self._h, _ip(sh)))
        self.shard = SimpleNamespace(step_begin=int(sh[0]), step_end=int(sh[1]), c_row_begin=int(sh[2]), c_row_end=int(sh[3]),
                                     vals_main_begin=int(sh[4]), vals_main_end=int(sh[5]), owns_first=bool(sh[6]),
                                     owns_last=bool(sh[7]))
        self._bounds = None

    def _ck(self, st):
        if st != _lib.CTD_OK:
            _raise(st, _lib.lib().ctd_last_error(self._h).decode() or _lib.lib().ctd_strerror(st).decode())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().ctd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def bounds(self):
        """docp.bounds with var_l, var_u, con_l, con_u (filled by __variables_bounds! / __constraints_bounds!)."""
        if self._bounds is None:
            lv = np.zeros(self.dim_NLP_variables); uv = np.zeros(self.dim_NLP_variables)
            lc = np.zeros(self.dim_NLP_constraints); uc = np.zeros(self.dim_NLP_constraints)
            self._ck(_lib.lib().ctd_bounds(self._h, _dp(lv), _dp(uv), _dp(lc), _dp(uc)))
            self._bounds = SimpleNamespace(var_l=lv, var_u=uv, con_l=lc, con_u=uc)
        return self._bounds

    def launch_info(self):
        o = np.zeros(8, dtype=np.int64)
        self._ck(_lib.lib().ctd_launch_info(self._h, _ip(o)))
        return dict(grid=int(o[0]), block=int(o[1]), lds_bytes=int(o[2]), steps_per_tile=int(o[3]),
                    csc_period=int(o[4]), edge_entries=int(o[5]), direct_tiles=int(o[6]), workgroups_per_cu=int(o[7]))

    def dropped_nonzeros(self):
        n = C.c_int64()
        self._ck(_lib.lib().ctd_dropped_nonzeros(self._h, C.byref(n)))
        return n.value

    # ---- NLPModels-style callbacks --------------------------------------------------------------------------
    def _check_x(self, x):
        """x has dim_NLP_variables entries; returns whether it is a tensor"""
        dev = _is_tensor(x)
        n = x.numel() if dev else x.size
        if n != self.dim_NLP_variables:
            raise ValueError(f"x has {n} entries, expected dim_NLP_variables = {self.dim_NLP_variables}")
        return dev

    def _dev_ptr(self, t, n, name):
        """The device pointer of the tensor t, checked: n float64 entries, contiguous, on the handle's GPU.  None (an optional
        argument left out) gives None, the C side's NULL"""
        if t is None:
            return None
        f64 = self._f64
        if f64 is None:                 # (torch is imported by the first call that is given a tensor)
            import torch
            f64 = self._f64 = torch.float64
        if not (t.is_cuda and t.dtype == f64 and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"{name} must be a contiguous float64 tensor of {n} entries on the handle's GPU")
        if t.device.index != self.device:
            raise ValueError(f"{name} lives on cuda:{t.device.index}, handle is bound to device {self.device}")
        return C.c_void_p(t.data_ptr())

    def cons_jac(self, x, c=None, vals=None, sync=True):
        """Fused cons!(nlp, x, c) + jac_coord!(nlp, x, vals): the benchmarked call.  Returns (c, vals)."""
        L = _lib.lib()
        self._check_x(x)
        if _is_tensor(x):
            import torch
            if c is None:
                c = torch.empty(self.dim_NLP_constraints, dtype=torch.float64, device=x.device)
            if vals is None:
                vals = torch.empty(self.nnzj, dtype=torch.float64, device=x.device)
            fn = L.ctd_cons_jac_dev if sync else L.ctd_cons_jac_dev_async
            self._ck(fn(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                        self._dev_ptr(c, self.dim_NLP_constraints, "c"), self._dev_ptr(vals, self.nnzj, "vals")))
            return c, vals
        x = np.ascontiguousarray(x, dtype=np.float64)
        c = np.empty(self.dim_NLP_constraints) if c is None else _host_out(c, self.dim_NLP_constraints, "c")
        vals = np.empty(self.nnzj) if vals is None else _host_out(vals, self.nnzj, "vals")
        self._ck(L.ctd_cons_jac(self._h, _dp(x), _dp(c), _dp(vals)))
        return c, vals

    def bind_cons_jac(self, x, c, vals, sync=False):
        """Pre-binds the device pointers of (x, c, vals) and returns a zero-argument callable that enqueues one fused
        evaluation -- the per-iteration path of a GPU-resident solver loop, without the Python argument checks."""
        L = _lib.lib()
        fn = L.ctd_cons_jac_dev if sync else L.ctd_cons_jac_dev_async
        h = self._h
        px = self._dev_ptr(x, self.dim_NLP_variables, "x")
        pc = self._dev_ptr(c, self.dim_NLP_constraints, "c")
        pv = self._dev_ptr(vals, self.nnzj, "vals")
        ck = self._ck

        def call():
            st = fn(h, px, pc, pv)
            if st:
                ck(st)
        return call

    def set_x_shards(self, step_begins, x_ptrs, self_index):
        """Sharded iterate read in place (`ctd_set_x_shards`): from now on the constraint / Jacobian kernels of this shard
        handle load the entries other shards own (next shard's first node, previous shard's last block, X_1, X_{N+1}) straight
        from `x_ptrs[k]` -- raw device pointers of the shards' full-length buffers (peer- or IPC-mapped).  `step_begins` has
        one entry per shard plus N.  `step_begins=None` switches back."""
        L = _lib.lib()
        if step_begins is None:
            self._ck(L.ctd_set_x_shards(self._h, 0, None, None, 0))
            return
        G = len(x_ptrs)
        sb = np.ascontiguousarray(step_begins, dtype=np.int64)
        assert sb.size == G + 1
        arr = (C.c_void_p * G)(*[int(p) if p else None for p in x_ptrs])
        self._ck(L.ctd_set_x_shards(self._h, G, _ip(sb), arr, int(self_index)))

    def stitch_c(self, comm, n_ranks, rank, c):
        """`ctd_stitch_c`: all-gather of the row blocks of the device tensor c over the ncclComm_t `comm` (an integer / c_void_p:
        the host's RCCL communicator), inside the library -- the one-process-per-GPU route that needs no torch.distributed."""
        self._ck(_lib.lib().ctd_stitch_c(self._h, C.c_void_p(int(comm)), int(n_ranks), int(rank),
                                         self._dev_ptr(c, self.dim_NLP_constraints, "c")))
        return c

    def cons(self, x, c=None):
        """cons!(nlp, x, c) = __constraints!(c, x, docp); returns c (the reference's closure must return c too)."""
        L = _lib.lib()
        self._check_x(x)
        if _is_tensor(x):
            import torch
            if c is None:
                c = torch.empty(self.dim_NLP_constraints, dtype=torch.float64, device=x.device)
            self._ck(L.ctd_cons_jac_dev(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                        self._dev_ptr(c, self.dim_NLP_constraints, "c"), None))
            return c
        x = np.ascontiguousarray(x, dtype=np.float64)
        c = np.empty(self.dim_NLP_constraints) if c is None else _host_out(c, self.dim_NLP_constraints, "c")
        self._ck(L.ctd_cons(self._h, _dp(x), _dp(c)))
        return c

    def jac_coord(self, x, vals=None):
        """jac_coord!(nlp, x, vals): Jacobian values in the CSC order of DOCP_Jacobian_pattern."""
        L = _lib.lib()
        self._check_x(x)
        if _is_tensor(x):
            import torch
            if vals is None:
                vals = torch.empty(self.nnzj, dtype=torch.float64, device=x.device)
            self._ck(L.ctd_cons_jac_dev(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"), None,
                                        self._dev_ptr(vals, self.nnzj, "vals")))
            return vals
        x = np.ascontiguousarray(x, dtype=np.float64)
        vals = np.empty(self.nnzj) if vals is None else _host_out(vals, self.nnzj, "vals")
        self._ck(L.ctd_jac_coord(self._h, _dp(x), _dp(vals)))
        return vals

    def obj(self, x):
        """obj(nlp, x) = __objective(x, docp).  For a sharded handle: the shard's partial sum."""
        L = _lib.lib()
        self._check_x(x)
        f = C.c_double()
        if _is_tensor(x):
            self._ck(L.ctd_obj_dev(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"), C.byref(f)))
        else:
            x = np.ascontiguousarray(x, dtype=np.float64)
            self._ck(L.ctd_obj(self._h, _dp(x), C.byref(f)))
        return f.value

    def obj_async(self, x, f):
        """Enqueue obj(nlp, x) with the value written to the 1-element device tensor `f` (no host copy, no wait)."""
        self._check_x(x)
        self._ck(_lib.lib().ctd_obj_dev_async(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"), self._dev_ptr(f, 1, "f")))
        return f

    def grad(self, x, g=None, sync=True):
        """grad!(nlp, x, g): gradient of __objective (ReverseDiff over the closure in the reference, src/collocation.jl:127)."""
        L = _lib.lib()
        self._check_x(x)
        if _is_tensor(x):
            import torch
            if g is None:
                g = torch.empty(self.dim_NLP_variables, dtype=torch.float64, device=x.device)
            fn = L.ctd_grad_dev if sync else L.ctd_grad_dev_async
            self._ck(fn(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"), self._dev_ptr(g, self.dim_NLP_variables, "g")))
            return g
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.empty(self.dim_NLP_variables) if g is None else _host_out(g, self.dim_NLP_variables, "g")
        self._ck(L.ctd_grad(self._h, _dp(x), _dp(g)))
        return g

    def _mf(self, op, shard, vecs, scalars, outs, sync):
        """One call of the matrix-free operator `op`, a row of _MF_OPS.  vecs: its vector inputs in the row's order, x first, None
        for an optional one left out; outs: its outputs, allocated when None.  shard: `ctd_<op>_shard_dev_async`, device tensors
        only, every length checked by name; otherwise `ctd_<op>_dev_async` for device tensors and `ctd_<op>` for NumPy arrays.
        Device calls are followed by a sync when `sync`.  Returns the output, or the tuple of them."""
        names, lens, nin, required, k, fns = self._mf_rows[op]
        for i in required:
            if vecs[i] is None:
                raise ValueError(f"{names[i]} is required")
        x = vecs[0]
        dev = hasattr(x, "is_cuda")
        if (x.numel() if dev else x.size) != lens[0]:
            self._check_x(x)
        if shard:
            for a, nm, n in zip(vecs + outs, names, lens):
                if a is not None:
                    if not hasattr(a, "is_cuda"):
                        raise TypeError(f"{nm} must be a device tensor: {op}_shard has no host path")
                    if a.numel() != n:
                        raise ValueError(f"{nm} has {a.numel()} entries, expected {n}")
        if dev:
            if outs[0] is None or outs[-1] is None:         # (one output or two)
                import torch
                outs = tuple(torch.empty(n, dtype=torch.float64, device=x.device) if a is None else a for a, n in zip(outs, lens[nin:]))
            args = list(map(self._dev_ptr, vecs + outs, lens, names))
            fn = fns[2 if shard else 1]
        else:
            args = []
            for a, nm, n in zip(vecs, names, lens):
                if a is not None:
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    if a.size != n:
                        raise ValueError(f"{nm} has {a.size} entries, expected {n}")
                args.append(_dp(a))
            outs = tuple(np.empty(n) if a is None else _host_out(a, n, nm) for a, nm, n in zip(outs, names[nin:], lens[nin:]))
            args.extend(map(_dp, outs))
            fn, sync = fns[0], False
        if scalars:
            args[k:k] = scalars
        self._ck(fn(self._h, *args))
        if sync:
            self.sync()
        return outs[0] if len(outs) == 1 else outs

    def jprod(self, x, v, out=None, sync=True):
        """jprod!(nlp, x, v, Jv): J(x) v without assembling J (ncon entries).  J is the exact derivative of the constraints
        (the structural Jacobian, whatever the pattern mode).  NumPy inputs use the host entry point; device tensors are
        enqueued on the handle's stream (`ctd_jprod_dev_async`), followed by a sync when `sync`."""
        return self._mf("jprod", False, (x, v), (), (out,), sync)

    def jtprod(self, x, w, out=None, sync=True):
        """jtprod!(nlp, x, w, Jtw): J(x)' w without assembling J (nvar entries); see `jprod`."""
        return self._mf("jtprod", False, (x, w), (), (out,), sync)

    def hprod(self, x, y, v, obj_weight=1.0, out=None, sync=True):
        """hprod!(nlp, x, y, v, Hv; obj_weight): (obj_weight d2 f + sum_i y_i d2 c_i)(x) v without assembling the Hessian (nvar
        entries).  y = None: the objective-only hprod!(nlp, x, v, Hv; obj_weight).  The Hessian is the exact second derivative
        of the objective and the constraints (the structural one, whatever the pattern mode).  NumPy inputs use the host entry
        point; device tensors are enqueued on the handle's stream (`ctd_hprod_dev_async`), followed by a sync when `sync`."""
        return self._mf("hprod", False, (x, y, v), (float(obj_weight),), (out,), sync)

    def kktprod(self, x, y, dx, dy, obj_weight=1.0, sx=None, sc=None, out=None, sync=True):
        """The regularised KKT operator of an interior-point / SQP step applied to (dx, dy), matrix-free:
            rx = (obj_weight d2 f + sum_i y_i d2 c_i)(x) dx + J(x)' dy + sx * dx      (nvar entries)
            rc = J(x) dx - sc * dy                                                    (ncon entries; note the sign of sc)
        in two kernel launches (`ctd_kktprod*`).  y = None: all multipliers zero; sx / sc = None: no diagonal term.  Returns
        (rx, rc); `out` is a pair (rx, rc), which may be two slices of one tensor, as may dx and dy.  The Hessian and the Jacobian
        are the structural ones (see `hprod`, `jprod`).  NumPy inputs use the host entry point; device tensors are enqueued on
        the handle's stream (`ctd_kktprod_dev_async`), followed by a sync when `sync`.  Whole-grid handles only: a shard handle
        calls `kktprod_shard`."""
        return self._mf("kktprod", False, (x, y, dx, dy, sx, sc), (float(obj_weight),), (None, None) if out is None else tuple(out), sync)

    def hdiag(self, x, y, obj_weight=1.0, out=None, sync=True):
        """The diagonal of the Hessian of the Lagrangian, (obj_weight d2 f + sum_i y_i d2 c_i)(x)_jj, without assembling it (nvar
        entries; `ctd_hdiag*`).  y = None: the objective only.  The structural Hessian, as for `hprod`.  NumPy inputs use the host
        entry point; device tensors are enqueued on the handle's stream, followed by a sync when `sync`."""
        return self._mf("hdiag", False, (x, y), (float(obj_weight),), (out,), sync)

    def jsq_rows(self, x, wx=None, out=None, sync=True):
        """diag(J diag(wx) J'): out_r = sum_j wx_j J_rj^2 without assembling J (ncon entries; `ctd_jsq_rows*`).  wx = None: ones,
        the squared row norms of J.  The structural Jacobian, as for `jprod`; inputs as for `hdiag`."""
        return self._mf("jsq_rows", False, (x, wx), (), (out,), sync)

    def jsq_cols(self, x, wc=None, out=None, sync=True):
        """diag(J' diag(wc) J): out_j = sum_r wc_r J_rj^2 without assembling J (nvar entries; `ctd_jsq_cols*`).  wc = None: ones,
        the squared column norms of J.  The structural Jacobian, as for `jprod`; inputs as for `hdiag`."""
        return self._mf("jsq_cols", False, (x, wc), (), (out,), sync)

    def kkt_diag_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, floor=1e-8):
        """The diagonal (scaling) preconditioner of the operator `kktprod`, K = [[H + Sx, J'], [J, -Sc]]: returns the pair
            px = max(|hdiag(x, y, obj_weight) + sx|, floor)        (nvar entries)
            pc = jsq_rows(x, 1 / px) + sc                          (ncon entries)
        i.e. the diagonal of the top block and the diagonal of the Schur complement J diag(px)^-1 J' + Sc taken with it.
        M = diag(1 / px, 1 / pc) is symmetric positive definite (given pc > 0: a nonzero row of J or sc_r > 0), which is what
        MINRES asks of a preconditioner.  Two engine calls plus element-wise operations, on the handle's stream for device tensors.

        WHEN IT HELPS: when the diagonals of K span orders of magnitude -- an interior-point step, whose barrier term
        sx = z / x does -- it removes that spread (Goddard, trapeze, N = 20, sx = 10^U(-3, 5): MINRES 1464 -> 120 iterations).
        WHEN IT DOES NOT: it is a scaling, not a constraint preconditioner: it does nothing for the coupling through J.  With
        multipliers of order 1 and sx of order 1e-2, where K's diagonal is already even, it does not reduce the iterations.
        It needs |H_jj + sx_j| away from zero: where that sum cancels, `floor` takes over and the scaling of that variable is
        arbitrary.  Block (per-node) and Riccati-type preconditioners are not provided."""
        if _is_tensor(x):
            import torch
            # the element-wise operations go to the handle's stream; where Python does not know it (stream="own") the two
            # streams are ordered by waiting instead
            known = self._stream_raw is not None
            if not known:
                st = torch.cuda.current_stream(x.device)
            elif self._stream_raw == 0:     # (the null stream: ExternalStream(0) is NOT it -- its cuda_stream is not 0)
                st = torch.cuda.default_stream(x.device)
            else:
                st = torch.cuda.ExternalStream(self._stream_raw, device=x.device)
            with torch.cuda.stream(st):
                px = self.hdiag(x, y, obj_weight, sync=not known)
                if sx is not None:
                    px += sx
                px = torch.clamp_min(torch.abs_(px), floor)
                w = torch.reciprocal(px)
                if not known:
                    st.synchronize()
                pc = self.jsq_rows(x, w, sync=not known)
                if sc is not None:
                    pc += sc
            st.synchronize()
            return px, pc
        px = self.hdiag(x, y, obj_weight)
        if sx is not None:
            px = px + np.asarray(sx, dtype=np.float64)
        px = np.maximum(np.abs(px), floor)
        pc = self.jsq_rows(x, 1.0 / px)
        if sc is not None:
            pc = pc + np.asarray(sc, dtype=np.float64)
        return px, pc

    # ---- chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*) -----------------------------------------------------------
    @staticmethod
    def _tensors_only(fn, **named):
        for nm, a in named.items():
            if a is not None and not _is_tensor(a):
                raise ValueError(f"{fn}: {nm} must be a device tensor on the handle's GPU; NumPy inputs are not accepted (the Schur "
                                 "preconditioner has no host path)")

    def _schur_solve(self, name, P, r, out, sync):
        """the solve of a family with the factor P: `ctd_<name>_dev_async` on (P.ws, r, out), out zeros when None"""
        self._tensors_only(name, r=r, out=out, ws=P.ws)
        ncon = self.dim_NLP_constraints
        if out is None:
            import torch
            out = torch.zeros(ncon, dtype=torch.float64, device=r.device)
            torch.cuda.current_stream(r.device).synchronize()
        self._ck(getattr(_lib.lib(), f"ctd_{name}_dev_async")(self._h, self._dev_ptr(P.ws, P.layout.workspace, "ws"), self._dev_ptr(r, ncon, "r"),
                                                             self._dev_ptr(out, ncon, "out")))
        if sync:
            self.sync()
        return out

    def _schur_info(self, name, P, *split):
        """the status query of a family: `ctd_<name>` on P.ws (split: n_ranks and rank where the entry point takes them)"""
        self._tensors_only(name, ws=P.ws)
        bad = C.c_int64(0)
        self._ck(getattr(_lib.lib(), "ctd_" + name)(self._h, self._dev_ptr(P.ws, P.layout.workspace, "ws"), *split, C.byref(bad)))
        return bad.value

    def kkt_schur_layout(self, chunk_steps=None):
        """`ctd_kkt_schur_layout`: N, block_rows (m), tail_rows, first_tail_row, tail_cols (nv), n_chunks, the effective chunk_steps
        and the workspace in doubles of the chunked block-tridiagonal Schur preconditioner; chunk_steps = None: one chunk.  Checks
        the handle's Jacobian pattern (rows sharing a non-tail column lie in the same or adjacent blocks).  Needs a CSR handle
        (value_order="csr") of the whole grid; works on host-only handles."""
        lay = _lib.ctd_schur_layout(struct_size=C.sizeof(_lib.ctd_schur_layout))
        self._ck(_lib.lib().ctd_kkt_schur_layout(self._h, int((1 << 62) if chunk_steps is None else chunk_steps), C.byref(lay)))
        return lay

    def kkt_schur_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, chunk_steps=None, floor=1e-8, jvals=None):
        """The chunked block-tridiagonal Schur preconditioner of the operator `kktprod`:
            M^-1 = blkdiag(diag(px), T_0, T_1, ..., diag(pc_tail)),   T_c = Jt_c diag(1 / px) Jt_c' + Sc_c
        with (px, pc) the pair of `kkt_diag_precond(x, y, obj_weight, sx, sc, floor)`, Jt the Jacobian without the nv tail columns
        and chunk c the constraint rows of chunk_steps consecutive time steps (None: one chunk, the whole grid); couplings between
        chunks are dropped.  Unlike the diagonal it sees the coupling of neighbouring steps through J, which is what the iteration
        count of MINRES on a collocation KKT system grows with.  jvals: the Jacobian values at x of this (CSR) handle, computed
        with `cons_jac` when None.  Runs the factor (`ctd_kkt_schur_factor_dev_async`, two launches) and returns a SchurPrecond
        (px, pc, ws, layout) for `kkt_minres(..., precond=P)`, `kkt_schur_solve` and `kkt_schur_info`.  Device tensors only."""
        self._tensors_only("kkt_schur_precond", x=x, y=y, sx=sx, sc=sc, jvals=jvals)
        import torch
        self._check_x(x)
        lay = self.kkt_schur_layout(chunk_steps)
        px, pc = self.kkt_diag_precond(x, y, obj_weight, sx, sc, floor)
        if jvals is None:
            _, jvals = self.cons_jac(x)
        ws = torch.empty(lay.workspace, dtype=torch.float64, device=x.device)
        return self.kkt_schur_factor(jvals, px, pc, sc, lay.chunk_steps, ws)

    def kkt_schur_factor(self, jvals, px, pc, sc, chunk_steps, ws):
        """`ctd_kkt_schur_factor_dev_async` on the caller's tensors (enqueue-only): the factor of T built from jvals, 1 / px and sc
        (None: zero) into ws (kkt_schur_layout(chunk_steps).workspace doubles).  Returns the SchurPrecond (px, pc, ws, layout)."""
        self._tensors_only("kkt_schur_factor", jvals=jvals, px=px, pc=pc, sc=sc, ws=ws)
        lay = self.kkt_schur_layout(chunk_steps)
        nvar, ncon = self.dim_NLP_variables, self.dim_NLP_constraints
        self._ck(_lib.lib().ctd_kkt_schur_factor_dev_async(
            self._h, self._dev_ptr(jvals, self.nnzj, "jvals"), self._dev_ptr(px, nvar, "px"), self._dev_ptr(sc, ncon, "sc"),
            int(lay.chunk_steps), self._dev_ptr(ws, lay.workspace, "ws")))
        self._dev_ptr(pc, ncon, "pc")
        return SchurPrecond(px, pc, ws, lay)

    def kkt_schur_solve(self, P, r, out=None, sync=True):
        """`ctd_kkt_schur_solve_dev_async`: out = blkdiag(T_c)^-1 r on the block rows (the first layout.first_tail_row entries); the
        tail rows of out are left untouched (zero in a tensor allocated here).  r, out: ncon entries, out must not be r."""
        return self._schur_solve("kkt_schur_solve", P, r, out, sync)

    def kkt_schur_info(self, P):
        """`ctd_kkt_schur_info`: waits for the handle's stream; -1 when every pivot of the factor was positive, otherwise the first
        block (time step) whose pivot was not positive or not finite -- the preconditioner is then unusable (MINRES: "breakdown")."""
        return self._schur_info("kkt_schur_info", P)

    # ---- log-depth exact block-tridiagonal Schur preconditioner (ctd_kkt_schur_cr*) --------------------------------------------------
    def kkt_schur_cr_layout(self):
        """`ctd_kkt_schur_cr_layout`: N, block_rows (m), tail_rows, first_tail_row, tail_cols (nv) as `kkt_schur_layout`, then
        n_levels = ceil(log2 N), factor_launches, solve_launches and the workspace in doubles of the log-depth exact
        block-tridiagonal Schur preconditioner.  The same checks and refusals; works on host-only handles."""
        lay = _lib.ctd_schur_cr_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_layout))
        self._ck(_lib.lib().ctd_kkt_schur_cr_layout(self._h, C.byref(lay)))
        return lay

    def kkt_schur_cr_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, floor=1e-8, jvals=None):
        """The exact block-tridiagonal Schur preconditioner of the operator `kktprod`:
            M^-1 = blkdiag(diag(px), T, diag(pc_tail)),   T = Jt diag(1 / px) Jt' + Sc
        the matrix of `kkt_schur_precond` with one chunk -- no coupling is dropped and there is no chunk length to choose --
        factored by block cyclic reduction: ceil(log2 N) levels of parallel block eliminations instead of a sweep over N blocks.
        Arguments as `kkt_schur_precond`.  Runs the factor (`ctd_kkt_schur_cr_factor_dev_async`) and returns a SchurCrPrecond
        (px, pc, ws, layout) for `kkt_minres(..., precond=P)`, `kkt_schur_cr_solve` and `kkt_schur_cr_info`.  Device tensors only."""
        self._tensors_only("kkt_schur_cr_precond", x=x, y=y, sx=sx, sc=sc, jvals=jvals)
        import torch
        self._check_x(x)
        lay = self.kkt_schur_cr_layout()
        px, pc = self.kkt_diag_precond(x, y, obj_weight, sx, sc, floor)
        if jvals is None:
            _, jvals = self.cons_jac(x)
        ws = torch.empty(lay.workspace, dtype=torch.float64, device=x.device)
        return self.kkt_schur_cr_factor(jvals, px, pc, sc, ws)

    def kkt_schur_cr_factor(self, jvals, px, pc, sc, ws):
        """`ctd_kkt_schur_cr_factor_dev_async` on the caller's tensors (enqueue-only): the factor of T built from jvals, 1 / px and
        sc (None: zero) into ws (kkt_schur_cr_layout().workspace doubles).  Returns the SchurCrPrecond (px, pc, ws, layout)."""
        self._tensors_only("kkt_schur_cr_factor", jvals=jvals, px=px, pc=pc, sc=sc, ws=ws)
        lay = self.kkt_schur_cr_layout()
        nvar, ncon = self.dim_NLP_variables, self.dim_NLP_constraints
        self._ck(_lib.lib().ctd_kkt_schur_cr_factor_dev_async(
            self._h, self._dev_ptr(jvals, self.nnzj, "jvals"), self._dev_ptr(px, nvar, "px"), self._dev_ptr(sc, ncon, "sc"),
            self._dev_ptr(ws, lay.workspace, "ws")))
        self._dev_ptr(pc, ncon, "pc")
        return SchurCrPrecond(px, pc, ws, lay)

    def kkt_schur_cr_solve(self, P, r, out=None, sync=True):
        """`ctd_kkt_schur_cr_solve_dev_async`: out = T^-1 r on the block rows (the first layout.first_tail_row entries); the tail
        rows of out are left untouched (zero in a tensor allocated here).  r, out: ncon entries, out must not be r; the scratch
        region of P.ws is written."""
        return self._schur_solve("kkt_schur_cr_solve", P, r, out, sync)

    def kkt_schur_cr_info(self, P):
        """`ctd_kkt_schur_cr_info`: waits for the handle's stream; -1 when every pivot of the factor was positive, otherwise the
        smallest block (time step) with a pivot that was not positive or not finite (MINRES: "breakdown")."""
        return self._schur_info("kkt_schur_cr_info", P)

    # ---- the shard form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_shard_*) ---------------------------------------------
    def kkt_schur_cr_shard_layout(self):
        """`ctd_kkt_schur_cr_shard_layout`: the handle's steps [step_begin, step_end) as the n_blocks blocks of T_r -- the principal
        submatrix of T of `kkt_schur_cr_precond` on those blocks --, first_row, n_levels = ceil(log2 n_blocks), the launch counts,
        the workspace in doubles, and the read set of the factor: jvals on [jvals_begin, jvals_end), px on [px_begin, px_end).  The
        tail fields are the grid's.  Every handle is accepted (a whole-grid handle is the single shard); works on host-only
        handles."""
        if self._schur_cr_shard_layout is None:     # (the read set is a walk of the rank's rows on the host: once per handle,
            lay = _lib.ctd_schur_cr_shard_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_shard_layout))      # whose steps never change)
            self._ck(_lib.lib().ctd_kkt_schur_cr_shard_layout(self._h, C.byref(lay)))
            self._schur_cr_shard_layout = lay
        return _lib.ctd_schur_cr_shard_layout.from_buffer_copy(self._schur_cr_shard_layout)      # (a copy: the caller's to keep)

    def kkt_schur_cr_shard_factor(self, jvals, px, pc, sc, ws=None):
        """`ctd_kkt_schur_cr_shard_factor_dev_async` (enqueue-only): the factor of T_r from jvals, 1 / px and sc (None: zero), read on
        the ranges the layout names, into ws (layout.workspace doubles, allocated when None).  All buffers are full-length with
        global indexing.  Returns the SchurCrShardPrecond (px, pc, ws, layout) for `kkt_schur_cr_shard_solve`, `_info` and the
        sharded solves (`dist.kkt_minres_shards`, `ShardedDOCP.kkt_minres`)."""
        self._tensors_only("kkt_schur_cr_shard_factor", jvals=jvals, px=px, pc=pc, sc=sc, ws=ws)
        lay = self.kkt_schur_cr_shard_layout()
        nvar, ncon = self.dim_NLP_variables, self.dim_NLP_constraints
        if ws is None:
            import torch
            ws = torch.empty(lay.workspace, dtype=torch.float64, device=px.device)
        self._dev_ptr(pc, ncon, "pc")           # (not the factor's, but the solve's that will carry it: checked before anything is enqueued)
        self._ck(_lib.lib().ctd_kkt_schur_cr_shard_factor_dev_async(
            self._h, self._dev_ptr(jvals, self.nnzj, "jvals"), self._dev_ptr(px, nvar, "px"), self._dev_ptr(sc, ncon, "sc"),
            self._dev_ptr(ws, lay.workspace, "ws")))
        return SchurCrShardPrecond(px, pc, ws, lay)

    def kkt_schur_cr_shard_solve(self, P, r, out=None, sync=True):
        """`ctd_kkt_schur_cr_shard_solve_dev_async`: out = T_r^-1 r on the handle's block rows [first_row, first_row + n_blocks
        block_rows); nothing else of out is written (zero in a tensor allocated here).  r, out: ncon entries, out must not be r."""
        return self._schur_solve("kkt_schur_cr_shard_solve", P, r, out, sync)

    def kkt_schur_cr_shard_info(self, P):
        """`ctd_kkt_schur_cr_shard_info`: waits for the handle's stream; -1 when every pivot of the factor was positive, otherwise
        the smallest GLOBAL block (time step) of the handle's range with a pivot that was not positive or not finite."""
        return self._schur_info("kkt_schur_cr_shard_info", P)

    # ---- the joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*): the couplings across the ranks restored ----
    def kkt_schur_cr_joint_layout(self, n_ranks, rank):
        """`ctd_kkt_schur_cr_joint_layout`: the handle's steps as rank `rank` of n_ranks -- the separator (its first block; -1 on rank 0),
        the interior [int_begin, step_end) of n_int blocks, the launch counts of the four phases, the record slots, the offsets into
        the workspace (doubles) and the read set of the factor: that of the shard form and the halo of jvals, [jvals_halo_begin,
        jvals_halo_end).  Works on host-only handles."""
        lay = _lib.ctd_schur_cr_joint_layout(struct_size=C.sizeof(_lib.ctd_schur_cr_joint_layout))
        self._ck(_lib.lib().ctd_kkt_schur_cr_joint_layout(self._h, int(n_ranks), int(rank), C.byref(lay)))
        return lay

    def kkt_schur_cr_joint_factor_local(self, jvals, px, pc, sc, n_ranks, rank, ws=None, send=None, xsend=None):
        """`ctd_kkt_schur_cr_joint_factor_local_dev_async`: the interface blocks, the factor of the interior, the spikes and the
        factor record, written into send (layout.factor_slot doubles).  The caller gathers the records of all ranks in rank order
        and hands them to `kkt_schur_cr_joint_factor_join`.  Returns the SchurCrJointPrecond (px, pc, ws, layout, send, xsend);
        xsend (layout.solve_slot doubles) is where `kkt_schur_cr_joint_solve_local` puts the solve record.  ws, send and xsend are
        allocated when None; with all three given (send and xsend may stay None with one rank, which has no record) the call
        allocates nothing and waits for nothing: enqueue-only, like the C entry point."""
        self._tensors_only("kkt_schur_cr_joint_factor_local", jvals=jvals, px=px, pc=pc, sc=sc, ws=ws, send=send, xsend=xsend)
        lay = self.kkt_schur_cr_joint_layout(n_ranks, rank)
        nvar, ncon = self.dim_NLP_variables, self.dim_NLP_constraints
        fresh = ws is None or (lay.n_ranks > 1 and (send is None or xsend is None))
        if fresh:
            import torch
            if ws is None:
                ws = torch.empty(lay.workspace, dtype=torch.float64, device=px.device)
            if lay.n_ranks > 1:
                send = torch.zeros(lay.factor_slot, dtype=torch.float64, device=px.device) if send is None else send
                xsend = torch.zeros(lay.solve_slot, dtype=torch.float64, device=px.device) if xsend is None else xsend
            torch.cuda.current_stream(px.device).synchronize()       # (the zeros are there before the handle's stream writes)
        self._dev_ptr(pc, ncon, "pc")
        self._ck(_lib.lib().ctd_kkt_schur_cr_joint_factor_local_dev_async(
            self._h, self._dev_ptr(jvals, self.nnzj, "jvals"), self._dev_ptr(px, nvar, "px"), self._dev_ptr(sc, ncon, "sc"),
            self._dev_ptr(ws, lay.workspace, "ws"), self._dev_ptr(send, lay.factor_slot, "send"), int(n_ranks), int(rank)))
        return SchurCrJointPrecond(px, pc, ws, lay, send, xsend)

    def kkt_schur_cr_joint_factor_join(self, P, gathered):
        """`ctd_kkt_schur_cr_joint_factor_join_dev_async`: the reduced matrix from the n_ranks gathered records (rank order,
        layout.factor_slot doubles apart) and its factor, into P's workspace.  Nothing is launched with one rank (gathered may be None)."""
        self._tensors_only("kkt_schur_cr_joint_factor_join", ws=P.ws, gathered=gathered)
        lay = P.layout
        self._ck(_lib.lib().ctd_kkt_schur_cr_joint_factor_join_dev_async(
            self._h, self._dev_ptr(P.ws, lay.workspace, "ws"), self._dev_ptr(gathered, lay.n_ranks * lay.factor_slot, "gathered"),
            lay.n_ranks, lay.rank))

    def kkt_schur_cr_joint_solve_local(self, P, r, out, send=None):
        """`ctd_kkt_schur_cr_joint_solve_local_dev_async`: out = A^-1 r on the rank's interior rows and the solve record into send
        (P.xsend when None; layout.solve_slot doubles).  r, out: ncon entries, out must not be r.  Returns send."""
        self._tensors_only("kkt_schur_cr_joint_solve_local", r=r, out=out, ws=P.ws, send=send)
        lay, ncon = P.layout, self.dim_NLP_constraints
        send = P.xsend if send is None else send
        self._ck(_lib.lib().ctd_kkt_schur_cr_joint_solve_local_dev_async(
            self._h, self._dev_ptr(P.ws, lay.workspace, "ws"), self._dev_ptr(r, ncon, "r"), self._dev_ptr(out, ncon, "out"),
            self._dev_ptr(send, lay.solve_slot, "send"), lay.n_ranks, lay.rank))
        return send

    def kkt_schur_cr_joint_solve_join(self, P, gathered, out, sync=True):
        """`ctd_kkt_schur_cr_joint_solve_join_dev_async`: the reduced solve from the n_ranks gathered solve records, then out = T^-1 r
        on the rank's block rows (the separator's rows and the correction of the interior rows `kkt_schur_cr_joint_solve_local`
        left in out).  Nothing else of out is written; nothing is launched with one rank."""
        self._tensors_only("kkt_schur_cr_joint_solve_join", out=out, ws=P.ws, gathered=gathered)
        lay = P.layout
        self._ck(_lib.lib().ctd_kkt_schur_cr_joint_solve_join_dev_async(
            self._h, self._dev_ptr(P.ws, lay.workspace, "ws"), self._dev_ptr(gathered, lay.n_ranks * lay.solve_slot, "gathered"),
            self._dev_ptr(out, self.dim_NLP_constraints, "out"), lay.n_ranks, lay.rank))
        if sync:
            self.sync()
        return out

    def kkt_schur_cr_joint_info(self, P):
        """`ctd_kkt_schur_cr_joint_info`: waits for the handle's stream; -1 when every pivot was positive, otherwise the smallest GLOBAL
        block with a recorded pivot among the rank's interior and the separators of the reduced factor."""
        return self._schur_info("kkt_schur_cr_joint_info", P, P.layout.n_ranks, P.layout.rank)

    # ---- device-resident preconditioned MINRES solve of K z = rhs (ctd_kkt_minres*) ---------------------------------------------
    def _kkt_system(self, fn, vecs, obj_weight, host_ok):
        """The ctd_kkt_system of a solve and the pointers of its other vectors.  vecs: (name, array, layout, required) rows, x
        first -- layout "v": nvar, "c": ncon, "k": nvar + ncon entries --; those named x, y, sx, sc, px, pc fill the struct.  Every
        length is checked by name, as DOCP._mf does.  Returns (dev, sys, pointers of the rows by name, arrays to keep alive)."""
        size = {"v": self.dim_NLP_variables, "c": self.dim_NLP_constraints, "k": self.dim_NLP_variables + self.dim_NLP_constraints}
        for nm, a, _, required in vecs:
            if required and a is None:
                raise ValueError(f"{nm} is required")
        dev = hasattr(vecs[0][1], "is_cuda")
        self._check_x(vecs[0][1])
        by = {nm: a for nm, a, _, _ in vecs}
        if (by.get("px") is None) != (by.get("pc") is None):
            raise ValueError("px and pc are given both (M = diag(1 / px, 1 / pc)) or neither")
        ptrs, keep = {}, []
        for nm, a, lay, _ in vecs:          # every kind and length first, by name
            if a is None:
                continue
            n = size[lay]
            if dev and not hasattr(a, "is_cuda"):
                raise TypeError(f"{nm} must be a device tensor like x")
            if not dev and not host_ok:
                raise TypeError(f"{nm} must be a device tensor: {fn} has no host path")
            if not dev and nm == "out":
                _host_out(a, n, nm)
            elif (a.numel() if dev else np.size(a)) != n:
                raise ValueError(f"{nm} has {a.numel() if dev else np.size(a)} entries, expected {n}")
        for nm, a, lay, _ in vecs:
            if a is None:
                ptrs[nm] = None
            elif dev:
                ptrs[nm] = self._dev_ptr(a, size[lay], nm)
            else:
                a = a if nm == "out" else np.ascontiguousarray(a, dtype=np.float64)
                keep.append(a)
                ptrs[nm] = C.c_void_p(a.ctypes.data)
        sys = _lib.ctd_kkt_system(struct_size=C.sizeof(_lib.ctd_kkt_system), obj_weight=float(obj_weight))
        for nm in ("x", "y", "sx", "sc", "px", "pc"):
            q = ptrs.get(nm)
            setattr(sys, nm, q.value if q is not None else None)
        return dev, sys, ptrs, keep

    @staticmethod
    def _minres_info(info):
        return MinresInfo(_lib.MINRES_STATUS[info.status], int(info.iterations), info.phibar, info.Anorm, info.ynorm, info.beta1)

    def kkt_minres(self, x, y, rhs, obj_weight=1.0, sx=None, sc=None, precond=None, rtol=1e-10, max_iter=None, check_every=16,
                   out=None):
        """Preconditioned MINRES on K z = rhs, K = [[H + Sx, J'], [J, -Sc]] the operator of `kktprod` at (x, y, obj_weight, sx, sc),
        entirely on the device (`ctd_kkt_minres*`): per iteration the two launches of `kktprod` and three vector kernels, the
        scalar recurrences and the stopping tests included; the host reads the status once per `check_every` iterations.  rhs
        and z have nvar + ncon entries, z0 = 0.  The recurrences and the stopping tests (rtol) are those of
        scipy.sparse.linalg.minres, so iteration counts are comparable with it.
        precond: None; a pair (px, pc), M = diag(1 / px, 1 / pc), which must be positive; "diag": the pair of
        `kkt_diag_precond(x, y, obj_weight, sx, sc)`; a SchurPrecond P of `kkt_schur_precond` (device tensors only:
        `ctd_kkt_minres_schur_dev`, one more launch per iteration); or "schur": that of `kkt_schur_precond(x, y, obj_weight, sx,
        sc)`, one chunk; a SchurCrPrecond of `kkt_schur_cr_precond` (`ctd_kkt_minres_schur_cr_dev`) or "schur_cr": the same matrix,
        factored and applied in ceil(log2 N) levels.  max_iter: default 5 (nvar + ncon), scipy's.
        Returns (z, info), info a MinresInfo: status "converged", "max_iter" or "breakdown" (M not positive definite, a NaN, or
        the Krylov space exhausted), the iterations done, phibar, Anorm, ynorm, beta1.  Iterations enqueued after the status was
        set change nothing: z does not depend on check_every.  Results are reproducible bit for bit.  NumPy inputs use the host
        entry point; device tensors the device one (`out`: z).  Whole-grid handles only."""
        L = _lib.lib()
        n = self.dim_NLP_variables + self.dim_NLP_constraints
        if x is None or rhs is None:
            raise ValueError(("x" if x is None else "rhs") + " is required")
        schur = None
        if isinstance(precond, str):
            if precond not in ("diag", "schur", "schur_cr"):
                raise ValueError(f'precond is None, a pair (px, pc), a SchurPrecond, a SchurCrPrecond, "diag", "schur" or "schur_cr", not {precond!r}')
            self._check_x(x)
            if precond == "schur":
                precond = self.kkt_schur_precond(x, y, obj_weight, sx, sc)
            elif precond == "schur_cr":
                precond = self.kkt_schur_cr_precond(x, y, obj_weight, sx, sc)
            else:
                px, pc = self.kkt_diag_precond(x, y, obj_weight, sx, sc)
        if isinstance(precond, (SchurPrecond, SchurCrPrecond)):
            self._tensors_only("kkt_minres with a Schur preconditioner", x=x, y=y, rhs=rhs, sx=sx, sc=sc, out=out)
            schur, px, pc = precond, precond.px, precond.pc
        elif not isinstance(precond, str):
            px, pc = (None, None) if precond is None else precond
        dev = hasattr(x, "is_cuda")
        if out is None:
            if dev:
                import torch
                out = torch.empty(n, dtype=torch.float64, device=x.device)
            else:
                out = np.empty(n)
        rows = (("x", x, "v", True), ("y", y, "c", False), ("rhs", rhs, "k", True), ("sx", sx, "v", False), ("sc", sc, "c", False),
                ("px", px, "v", False), ("pc", pc, "c", False), ("out", out, "k", True))
        dev, sys, p, keep = self._kkt_system("kkt_minres", rows, obj_weight, True)
        info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
        if schur is not None:
            drive = L.ctd_kkt_minres_schur_cr_dev if isinstance(schur, SchurCrPrecond) else L.ctd_kkt_minres_schur_dev
            self._ck(drive(self._h, C.byref(sys), self._dev_ptr(schur.ws, schur.layout.workspace, "ws"), p["rhs"],
                           p["out"], float(rtol), int(5 * n if max_iter is None else max_iter), int(check_every), C.byref(info)))
            return out, self._minres_info(info)
        fn = L.ctd_kkt_minres_dev if dev else L.ctd_kkt_minres
        rhs_p, out_p = (p["rhs"], p["out"]) if dev else (C.cast(p["rhs"], C.POINTER(C.c_double)), C.cast(p["out"], C.POINTER(C.c_double)))
        self._ck(fn(self._h, C.byref(sys), rhs_p, out_p, float(rtol), int(5 * n if max_iter is None else max_iter), int(check_every),
                    C.byref(info)))
        return out, self._minres_info(info)

    def kkt_minres_start(self, x, y, rhs, z, obj_weight=1.0, sx=None, sc=None, precond=None, rtol=1e-10):
        """`ctd_kkt_minres_start_dev_async`: enqueues the initialisation of a solve on the device tensors (z = 0, the state) on the
        handle's stream; precond: None or a pair (px, pc), read now only, or a SchurPrecond
        or SchurCrPrecond (`ctd_kkt_minres_schur_start_dev_async`, `ctd_kkt_minres_schur_cr_start_dev_async`: its workspace is
        used by every iteration).  No iteration cap.  See `kkt_minres`."""
        schur = precond if isinstance(precond, (SchurPrecond, SchurCrPrecond)) else None
        px, pc = (None, None) if precond is None else ((precond.px, precond.pc) if schur else precond)
        rows = (("x", x, "v", True), ("y", y, "c", False), ("rhs", rhs, "k", True), ("z", z, "k", True), ("sx", sx, "v", False),
                ("sc", sc, "c", False), ("px", px, "v", False), ("pc", pc, "c", False))
        _, sys, p, _ = self._kkt_system("kkt_minres_start", rows, obj_weight, False)
        if schur:
            start = (_lib.lib().ctd_kkt_minres_schur_cr_start_dev_async if isinstance(schur, SchurCrPrecond)
                     else _lib.lib().ctd_kkt_minres_schur_start_dev_async)
            self._ck(start(
                self._h, C.byref(sys), self._dev_ptr(schur.ws, schur.layout.workspace, "ws"), p["rhs"], p["z"], float(rtol)))
            return
        self._ck(_lib.lib().ctd_kkt_minres_start_dev_async(self._h, C.byref(sys), p["rhs"], p["z"], float(rtol)))

    def kkt_minres_iters(self, x, y, z, k, obj_weight=1.0, sx=None, sc=None):
        """`ctd_kkt_minres_iters_dev_async`: enqueues k iterations of the solve started last, on the same z and the same operator;
        they change nothing once the status is set.  Enqueue-only on the handle's stream."""
        rows = (("x", x, "v", True), ("y", y, "c", False), ("z", z, "k", True), ("sx", sx, "v", False), ("sc", sc, "c", False))
        _, sys, p, _ = self._kkt_system("kkt_minres_iters", rows, obj_weight, False)
        self._ck(_lib.lib().ctd_kkt_minres_iters_dev_async(self._h, C.byref(sys), p["z"], int(k)))

    def kkt_minres_info(self):
        """`ctd_kkt_minres_info`: waits for the handle's stream and returns the MinresInfo of the solve started last."""
        info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
        self._ck(_lib.lib().ctd_kkt_minres_info(self._h, C.byref(info)))
        return self._minres_info(info)

    # ---- the solve on a shard of the grid: the phases between the caller's all-gathers.  One implementation (_phase_*) for the
    # three families of _PHASE_FAMILIES; the public methods below name the family -------------------------------------------------
    def _phase_layout(self, fam, n_ranks, rank=None):
        lay = _lib.ctd_minres_shard_layout(struct_size=C.sizeof(_lib.ctd_minres_shard_layout))
        split = (int(n_ranks), int(rank)) if fam.layout_rank else (int(n_ranks),)
        self._ck(getattr(_lib.lib(), fam.prefix + "layout")(self._h, *split, C.byref(lay)))
        return lay

    def _phase_workspace(self, fam, n_ranks, rank=None, ws=None):
        import torch
        lay = self._phase_layout(fam, n_ranks, rank)
        if ws is None:
            ws = torch.zeros(lay.workspace, dtype=torch.float64, device=torch.device("cuda", self.device))
        self._dev_ptr(ws, lay.workspace, "ws")
        nvar, n, slot, G = self.dim_NLP_variables, lay.n, lay.slot, int(n_ranks)
        cut = lambda off, k: ws[off:off + k]        # noqa: E731
        return MinresShardWorkspace(ws, lay, G, cut(lay.off_v, nvar), cut(lay.off_v + nvar, n - nvar), cut(lay.off_kv, nvar),
                                    cut(lay.off_kv + nvar, n - nvar), cut(lay.off_send_a, slot), cut(lay.off_send_b, slot),
                                    cut(lay.off_gathered_a, G * slot), cut(lay.off_gathered_b, G * slot))

    def _phase_ws_ptr(self, fam, w):
        """the workspace's pointer: the C side lays the pointer out with the family's slot length and cannot know the tensor's, so a
        workspace cut for another family never reaches a kernel"""
        if w.layout.slot != fam.slot:
            raise ValueError(f"the workspace was cut with slots of {w.layout.slot} doubles, this phase family needs {fam.slot}: take it from "
                             "the family's own kkt_minres_*_workspace")
        return self._dev_ptr(w.ws, w.layout.workspace, "ws")

    def _phase_schur(self, fam, phase, precond):
        """the factor's workspace as the leading argument of the phases of the family that take it"""
        return (self._dev_ptr(precond.ws, precond.layout.workspace, "schur_ws"),) if phase in fam.schur else ()

    def _phase_start(self, fam, precond, rhs, z, w, rank, rtol=1e-10, max_iter=None):
        """precond: the family's preconditioner; the diagonal form's: None or a pair (px, pc)"""
        nvar, ncon = self.dim_NLP_variables, self.dim_NLP_constraints
        px, pc = (None, None) if precond is None else ((precond.px, precond.pc) if fam.precond else precond)
        if (px is None) != (pc is None):
            raise ValueError("px and pc are given both (M = diag(1 / px, 1 / pc)) or neither")
        for nm, a in (("rhs", rhs), ("z", z)):
            if a is None:
                raise ValueError(f"{nm} is required")
        sys = _lib.ctd_kkt_system(struct_size=C.sizeof(_lib.ctd_kkt_system), obj_weight=1.0)
        if px is not None:
            sys.px, sys.pc = self._dev_ptr(px, nvar, "px").value, self._dev_ptr(pc, ncon, "pc").value
        self._ck(getattr(_lib.lib(), fam.prefix + "start_dev_async")(
            self._h, C.byref(sys), *self._phase_schur(fam, "start", precond), self._dev_ptr(rhs, nvar + ncon, "rhs"),
            self._dev_ptr(z, nvar + ncon, "z"), self._phase_ws_ptr(fam, w), w.n_ranks, int(rank), float(rtol),
            int(5 * (nvar + ncon) if max_iter is None else max_iter)))

    def _phase(self, fam, phase, precond, z, w, rank):
        """begin (which has no z), alfa, lanczos, update"""
        zp = () if phase == "begin" else (self._dev_ptr(z, w.layout.n, "z"),)
        self._ck(getattr(_lib.lib(), f"{fam.prefix}{phase}_dev_async")(
            self._h, *self._phase_schur(fam, phase, precond), *zp, self._phase_ws_ptr(fam, w), w.n_ranks, int(rank)))

    def _phase_info(self, fam, w):
        info = _lib.ctd_minres_info(struct_size=C.sizeof(_lib.ctd_minres_info))
        self._ck(getattr(_lib.lib(), fam.prefix + "info")(self._h, self._phase_ws_ptr(fam, w), w.n_ranks, C.byref(info)))
        return self._minres_info(info)

    # the diagonal form (ctd_kkt_minres_shard_*)
    def kkt_minres_shard_layout(self, n_ranks):
        """`ctd_kkt_minres_shard_layout`: what this handle's shard owns of a Krylov vector (var_*, tail_*, row_*: index ranges of an
        (nvar + ncon)-vector; n_own, n_dot), the launch geometry (nwg, chunk) and the offsets of the workspace, for a split of the
        grid into n_ranks blocks.  Needs no device."""
        return self._phase_layout(_PLAIN, n_ranks)

    def kkt_minres_shard_workspace(self, n_ranks, ws=None):
        """The caller-owned workspace of one sharded solve on this handle's GPU (`ws`: the caller's tensor of
        kkt_minres_shard_layout(n_ranks).workspace doubles, allocated when None): a MinresShardWorkspace with the tensor `ws` and
        named views of it -- v_x, v_c (the Lanczos vector the operator is applied to), kv_x, kv_c (where `kktprod_shard` puts K v),
        send_a, send_b (this rank's slots) and gathered_a, gathered_b (n_ranks slots each, rank-major: what the all-gathers
        fill; with one rank they are the send slots)."""
        return self._phase_workspace(_PLAIN, n_ranks, ws=ws)

    def kkt_minres_shard_start(self, rhs, z, w, rank, precond=None, rtol=1e-10, max_iter=None):
        """`ctd_kkt_minres_shard_start_dev_async` on the workspace w: z = 0 and the vectors on the owned entries, the partial sums
        of beta1^2 into w.send_a.  precond: None or a pair (px, pc), read now only.  max_iter: default 5 (nvar + ncon)."""
        self._phase_start(_PLAIN, precond, rhs, z, w, rank, rtol, max_iter)

    def kkt_minres_shard_begin(self, w, rank):
        """`ctd_kkt_minres_shard_begin_dev_async`: beta1 from w.gathered_a, the first Lanczos vector, the state."""
        self._phase(_PLAIN, "begin", None, None, w, rank)

    def kkt_minres_shard_alfa(self, z, w, rank):
        """`ctd_kkt_minres_shard_alfa_dev_async`: phase (A), after `kktprod_shard` wrote K v into (w.kv_x, w.kv_c)."""
        self._phase(_PLAIN, "alfa", None, z, w, rank)

    def kkt_minres_shard_lanczos(self, z, w, rank):
        """`ctd_kkt_minres_shard_lanczos_dev_async`: phase (B), after w.gathered_a was filled."""
        self._phase(_PLAIN, "lanczos", None, z, w, rank)

    def kkt_minres_shard_update(self, z, w, rank):
        """`ctd_kkt_minres_shard_update_dev_async`: phase (C), after w.gathered_b was filled."""
        self._phase(_PLAIN, "update", None, z, w, rank)

    def kkt_minres_shard_info(self, w):
        """`ctd_kkt_minres_shard_info`: waits for the handle's stream and returns the MinresInfo in the workspace's state."""
        return self._phase_info(_PLAIN, w)

    # ... with the shard form of the log-depth Schur preconditioner (ctd_kkt_minres_schur_cr_shard_*): the same phases on larger
    # slots; P is the SchurCrShardPrecond of this handle
    def kkt_minres_schur_shard_layout(self, n_ranks):
        """`ctd_kkt_minres_schur_cr_shard_layout`: `kkt_minres_shard_layout` with slots of CTD_KKT_MINRES_SCHUR_SHARD_SLOT doubles."""
        return self._phase_layout(_SCHUR_SHARD, n_ranks)

    def kkt_minres_schur_shard_workspace(self, n_ranks, ws=None):
        """`kkt_minres_shard_workspace` for the solve with a SchurCrShardPrecond: the same views, cut with the larger slots."""
        return self._phase_workspace(_SCHUR_SHARD, n_ranks, ws=ws)

    def kkt_minres_schur_shard_start(self, P, rhs, z, w, rank, rtol=1e-10, max_iter=None):
        """`ctd_kkt_minres_schur_cr_shard_start_dev_async`: the start of `kkt_minres_shard_start` with M of P; the partial sums of
        beta1^2 -- the solve's behind the init kernel's -- go into w.send_a."""
        self._phase_start(_SCHUR_SHARD, P, rhs, z, w, rank, rtol, max_iter)

    def kkt_minres_schur_shard_begin(self, w, rank):
        """`ctd_kkt_minres_schur_cr_shard_begin_dev_async`"""
        self._phase(_SCHUR_SHARD, "begin", None, None, w, rank)

    def kkt_minres_schur_shard_alfa(self, z, w, rank):
        """`ctd_kkt_minres_schur_cr_shard_alfa_dev_async`: phase (A)"""
        self._phase(_SCHUR_SHARD, "alfa", None, z, w, rank)

    def kkt_minres_schur_shard_lanczos(self, P, z, w, rank):
        """`ctd_kkt_minres_schur_cr_shard_lanczos_dev_async`: phase (B), the solve with P's factor on the handle's block rows, and
        its partial sums into w.send_b"""
        self._phase(_SCHUR_SHARD, "lanczos", P, z, w, rank)

    def kkt_minres_schur_shard_update(self, z, w, rank):
        """`ctd_kkt_minres_schur_cr_shard_update_dev_async`: phase (C)"""
        self._phase(_SCHUR_SHARD, "update", None, z, w, rank)

    def kkt_minres_schur_shard_info(self, w):
        """`ctd_kkt_minres_schur_cr_shard_info`"""
        return self._phase_info(_SCHUR_SHARD, w)

    # ... with the joined form (ctd_kkt_minres_schur_cr_joint_*): the same phases on slots that also carry the solve records; P is the
    # SchurCrJointPrecond of this handle, joined (kkt_schur_cr_joint_factor_join)
    def kkt_minres_schur_joint_layout(self, n_ranks, rank):
        """`ctd_kkt_minres_schur_cr_joint_layout`: `kkt_minres_shard_layout` with slots of CTD_KKT_MINRES_SCHUR_JOINT_SLOT doubles."""
        return self._phase_layout(_SCHUR_JOINT, n_ranks, rank)

    def kkt_minres_schur_joint_workspace(self, n_ranks, rank, ws=None):
        """`kkt_minres_shard_workspace` for the solve with a SchurCrJointPrecond: the same views, cut with the larger slots."""
        return self._phase_workspace(_SCHUR_JOINT, n_ranks, rank, ws)

    def kkt_minres_schur_joint_start(self, P, rhs, z, w, rank, rtol=1e-10, max_iter=None):
        """`ctd_kkt_minres_schur_cr_joint_start_dev_async`: the start with M of P; the partial sums of beta1^2 and the rank's solve
        record go into w.send_a."""
        self._phase_start(_SCHUR_JOINT, P, rhs, z, w, rank, rtol, max_iter)

    def kkt_minres_schur_joint_begin(self, P, w, rank):
        """`ctd_kkt_minres_schur_cr_joint_begin_dev_async`: the two join launches, then beta1 and the first Lanczos vector"""
        self._phase(_SCHUR_JOINT, "begin", P, None, w, rank)

    def kkt_minres_schur_joint_alfa(self, z, w, rank):
        """`ctd_kkt_minres_schur_cr_joint_alfa_dev_async`: phase (A)"""
        self._phase(_SCHUR_JOINT, "alfa", None, z, w, rank)

    def kkt_minres_schur_joint_lanczos(self, P, z, w, rank):
        """`ctd_kkt_minres_schur_cr_joint_lanczos_dev_async`: phase (B), the interior's solve, its partial sums and the solve record
        into w.send_b"""
        self._phase(_SCHUR_JOINT, "lanczos", P, z, w, rank)

    def kkt_minres_schur_joint_update(self, P, z, w, rank):
        """`ctd_kkt_minres_schur_cr_joint_update_dev_async`: the two join launches, then phase (C)"""
        self._phase(_SCHUR_JOINT, "update", P, z, w, rank)

    def kkt_minres_schur_joint_info(self, w):
        """`ctd_kkt_minres_schur_cr_joint_info`"""
        return self._phase_info(_SCHUR_JOINT, w)

    def grad_shard(self, x, g, sync=False):
        """`ctd_grad_shard_dev_async`: the gradient entries of THIS shard's own variables into the full-length device tensor g
        (+ the shard's partial sums of d/dv in the nv tail entries), from a sharded iterate read in place -- no all-gathered x."""
        self._check_x(x)
        self._ck(_lib.lib().ctd_grad_shard_dev_async(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                                     self._dev_ptr(g, self.dim_NLP_variables, "g")))
        if sync:
            self.sync()
        return g

    def jprod_shard(self, x, v, out, sync=False):
        """`ctd_jprod_shard_dev_async`: THIS shard's rows of J(x) v -- the rows of its own steps; the last shard also the final path
        and boundary rows -- into the full-length device tensor `out`; nothing else of `out` is touched.  x is read through the
        table of `set_x_shards` when one is set, otherwise from x itself (halos copied in); v is always read from the tensor
        passed.  include/ctdirect_hip.h lists the entries read."""
        return self._mf("jprod", True, (x, v), (), (out,), sync)

    def jtprod_shard(self, x, w, out, sync=False):
        """`ctd_jtprod_shard_dev_async`: the entries of J(x)' w of THIS shard's own variables into the full-length device tensor
        `out`, + the shard's partial sums of d/dv in the nv tail entries (the caller adds them over the shards); see `jprod_shard`."""
        return self._mf("jtprod", True, (x, w), (), (out,), sync)

    def hprod_shard(self, x, y, v, obj_weight=1.0, out=None, sync=False):
        """`ctd_hprod_shard_dev_async`: the entries of (obj_weight d2 f + sum_i y_i d2 c_i)(x) v of THIS shard's own variables into
        the full-length device tensor `out` (allocated, uninitialised elsewhere, when None), + the shard's partial sums of d/dv in
        the nv tail entries.  y = None: objective only.  See `jprod_shard`."""
        return self._mf("hprod", True, (x, y, v), (float(obj_weight),), (out,), sync)

    def kktprod_shard(self, x, y, dx, dy, obj_weight=1.0, sx=None, sc=None, out=None, sync=False):
        """`ctd_kktprod_shard_dev_async`: `kktprod` on THIS shard, device tensors only.  Into the full-length pair `out` = (rx, rc)
        (allocated, uninitialised elsewhere, when None) go the entries of rx of the shard's own variables, + the shard's partial sums
        in the nv tail entries (the caller adds them over the shards; sx * dx of those entries is in the last shard's), and the
        shard's own rows of rc (the last shard: also the final path and boundary rows); nothing else is touched.  x is read through
        the table of `set_x_shards` when one is set, otherwise from x itself (halos copied in); y, dx, dy, sx and sc are always read
        from the tensors passed.  include/ctdirect_hip.h lists the entries read.  Returns (rx, rc)."""
        return self._mf("kktprod", True, (x, y, dx, dy, sx, sc), (float(obj_weight),), (None, None) if out is None else tuple(out), sync)

    def hdiag_shard(self, x, y, obj_weight=1.0, out=None, sync=False):
        """`ctd_hdiag_shard_dev_async`: `hdiag` on THIS shard, device tensors only.  Into the full-length `out` (allocated,
        uninitialised elsewhere, when None) go the entries of the shard's own variables, + the shard's partial sums in the nv tail
        entries (the caller adds them over the shards); nothing else is touched.  x is read through the table of `set_x_shards`
        when one is set, otherwise from x itself (halos copied in); y (None: objective only) is always read from the tensor passed:
        the constraint-layout read set of include/ctdirect_hip.h."""
        return self._mf("hdiag", True, (x, y), (float(obj_weight),), (out,), sync)

    def jsq_rows_shard(self, x, wx=None, out=None, sync=False):
        """`ctd_jsq_rows_shard_dev_async`: THIS shard's rows of `jsq_rows` -- the rows of its own steps; the last shard also the
        final path and boundary rows -- into the full-length `out`; every row sum is complete.  wx (None: ones) is read from the
        tensor passed: the variable-layout read set of include/ctdirect_hip.h.  See `hdiag_shard`."""
        return self._mf("jsq_rows", True, (x, wx), (), (out,), sync)

    def jsq_cols_shard(self, x, wc=None, out=None, sync=False):
        """`ctd_jsq_cols_shard_dev_async`: the entries of `jsq_cols` of THIS shard's own variables into the full-length `out`, + the
        shard's partial sums in the nv tail entries.  wc (None: ones) is read from the tensor passed: the constraint-layout read
        set of include/ctdirect_hip.h.  See `hdiag_shard`."""
        return self._mf("jsq_cols", True, (x, wc), (), (out,), sync)

    def eval_all(self, x, y=None, obj_weight=1.0, f=None, g=None, c=None, vals=None, hvals=None, sync=False):
        """One solver iteration in one call (`ctd_eval_all_dev_async`): objective -> f[0], gradient -> g, constraints -> c,
        Jacobian values -> vals, Hessian values of the Lagrangian -> hvals, for device tensors; outputs left None are skipped.
        The callbacks run side by side on the GPU."""
        self._check_x(x)
        P = lambda t, n, name: None if t is None else self._dev_ptr(t, n, name)      # noqa: E731
        self._ck(_lib.lib().ctd_eval_all_dev_async(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                                   P(y, self.dim_NLP_constraints, "y"), float(obj_weight), P(f, 1, "f"),
                                                   P(g, self.dim_NLP_variables, "g"), P(c, self.dim_NLP_constraints, "c"),
                                                   P(vals, self.nnzj, "vals"), P(hvals, self.nnzh, "hvals")))
        if sync:
            self.sync()

    # ---- batched callbacks: K iterates of this transcription per launch -----------------------------------------
    def _batch_rows(self, t, n, name, k=None):
        """A (K, n) float64 device tensor whose rows are contiguous (stride(1) == 1) on the handle's GPU, as (pointer, K, leading
        dimension = stride(0)): row slices of wider buffers are fine.  NumPy arrays are refused -- there is no host batch path."""
        if not _is_tensor(t):
            raise TypeError(f"{name}: the batched callbacks take a (K, {n}) torch device tensor, not {type(t).__name__} "
                            "(there is no host batch path)")
        import torch
        if not (t.is_cuda and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == n and t.shape[0] >= 1
                and (t.stride(1) == 1 or n == 1) and t.stride(0) >= n):
            raise ValueError(f"{name} must be a (K, {n}) float64 tensor on the handle's GPU with contiguous rows (stride(1) == 1), "
                             f"got shape {tuple(t.shape)}, strides {tuple(t.stride())}, dtype {t.dtype}")
        if t.device.index != self.device:
            raise ValueError(f"{name} lives on cuda:{t.device.index}, handle is bound to device {self.device}")
        if k is not None and t.shape[0] != k:
            raise ValueError(f"{name} has {t.shape[0]} rows, X has {k}")
        return C.c_void_p(t.data_ptr()), int(t.shape[0]), int(t.stride(0))

    def _batch_out(self, t, x, n, name, k):
        import torch
        if t is None:
            return torch.empty((k, n), dtype=torch.float64, device=x.device)
        self._batch_rows(t, n, name, k)
        return t

    def cons_jac_batch(self, X, C=None, V=None, sync=True):
        """cons! + jac_coord! at the K rows of X in ONE launch (`ctd_cons_jac_batch_dev_async`): row b of C / V equals
        cons_jac(X[b]) bit for bit.  X: (K, nvar) device tensor with contiguous rows; C (K, ncon), V (K, nnzj) are allocated when
        not given.  Returns (C, V)."""
        px, k, ldx = self._batch_rows(X, self.dim_NLP_variables, "X")
        C = self._batch_out(C, X, self.dim_NLP_constraints, "C", k)
        V = self._batch_out(V, X, self.nnzj, "V", k)
        self._ck(_lib.lib().ctd_cons_jac_batch_dev_async(self._h, k, px, ldx, C.data_ptr(), C.stride(0), V.data_ptr(), V.stride(0)))
        if sync:
            self.sync()
        return C, V

    def obj_batch(self, X, f=None, sync=True):
        """obj(nlp, x) at the K rows of X (`ctd_obj_batch_dev_async`): f[b] = obj(X[b]).  f: K contiguous doubles on the device
        (allocated when not given).  Returns f."""
        import torch
        px, k, ldx = self._batch_rows(X, self.dim_NLP_variables, "X")
        if f is None:
            f = torch.empty(k, dtype=torch.float64, device=X.device)
        elif not (_is_tensor(f) and f.is_cuda and f.dtype == torch.float64 and f.is_contiguous() and f.numel() == k
                  and f.device.index == self.device):
            raise ValueError(f"f must be a contiguous float64 tensor of {k} entries on the handle's GPU")
        self._ck(_lib.lib().ctd_obj_batch_dev_async(self._h, k, px, ldx, C.c_void_p(f.data_ptr())))
        if sync:
            self.sync()
        return f

    def grad_batch(self, X, G=None, sync=True):
        """grad!(nlp, x, g) at the K rows of X (`ctd_grad_batch_dev_async`).  G: (K, nvar), allocated when not given.  Returns G."""
        px, k, ldx = self._batch_rows(X, self.dim_NLP_variables, "X")
        G = self._batch_out(G, X, self.dim_NLP_variables, "G", k)
        self._ck(_lib.lib().ctd_grad_batch_dev_async(self._h, k, px, ldx, C.c_void_p(G.data_ptr()), G.stride(0)))
        if sync:
            self.sync()
        return G

    def hess_coord_batch(self, X, Y, obj_weight=1.0, H=None, sync=True):
        """hess_coord!(nlp, x, y, vals; obj_weight) at the K rows of X with the multipliers of the K rows of Y
        (`ctd_hess_coord_batch_dev_async`; obj_weight is shared).  H: (K, nnzh), allocated when not given.  Returns H."""
        px, k, ldx = self._batch_rows(X, self.dim_NLP_variables, "X")
        py, _, ldy = self._batch_rows(Y, self.dim_NLP_constraints, "Y", k)
        H = self._batch_out(H, X, self.nnzh, "H", k)
        self._ck(_lib.lib().ctd_hess_coord_batch_dev_async(self._h, k, px, ldx, py, ldy, float(obj_weight),
                                                            C.c_void_p(H.data_ptr()), H.stride(0)))
        if sync:
            self.sync()
        return H

    def sync(self):
        self._ck(_lib.lib().ctd_sync(self._h))

    def set_stream(self, stream=None):
        """Launch on `stream` from now on (a torch.cuda.Stream, a raw hipStream_t or None = torch's current stream), e.g.
        inside `torch.cuda.graph(...)` to record a whole solver iteration into one HIP graph."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        raw = getattr(stream, "cuda_stream", stream)
        self._ck(_lib.lib().ctd_set_stream(self._h, C.c_void_p(int(raw))))
        self._stream_raw = int(raw)

    def time_cons_jac(self, x, c, vals, iters=20):
        """Mean duration (ms) of one fused-kernel launch, from HIP events recorded by each dispatch on the handle's stream."""
        ms = C.c_double()
        self._ck(_lib.lib().ctd_time_cons_jac_dev(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                                  self._dev_ptr(c, self.dim_NLP_constraints, "c"),
                                                  self._dev_ptr(vals, self.nnzj, "vals"), int(iters), C.byref(ms)))
        return ms.value

    def debug_stamps(self, x, c, vals, sub=False):
        """Diagnostics: per-workgroup phase stamps of one launch, array [grid, 6, 2] (realtime 100 MHz, shader cycles)."""
        grid = self.launch_info()["grid"]
        out = np.zeros(grid * (28 if sub else 12), dtype=np.uint64)
        self._ck(_lib.lib().ctd_debug_stamps(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                             self._dev_ptr(c, self.dim_NLP_constraints, "c"),
                                             self._dev_ptr(vals, self.nnzj, "vals"),
                                             out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        if sub:      # experiment builds (-DCTD_SUBSTAMPS): [grid, wave 0/1, 8] cycle stamps inside the evaluation phase
            return out[:grid * 12].reshape(grid, 6, 2), out[grid * 12:].reshape(grid, 2, 8)
        return out.reshape(grid, 6, 2)

    # ---- Hessian of the Lagrangian ------------------------------------------------------------------------
    def hess_structure(self):
        """hess_structure!(nlp, rows, cols): 1-based COO (row >= col) of the lower triangle of DOCP_Hessian_pattern."""
        rows = np.zeros(self.nnzh, dtype=np.int64)
        cols = np.zeros(self.nnzh, dtype=np.int64)
        self._ck(_lib.lib().ctd_hess_structure(self._h, _ip(rows), _ip(cols)))
        return rows, cols

    def hess_coord(self, x, y, obj_weight=1.0, vals=None, sync=True):
        """hess_coord!(nlp, x, y, vals; obj_weight): obj_weight * d2 f + sum_i y_i d2 c_i on hess_structure()."""
        L = _lib.lib()
        self._check_x(x)
        if _is_tensor(x):
            import torch
            if vals is None:
                vals = torch.empty(self.nnzh, dtype=torch.float64, device=x.device)
            fn = L.ctd_hess_coord_dev if sync else L.ctd_hess_coord_dev_async
            self._ck(fn(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"), self._dev_ptr(y, self.dim_NLP_constraints, "y"),
                        float(obj_weight), self._dev_ptr(vals, self.nnzh, "vals")))
            return vals
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.size != self.dim_NLP_constraints:
            raise ValueError(f"y has {y.size} entries, expected dim_NLP_constraints = {self.dim_NLP_constraints}")
        vals = np.empty(self.nnzh) if vals is None else _host_out(vals, self.nnzh, "vals")
        self._ck(L.ctd_hess_coord(self._h, _dp(x), _dp(y), float(obj_weight), _dp(vals)))
        return vals

    def time_hess(self, x, y, vals, obj_weight=1.0, iters=20):
        """Mean duration (ms) of one Hessian-kernel launch (per-dispatch HIP events on the handle's stream)."""
        ms = C.c_double()
        self._ck(_lib.lib().ctd_time_hess_dev(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                              self._dev_ptr(y, self.dim_NLP_constraints, "y"), float(obj_weight),
                                              self._dev_ptr(vals, self.nnzh, "vals"), int(iters), C.byref(ms)))
        return ms.value

    def hess_debug_stamps(self, x, y, vals, obj_weight=1.0):
        """Diagnostics: per-workgroup phase stamps of one Hessian launch, array [grid, 5, 2] (realtime 100 MHz, cycles)."""
        grid = self.hess_launch_info()["grid"]
        out = np.zeros(grid * 10, dtype=np.uint64)
        self._ck(_lib.lib().ctd_hess_debug_stamps(self._h, self._dev_ptr(x, self.dim_NLP_variables, "x"),
                                                  self._dev_ptr(y, self.dim_NLP_constraints, "y"), float(obj_weight),
                                                  self._dev_ptr(vals, self.nnzh, "vals"),
                                                  out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return out.reshape(grid, 5, 2)

    def hess_shard_info(self):
        """(vals_main_begin, vals_main_end, positions of the V x V entries): on a sharded handle hess_coord leaves partial
        sums in the V x V entries, to be added over the shards."""
        o = np.zeros(13, dtype=np.int64)
        self._ck(_lib.lib().ctd_hess_shard_info(self._h, _ip(o)))
        return int(o[0]), int(o[1]), o[3:3 + int(o[2])].copy()

    def hess_launch_info(self):
        o = np.zeros(10, dtype=np.int64)
        self._ck(_lib.lib().ctd_hess_launch_info(self._h, _ip(o)))
        return dict(grid=int(o[0]), block=int(o[1]), lds_bytes=int(o[2]), steps_per_tile=int(o[3]), csc_period=int(o[4]),
                    edge_entries=int(o[5]), stage_lanes=int(o[6]), path_lanes=int(o[7]), boundary_lanes=int(o[8]),
                    segment_terms=int(o[9]))

    def hess_kernel_info(self):
        """which Hessian kernel takes the regular steps: dict(kernel='tile' | 'step', grid=workgroups)"""
        o = np.zeros(2, dtype=np.int64)
        self._ck(_lib.lib().ctd_hess_kernel_info(self._h, _ip(o)))
        return dict(kernel="step" if o[0] == 1 else "tile", grid=int(o[1]))

    def jac_structure(self):
        """jac_structure!(nlp, rows, cols): 1-based COO in CSC order."""
        rows = np.zeros(self.nnzj, dtype=np.int64)
        cols = np.zeros(self.nnzj, dtype=np.int64)
        self._ck(_lib.lib().ctd_jac_structure(self._h, _ip(rows), _ip(cols)))
        return rows, cols


# ---- free functions named after the reference's --------------------------------------------------------------
def constraints(c, xu, docp):
    """`CTDirect.__constraints!(c, xu, docp)`; returns c."""
    return docp.cons(xu, c)


def objective(xu, docp):
    """`CTDirect.__objective(xu, docp)`."""
    return docp.obj(xu)


def gradient(xu, docp, g=None):
    """Gradient of `CTDirect.__objective(xu, docp)` (NLPModels `grad!`)."""
    return docp.grad(xu, g)


def variables_bounds(docp):
    """`CTDirect.__variables_bounds!(docp)` -> (var_l, var_u)."""
    return docp.bounds.var_l, docp.bounds.var_u


def constraints_bounds(docp):
    """`CTDirect.__constraints_bounds!(docp)` -> (lb, ub)."""
    return docp.bounds.con_l, docp.bounds.con_u


class _Pinned:
    """owner of one ctd_host_alloc block (freed when the last array viewing it goes away)"""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        st = _lib.lib().ctd_host_alloc(C.byref(self.ptr), nbytes)
        if st:
            _raise(st, _lib.lib().ctd_last_error(None).decode())

    def __del__(self):
        try:
            _lib.lib().ctd_host_free(self.ptr)
        except Exception:
            pass


def pinned_empty(n, dtype=np.float64):
    """NumPy array in page-locked host memory (`ctd_host_alloc`): passing such arrays to the host-pointer calls
    (`docp.cons_jac(x, c, vals)` with NumPy arguments, ...) lets the copies run as direct DMA at PCIe rate."""
    dtype = np.dtype(dtype)
    own = _Pinned(int(n) * dtype.itemsize)
    buf = (C.c_char * (int(n) * dtype.itemsize)).from_address(own.ptr.value)
    a = np.frombuffer(buf, dtype=dtype, count=int(n))
    _pinned_owners[a.__array_interface__["data"][0]] = own      # keeps the block alive as long as the module does ...
    import weakref
    weakref.finalize(a, _pinned_owners.pop, a.__array_interface__["data"][0], None)   # ... or until the array is collected
    return a


_pinned_owners = {}


def initial_guess(docp, init=None):
    """`CTDirect.__initial_guess(docp, init)`.  init: None (everything 0.1), "problem" (the problem file's init
    tuple) or a dict with optional constant `state`, `control`, `variable` entries; with a `time` entry (K increasing
    times) `state` [K, n] and `control` [K, m] are trajectories -- the interpolated / warm-start guesses of the reference
    (test/ci/test_initial_guess.jl), e.g. the T, X, U of `unpack_solution` -- interpolated linearly at the node (and stage)
    times."""
    x0 = np.zeros(docp.dim_NLP_variables)
    ci = _lib.ctd_init()
    keep = []
    if init == "problem":
        ci.use_problem_default = 1
    elif isinstance(init, dict) and init.get("time") is not None:
        t = np.ascontiguousarray(init["time"], dtype=np.float64)
        keep.append(t)
        ci.n_samples, ci.t_samples = len(t), _dp(t)
        for key, dim in (("state", docp.dims.NLP_x), ("control", docp.dims.NLP_u)):
            if init.get(key) is not None and dim > 0:
                a = np.ascontiguousarray(init[key], dtype=np.float64).reshape(len(t), dim)
                keep.append(a)
                setattr(ci, key + "_samples", _dp(a))
        if init.get("variable") is not None:
            a = np.ascontiguousarray(init["variable"], dtype=np.float64)
            keep.append(a)
            ci.variable = _dp(a)
    elif isinstance(init, dict):
        for key in ("state", "control", "variable"):
            if init.get(key) is not None:
                a = np.ascontiguousarray(init[key], dtype=np.float64)
                keep.append(a)
                setattr(ci, key, _dp(a))
    docp._ck(_lib.lib().ctd_initial_guess(docp._h, _dp(x0), C.byref(ci)))
    return x0


def DOCP_Jacobian_pattern(docp):
    """`CTDirect.DOCP_Jacobian_pattern(docp)` as 0-based CSC arrays (colptr, rowval) of the Bool sparse matrix."""
    colptr = np.zeros(docp.dim_NLP_variables + 1, dtype=np.int64)
    rowval = np.zeros(docp.nnzj, dtype=np.int64)
    docp._ck(_lib.lib().ctd_jac_csc(docp._h, _ip(colptr), _ip(rowval)))
    return colptr, rowval


def DOCP_Jacobian_csr(docp):
    """The same pattern as 0-based CSR arrays (rowptr, colind): the order of the values of a DOCP built with value_order="csr"."""
    rowptr = np.zeros(docp.dim_NLP_constraints + 1, dtype=np.int64)
    colind = np.zeros(docp.nnzj, dtype=np.int64)
    docp._ck(_lib.lib().ctd_jac_csr(docp._h, _ip(rowptr), _ip(colind)))
    return rowptr, colind


def DOCP_Hessian_csr(docp):
    """(rowptr, colind) of the UPPER triangle by rows -- the CSR reading of the value array hess_coord fills (the lower triangle by
    columns of a symmetric matrix is its upper triangle by rows)."""
    rowptr = np.zeros(docp.dim_NLP_variables + 1, dtype=np.int64)
    colind = np.zeros(docp.nnzh, dtype=np.int64)
    docp._ck(_lib.lib().ctd_hess_csr(docp._h, _ip(rowptr), _ip(colind)))
    return rowptr, colind


def DOCP_Hessian_pattern(docp):
    """Lower triangle of `CTDirect.DOCP_Hessian_pattern(docp)` as 0-based CSC arrays (colptr, rowval) -- the part of the
    symmetric Bool pattern ADNLPModels keeps for hess_structure!."""
    colptr = np.zeros(docp.dim_NLP_variables + 1, dtype=np.int64)
    rowval = np.zeros(docp.nnzh, dtype=np.int64)
    docp._ck(_lib.lib().ctd_hess_csc(docp._h, _ip(colptr), _ip(rowval)))
    return colptr, rowval


def get_time_grid(xu, docp):
    """`CTDirect.get_time_grid(xu, docp)` (src/DOCP_data.jl:437-458): t_i = t0 + tau_i (tf - t0), t0 / tf fixed or entries of v."""
    xu = np.ascontiguousarray(xu.detach().cpu().numpy() if _is_tensor(xu) else xu, dtype=np.float64)
    grid = np.zeros(docp.time.steps + 1)
    docp._ck(_lib.lib().ctd_time_grid_at(docp._h, _dp(xu), _dp(grid)))
    return grid


def _state_control_variable(docp, data):
    """X[N+1, n], U[N+1, m], v read from any vector with the NLP variable layout (the primal iterate or a vector of bound
    multipliers) with the reference's getters (`getter(...; val=:state | :control | :variable)`, src/ode/common.jl:50-84)"""
    n, m, nv = docp.dims.NLP_x, docp.dims.NLP_u, docp.dims.NLP_v
    N, blk = docp.time.steps, docp.discretization._step_variables_block
    X = np.stack([data[i * blk:i * blk + n] for i in range(N + 1)])
    stage = docp.discretization.stage
    stagewise = docp.scheme in ("gauss_legendre_2", "gauss_legendre_3")
    cs = getattr(docp.time, "control_steps", 1)
    if cs > 1:
        # getter(...; val = :control) with several controls per step (src/ode/common.jl:84-98): N control_steps + 1 rows, the
        # controls of every step in order, then get_OCP_control_at_time_step(N + 1) = the first control of the last step
        U = np.zeros((N * cs + 1, m))
        for i in range(N):
            for j in range(cs):
                U[i * cs + j] = data[i * blk + n + j * m:i * blk + n + (j + 1) * m]
        U[N * cs] = data[(N - 1) * blk + n:(N - 1) * blk + n + m]
        return X, U, data[len(data) - nv:].copy()
    U = np.zeros((N + 1, m))
    if m:
        b = docp.discretization.butcher_b if stagewise else None
        for i in range(N + 1):
            j = i if (i < N or docp.discretization._final_control) else N - 1     # u(t_f) = U_N convention
            if docp.scheme == "euler_implicit":
                j = max(i - 1, 0) if i > 0 else 0                                # u(t_i) = U_{i-1}, u(t_0) = U_0
            o = j * blk + n
            U[i] = sum(b[s] * data[o + s * m:o + (s + 1) * m] for s in range(stage)) if stagewise else data[o:o + m]
    return X, U, data[len(data) - nv:].copy()


def unpack_solution(docp, x, multipliers=None, multipliers_L=None, multipliers_U=None):
    """The arrays `CTDirect.build_OCP_solution` hands to CTModels (src/DOCP_data.jl:514-633) from an NLP solution, with the
    reference's getter conventions (src/ode/common.jl:7-104): X[N+1, n], U[N+1, m] (control of the scheme at every node,
    final control duplicated when the scheme has none), v, and from the constraint multipliers the costate P[N, n] (the
    multipliers of the state-equation rows), the path-constraint duals divided by the step length and the boundary duals;
    from the bound multipliers (`multipliers_L`, `multipliers_U`, nvar entries each) the state / control / variable box
    duals, read with the same getters as the primal arrays."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if _is_tensor(x) else x, dtype=np.float64)
    N = docp.time.steps
    T = get_time_grid(x, docp)
    X, U, v = _state_control_variable(docp, x)
    out = dict(T=T, X=X, U=U, v=v)
    cs = getattr(docp.time, "control_steps", 1)
    # time grid of the control rows (src/DOCP_data.jl:557-567): T_control[k] = T[i] + (j - 1) h_i / control_steps, last = T[end]
    out["T_control"] = np.concatenate([(T[:-1, None] + np.arange(cs)[None, :] * (np.diff(T)[:, None] / cs)).ravel(), T[-1:]]) if cs > 1 else T
    for z, tag in ((multipliers_L, "lb"), (multipliers_U, "ub")):
        zz = np.zeros_like(x) if z is None else np.ascontiguousarray(z, dtype=np.float64)
        ZX, ZU, Zv = _state_control_variable(docp, zz)
        out["state_constraints_%s_dual" % tag], out["control_constraints_%s_dual" % tag] = ZX, ZU
        out["variable_constraints_%s_dual" % tag] = Zv
    if multipliers is not None:
        y = np.ascontiguousarray(multipliers, dtype=np.float64)
        n = docp.dims.NLP_x
        eqs, p, bc = docp.discretization._state_stage_eqs_block, docp.dims.path_cons, docp.dims.boundary_cons
        cb = eqs + p
        out["P"] = np.stack([y[i * cb:i * cb + n] for i in range(N)])
        h = np.diff(T)
        raw = np.stack([y[i * cb + eqs:i * cb + eqs + p] for i in range(N)] + [y[N * cb:N * cb + p]]) if p else np.zeros((N + 1, 0))
        out["path_constraints_dual"] = raw / np.concatenate([h, h[-1:]])[:, None]
        out["boundary_constraints_dual"] = y[N * cb + p:N * cb + p + bc].copy()
    return out


class MultiDeviceDOCP:
    """One transcription sharded by time step over several GPUs of THIS process (`ctd_create_sharded`): the single-process
    counterpart of `dist.ShardedDOCP`.  Buffers are full-length on every device (global indexing); shard k writes its rows
    of c and its CSC ranges of the Jacobian values.  `devices` may repeat an ordinal (tests on a one-GPU box)."""

    # include/ctdirect_hip.h: X_SHARDED copies the halo entries (peer copies ordered by events, any topology); X_SHARDED_IN_PLACE lets
    # the kernels load them from the owner's buffer (needs peer access; falls back to the copies when a pair of devices has none)
    X_IN_PLACE, X_SHARDED, X_FROM_DEVICE0, X_SHARDED_COPY, X_SHARDED_IN_PLACE = 0, 1, 2, 3, 4

    def __init__(self, ocp, grid_size, scheme, devices, time_grid=None, pattern="manual", stream="torch", value_order="csc"):
        L = _lib.lib()
        pid = PROBLEMS[ocp] if isinstance(ocp, str) else int(ocp)
        scheme = SCHEME_ALIASES.get(scheme, scheme) if isinstance(scheme, str) else scheme
        d = _lib.ctd_desc()
        d.problem, d.scheme = pid, SCHEMES[scheme] if isinstance(scheme, str) else int(scheme)
        d.pattern_mode = PATTERN_MODES[pattern] if isinstance(pattern, str) else int(pattern)
        d.device = -1
        d.value_order = VALUE_ORDERS[value_order] if isinstance(value_order, str) else int(value_order)
        self._tg = None
        if time_grid is not None:
            self._tg = np.ascontiguousarray(time_grid, dtype=np.float64)
            d.time_grid, d.time_grid_len, d.grid_size = _dp(self._tg), len(self._tg), len(self._tg) - 1
        else:
            d.time_grid, d.time_grid_len, d.grid_size = None, 0, int(grid_size)
        self.devices = [int(k) for k in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        st = L.ctd_create_sharded(C.byref(d), arr, len(self.devices), C.byref(h))
        if st != _lib.CTD_OK:
            _raise(st, L.ctd_sharded_last_error(None).decode())
        self._s = h
        self.shards = []
        for k in range(len(self.devices)):
            o = np.zeros(10, dtype=np.int64)
            self._ck(L.ctd_sharded_shard_info(self._s, k, _ip(o)))
            self.shards.append(SimpleNamespace(device=int(o[1]), step_begin=int(o[2]), step_end=int(o[3]), c_row_begin=int(o[4]),
                                               c_row_end=int(o[5]), vals_main_begin=int(o[6]), vals_main_end=int(o[7])))
        nvar, ncon, nnzj, nnzh = (C.c_int64() for _ in range(4))
        h0 = C.c_void_p()
        self._ck(L.ctd_sharded_handle(self._s, 0, C.byref(h0)))
        L.ctd_sizes(h0, C.byref(nvar), C.byref(ncon), C.byref(nnzj), C.byref(nnzh))
        self.dim_NLP_variables, self.dim_NLP_constraints, self.nnzj, self.nnzh = nvar.value, ncon.value, nnzj.value, nnzh.value
        # stream="torch" (default, like DOCP): every shard launches on torch's current stream of its device, so the engine's
        # copies and kernels are ordered with the caller's tensor work on x / c / vals (the private non-blocking streams of
        # stream="own" are not: the caller then synchronises itself)
        self._streams = None
        if stream == "torch":
            self.bind_torch_streams()

    def bind_torch_streams(self):
        import torch
        L = _lib.lib()
        cur = [torch.cuda.current_stream(dev).cuda_stream for dev in self.devices]
        if cur != self._streams:
            for k, st in enumerate(cur):
                hk = C.c_void_p()
                self._ck(L.ctd_sharded_handle(self._s, k, C.byref(hk)))
                self._ck(L.ctd_set_stream(hk, C.c_void_p(st)))
            self._streams = cur

    def _ck(self, st):
        if st != _lib.CTD_OK:
            _raise(st, _lib.lib().ctd_sharded_last_error(self._s).decode() or _lib.lib().ctd_strerror(st).decode())

    def _ptrs(self, tensors, n, name):
        import torch
        if tensors is None:
            return None
        assert len(tensors) == len(self.devices)
        for k, t in enumerate(tensors):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n and t.device.index == self.devices[k]):
                raise ValueError(f"{name}[{k}] must be a contiguous float64 tensor of {n} entries on cuda:{self.devices[k]}")
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def cons_jac(self, x, c, vals, x_mode=0, stitch=False, sync=True):
        """x, c, vals: lists of one full-length tensor per shard (on that shard's device)."""
        if self._streams is not None:
            self.bind_torch_streams()          # (a cheap compare; rebinds when the caller switched torch streams)
        self._ck(_lib.lib().ctd_cons_jac_sharded_dev_async(self._s, self._ptrs(x, self.dim_NLP_variables, "x"),
                                                           self._ptrs(c, self.dim_NLP_constraints, "c"),
                                                           self._ptrs(vals, self.nnzj, "vals"), int(x_mode), int(bool(stitch))))
        if sync:
            self.sync()

    def sync(self):
        self._ck(_lib.lib().ctd_sharded_sync(self._s))

    def last_error(self):
        """`ctd_sharded_last_error`: the message of the last failed call -- or of the last fallback (X_SHARDED_IN_PLACE on devices
        without peer access takes the copying protocol and says so here)."""
        return _lib.lib().ctd_sharded_last_error(self._s).decode()

    def close(self):
        if getattr(self, "_s", None):
            _lib.lib().ctd_sharded_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
