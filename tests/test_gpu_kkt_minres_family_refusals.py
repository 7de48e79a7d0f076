"""The C-level refusals of the three sharded MINRES phase families on the MI355X, from one table: ctd_kkt_minres_shard_*,
ctd_kkt_minres_schur_cr_shard_* and ctd_kkt_minres_schur_cr_joint_* (start, begin, alfa, lanczos, update, info).

One case: Goddard, trapeze, N = 20, CSR handles of the steps (0, 7), (7, 14), (14, 20) -- every rank past the first has at least two
steps, as the joined form needs --, the calls made on the middle rank.  Every row is a call with exactly one fault.  It returns
CTD_EINVAL, ctd_last_error starts with the entry point's own name and contains the fragment naming the fault, and nothing was
written: z, the solve's workspace (its state words included) and the factor's workspace have the bits they had before.  Nothing is
launched on a bad pointer: every fault is found by the host checks."""
import ctypes as C
from collections import namedtuple

import pytest

import ctdirect_jl_amd as ct
from test_gpu_kkt_schur_cr_joint import JointCase

pytestmark = pytest.mark.gpu

CASE = ("goddard", "trapeze", 20, (0, 7, 14, 20), False, False)
G, RANK = 3, 1
PHASES = ("start", "begin", "alfa", "lanczos", "update", "info")
# a phase family: its name, the prefix of its entry points, the phases that take the factor's workspace
Family = namedtuple("Family", "name prefix schur")
FAMILIES = (Family("plain", "ctd_kkt_minres_shard_", ()),
            Family("schur_cr_shard", "ctd_kkt_minres_schur_cr_shard_", ("start", "lanczos")),
            Family("schur_cr_joint", "ctd_kkt_minres_schur_cr_joint_", ("start", "begin", "lanczos", "update")))


def arguments(fam, phase):
    """the names of the entry point's arguments behind the handle, in the header's order"""
    return ((["sys"] if phase == "start" else []) + (["schur_ws"] if phase in fam.schur else []) + (["rhs"] if phase == "start" else []) +
            (["z"] if phase in ("start", "alfa", "lanczos", "update") else []) + ["ws", "n_ranks"] + (["rank"] if phase != "info" else []) +
            (["rtol", "max_iter"] if phase == "start" else []) + (["info"] if phase == "info" else []))


def entry(fam, phase):
    return fam.prefix + phase + ("" if phase == "info" else "_dev_async")


# One fault per row: (id, the arguments it replaces, their values -- from the environment e of the family --, the fragment of the message; a dict
# where the families word it differently: the diagonal form takes both of px / pc or neither, the Schur forms need both).  A row is
# run on every phase whose entry point has all the arguments it names (the last two name both buffers of the pair that is the fault:
# a phase with only one of them has no such fault).
NEEDS_BOTH = {"plain": b"px and pc are given both", "schur_cr_shard": b"null argument (px is required)",
              "schur_cr_joint": b"null argument (px is required)"}
NEEDS_PC = dict(NEEDS_BOTH, schur_cr_shard=b"null argument (pc is required)", schur_cr_joint=b"null argument (pc is required)")
ROWS = [
    ("n_ranks-0", ("n_ranks",), lambda e: dict(n_ranks=0), b"n_ranks = 0, must be at least 1"),
    ("n_ranks-negative", ("n_ranks",), lambda e: dict(n_ranks=-2), b"n_ranks = -2, must be at least 1"),
    ("n_ranks-above-N", ("n_ranks",), lambda e: dict(n_ranks=21), b"n_ranks = 21 exceeds the 20 steps"),
    ("rank-negative", ("rank",), lambda e: dict(rank=-1), b"rank = -1 is outside [0, n_ranks = 3)"),
    ("rank-n_ranks", ("rank",), lambda e: dict(rank=3), b"rank = 3 is outside [0, n_ranks = 3)"),
    ("rank-first", ("rank",), lambda e: dict(rank=0), b"cannot be block rank = 0 of n_ranks = 3"),
    ("rank-last", ("rank",), lambda e: dict(rank=2), b"cannot be block rank = 2 of n_ranks = 3"),
    ("rank-last-of-two", ("n_ranks", "rank",), lambda e: dict(n_ranks=2, rank=1), b"cannot be block rank = 1 of n_ranks = 2"),
    ("rhs-null", ("rhs",), lambda e: dict(rhs=None), b"null argument (rhs is required)"),
    ("z-null", ("z",), lambda e: dict(z=None), b"null argument (z is required)"),
    ("ws-null", ("ws",), lambda e: dict(ws=None), b"null argument (ws is required)"),
    ("schur_ws-null", ("schur_ws",), lambda e: dict(schur_ws=None), b"null argument (schur_ws is required)"),
    ("px-null", ("sys",), lambda e: dict(sys=e.system(px=None)), NEEDS_BOTH),
    ("pc-null", ("sys",), lambda e: dict(sys=e.system(pc=None)), NEEDS_PC),
    ("rhs-misaligned", ("rhs",), lambda e: dict(rhs=e.V(e.rhs, 4)), b"rhs is not aligned to 8 bytes"),
    ("z-misaligned", ("z",), lambda e: dict(z=e.V(e.z, 4)), b": z is not aligned to 8 bytes"),
    ("ws-misaligned", ("ws",), lambda e: dict(ws=e.V(e.w.ws, 4)), b": ws is not aligned to 8 bytes"),
    ("schur_ws-misaligned", ("schur_ws",), lambda e: dict(schur_ws=e.V(e.P.ws, 4)), b"schur_ws is not aligned to 8 bytes"),
    ("px-misaligned", ("sys",), lambda e: dict(sys=e.system(px=e.px.data_ptr() + 4)), b"px is not aligned to 8 bytes"),
    ("pc-misaligned", ("sys",), lambda e: dict(sys=e.system(pc=e.pc.data_ptr() + 4)), b"pc is not aligned to 8 bytes"),
    ("z-inside-ws", ("z",), lambda e: dict(z=e.V(e.w.ws, 8 * 64)), b"z overlaps the workspace"),
    ("schur_ws-inside-ws", ("schur_ws",), lambda e: dict(schur_ws=e.V(e.w.ws, 8 * 64)), b"schur_ws must not overlap z or the workspace"),
    ("schur_ws-is-z", ("schur_ws", "z"), lambda e: dict(schur_ws=e.V(e.z), z=e.V(e.z)), b"schur_ws must not overlap z or the workspace"),
    ("z-is-rhs", ("z", "rhs"), lambda e: dict(z=e.V(e.rhs), rhs=e.V(e.rhs)), b"must not overlap an input buffer"),
    ("rtol-negative", ("rtol",), lambda e: dict(rtol=-1.0), b"rtol must not be negative"),
    ("rtol-nan", ("rtol",), lambda e: dict(rtol=float("nan")), b"rtol must not be negative"),
    ("max_iter-0", ("max_iter",), lambda e: dict(max_iter=0), b"max_iter = 0, must be at least 1"),
    ("sys-struct_size-0", ("sys",), lambda e: dict(sys=e.system(struct_size=0)), b"sys is null or its struct_size is not sizeof(ctd_kkt_system)"),
    ("sys-struct_size-large", ("sys",), lambda e: dict(sys=e.system(struct_size=C.sizeof(ct._lib.ctd_kkt_system) + 8)),
     b"sys is null or its struct_size is not sizeof(ctd_kkt_system)"),
    ("sys-null", ("sys",), lambda e: dict(sys=None), b"sys is null or its struct_size is not sizeof(ctd_kkt_system)"),
    ("info-null", ("info",), lambda e: dict(info=None), b"info is null or its struct_size is not sizeof(ctd_minres_info)"),
    ("info-struct_size", ("info",), lambda e: dict(info=ct._lib.ctd_minres_info(struct_size=8)),
     b"info is null or its struct_size is not sizeof(ctd_minres_info)"),
]


class Env:
    """the middle rank's arguments of one family: its handle, the workspace (zeros), z (sevens), the factor of the family"""

    def __init__(self, torch, s, fam):
        self.fam, self.h = fam, s.hs[RANK]
        self.rhs, self.px, self.pc = s.rhs, s.pxd, s.pcd
        self.P = {"plain": None, "schur_cr_shard": lambda: s.factors()[RANK], "schur_cr_joint": lambda: s.joint()[RANK]}[fam.name]
        self.P = self.P() if self.P else None
        # z: the head of a buffer long enough that the factor's workspace laid at z (schur_ws-is-z) ends inside it
        self.zbuf = torch.full((s.n + (self.P.layout.workspace if self.P else 0),), 7.0, dtype=torch.float64, device="cuda")
        self.z = self.zbuf[:s.n]
        self.w = {"plain": lambda: self.h.kkt_minres_shard_workspace(G), "schur_cr_shard": lambda: self.h.kkt_minres_schur_shard_workspace(G),
                  "schur_cr_joint": lambda: self.h.kkt_minres_schur_joint_workspace(G, RANK)}[fam.name]()
        # ... and laid 64 doubles into the solve's workspace (schur_ws-inside-ws) it ends inside that
        assert self.P is None or 64 + self.P.layout.workspace <= self.w.layout.workspace
        self.h.sync()
        self.rhs_bits = self.rhs.clone()
        self.P_bits = None if self.P is None else self.P.ws.view(torch.int64).clone()
        self.torch = torch

    @staticmethod
    def V(a, off=0):
        return C.c_void_p(a.data_ptr() + off)

    def system(self, **kw):
        lib = ct._lib
        return lib.ctd_kkt_system(**dict(dict(struct_size=C.sizeof(lib.ctd_kkt_system), obj_weight=1.0, px=self.px.data_ptr(),
                                              pc=self.pc.data_ptr()), **kw))

    def call(self, phase, **replaced):
        lib = ct._lib
        a = dict(sys=self.system(), schur_ws=self.P and self.V(self.P.ws), rhs=self.V(self.rhs), z=self.V(self.z), ws=self.V(self.w.ws),
                 n_ranks=G, rank=RANK, rtol=1e-10, max_iter=10, info=lib.ctd_minres_info(struct_size=C.sizeof(lib.ctd_minres_info)))
        a.update(replaced)
        byref = lambda nm: None if a[nm] is None else C.byref(a[nm]) if nm in ("sys", "info") else a[nm]      # noqa: E731
        return getattr(lib.lib(), entry(self.fam, phase))(self.h._h, *[byref(nm) for nm in arguments(self.fam, phase)])

    def untouched(self):
        t = self.torch
        self.h.sync()
        return (bool((self.zbuf == 7.0).all()) and not bool(self.w.ws.any()) and t.equal(self.rhs, self.rhs_bits) and
                (self.P is None or t.equal(self.P.ws.view(t.int64), self.P_bits)))


@pytest.fixture(scope="module")
def envs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    s = JointCase(torch, CASE)
    assert all(s.cuts[k + 1] - s.cuts[k] >= 2 for k in range(1, G))
    yield {fam.name: Env(torch, s, fam) for fam in FAMILIES}
    s.close()


def phases_of(fam, row):
    return [phase for phase in PHASES if set(row[1]) <= set(arguments(fam, phase))]


TABLE = [(fam, row) for fam in FAMILIES for row in ROWS if phases_of(fam, row)]       # (the diagonal form has no schur_ws rows)


@pytest.mark.parametrize("fam, row", TABLE, ids=[f"{fam.name}-{row[0]}" for fam, row in TABLE])
def test_one_fault_is_refused_by_name(envs, fam, row):
    e = envs[fam.name]
    _, keys, replace, what = row
    what = what[fam.name] if isinstance(what, dict) else what
    replaced = replace(e)
    assert set(replaced) == set(keys)
    for phase in phases_of(fam, row):
        assert e.call(phase, **replaced) == ct._lib.CTD_EINVAL, (phase, row[0])
        err = ct._lib.lib().ctd_last_error(e.h._h)
        assert err.startswith(entry(fam, phase).encode() + b": ") and what in err, (phase, row[0], what, err)
        assert e.untouched(), (phase, row[0], "a refused call wrote something")


@pytest.mark.parametrize("fam", FAMILIES, ids=[f.name for f in FAMILIES])
def test_the_good_calls_go_through(envs, fam):
    """the defaults of the table are a valid call of every phase: each row's fault is its only one"""
    e = envs[fam.name]
    for phase in ("info", "start"):         # (the state words of a zeroed workspace, then the one phase that needs no gather before it)
        assert e.call(phase) == 0, (phase, ct._lib.lib().ctd_last_error(e.h._h))
    e.h.sync()
    assert not bool((e.z == 7.0).all()) and bool(e.w.ws.any())
    e.zbuf.fill_(7.0)           # as the rows found it
    e.w.ws.zero_()
    if e.P is not None:
        e.P.ws.view(e.torch.int64).copy_(e.P_bits)
    e.torch.cuda.synchronize()
    assert e.untouched()
