"""Time-step sharding of one transcription across the GPUs of a node (one process per GPU, torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" on CPU for tests).

The reference has no parallelism of any kind; what is partitioned here is its main loop
`for i in 1:docp.time.steps` (src/DOCP_functions.jl:92-98): step i reads X_i, U_i, K_i, X_{i+1} and v, and writes only
its own rows c[(i-1)(eqs+p)+1 : i(eqs+p)] and the Jacobian entries of those rows.

  * rank r evaluates the contiguous block of steps [r N/G, (r+1) N/G); the first rank also owns the irregular first-step
    columns, the last rank the final-state columns;
  * the ITERATE is sharded like the steps: rank r holds the variables of its own steps inside a
    full-length buffer (global indexing, so the engine's shard handles read it as it is).  What a rank needs from the
    others is tiny: the state X of the NEXT rank's first node (+ its control for trapeze), the first and the final state for
    the boundary rows, and the replicated optimisation variables v.  `exchange_halo` moves them with ONE all-gather of
    n (+m) + n doubles per rank per iterate;
  * a consumer that keeps the whole iterate on one rank calls `broadcast_iterate` instead: one broadcast of nvar doubles;
  * each rank writes its rows straight into a full-length c buffer at their global position; the p+bc tail rows
    (final-time path and boundary constraints) are authoritative on the LAST rank (it owns X_{N+1} and the last controls and
    receives X_1); other ranks only hold them after stitching;
  * outputs stay ROW-SHARDED: rank r holds its rows of c and, for the Jacobian values, one contiguous range of the global
    CSC value array (its step columns) plus its slice of every V column -- what a distributed KKT consumer wants;
    `DOCP.shard` gives the ranges.  The evaluation itself needs no collective;
  * the matrix-free products (`ShardedDOCP.jprod` / `jtprod` / `hprod`) keep their directions and results sharded the same
    way: a rank fetches the few halo entries of a direction with one small all-gather (`exchange_product_halo` for a
    variable-layout vector, `exchange_product_rows` for a constraint-layout one) and a transposed product adds the nv
    entries of d/dv with one all-reduce;
  * a consumer that wants the residual vector whole on every rank asks for it (`stitch=True`): ONE all-gather of the row
    blocks per evaluation (in place when the blocks are equal, through a padded buffer + one index kernel when ragged).

Every collective is enqueued on torch's current stream, and so are the engine's kernels (`ShardedDOCP` rebinds the handle
to that stream): nothing here synchronises with the host.
"""
import os

import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .docp import _PHASE_FAMILIES, SchurCrJointPrecond, _phase_family

# Rehearsal knob: run the collectives on a ONE-rank group too (they are no-ops for the data, but every RCCL call of the
# multi-GPU path -- in-place / padded all-gather, halo all-gather, all-reduce, broadcast -- is issued exactly as on 8 GPUs),
# so the one-GPU box can exercise the real backend
_FORCE = os.environ.get("CTD_DIST_FORCE") == "1"


def shard_steps(N, world, rank):
    """Contiguous block of ceil/floor(N / world) steps for `rank` (equal blocks when world divides N)."""
    base, rem = divmod(N, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


_FLAT_GATHER = {}


def _all_gather_into(recv, send, group=None):
    """recv[r * len(send) : (r+1) * len(send)] = rank r's `send`.  RCCL ("nccl"): one all_gather_into_tensor (send may be a
    view of recv: in place), unguarded -- a failing collective raises on the rank it fails on.  gloo (CPU tests and the
    one-GPU rehearsal; it moves host memory only) goes through the list form, staged on the host when the tensors live on a
    GPU.  The choice is made once per group from the backend's name, never by catching an error of the collective."""
    flat = _FLAT_GATHER.get(group)
    if flat is None:
        flat = _FLAT_GATHER[group] = str(dist.get_backend(group)).lower() in ("nccl", "rccl")
    if flat:
        dist.all_gather_into_tensor(recv, send, group=group)
        return
    world = dist.get_world_size(group)
    n = send.numel()
    if send.is_cuda:
        hs = send.cpu()
        parts = [torch.empty_like(hs) for _ in range(world)]
        dist.all_gather(parts, hs, group=group)
        recv.copy_(torch.cat(parts))
    else:
        dist.all_gather([recv[r * n:(r + 1) * n] for r in range(world)], send.clone(), group=group)


class _Stitcher:
    """All-gather of the per-rank row blocks of c, with the p + bc tail rows (final-time path and boundary constraints) taken
    from the LAST rank -- the only one that holds everything they read when the iterate is sharded.  Every rank sends its
    block padded to the longest one (+ the tail slot), ONE all_gather_into_tensor, then one index kernel writes the whole c
    (index built once).  Equal blocks without tail rows are gathered in place."""

    def __init__(self, N, cb, ncon, world, rank, device, group=None):
        self.N, self.cb, self.world, self.rank, self.group = N, cb, world, rank, group
        self.tail = ncon - N * cb
        self.in_place = (N % world == 0) and self.tail == 0
        if not self.in_place and (world > 1 or _FORCE):
            blocks = [shard_steps(N, world, r) for r in range(world)]
            self.smax = max(e - b for b, e in blocks) * cb + self.tail
            self.begin, self.end = blocks[rank][0] * cb, blocks[rank][1] * cb
            idx = torch.empty(ncon, dtype=torch.long)
            for r, (b, e) in enumerate(blocks):
                idx[b * cb:e * cb] = r * self.smax + torch.arange((e - b) * cb)
            last_rows = (blocks[-1][1] - blocks[-1][0]) * cb
            idx[N * cb:] = (world - 1) * self.smax + last_rows + torch.arange(self.tail)
            self.idx = idx.to(device)
            self.send = torch.zeros(self.smax, dtype=torch.float64, device=device)
            self.recv = torch.zeros(world * self.smax, dtype=torch.float64, device=device)

    def __call__(self, c):
        if self.world == 1 and not _FORCE:
            return c
        N, cb, world, rank = self.N, self.cb, self.world, self.rank
        if self.in_place:
            S = (N // world) * cb
            body = c[:N * cb]
            _all_gather_into(body, body[rank * S:(rank + 1) * S], self.group)
            return c
        own = self.end - self.begin
        self.send[:own].copy_(c[self.begin:self.end])
        if rank == world - 1 and self.tail:
            self.send[own:own + self.tail].copy_(c[N * cb:])
        _all_gather_into(self.recv, self.send, self.group)
        torch.index_select(self.recv, 0, self.idx, out=c)
        return c


def stitch_constraints(c, N, cb, world, rank, group=None):
    """All-gather the per-rank row blocks of `c`.  `c` is the full-length constraint vector in which this rank has already
    written its step rows [begin*cb, end*cb); the tail rows [N*cb, ncon) are taken from the last rank.  Returns c.
    (One-shot form; `ShardedDOCP` keeps a `_Stitcher` so the index is built only once.)"""
    return _Stitcher(N, cb, c.numel(), world, rank, c.device, group)(c)


def reduce_objective(partial, group=None, device=None):
    """Sum of the per-shard objective partials (Lagrange partial sums; the last shard adds the Mayer term).  `partial`: a
    float, or a 1-element tensor that is reduced in place and returned (no host round trip)."""
    if torch.is_tensor(partial):
        dist.all_reduce(partial, op=dist.ReduceOp.SUM, group=group)
        return partial
    t = torch.tensor([partial], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return float(t[0])


def reduce_hessian_vv(vals, vv_idx, group=None):
    """Adds the shards' partial sums of the variable x variable Hessian entries (the only entries of hess_coord! that sum
    over every time step): one all-reduce of nv (nv+1)/2 doubles, in place.  `vv_idx` from DOCP.hess_shard_info(), or the
    same positions as a long tensor on vals' device."""
    if len(vv_idx) == 0:
        return vals
    idx = vv_idx if torch.is_tensor(vv_idx) else torch.as_tensor(vv_idx, dtype=torch.long, device=vals.device)
    part = vals.index_select(0, idx)
    dist.all_reduce(part, op=dist.ReduceOp.SUM, group=group)
    vals.index_copy_(0, idx, part)
    return vals


def _shard_dims(d):
    """The block sizes of a handle's transcription that the halo exchanges are built from: (blk variables per step, cb rows per
    step, eqs state / stage rows per step, n states, m controls, halo_w = n (+ m on the trapeze: the next node's control too))"""
    disc = d.discretization
    eqs = disc._state_stage_eqs_block
    n, m = d.dims.NLP_x, d.dims.NLP_u
    return disc._step_variables_block, eqs + disc._step_pathcons_block, eqs, n, m, n + (m if getattr(disc, "_final_control", False) else 0)


def _kkt_halo_ranges(b, e, N, n, w, blk, cb, eqs, ncon):
    """THE read set of ctd_kktprod_shard_dev_async's directions (dx, dy) outside what the shard of the steps [b, e) owns
    (include/ctdirect_hip.h), stated once for `ShardedDOCP.exchange_kkt_halo` and `minres_shards`: (start, length) ranges of dx owned
    by lower shards (X_1, the whole block b - 1) and by higher ones (the first node of block e, X_{N+1}), then of dy owned by lower
    shards (the state / stage rows of step b - 1) and by higher ones (the path rows of node e, the tail rows)."""
    lo_x = [(0, n), ((b - 1) * blk, blk)] if b > 0 else []
    hi_x = [(e * blk, w), (N * blk, n)] if e < N else []
    lo_c = [((b - 1) * cb, eqs)] if b > 0 else []
    hi_c = [(e * cb + eqs, cb - eqs), (N * cb, ncon - N * cb)] if e < N else []
    return lo_x, hi_x, lo_c, hi_c


class _MinresRank:
    """One rank of a sharded MINRES solve: the shard handle, its rank, its workspace and iterate, the operator's arguments"""
    __slots__ = ("docp", "rank", "w", "z", "x", "y", "sigma", "sx", "sc", "rhs", "precond")

    def __init__(self, docp, rank, w, z, x, y, sigma, sx, sc, rhs, precond):
        self.docp, self.rank, self.w, self.z, self.x, self.y, self.sigma = docp, rank, w, z, x, y, float(sigma)
        self.sx, self.sc, self.rhs, self.precond = sx, sc, rhs, precond


class MinresPhases:
    """THE phase order of the sharded MINRES solve (ctd_kkt_minres_shard_*, include/ctdirect_hip.h), written once for both drivers:
    `ShardedDOCP.kkt_minres` (one rank per process, the gathers are collectives of the process group) and `kkt_minres_shards` (every
    rank in this process, the gathers are device copies).  ranks: the _MinresRank of every rank this process drives; halo(): fills
    the halo of every rank's Lanczos vector (w.v_x, w.v_c); gather(which): fills every rank's w.gathered_a / w.gathered_b ("a" / "b")
    from the ranks' send slots.  Everything is enqueued on one stream; nothing here waits for the host except `infos`."""

    def __init__(self, ranks, halo, gather):
        self.ranks, self.halo, self.gather = ranks, halo, gather
        # The phase family (docp._PHASE_FAMILIES), from the first rank's preconditioner: a SchurCrShardPrecond per rank is the family
        # ctd_kkt_minres_schur_cr_shard_* on workspaces with the larger slots; a SchurCrJointPrecond per rank (factored AND joined)
        # the family ctd_kkt_minres_schur_cr_joint_*, whose slots also carry the solve records and whose begin and (C) take the
        # factor's workspace.  The same phases, the same gathers; either kind on every rank or on none
        self.family = _phase_family(ranks[0].precond)
        for fam in _PHASE_FAMILIES:
            if fam.precond is not None and any(isinstance(r.precond, fam.precond) != (fam is self.family) for r in ranks):
                raise ValueError(f"precond: a {fam.precond.__name__} on every shard or on none")

    def _phase(self, phase):
        for r in self.ranks:
            r.docp._phase(self.family, phase, r.precond, r.z, r.w, r.rank)

    def start(self, rtol, max_iter):
        for r in self.ranks:
            r.docp._phase_start(self.family, r.precond, r.rhs, r.z, r.w, r.rank, rtol, max_iter)
        self.gather("a")
        self._phase("begin")

    def iterate(self, k):
        """k iterations: per iteration the halo of v, K v (two launches per rank), (A), the gather of slot A, (B), the gather of
        slot B, (C)"""
        for _ in range(k):
            self.halo()
            for r in self.ranks:
                r.docp.kktprod_shard(r.x, r.y, r.w.v_x, r.w.v_c, r.sigma, r.sx, r.sc, out=(r.w.kv_x, r.w.kv_c))
                r.docp._phase(self.family, "alfa", r.precond, r.z, r.w, r.rank)
            self.gather("a")
            self._phase("lanczos")
            self.gather("b")
            self._phase("update")

    def infos(self):
        """every rank's MinresInfo: the one host read per chunk"""
        return [r.docp._phase_info(self.family, r.w) for r in self.ranks]

    def solve(self, rtol, max_iter, check_every, on_chunk=None):
        """start, then chunks of check_every iterations with one read of the state between chunks.  Every rank's state has the
        same bytes (every cross-rank sum is formed from the same gathered slots in the same order on every rank), so the first
        rank's status decides for all of them."""
        if check_every < 1 or max_iter < 1:
            raise ValueError("check_every and max_iter must be at least 1")
        self.start(rtol, max_iter)
        done = 0
        while True:
            self.iterate(check_every)
            done += check_every
            infos = self.infos()
            if on_chunk is not None:
                on_chunk(self, infos)
            if infos[0].status != "running" or done >= max_iter:
                return infos


def _kkt_halo_index(d, lay):
    """`_kkt_halo_ranges` of the handle d's shard as one sorted index tensor (CPU) into an (nvar + ncon)-vector, without the
    entries the shard owns (lay: its ctd_minres_shard_layout)"""
    blk, cb, eqs, n, _, w = _shard_dims(d)
    nvar, ncon = d.dim_NLP_variables, d.dim_NLP_constraints
    lo_x, hi_x, lo_c, hi_c = _kkt_halo_ranges(d.shard.step_begin, d.shard.step_end, d.time.steps, n, w, blk, cb, eqs, ncon)
    parts = [s + torch.arange(k) for s, k in lo_x + hi_x] + [nvar + s + torch.arange(k) for s, k in lo_c + hi_c]
    if not parts:
        return torch.zeros(0, dtype=torch.long)
    idx = torch.unique(torch.cat(parts))
    own = ((idx >= lay.var_begin) & (idx < lay.var_end)) | ((idx >= lay.row_begin) & (idx < lay.row_end)) | \
          ((idx >= lay.tail_begin) & (idx < lay.tail_end))
    return idx[~own]


def minres_shards(handles, xs, y, rhs, obj_weight=1.0, sx=None, sc=None, precond=None, out=None, workspaces=None):
    """The MinresPhases of a solve whose shards are ALL in this process: `handles` are the shard handles of one transcription in
    ascending order of their steps (one whole-grid handle: the single shard), on one GPU and one stream (torch's current one).
    xs: one x per handle (a shard's own entries and the halo it reads valid, or the table of `set_x_shards` set); y, rhs, sx, sc:
    full-length tensors shared by the shards, or one per shard (a list); precond: None, a pair (px, pc), one pair per shard, or one
    SchurCrShardPrecond per shard (`DOCP.kkt_schur_cr_shard_factor`: the log-depth Schur preconditioner, exact inside a shard and cut
    at the shard boundaries; the workspaces are then those of `DOCP.kkt_minres_schur_shard_workspace`), or one SchurCrJointPrecond per
    shard (`kkt_schur_cr_joint_shards`, which also does the factor-time gather as device copies: the couplings across the shards
    restored; workspaces of `DOCP.kkt_minres_schur_joint_workspace`).
    out / workspaces: one z / one MinresShardWorkspace per shard, allocated when None.  The gathers are device copies of every
    send slot into every shard's gathered area; the halo of the Lanczos vector is copied from the owners' vectors."""
    G = len(handles)
    dev = xs[0].device
    per = lambda a: list(a) if isinstance(a, (list, tuple)) else [a] * G      # noqa: E731
    ys, rhss, sxs, scs = per(y), per(rhs), per(sx), per(sc)
    pres = list(precond) if precond is not None and isinstance(precond[0], (list, tuple)) else [precond] * G
    cur = torch.cuda.current_stream(dev).cuda_stream
    ranks = []
    for k, h in enumerate(handles):
        if h._stream_raw != cur:
            h.set_stream(cur)
        w = workspaces[k] if workspaces is not None else h._phase_workspace(_phase_family(pres[k]), G, k)
        z = out[k] if out is not None else torch.empty(w.layout.n, dtype=torch.float64, device=dev)
        ranks.append(_MinresRank(h, k, w, z, xs[k], ys[k], obj_weight, sxs[k], scs[k], rhss[k], pres[k]))
    if G == 1:
        return MinresPhases(ranks, lambda: None, lambda which: None)
    n = ranks[0].w.layout.n
    full = torch.empty(n, dtype=torch.float64, device=dev)
    vs = [r.w.ws[r.w.layout.off_v:r.w.layout.off_v + n] for r in ranks]
    halos = [_kkt_halo_index(r.docp, r.w.layout).to(dev) for r in ranks]
    slot = ranks[0].w.layout.slot

    def halo():
        for r, v in zip(ranks, vs):
            lay = r.w.layout
            full[lay.var_begin:lay.var_end].copy_(v[lay.var_begin:lay.var_end])
            full[lay.row_begin:lay.row_end].copy_(v[lay.row_begin:lay.row_end])
        for v, idx in zip(vs, halos):
            if idx.numel():
                v.index_copy_(0, idx, full.index_select(0, idx))

    def gather(which):
        for r in ranks:
            send = r.w.send_a if which == "a" else r.w.send_b
            for q in ranks:
                (q.w.gathered_a if which == "a" else q.w.gathered_b)[r.rank * slot:(r.rank + 1) * slot].copy_(send)

    return MinresPhases(ranks, halo, gather)


def kkt_minres_shards(handles, xs, y, rhs, obj_weight=1.0, sx=None, sc=None, precond=None, rtol=1e-10, max_iter=None, check_every=16,
                      out=None, workspaces=None, on_chunk=None):
    """Preconditioned MINRES on K z = rhs over several shard handles of ONE process (`minres_shards` describes the arguments): the
    in-process counterpart of `ShardedDOCP.kkt_minres`, for hosts that drive all GPUs from one process.  The same phase order
    (MinresPhases) issues the same kernel launches on the same bytes as one process per rank does.  Returns (zs, infos): every
    shard's full-length z (its owned entries and the nv tail valid) and MinresInfo; on_chunk(phases, infos) is called after every
    chunk of check_every iterations."""
    ph = minres_shards(handles, xs, y, rhs, obj_weight, sx, sc, precond, out, workspaces)
    n = ph.ranks[0].w.layout.n
    infos = ph.solve(float(rtol), int(5 * n if max_iter is None else max_iter), int(check_every), on_chunk)
    return [r.z for r in ph.ranks], infos


def kkt_schur_cr_joint_shards(handles, jvals, px, pc, sc):
    """The joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*) over shard handles that are ALL in this
    process, in ascending order of their steps, on one GPU and one stream (torch's current one): every rank's local factor, the
    all-gather of the factor records as device copies, every rank's join.  jvals, px, pc, sc: full-length tensors shared by the
    shards, or one per shard (a list); a shard's jvals must be valid on its own range and on the halo its layout names.  Returns one
    SchurCrJointPrecond per shard, for `kkt_schur_cr_joint_apply_shards`."""
    G = len(handles)
    per = lambda a: list(a) if isinstance(a, (list, tuple)) else [a] * G      # noqa: E731
    jv, pxs, pcs, scs = per(jvals), per(px), per(pc), per(sc)
    cur = torch.cuda.current_stream(pxs[0].device).cuda_stream
    for h in handles:
        if h._stream_raw != cur:
            h.set_stream(cur)
    Ps = [h.kkt_schur_cr_joint_factor_local(jv[k], pxs[k], pcs[k], scs[k], G, k) for k, h in enumerate(handles)]
    if G == 1:
        return Ps
    gathered = torch.cat([P.send for P in Ps])
    for h, P in zip(handles, Ps):
        h.kkt_schur_cr_joint_factor_join(P, gathered)
    return Ps


def kkt_schur_cr_joint_apply_shards(handles, Ps, r, out=None):
    """out = T^-1 r on the block rows with the factors of `kkt_schur_cr_joint_shards`: every rank's local solve, the all-gather of the
    solve records as device copies, every rank's join.  r: ncon entries, shared by the shards or one per shard (a rank reads its own
    block rows); out: one tensor of ncon entries -- every rank writes its own block rows of it, the tail rows are left untouched -- or
    one per shard; zeros when None.  Enqueue-only but for the allocation; returns out."""
    G = len(handles)
    rs = list(r) if isinstance(r, (list, tuple)) else [r] * G
    if out is None:
        out = torch.zeros_like(rs[0])
    outs = list(out) if isinstance(out, (list, tuple)) else [out] * G
    for k, (h, P) in enumerate(zip(handles, Ps)):
        h.kkt_schur_cr_joint_solve_local(P, rs[k], outs[k])
    if G > 1:
        gathered = torch.cat([P.xsend for P in Ps])
        for k, (h, P) in enumerate(zip(handles, Ps)):
            h.kkt_schur_cr_joint_solve_join(P, gathered, outs[k], sync=False)
    return out


class ShardedDOCP:
    """One rank's view of a grid-sharded transcription.  `make_docp(steps=(begin, end))` builds the engine handle
    (ctdirect DOCP) for the rank's block of steps."""

    def __init__(self, make_docp, N, world=None, rank=None, group=None):
        self.world = dist.get_world_size(group) if world is None else world
        self.rank = dist.get_rank(group) if rank is None else rank
        self.group = group
        self.N = N
        self.steps = shard_steps(N, self.world, self.rank)
        self.docp = make_docp(steps=self.steps)
        d = self.docp
        disc = d.discretization
        self.blk, self.cb, _, self.n, self.m, self.halo_w = _shard_dims(d)                   # (halo_w: trapeze: the next node's control too)
        # one-point schemes (midpoint, Euler): the residual of the step BEFORE this rank's first one depends on this rank's
        # first state, and the rank owns those Jacobian entries: it needs that step's block too
        self.halo_lo = self.blk if (disc.stage == 0 and not getattr(disc, "_final_control", False)) else 0
        self._dev = None
        self._stream = None
        if d.device is not None and d.device >= 0:
            self._dev = torch.device("cuda", d.device)
            self._rebind()                  # launch on torch's current stream: ordered with the collectives issued here
        self._stitch = None
        self._halo = None
        self._yhalo = None
        self._phalo = {}                    # (layout, device) -> index sets and buffers of exchange_product_halo / _rows
        self._vv = None
        self._f = None
        self._minres_ws = {}                # the workspaces of `kkt_minres`, kept between solves: one per phase family
        self._peer = None                   # data_ptr of the x buffer the peer table is ACTIVE for (enable_peer_x), None: off
        self._peer_tables = {}              # x data_ptr -> (the tensor itself, mapped pointers of the other ranks' buffers): the
                                            # tensor is kept alive so the allocator cannot hand its address to another buffer
                                            # while the other ranks still hold a mapping of it
        self._ipc_bases = []                # (device, base) of every IPC mapping this object opened
        self._bind_gen = 0                  # bumped whenever the handle's iterate mode changes: bound callables re-assert theirs

    def _rebind(self):
        """The engine's kernels and the collectives issued here must share a stream: follow torch's current stream (a cheap
        integer compare per call; a caller inside `with torch.cuda.stream(s)` or a graph capture gets both on s)."""
        if self._dev is None:
            return
        cur = torch.cuda.current_stream(self._dev).cuda_stream
        if cur != self._stream:
            self.docp.set_stream(cur)
            self._stream = cur

    # ---- iterate distribution ------------------------------------------------------------------------------------------
    def owned_variables(self):
        """[begin, end) of the entries of x this rank owns: the blocks of its own steps; the last rank also the final state
        (+ final control) -- the optimisation variables v at the tail are replicated on every rank."""
        b, e = self.steps
        end = e * self.blk
        if self.rank == self.world - 1:
            end = self.docp.dim_NLP_variables - self.docp.dims.NLP_v
        return b * self.blk, end

    def exchange_halo(self, x):
        """Sharded iterate: fills, inside this rank's full-length x, the few entries other ranks own that its rows and its
        Jacobian columns read -- the next rank's first node (X, + U for trapeze); for the one-point schemes (midpoint, Euler)
        the previous rank's last step block, whose residual depends on this rank's first state; X_1 and X_{N+1} (boundary rows,
        Mayer cost) -- with ONE all-gather of (halo_w + low + n) doubles per rank.  v is replicated by the solver and not
        touched.  Three small kernels around the collective: pack (index_select), unpack (index_select + index_copy_)."""
        if self.world == 1 and not _FORCE:
            return x
        if self._halo is None:
            w, n, blk, N, lo = self.halo_w, self.n, self.blk, self.N, self.halo_lo
            L = w + lo + n
            b, e = self.steps
            r, G = self.rank, self.world
            ar = torch.arange
            pack = torch.cat([b * blk + ar(w), (e - 1) * blk + ar(lo), N * blk + ar(n)])      # my first node | last block | final state
            dst, src = [], []
            if r + 1 < G:
                dst += [e * blk + ar(w), N * blk + ar(n)]
                src += [(r + 1) * L + ar(w), (G - 1) * L + w + lo + ar(n)]
            if r > 0:
                if lo:
                    dst.append((b - 1) * blk + ar(lo))
                    src.append((r - 1) * L + w + ar(lo))
                dst.append(ar(n))
                src.append(ar(n))
            empty = torch.zeros(0, dtype=torch.long)
            self._halo = (pack.to(x.device), (torch.cat(dst) if dst else empty).to(x.device), (torch.cat(src) if src else empty).to(x.device),
                          torch.zeros(L, dtype=torch.float64, device=x.device), torch.zeros(G * L, dtype=torch.float64, device=x.device))
        pack, dst, src, send, recv = self._halo
        torch.index_select(x, 0, pack, out=send)
        _all_gather_into(recv, send, self.group)
        if dst.numel():
            x.index_copy_(0, dst, recv.index_select(0, src))
        return x

    def owned_constraints(self):
        """[begin, end) of the rows of c -- and of the multipliers y -- this rank owns: the rows of its own steps; the last rank also
        the tail (final path rows + boundary rows), as in `stitch_constraints`."""
        b, e = self.steps
        return b * self.cb, (self.docp.dim_NLP_constraints if self.rank == self.world - 1 else e * self.cb)

    def exchange_multipliers(self, y):
        """Sharded multipliers for `hess_coord`: fills, inside this rank's full-length y, the rows other ranks own that its Hessian
        entries read -- the PREVIOUS rank's last step (the second-order terms of that step's defect in this rank's first node:
        trapeze, midpoint, implicit Euler; the Gauss-Legendre schemes read none) and the tail rows (final path + boundary
        multipliers, owned by the last rank) -- with ONE all-gather of (cb + tail) doubles per rank, instead of a replicated y
        (an all-gather of all ncon rows).  Entries: /root/reference/src/DOCP_functions.jl:80-140 rows, multiplied into the
        Lagrangian by hess_coord!(nlp, x, y, vals; obj_weight)."""
        if self.world == 1 and not _FORCE:
            return y
        if self._yhalo is None:
            cb, N = self.cb, self.N
            tail = self.docp.dim_NLP_constraints - N * cb
            b, e = self.steps
            r, G = self.rank, self.world
            ar = torch.arange
            Ly = cb + tail
            pack = torch.cat([(e - 1) * cb + ar(cb), N * cb + ar(tail)])            # my last step | the tail (meaningful on the last rank)
            dst, src = [], []
            if r > 0:
                dst.append((b - 1) * cb + ar(cb))
                src.append((r - 1) * Ly + ar(cb))
            if r + 1 < G and tail:
                dst.append(N * cb + ar(tail))
                src.append((G - 1) * Ly + cb + ar(tail))
            empty = torch.zeros(0, dtype=torch.long)
            self._yhalo = (pack.to(y.device), (torch.cat(dst) if dst else empty).to(y.device), (torch.cat(src) if src else empty).to(y.device),
                           torch.zeros(Ly, dtype=torch.float64, device=y.device), torch.zeros(G * Ly, dtype=torch.float64, device=y.device))
        pack, dst, src, send, recv = self._yhalo
        torch.index_select(y, 0, pack, out=send)
        _all_gather_into(recv, send, self.group)
        if dst.numel():
            y.index_copy_(0, dst, recv.index_select(0, src))
        return y

    def _exchange(self, t, key, build):
        """One all-gather of a few entries per rank: every rank packs `pack` of its own entries of the full-length t, and copies
        the entries `src` of the gathered buffer to the positions `dst` of t.  build() -> (pack, dst, src) as index lists, made
        once per (key, device) and kept with the send / receive buffers."""
        if self.world == 1 and not _FORCE:
            return t
        ent = self._phalo.get((key, t.device))
        if ent is None:
            pack, dst, src = build()
            cat = lambda parts: (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.long)).to(t.device)      # noqa: E731
            n = sum(int(q.numel()) for q in pack)
            ent = self._phalo[(key, t.device)] = (cat(pack), cat(dst), cat(src), torch.zeros(n, dtype=torch.float64, device=t.device),
                                                  torch.zeros(self.world * n, dtype=torch.float64, device=t.device))
        pack, dst, src, send, recv = ent
        torch.index_select(t, 0, pack, out=send)
        _all_gather_into(recv, send, self.group)
        if dst.numel():
            t.index_copy_(0, dst, recv.index_select(0, src))
        return t

    def exchange_product_halo(self, t):
        """Matrix-free products on a shard: fills, inside this rank's full-length VARIABLE-layout tensor t (a direction v, or the
        iterate x when it is not read in place), the entries other ranks own that `jprod` / `jtprod` / `hprod` read (the read set of
        ctd_*prod_shard_dev_async, include/ctdirect_hip.h): the previous rank's whole last block, the next rank's first node (X, + U
        for trapeze), X_1 and X_{N+1} -- with ONE all-gather of (halo_w + blk + n) doubles per rank.  The nv tail is replicated and
        not touched."""
        def build():
            w, n, blk, N = self.halo_w, self.n, self.blk, self.N
            L = w + blk + n
            (b, e), r, G, ar = self.steps, self.rank, self.world, torch.arange
            pack = [b * blk + ar(w), (e - 1) * blk + ar(blk), N * blk + ar(n)]        # my first node | last block | final state
            dst, src = [], []
            if r > 0:
                # (rank 1 of one-step-first shards: block b - 1 is block 0 and holds X_1 too -- index_copy_ then gets those n
                # positions twice, with the same values from the same rank)
                dst += [ar(n), (b - 1) * blk + ar(blk)]
                src += [ar(n), (r - 1) * L + w + ar(blk)]
            if r + 1 < G:
                dst += [e * blk + ar(w), N * blk + ar(n)]
                src += [(r + 1) * L + ar(w), (G - 1) * L + w + blk + ar(n)]
            return pack, dst, src
        return self._exchange(t, "var", build)

    def exchange_product_rows(self, w):
        """The same for a CONSTRAINT-layout tensor (w of `jtprod`, y of `hprod`): the state / stage rows of the previous rank's last
        step, the path rows of the next rank's first node and the tail rows (final path + boundary rows, owned by the last rank) --
        ONE all-gather of (cb + tail) doubles per rank."""
        def build():
            cb, N = self.cb, self.N
            eqs = self.docp.discretization._state_stage_eqs_block
            p = cb - eqs
            tail = self.docp.dim_NLP_constraints - N * cb
            Ly = p + eqs + tail
            (b, e), r, G, ar = self.steps, self.rank, self.world, torch.arange
            pack = [b * cb + eqs + ar(p), (e - 1) * cb + ar(eqs), N * cb + ar(tail)]  # my first node's path rows | last step | tail
            dst, src = [], []
            if r > 0:
                dst.append((b - 1) * cb + ar(eqs))
                src.append((r - 1) * Ly + p + ar(eqs))
            if r + 1 < G:
                dst += [e * cb + eqs + ar(p), N * cb + ar(tail)]
                src += [(r + 1) * Ly + ar(p), (G - 1) * Ly + p + eqs + ar(tail)]
            return pack, dst, src
        return self._exchange(w, "con", build)

    def exchange_kkt_halo(self, dx, dy):
        """`exchange_product_halo(dx)` and `exchange_product_rows(dy)` in ONE all-gather of (halo_w + blk + n) + (cb + tail) doubles
        per rank: the two halves of a Krylov vector -- usually one buffer -- need their halos at the same moment, once per inner
        iteration, and a second collective would cost a second latency.  Fills exactly the read sets of
        ctd_kktprod_shard_dev_async (include/ctdirect_hip.h) inside the full-length dx (variable layout) and dy (constraint
        layout); returns (dx, dy)."""
        if self.world == 1 and not _FORCE:
            return dx, dy
        ent = self._phalo.get(("kkt", dx.device))
        if ent is None:
            w, n, blk, N, cb = self.halo_w, self.n, self.blk, self.N, self.cb
            eqs = self.docp.discretization._state_stage_eqs_block
            p = cb - eqs
            tail = self.docp.dim_NLP_constraints - N * cb
            Lx = w + blk + n
            L = Lx + p + eqs + tail
            (b, e), r, G, ar = self.steps, self.rank, self.world, torch.arange
            # my first node | last block | final state || my first node's path rows | last step's state / stage rows | tail
            pack_x = [b * blk + ar(w), (e - 1) * blk + ar(blk), N * blk + ar(n)]
            pack_c = [b * cb + eqs + ar(p), (e - 1) * cb + ar(eqs), N * cb + ar(tail)]
            # where the entries go: the read set, stated once (rank r > 0 <=> b > 0, r + 1 < G <=> e < N); where they come from
            lo_x, hi_x, lo_c, hi_c = _kkt_halo_ranges(b, e, N, n, w, blk, cb, eqs, self.docp.dim_NLP_constraints)
            at = lambda ranges: [s + ar(k) for s, k in ranges]      # noqa: E731
            dst_x, dst_c, src_x, src_c = at(lo_x) + at(hi_x), at(lo_c) + at(hi_c), [], []
            if r > 0:
                src_x += [ar(n), (r - 1) * L + w + ar(blk)]
                src_c.append((r - 1) * L + Lx + p + ar(eqs))
            if r + 1 < G:
                src_x += [(r + 1) * L + ar(w), (G - 1) * L + w + blk + ar(n)]
                src_c += [(r + 1) * L + Lx + ar(p), (G - 1) * L + Lx + p + eqs + ar(tail)]
            cat = lambda parts: (torch.cat(parts) if parts else torch.zeros(0, dtype=torch.long)).to(dx.device)      # noqa: E731
            ent = self._phalo[("kkt", dx.device)] = (cat(pack_x), cat(pack_c), cat(dst_x), cat(src_x), cat(dst_c), cat(src_c), Lx,
                                                     torch.zeros(L, dtype=torch.float64, device=dx.device),
                                                     torch.zeros(G * L, dtype=torch.float64, device=dx.device))
        pack_x, pack_c, dst_x, src_x, dst_c, src_c, Lx, send, recv = ent
        torch.index_select(dx, 0, pack_x, out=send[:Lx])
        torch.index_select(dy, 0, pack_c, out=send[Lx:])
        _all_gather_into(recv, send, self.group)
        if dst_x.numel():
            dx.index_copy_(0, dst_x, recv.index_select(0, src_x))
        if dst_c.numel():
            dy.index_copy_(0, dst_c, recv.index_select(0, src_c))
        return dx, dy

    def enable_peer_x(self, x):
        """Sharded iterate read IN PLACE (`ctd_set_x_shards`): every rank exports its full-length x buffer once (IPC handle,
        all-gathered as Python objects -- set-up, not the step), maps the other ranks' buffers, and from then on this rank's
        constraint / Jacobian kernels load the few entries its neighbours own (next rank's first node, previous rank's last
        block, X_1, X_{N+1}) straight from their HBM over xGMI.  The evaluation of a step then contains NO collective, no
        pack / unpack kernel and no copy.  `x` must stay the iterate buffer (same storage) for the life of this object; the
        solver's update of x on every rank has to be complete before the evaluations that follow it are enqueued (its step
        acceptance is a collective anyway).  The shard table is state of the HANDLE: while it is active, `cons_jac`, `obj` and
        `hess_coord` and `grad` read the neighbours' entries in place too and must be given this same x (anything else raises);
        `docp.grad` (the C ABI's ctd_grad*) stays the whole objective's gradient and needs an all-gathered x.  `disable_peer_x`
        (or binding another x_mode) switches back."""
        from . import _lib
        import ctypes as C
        if self.world == 1:
            return x
        begins = [shard_steps(self.N, self.world, r)[0] for r in range(self.world)] + [self.N]
        if self._peer == x.data_ptr():
            return x
        if x.data_ptr() in self._peer_tables:            # mapped before (the caller alternates between modes)
            self.docp.set_x_shards(begins, self._peer_tables[x.data_ptr()][1], self.rank)
            self._peer = x.data_ptr()
            self._bind_gen += 1
            return x
        L = _lib.lib()
        dev = x.device.index
        hbuf = (C.c_ubyte * 64)()
        off = C.c_int64()
        # Every rank goes through the same collectives whatever fails locally (a rank that raised early would leave the
        # others waiting): errors are collected, agreed on with one all-reduce, and raised on EVERY rank together.
        err = None
        st = L.ctd_ipc_export(dev, C.c_void_p(x.data_ptr()), hbuf, C.byref(off))
        if st:
            err = "ctd_ipc_export: " + L.ctd_last_error(None).decode()
        mine = (bytes(hbuf), int(off.value), os.getpid(), int(x.data_ptr()), err is None)
        everyone = [None] * self.world
        dist.all_gather_object(everyone, mine, group=self.group)
        ptrs, opened = [], []
        if all(e[4] for e in everyone):
            for r, (hb, o, pid, raw, _) in enumerate(everyone):
                if r == self.rank:
                    ptrs.append(0)
                elif pid == os.getpid():      # same process (several ranks of a test harness): the pointer is valid as it is
                    ptrs.append(raw)
                else:
                    base = C.c_void_p()
                    st = L.ctd_ipc_open(dev, (C.c_ubyte * 64).from_buffer_copy(hb), C.byref(base))
                    if st:
                        err = f"ctd_ipc_open (rank {r}'s buffer): " + L.ctd_last_error(None).decode()
                        break
                    opened.append((dev, base.value))
                    ptrs.append(base.value + o)
                    # one read through the mapping by a plain device copy: an unreachable mapping is an error here, not a fault
                    # inside the evaluation kernel
                    if L.ctd_ipc_probe(dev, C.c_void_p(base.value + o), 8):
                        err = f"ctd_ipc_probe (rank {r}'s buffer): " + L.ctd_last_error(None).decode()
                        break
        elif err is None:
            err = "another rank could not export its buffer"
        flat = str(dist.get_backend(self.group)).lower() in ("nccl", "rccl")
        ok = torch.tensor([0.0 if err else 1.0], dtype=torch.float64, device=x.device if flat else "cpu")
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)     # also: every rank has mapped the others before anyone evaluates
        if ok.item() != 1.0:
            for d_, b_ in opened:
                L.ctd_ipc_close(d_, b_)
            raise RuntimeError("enable_peer_x: " + (err or "another rank could not map the buffers"))
        self._ipc_bases += opened
        self.docp.set_x_shards(begins, ptrs, self.rank)
        self._peer_tables[x.data_ptr()] = (x, ptrs)
        self._peer = x.data_ptr()
        self._bind_gen += 1
        return x

    def disable_peer_x(self):
        """Back to "the x passed to a call holds everything the rank reads" (the mappings stay open for a later enable_peer_x)."""
        if self._peer is not None:
            self.docp.set_x_shards(None, None, 0)
            self._peer = None
            self._bind_gen += 1

    def _check_peer(self, x, what):
        """While the shard table is active the kernels take a rank's own entries from the x of the call and its neighbours'
        entries from the buffers registered with enable_peer_x: any other x would silently mix two iterates."""
        if self._peer is not None and torch.is_tensor(x) and x.data_ptr() != self._peer:
            raise ValueError(f"ShardedDOCP.{what}: the sharded iterate is read in place from the buffers registered with "
                             "enable_peer_x; pass that same x, or call disable_peer_x() first")

    def broadcast_iterate(self, x, src=0):
        """Replicated iterate: the rank that holds the new x sends all of it (nvar doubles) to every other rank."""
        if self.world > 1 or _FORCE:
            dist.broadcast(x, src=src, group=self.group)
        return x

    # ---- callbacks -------------------------------------------------------------------------------------------------------
    def _stitcher(self, c):
        if self._stitch is None:
            self._stitch = _Stitcher(self.N, self.cb, c.numel(), self.world, self.rank, c.device, self.group)
        return self._stitch

    def cons_jac(self, x, c, vals, stitch=True):
        """Evaluate this rank's rows into the full-length c / vals buffers; `stitch`: all-gather the row blocks of c so that
        every rank holds the whole residual (the Jacobian values always stay sharded)."""
        self._rebind()
        self._check_peer(x, "cons_jac")
        self.docp.cons_jac(x, c, vals, sync=False)
        if stitch:
            self._stitcher(c)(c)
        return c, vals

    def bind_cons_jac(self, x, c, vals, stitch=True, x_mode=None):
        """Zero-argument callable for a solver loop, pointers pre-bound: [distribute the iterate: x_mode "peer" (sharded x,
        neighbours' entries read in place by the kernel: nothing per step) / "halo" (sharded x, exchange_halo: one all-gather) /
        "broadcast" (replicated x from rank 0) / None] + enqueue this rank's evaluation [+ the all-gather of c
        when `stitch`]."""
        self._rebind()
        launch = self.docp.bind_cons_jac(x, c, vals, sync=False)
        if self.world == 1 and not _FORCE:
            return launch
        def assert_mode():                   # (the shard table is per-handle state: the callable bound LAST owns it ...)
            if x_mode == "peer":             # neighbours' entries are read in place by the kernel: nothing precedes the launch
                self.enable_peer_x(x)        # (first time: collective set-up; afterwards a table lookup)
            else:
                self.disable_peer_x()
            return self._bind_gen
        gen = [assert_mode()]
        pre = {None: None, "peer": None, "halo": self.exchange_halo, "broadcast": self.broadcast_iterate}[x_mode]
        post = self._stitcher(c) if stitch else None

        def call():
            if gen[0] != self._bind_gen:     # (... and an older callable that runs again puts its own mode back first)
                gen[0] = assert_mode()
            if pre is not None:
                pre(x)
            launch()
            if post is not None:
                post(c)
        return call

    def hess_coord(self, x, y, obj_weight, vals):
        """This rank's entries of hess_coord!(nlp, x, y, vals; obj_weight) into the full-length `vals` (they stay sharded like
        the Jacobian values), plus the all-reduced variable x variable entries on every rank.  No host synchronisation: the
        kernel and the all-reduce are ordered on torch's current stream.  `y` is full-length; only this rank's own rows, the
        previous rank's last step and the tail rows are read (`exchange_multipliers` fills the latter two of a sharded y)."""
        self._rebind()
        self._check_peer(x, "hess_coord")
        self.docp.hess_coord(x, y, obj_weight, vals, sync=False)
        if self.world > 1 or _FORCE:
            if self._vv is None:
                self._vv = torch.as_tensor(self.docp.hess_shard_info()[2], dtype=torch.long, device=vals.device)
            reduce_hessian_vv(vals, self._vv, self.group)
        return vals

    def grad(self, x, g):
        """grad!(nlp, x, g) of the sharded transcription: this rank's own entries of g (its step blocks; the last rank also the
        final state) into the full-length g, from the sharded iterate read in place (or with copied halos) -- no all-gathered x --
        plus ONE all-reduce of the nv entries of d/dv, which sum over every step.  Entries other ranks own are left untouched."""
        self._rebind()
        self._check_peer(x, "grad")
        self.docp.grad_shard(x, g)
        nv = self.docp.dims.NLP_v
        if nv and (self.world > 1 or _FORCE):
            tail = g[g.numel() - nv:]
            dist.all_reduce(tail, op=dist.ReduceOp.SUM, group=self.group)
        return g

    def _product_x(self, x, what, x_halo_valid):
        """the iterate of a product: read in place when the peer table is active for it; otherwise its halo entries are copied
        INTO the caller's x (one all-gather), unless the caller says they are already there"""
        self._rebind()
        self._check_peer(x, what)
        if self._peer is None and not x_halo_valid:
            self.exchange_product_halo(x)

    def _reduce_tail(self, out):
        nv = self.docp.dims.NLP_v
        if nv and (self.world > 1 or _FORCE):
            dist.all_reduce(out[out.numel() - nv:], op=dist.ReduceOp.SUM, group=self.group)
        return out

    def jprod(self, x, v, out, stitch=False, x_halo_valid=False):
        """jprod!(nlp, x, v, Jv) of the sharded transcription: this rank's rows of J(x) v (its step rows; the last rank also the tail
        rows) into the full-length `out`, other rows untouched.  x, v: full-length tensors of which this rank holds its own entries
        and the nv tail; the halo of v (and of x, unless x is read in place: `enable_peer_x`) is exchanged here -- one small
        all-gather each -- and written INTO v and x: both are modified outside the rank's own entries.  x does not change between
        the products of one outer iteration: after the first product (or one `exchange_product_halo(x)`) pass
        `x_halo_valid=True` to skip its all-gather.  `stitch`: all-gather the row blocks so that every rank holds the whole Jv."""
        self._product_x(x, "jprod", x_halo_valid)
        self.exchange_product_halo(v)
        self.docp.jprod_shard(x, v, out)
        if stitch:
            self._stitcher(out)(out)
        return out

    def jtprod(self, x, w, out, x_halo_valid=False):
        """jtprod!(nlp, x, w, Jtw) of the sharded transcription: the entries of J(x)' w of this rank's own variables into the
        full-length `out`, plus the d/dv entries all-reduced (nv doubles) on every rank.  w: full-length, this rank's own rows
        valid; its halo rows are exchanged here (one small all-gather, written into w), and x's as in `jprod`
        (`x_halo_valid`)."""
        self._product_x(x, "jtprod", x_halo_valid)
        self.exchange_product_rows(w)
        self.docp.jtprod_shard(x, w, out)
        return self._reduce_tail(out)

    def hprod(self, x, y, v, obj_weight, out, x_halo_valid=False):
        """hprod!(nlp, x, y, v, Hv; obj_weight) of the sharded transcription (y = None: objective only): the entries of Hv of this
        rank's own variables into the full-length `out`, plus the d/dv entries all-reduced on every rank.  Exchanges the halos of v
        and y (two small all-gathers, written into v and y), and of x as in `jprod` (`x_halo_valid`)."""
        self._product_x(x, "hprod", x_halo_valid)
        self.exchange_product_halo(v)
        if y is not None:
            self.exchange_product_rows(y)
        self.docp.hprod_shard(x, y, v, obj_weight, out)
        return self._reduce_tail(out)

    def kktprod(self, x, y, dx, dy, obj_weight, sx, sc, out, x_halo_valid=False, y_halo_valid=False):
        """The fused KKT product (`DOCP.kktprod`) of the sharded transcription: into the full-length pair `out` = (rx, rc) go the
        entries of rx of this rank's own variables, the v entries all-reduced (nv doubles) on every rank, and this rank's rows of rc;
        everything else is left untouched.  Every tensor is full-length with this rank's own entries valid (x, dx: + the nv tail; sx:
        the nv tail on the last rank only; y, sx, sc may be None).  The halos of dx and dy are exchanged here with ONE all-gather
        (`exchange_kkt_halo`) and written INTO them; x as in `jprod` (`x_halo_valid`); y's halo rows are exchanged
        (`exchange_product_rows`) unless `y_halo_valid` -- y, like x, is fixed over the inner iterations of one outer step.  With x
        read in place (or valid) and y valid, a Krylov iteration costs two launches, one all-gather and one all-reduce."""
        self._product_x(x, "kktprod", x_halo_valid)
        if y is not None and not y_halo_valid:
            self.exchange_product_rows(y)
        self.exchange_kkt_halo(dx, dy)
        self.docp.kktprod_shard(x, y, dx, dy, obj_weight, sx, sc, out)
        self._reduce_tail(out[0])
        return out

    def hdiag(self, x, y, obj_weight, out, x_halo_valid=False, y_halo_valid=False):
        """`DOCP.hdiag` of the sharded transcription (y = None: objective only): the entries of diag(H) of this rank's own variables
        into the full-length `out`, plus the nv entries all-reduced on every rank.  y's halo rows are exchanged
        (`exchange_product_rows`, written into y) unless `y_halo_valid`; x as in `jprod` (`x_halo_valid`)."""
        self._product_x(x, "hdiag", x_halo_valid)
        if y is not None and not y_halo_valid:
            self.exchange_product_rows(y)
        self.docp.hdiag_shard(x, y, obj_weight, out)
        return self._reduce_tail(out)

    def jsq_cols(self, x, wc, out, x_halo_valid=False):
        """`DOCP.jsq_cols` of the sharded transcription (wc = None: ones): the entries of diag(J' diag(wc) J) of this rank's own
        variables into the full-length `out`, plus the nv entries all-reduced on every rank.  wc: full-length, this rank's own rows
        valid; its halo rows are exchanged here (written into wc); x as in `jprod` (`x_halo_valid`)."""
        self._product_x(x, "jsq_cols", x_halo_valid)
        if wc is not None:
            self.exchange_product_rows(wc)
        self.docp.jsq_cols_shard(x, wc, out)
        return self._reduce_tail(out)

    def jsq_rows(self, x, wx, out, x_halo_valid=False):
        """`DOCP.jsq_rows` of the sharded transcription (wx = None: ones): this rank's rows of diag(J diag(wx) J') into the
        full-length `out`, other rows untouched; every row sum is complete, nothing is reduced.  wx: full-length, this rank's own
        entries and the nv tail valid; its halo is exchanged here (written into wx); x as in `jprod` (`x_halo_valid`)."""
        self._product_x(x, "jsq_rows", x_halo_valid)
        if wx is not None:
            self.exchange_product_halo(wx)
        self.docp.jsq_rows_shard(x, wx, out)
        return out

    def kkt_diag_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, floor=1e-8, x_halo_valid=False, y_halo_valid=False):
        """`DOCP.kkt_diag_precond` of the sharded transcription: returns the full-length pair (px, pc) of which this rank's own
        entries -- and the nv tail of px, replicated -- are valid:
            px = max(|hdiag(x, y, obj_weight) + sx|, floor),   pc = jsq_rows(x, 1 / px) + sc
        Every input is full-length with this rank's own entries valid (x: + the nv tail; sx: the nv tail on the last rank only, the
        convention of `kktprod`; y, sx, sc may be None).  The last rank adds the tail of sx to its partial sums of the nv entries
        before they are all-reduced.  Three launches, one all-reduce of nv doubles and one small all-gather (the halo of 1 / px),
        besides the halos of x and y (`x_halo_valid`, `y_halo_valid`: as in `kktprod`)."""
        d = self.docp
        nvar, nv = d.dim_NLP_variables, d.dims.NLP_v
        lo, hi = self.owned_variables()
        self._product_x(x, "kkt_diag_precond", x_halo_valid)
        if y is not None and not y_halo_valid:
            self.exchange_product_rows(y)
        px = d.hdiag_shard(x, y, obj_weight)
        own = px[lo:hi]
        if sx is not None:
            own += sx[lo:hi]
            if nv and self.rank == self.world - 1:
                px[nvar - nv:] += sx[nvar - nv:]
        self._reduce_tail(px)
        torch.clamp_min(torch.abs_(own), floor, out=own)
        if nv:
            tail = px[nvar - nv:]
            torch.clamp_min(torch.abs_(tail), floor, out=tail)
        wx = torch.empty_like(px)
        torch.reciprocal(own, out=wx[lo:hi])
        if nv:
            torch.reciprocal(px[nvar - nv:], out=wx[nvar - nv:])
        self.exchange_product_halo(wx)
        pc = d.jsq_rows_shard(x, wx)
        if sc is not None:
            r0, r1 = self.owned_constraints()
            pc[r0:r1] += sc[r0:r1]
        return px, pc

    def kkt_schur_cr_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, floor=1e-8, jvals=None, x_halo_valid=False,
                             y_halo_valid=False):
        """`DOCP.kkt_schur_cr_precond` of the sharded transcription: the log-depth Schur preconditioner, exact inside this rank's
        steps and cut at the rank boundaries -- M^-1 = blkdiag(diag(px), T_0, ..., T_{G-1}, diag(pc_tail)), T_r the principal
        submatrix of T = Jt diag(1 / px) Jt' + Sc on rank r's blocks; each of the G - 1 cuts drops one coupling block.  Built from
        this rank's own Jacobian values on a CSR handle (`jvals`: full-length, this rank's rows valid; None: evaluated here),
        `kkt_diag_precond` and ONE halo exchange of px (`exchange_product_halo`: the next rank's first node); the factor needs no
        collective.  Returns the SchurCrShardPrecond for `kkt_minres(precond=P)`.  Inputs as `kkt_diag_precond`."""
        px, pc, jvals = self._schur_cr_inputs(x, y, obj_weight, sx, sc, floor, jvals, x_halo_valid, y_halo_valid)
        return self.docp.kkt_schur_cr_shard_factor(jvals, px, pc, sc)

    def _schur_cr_inputs(self, x, y, obj_weight, sx, sc, floor, jvals, x_halo_valid, y_halo_valid):
        """what both forms of the log-depth Schur preconditioner are factored from: the pair of `kkt_diag_precond`, px with its halo
        (the next rank's first node), this rank's Jacobian values (evaluated here when None)"""
        d = self.docp
        px, pc = self.kkt_diag_precond(x, y, obj_weight, sx, sc, floor, x_halo_valid, y_halo_valid)
        self.exchange_product_halo(px)
        if jvals is None:
            jvals = torch.empty(d.nnzj, dtype=torch.float64, device=x.device)
            c = torch.empty(d.dim_NLP_constraints, dtype=torch.float64, device=x.device)
            self.cons_jac(x, c, jvals, stitch=False)
        return px, pc, jvals

    def exchange_jvals_block_halo(self, jvals):
        """The joined form of the Schur preconditioner: fills, inside this rank's full-length Jacobian values (CSR order), the values
        of the rows of block `step_end` -- the next rank's first block, which E[b] = T(step_end, step_end - 1) reads
        (`ctd_kkt_schur_cr_joint_layout`: [jvals_halo_begin, jvals_halo_end)) -- with ONE all-gather, shaped like
        `exchange_product_halo`: every rank sends the values of the rows of its own first block, padded to the longest block of
        the grid so that all ranks send alike."""
        def build():
            d = self.docp
            rowptr = np.empty(d.dim_NLP_constraints + 1, dtype=np.int64)
            colind = np.empty(d.nnzj, dtype=np.int64)
            d._ck(_lib.lib().ctd_jac_csr(d._h, rowptr.ctypes.data_as(C.POINTER(C.c_int64)), colind.ctypes.data_as(C.POINTER(C.c_int64))))
            m = int(d.kkt_schur_cr_shard_layout().block_rows)
            (b, e), r, G, N, ar = self.steps, self.rank, self.world, self.N, torch.arange
            L = int(max(rowptr[(k + 1) * m] - rowptr[k * m] for k in range(N)))
            pack = [torch.clamp(int(rowptr[b * m]) + ar(L), max=d.nnzj - 1)]        # (the padding repeats the last value: never read)
            dst, src = [], []
            if r + 1 < G:
                Lh = int(rowptr[(e + 1) * m] - rowptr[e * m])
                dst, src = [int(rowptr[e * m]) + ar(Lh)], [(r + 1) * L + ar(Lh)]
            return pack, dst, src
        return self._exchange(jvals, "jvals_block", build)

    def kkt_schur_cr_joint_precond(self, x, y, obj_weight=1.0, sx=None, sc=None, floor=1e-8, jvals=None, x_halo_valid=False,
                                   y_halo_valid=False):
        """`kkt_schur_cr_precond` with the couplings across the ranks restored (`ctd_kkt_schur_cr_joint_*`): T^-1 itself on the block
        rows.  Every rank but the first gives up its first block as a separator (it needs at least two steps).  Built like
        `kkt_schur_cr_precond`, with TWO more collectives, at factor time only: one small halo exchange of the Jacobian values
        (`exchange_jvals_block_halo`) and one all-gather of the factor records, after which every rank factors the same reduced
        system.  Returns the SchurCrJointPrecond for `kkt_minres(precond=P)`.  Inputs as `kkt_diag_precond`."""
        d = self.docp
        px, pc, jvals = self._schur_cr_inputs(x, y, obj_weight, sx, sc, floor, jvals, x_halo_valid, y_halo_valid)
        self.exchange_jvals_block_halo(jvals)
        cur = torch.cuda.current_stream(x.device).cuda_stream
        if d._stream_raw != cur:
            d.set_stream(cur)
        P = d.kkt_schur_cr_joint_factor_local(jvals, px, pc, sc, self.world, self.rank)
        if self.world > 1:
            gathered = torch.empty(self.world * P.layout.factor_slot, dtype=torch.float64, device=x.device)
            _all_gather_into(gathered, P.send, self.group)
            d.kkt_schur_cr_joint_factor_join(P, gathered)
        return P

    def kkt_minres(self, x, y, rhs, obj_weight=1.0, sx=None, sc=None, precond=None, rtol=1e-10, max_iter=None, check_every=16,
                   out=None, x_halo_valid=False, y_halo_valid=False):
        """`DOCP.kkt_minres` of the sharded transcription: preconditioned MINRES on K z = rhs with K the operator of `kktprod`,
        device-resident, every rank working on its own entries of the Krylov vectors (`ctd_kkt_minres_shard_*`).  Every tensor
        is full-length with this rank's own entries valid (x, rhs, px: + the nv tail; sx: the nv tail on the last rank only; y, sx,
        sc may be None).  precond: None, a pair (px, pc), or "diag": the pair of `kkt_diag_precond`; a SchurCrShardPrecond P of
        `kkt_schur_cr_precond`, or "schur_cr": that of `kkt_schur_cr_precond(x, y, obj_weight, sx, sc)` (the phases
        `ctd_kkt_minres_schur_cr_shard_*`: the same three gathers on larger slots, no collective added); a SchurCrJointPrecond P of
        `kkt_schur_cr_joint_precond`, or "schur_cr_joint": the same with the couplings across the ranks restored (the phases
        `ctd_kkt_minres_schur_cr_joint_*`: the same three gathers on slots that also carry the solve records).  Returns (z, MinresInfo): z
        full-length, this rank's own entries and the nv tail valid (`out`: z).
        The halos of x and y are exchanged once before the loop (`x_halo_valid`, `y_halo_valid`: as in `kktprod`).  Per iteration:
        the halo of the Lanczos vector (`exchange_kkt_halo`), the two launches of `kktprod_shard`, three vector launches and two
        more small all-gathers (the send slots); NO all-reduce: every cross-rank sum is an all-gather followed by a sum in rank
        order on the device, so the bits depend on the split of the grid only.  Everything runs on torch's current stream; the
        host reads the state once per `check_every` iterations.
        NO COLLECTIVE AGREES ON STOPPING, and none is needed: every rank forms every scalar from the same gathered bytes in the
        same order, so the state every rank reads has the same bytes, every rank leaves the loop after the same chunk, and the
        collective counts match."""
        d = self.docp
        n = d.dim_NLP_variables + d.dim_NLP_constraints
        if x is None or rhs is None:
            raise ValueError(("x" if x is None else "rhs") + " is required")
        self._product_x(x, "kkt_minres", x_halo_valid)
        if y is not None and not y_halo_valid:
            self.exchange_product_rows(y)
        if isinstance(precond, str):
            if precond not in ("diag", "schur_cr", "schur_cr_joint"):
                raise ValueError('precond is None, a pair (px, pc), a SchurCrShardPrecond, a SchurCrJointPrecond, "diag", "schur_cr" or '
                                 f'"schur_cr_joint", not {precond!r}')
            build = {"diag": self.kkt_diag_precond, "schur_cr": self.kkt_schur_cr_precond, "schur_cr_joint": self.kkt_schur_cr_joint_precond}[precond]
            precond = build(x, y, obj_weight, sx, sc, x_halo_valid=True, y_halo_valid=True)
        collective = self.world > 1 or _FORCE
        if isinstance(precond, SchurCrJointPrecond) and (precond.layout.n_ranks, precond.layout.rank) != (self.world, self.rank):
            raise ValueError(f"precond was factored as rank {precond.layout.rank} of {precond.layout.n_ranks}, this is rank {self.rank} of {self.world}")
        fam = _phase_family(precond)           # (every family cuts its own slots: a workspace per family)
        w = self._minres_ws.get(fam)
        if w is None or w.ws.device != x.device:
            w = self._minres_ws[fam] = d._phase_workspace(fam, self.world, self.rank)
        z = torch.empty(n, dtype=torch.float64, device=x.device) if out is None else out

        def gather(which):
            # (one rank and no rehearsal: the layout makes the gathered areas the send slots)
            if collective:
                _all_gather_into(w.gathered_a if which == "a" else w.gathered_b, w.send_a if which == "a" else w.send_b, self.group)

        ph = MinresPhases([_MinresRank(d, self.rank, w, z, x, y, obj_weight, sx, sc, rhs, precond)],
                          lambda: self.exchange_kkt_halo(w.v_x, w.v_c), gather)
        info = ph.solve(float(rtol), int(5 * n if max_iter is None else max_iter), int(check_every))[0]
        return z, info

    def obj(self, x, as_tensor=False):
        """Objective of the whole transcription: the shards' partial sums added with one all-reduce of one double that never
        leaves the device; `as_tensor=False` reads the result back at the end (the only host round trip)."""
        if not torch.is_tensor(x):
            return reduce_objective(self.docp.obj(x), self.group)
        if self._f is None:
            self._f = torch.zeros(1, dtype=torch.float64, device=x.device)
        self._rebind()
        self._check_peer(x, "obj")
        self.docp.obj_async(x, self._f)
        if self.world > 1 or _FORCE:
            dist.all_reduce(self._f, op=dist.ReduceOp.SUM, group=self.group)
        return self._f if as_tensor else float(self._f.item())

    def close(self):
        if self._ipc_bases:
            from . import _lib
            torch.cuda.synchronize(self._dev)
            for dev, b in self._ipc_bases:
                _lib.lib().ctd_ipc_close(dev, b)
            self._ipc_bases = []
        self._peer = None
        self._peer_tables = {}
        self.docp.close()
