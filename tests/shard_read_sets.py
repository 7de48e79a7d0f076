"""The write and read sets of the matrix-free products on a shard (ctd_*prod_shard_dev_async), restated from
include/ctdirect_hip.h ("matrix-free products on a shard of the grid") as boolean index masks -- not taken from the engine or
from dist.py.  Shared by tests/test_products_shard_cpu.py and tests/test_gpu_products_shard.py."""
import numpy as np


def variable_read_set(sb, se, N, n, m, blk, nvar, nv, trapeze):
    """own entries; [v_off, nvar); the whole block sb - 1 if sb > 0; if se < N the first n entries of block se (+ the m controls
    behind them on the trapeze); [0, n) and [N blk, N blk + n)"""
    v_off = nvar - nv
    own = np.zeros(nvar, dtype=bool)
    own[sb * blk:(se * blk if se < N else v_off)] = True
    own[v_off:] = True
    need = own.copy()
    if sb > 0:
        need[(sb - 1) * blk:sb * blk] = True
    if se < N:
        need[se * blk:se * blk + n + (m if trapeze else 0)] = True
    need[0:n] = True
    need[N * blk:N * blk + n] = True
    return own, need


def constraint_read_set(sb, se, N, cb, eqs, ncon):
    """own rows (the tail on the last shard); the eqs state / stage rows of step sb - 1 if sb > 0; the p path rows of node se,
    [se cb + eqs, (se + 1) cb), if se < N; the tail [N cb, ncon)"""
    own = np.zeros(ncon, dtype=bool)
    own[sb * cb:(se * cb if se < N else ncon)] = True
    need = own.copy()
    if sb > 0:
        need[(sb - 1) * cb:(sb - 1) * cb + eqs] = True
    if se < N:
        need[se * cb + eqs:(se + 1) * cb] = True
    need[N * cb:] = True
    return own, need
