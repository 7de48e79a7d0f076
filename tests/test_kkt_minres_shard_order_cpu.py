"""The summation order of the shard form of the MINRES solve, transcribed in NumPy and checked without a GPU and without the kernels.

`minres_sharded` restates csrc/ctd_krylov_shard_kernels.hpp: the compacted list of a rank's owned indices cut into workgroups by
krylov_geom(n_own); per thread the terms of its positions in ascending order from 0.0, the shuffle tree per wave, the four waves in
order from 0.0; the partial sums in a send slot of CTD_KKT_MINRES_SHARD_SLOT doubles -- start and (A) at stride 1, (B) at stride 4,
padded with +0.0, the workgroup count in its own field; every cross-rank sum one running sum from 0.0 over the gathered slots, ranks
ascending, workgroups ascending, the padding skipped by count; the tail of K v taken as the ranks' partial sums added in rank order
STARTING FROM RANK 0's VALUE; the tail terms of an inner product counted by the last rank only, and alfa's tail terms, with several
ranks, added by (B) after the last rank's workgroups.  `minres_whole` restates csrc/ctd_krylov_kernels.hpp the same way (one
geometry over 0 .. n - 1, one row of partial sums).  Every expression of the recurrences is scipy.sparse.linalg.minres's.

CHECKED
  one rank      minres_sharded with the single rank that owns 0 .. n - 1 gives the BITS of minres_whole: z after k = 1 .. 5
                iterations and every scalar of the state, with and without M.
  three ranks   z after k = 1 .. 5 iterations against scipy.sparse.linalg.minres on the same matrix (rtol = 0, maxiter = k):
                |z - z_scipy| / |z_scipy| <= BOUND = 16 k n eps.  Where the bound comes from: the two runs evaluate the same
                recurrences and differ only in the order of the additions of the inner products (and of the tail of K v); an inner
                product of n terms carries a relative rounding error of at most n eps in any order; an iteration has a handful of
                them and k iterations compound at most linearly at this size, which the factor 16 covers.  The matrix is built
                quasi-definite with diagonals of order 1 so that no cancellation amplifies it further.  The observed figures are
                printed.  (tests/test_kkt_minres_cpu.py, which the issue names as the source of a dense matrix and of a rule, holds
                neither: the matrix and the bound are this file's, by the reasoning above.)
  the test bites a variant of the transcription with one convention changed -- the tail of K v summed from 0.0 in reverse rank order,
                alfa's tail terms left out -- no longer meets a bound (shown for the second; the first changes bits only).

The sizes: n = 3600 (2100 variables of which the last two are the replicated tail, 1500 rows); the whole grid spans 4 workgroups of a
chunk of 1024 (the last one partly filled); the three ranks own 1202, 1202 and 1200 entries: 2 workgroups each with a chunk of 768,
three passes per thread, so a cross-rank sum has six terms and a slot holds a count of 2 and padding."""
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator, minres

from test_gpu_kkt_minres import krylov_constants, krylov_geom

BLOCK, SPAN, MAX_WG = krylov_constants()
SLOT_TAIL, TAIL_MAX = 4 * MAX_WG, 16
SLOT_COUNT = SLOT_TAIL + TAIL_MAX
SLOT = SLOT_COUNT + 16
EPS = float(np.finfo(np.float64).eps)
NVAR, NV, NCON = 2100, 2, 1500
N = NVAR + NCON
TAIL = np.arange(NVAR - NV, NVAR)


def test_the_slot_constants_are_the_header_s():
    import os
    import re
    import ctdirect_jl_amd as ct
    root = os.path.dirname(os.path.abspath(ct.__file__))
    with open(os.path.join(root, "..", "include", "ctdirect_hip.h")) as f:
        assert int(re.search(r"#define CTD_KKT_MINRES_SHARD_SLOT (\d+)", f.read()).group(1)) == SLOT == ct._lib.KKT_MINRES_SHARD_SLOT
    assert (BLOCK, SPAN, MAX_WG) == (256, 1024, 512)


# ---- the sums ---------------------------------------------------------------------------------------------------------------------
def wave_tree(a):
    a = a.copy()
    for off in (32, 16, 8, 4, 2, 1):
        a[:off] = a[:off] + a[off:2 * off]
    return a[0]


def block_partials(terms, counted, nwg, chunk):
    """the workgroups' partial sums of `terms` (one per position, a row per position when several sums are formed together); a
    position that is not `counted` adds nothing"""
    terms = terms.reshape(len(terms), -1)
    npos, ns = terms.shape
    out = np.zeros((nwg, ns))
    for b in range(nwg):
        lo, hi = b * chunk, min(npos, (b + 1) * chunk)
        acc = np.zeros((BLOCK, ns))
        for p0 in range(lo, hi, BLOCK):               # the passes of the threads, in order
            k = min(BLOCK, hi - p0)
            c = counted[p0:p0 + k, None]
            acc[:k] = np.where(c, acc[:k] + terms[p0:p0 + k], acc[:k])
        for j in range(ns):
            s = 0.0
            for wv in range(BLOCK // 64):
                s = s + wave_tree(acc[64 * wv:64 * wv + 64, j])
            out[b, j] = s
    return out


def new_slot(nwg):
    s = np.zeros(SLOT)
    s[SLOT_COUNT] = float(nwg)
    return s


def gathered_sum(slots, stride, j):
    s = 0.0
    for slot in slots:                                # ranks ascending
        for b in range(int(slot[SLOT_COUNT])):        # workgroups ascending, the padding skipped by count
            s = s + slot[b * stride + j]
    return s


def gathered_kv_tail(slots, j, from_zero_reversed=False):
    if from_zero_reversed:                            # (the variant the last test shows to differ)
        s = 0.0
        for slot in reversed(slots):
            s = s + slot[SLOT_TAIL + j]
        return s
    s = slots[0][SLOT_TAIL + j]                       # from rank 0's value
    for slot in slots[1:]:
        s = s + slot[SLOT_TAIL + j]
    return s


def rowdot(row, v, cols):
    s = 0.0
    for c in cols:
        s = s + row[c] * v[c]
    return s


# ---- the scalar recurrences of (C), scipy's expressions ------------------------------------------------------------------------------
def new_state(beta1):
    return dict(oldb=0.0, beta=beta1, dbar=0.0, epsln=0.0, phibar=beta1, cs=-1.0, sn=0.0, tnorm2=0.0, itn=0)


def rotate(s, alfa, b2):
    """(C)'s scalars: the new state, and oldeps, delta, denom, phi for the vector update"""
    t = dict(s)
    t["oldb"] = s["beta"]
    t["beta"] = math.sqrt(b2)
    t["tnorm2"] = s["tnorm2"] + ((alfa * alfa + t["oldb"] * t["oldb"]) + t["beta"] * t["beta"])
    oldeps = s["epsln"]
    delta = s["cs"] * s["dbar"] + s["sn"] * alfa
    gbar = s["sn"] * s["dbar"] - s["cs"] * alfa
    t["epsln"] = s["sn"] * t["beta"]
    t["dbar"] = -s["cs"] * t["beta"]
    gamma = max(math.sqrt(gbar * gbar + t["beta"] * t["beta"]), EPS)
    t["cs"] = gbar / gamma
    t["sn"] = t["beta"] / gamma
    phi = t["cs"] * s["phibar"]
    t["phibar"] = t["sn"] * s["phibar"]
    t["itn"] = s["itn"] + 1
    return t, oldeps, delta, 1.0 / gamma, phi


# ---- the operator: K v off the tail from one product; a tail entry as the sum of per-rank partial sums over the ranks' columns -------
class Operator:
    def __init__(self, K):
        self.K = K.tocsr()
        self.tail_rows = [np.asarray(self.K[t].todense()).ravel() for t in TAIL]

    def apply(self, v, rank_cols):
        """(K v with the tail entries unset, [per rank: its partial sums of the tail entries])"""
        kv = self.K @ v
        kv[TAIL] = np.nan
        return kv, [np.array([rowdot(row, v, cols) for row in self.tail_rows]) for cols in rank_cols]


def lanczos_y(kv, r1, ortho, c1):
    return kv - c1 * r1 if ortho else kv


# ---- the whole-grid solve (csrc/ctd_krylov_kernels.hpp) --------------------------------------------------------------------------------
def minres_whole(op, rhs, minv, k):
    n = len(rhs)
    nwg, chunk = krylov_geom(n)
    every = np.ones(n, dtype=bool)
    total = lambda terms: sum_in_order(block_partials(terms, every, nwg, chunk))      # noqa: E731
    r1, r2 = rhs.copy(), rhs.copy()
    y = minv * rhs if minv is not None else rhs.copy()
    z, w, w2 = np.zeros(n), np.zeros(n), np.zeros(n)
    beta1 = math.sqrt(total(rhs * y)[0])
    v = (1.0 / beta1) * y
    s = new_state(beta1)
    for _ in range(k):
        kv, (tail,) = op.apply(v, [np.arange(n)])
        kv[TAIL] = tail
        ortho = s["itn"] >= 1
        c1 = s["beta"] / s["oldb"] if ortho else 0.0
        alfa = total(v * lanczos_y(kv, r1, ortho, c1))[0]                              # (A)
        c2 = alfa / s["beta"]                                                         # (B)
        yv = lanczos_y(kv, r1, ortho, c1) - c2 * r2
        r1, r2 = r2, yv
        y = minv * yv if minv is not None else yv.copy()
        u = (v - s["epsln"] * w2) - (s["cs"] * s["dbar"] + s["sn"] * alfa) * w
        b2, _, _, _ = total(np.stack([yv * y, z * z, z * u, u * u], axis=1))
        s, oldeps, delta, denom, phi = rotate(s, alfa, b2)                            # (C)
        wn = ((v - oldeps * w2) - delta * w) * denom
        w2, w = w, wn
        z = z + phi * wn
        v = (1.0 / s["beta"]) * y
    return z, s


def sum_in_order(partials):
    s = np.zeros(partials.shape[1])
    for row in partials:
        s = s + row
    return s


# ---- the shard form (csrc/ctd_krylov_shard_kernels.hpp) --------------------------------------------------------------------------------
def minres_sharded(op, rhs, minv, owned, k, kv_tail_variant=False, drop_alfa_tail=False):
    """owned[r]: the ascending global indices rank r owns (the tail in every list).  Every entry is updated by its owner -- the tail by
    every rank with the same bits, kept once here; what is per rank is what the kernels keep per rank: partial sums and slots."""
    n, G = len(rhs), len(owned)
    geom = [krylov_geom(len(o)) for o in owned]
    is_tail = [np.isin(o, TAIL) for o in owned]
    in_dot = [~t | (r == G - 1) for r, t in enumerate(is_tail)]           # the tail terms: the last rank only
    in_alfa = [~t | (G == 1) for t in is_tail]                           # (A): only where K v is complete at the tail
    dot_cols = [o[m] for o, m in zip(owned, in_dot)]                     # the columns of a rank's partial sums of the tail of K v

    def slots_of(terms, counted, stride):
        out = []
        for r, o in enumerate(owned):
            nwg, chunk = geom[r]
            slot = new_slot(nwg)
            part = block_partials(terms[o], counted[r], nwg, chunk)
            for b in range(nwg):
                slot[b * stride:b * stride + part.shape[1]] = part[b]
            out.append(slot)
        return out

    r1, r2 = rhs.copy(), rhs.copy()
    y = minv * rhs if minv is not None else rhs.copy()
    z, w, w2 = np.zeros(n), np.zeros(n), np.zeros(n)
    beta1 = math.sqrt(gathered_sum(slots_of(rhs * y, in_dot, 1), 1, 0))
    v = (1.0 / beta1) * y
    s = new_state(beta1)
    for _ in range(k):
        kv, tails = op.apply(v, dot_cols)
        ortho = s["itn"] >= 1
        c1 = s["beta"] / s["oldb"] if ortho else 0.0
        # (A): with one rank the rank's own tail of K v is complete
        kva = kv.copy()
        kva[TAIL] = tails[0] if G == 1 else 0.0
        slots_a = slots_of(v * lanczos_y(kva, r1, ortho, c1), in_alfa, 1)
        for r in range(G):
            slots_a[r][SLOT_TAIL:SLOT_TAIL + NV] = tails[r]
        vt, r1t = v[TAIL].copy(), r1[TAIL].copy()
        # (B)
        alfa = gathered_sum(slots_a, 1, 0)
        kvt = np.array([gathered_kv_tail(slots_a, j, kv_tail_variant) for j in range(NV)])
        if G > 1 and not drop_alfa_tail:
            for j in range(NV):
                alfa = alfa + vt[j] * lanczos_y(kvt[j], r1t[j], ortho, c1)
        kv[TAIL] = kvt
        c2 = alfa / s["beta"]
        yv = lanczos_y(kv, r1, ortho, c1) - c2 * r2
        r1, r2 = r2, yv
        y = minv * yv if minv is not None else yv.copy()
        u = (v - s["epsln"] * w2) - (s["cs"] * s["dbar"] + s["sn"] * alfa) * w
        slots_b = slots_of(np.stack([yv * y, z * z, z * u, u * u], axis=1), in_dot, 4)
        # (C)
        b2 = gathered_sum(slots_b, 4, 0)
        s, oldeps, delta, denom, phi = rotate(s, alfa, b2)
        wn = ((v - oldeps * w2) - delta * w) * denom
        w2, w = w, wn
        z = z + phi * wn
        v = (1.0 / s["beta"]) * y
    return z, s


# ---- the data ---------------------------------------------------------------------------------------------------------------------
def system():
    """K = [[H, J'], [J, -Sc]] quasi-definite with diagonals of order 1; the two tail variables couple to every variable and row, as the
    optimisation variables of a transcription do"""
    r = np.random.default_rng(5)
    A = sp.random(NVAR, NVAR, density=2e-3, random_state=r, data_rvs=lambda k: 0.05 * r.uniform(-1, 1, k))
    H = (A + A.T + sp.diags(r.uniform(2.0, 3.0, NVAR))).tolil()
    J = sp.random(NCON, NVAR, density=3e-3, random_state=r, data_rvs=lambda k: r.uniform(-1, 1, k)).tolil()
    for t in TAIL:
        col = 0.02 * r.uniform(-1, 1, NVAR)
        col[t] = 2.5
        H[t, :] = col
        H[:, t] = col.reshape(-1, 1)
        J[:, t] = 0.05 * r.uniform(-1, 1, (NCON, 1))
    H = H.tocsr()
    H = (H + H.T) * 0.5
    K = sp.bmat([[H, J.T], [J, -sp.diags(r.uniform(1.0, 2.0, NCON))]]).tocsr()
    assert abs(K - K.T).max() == 0.0
    return Operator(K), r.uniform(-1.0, 1.0, N), 1.0 / r.uniform(0.5, 2.0, N)


SYSTEM = system()
CUTS_V, CUTS_C = (0, 700, 1400, NVAR - NV), (0, 500, 1000, NCON)
THREE = [np.r_[np.arange(CUTS_V[r], CUTS_V[r + 1]), TAIL, NVAR + np.arange(CUTS_C[r], CUTS_C[r + 1])] for r in range(3)]


def test_the_geometry_exercises_counts_padding_and_passes():
    assert krylov_geom(N) == (4, 1024)
    assert [krylov_geom(len(o)) for o in THREE] == [(2, 768)] * 3 and [len(o) for o in THREE] == [1202, 1202, 1200]


def test_one_rank_gives_the_bits_of_the_whole_grid_order():
    op, rhs, minv = SYSTEM
    for m in (None, minv):
        for k in (1, 2, 5):
            zw, sw = minres_whole(op, rhs, m, k)
            zs, ss = minres_sharded(op, rhs, m, [np.arange(N)], k)
            assert ss == sw, (k, ss, sw)
            assert np.array_equal(zs, zw), (k, "z: not the bits of the whole-grid order")


def test_three_ranks_reproduce_scipy_s_first_five_iterates():
    op, rhs, minv = SYSTEM
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))      # noqa: E731
    for m in (None, minv):
        M = None if m is None else LinearOperator((N, N), matvec=lambda x, m=m: m * np.asarray(x).ravel(), dtype=np.float64)
        for k in (1, 2, 3, 4, 5):
            z_ref, _ = minres(op.K, rhs, M=M, rtol=0.0, maxiter=k)
            z3, s3 = minres_sharded(op, rhs, m, THREE, k)
            zw, _ = minres_whole(op, rhs, m, k)
            bound = 16.0 * k * N * EPS
            print("preconditioned" if m is not None else "plain", "k", k, "three ranks vs scipy", rel(z3, z_ref), "whole-grid order vs scipy",
                  rel(zw, z_ref), "three ranks vs whole-grid order", rel(z3, zw), "bound", bound)
            assert s3["itn"] == k
            assert rel(z3, z_ref) <= bound, (k, rel(z3, z_ref), bound)
            assert rel(z3, zw) <= bound, (k, rel(z3, zw), bound)


def test_a_changed_convention_is_seen():
    """the order is pinned, not only the value: the tail of K v summed from 0.0 in reverse rank order changes bits of the iterate;
    alfa without its tail terms no longer meets the bound"""
    op, rhs, minv = SYSTEM
    z3, _ = minres_sharded(op, rhs, minv, THREE, 5)
    zv, _ = minres_sharded(op, rhs, minv, THREE, 5, kv_tail_variant=True)
    assert not np.array_equal(zv, z3)
    z_ref, _ = minres(op.K, rhs, M=LinearOperator((N, N), matvec=lambda x: minv * np.asarray(x).ravel(), dtype=np.float64), rtol=0.0, maxiter=5)
    zd, _ = minres_sharded(op, rhs, minv, THREE, 5, drop_alfa_tail=True)
    assert np.linalg.norm(zd - z_ref) / np.linalg.norm(z_ref) > 16.0 * 5 * N * EPS
