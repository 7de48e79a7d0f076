"""The shard form of the log-depth Schur preconditioner stated densely in NumPy / scipy: the reference of
tests/test_kkt_schur_cr_shard_cpu.py and tests/test_gpu_kkt_schur_cr_shard.py.  No code under test is involved: the matrix is built
from K_asm's own blocks (minres_case of test_gpu_kkt_minres.py), the three integers of the layout (N, block_rows m, tail_cols nv) and
the cuts -- the ascending first steps of the ranks, 0 first and N last, of any lengths.

    T_r   = the principal submatrix of T = Jt diag(1 / px) Jt' + Sc on the blocks [cuts[r], cuts[r + 1])
    M^-1  = blkdiag(diag(px), T_0, ..., T_{G-1}, diag(pc_tail))

and the order of the cross-rank sum of beta1^2 / beta^2 of csrc/ctd_krylov_shard_kernels.hpp, transcribed."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator


def shard_cuts(N, G):
    """the cuts of dist.shard_steps / ctd_shard_steps"""
    base, rem = divmod(N, G)
    return [r * base + min(r, rem) for r in range(G)] + [N]


def full_T(c, px, m, N, nv):
    nvar = c["nvar"]
    Jt = c["J"].tocsc()[:N * m, :nvar - nv]
    return (Jt @ sp.diags(1.0 / px[:nvar - nv]) @ Jt.T).toarray() + np.diag(c["sc"][:N * m])


def cut_T(c, px, m, N, nv, cuts):
    """dense blkdiag(T_r) on the N m block rows: T with the G - 1 coupling blocks across the cuts (and their transposes) dropped"""
    assert cuts[0] == 0 and cuts[-1] == N and all(a < b for a, b in zip(cuts, cuts[1:])), cuts
    S = full_T(c, px, m, N, nv)
    T = np.zeros_like(S)
    for k0, k1 in zip(cuts, cuts[1:]):
        sl = slice(k0 * m, k1 * m)
        T[sl, sl] = S[sl, sl]
    return T


class SchurCutRef:
    """M as a function: variables / px, a rank's rows through the Cholesky factor of T_r, tail rows / pc"""
    def __init__(self, c, px, pc, m, N, nv, cuts):
        self.nvar, self.ncon, self.nb, self.m, self.cuts = c["nvar"], c["ncon"], N * m, m, list(cuts)
        self.px, self.pc = px, pc
        self.T = cut_T(c, px, m, N, nv, cuts)
        self.rows = [slice(k0 * m, k1 * m) for k0, k1 in zip(cuts, cuts[1:])]
        self.fac = [sla.cho_factor(self.T[sl, sl], lower=True) for sl in self.rows]

    def T_r(self, r):
        return self.T[self.rows[r], self.rows[r]]

    def solve_rank(self, r, rhs):
        """T_r^-1 on the rank's rows of a vector of the block rows"""
        return sla.cho_solve(self.fac[r], rhs[self.rows[r]])

    def solve_rows(self, rhs):
        out = np.zeros(self.nb)
        for r, sl in enumerate(self.rows):
            out[sl] = self.solve_rank(r, rhs)
        return out

    def apply(self, v):
        v = np.asarray(v, dtype=np.float64).ravel()
        rc = v[self.nvar:]
        return np.r_[v[:self.nvar] / self.px, self.solve_rows(rc[:self.nb]), rc[self.nb:] / self.pc[self.nb:]]

    def operator(self):
        n = self.nvar + self.ncon
        return LinearOperator((n, n), matvec=self.apply, dtype=np.float64)


def cross_rank_sum(own, solve):
    """beta1^2 / beta^2 of the Schur form from the gathered slots.  own[r]: rank r's partial sums of the init kernel or of (B), in
    workgroup order; solve[r]: its solve's partial sums, in workgroup order.  One running sum from 0.0: the ranks ascending with
    their own terms, then the ranks ascending again with the solve's"""
    s = np.float64(0.0)
    for part in list(own) + list(solve):
        for t in part:
            s = s + np.float64(t)
    return float(s)


def solve_partial_sums(r, y, m, n_blocks, cap=256):
    """the partial sums of r . y over a rank's n_blocks blocks as its last launch leaves them: G_r = min(n_blocks, cap) workgroups,
    workgroup g adds in lane a the local blocks g, g + G_r, ... from 0.0, then the shuffle tree over 64 lanes (off = 32, ..., 1)"""
    G = min(n_blocks, cap)
    out = []
    for g in range(G):
        lanes = np.zeros(64)
        for a in range(m):
            acc = np.float64(0.0)
            for k in range(g, n_blocks, G):
                acc = acc + np.float64(r[k * m + a]) * np.float64(y[k * m + a])
            lanes[a] = acc
        off = 32
        while off:
            lanes[:64 - off] = lanes[:64 - off] + lanes[off:]
            off >>= 1
        out.append(float(lanes[0]))
    return out
