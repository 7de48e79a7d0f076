"""The chunked block-tridiagonal Schur preconditioner stated densely in NumPy / scipy: the reference of tests/test_kkt_schur_cpu.py
and tests/test_gpu_kkt_schur.py.  No code under test is involved: everything is built from K_asm's own blocks (minres_case of
test_gpu_kkt_minres.py) and the three integers of the layout (N, block_rows m, tail_cols nv).

    T_c   = Jt_c diag(1 / px) Jt_c' + Sc_c        Jt: J without the last nv columns, rows of the blocks [c L, min((c + 1) L, N))
    M^-1  = blkdiag(diag(px), T_0, T_1, ..., diag(pc_tail))
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
from scipy.sparse.linalg import LinearOperator


def chunks(N, L):
    L = min(int(L), N)
    return [(k, min(k + L, N)) for k in range(0, N, L)]


def schur_T(c, px, m, N, nv, L):
    """dense blkdiag(T_c) on the N m block rows"""
    nvar = c["nvar"]
    Jt = c["J"].tocsc()[:N * m, :nvar - nv]
    S = (Jt @ sp.diags(1.0 / px[:nvar - nv]) @ Jt.T).toarray() + np.diag(c["sc"][:N * m])
    T = np.zeros_like(S)
    for k0, k1 in chunks(N, L):
        sl = slice(k0 * m, k1 * m)
        T[sl, sl] = S[sl, sl]
    return T


class SchurRef:
    """M as a function: variables / px, chunk rows through the Cholesky factor of T_c, tail rows / pc"""
    def __init__(self, c, px, pc, m, N, nv, L):
        self.nvar, self.ncon, self.nb = c["nvar"], c["ncon"], N * m
        self.px, self.pc = px, pc
        self.T = schur_T(c, px, m, N, nv, L)
        self.fac = [(slice(k0 * m, k1 * m), sla.cho_factor(self.T[k0 * m:k1 * m, k0 * m:k1 * m], lower=True)) for k0, k1 in chunks(N, L)]

    def solve_rows(self, r):
        out = np.zeros(self.nb)
        for sl, f in self.fac:
            out[sl] = sla.cho_solve(f, r[sl])
        return out

    def apply(self, v):
        v = np.asarray(v, dtype=np.float64).ravel()
        rc = v[self.nvar:]
        return np.r_[v[:self.nvar] / self.px, self.solve_rows(rc[:self.nb]), rc[self.nb:] / self.pc[self.nb:]]

    def operator(self):
        n = self.nvar + self.ncon
        return LinearOperator((n, n), matvec=self.apply, dtype=np.float64)


def small_sc_case(c, scv=1e-8):
    """the system of minres_case with sc = scv U(1, 2) (the same draws: minres_case's sc is 1e-2 U(1, 2)) and sx shifted by
    max(0, -lambda_min(H)) where minres_case has not done so (it does for N = 20 only): H + Sx positive definite"""
    d = dict(c)
    if c["N"] != 20:
        lam_min = float(np.linalg.eigvalsh(c["H"].toarray())[0])
        d["sx"] = c["sx"] + max(0.0, -lam_min)
    d["sc"] = c["sc"] * (scv / 1e-2)
    d["K_asm"] = sp.bmat([[c["H"] + sp.diags(d["sx"]), c["J"].T], [c["J"], -sp.diags(d["sc"])]]).tocsr()
    return d
