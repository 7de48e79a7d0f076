"""The log-depth exact block-tridiagonal Schur preconditioner stated in NumPy on dense blocks: block odd-even (cyclic) reduction of
T = Jt diag(1 / px) Jt' + Sc in the documented order (csrc/ctd_schur_cr_kernels.hpp).  The reference of tests/test_kkt_schur_cr_cpu.py
and tests/test_gpu_kkt_schur_cr.py; no code under test is involved: the input is the dense one-chunk T of tests/schur_ref.py.

Level l = 0 .. ceil(log2 N) - 1, h = 2^l: the blocks that are odd multiples of h are eliminated (left neighbour i - h, right
neighbour i + h when below N), the even multiples survive; E[k] is the current coupling of the active block k to the next one.
"""
import numpy as np


def levels(N):
    return (int(N) - 1).bit_length()


def eliminated(N, l):
    h = 1 << l
    return list(range(h, N, 2 * h))


def chol(A):
    """column by column, divisions by a pivot's root as products with its reciprocal; (L, -1), or (NaN, the column of the pivot that
    is not positive or not finite)"""
    m = len(A)
    L = np.tril(np.array(A, dtype=np.float64))
    for j in range(m):
        L[j:, j] -= L[j:, :j] @ L[j, :j]
        d = L[j, j]
        if not (d > 0.0) or not np.isfinite(d):
            return np.full((m, m), np.nan), j
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] *= 1.0 / L[j, j]
    return L, -1


def forward(L, B):
    """L^-1 B"""
    X = np.array(B, dtype=np.float64)
    for j in range(len(L)):
        X[j] = (X[j] - L[j, :j] @ X[:j]) * (1.0 / L[j, j])
    return X


def backward(L, B):
    """L^-T B"""
    X = np.array(B, dtype=np.float64)
    for j in range(len(L) - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) * (1.0 / L[j, j])
    return X


class SchurCrRef:
    """the factor of the dense block-tridiagonal T (N blocks of m rows) and its solve"""
    def __init__(self, T, N, m):
        self.N, self.m, self.n_levels = N, m, levels(N)
        blk = lambda i, k: np.array(T[i * m:(i + 1) * m, k * m:(k + 1) * m], dtype=np.float64)      # noqa: E731
        D = [blk(i, i) for i in range(N)]
        E = {i: blk(i + 1, i) for i in range(N - 1)}
        self.L, self.Gm, self.Gp = {}, {}, {}
        self.status = -np.ones(N, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for l in range(self.n_levels):
                h = 1 << l
                for i in eliminated(N, l):
                    self.L[i], self.status[i] = chol(D[i])
                    self.Gm[i] = forward(self.L[i], E[i - h])
                    if i + h < N:
                        self.Gp[i] = forward(self.L[i], E[i].T).T
                for k in range(0, N, 2 * h):
                    if k >= h:                      # the left neighbour's term first
                        D[k] = D[k] - self.Gp[k - h] @ self.Gp[k - h].T
                    if k + h < N:
                        D[k] = D[k] - self.Gm[k + h].T @ self.Gm[k + h]
                    if k + 2 * h < N:
                        E[k] = -(self.Gp[k + h] @ self.Gm[k + h])
            self.L[0], self.status[0] = chol(D[0])

    def info(self):
        bad = np.flatnonzero(self.status >= 0)
        return int(bad[0]) if len(bad) else -1

    def solve(self, r):
        N, m = self.N, self.m
        rhs = np.array(r[:N * m], dtype=np.float64).reshape(N, m)
        y, x = {}, np.zeros((N, m))
        with np.errstate(invalid="ignore"):
            for l in range(self.n_levels):
                h = 1 << l
                for i in eliminated(N, l):
                    y[i] = forward(self.L[i], rhs[i])
                for k in range(0, N, 2 * h):
                    if k >= h:
                        rhs[k] = rhs[k] - self.Gp[k - h] @ y[k - h]
                    if k + h < N:
                        rhs[k] = rhs[k] - self.Gm[k + h].T @ y[k + h]
            x[0] = backward(self.L[0], forward(self.L[0], rhs[0]))
            for l in range(self.n_levels - 1, -1, -1):
                h = 1 << l
                for i in eliminated(N, l):
                    g = y[i] - self.Gm[i] @ x[i - h]
                    if i + h < N:
                        g = g - self.Gp[i].T @ x[i + h]
                    x[i] = backward(self.L[i], g)
        return x.ravel()
