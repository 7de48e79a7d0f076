"""The joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*) stated densely in NumPy / scipy: the reference of
tests/test_kkt_schur_cr_joint_cpu.py and tests/test_gpu_kkt_schur_cr_joint.py.  No code under test is involved: the matrix is
full_T of tests/schur_shard_ref.py on K_asm's own blocks, the three integers of the layout (N, block_rows m, tail_cols nv) and the
cuts -- the ascending first steps of the ranks, 0 first and N last; every rank but the first has at least two steps.

    separators   s_r = cuts[r], r = 1 .. G - 1;  interior I_r = [cuts[r] + (r > 0), cuts[r + 1]),  A_r = T on I_r,  a / b its first / last
    spikes       Wl = A_r^-1 (e_a E[s_r]),  Wr = A_r^-1 (e_b E[b]'),  E[k] = T(k + 1, k)
    reduced      S(r, r) = (D_s - Crr^(r-1)) - Cll^(r),  S(r + 1, r) = -Crl^(r);  Cll = E[s]' Wl[a], Crl = E[b] Wl[b], Crr = E[b] Wr[b]
    apply        g = A_r^-1 r_I;  rs~_r = (r_s - qd^(r-1)) - qu^(r), qu = E[s]' g[a], qd = E[b] g[b];  x_s = S^-1 rs~;
                 y_s = x_s,  y_I = (g - Wl x_{s_r}) - Wr x_{s_{r+1}}
    identity     r . y = sum_r r_I . g_r + x_s . rs~          (r' T^-1 r split by the block elimination)"""
import numpy as np
import scipy.linalg as sla
from scipy.sparse.linalg import LinearOperator

from schur_shard_ref import full_T


class SchurJointRef:
    def __init__(self, c, px, pc, m, N, nv, cuts):
        cuts = list(cuts)
        assert cuts[0] == 0 and cuts[-1] == N and all(a < b for a, b in zip(cuts, cuts[1:])), cuts
        assert all(b - a >= 2 for a, b in zip(cuts[1:], cuts[2:])), ("a rank >= 1 needs an interior block", cuts)
        self.nvar, self.ncon, self.nb, self.m, self.N, self.cuts, self.G = c["nvar"], c["ncon"], N * m, m, N, cuts, len(cuts) - 1
        self.px, self.pc = px, pc
        self.T = T = full_T(c, px, m, N, nv)
        blk = lambda i, j: T[i * m:(i + 1) * m, j * m:(j + 1) * m]      # noqa: E731
        G = self.G
        self.ranks = []
        for r in range(G):
            sb, se = cuts[r], cuts[r + 1]
            a = sb + (1 if r > 0 else 0)
            rows = slice(a * m, se * m)
            n_int = se - a
            fac = sla.cho_factor(T[rows, rows], lower=True)
            d = dict(sb=sb, se=se, a=a, rows=rows, n_int=n_int, fac=fac, Es=None, Eb=None, Wl=None, Wr=None)
            if r > 0:
                d["Es"] = blk(a, sb)
                rhs = np.zeros((n_int * m, m))
                rhs[:m] = d["Es"]
                d["Wl"] = sla.cho_solve(fac, rhs)
                d["Ds"] = blk(sb, sb)
                d["Cll"] = d["Es"].T @ d["Wl"][:m]
            if r < G - 1:
                d["Eb"] = blk(se, se - 1)
                rhs = np.zeros((n_int * m, m))
                rhs[-m:] = d["Eb"].T
                d["Wr"] = sla.cho_solve(fac, rhs)
                d["Crr"] = d["Eb"] @ d["Wr"][-m:]
                if r > 0:
                    d["Crl"] = d["Eb"] @ d["Wl"][-m:]
            self.ranks.append(d)
        n = G - 1
        self.S = S = np.zeros((n * m, n * m))
        for r in range(1, G):
            k, d = r - 1, self.ranks[r]
            S[k * m:(k + 1) * m, k * m:(k + 1) * m] = (d["Ds"] - self.ranks[r - 1]["Crr"]) - d["Cll"]
            if r < G - 1:
                S[(k + 1) * m:(k + 2) * m, k * m:(k + 1) * m] = -d["Crl"]
                S[k * m:(k + 1) * m, (k + 1) * m:(k + 2) * m] = -d["Crl"].T
        self.Sfac = sla.cho_factor(S, lower=True) if n else None

    def solve_parts(self, rhs):
        """T^-1 on a vector of the block rows and what the identity is made of: (y, [r_I . g_r per rank], sigma, rs~, x_s)"""
        m, G = self.m, self.G
        y = np.zeros(self.nb)
        inner, g = [], []
        for d in self.ranks:
            g.append(sla.cho_solve(d["fac"], rhs[d["rows"]]))
            inner.append(float(rhs[d["rows"]] @ g[-1]))
        if G == 1:
            y[self.ranks[0]["rows"]] = g[0]
            return y, inner, 0.0, np.zeros(0), np.zeros(0)
        rs = np.zeros((G - 1) * m)
        for r in range(1, G):
            d, left = self.ranks[r], self.ranks[r - 1]
            qd = left["Eb"] @ g[r - 1][-m:]
            qu = d["Es"].T @ g[r][:m]
            rs[(r - 1) * m:r * m] = (rhs[d["sb"] * m:(d["sb"] + 1) * m] - qd) - qu
        xs = sla.cho_solve(self.Sfac, rs)
        for r, d in enumerate(self.ranks):
            v = g[r]
            if r > 0:
                y[d["sb"] * m:(d["sb"] + 1) * m] = xs[(r - 1) * m:r * m]
                v = v - d["Wl"] @ xs[(r - 1) * m:r * m]
            if r < G - 1:
                v = v - d["Wr"] @ xs[r * m:(r + 1) * m]
            y[d["rows"]] = v
        return y, inner, float(xs @ rs), rs, xs

    def solve_rows(self, rhs):
        return self.solve_parts(rhs)[0]

    def apply(self, v):
        v = np.asarray(v, dtype=np.float64).ravel()
        rc = v[self.nvar:]
        return np.r_[v[:self.nvar] / self.px, self.solve_rows(rc[:self.nb]), rc[self.nb:] / self.pc[self.nb:]]

    def operator(self):
        n = self.nvar + self.ncon
        return LinearOperator((n, n), matvec=self.apply, dtype=np.float64)


def backward_error(T, y, r):
    return float(np.abs(T @ y - r).max() / (np.abs(T).sum(axis=1).max() * np.abs(y).max() + np.abs(r).max()))


def joint_sum(own, solve, sigma):
    """beta1^2 / beta^2 of the joined form from the gathered slots: the order of cross_rank_sum of tests/schur_shard_ref.py -- the ranks
    ascending with their own terms, the ranks ascending again with the partial sums of r_I . g_r --, then sigma, one running sum
    from 0.0.  With one rank sigma is not added (there is no separator): the order of the shard form"""
    s = np.float64(0.0)
    for part in list(own) + list(solve):
        for t in part:
            s = s + np.float64(t)
    if len(own) > 1:
        s = s + np.float64(sigma)
    return float(s)
