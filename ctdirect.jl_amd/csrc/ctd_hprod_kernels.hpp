// ctd_hprod_kernels.hpp -- matrix-free Hessian-of-the-Lagrangian products: hprod!(nlp, x, y, v, Hv; obj_weight) and the
// objective-only hprod!(nlp, x, v, Hv; obj_weight).
//
//   Hv = (obj_weight H_f(x) + sum_r y_r H_{c_r}(x)) v
//
// H is the exact second derivative of what ctd_obj and ctd_cons compute (the STRUCTURAL Hessian, whatever pattern the handle
// emits).  The reference leaves the backend empty (hprod_backend = EmptyADbackend, src/collocation.jl:104-110).
//
// Hv is the derivative along v of the gradient of Phi = obj_weight f + y'c, and that gradient is what jtprod computes (with w = y)
// plus the objective's terms.  So the lanes are the jtprod lanes (ctd_prod_kernels.hpp) one derivative order up: one lane per
// (node k, chunk of JC directions of the variables node k owns), which evaluates, on Dual2<JC>, every piece of Phi that reads those
// variables -- the rows of step k and the path rows of node k, the rows of step k-1 when they read X_k (U_k on the trapeze) other
// than through the identity, the path rows of node k+1 when they read U_k, and the Lagrange cost of the quadrature units that read
// node k.  Every input carries the tangent v (Dual2::a) and the lane's own directions carry the unit seeds (Dual2::b): the mixed
// parts ab are the entries of Hv the lane owns.  The d/dv entries are reduced per workgroup with wave shuffles in a fixed order, and
// hprod_finish_kernel sums them in block order and adds the boundary rows and the Mayer term.  No atomics, fixed summation order.
//
// Unlike jtprod, Gauss-Legendre steps do NOT seed x_kj: with free times the map (X_k, K_l, v) -> x_kj = X_k + h(v) sum_l a_jl K_l
// is bilinear, so its K x V and V x V second-order terms would be lost.  The lanes seed X_k, K_l and v themselves and the dual
// arithmetic carries every term, the time grid and h included.
//
// The bodies read neither the emit tables nor the pattern: the products are the same bits for every pattern_mode / value_order of
// one transcription.
#pragma once
#include "ctd_prod_kernels.hpp"

namespace ctd {

struct HProdParams {
    ProdParams p;           // p.dir: multipliers y (ncon entries) or null (objective only); p.out: Hv (nvar); p.partial, p.nblocks, p.nch
    const double* vt;       // the direction v (nvar entries)
    double sigma;           // obj_weight
};

// directions per hprod lane.  Dual2<JC> holds 2 + 2 JC doubles: one direction for the wide OCPs (with two, the 12-state
// quadrotor's Gauss-Legendre 3 lane spills 184 bytes), otherwise up to four.  The host derives the chunk of a run-time OCP with
// the same function.  The second-order number is ctd::Dual2 -- the forward number of the Hessian kernel, a Dual<K> over Dual<1>:
// a = the tangent v, b = the K unit seeds, ab = the mixed second derivatives -- so kinks follow hess_coord's conventions.
CTD_HD constexpr int hprod_chunk(int n, int dc) { return n >= 8 ? 1 : (dc < 4 ? dc : 4); }
template <class P> struct HProdDirs {
    static constexpr int JC = hprod_chunk(P::NX, P::DC);
};

// the directions per node of the hprod lanes: the node's block and v (every scheme)
CTD_HD int hprod_dirs_per_node(const Layout& L) { return L.blk + L.nv; }

// every entry carries the tangent v; direction id `dir` is seed dir - g0 of this chunk
template <int K> struct HSeedSrc {
    const double* x;
    const double* t;
    int g0;
    XWhere wh;          // (where x is found on a shard: ctd_prod_kernels.hpp; t is always the caller's pointer)
    CTD_HD const double* buf(int64_t g) const { return (wh.nr && wh.edge) ? xnear(*wh.nr, x, g) : x; }
    CTD_HD Dual2<K> at(const double* xb, int64_t g, int dir) const {
        Dual2<K> r; r.v = xb[g]; r.a = t[g];
#pragma unroll
        for (int d = 0; d < K; ++d) { r.b[d] = (dir >= 0 && dir - g0 == d) ? 1.0 : 0.0; r.ab[d] = 0.0; }
        return r;
    }
    CTD_HD Dual2<K> at(int64_t g, int dir) const { return at(x, g, dir); }
};

// Lagrange cost of quadrature unit i (trapeze: node i; otherwise step i) on scalar type T, in the form of lagrange_unit
// (ctd_kernels.hpp): trapeze.jl:78-110, midpoint.jl:87-116, euler.jl:112-134, irk.jl:179-228, irk_stagewise.jl:344-384
template <class P, int SC, int S, class T, class Src>
__device__ __forceinline__ T prod_lagrange_unit(const ProdParams& pp, const Src& src, int64_t i, const ProdRoles& ro) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV;
    const Layout& L = pp.L;
    const int64_t b0 = i * (int64_t)L.blk, b1 = (i + 1) * (int64_t)L.blk;
    const double* x0 = src.buf(b0);
    T V[nv > 0 ? nv : 1], xa[n > 0 ? n : 1], u[m > 0 ? m : 1];
#pragma unroll
    for (int k = 0; k < nv; ++k) V[k] = src.at(L.v_off + k, prod_dir(ro.v, k));
    if constexpr (SC == SC_TRAPEZE) {
        const int64_t ia = i == 0 ? 0 : i - 1, ib = i == L.N ? L.N : i + 1;
        const T w = (prod_time<P, T>(pp, V, prod_tau(pp, ib)) - prod_time<P, T>(pp, V, prod_tau(pp, ia))) / 2.0;
#pragma unroll
        for (int c = 0; c < n; ++c) xa[c] = src.at(x0, b0 + c, prod_dir(ro.xi, c));
#pragma unroll
        for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + c, prod_dir(ro.bi, c));
        return w * P::template lagrange<T>(prod_time<P, T>(pp, V, prod_tau(pp, i)), xa, u, V);
    } else {
        const T ti = prod_time<P, T>(pp, V, prod_tau(pp, i)), tip1 = prod_time<P, T>(pp, V, prod_tau(pp, i + 1));
        const T h = tip1 - ti;
        if constexpr (SC == SC_MIDPOINT) {
            const double* x1 = src.buf(b1);
            if (L.cs > 1) {
                const T hi = h / (double)L.cs;
#pragma unroll
                for (int c = 0; c < n; ++c) xa[c] = 0.5 * (src.at(x0, b0 + c, prod_dir(ro.xi, c)) + src.at(x1, b1 + c, prod_dir(ro.xn, c)));
                T val(0.0);
                for (int j = 1; j <= L.cs; ++j) {
#pragma unroll
                    for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + (j - 1) * m + c, prod_dir(ro.bi, (j - 1) * m + c));
                    const T term = hi * P::template lagrange<T>(ti + ((double)j - 0.5) * hi, xa, u, V);
                    val = (j == 1) ? term : val + term;
                }
                return val;
            }
#pragma unroll
            for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + c, prod_dir(ro.bi, c));
            if (L.euler == 0) {
#pragma unroll
                for (int c = 0; c < n; ++c) xa[c] = 0.5 * (src.at(x0, b0 + c, prod_dir(ro.xi, c)) + src.at(x1, b1 + c, prod_dir(ro.xn, c)));
                return h * P::template lagrange<T>(0.5 * (ti + tip1), xa, u, V);
            }
            const bool expl = L.euler == 1;
#pragma unroll
            for (int c = 0; c < n; ++c) xa[c] = expl ? src.at(x0, b0 + c, prod_dir(ro.xi, c)) : src.at(x1, b1 + c, prod_dir(ro.xn, c));
            return h * P::template lagrange<T>(expl ? ti : tip1, xa, u, V);
        } else {
            const int ko = n + L.cu;
            T local(0.0);
#pragma unroll
            for (int j = 0; j < S; ++j) {
#pragma unroll
                for (int c = 0; c < n; ++c) {
                    T xc = src.at(x0, b0 + c, prod_dir(ro.xi, c));
#pragma unroll
                    for (int l = 0; l < S; ++l) xc = xc + h * L.a[3 * j + l] * src.at(x0, b0 + ko + l * n + c, prod_dir(ro.bi, L.cu + l * n + c));
                    xa[c] = xc;
                }
                const int uo = L.stagewise ? j * m : 0;
#pragma unroll
                for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + uo + c, prod_dir(ro.bi, uo + c));
                const T term = L.b[j] * P::template lagrange<T>(ti + L.c[j] * h, xa, u, V);
                local = (j == 0) ? term : local + term;
            }
            return h * local;
        }
    }
}

// lane (node k, chunk q): the JC entries of Hv in directions [q JC, (q + 1) JC) of node k's variables -- its block (bk entries)
// and v [bk, bk + nv).  Block entries go to Hv, v entries to gv.
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void hprod_unit_body(const HProdParams& hp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = HProdDirs<P>::JC;
    using T = Dual2<JC>;
    const ProdParams& pp = hp.p;
    const Layout& L = pp.L;
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;         // the last node of the other schemes owns X_{N+1} only
    const int g0 = q * JC;
    if (g0 >= bk + nv) return;
    const HSeedSrc<JC> src{xu, hp.vt, g0, prod_where<SH>(pp, k)};
    const double* y = pp.dir;
    double acc[JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    const bool hits_x = g0 < n;                     // the chunk holds X_k directions
    const bool hits_u = g0 < n + L.cu && g0 + JC > n && m > 0;      // ... or control directions
    if (y) {
        // rows of step k and path rows of node k: every input of node k carries its direction
        if (k < L.N) {
            auto sink = weighted_rows<JC>(y, k * (int64_t)L.cb, acc);
            prod_step_rows<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
        }
        if (P::NPATH > 0) {
            auto sink = weighted_rows<JC>(y, k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
            prod_path_rows<P, SC, S, T>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
        }
        // rows of step k-1: they read X_k (and U_k on the trapeze); Gauss-Legendre and explicit Euler read X_{i+1} through the
        // identity only, which has no second derivative
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (k >= 1 && !one_point && (hits_x || (SC == SC_TRAPEZE && hits_u))) {
            auto sink = weighted_rows<JC>(y, (k - 1) * (int64_t)L.cb, acc);
            prod_step_rows<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
        // path rows of node k+1 when they read U_k
        if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
            auto sink = weighted_rows<JC>(y, k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
            prod_path_rows<P, SC, S, T>(pp, src, k + 1, -1, n, -1, sink);
        }
    }
    // Lagrange cost: the unit of node k (trapeze) or of step k, and the cost of step k-1 where it reads X_k (midpoint, implicit Euler)
    if constexpr (P::HAS_LAGRANGE) {
        const double sg = hp.sigma;
        if (SC == SC_TRAPEZE || k < L.N) {
            const T c = prod_lagrange_unit<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk});
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = acc[d] + sg * c.ab[d];
        }
        if (SC == SC_MIDPOINT && L.euler != 1 && k >= 1 && hits_x) {
            const T c = prod_lagrange_unit<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1});
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = acc[d] + sg * c.ab[d];
        }
    }
    prod_write_out<JC, nv>(acc, g0, bk, pp.out + k * (int64_t)L.blk, gv);
}

// the unit pass and the finish of ctd_prod_kernels.hpp (prod_units_body, prod_finish_body) around the second-order lanes
template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) hprod_units_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    prod_units_body<P::NV, SH>(hp.p, (int)blockIdx.x, wsum,
                               [&](int64_t k, int q, double* gv) { hprod_unit_body<P, SC, S, SH>(hp, xu, k, q, gv); });
}

template <class P, bool SH = false>
__global__ void __launch_bounds__(64) hprod_finish_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    constexpr int JC = HProdDirs<P>::JC;
    prod_finish_body<P, JC, true, SH>(hp.p, bv, [&](int g0) { return HSeedSrc<JC>{xu, hp.vt, g0, finish_where<SH>(hp.p)}; }, hp.sigma);
}

#if !defined(__HIPCC_RTC__)
// ---- launcher (launch_prod_units, instantiated per registry problem in ctd_pkern_*.hip) ----------------------------------
struct HprodKernels {
    using Params = HProdParams;
    static constexpr bool kShardForm = true;
    static ProdParams& prod(Params& a) { return a.p; }
    static const ProdParams& prod(const Params& a) { return a.p; }
    template <class P, int SC, int S, bool SH> static constexpr auto units = &hprod_units_kernel<P, SC, S, SH>;
    template <class P, bool SH> static constexpr auto finish = &hprod_finish_kernel<P, SH>;
};

#define CTD_HPROD_LAUNCHERS(X, P)                                                                                        \
    X template hipError_t launch_prod_units<P, HprodKernels, false>(const HProdParams&, const double*, hipStream_t);     \
    X template hipError_t launch_prod_units<P, HprodKernels, true>(const HProdParams&, const double*, hipStream_t);
#define CTD_INSTANTIATE_HPROD(P) CTD_HPROD_LAUNCHERS(, P)
#define CTD_EXTERN_HPROD(P) CTD_HPROD_LAUNCHERS(extern, P)
#endif  // !__HIPCC_RTC__

}  // namespace ctd
