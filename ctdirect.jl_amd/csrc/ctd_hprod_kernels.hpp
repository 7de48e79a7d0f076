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
    CTD_HD Dual2<K> at(int64_t g, int dir) const {
        Dual2<K> r; r.v = x[g]; r.a = t[g];
#pragma unroll
        for (int d = 0; d < K; ++d) { r.b[d] = (dir >= 0 && dir - g0 == d) ? 1.0 : 0.0; r.ab[d] = 0.0; }
        return r;
    }
};

// Lagrange cost of quadrature unit i (trapeze: node i; otherwise step i) on scalar type T, in the form of lagrange_unit
// (ctd_kernels.hpp): trapeze.jl:78-110, midpoint.jl:87-116, euler.jl:112-134, irk.jl:179-228, irk_stagewise.jl:344-384
template <class P, int SC, int S, class T, class Src>
__device__ __forceinline__ T prod_lagrange_unit(const ProdParams& pp, const Src& src, int64_t i, const ProdRoles& ro) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV;
    const Layout& L = pp.L;
    const int64_t b0 = i * (int64_t)L.blk, b1 = (i + 1) * (int64_t)L.blk;
    T V[nv > 0 ? nv : 1], xa[n > 0 ? n : 1], u[m > 0 ? m : 1];
#pragma unroll
    for (int k = 0; k < nv; ++k) V[k] = src.at(L.v_off + k, prod_dir(ro.v, k));
    if constexpr (SC == SC_TRAPEZE) {
        const int64_t ia = i == 0 ? 0 : i - 1, ib = i == L.N ? L.N : i + 1;
        const T w = (prod_time<P, T>(pp, V, prod_tau(pp, ib)) - prod_time<P, T>(pp, V, prod_tau(pp, ia))) / 2.0;
#pragma unroll
        for (int c = 0; c < n; ++c) xa[c] = src.at(b0 + c, prod_dir(ro.xi, c));
#pragma unroll
        for (int c = 0; c < m; ++c) u[c] = src.at(b0 + n + c, prod_dir(ro.bi, c));
        return w * P::template lagrange<T>(prod_time<P, T>(pp, V, prod_tau(pp, i)), xa, u, V);
    } else {
        const T ti = prod_time<P, T>(pp, V, prod_tau(pp, i)), tip1 = prod_time<P, T>(pp, V, prod_tau(pp, i + 1));
        const T h = tip1 - ti;
        if constexpr (SC == SC_MIDPOINT) {
            if (L.cs > 1) {
                const T hi = h / (double)L.cs;
#pragma unroll
                for (int c = 0; c < n; ++c) xa[c] = 0.5 * (src.at(b0 + c, prod_dir(ro.xi, c)) + src.at(b1 + c, prod_dir(ro.xn, c)));
                T val(0.0);
                for (int j = 1; j <= L.cs; ++j) {
#pragma unroll
                    for (int c = 0; c < m; ++c) u[c] = src.at(b0 + n + (j - 1) * m + c, prod_dir(ro.bi, (j - 1) * m + c));
                    const T term = hi * P::template lagrange<T>(ti + ((double)j - 0.5) * hi, xa, u, V);
                    val = (j == 1) ? term : val + term;
                }
                return val;
            }
#pragma unroll
            for (int c = 0; c < m; ++c) u[c] = src.at(b0 + n + c, prod_dir(ro.bi, c));
            if (L.euler == 0) {
#pragma unroll
                for (int c = 0; c < n; ++c) xa[c] = 0.5 * (src.at(b0 + c, prod_dir(ro.xi, c)) + src.at(b1 + c, prod_dir(ro.xn, c)));
                return h * P::template lagrange<T>(0.5 * (ti + tip1), xa, u, V);
            }
            const bool expl = L.euler == 1;
#pragma unroll
            for (int c = 0; c < n; ++c) xa[c] = expl ? src.at(b0 + c, prod_dir(ro.xi, c)) : src.at(b1 + c, prod_dir(ro.xn, c));
            return h * P::template lagrange<T>(expl ? ti : tip1, xa, u, V);
        } else {
            const int ko = n + L.cu;
            T local(0.0);
#pragma unroll
            for (int j = 0; j < S; ++j) {
#pragma unroll
                for (int c = 0; c < n; ++c) {
                    T xc = src.at(b0 + c, prod_dir(ro.xi, c));
#pragma unroll
                    for (int l = 0; l < S; ++l) xc = xc + h * L.a[3 * j + l] * src.at(b0 + ko + l * n + c, prod_dir(ro.bi, L.cu + l * n + c));
                    xa[c] = xc;
                }
                const int uo = L.stagewise ? j * m : 0;
#pragma unroll
                for (int c = 0; c < m; ++c) u[c] = src.at(b0 + n + uo + c, prod_dir(ro.bi, uo + c));
                const T term = L.b[j] * P::template lagrange<T>(ti + L.c[j] * h, xa, u, V);
                local = (j == 0) ? term : local + term;
            }
            return h * local;
        }
    }
}

// lane (node k, chunk q): the JC entries of Hv in directions [q JC, (q + 1) JC) of node k's variables -- its block (bk entries)
// and v [bk, bk + nv).  Block entries go to Hv, v entries to gv.
template <class P, int SC, int S>
__device__ __forceinline__ void hprod_unit_body(const HProdParams& hp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = HProdDirs<P>::JC;
    using T = Dual2<JC>;
    const ProdParams& pp = hp.p;
    const Layout& L = pp.L;
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;         // the last node of the other schemes owns X_{N+1} only
    const int g0 = q * JC;
    if (g0 >= bk + nv) return;
    const HSeedSrc<JC> src{xu, hp.vt, g0};
    const double* y = pp.dir;
    double acc[JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    const bool hits_x = g0 < n;                     // the chunk holds X_k directions
    const bool hits_u = g0 < n + L.cu && g0 + JC > n && m > 0;      // ... or control directions
    auto rows_at = [&](int64_t r0) {
        return [&, r0](int r, const T& val) {
            const double wr = y[r0 + r];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = acc[d] + wr * val.ab[d];
        };
    };
    if (y) {
        // rows of step k and path rows of node k: every input of node k carries its direction
        if (k < L.N) {
            auto sink = rows_at(k * (int64_t)L.cb);
            prod_step_rows<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
        }
        if (P::NPATH > 0) {
            auto sink = rows_at(k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb);
            prod_path_rows<P, SC, S, T>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
        }
        // rows of step k-1: they read X_k (and U_k on the trapeze); Gauss-Legendre and explicit Euler read X_{i+1} through the
        // identity only, which has no second derivative
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (k >= 1 && !one_point && (hits_x || (SC == SC_TRAPEZE && hits_u))) {
            auto sink = rows_at((k - 1) * (int64_t)L.cb);
            prod_step_rows<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
        // path rows of node k+1 when they read U_k
        if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
            auto sink = rows_at(k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb);
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
    double* out = pp.out + k * (int64_t)L.blk;
#pragma unroll
    for (int d = 0; d < JC; ++d) {
        const int g = g0 + d;
        if (g < bk) out[g] = acc[d];
        else if (g < bk + nv) {
#pragma unroll
            for (int j = 0; j < nv; ++j)
                if (g - bk == j) gv[j] = acc[d];
        }
    }
}

// body of the unit pass for workgroup `block` (wsum: 4 * kMaxNV doubles of LDS)
template <class P, int SC, int S>
__device__ __forceinline__ void hprod_units_body(const HProdParams& hp, const double* __restrict__ xu, int block, double (*wsum)[kMaxNV]) {
    constexpr int nv = P::NV;
    const ProdParams& pp = hp.p;
    double gv[nv > 0 ? nv : 1];
#pragma unroll
    for (int j = 0; j < nv; ++j) gv[j] = 0.0;
    const int64_t id = (int64_t)block * blockDim.x + threadIdx.x;
    const int64_t k = id / pp.nch;
    if (k <= pp.L.N) hprod_unit_body<P, SC, S>(hp, xu, k, (int)(id - k * pp.nch), gv);
    if constexpr (nv > 0) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int j = 0; j < nv; ++j) {
            double s = gv[j];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            if (lane == 0) wsum[wave][j] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int j = 0; j < nv; ++j) {
                double s = 0.0;
                for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) s += wsum[wv][j];
                pp.partial[(int64_t)block * kMaxNV + j] = s;
            }
        }
    }
}

template <class P, int SC, int S>
__global__ void __launch_bounds__(256) hprod_units_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    hprod_units_body<P, SC, S>(hp, xu, (int)blockIdx.x, wsum);
}

// one wave: the boundary rows and the Mayer term -- lane l differentiates chunks l, l + 64, ... of (X_1, X_{N+1}, v) and adds to
// the entries it owns -- then the v partials in block order (lane l adds blocks l, l + 64, ..., then a fixed shuffle tree)
template <class P>
__device__ __forceinline__ void hprod_finish_body(const HProdParams& hp, const double* __restrict__ xu, double* bv) {
    constexpr int n = P::NX, nv = P::NV, nb = P::NBC, JC = HProdDirs<P>::JC;
    using T = Dual2<JC>;
    const ProdParams& pp = hp.p;
    const Layout& L = pp.L;
    const int lane = (int)threadIdx.x;
    if (lane < kMaxNV) bv[lane] = 0.0;
    __syncthreads();
    const bool rows = nb > 0 && pp.dir != nullptr;
    if (rows || P::HAS_MAYER) {
        const int64_t gf = L.N * (int64_t)L.blk;
        for (int g0 = lane * JC; g0 < 2 * n + nv; g0 += 64 * JC) {
            const HSeedSrc<JC> src{xu, hp.vt, g0};
            double acc[JC];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = 0.0;
            if (rows) {
                const int64_t rb = L.ncon - L.bc;
                auto sink = [&](int r, const T& val) {
                    const double wr = pp.dir[rb + r];
#pragma unroll
                    for (int d = 0; d < JC; ++d) acc[d] = acc[d] + wr * val.ab[d];
                };
                prod_boundary_rows<P, T>(pp, src, true, sink);
            }
            if constexpr (P::HAS_MAYER) {        // src/DOCP_functions.jl:35-48; directions as the boundary rows'
                T x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], V[nv > 0 ? nv : 1];
#pragma unroll
                for (int c = 0; c < n; ++c) { x0[c] = src.at(c, c); xf[c] = src.at(gf + c, n + c); }
#pragma unroll
                for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, 2 * n + j);
                const T r = P::template mayer<T>(x0, xf, V);
#pragma unroll
                for (int d = 0; d < JC; ++d) acc[d] = acc[d] + hp.sigma * r.ab[d];
            }
#pragma unroll
            for (int d = 0; d < JC; ++d) {
                const int g = g0 + d;
                if (g < n) pp.out[g] += acc[d];
                else if (g < 2 * n) pp.out[gf + g - n] += acc[d];
                else if (g < 2 * n + nv) bv[g - 2 * n] = acc[d];
            }
        }
    }
    __syncthreads();
    if constexpr (nv > 0) {
        for (int j = 0; j < nv; ++j) {
            double s = 0.0;
            for (int b = lane; b < pp.nblocks; b += 64) s += pp.partial[(int64_t)b * kMaxNV + j];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            if (lane == 0) pp.out[L.v_off + j] = s + bv[j];
        }
    }
}

template <class P>
__global__ void __launch_bounds__(64) hprod_finish_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    hprod_finish_body<P>(hp, xu, bv);
}

#if !defined(__HIPCC_RTC__)
// ---- launchers (instantiated per registry problem in ctd_pkern_*.hip) ---------------------------------------------------
// hp.p.nblocks / nch / partial filled in by the caller (enqueue_hprod)
template <class P>
hipError_t launch_hprod(const HProdParams& hp, const double* xu, hipStream_t st) {
    const int sc = hp.p.L.sc, s = hp.p.L.s;
    const unsigned grid = (unsigned)hp.p.nblocks;
    if (sc == SC_TRAPEZE) hprod_units_kernel<P, SC_TRAPEZE, 1><<<grid, 256, 0, st>>>(hp, xu);
    else if (sc == SC_MIDPOINT) hprod_units_kernel<P, SC_MIDPOINT, 1><<<grid, 256, 0, st>>>(hp, xu);
    else if (s == 1) hprod_units_kernel<P, SC_IRK, 1><<<grid, 256, 0, st>>>(hp, xu);
    else if (s == 2) hprod_units_kernel<P, SC_IRK, 2><<<grid, 256, 0, st>>>(hp, xu);
    else hprod_units_kernel<P, SC_IRK, 3><<<grid, 256, 0, st>>>(hp, xu);
    hprod_finish_kernel<P><<<1, 64, 0, st>>>(hp, xu);
    return hipGetLastError();
}
template <class P> int hprod_chunk_of() { return HProdDirs<P>::JC; }

#define CTD_INSTANTIATE_HPROD(P)                                                      \
    template hipError_t launch_hprod<P>(const HProdParams&, const double*, hipStream_t); \
    template int hprod_chunk_of<P>();
#define CTD_EXTERN_HPROD(P)                                                                  \
    extern template hipError_t launch_hprod<P>(const HProdParams&, const double*, hipStream_t); \
    extern template int hprod_chunk_of<P>();
#endif  // !__HIPCC_RTC__

}  // namespace ctd
