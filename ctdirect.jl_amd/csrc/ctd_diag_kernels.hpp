// ctd_diag_kernels.hpp -- matrix-free diagonals of the blocks of the KKT matrix K = [[H + Sx, J'], [J, -Sc]]: what a first-level
// (scaling) preconditioner of the operator ctd_kktprod needs, and what gradient-based NLP scaling is computed from:
//
//   hdiag:     Hd_j  = (sigma H_f(x) + sum_r y_r H_{c_r}(x))_jj                       (nvar entries)
//   jsq_rows:  out_r = sum_j wx_j J_rj^2 = diag(J diag(wx) J')_r                       (ncon entries)
//   jsq_cols:  out_j = sum_r wc_r J_rj^2 = diag(J' diag(wc) J)_j                       (nvar entries)
//
// H and J are the structural ones of ctd_hprod_kernels.hpp / ctd_prod_kernels.hpp; nothing here assembles them, reads the emit
// tables or the pattern: the results are the same bits for every pattern_mode / value_order of one transcription.
//
//   hdiag:     hprod with the tangent equal to the lane's own seed.  One lane per (node k, direction j of node k's block and v) on
//              Dual2<1> whose a and b both carry e_j: the ab part of every piece of the Lagrangian that reads the variable is
//              e_j' H e_j.  The pieces, the skip rules and the Lagrange units are hprod_unit_body's; the rows the one-point schemes
//              read through the identity have no second derivative.  The v entries go through the per-workgroup partial sums;
//              the finish (prod_finish_body, unchanged) adds the boundary rows and the Mayer term to X_1, X_{N+1} and v, then the
//              partials in block order.
//   jsq_cols:  the general jtprod lane (node k, chunk of JC directions of node k's block and v) on Dual<JC> with unit seeds; the
//              sink adds wc_r b[d]^2 where jtprod adds w_r b[d].  The Gauss-Legendre shortcut of jtprod_irk_step is NOT used:
//              it seeds x_kj and applies the chain rule when it writes, and squares do not pass through the chain rule -- X_k and
//              K_l are seeded themselves.  The identity rows of the one-point schemes add wc_r * 1 to the X_k entries.  Rows are
//              added in the order of the lane's evaluations: step k, path rows of node k, step k-1, path rows of node k+1;
//              the finish adds the boundary rows and the v partials in block order.
//   jsq_rows:  row ownership is jprod's: one lane per node k owns the rows of step k and the path rows of node k (lane N: the
//              final path rows and the boundary rows).  SUMMATION ORDER of a row: the lane walks the directions the row's
//              evaluation reads in chunks of JC in ascending direction id, and within a chunk adds wx_j b[d]^2 for d = 0..JC-1,
//              every row sum starting from 0.0.  Direction ids: step rows -- node k's block [0, blk), X_{k+1} [blk, blk + n),
//              on the trapeze U_{k+1} behind it, then v; path rows -- X_k [0, n), the control block read [n, n + cu), v;
//              boundary rows -- X_1, X_{N+1}, v.  One launch, no reduction across lanes.
//
// Two launches (units, finish) for hdiag and jsq_cols, one for jsq_rows.  No atomics, fixed summation order.
//
// On a shard of the grid (ctd_hdiag_shard_dev_async, ctd_jsq_rows_shard_dev_async, ctd_jsq_cols_shard_dev_async: the SH = true
// instantiations) the same lanes run over the nodes of the shard's steps only, as the products' lanes do (ProdParams,
// ctd_prod_kernels.hpp): the lanes at the shard's two ends resolve every region of the iterate they read through buf(), the
// finishes add the boundary rows' (hdiag: and the Mayer term's) entries the shard owns, and the nv entries of hdiag / jsq_cols are
// the shard's partial sums.  Weights and multipliers are always read from the pointer passed, at global indices.
#pragma once
#include "ctd_hprod_kernels.hpp"

namespace ctd {

// ---- hdiag ----------------------------------------------------------------------------------------------------------------
// direction id g0 carries the tangent AND the seed: ab = e_g0' H e_g0
template <bool SH = false> struct DiagSeedSrc {
    const double* x;
    int g0;
    CTD_HD const double* buf(int64_t) const { return x; }
    CTD_HD Dual2<1> at(const double* xb, int64_t g, int dir) const {
        Dual2<1> r; r.v = xb[g];
        const double s = (dir >= 0 && dir == g0) ? 1.0 : 0.0;
        r.a = s; r.b[0] = s; r.ab[0] = 0.0;
        return r;
    }
    CTD_HD Dual2<1> at(int64_t g, int dir) const { return at(x, g, dir); }
};
// On a shard: where x is found (XWhere, ctd_prod_kernels.hpp), buf() as HSeedSrc's.  A type of its own: with the member in the
// whole-grid source too -- null there, folded away -- the whole-grid unit kernels came out of the compiler as other code.
template <> struct DiagSeedSrc<true> : DiagSeedSrc<false> {
    XWhere wh;
    CTD_HD const double* buf(int64_t g) const { return (wh.nr && wh.edge) ? xnear(*wh.nr, x, g) : x; }
};
template <bool SH> CTD_HD DiagSeedSrc<SH> diag_src(const double* xu, int g0, const XWhere& wh) {
    if constexpr (SH) return DiagSeedSrc<true>{{xu, g0}, wh};
    else return DiagSeedSrc<false>{xu, g0};
}

// lane (node k, direction q of node k's variables): its block (bk entries) and v [bk, bk + nv), as hprod_unit_body with JC = 1
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void hdiag_unit_body(const HProdParams& hp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV;
    using T = Dual2<1>;
    const ProdParams& pp = hp.p;
    const Layout& L = pp.L;
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;         // the last node of the other schemes owns X_{N+1} only
    const int g0 = q;
    if (g0 >= bk + nv) return;
    const DiagSeedSrc<SH> src = diag_src<SH>(xu, g0, prod_where<SH>(pp, k));
    const double* y = pp.dir;
    double acc[1] = {0.0};
    const bool hits_x = g0 < n;                     // an X_k direction
    const bool hits_u = g0 >= n && g0 < n + L.cu && m > 0;      // ... or a control direction
    if (y) {
        if (k < L.N) {
            auto sink = weighted_rows<1>(y, k * (int64_t)L.cb, acc);
            prod_step_rows<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
        }
        if (P::NPATH > 0) {
            auto sink = weighted_rows<1>(y, k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
            prod_path_rows<P, SC, S, T>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
        }
        // rows of step k-1: Gauss-Legendre and explicit Euler read X_{i+1} through the identity only -- no second derivative
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (k >= 1 && !one_point && (hits_x || (SC == SC_TRAPEZE && hits_u))) {
            auto sink = weighted_rows<1>(y, (k - 1) * (int64_t)L.cb, acc);
            prod_step_rows<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
        if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
            auto sink = weighted_rows<1>(y, k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
            prod_path_rows<P, SC, S, T>(pp, src, k + 1, -1, n, -1, sink);
        }
    }
    if constexpr (P::HAS_LAGRANGE) {
        const double sg = hp.sigma;
        if (SC == SC_TRAPEZE || k < L.N) {
            const T c = prod_lagrange_unit<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk});
            acc[0] = acc[0] + sg * c.ab[0];
        }
        if (SC == SC_MIDPOINT && L.euler != 1 && k >= 1 && hits_x) {
            const T c = prod_lagrange_unit<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1});
            acc[0] = acc[0] + sg * c.ab[0];
        }
    }
    prod_write_out<1, nv>(acc, g0, bk, pp.out + k * (int64_t)L.blk, gv);
}

template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) hdiag_units_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    prod_units_body<P::NV, SH>(hp.p, (int)blockIdx.x, wsum,
                               [&](int64_t k, int q, double* gv) { hdiag_unit_body<P, SC, S, SH>(hp, xu, k, q, gv); });
}

// the finish of hprod on the diagonal's seeds: boundary rows (with multipliers) and the Mayer term, then the v partials
template <class P, bool SH = false>
__global__ void __launch_bounds__(64) hdiag_finish_kernel(const HProdParams hp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    prod_finish_body<P, 1, true, SH>(hp.p, bv, [&](int g0) { return diag_src<SH>(xu, g0, finish_where<SH>(hp.p)); }, hp.sigma);
}

// ---- jsq_cols -------------------------------------------------------------------------------------------------------------
// directions per jsq_cols lane and per chunk of a jsq_rows lane: jtprod's chunk, but fewer for the wide OCPs -- their Gauss-Legendre
// lanes are the general ones here (no x_kj shortcut).  The 12-state quadrotor's Gauss-Legendre 3 jsq_cols lane spills 512 bytes of
// scratch per lane with three directions and 76 with two: one direction from 12 states, two from 8.  The host sizes the grid of a
// run-time OCP with the same function.
CTD_HD constexpr int jsq_chunk(int n, int dc) { return n >= 12 ? 1 : (n >= 8 ? 2 : jtprod_chunk(n, dc)); }
template <class P> struct JsqDirs {
    static constexpr int JC = jsq_chunk(P::NX, P::DC);
};
// sink of the row evaluators: acc[d] += wc[r0 + r] * (row r's derivative along direction d)^2; wc null: ones.  Keeps REFERENCES
// to w and acc, like weighted_rows
template <int JC> __device__ __forceinline__ auto squared_rows(const double* const& w, int64_t r0, double (&acc)[JC]) {
    return [&w, r0, &acc](int r, const Dual<JC>& val) {
        const double wr = w ? w[r0 + r] : 1.0;
#pragma unroll
        for (int d = 0; d < JC; ++d) acc[d] = acc[d] + wr * (val.d[d] * val.d[d]);
    };
}

// lane (node k, chunk q): the JC entries in directions [q JC, (q + 1) JC) of node k's variables -- its block (bk entries) and
// v [bk, bk + nv) -- every scheme on the general lane of jtprod_unit_body
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void jsq_cols_unit_body(const ProdParams& pp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = JsqDirs<P>::JC;
    using T = Dual<JC>;
    const Layout& L = pp.L;
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;
    const int g0 = q * JC;
    if (g0 >= bk + nv) return;
    const SeedSrc<JC> src{xu, g0, prod_where<SH>(pp, k)};
    const double* w = pp.dir;
    double acc[JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    const bool hits_x = g0 < n;
    const bool hits_u = g0 < n + L.cu && g0 + JC > n && m > 0;
    if (k < L.N) {
        auto sink = squared_rows<JC>(w, k * (int64_t)L.cb, acc);
        prod_step_rows<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
    }
    if (P::NPATH > 0) {
        auto sink = squared_rows<JC>(w, k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
        prod_path_rows<P, SC, S, T>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
    }
    if (k >= 1) {
        const int64_t r0 = (k - 1) * (int64_t)L.cb;
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (one_point) {        // the X_{i+1} column of the state rows is the identity: wc_r * 1^2
            if (hits_x) {
#pragma unroll
                for (int d = 0; d < JC; ++d)
                    if (g0 + d < n) acc[d] = acc[d] + (w ? w[r0 + g0 + d] : 1.0);
            }
        } else if (hits_x || (SC == SC_TRAPEZE && hits_u)) {
            auto sink = squared_rows<JC>(w, r0, acc);
            prod_step_rows<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
    }
    if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
        auto sink = squared_rows<JC>(w, k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
        prod_path_rows<P, SC, S, T>(pp, src, k + 1, -1, n, -1, sink);
    }
    prod_write_out<JC, nv>(acc, g0, bk, pp.out + k * (int64_t)L.blk, gv);
}

template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) jsq_cols_units_kernel(const ProdParams pp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    prod_units_body<P::NV, SH>(pp, (int)blockIdx.x, wsum,
                               [&](int64_t k, int q, double* gv) { jsq_cols_unit_body<P, SC, S, SH>(pp, xu, k, q, gv); });
}

// The finish, one wave.  prod_finish_body fixes its row sink (weighted_rows) and needs multipliers; here the sink squares and the
// weights may be null.  Chunks, directions, the ordered sum of the v partials and the shard rules (SH: chunks on the shards that
// own X_1 or X_{N+1} only, an entry added where the shard owns it, the nv entries the shard's partial sums) are prod_finish_body's.
template <class P, bool SH = false>
__global__ void __launch_bounds__(64) jsq_cols_finish_kernel(const ProdParams pp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    constexpr int n = P::NX, nv = P::NV, nb = P::NBC, JC = JsqDirs<P>::JC;
    const Layout& L = pp.L;
    const int lane = (int)threadIdx.x;
    if (lane < kMaxNV) bv[lane] = 0.0;
    __syncthreads();
    if constexpr (nb > 0) {
        const bool first = !SH || pp.owns_first, last = !SH || pp.owns_last;
        const int64_t gf = L.N * (int64_t)L.blk;
        for (int g0 = lane * JC; (first || last) && g0 < 2 * n + nv; g0 += 64 * JC) {
            const SeedSrc<JC> src{xu, g0, finish_where<SH>(pp)};
            double acc[JC];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = 0.0;
            auto sink = squared_rows<JC>(pp.dir, L.ncon - L.bc, acc);
            prod_boundary_rows<P, Dual<JC>>(pp, src, true, sink);
#pragma unroll
            for (int d = 0; d < JC; ++d) {
                const int g = g0 + d;
                if (g < n) { if (first) pp.out[g] += acc[d]; }
                else if (g < 2 * n) { if (last) pp.out[gf + g - n] += acc[d]; }
                else if (g < 2 * n + nv) { if (last) bv[g - 2 * n] = acc[d]; }
            }
        }
    }
    __syncthreads();
    if constexpr (nv > 0) {
        for (int j = 0; j < nv; ++j) {
            const double s = ordered_rows_sum<kMaxNV>(pp.partial, pp.nblocks, j);
            if (lane == 0) pp.out[L.v_off + j] = s + bv[j];
        }
    }
}

// ---- jsq_rows -------------------------------------------------------------------------------------------------------------
// One evaluation group of a row owner: NR rows over D directions in chunks of JC (ascending), row r's sum in acc[r].
// eval(src, sink): the row evaluator on Dual<JC>; widx(g): where direction g's weight is found in wx (null: ones).
// SH: lane k finds the iterate where prod_where says; the weights are read from wx at global indices always
template <int JC, int NR, bool SH, class Eval, class WIdx>
__device__ __forceinline__ void jsq_rows_group(const ProdParams& pp, int64_t k, const double* xu, const double* wx, int D, double (&acc)[NR],
                                               Eval&& eval, WIdx&& widx) {
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    for (int g0 = 0; g0 < D; g0 += JC) {
        // The chunk is the same in every lane, so the compiler would keep every seed comparison in scalar registers: the wide
        // OCPs then run out of them and reserve spill slots in scratch.  The empty statement moves the seeds' base to a vector
        // register.
        int gs = g0;
        asm volatile("" : "+v"(gs));
        const SeedSrc<JC> src{xu, gs, prod_where<SH>(pp, k)};
        double wj[JC];
#pragma unroll
        for (int d = 0; d < JC; ++d) wj[d] = g0 + d < D ? (wx ? wx[widx(g0 + d)] : 1.0) : 0.0;
        auto sink = [&](int r, const Dual<JC>& val) __attribute__((always_inline)) {
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[r] = acc[r] + wj[d] * (val.d[d] * val.d[d]);
        };
        eval(src, sink);
    }
}

// On a shard (SH) the direction ids and the weights' indices keep this layout; the iterate's values of X_{k+1} (U_{k+1}), of the
// control block the path rows read and of X_1 / X_{N+1} come through buf() per region in the row evaluators.
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void jsq_rows_unit_body(const ProdParams& pp, const double* __restrict__ xu, int64_t k) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, p = P::NPATH, nb = P::NBC, JC = JsqDirs<P>::JC;
    constexpr int EQ = SC == SC_IRK ? n * (S + 1) : n;         // rows of a step
    using T = Dual<JC>;
    const Layout& L = pp.L;
    const double* wx = pp.dir;
    double* out = pp.out;
    const int64_t b0 = k * (int64_t)L.blk;
    if (k < L.N) {
        // node k's block, X_{k+1} (trapeze: and U_{k+1}) -- contiguous behind it in x -- then v
        const int vd = L.blk + n + (SC == SC_TRAPEZE ? m : 0);
        const ProdRoles ro{0, n, L.blk, SC == SC_TRAPEZE ? L.blk + n : -1, vd};
        double acc[EQ > 0 ? EQ : 1];
        jsq_rows_group<JC, (EQ > 0 ? EQ : 1), SH>(
            pp, k, xu, wx, vd + nv, acc,
            [&](const SeedSrc<JC>& src, auto& sink) __attribute__((always_inline)) {
                prod_step_rows<P, SC, S, T>(pp, src, k, ro, sink);
            },
            [&](int g) __attribute__((always_inline)) { return g < vd ? b0 + g : L.v_off + (g - vd); });
        const int64_t r0 = k * (int64_t)L.cb;
#pragma unroll
        for (int r = 0; r < EQ; ++r) out[r0 + r] = acc[r];
    }
    if constexpr (p > 0) {
        const int vd = n + L.cu;
        const int64_t ub = path_ctrl_node(L, k) * (int64_t)L.blk;
        double acc[p];
        jsq_rows_group<JC, p, SH>(
            pp, k, xu, wx, vd + nv, acc,
            [&](const SeedSrc<JC>& src, auto& sink) __attribute__((always_inline)) { prod_path_rows<P, SC, S, T>(pp, src, k, 0, n, vd, sink); },
            [&](int g) __attribute__((always_inline)) { return g < n ? b0 + g : (g < vd ? ub + g : L.v_off + (g - vd)); });
        const int64_t rp = k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb;
#pragma unroll
        for (int r = 0; r < p; ++r) out[rp + r] = acc[r];
    }
    if constexpr (nb > 0) {
        if (k == L.N) {
            const int64_t gf = L.N * (int64_t)L.blk;
            double acc[nb];
            jsq_rows_group<JC, nb, SH>(
                pp, k, xu, wx, 2 * n + nv, acc,
                [&](const SeedSrc<JC>& src, auto& sink) __attribute__((always_inline)) { prod_boundary_rows<P, T>(pp, src, true, sink); },
                [&](int g) __attribute__((always_inline)) { return g < n ? (int64_t)g : (g < 2 * n ? gf + (g - n) : L.v_off + (g - 2 * n)); });
            const int64_t rb = L.ncon - L.bc;
#pragma unroll
            for (int r = 0; r < nb; ++r) out[rb + r] = acc[r];
        }
    }
}

template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) jsq_rows_kernel(const ProdParams pp, const double* __restrict__ xu) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (SH) {
        if (pp.unit_begin + id < pp.unit_end) jsq_rows_unit_body<P, SC, S, true>(pp, xu, pp.unit_begin + id);
    } else if (id <= pp.L.N) jsq_rows_unit_body<P, SC, S>(pp, xu, id);
}

#if !defined(__HIPCC_RTC__)
// ---- launchers (instantiated per registry problem: whole grid in ctd_dkern_*.hip, the shard forms in ctd_dskern_*.hip) -----
struct HdiagKernels {
    using Params = HProdParams;
    static constexpr bool kShardForm = true;
    static ProdParams& prod(Params& a) { return a.p; }
    static const ProdParams& prod(const Params& a) { return a.p; }
    template <class P, int SC, int S, bool SH> static constexpr auto units = &hdiag_units_kernel<P, SC, S, SH>;
    template <class P, bool SH> static constexpr auto finish = &hdiag_finish_kernel<P, SH>;
};
struct JsqColsKernels {
    using Params = ProdParams;
    static constexpr bool kShardForm = true;
    static ProdParams& prod(Params& a) { return a; }
    static const ProdParams& prod(const Params& a) { return a; }
    template <class P, int SC, int S, bool SH> static constexpr auto units = &jsq_cols_units_kernel<P, SC, S, SH>;
    template <class P, bool SH> static constexpr auto finish = &jsq_cols_finish_kernel<P, SH>;
};
// SH: the grid covers the nodes [unit_begin, unit_end)
template <class P, bool SH = false>
hipError_t launch_jsq_rows(const ProdParams& pp, const double* xu, hipStream_t st) {
    const unsigned grid = (unsigned)(((SH ? pp.unit_end - pp.unit_begin : pp.L.N + 1) + 255) / 256);
    for_scheme<false>(pp.L, [&](auto t) { jsq_rows_kernel<P, t.sc, t.s, SH><<<grid, 256, 0, st>>>(pp, xu); });
    return hipGetLastError();
}

#define CTD_DIAG_LAUNCHERS(X, P)                                                                                        \
    X template hipError_t launch_prod_units<P, HdiagKernels, false>(const HProdParams&, const double*, hipStream_t);    \
    X template hipError_t launch_prod_units<P, JsqColsKernels, false>(const ProdParams&, const double*, hipStream_t);   \
    X template hipError_t launch_jsq_rows<P, false>(const ProdParams&, const double*, hipStream_t);
#define CTD_DIAG_SHARD_LAUNCHERS(X, P)                                                                                  \
    X template hipError_t launch_prod_units<P, HdiagKernels, true>(const HProdParams&, const double*, hipStream_t);     \
    X template hipError_t launch_prod_units<P, JsqColsKernels, true>(const ProdParams&, const double*, hipStream_t);    \
    X template hipError_t launch_jsq_rows<P, true>(const ProdParams&, const double*, hipStream_t);
#define CTD_INSTANTIATE_DIAG(P) CTD_DIAG_LAUNCHERS(, P)
#define CTD_INSTANTIATE_DIAG_SHARD(P) CTD_DIAG_SHARD_LAUNCHERS(, P)
#define CTD_EXTERN_DIAG(P) CTD_DIAG_LAUNCHERS(extern, P) CTD_DIAG_SHARD_LAUNCHERS(extern, P)
#endif  // !__HIPCC_RTC__

}  // namespace ctd
