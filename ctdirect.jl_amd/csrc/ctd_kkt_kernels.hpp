// ctd_kkt_kernels.hpp -- the matrix-free product with the regularised augmented (KKT) matrix of an interior-point / SQP step, the
// operator a Krylov solver applies once per inner iteration:
//
//   rx = (sigma H_f(x) + sum_r y_r H_{c_r}(x)) dx + J(x)' dy + sx o dx
//   rc = J(x) dx - sc o dy
//
// H and J are the structural ones of ctd_hprod_kernels.hpp / ctd_prod_kernels.hpp.  The lanes are the hprod lanes: one lane per
// (node k, chunk q of JC directions of the variables node k owns) on Dual2<JC>, whose tangent a is dx and whose b parts are the
// lane's unit seeds.  Of a row r evaluated to `val`, hprod keeps y_r val.ab; the same number also holds
//   val.b  = the row's derivative along the lane's directions: dy_r val.b is the lane's share of J' dy (jtprod's second launch),
//   val.a  = the row's derivative along dx: (J dx)_r (jprod's launch),
// so one sink gives both blocks of the product: acc[d] += y_r val.ab[d] + dy_r val.b[d], and the row's OWNER stores
// rc_r = val.a - sc_r dy_r.  Every row has exactly one owner, the ownership of jprod: lane (k, q = 0) owns the rows of step k
// (k < N) and the path rows of node k (node N: the final path rows); the finish owns the boundary rows, stored by the lane of
// its first chunk from the evaluation that adds their part to X_1.  Every evaluation reads all its inputs through HSeedSrc, which
// sets the tangent of every entry whatever the seeds: val.a is complete in every lane, the owner's included.
//
// What differs from hprod_unit_body: the rows are evaluated without multipliers too (J' dy and J dx need them), and the rows of
// step k-1 of the one-point schemes (Gauss-Legendre, explicit Euler) -- which reach X_k through the identity only and have no
// second derivative there -- contribute dy to the X_k entries as in jtprod_unit_body.  Two launches (units, finish), no atomics,
// fixed summation order; nothing reads the emit tables or the pattern.
//
// On a shard of the grid (ctd_kktprod_shard_dev_async: the SH = true instantiations) the unit pass runs over the nodes of the
// shard's steps, as hprod's does (ProdParams, ctd_prod_kernels.hpp), and reads of another shard exactly what hprod reads: the block
// of step unit_begin - 1, node unit_end and, for the Gauss-Legendre lanes, X_{k+1}.  rc keeps jprod's ownership, so a shard stores
// the rows of its own steps (the last one also the tail rows); re-evaluations of a neighbour's rows add to acc only.  The finish
// evaluates its chunks on the shards that own X_1 or X_{N+1}, adds the X_1 entries on the first shard, the X_{N+1} entries, the v
// entries, sx o dx of the v entries and the boundary rows' entries of rc on the last: the nv entries of rx are partial sums the
// caller adds over the shards.  dx, dy, y, sx and sc are always read from the pointers passed.
#pragma once
#include "ctd_hprod_kernels.hpp"

namespace ctd {

struct KktParams {
    HProdParams h;          // h.p.dir: multipliers y (ncon) or null; h.p.out: rx (nvar); h.vt: dx (nvar); h.sigma: obj_weight
    const double* dy;       // ncon entries
    const double* sx;       // nvar entries or null: the diagonal added to the top block
    const double* sc;       // ncon entries or null: the diagonal subtracted in the bottom block
    double* rc;             // ncon entries
};

// HSeedSrc for the fused lanes.  Its table lookup loads the four neighbour pointers BEFORE it chooses among them: with xnear's
// loads inside the branches, the compiler merges them into one load at a computed offset of the kernel-argument block, which then
// has to live in scratch (448 bytes per lane in every midpoint-class shard instantiation).  Whole-grid launches never get here.
CTD_HD const double* kkt_xnear(const XNear& nr, const double* xu, int64_t g) {
    const double *prev = nr.prev, *next = nr.next, *first = nr.first, *last = nr.last;
    if ((g >= nr.own_lo && g < nr.own_hi) || g >= nr.v_off) return xu;
    const double* p = g >= nr.own_hi ? (g >= nr.last_lo ? last : next) : (g >= nr.prev_lo ? prev : first);
    return p ? p : xu;
}
template <int K> struct KktSrc : HSeedSrc<K> {
    CTD_HD const double* buf(int64_t g) const { return (this->wh.nr && this->wh.edge) ? kkt_xnear(*this->wh.nr, this->x, g) : this->x; }
};

// sink of the row evaluators: rows r0 + r; own: this lane stores the rows' entries of rc
template <int JC> __device__ __forceinline__ auto kkt_rows(const KktParams& kp, int64_t r0, double (&acc)[JC], bool own) {
    return [&kp, r0, &acc, own](int r, const Dual2<JC>& val) {
        const double* y = kp.h.p.dir;
        const double wr = kp.dy[r0 + r];
        if (y) {
            const double yr = y[r0 + r];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = acc[d] + (yr * val.ab[d] + wr * val.b[d]);
        } else {
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = acc[d] + wr * val.b[d];
        }
        if (own) kp.rc[r0 + r] = kp.sc ? val.a - kp.sc[r0 + r] * wr : val.a;
    };
}

// lane (node k, chunk q): the JC entries of rx in directions [q JC, (q + 1) JC) of node k's variables (block entries to rx, v
// entries to gv, as hprod_unit_body); q = 0 also the entries of rc of the rows node k owns
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void kktprod_unit_body(const KktParams& kp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = HProdDirs<P>::JC;
    using T = Dual2<JC>;
    const ProdParams& pp = kp.h.p;
    const Layout& L = pp.L;
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;         // the last node of the other schemes owns X_{N+1} only
    const int g0 = q * JC;
    if (g0 >= bk + nv) return;
    const KktSrc<JC> src{{xu, kp.h.vt, g0, prod_where<SH>(pp, k)}};
    double acc[JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    const bool own = q == 0;
    const bool hits_x = g0 < n;                     // the chunk holds X_k directions
    const bool hits_u = g0 < n + L.cu && g0 + JC > n && m > 0;      // ... or control directions
    // rows of step k and path rows of node k: every input of node k carries its direction
    if (k < L.N) {
        auto sink = kkt_rows<JC>(kp, k * (int64_t)L.cb, acc, own);
        prod_step_rows<P, SC, S, T>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
    }
    if (P::NPATH > 0) {
        auto sink = kkt_rows<JC>(kp, k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc, own);
        prod_path_rows<P, SC, S, T>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
    }
    // rows of step k-1: they read X_k (and U_k on the trapeze); owned by node k-1
    if (k >= 1) {
        const int64_t r0 = (k - 1) * (int64_t)L.cb;
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (one_point) {        // the X_{i+1} column of the state rows is the identity: no second derivative, dy alone
            if (hits_x) {
#pragma unroll
                for (int d = 0; d < JC; ++d)
                    if (g0 + d < n) acc[d] = acc[d] + kp.dy[r0 + g0 + d];
            }
        } else if (hits_x || (SC == SC_TRAPEZE && hits_u)) {
            auto sink = kkt_rows<JC>(kp, r0, acc, false);
            prod_step_rows<P, SC, S, T>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
    }
    // path rows of node k+1 when they read U_k; owned by node k+1
    if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
        auto sink = kkt_rows<JC>(kp, k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc, false);
        prod_path_rows<P, SC, S, T>(pp, src, k + 1, -1, n, -1, sink);
    }
    // Lagrange cost, as hprod_unit_body
    if constexpr (P::HAS_LAGRANGE) {
        const double sg = kp.h.sigma;
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
    // block entries with their diagonal term; the v entries get theirs once, in the finish
    const int64_t b0 = k * (int64_t)L.blk;
#pragma unroll
    for (int d = 0; d < JC; ++d) {
        const int g = g0 + d;
        if (g < bk) pp.out[b0 + g] = kp.sx ? acc[d] + kp.sx[b0 + g] * kp.h.vt[b0 + g] : acc[d];
        else if (g < bk + nv) {
#pragma unroll
            for (int j = 0; j < nv; ++j)
                if (g - bk == j) gv[j] = acc[d];
        }
    }
}

// the unit pass of ctd_prod_kernels.hpp (prod_units_body) around the fused lanes
template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) kktprod_units_kernel(const KktParams kp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    prod_units_body<P::NV, SH>(kp.h.p, (int)blockIdx.x, wsum,
                               [&](int64_t k, int q, double* gv) { kktprod_unit_body<P, SC, S, SH>(kp, xu, k, q, gv); });
}

// The finish, one wave.  prod_finish_body fixes its row sink (weighted_rows on the multipliers) and skips the boundary rows
// without multipliers; here the rows are always evaluated, through kkt_rows, and the lane of chunk 0 stores their entries of rc.
// Chunks, directions, the Mayer term and the ordered sum of the v partials are prod_finish_body's; the v entries also get
// sx o dx.
// On a shard (SH), as prod_finish_body: the chunks are evaluated by the shards that own X_1 or X_{N+1} only (both read through the
// table when the iterate is in place); the X_1 entries are added on the first shard; the X_{N+1} entries, the v entries with their
// sx o dx, and the boundary rows' entries of rc -- tail rows -- on the last.  val.a does not depend on the seeds or on the shard.
template <class P, bool SH = false>
__global__ void __launch_bounds__(64) kktprod_finish_kernel(const KktParams kp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    constexpr int n = P::NX, nv = P::NV, nb = P::NBC, JC = HProdDirs<P>::JC;
    using T = Dual2<JC>;
    const ProdParams& pp = kp.h.p;
    const Layout& L = pp.L;
    const int lane = (int)threadIdx.x;
    if (lane < kMaxNV) bv[lane] = 0.0;
    __syncthreads();
    const bool first = !SH || pp.owns_first, last = !SH || pp.owns_last;
    if constexpr (nb > 0 || P::HAS_MAYER) {
        const int64_t gf = L.N * (int64_t)L.blk;
        for (int g0 = lane * JC; (first || last) && g0 < 2 * n + nv; g0 += 64 * JC) {
            const KktSrc<JC> src{{xu, kp.h.vt, g0, finish_where<SH>(pp)}};
            double acc[JC];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = 0.0;
            if constexpr (nb > 0) {
                auto sink = kkt_rows<JC>(kp, L.ncon - L.bc, acc, g0 == 0 && last);
                prod_boundary_rows<P, T>(pp, src, true, sink);
            }
            if constexpr (P::HAS_MAYER) {        // src/DOCP_functions.jl:35-48; directions as the boundary rows'
                T x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], V[nv > 0 ? nv : 1];
                const double *xa = src.buf(0), *xb = src.buf(gf);
#pragma unroll
                for (int c = 0; c < n; ++c) { x0[c] = src.at(xa, c, c); xf[c] = src.at(xb, gf + c, n + c); }
#pragma unroll
                for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, 2 * n + j);
                const T r = P::template mayer<T>(x0, xf, V);
#pragma unroll
                for (int d = 0; d < JC; ++d) acc[d] = acc[d] + kp.h.sigma * r.ab[d];
            }
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
            if (lane == 0) {
                const double r = s + bv[j];
                pp.out[L.v_off + j] = (kp.sx && last) ? r + kp.sx[L.v_off + j] * kp.h.vt[L.v_off + j] : r;
            }
        }
    }
}

#if !defined(__HIPCC_RTC__)
// ---- launcher (launch_prod_units, instantiated per registry problem in ctd_pkern_*.hip) ----------------------------------
struct KktKernels {
    using Params = KktParams;
    static constexpr bool kShardForm = true;
    static ProdParams& prod(Params& a) { return a.h.p; }
    static const ProdParams& prod(const Params& a) { return a.h.p; }
    template <class P, int SC, int S, bool SH> static constexpr auto units = &kktprod_units_kernel<P, SC, S, SH>;
    template <class P, bool SH> static constexpr auto finish = &kktprod_finish_kernel<P, SH>;
};

#define CTD_KKT_LAUNCHERS(X, P)                                                                                      \
    X template hipError_t launch_prod_units<P, KktKernels, false>(const KktParams&, const double*, hipStream_t);     \
    X template hipError_t launch_prod_units<P, KktKernels, true>(const KktParams&, const double*, hipStream_t);
#define CTD_INSTANTIATE_KKT(P) CTD_KKT_LAUNCHERS(, P)
#define CTD_EXTERN_KKT(P) CTD_KKT_LAUNCHERS(extern, P)
#endif  // !__HIPCC_RTC__

}  // namespace ctd
