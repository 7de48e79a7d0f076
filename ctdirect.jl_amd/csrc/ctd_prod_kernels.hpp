// ctd_prod_kernels.hpp -- matrix-free Jacobian products: jprod!(nlp, x, v, Jv) and jtprod!(nlp, x, w, Jtw).
//
// J is the exact derivative of the constraints ctd_cons computes (the STRUCTURAL Jacobian: the rows are differentiated as
// written, whatever pattern the handle emits).  The reference leaves both backends empty (jprod_backend / jtprod_backend =
// EmptyADbackend, src/collocation.jl:104-110); ADNLPModels' own product backends push ForwardDiff duals through c!.
//
//   jprod:  one lane per node k in [0, N]: the rows of step k (C_k^x, C_k^{k,1..s}) and the path rows of node k, evaluated on
//           Dual<1> seeded with the direction's entries, written straight to their final rows; lane N also writes the boundary
//           rows.  No reduction.
//   jtprod: the gradient of w'c(x).  One lane per (node k, chunk of JC directions) of the variables node k owns (its block, and
//           v).  It differentiates, on Dual<JC>, every evaluation that reads those variables: the rows of step k and the path
//           rows of node k, the rows of step k-1 (which read X_k, and U_k on the trapeze), and the path rows of node k+1 when
//           they read U_k (implicit Euler; the final node of the schemes without a final control).  For Gauss-Legendre and
//           explicit Euler the X_{k+1} column of step k's rows is the identity: no re-evaluation there.  Every lane writes the
//           entries of its own directions (owner computes); the d/dv partials are reduced per workgroup with wave shuffles in
//           a fixed order, and jtprod_finish_kernel sums them in block order and adds the boundary rows' contributions to X_1,
//           X_{N+1} and v.  Deterministic: no atomics, fixed summation order.
//
// On a shard of the grid (ctd_jprod_shard_dev_async, ctd_jtprod_shard_dev_async: the SH = true instantiations) the same lanes run
// over the nodes of the shard's steps only, and the finish adds the boundary rows' entries the shard owns: see ProdParams.
//
// The bodies are __device__ functions of (params, x, unit) so other drivers can call them; nothing here reads the emit tables
// or the pattern, so the products are the same bits for every pattern_mode / value_order of one transcription.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#endif

#include "ctd_kernel_body.hpp"      // (what a run-time OCP's functor is compiled against, as for the constraint kernels)
#if !defined(__HIPCC_RTC__)
#include "ctd_problems.hpp"
#endif

namespace ctd {

struct ProdParams {
    Layout L;
    const double* tau;      // normalized time grid (N + 1 entries)
    const double* dir;      // v (jprod, nvar entries) or w (jtprod, ncon entries)
    double* out;            // Jv (ncon) or Jtw (nvar)
    double* partial;        // jtprod: nblocks * kMaxNV partial sums of d/dv
    int32_t nblocks;        // jtprod: workgroups of the unit kernel
    int32_t nch;            // jtprod: direction chunks per node
    // ON A SHARD (ctd_*prod_shard_dev_async, the SH = true instantiations): the nodes [unit_begin, unit_end) of the handle's steps
    // -- node N included on the last shard -- are the only ones evaluated; thread ids, the grid and the partial sums count from
    // unit_begin.  The finish adds the boundary rows' (hprod: and the Mayer term's) part of X_1 on the shard that owns it, of
    // X_{N+1} and v on the last one.  halo set (ctd_set_x_shards): the iterate's entries of other shards come from their owners'
    // buffers, resolved with `near` once per region read by the lanes at the shard's two ends and by the finish; null: xu holds
    // everything the shard reads.  The whole-grid instantiations read none of these.
    int64_t unit_begin, unit_end;
    int32_t owns_first, owns_last;
    const XHalo* halo;
    XNear near;
};

// directions per jtprod lane: three for the wide OCPs -- their Gauss-Legendre 3 lanes need 256 registers with three and spill
// with four (288 bytes of scratch per lane for the 12-state quadrotor); fewer chunks mean fewer repeated primal evaluations.
// The host sizes the grid of a run-time OCP with the same function (n states, dc = its DC).
CTD_HD constexpr int jtprod_chunk(int n, int dc) { return n >= 8 ? 3 : (dc < 4 ? dc : 4); }
template <class P> struct ProdDirs {
    static constexpr int JC = jtprod_chunk(P::NX, P::DC);
};

// direction id of entry c of an input category (base < 0: the category carries no direction in this evaluation)
struct ProdRoles { int xi, bi, xn, un, v; };       // X_i, rest of step i's block (controls, stage variables), X_{i+1}, U_{i+1}, v
CTD_HD int prod_dir(int base, int c) { return base >= 0 ? base + c : -1; }

// Where a source finds the iterate.  x: the launch's own buffer -- v and every block of a whole-grid launch.  On a shard whose
// iterate is read in place, a lane at one of the shard's ends (edge) asks buf(g) ONCE per region it reads -- the block of a step,
// X_1, X_{N+1} -- for the buffer that holds it (xnear, ctd_layout.hpp: compares on kernel arguments, no table load); interior
// lanes and whole-grid launches (nr = null: the test folds away) read x.  The sources' at(xb, g, dir) reads entry g from xb,
// at(g, dir) from x; directions are always read from the pointer the caller passed.
// The rule: an edge lane resolves EVERY region it reads, its own blocks included (xnear returns x for those); an interior lane
// resolves none.  A lane that reads a block of another shard, X_1 or X_{N+1} without being an edge lane is a bug; v is in x always.
struct XWhere {
    const XNear* nr = nullptr;
    bool edge = false;
};
// the lanes that may look at the table: the shard's first node when a shard lies below it (it reads step unit_begin - 1), its last
// node when one lies above (it reads node unit_end), and node N -- jprod's lane of the boundary rows, which read X_1
template <bool SH> CTD_HD XWhere prod_where(const ProdParams& pp, int64_t k) {
    if constexpr (SH)
        return XWhere{&pp.near, pp.halo != nullptr && ((k == pp.unit_begin && !pp.owns_first) || (k + 1 >= pp.unit_end && !pp.owns_last) ||
                                                       (k == pp.L.N && !pp.owns_first))};
    else return XWhere{};
}
// the tangent of jprod: the direction's entry at the same position of x
struct FwdSrc {
    const double* x;
    const double* dx;
    XWhere wh;
    CTD_HD const double* buf(int64_t g) const { return (wh.nr && wh.edge) ? xnear(*wh.nr, x, g) : x; }
    CTD_HD Dual<1> at(const double* xb, int64_t g, int) const { Dual<1> r; r.v = xb[g]; r.d[0] = dx[g]; return r; }
    CTD_HD Dual<1> at(int64_t g, int dir) const { return at(x, g, dir); }
};
// unit seeds of jtprod: direction id `dir` is tangent dir - g0 of this chunk
template <int K> struct SeedSrc {
    const double* x;
    int g0;
    XWhere wh;
    CTD_HD const double* buf(int64_t g) const { return (wh.nr && wh.edge) ? xnear(*wh.nr, x, g) : x; }
    CTD_HD Dual<K> at(const double* xb, int64_t g, int dir) const {
        Dual<K> r; r.v = xb[g];
#pragma unroll
        for (int d = 0; d < K; ++d) r.d[d] = (dir >= 0 && dir - g0 == d) ? 1.0 : 0.0;
        return r;
    }
    CTD_HD Dual<K> at(int64_t g, int dir) const { return at(x, g, dir); }
};

CTD_HD double prod_tau(const ProdParams& pp, int64_t i) { return pp.tau ? pp.tau[i] : (double)i / (double)pp.L.N; }
// get_time_grid (src/DOCP_data.jl:437-458): t_i = t0 + tau_i (tf - t0); with t0 / tf in v the tangent follows the dual arithmetic
template <class P, class T> CTD_HD T prod_time(const ProdParams& pp, const T* V, double tau) {
    const T t0 = (P::IT0 >= 0) ? V[P::IT0 >= 0 ? P::IT0 : 0] : T(pp.L.t0);
    const T tf = (P::ITF >= 0) ? V[P::ITF >= 0 ? P::ITF : 0] : T(pp.L.tf);
    return t0 + tau * (tf - t0);
}
// the node whose control block the path constraints of node k read (get_OCP_control): the node itself on the trapeze; the
// previous step for implicit Euler (u(t_1) = U_1); the last step for the final node of the schemes without a final control
CTD_HD int64_t path_ctrl_node(const Layout& L, int64_t k) {
    if (L.sc == SC_TRAPEZE) return k;
    if (L.sc == SC_MIDPOINT && L.euler == 2) return k == 0 ? 0 : k - 1;
    return k == L.N ? L.N - 1 : k;
}

// rows [C_i^x, C_i^{k,1..s}] of step i on scalar type T: sink(r, value), r in [0, eqs).  Restates the residuals of the
// constraint kernels: trapeze.jl:118-142, midpoint.jl:124-156 (control_steps), euler.jl:141-159, irk.jl:236-308,
// irk_stagewise.jl:394-460.
template <class P, int SC, int S, class T, class Src, class Sink>
__device__ __forceinline__ void prod_step_rows(const ProdParams& pp, const Src& src, int64_t i, const ProdRoles& ro, Sink& sink) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV;
    const Layout& L = pp.L;
    const int64_t b0 = i * (int64_t)L.blk, b1 = (i + 1) * (int64_t)L.blk;
    const double *x0 = src.buf(b0), *x1 = src.buf(b1);
    T V[nv > 0 ? nv : 1];
#pragma unroll
    for (int k = 0; k < nv; ++k) V[k] = src.at(L.v_off + k, prod_dir(ro.v, k));
    const T ti = prod_time<P, T>(pp, V, prod_tau(pp, i)), tip1 = prod_time<P, T>(pp, V, prod_tau(pp, i + 1));
    T xa[n > 0 ? n : 1], f[n > 0 ? n : 1], u[m > 0 ? m : 1];
    if constexpr (SC == SC_TRAPEZE) {
        const T hh = 0.5 * (tip1 - ti);
        T g[n > 0 ? n : 1];
#pragma unroll
        for (int c = 0; c < n; ++c) xa[c] = src.at(x0, b0 + c, prod_dir(ro.xi, c));
#pragma unroll
        for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + c, prod_dir(ro.bi, c));
        P::template dynamics<T>(f, ti, xa, u, V);
#pragma unroll
        for (int c = 0; c < n; ++c) xa[c] = src.at(x1, b1 + c, prod_dir(ro.xn, c));
#pragma unroll
        for (int c = 0; c < m; ++c) u[c] = src.at(x1, b1 + n + c, prod_dir(ro.un, c));
        P::template dynamics<T>(g, tip1, xa, u, V);
#pragma unroll
        for (int c = 0; c < n; ++c) {
            const T xi = src.at(x0, b0 + c, prod_dir(ro.xi, c));
            sink(c, xa[c] - (xi + hh * (f[c] + g[c])));
        }
    } else if constexpr (SC == SC_MIDPOINT) {
        if (L.euler == 0) {
            // x_next = x_i + h_i f(t_s, x_s, U_i^j), j = 1..cs, h_i = h / cs, the same (t_s, x_s) for every control
            const T hi = (tip1 - ti) / (double)L.cs, ts = 0.5 * (ti + tip1);
#pragma unroll
            for (int c = 0; c < n; ++c) xa[c] = 0.5 * (src.at(x0, b0 + c, prod_dir(ro.xi, c)) + src.at(x1, b1 + c, prod_dir(ro.xn, c)));
            T xn[n > 0 ? n : 1];
#pragma unroll
            for (int c = 0; c < n; ++c) xn[c] = src.at(x0, b0 + c, prod_dir(ro.xi, c));
            for (int j = 0; j < L.cs; ++j) {
#pragma unroll
                for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + j * m + c, prod_dir(ro.bi, j * m + c));
                P::template dynamics<T>(f, ts, xa, u, V);
#pragma unroll
                for (int c = 0; c < n; ++c) xn[c] = xn[c] + hi * f[c];
            }
#pragma unroll
            for (int c = 0; c < n; ++c) sink(c, src.at(x1, b1 + c, prod_dir(ro.xn, c)) - xn[c]);
        } else {
            // explicit: f(t_i, X_i, U_i); implicit: f(t_{i+1}, X_{i+1}, U_i)
            const T hi = tip1 - ti;
            const bool expl = L.euler == 1;
#pragma unroll
            for (int c = 0; c < n; ++c) xa[c] = expl ? src.at(x0, b0 + c, prod_dir(ro.xi, c)) : src.at(x1, b1 + c, prod_dir(ro.xn, c));
#pragma unroll
            for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + c, prod_dir(ro.bi, c));
            P::template dynamics<T>(f, expl ? ti : tip1, xa, u, V);
#pragma unroll
            for (int c = 0; c < n; ++c)
                sink(c, src.at(x1, b1 + c, prod_dir(ro.xn, c)) - (src.at(x0, b0 + c, prod_dir(ro.xi, c)) + hi * f[c]));
        }
    } else {
        // stage j: K_j - f(t_i + c_j h, X_i + h sum_l a_jl K_l, U_j); state row: X_{i+1} - (X_i + h sum_j b_j K_j)
        const T hi = tip1 - ti;
        const int ko = n + L.cu;            // first stage variable inside the block
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const T tij = ti + L.c[j] * hi;
#pragma unroll
            for (int c = 0; c < n; ++c) {
                T xc = src.at(x0, b0 + c, prod_dir(ro.xi, c));
#pragma unroll
                for (int l = 0; l < S; ++l) xc = xc + hi * L.a[3 * j + l] * src.at(x0, b0 + ko + l * n + c, prod_dir(ro.bi, L.cu + l * n + c));
                xa[c] = xc;
            }
            const int uo = L.stagewise ? j * m : 0;
#pragma unroll
            for (int c = 0; c < m; ++c) u[c] = src.at(x0, b0 + n + uo + c, prod_dir(ro.bi, uo + c));
            P::template dynamics<T>(f, tij, xa, u, V);
#pragma unroll
            for (int c = 0; c < n; ++c) sink(n + j * n + c, src.at(x0, b0 + ko + j * n + c, prod_dir(ro.bi, L.cu + j * n + c)) - f[c]);
        }
#pragma unroll
        for (int c = 0; c < n; ++c) {
            T sb = L.b[0] * src.at(x0, b0 + ko + c, prod_dir(ro.bi, L.cu + c));
#pragma unroll
            for (int j = 1; j < S; ++j) sb = sb + L.b[j] * src.at(x0, b0 + ko + j * n + c, prod_dir(ro.bi, L.cu + j * n + c));
            sink(c, src.at(x1, b1 + c, prod_dir(ro.xn, c)) - (src.at(x0, b0 + c, prod_dir(ro.xi, c)) + hi * sb));
        }
    }
}

// path rows of node k (stepPathConstraints!, DOCP_functions.jl:122-140): sink(r, value), r in [0, p).  xd / ud / vd: direction
// bases of X_k, of the control block read (the rest of node path_ctrl_node(k)'s block) and of v
template <class P, int SC, int S, class T, class Src, class Sink>
__device__ __forceinline__ void prod_path_rows(const ProdParams& pp, const Src& src, int64_t k, int xd, int ud, int vd, Sink& sink) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, p = P::NPATH;
    if constexpr (p > 0) {
        const Layout& L = pp.L;
        T V[nv > 0 ? nv : 1], x[n > 0 ? n : 1], u[m > 0 ? m : 1], r[p];
#pragma unroll
        for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, prod_dir(vd, j));
        const double* xk = src.buf(k * (int64_t)L.blk);
#pragma unroll
        for (int c = 0; c < n; ++c) x[c] = src.at(xk, k * (int64_t)L.blk + c, prod_dir(xd, c));
        const int64_t ub = path_ctrl_node(L, k) * (int64_t)L.blk + n;
        const double* xc = src.buf(ub);
        if (SC == SC_IRK && L.stagewise) {          // b-weighted stage average (irk_stagewise.jl:197-205)
#pragma unroll
            for (int c = 0; c < m; ++c) {
                T uc = L.b[0] * src.at(xc, ub + c, prod_dir(ud, c));
#pragma unroll
                for (int j = 1; j < S; ++j) uc = uc + L.b[j] * src.at(xc, ub + j * m + c, prod_dir(ud, j * m + c));
                u[c] = uc;
            }
        } else {
#pragma unroll
            for (int c = 0; c < m; ++c) u[c] = src.at(xc, ub + c, prod_dir(ud, c));
        }
        const T t = prod_time<P, T>(pp, V, prod_tau(pp, k));
        P::template path<T>(r, t, x, u, V);
#pragma unroll
        for (int j = 0; j < p; ++j) sink(j, r[j]);
    }
}

// boundary rows B(X_1, X_{N+1}, v) (DOCP_functions.jl:103-111); directions: X_1 [0, n), X_{N+1} [n, 2n), v [2n, 2n + nv)
template <class P, class T, class Src, class Sink>
__device__ __forceinline__ void prod_boundary_rows(const ProdParams& pp, const Src& src, bool seeded, Sink& sink) {
    constexpr int n = P::NX, nv = P::NV, nb = P::NBC;
    if constexpr (nb > 0) {
        const Layout& L = pp.L;
        T x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], V[nv > 0 ? nv : 1], r[nb];
        const int64_t gf = L.N * (int64_t)L.blk;
        const double *xa = src.buf(0), *xb = src.buf(gf);
#pragma unroll
        for (int c = 0; c < n; ++c) { x0[c] = src.at(xa, c, seeded ? c : -1); xf[c] = src.at(xb, gf + c, seeded ? n + c : -1); }
#pragma unroll
        for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, seeded ? 2 * n + j : -1);
        P::template boundary<T>(r, x0, xf, V);
#pragma unroll
        for (int j = 0; j < nb; ++j) sink(j, r[j]);
    }
}

// the part of a number that holds the derivatives along a lane's JC directions: the tangents of a Dual, the mixed second
// derivatives of a Dual2 (whose tangent a is the direction of the Hessian product)
template <int K> CTD_HD double dir_part(const Dual<K>& x, int d) { return x.d[d]; }
template <int K> CTD_HD double dir_part(const Dual2<K>& x, int d) { return x.ab[d]; }
// sink of the row evaluators for the transposed products: acc[d] += w[r0 + r] * (row r's derivative along direction d).
// The sink keeps REFERENCES to w and acc, as the lambdas written out in the lanes did (captured by value, the lanes' code
// objects change): pass w as a named pointer that outlives the sink, never an expression such as `w + off`.
template <int JC> __device__ __forceinline__ auto weighted_rows(const double* const& w, int64_t r0, double (&acc)[JC]) {
    return [&w, r0, &acc](int r, const auto& val) {
        const double wr = w[r0 + r];
#pragma unroll
        for (int d = 0; d < JC; ++d) acc[d] = acc[d] + wr * dir_part(val, d);
    };
}
// the tail of a lane: entry d of acc belongs to direction g0 + d of the node -- block entries [0, bk) go to out, v entries
// [bk, bk + NV) to gv
template <int JC, int NV> __device__ __forceinline__ void prod_write_out(const double* acc, int g0, int bk, double* out, double* gv) {
#pragma unroll
    for (int d = 0; d < JC; ++d) {
        const int g = g0 + d;
        if (g < bk) out[g] = acc[d];
        else if (g < bk + NV) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (g - bk == j) gv[j] = acc[d];
        }
    }
}

// ---- jprod ----------------------------------------------------------------------------------------------------------------
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void jprod_unit_body(const ProdParams& pp, const double* __restrict__ xu, int64_t k) {
    const Layout& L = pp.L;
    const FwdSrc src{xu, pp.dir, prod_where<SH>(pp, k)};
    double* out = pp.out;
    if (k < L.N) {
        const int64_t r0 = k * (int64_t)L.cb;
        auto sink = [&](int r, const Dual<1>& val) { out[r0 + r] = val.d[0]; };
        prod_step_rows<P, SC, S, Dual<1>>(pp, src, k, ProdRoles{0, 0, 0, 0, 0}, sink);
    }
    const int64_t rp = k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb;      // G_k, or G_{N+1} behind the last step
    auto psink = [&](int r, const Dual<1>& val) { out[rp + r] = val.d[0]; };
    prod_path_rows<P, SC, S, Dual<1>>(pp, src, k, 0, 0, 0, psink);
    if (k == L.N) {
        const int64_t rb = L.ncon - L.bc;
        auto bsink = [&](int r, const Dual<1>& val) { out[rb + r] = val.d[0]; };
        prod_boundary_rows<P, Dual<1>>(pp, src, false, bsink);
    }
}

template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) jprod_kernel(const ProdParams pp, const double* __restrict__ xu) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (SH) {
        if (pp.unit_begin + id < pp.unit_end) jprod_unit_body<P, SC, S, true>(pp, xu, pp.unit_begin + id);
    } else if (id <= pp.L.N) jprod_unit_body<P, SC, S>(pp, xu, id);
}

// ---- jtprod ---------------------------------------------------------------------------------------------------------------
// Gauss-Legendre step k < N: X_k and the stage variables K_l reach stage j only through x_kj = X_k + h sum_l a_jl K_l, so the
// lanes differentiate with respect to x_kj itself -- directions [0, n) -- and apply the chain rule when they write:
//   Jtw[X_k]   = sum_j g_j - w_C + w_{C,k-1} + (path rows of node k)
//   Jtw[K_l]   = w_{K_l} + h sum_j a_jl g_j - h b_l w_C
// with g_j = w_{K_j}' d(stage row j) / d x_kj.  Controls [n, n + cu) and v [n + cu, n + cu + nv) are seeded where they are read.
// 25 directions per step instead of 61 for the 12-state quadrotor on Gauss-Legendre 3 (every X / K direction of the general
// lane repeats the same derivative of the stages).
template <class P, int S>
__device__ __forceinline__ void jtprod_irk_step(const ProdParams& pp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = ProdDirs<P>::JC;
    using T = Dual<JC>;
    const Layout& L = pp.L;
    const int g0 = q * JC, du = n, dv = n + L.cu;
    if (g0 >= dv + nv) return;
    const SeedSrc<JC> src{xu, g0};
    const double* w = pp.dir;
    const int64_t b0 = k * (int64_t)L.blk, r0 = k * (int64_t)L.cb;
    const int ko = n + L.cu;
    double acc[JC], gj[S][JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    T V[nv > 0 ? nv : 1];
#pragma unroll
    for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, dv + j);
    const T ti = prod_time<P, T>(pp, V, prod_tau(pp, k)), tip1 = prod_time<P, T>(pp, V, prod_tau(pp, k + 1));
    const T hi = tip1 - ti;
    T xa[n > 0 ? n : 1], f[n > 0 ? n : 1], u[m > 0 ? m : 1];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const T tij = ti + L.c[j] * hi;
#pragma unroll
        for (int c = 0; c < n; ++c) {
            T xc = src.at(b0 + c, -1);
#pragma unroll
            for (int l = 0; l < S; ++l) xc = xc + hi * L.a[3 * j + l] * src.at(b0 + ko + l * n + c, -1);
#pragma unroll
            for (int d = 0; d < JC; ++d) if (c - g0 == d) xc.d[d] = xc.d[d] + 1.0;          // x_kj seeded in place
            xa[c] = xc;
        }
        const int uo = L.stagewise ? j * m : 0;
#pragma unroll
        for (int c = 0; c < m; ++c) u[c] = src.at(b0 + n + uo + c, du + uo + c);
        P::template dynamics<T>(f, tij, xa, u, V);
#pragma unroll
        for (int d = 0; d < JC; ++d) gj[j][d] = 0.0;
#pragma unroll
        for (int c = 0; c < n; ++c) {
            const double wr = w[r0 + n + j * n + c];
#pragma unroll
            for (int d = 0; d < JC; ++d) gj[j][d] = gj[j][d] - wr * f[c].d[d];        // row K_j - f: the K_j term is added below
        }
#pragma unroll
        for (int d = 0; d < JC; ++d) acc[d] = acc[d] + gj[j][d];
    }
    // state rows X_{k+1} - (X_k + h sum_j b_j K_j): through h only here (v directions); X_k and K_l terms below
#pragma unroll
    for (int c = 0; c < n; ++c) {
        double sb = L.b[0] * xu[b0 + ko + c];
#pragma unroll
        for (int j = 1; j < S; ++j) sb = sb + L.b[j] * xu[b0 + ko + j * n + c];
        const double wr = w[r0 + c];
#pragma unroll
        for (int d = 0; d < JC; ++d) acc[d] = acc[d] - wr * (hi.d[d] * sb);
    }
    // path rows of node k (X_k, own controls, v), and of node N when it reads this step's controls
    if (P::NPATH > 0) {
        auto sink = weighted_rows<JC>(w, r0 + L.eqs, acc);
        prod_path_rows<P, SC_IRK, S, T>(pp, src, k, 0, du, dv, sink);
        if (k + 1 == L.N && g0 + JC > du && g0 < dv) {
            auto fsink = weighted_rows<JC>(w, L.N * (int64_t)L.cb, acc);
            prod_path_rows<P, SC_IRK, S, T>(pp, src, k + 1, -1, du, -1, fsink);
        }
    }
    double* out = pp.out + b0;
    const double h = hi.v;
#pragma unroll
    for (int d = 0; d < JC; ++d) {
        const int g = g0 + d;
        if (g < n) {
            double xk = acc[d] - w[r0 + g];
            if (k >= 1) xk = xk + w[r0 - L.cb + g];                // X_k is X_{i+1} of step k-1: the identity
            out[g] = xk;
#pragma unroll
            for (int l = 0; l < S; ++l) {
                double kl = 0.0;
#pragma unroll
                for (int j = 0; j < S; ++j) kl = kl + L.a[3 * j + l] * gj[j][d];
                out[ko + l * n + g] = w[r0 + n + l * n + g] + h * kl - h * L.b[l] * w[r0 + g];
            }
        } else if (g < dv) out[g] = acc[d];
        else if (g < dv + nv) {
#pragma unroll
            for (int j = 0; j < nv; ++j)
                if (g - dv == j) gv[j] = acc[d];
        }
    }
}

// the directions per node of the jtprod lanes (Gauss-Legendre: x_kj, the controls and v; otherwise the node's block and v)
CTD_HD int prod_dirs_per_node(const Layout& L) { return L.sc == SC_IRK ? L.n + L.cu + L.nv : L.blk + L.nv; }

// lane (node k, chunk q): the JC entries of w'J in directions [q JC, (q + 1) JC) of node k's variables -- its block
// (X_k, then controls / stage variables: bk entries) and v [bk, bk + nv).  Block entries go to Jtw, v entries to gv.
// On a shard (SH): the Gauss-Legendre lanes read their own step's block, v and, on the last shard, node N only -- nothing of
// another shard, so they never look at the table; the other schemes' first and last lanes do (step k-1's block, node k+1).
template <class P, int SC, int S, bool SH = false>
__device__ __forceinline__ void jtprod_unit_body(const ProdParams& pp, const double* __restrict__ xu, int64_t k, int q, double* gv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, JC = ProdDirs<P>::JC;
    const Layout& L = pp.L;
    if constexpr (SC == SC_IRK) {
        if (k < L.N) { jtprod_irk_step<P, S>(pp, xu, k, q, gv); return; }
    }
    const int bk = (k < L.N || SC == SC_TRAPEZE) ? L.blk : n;         // the last node of the other schemes owns X_{N+1} only
    const int g0 = q * JC;
    if (g0 >= bk + nv) return;
    const SeedSrc<JC> src{xu, g0, prod_where<SH && SC != SC_IRK>(pp, k)};
    const double* w = pp.dir;
    double acc[JC];
#pragma unroll
    for (int d = 0; d < JC; ++d) acc[d] = 0.0;
    const bool hits_x = g0 < n;                     // the chunk holds X_k directions
    const bool hits_u = g0 < n + L.cu && g0 + JC > n && m > 0;      // ... or control directions
    // rows of step k and path rows of node k: every input of node k carries its direction
    if (k < L.N) {
        auto sink = weighted_rows<JC>(w, k * (int64_t)L.cb, acc);
        prod_step_rows<P, SC, S, Dual<JC>>(pp, src, k, ProdRoles{0, n, -1, -1, bk}, sink);
    }
    if (P::NPATH > 0) {
        auto sink = weighted_rows<JC>(w, k < L.N ? k * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
        prod_path_rows<P, SC, S, Dual<JC>>(pp, src, k, 0, path_ctrl_node(L, k) == k ? n : -1, bk, sink);
    }
    // rows of step k-1: they read X_k (and U_k on the trapeze)
    if (k >= 1) {
        const int64_t r0 = (k - 1) * (int64_t)L.cb;
        const bool one_point = SC == SC_IRK || (SC == SC_MIDPOINT && L.euler == 1);
        if (one_point) {        // the X_{i+1} column of the state rows is the identity
            if (hits_x) {
#pragma unroll
                for (int d = 0; d < JC; ++d)
                    if (g0 + d < n) acc[d] = acc[d] + w[r0 + g0 + d];
            }
        } else if (hits_x || (SC == SC_TRAPEZE && hits_u)) {
            auto sink = weighted_rows<JC>(w, r0, acc);
            prod_step_rows<P, SC, S, Dual<JC>>(pp, src, k - 1, ProdRoles{-1, -1, 0, n, -1}, sink);
        }
    }
    // path rows of node k+1 when they read U_k
    if (P::NPATH > 0 && k < L.N && path_ctrl_node(L, k + 1) == k && hits_u) {
        auto sink = weighted_rows<JC>(w, k + 1 < L.N ? (k + 1) * (int64_t)L.cb + L.eqs : L.N * (int64_t)L.cb, acc);
        prod_path_rows<P, SC, S, Dual<JC>>(pp, src, k + 1, -1, n, -1, sink);
    }
    prod_write_out<JC, nv>(acc, g0, bk, pp.out + k * (int64_t)L.blk, gv);
}

// the unit pass of a transposed product for workgroup `block` (wsum: 4 * kMaxNV doubles of LDS): thread id = (node k, chunk q),
// lane(k, q, gv) writes the entries of its own block and leaves its d/dv entries in gv; their sum over the workgroup becomes row
// `block` of pp.partial (block_partial_sums, ctd_common.hpp)
// SH: node k counts from the shard's first node and stops at its last
template <int NV, bool SH = false, class Lane>
__device__ __forceinline__ void prod_units_body(const ProdParams& pp, int block, double (*wsum)[kMaxNV], Lane&& lane) {
    double gv[NV > 0 ? NV : 1];
#pragma unroll
    for (int j = 0; j < NV; ++j) gv[j] = 0.0;
    const int64_t id = (int64_t)block * blockDim.x + threadIdx.x;
    const int64_t k = id / pp.nch;
    if constexpr (SH) {
        if (pp.unit_begin + k < pp.unit_end) lane(pp.unit_begin + k, (int)(id - k * pp.nch), gv);
    } else if (k <= pp.L.N) lane(k, (int)(id - k * pp.nch), gv);
    if constexpr (NV > 0) block_partial_sums<NV, kMaxNV>(gv, &wsum[0][0], pp.partial + (int64_t)block * kMaxNV);
}

template <class P, int SC, int S, bool SH = false>
__global__ void __launch_bounds__(256) jtprod_units_kernel(const ProdParams pp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    prod_units_body<P::NV, SH>(pp, (int)blockIdx.x, wsum,
                               [&](int64_t k, int q, double* gv) { jtprod_unit_body<P, SC, S, SH>(pp, xu, k, q, gv); });
}

// the finish of a transposed product, one wave: the boundary rows (and, SECOND order: the Mayer term, weight sigma) -- lane l
// differentiates chunks l, l + 64, ... of (X_1, X_{N+1}, v), JC directions each, on the numbers make_src(g0) seeds, and adds to the
// entries it owns -- then the v partials in block order (ordered_rows_sum, ctd_common.hpp).  First order (jtprod): pp.dir is never
// null and the objective has no part in it; second order (hprod): the rows only with multipliers.
// On a shard (SH): the chunks are evaluated by the shards that own X_1 or X_{N+1} only (X_1, X_{N+1} read through the table when
// the iterate is in place), a direction's entry is added where the shard owns it -- X_1 on the first shard, X_{N+1} and v on the
// last -- and pp.partial holds the shard's own blocks: the nv entries of pp.out are the shard's partial sums.
template <class P, int JC, bool SECOND, bool SH = false, class MakeSrc>
__device__ __forceinline__ void prod_finish_body(const ProdParams& pp, double* bv, MakeSrc&& make_src, double sigma = 0.0) {
    constexpr int n = P::NX, nv = P::NV, nb = P::NBC;
    constexpr bool MAYER = SECOND && P::HAS_MAYER;
    const Layout& L = pp.L;
    const int lane = (int)threadIdx.x;
    if (lane < kMaxNV) bv[lane] = 0.0;
    __syncthreads();
    const bool rows = nb > 0 && (!SECOND || pp.dir != nullptr);
    const bool first = !SH || pp.owns_first, last = !SH || pp.owns_last;
    if ((rows || MAYER) && (first || last)) {
        const int64_t gf = L.N * (int64_t)L.blk;
        for (int g0 = lane * JC; g0 < 2 * n + nv; g0 += 64 * JC) {
            const auto src = make_src(g0);
            using T = decltype(src.at(0, 0));
            double acc[JC];
#pragma unroll
            for (int d = 0; d < JC; ++d) acc[d] = 0.0;
            if (rows) {
                auto sink = weighted_rows<JC>(pp.dir, L.ncon - L.bc, acc);
                prod_boundary_rows<P, T>(pp, src, true, sink);
            }
            if constexpr (MAYER) {        // src/DOCP_functions.jl:35-48; directions as the boundary rows'
                T x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], V[nv > 0 ? nv : 1];
                const double *xa = src.buf(0), *xb = src.buf(gf);
#pragma unroll
                for (int c = 0; c < n; ++c) { x0[c] = src.at(xa, c, c); xf[c] = src.at(xb, gf + c, n + c); }
#pragma unroll
                for (int j = 0; j < nv; ++j) V[j] = src.at(L.v_off + j, 2 * n + j);
                const T r = P::template mayer<T>(x0, xf, V);
#pragma unroll
                for (int d = 0; d < JC; ++d) acc[d] = acc[d] + sigma * dir_part(r, d);
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
            if (lane == 0) pp.out[L.v_off + j] = s + bv[j];
        }
    }
}

// the finish's sources: every lane may look at the table (X_1 and X_{N+1} are the only blocks it reads)
template <bool SH> CTD_HD XWhere finish_where(const ProdParams& pp) {
    if constexpr (SH) return XWhere{&pp.near, pp.halo != nullptr};
    else return XWhere{};
}
template <class P, bool SH = false>
__global__ void __launch_bounds__(64) jtprod_finish_kernel(const ProdParams pp, const double* __restrict__ xu) {
    __shared__ double bv[kMaxNV];
    constexpr int JC = ProdDirs<P>::JC;
    prod_finish_body<P, JC, false, SH>(pp, bv, [&](int g0) { return SeedSrc<JC>{xu, g0, finish_where<SH>(pp)}; });
}

#if !defined(__HIPCC_RTC__)
// ---- launchers (instantiated per registry problem in ctd_pkern_*.hip) ---------------------------------------------------
// SH: the shard form of the kernels (ctd_*prod_shard_dev_async); the grid covers the nodes [unit_begin, unit_end)
template <class P, bool SH = false>
hipError_t launch_jprod(const ProdParams& pp, const double* xu, hipStream_t st) {
    const unsigned grid = (unsigned)(((SH ? pp.unit_end - pp.unit_begin : pp.L.N + 1) + 255) / 256);
    for_scheme<false>(pp.L, [&](auto t) { jprod_kernel<P, t.sc, t.s, SH><<<grid, 256, 0, st>>>(pp, xu); });
    return hipGetLastError();
}
// A transposed product: K names its argument struct (Params; prod(a): the ProdParams inside) and its two kernels.  The units
// kernel over nblocks workgroups, then the finish kernel on one wave; nblocks / nch / partial filled in by the caller
// (enqueue_prod_units, ctd_engine.hip)
struct JtprodKernels {
    using Params = ProdParams;
    static constexpr bool kShardForm = true;        // (the SH = true kernels exist: enqueue_prod_units, ctd_engine.hip)
    static ProdParams& prod(Params& a) { return a; }
    static const ProdParams& prod(const Params& a) { return a; }
    template <class P, int SC, int S, bool SH> static constexpr auto units = &jtprod_units_kernel<P, SC, S, SH>;
    template <class P, bool SH> static constexpr auto finish = &jtprod_finish_kernel<P, SH>;
};
template <class P, class K, bool SH = false>
hipError_t launch_prod_units(const typename K::Params& a, const double* xu, hipStream_t st) {
    const ProdParams& pp = K::prod(a);
    for_scheme<false>(pp.L, [&](auto t) { K::template units<P, t.sc, t.s, SH><<<(unsigned)pp.nblocks, 256, 0, st>>>(a, xu); });
    K::template finish<P, SH><<<1, 64, 0, st>>>(a, xu);
    return hipGetLastError();
}

#define CTD_PROD_LAUNCHERS(X, P)                                                                          \
    X template hipError_t launch_jprod<P, false>(const ProdParams&, const double*, hipStream_t);          \
    X template hipError_t launch_jprod<P, true>(const ProdParams&, const double*, hipStream_t);           \
    X template hipError_t launch_prod_units<P, JtprodKernels, false>(const ProdParams&, const double*, hipStream_t);  \
    X template hipError_t launch_prod_units<P, JtprodKernels, true>(const ProdParams&, const double*, hipStream_t);
#define CTD_INSTANTIATE_PROD(P) CTD_PROD_LAUNCHERS(, P)
#define CTD_EXTERN_PROD(P) CTD_PROD_LAUNCHERS(extern, P)
#endif  // !__HIPCC_RTC__

}  // namespace ctd
