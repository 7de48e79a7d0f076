// ctd_kernels.hpp -- __global__ wrappers around the phase functions of ctd_kernel_body.hpp, plus the objective kernels.
// Included by the per-problem translation units (ctd_kern_*.hip), which explicitly instantiate launch_* for one OCP
// so the registry compiles in parallel.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#endif

#include "ctd_kernel_body.hpp"
#if !defined(__HIPCC_RTC__)
#include "ctd_problems.hpp"
#endif

namespace ctd {

// Fused constraints + sparse Jacobian values.  One workgroup = one tile of time steps (block 0 = edge block when
// kp.has_edge).  Dynamic LDS = lds_doubles(kp) * 8 bytes.
// DBG = true is the diagnostics instantiation (ctd_debug_stamps, env CTD_DEBUG_STOP): phase stamps and early returns.  The
// default instantiation holds neither, so no launch pays for their branches or their kernel-argument loads.
#ifndef CTD_MULTI_TILE_LOOP
#define CTD_MULTI_TILE_LOOP 0
#endif
constexpr bool kMultiTileLoop = CTD_MULTI_TILE_LOOP != 0;

template <bool DBG>
__device__ __forceinline__ void ctd_stamp(const KParams& kp, int slot) {
    if constexpr (DBG) {
        if (kp.stamps && threadIdx.x == 0) {
            unsigned long long* p = kp.stamps + ((size_t)blockIdx.x * 6 + slot) * 2;
            p[0] = wall_clock64();   // constant 100 MHz counter, comparable across workgroups
            p[1] = clock64();        // shader cycles
        }
    }
}

// The kernel arguments are read with scalar loads where they are first used; behind branches that is one dependent
// scalar-cache miss after the other (nine rounds in the first version of this kernel, ~1 us before the first load of x was
// issued).  Naming every field the tile path needs as an input of one empty asm statement makes the compiler issue all their
// loads back to back at the top of the kernel: one miss latency, then everything sits in scalar registers.
template <int S, bool LEAN = false>
__device__ __forceinline__ void ctd_pin_kernargs(const KParams& kp, const double* xu) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LEAN) {
        // the lean variant: neither the shard table nor the early-emission fields, and none of what its static layout fixes (block
        // sizes, counts, Butcher tables, the divisor cb)
        asm volatile("" ::"s"(kp.has_edge), "s"(kp.ntiles), "s"(kp.T), "s"(kp.HL), "s"(kp.HH), "s"(kp.step_begin),
                     "s"(kp.step_end), "s"(kp.L.N), "s"(kp.L.v_off), "s"(kp.L.stagewise), "s"(kp.L.euler), "s"(kp.tau), "s"(kp.L.t0),
                     "s"(kp.L.tf), "s"(xu), "s"(blockDim.x));
        asm volatile("" ::"s"(kp.tmpl), "s"(kp.vtmpl), "s"(kp.Lseg), "s"(kp.vr), "s"(kp.div_Lseg.M), "s"(kp.div_vr.M),
                     "s"(kp.div_Lseg.d), "s"(kp.div_vr.d), "s"(kp.seg_base), "s"(kp.reg_first), "s"(kp.reg_last),
                     "s"(kp.vcol_base[0]), "s"(kp.c), "s"(kp.vals));
        return;
    }
    asm volatile("" ::"s"(kp.has_edge), "s"(kp.ntiles), "s"(kp.T), "s"(kp.HL), "s"(kp.HH), "s"(kp.step_begin),
                 "s"(kp.step_end), "s"(kp.L.blk), "s"(kp.L.N), "s"(kp.L.v_off), "s"(kp.L.cu), "s"(kp.L.stagewise), "s"(kp.L.nv),
                 "s"(kp.L.cb), "s"(kp.L.eqs), "s"(kp.L.euler), "s"(kp.tau), "s"(kp.L.t0), "s"(kp.L.tf), "s"(xu), "s"(blockDim.x));
    asm volatile("" ::"s"(kp.tmpl), "s"(kp.vtmpl), "s"(kp.Lseg), "s"(kp.vr), "s"(kp.div_cb.M), "s"(kp.div_Lseg.M), "s"(kp.div_vr.M),
                 "s"(kp.div_cb.d), "s"(kp.div_Lseg.d), "s"(kp.div_vr.d), "s"(kp.seg_base), "s"(kp.reg_first), "s"(kp.reg_last),
                 "s"(kp.vcol_base[0]), "s"(kp.c), "s"(kp.vals), "s"(kp.halo), "s"(kp.pos), "s"(kp.n_early), "s"(kp.n_late));
    if (S >= 1) asm volatile("" ::"s"(kp.L.a[0]), "s"(kp.L.b[0]), "s"(kp.L.c[0]));
    if (S >= 2) asm volatile("" ::"s"(kp.L.a[1]), "s"(kp.L.a[3]), "s"(kp.L.a[4]), "s"(kp.L.b[1]), "s"(kp.L.c[1]));
    if (S >= 3) asm volatile("" ::"s"(kp.L.a[2]), "s"(kp.L.a[5]), "s"(kp.L.a[6]), "s"(kp.L.a[7]), "s"(kp.L.a[8]), "s"(kp.L.b[2]), "s"(kp.L.c[2]));
#endif
}

// The same for the emit phase.  The evaluation needs every scalar register it can get, so the values pinned at the top of the
// kernel do not survive it: the compiler re-loads each kernel argument where the emit phase first uses it -- behind a branch
// each, i.e. one scalar-cache round trip after the other again (a dozen `s_load; s_waitcnt lgkmcnt(0)` pairs on the critical path
// of a 1.4 us phase).  Named once more in front of the barrier, they arrive together while the waves wait for each other.
template <bool LEAN = false>
__device__ __forceinline__ void ctd_pin_emit_kernargs(const KParams& kp) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (LEAN)
        asm volatile("" ::"s"(kp.c), "s"(kp.vals), "s"(kp.Lseg), "s"(kp.vr), "s"(kp.div_Lseg.M), "s"(kp.div_vr.M),
                     "s"(kp.div_Lseg.d), "s"(kp.div_vr.d), "s"(kp.seg_base), "s"(kp.reg_first), "s"(kp.reg_last),
                     "s"(kp.vcol_base[0]));
    else
        asm volatile("" ::"s"(kp.c), "s"(kp.vals), "s"(kp.L.cb), "s"(kp.Lseg), "s"(kp.vr), "s"(kp.div_cb.M), "s"(kp.div_Lseg.M), "s"(kp.div_vr.M),
                     "s"(kp.div_cb.d), "s"(kp.div_Lseg.d), "s"(kp.div_vr.d), "s"(kp.seg_base), "s"(kp.reg_first), "s"(kp.reg_last),
                     "s"(kp.vcol_base[0]), "s"(kp.n_early), "s"(kp.c_early), "s"(kp.vr_early), "s"(kp.n_late), "s"(kp.div_late.M), "s"(kp.div_late.d));
#endif
}

// workgroup `block` of the evaluation (the kernel below; also a branch of the fused iteration kernel, ctd_iter_kernels.hpp).
// B = true: the batched kernel (cons_jac_batch_kernel) -- the workgroup evaluates member blockIdx.y of the batch: its iterate at
// xu + blockIdx.y * ldx, its outputs at c + blockIdx.y * ldc, vals + blockIdx.y * ldv (BatchLd, member_out); the tiles, edge
// blocks and every table are the handle's, shared by the members.  B = false compiles none of it.
// LEAN = true: the lean variant (block_halo, ctd_kernel_body.hpp) -- whole iterate, no early emission; picked by launch_cons_jac.
template <class P, int SC, int S, bool DBG, bool B = false, bool LEAN = false>
__device__ __forceinline__ void cons_jac_body(const KParams& kp, const double* __restrict__ xu, int block, double* ctd_lds,
                                              const BatchLd bl = BatchLd{}) {
    if constexpr (B) xu += batch_member() * bl.ldx;
    ctd_pin_kernargs<SC == SC_IRK ? S : 0, LEAN>(kp, xu);
    ctd_stamp<DBG>(kp, 0);
    if (DBG && kp.debug_stop == 1) return;
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    if constexpr (DirectTile<P, SC>::value) {
        // direct driver: no staging of xu, one barrier (see make_direct_ctx); the staged phases below are not instantiated
        const BlockCtx cx = make_direct_ctx<LEAN>(kp, block, ctd_lds, xu, LV<P, SC, S, LEAN>::blk(kp), LEAN ? P::NV : -1);
        const EmitPre pre = emit_prefetch<P, 1, LEAN>(kp, cx, tid, nthr);
        ctd_stamp<DBG>(kp, 1);
        phase_eval<P, SC, S, RegEval<P, SC, S>::value, 1, B, LEAN>(kp, cx, tid, nthr, &pre, bl);
        ctd_pin_emit_kernargs<LEAN>(kp);
        __syncthreads();
        ctd_stamp<DBG>(kp, 2);
        ctd_stamp<DBG>(kp, 3);
        if (DBG && kp.debug_stop >= 2 && kp.debug_stop <= 4) return;
        phase_emit<P, SC, S, 1, B, LEAN>(kp, cx, tid, nthr, &pre, bl);
        ctd_stamp<DBG>(kp, 4);
        if (DBG && kp.stamps) {
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            ctd_stamp<DBG>(kp, 5);
        }
        return;
    }
    BlockCtx cx = make_ctx<LEAN>(kp, block, ctd_lds);
    // codes not staged in LDS (long periods): every code the lane will need is fetched now, the latency hidden behind load + eval
    constexpr int NB = EmitN<P, SC, S>::value;
    EmitPreT<NB> pre = {};
    const bool use_pre = !cx.is_edge && !codes_staged(kp);
    if (use_pre) pre = emit_prefetch<P, NB, LEAN>(kp, cx, tid, nthr);
    phase_load<P, SC, S, true, LEAN>(kp, cx, xu, tid, nthr);
    // multi-tile workgroups (kp.wg_stride > 0; EXPERIMENT, compiled with -DCTD_MULTI_TILE_LOOP=1 only): this workgroup goes on with
    // block + wg_stride, ... -- the templates, v and the lane's codes stay where they are (the period of the tables is the step:
    // the same for every tile), the x slice of the next tile travels while this one is emitted.  One barrier per tile boundary: it
    // orders the emission's reads of the records and the staged copy of the next slice before the next evaluation.
    // Measured on MI355X (profiles/r03_experiments.md): SLOWER than one tile per workgroup -- 12-state quadrotor GL3 124 us against
    // 106, optimized pattern 55.5 against 42.4.  A resident round of workgroups that all start together stays in lock-step (every
    // workgroup evaluates, then every workgroup stores: the memory system idles, then saturates), while the hardware dispatcher
    // starts the next tile whenever a slot frees and so spreads the phases; the loop also costs 30 - 55 registers.
    const int nblk = kp.ntiles + kp.has_edge;
    for (;;) {
        __syncthreads();
        ctd_stamp<DBG>(kp, 1);
        if (DBG && kp.debug_stop == 2) return;
        phase_eval<P, SC, S, false, 1, B, LEAN>(kp, cx, tid, nthr, nullptr, bl);
        ctd_pin_emit_kernargs<LEAN>(kp);
        __syncthreads();
        ctd_stamp<DBG>(kp, 2);
        if (DBG && kp.debug_stop == 3) return;
        if (!Dirs<P>::FUSED && !fin_folded<P, SC, S>(cx)) {     // (block-uniform)
            phase_fin<P, SC, S>(kp, cx, tid, nthr);
            __syncthreads();
        }
        if (SC == SC_TRAPEZE) {
            phase_fin2<P, SC, S>(kp, cx, tid, nthr);
            __syncthreads();
        }
        ctd_stamp<DBG>(kp, 3);
        if (DBG && kp.debug_stop == 4) return;
        block += kp.wg_stride;
        const bool more = kMultiTileLoop && kp.wg_stride > 0 && !cx.is_edge && block < nblk;
        BlockCtx nx = cx;
        TileIn tin{0.0, 0.0, 0.0};
        if (more) {
            nx = make_ctx<LEAN>(kp, block, ctd_lds);
            tin = load_issue<P>(kp, nx, xu, tid, nthr);
        }
        phase_emit_impl<P, SC, S, NB, B, LEAN>(kp, cx, tid, nthr, pre, use_pre, bl);
        ctd_stamp<DBG>(kp, 4);
        if (!more) break;
        load_commit<P, SC, S>(kp, nx, xu, tin, tid, nthr);
        cx = nx;
    }
    if (DBG && kp.stamps) {      // diagnostics: time until this workgroup's stores have left the CU
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        ctd_stamp<DBG>(kp, 5);
    }
}

// Waves per SIMD the kernel is compiled for (the second launch bound caps the registers per lane at 512 / value).  Four: the
// 12-state quadrotor's Gauss-Legendre 3 instantiation needed 129 registers -- ONE more than four waves per SIMD allow -- and ran
// three workgroups per CU where its 15 KiB of LDS would let ten in.  The midpoint kernels with several controls per step
// (195 - 245 registers) and OCPs wider than the registry's keep the compiler's own choice.
template <class P, int SC, int S> struct MinWaves {
    static constexpr int value = (P::NX <= 12 && !(SC == SC_MIDPOINT && S > 1)) ? 4 : 1;
};

template <class P, int SC, int S, bool DBG, bool LEAN = false>
__global__ void __launch_bounds__(P::MAXB, (MinWaves<P, SC, S>::value)) cons_jac_kernel(const KParams kp, const double* __restrict__ xu) {
    extern __shared__ double ctd_lds[];
    cons_jac_body<P, SC, S, DBG, false, LEAN>(kp, xu, (int)blockIdx.x, ctd_lds);
}
// The STATIC-EMIT variant of the lean kernel (ctd_emit_static.hpp): direct tiles whose emit periods are the static ones of
// <P, SC, S> (manual pattern, CSC order, whole grid), launched with NTHR lanes; WT: the emit phase's stores are write-through
// (KParams::wt_store as a constant).  The body is chosen ONCE at entry: the edge workgroups run the lean body as it is, so the
// tile's path -- pin, prefetch, evaluation, barrier, emit -- is one contiguous run of code with the workgroup size a constant.
// Behind the barrier the tile reads no kernel argument at all.
//
// The tile arm reads TileArgs (ctd_layout.hpp) and nothing of kp: every one of its fields is named as an input of the empty asm
// statements at entry, IN FRONT of the edge / tile branch, so the compiler fetches the whole block with a few wide scalar loads
// behind one another and waits once.  The phase functions take a KParams; the arm hands them a local one filled from TileArgs
// (tile_kparams) -- every function is inlined, so that struct never exists: each field read becomes the scalar register the
// entry loads filled, each field the tile does not use a constant zero.  The six values of the emit phase (c, vals, seg_base,
// reg_first, reg_last, vcol_base) pass through an asm statement as outputs: the compiler can then no longer fetch them a second
// time behind the evaluation, it has to keep them (in scalar registers, or in lanes of a vector register where those run out).
template <class P>
__device__ __forceinline__ KParams tile_kparams(const TileArgs& ta) {
    KParams tk{};
    tk.L.N = ta.N; tk.L.v_off = ta.v_off; tk.L.stagewise = ta.stagewise; tk.L.t0 = ta.t0; tk.L.tf = ta.tf;
    tk.tau = ta.tau; tk.T = ta.T; tk.has_edge = ta.has_edge; tk.step_begin = ta.step_begin; tk.step_end = ta.step_end;
    tk.tmpl = ta.tmpl; tk.vtmpl = ta.vtmpl;
    int64_t seg_base = ta.seg_base, reg_first = ta.reg_first, reg_last = ta.reg_last;
    double *c = ta.c, *vals = ta.vals;
    int64_t vb[kMaxNV] = {ta.vcol_base[0], ta.vcol_base[1], ta.vcol_base[2], ta.vcol_base[3]};
#if defined(__HIP_DEVICE_COMPILE__)
    // (the two pointers pass as GLOBAL pointers: a generic one that comes out of an asm statement has lost its address space, and
    // the emit's stores would become flat ones)
    using gdouble = __attribute__((address_space(1))) double;
    gdouble *cg = (gdouble*)c, *vg = (gdouble*)vals;
    asm volatile("" : "+s"(cg), "+s"(vg), "+s"(seg_base), "+s"(reg_first), "+s"(reg_last));
    c = (double*)cg; vals = (double*)vg;
#pragma unroll
    for (int kk = 0; kk < P::NV; ++kk) asm volatile("" : "+s"(vb[kk]));
#endif
    tk.c = c; tk.vals = vals; tk.seg_base = seg_base; tk.reg_first = reg_first; tk.reg_last = reg_last;
#pragma unroll
    for (int kk = 0; kk < P::NV; ++kk) tk.vcol_base[kk] = vb[kk];
    return tk;
}
template <class P, int SC, int S, bool DBG, int NTHR, bool WT>
__device__ __forceinline__ void cons_jac_static_body(const TileArgs& ta, const KParams& kp, int block, double* ctd_lds) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" ::"s"(ta.xu), "s"(ta.tau), "s"(ta.tmpl), "s"(ta.vtmpl), "s"(ta.c), "s"(ta.vals), "s"(ta.step_begin), "s"(ta.step_end),
                 "s"(ta.N), "s"(ta.v_off), "s"(ta.t0), "s"(ta.tf), "s"(ta.seg_base), "s"(ta.reg_first), "s"(ta.reg_last),
                 "s"(ta.vcol_base[0]), "s"(ta.vcol_base[P::NV > 1 ? 1 : 0]), "s"(ta.vcol_base[P::NV > 2 ? 2 : 0]),
                 "s"(ta.vcol_base[P::NV > 3 ? 3 : 0]), "s"(ta.has_edge), "s"(ta.T), "s"(ta.stagewise));
    if constexpr (DBG) asm volatile("" ::"s"(kp.stamps), "s"(kp.debug_stop));      // (diagnostics: in the same round)
#endif
    if (__builtin_expect(block < ta.has_edge, 0)) {
        __builtin_assume(block < kp.has_edge);      // (make_tile_args: the same count -- the lean body's tile path is not compiled here)
        cons_jac_body<P, SC, S, DBG, false, true>(kp, ta.xu, block, ctd_lds);
        return;
    }
    const KParams tk = tile_kparams<P>(ta);
    __builtin_assume(tk.tau != nullptr);        // (make_tile_args: a static tile is never launched without the table, so tau_global
                                                // is its table load -- the division arm and its test are not compiled)
    ctd_stamp<DBG>(kp, 0);
    if (DBG && kp.debug_stop == 1) return;
    const int tid = (int)threadIdx.x;
    const double* __restrict__ xu = ta.xu;
    BlockCtx cx = make_direct_ctx<true>(tk, block, ctd_lds, xu, LV<P, SC, S, true>::blk(tk), P::NV);
    cx.is_edge = 0;          // (this arm)
    cx.edge_part = 0;
    const EmitPre pre = emit_prefetch_static<P, SC, S, NTHR>(tk, tid);
    ctd_stamp<DBG>(kp, 1);
    phase_eval<P, SC, S, RegEval<P, SC, S>::value, 1, false, true, true>(tk, cx, tid, NTHR, &pre, BatchLd{});
    __syncthreads();
    ctd_stamp<DBG>(kp, 2);
    ctd_stamp<DBG>(kp, 3);
    if (DBG && kp.debug_stop >= 2 && kp.debug_stop <= 4) return;
    phase_emit_static<P, SC, S, NTHR, WT>(tk, cx, tid, pre);
    ctd_stamp<DBG>(kp, 4);
    if (DBG && kp.stamps) {
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        ctd_stamp<DBG>(kp, 5);
    }
}
template <class P, int SC, int S, bool DBG, int NTHR, bool WT>
__global__ void __launch_bounds__(NTHR, (MinWaves<P, SC, S>::value)) cons_jac_static_kernel(const TileArgs ta, const KParams kp) {
    extern __shared__ double ctd_lds[];
    cons_jac_static_body<P, SC, S, DBG, NTHR, WT>(ta, kp, (int)blockIdx.x, ctd_lds);
}
// K iterates per launch (ctd_cons_jac_batch_dev_async): grid (tiles, members), the same bodies with B = true
template <class P, int SC, int S>
__global__ void __launch_bounds__(P::MAXB, (MinWaves<P, SC, S>::value)) cons_jac_batch_kernel(const KParams kp, const double* __restrict__ xu,
                                                                                          const BatchLd bl) {
    extern __shared__ double ctd_lds[];
    cons_jac_body<P, SC, S, false, true>(kp, xu, (int)blockIdx.x, ctd_lds, bl);
}

// ---- objective: Mayer + Lagrange quadrature (src/DOCP_functions.jl:23-54) ------------------------------------
// One lane per quadrature unit (trapeze: node, otherwise: step) of the shard; per-workgroup partial sums are
// reduced with wave shuffles and written to partial[blockIdx]; obj_finish_kernel adds them in index order
// (deterministic) together with the Mayer term.
struct ObjParams {
    Layout L;
    const double* tau;
    int64_t unit_begin, unit_end;   // nodes (trapeze) or steps
    int32_t add_mayer;
    double* partial;
    double* out;
    int32_t nblocks;
    // sharded iterate read in place (ctd_set_x_shards): the next shard's first node (midpoint / Euler units of a shard's last step)
    // and X_1 / X_{N+1} of the Mayer term come from the owners' buffers; null: xu holds everything
    const XHalo* halo;
    XNear near;             // (the same buffers in the kernel arguments: one memory round trip per remote entry)
    // batched launches (ctd_obj_batch_dev_async): member b = blockIdx.y reads xu + b * ldx, writes partial[b * nblocks ..] and out[b]
    int64_t ldx;
};

template <class P> __device__ double obj_time(const ObjParams& op, const double* v, int64_t i) {
    const double t0 = (P::IT0 >= 0) ? v[P::IT0 >= 0 ? P::IT0 : 0] : op.L.t0;
    const double tf = (P::ITF >= 0) ? v[P::ITF >= 0 ? P::ITF : 0] : op.L.tf;
    const double tau = op.tau ? op.tau[i] : (double)i / (double)op.L.N;
    return t0 + tau * (tf - t0);
}

template <class P, int SC>
__device__ double lagrange_unit(const ObjParams& op, const double* __restrict__ xu, const double* v, int64_t i) {
    constexpr int n = P::NX, m = P::NU;
    const Layout& L = op.L;
    const double* base = xu + i * (int64_t)L.blk;
    // X_{i+1} sits behind the step's block -- in the next shard's buffer for the last step of a shard of a sharded iterate
    const int64_t gn = (i + 1) * (int64_t)L.blk;
    const double* nxt = ((op.halo && i + 1 >= op.unit_end) ? xnear(op.near, xu, gn) : xu) + gn;      // (only the shard's last unit looks at the table)
    double x[n > 0 ? n : 1], u[m > 0 ? m : 1];
    if (SC == SC_TRAPEZE) {            // trapeze.jl:78-110: node weights h_1/2, (t_{i+1}-t_{i-1})/2, h_N/2
        double w;
        if (i == 0) w = (obj_time<P>(op, v, 1) - obj_time<P>(op, v, 0)) / 2.0;
        else if (i == L.N) w = (obj_time<P>(op, v, L.N) - obj_time<P>(op, v, L.N - 1)) / 2.0;
        else w = (obj_time<P>(op, v, i + 1) - obj_time<P>(op, v, i - 1)) / 2.0;
        for (int c = 0; c < n; ++c) x[c] = base[c];
        for (int c = 0; c < m; ++c) u[c] = base[n + c];
        return w * P::template lagrange<double>(obj_time<P>(op, v, i), x, u, v);
    }
    const double ti = obj_time<P>(op, v, i), tip1 = obj_time<P>(op, v, i + 1);
    const double h = tip1 - ti;
    if (SC == SC_MIDPOINT) {           // midpoint.jl:87-97; Euler (euler.jl:112-134): (t_i, X_i, U_i) or (t_{i+1}, X_{i+1}, U_i)
        if (L.cs > 1) {                // control_steps > 1 (midpoint.jl:99-116): h_i = h / cs, l(t_i + (j - 1/2) h_i, x_s, U_i^j, v), j = 1..cs
            const double hi = h / (double)L.cs;
            for (int c = 0; c < n; ++c) x[c] = 0.5 * (base[c] + nxt[c]);
            double val = 0.0;
            for (int j = 1; j <= L.cs; ++j) {
                for (int c = 0; c < m; ++c) u[c] = base[n + (j - 1) * m + c];
                const double term = hi * P::template lagrange<double>(ti + ((double)j - 0.5) * hi, x, u, v);
                val = (j == 1) ? term : val + term;
            }
            return val;
        }
        for (int c = 0; c < m; ++c) u[c] = base[n + c];
        if (L.euler == 0) {
            for (int c = 0; c < n; ++c) x[c] = 0.5 * (base[c] + nxt[c]);
            return h * P::template lagrange<double>(0.5 * (ti + tip1), x, u, v);
        }
        for (int c = 0; c < n; ++c) x[c] = (L.euler == 1) ? base[c] : nxt[c];
        return h * P::template lagrange<double>(L.euler == 1 ? ti : tip1, x, u, v);
    }
    // irk.jl:179-228 / irk_stagewise.jl:344-384
    const double* K = base + n + L.cu;
    double local = 0.0;
    for (int j = 0; j < L.s; ++j) {
        for (int c = 0; c < n; ++c) {
            double xc = base[c];
            for (int l = 0; l < L.s; ++l) xc = xc + h * L.a[3 * j + l] * K[l * n + c];
            x[c] = xc;
        }
        const double* U = base + n + (L.stagewise ? j * m : 0);
        for (int c = 0; c < m; ++c) u[c] = U[c];
        const double term = L.b[j] * P::template lagrange<double>(ti + L.c[j] * h, x, u, v);
        local = (j == 0) ? term : local + term;
    }
    return h * local;
}

// body of the quadrature pass for workgroup `block` of `nblocks` (wsum: 4+ doubles of LDS); also a branch of the fused
// iteration kernel (iter_main_kernel).  mb: member of a batched launch (xu is already the member's iterate)
template <class P, int SC>
__device__ __forceinline__ void obj_partial_body(const ObjParams& op, const double* __restrict__ xu, int block, int nblocks, double* wsum,
                                                 int64_t mb = 0) {
    double v[P::NV > 0 ? P::NV : 1];
    for (int k = 0; k < P::NV; ++k) v[k] = xu[op.L.v_off + k];
    double acc = 0.0;
    if (P::HAS_LAGRANGE) {
        for (int64_t i = op.unit_begin + (int64_t)block * blockDim.x + threadIdx.x; i < op.unit_end;
             i += (int64_t)nblocks * blockDim.x)
            acc += lagrange_unit<P, SC>(op, xu, v, i);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += wsum[w];
        op.partial[mb * nblocks + block] = s;
    }
}
template <class P, int SC>
__global__ void __launch_bounds__(256) obj_partial_kernel(const ObjParams op, const double* __restrict__ xu) {
    __shared__ double wsum[4];
    const int64_t mb = batch_member();
    obj_partial_body<P, SC>(op, xu + mb * op.ldx, (int)blockIdx.x, (int)gridDim.x, wsum, mb);
}

template <class P>
__device__ __forceinline__ void obj_finish_body(const ObjParams& op, const double* __restrict__ xu, int64_t mb = 0) {
    if (threadIdx.x >= 64) return;
    // one wave: lane l adds the partials l, l + 64, ... in index order, then a fixed shuffle tree (deterministic; the
    // loads of the 64 lanes are in flight together instead of one dependent chain of nblocks loads)
    const double* part = op.partial + mb * op.nblocks;
    double s = 0.0;
    for (int b = threadIdx.x; b < op.nblocks; b += 64) s += part[b];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (threadIdx.x != 0) return;
    double mayer = 0.0;
    if (P::HAS_MAYER && op.add_mayer) {
        constexpr int n = P::NX, nv = P::NV;
        double x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], v[nv > 0 ? nv : 1];
        const int64_t gf = op.L.N * (int64_t)op.L.blk;
        const double* xa = op.halo ? xnear(op.near, xu, 0) : xu;
        const double* xb = op.halo ? xnear(op.near, xu, gf) : xu;
        for (int c = 0; c < n; ++c) { x0[c] = xa[c]; xf[c] = xb[gf + c]; }
        for (int k = 0; k < nv; ++k) v[k] = xu[op.L.v_off + k];
        mayer = P::template mayer<double>(x0, xf, v);
    }
    op.out[mb] = mayer + s;
}
// (one workgroup per member of a batched launch: grid (1, batch))
template <class P>
__global__ void obj_finish_kernel(const ObjParams op, const double* __restrict__ xu) {
    if (blockIdx.x != 0) return;
    const int64_t mb = batch_member();
    obj_finish_body<P>(op, xu + mb * op.ldx, mb);
}

// ---- objective gradient: grad!(nlp, x, g) -----------------------------------------------------------------------------
// In the reference the gradient is ReverseDiff over __objective (gradient_backend = ReverseDiffADGradient,
// src/collocation.jl:127).  Here: forward duals over the Lagrange / Mayer functions + the quadrature's chain rule.
// Owner-computes, no atomics: one lane per quadrature unit writes the gradient entries of its own variables (trapeze:
// node; midpoint: node, gathering the two adjacent steps; Gauss-Legendre: step); the partials with respect to v are
// reduced per workgroup and summed in index order by grad_finish_kernel, which also adds the Mayer term.
struct GradParams {
    Layout L;
    const double* tau;
    double* g;          // nvar, zero-filled before the launch
    double* partial;    // nblocks * kMaxNV
    int32_t nblocks;
    // quadrature units [unit_begin, unit_end) this launch evaluates: all of them (ctd_grad*: the whole objective's gradient), or the
    // units of a shard of the grid (ctd_grad_shard_dev_async: the shard's own entries of g + its partial sums of d/dv)
    int64_t unit_begin, unit_end;
    int32_t owns_first, owns_last;      // the Mayer term's d/dx0 goes to the shard that owns X_1, d/dxf and d/dv to the one that owns X_{N+1}
    // sharded iterate read in place (ctd_set_x_shards): blocks of other shards come from their owners' buffers; null: xu holds everything
    const XHalo* halo;
    XNear near;
    // batched launches (ctd_grad_batch_dev_async): member b = blockIdx.y reads xu + b * ldx, writes g + b * ldg and the partial
    // rows [b * nblocks, (b + 1) * nblocks)
    int64_t ldx, ldg;
};
// start of the variable block of step / node `st` in the buffer that owns it
CTD_HD const double* grad_block(const GradParams& gp, const double* xu, int64_t st) {
    const int64_t g = st * (int64_t)gp.L.blk;
    return (gp.halo ? xnear(gp.near, xu, g) : xu) + g;
}

template <class P> struct LagDirs {
    static constexpr int N = P::NX + P::NU + (P::LAG_T ? 1 : 0) + (P::LAG_V ? P::NV : 0);
    static constexpr int NCH = (N + P::DC - 1) / P::DC;
    static constexpr int NMAY = 2 * P::NX + P::NV;
    static constexpr int NCH_MAY = (NMAY + P::DC - 1) / P::DC;
};

// d lagrange / d (x, u, t, v) at one point, DC directions per pass, chunk index compile-time (no runtime-indexed arrays)
template <class P, int Q>
__device__ __forceinline__ void lagrange_partials(double t, const double* x, const double* u, const double* v, double& val,
                                                  double* lx, double* lu, double& lt, double* lv) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV, DC = P::DC;
    if constexpr (SymLag<P>::value) {          // generated straight-line code (symbolic first derivatives, ctd_sym.hpp)
        double prm[1 + n + m + nv], out[2 + n + m + nv];
        prm[0] = t;
#pragma unroll
        for (int c = 0; c < n; ++c) prm[1 + c] = x[c];
#pragma unroll
        for (int c = 0; c < m; ++c) prm[1 + n + c] = u[c];
#pragma unroll
        for (int c = 0; c < nv; ++c) prm[1 + n + m + c] = v[c];
        SymLag<P>::eval(prm, out);
        val = out[0];
#pragma unroll
        for (int c = 0; c < n; ++c) lx[c] = out[1 + c];
#pragma unroll
        for (int c = 0; c < m; ++c) lu[c] = out[1 + n + c];
        if (P::LAG_T) lt = out[1 + n + m];
        if (P::LAG_V) {
#pragma unroll
            for (int c = 0; c < nv; ++c) lv[c] = out[2 + n + m + c];
        }
        return;
    }
    using D = Dual<DC>;
    constexpr int g0 = Q * DC, gT = n + m, gV = n + m + (P::LAG_T ? 1 : 0);
    D X[n > 0 ? n : 1], U[m > 0 ? m : 1], V[nv > 0 ? nv : 1], Tt;
#pragma unroll
    for (int c = 0; c < n; ++c) {
        X[c].v = x[c];
#pragma unroll
        for (int d = 0; d < DC; ++d) X[c].d[d] = (g0 + d == c) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int c = 0; c < m; ++c) {
        U[c].v = u[c];
#pragma unroll
        for (int d = 0; d < DC; ++d) U[c].d[d] = (g0 + d == n + c) ? 1.0 : 0.0;
    }
    Tt.v = t;
#pragma unroll
    for (int d = 0; d < DC; ++d) Tt.d[d] = (P::LAG_T && g0 + d == gT) ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < nv; ++c) {
        V[c].v = v[c];
#pragma unroll
        for (int d = 0; d < DC; ++d) V[c].d[d] = (P::LAG_V && g0 + d == gV + c) ? 1.0 : 0.0;
    }
    const D r = P::template lagrange<D>(Tt, X, U, V);
#pragma unroll
    for (int d = 0; d < DC; ++d) {
        constexpr int dummy = 0; (void)dummy;
        const int g = g0 + d;
        if (g < n) lx[g] = r.d[d];
        else if (g < n + m) lu[g - n] = r.d[d];
        else if (P::LAG_T && g == gT) lt = r.d[d];
        else if (P::LAG_V && g < LagDirs<P>::N) lv[g - gV] = r.d[d];
    }
    if (Q == 0) val = r.v;
    if constexpr (Q + 1 < LagDirs<P>::NCH) lagrange_partials<P, Q + 1>(t, x, u, v, val, lx, lu, lt, lv);
}

template <class P, int Q>
__device__ __forceinline__ void mayer_partials(const double* x0, const double* xf, const double* v, double* g0x, double* gfx, double* gv) {
    constexpr int n = P::NX, nv = P::NV, DC = P::DC;
    using D = Dual<DC>;
    constexpr int g0 = Q * DC;
    D X0[n > 0 ? n : 1], XF[n > 0 ? n : 1], V[nv > 0 ? nv : 1];
#pragma unroll
    for (int c = 0; c < n; ++c) {
        X0[c].v = x0[c]; XF[c].v = xf[c];
#pragma unroll
        for (int d = 0; d < DC; ++d) { X0[c].d[d] = (g0 + d == c) ? 1.0 : 0.0; XF[c].d[d] = (g0 + d == n + c) ? 1.0 : 0.0; }
    }
#pragma unroll
    for (int c = 0; c < nv; ++c) {
        V[c].v = v[c];
#pragma unroll
        for (int d = 0; d < DC; ++d) V[c].d[d] = (g0 + d == 2 * n + c) ? 1.0 : 0.0;
    }
    const D r = P::template mayer<D>(X0, XF, V);
#pragma unroll
    for (int d = 0; d < DC; ++d) {
        const int g = g0 + d;
        if (g < n) g0x[g] = r.d[d];
        else if (g < 2 * n) gfx[g - n] = r.d[d];
        else if (g < 2 * n + nv) gv[g - 2 * n] = r.d[d];
    }
    if constexpr (Q + 1 < LagDirs<P>::NCH_MAY) mayer_partials<P, Q + 1>(x0, xf, v, g0x, gfx, gv);
}

template <class P> __device__ __forceinline__ double grad_tau(const GradParams& gp, int64_t i) {
    return gp.tau ? gp.tau[i] : (double)i / (double)gp.L.N;
}
template <class P> __device__ __forceinline__ double grad_time(const GradParams& gp, const double* v, double tau) {
    const double t0 = (P::IT0 >= 0) ? v[P::IT0 >= 0 ? P::IT0 : 0] : gp.L.t0;
    const double tf = (P::ITF >= 0) ? v[P::ITF >= 0 ? P::ITF : 0] : gp.L.tf;
    return t0 + tau * (tf - t0);
}

// body of the gradient pass for workgroup `block` (wsum: 4 * kMaxNV doubles of LDS); also a branch of iter_main_kernel.
// mb: member of a batched launch (xu is already the member's iterate)
template <class P, int SC, int S>
__device__ __forceinline__ void grad_units_body(const GradParams& gp, const double* __restrict__ xu, int block, double (*wsum)[kMaxNV],
                                                int64_t mb = 0) {
    constexpr int n = P::NX, m = P::NU, nv = P::NV;
    constexpr bool FREE = (P::IT0 >= 0) || (P::ITF >= 0);
    const Layout& L = gp.L;
    double v[nv > 0 ? nv : 1], gv[nv > 0 ? nv : 1];
    for (int k = 0; k < nv; ++k) { v[k] = xu[L.v_off + k]; gv[k] = 0.0; }
    const int64_t i = gp.unit_begin + (int64_t)block * blockDim.x + threadIdx.x;      // step, or node for trapeze / midpoint
    if (P::HAS_LAGRANGE && i < gp.unit_end) {
        double* g = gp.g + mb * gp.ldg;
        const double* base = grad_block(gp, xu, i);
        const double* nextb = (SC == SC_MIDPOINT && i < L.N) ? grad_block(gp, xu, i + 1) : base;      // X_{i+1}: the next shard's for a shard's last node
        double x[n > 0 ? n : 1], u[m > 0 ? m : 1], lx[n > 0 ? n : 1], lu[m > 0 ? m : 1], lv[nv > 0 ? nv : 1];
        double lt = 0.0, val = 0.0;
        for (int k = 0; k < nv; ++k) lv[k] = 0.0;
        if (SC == SC_TRAPEZE) {
            // node weight w_i = h_1/2, (t_{i+1}-t_{i-1})/2, h_N/2   (trapeze.jl:78-110)
            const int64_t ia = i == 0 ? 0 : i - 1, ib = i == L.N ? L.N : i + 1;
            const double ta = grad_tau<P>(gp, ia), tb = grad_tau<P>(gp, ib), ti = grad_tau<P>(gp, i);
            const double w = (grad_time<P>(gp, v, tb) - grad_time<P>(gp, v, ta)) / 2.0;
            for (int c = 0; c < n; ++c) x[c] = base[c];
            for (int c = 0; c < m; ++c) u[c] = base[n + c];
            lagrange_partials<P, 0>(grad_time<P>(gp, v, ti), x, u, v, val, lx, lu, lt, lv);
            for (int c = 0; c < n; ++c) g[i * L.blk + c] = w * lx[c];
            for (int c = 0; c < m; ++c) g[i * L.blk + n + c] = w * lu[c];
            for (int k = 0; k < nv; ++k) {
                const double dw = FREE ? (dtime_of<P>(tb, k) - dtime_of<P>(ta, k)) / 2.0 : 0.0;
                gv[k] = dw * val + w * ((P::LAG_V ? lv[k] : 0.0) + ((P::LAG_T && FREE) ? lt * dtime_of<P>(ti, k) : 0.0));
            }
        } else if (SC == SC_MIDPOINT) {
            // node i gathers step i (x_i, u_i, v) and step i-1 (x_i): h * l(0.5(t_i+t_{i+1}), 0.5(x_i+x_{i+1}), u_i, v)   (midpoint.jl:87-97).
            // Euler (euler.jl:112-134) evaluates at (t_i, x_i) [explicit: only the own step reaches x_i] or (t_{i+1}, x_{i+1})
            // [implicit: only the previous step does]; wa / wb are d x_eval / d x_i of the own / previous step's point
            const double wa = L.euler == 0 ? 0.5 : (L.euler == 1 ? 1.0 : 0.0), wb = L.euler == 0 ? 0.5 : (L.euler == 1 ? 0.0 : 1.0);
            double gx[n > 0 ? n : 1];
            for (int c = 0; c < n; ++c) gx[c] = 0.0;
            if (L.cs > 1) {
                // control_steps > 1 (midpoint.jl:99-116): the step's cost is sum_j h_i l(t_ij, x_s, U_i^j, v), h_i = h / cs,
                // t_ij = t_i + (j - 1/2) h_i; node i owns x_i (half of x_s of its own step and of the previous one) and its U_i^j
                const double cs = (double)L.cs;
                for (int side = 0; side < 2; ++side) {           // 0: own step i, 1: previous step i - 1
                    const int64_t st = side == 0 ? i : i - 1;
                    if (st < 0 || st >= L.N) continue;
                    const double* sb = grad_block(gp, xu, st);
                    const double* sn = grad_block(gp, xu, st + 1);
                    const double t0 = grad_tau<P>(gp, st), t1 = grad_tau<P>(gp, st + 1);
                    const double ta = grad_time<P>(gp, v, t0), hi = (grad_time<P>(gp, v, t1) - ta) / cs;
                    for (int c = 0; c < n; ++c) x[c] = 0.5 * (sb[c] + sn[c]);
                    for (int j = 1; j <= L.cs; ++j) {
                        for (int c = 0; c < m; ++c) u[c] = sb[n + (j - 1) * m + c];
                        const double w = (double)j - 0.5;
                        lagrange_partials<P, 0>(ta + w * hi, x, u, v, val, lx, lu, lt, lv);
                        for (int c = 0; c < n; ++c) gx[c] = gx[c] + hi * (0.5 * lx[c]);
                        if (side == 0) {
                            for (int c = 0; c < m; ++c) g[i * L.blk + n + (j - 1) * m + c] = hi * lu[c];
                            for (int k = 0; k < nv; ++k) {
                                const double d0 = FREE ? dtime_of<P>(t0, k) : 0.0, d1 = FREE ? dtime_of<P>(t1, k) : 0.0;
                                const double dhi = (d1 - d0) / cs;
                                gv[k] = gv[k] + dhi * val + hi * ((P::LAG_V ? lv[k] : 0.0) + ((P::LAG_T && FREE) ? lt * (d0 + w * dhi) : 0.0));
                            }
                        }
                    }
                }
            } else {
            if (i < L.N) {
                const double t0 = grad_tau<P>(gp, i), t1 = grad_tau<P>(gp, i + 1);
                const double ta = grad_time<P>(gp, v, t0), tb = grad_time<P>(gp, v, t1), h = tb - ta;
                for (int c = 0; c < n; ++c) x[c] = L.euler == 0 ? 0.5 * (base[c] + nextb[c]) : (L.euler == 1 ? base[c] : nextb[c]);
                for (int c = 0; c < m; ++c) u[c] = base[n + c];
                lagrange_partials<P, 0>(L.euler == 0 ? 0.5 * (ta + tb) : (L.euler == 1 ? ta : tb), x, u, v, val, lx, lu, lt, lv);
                if (wa != 0.0) for (int c = 0; c < n; ++c) gx[c] = h * (wa * lx[c]);
                for (int c = 0; c < m; ++c) g[i * L.blk + n + c] = h * lu[c];
                for (int k = 0; k < nv; ++k) {
                    const double d0 = FREE ? dtime_of<P>(t0, k) : 0.0, d1 = FREE ? dtime_of<P>(t1, k) : 0.0;
                    const double dts = L.euler == 0 ? 0.5 * (d0 + d1) : (L.euler == 1 ? d0 : d1);
                    gv[k] = (d1 - d0) * val + h * ((P::LAG_V ? lv[k] : 0.0) + ((P::LAG_T && FREE) ? lt * dts : 0.0));
                }
            }
            if (i >= 1 && wb != 0.0) {
                const double* pb = grad_block(gp, xu, i - 1);      // (the previous shard's last block for a shard's first node)
                const double ta = grad_time<P>(gp, v, grad_tau<P>(gp, i - 1)), tb = grad_time<P>(gp, v, grad_tau<P>(gp, i));
                const double h = tb - ta;
                for (int c = 0; c < n; ++c) x[c] = L.euler == 0 ? 0.5 * (pb[c] + base[c]) : base[c];
                for (int c = 0; c < m; ++c) u[c] = pb[n + c];
                double val2 = 0.0, lt2 = 0.0, lu2[m > 0 ? m : 1], lv2[nv > 0 ? nv : 1];
                lagrange_partials<P, 0>(L.euler == 0 ? 0.5 * (ta + tb) : tb, x, u, v, val2, lx, lu2, lt2, lv2);
                for (int c = 0; c < n; ++c) gx[c] = gx[c] + h * (wb * lx[c]);
            }
            }
            for (int c = 0; c < n; ++c) g[i * L.blk + c] = gx[c];
        } else {
            // step i: h sum_j b_j l(t_ij, x_ij, u_ij, v)   (irk.jl:179-228, irk_stagewise.jl:344-384)
            const double t0 = grad_tau<P>(gp, i), t1 = grad_tau<P>(gp, i + 1);
            const double ti = grad_time<P>(gp, v, t0), h = grad_time<P>(gp, v, t1) - ti;
            const double* K = base + n + L.cu;
            double gx[n > 0 ? n : 1], gK[S][n > 0 ? n : 1], gu[m > 0 ? m : 1];
            for (int c = 0; c < n; ++c) { gx[c] = 0.0; for (int l = 0; l < S; ++l) gK[l][c] = 0.0; }
            for (int c = 0; c < m; ++c) gu[c] = 0.0;
            double sum_bl = 0.0;
            // not unrolled: with the stages unrolled the compiler keeps every stage's x_ij, sum a K and l_x live at once
            // (364 registers per lane for the 12-state quadrotor at S = 3, one wave per SIMD); j is wave-uniform
#pragma unroll 1
            for (int j = 0; j < S; ++j) {
                double sa[n > 0 ? n : 1];              // sum_l a_jl K^l (for d x_ij / d v)
                for (int c = 0; c < n; ++c) {
                    double xc = base[c], acc = 0.0;
#pragma unroll
                    for (int l = 0; l < S; ++l) { xc = xc + h * L.a[3 * j + l] * K[l * n + c]; acc = acc + L.a[3 * j + l] * K[l * n + c]; }
                    x[c] = xc; sa[c] = acc;
                }
                const double* U = base + n + (L.stagewise ? j * m : 0);
                for (int c = 0; c < m; ++c) u[c] = U[c];
                lagrange_partials<P, 0>(ti + L.c[j] * h, x, u, v, val, lx, lu, lt, lv);
                const double hb = h * L.b[j];
                for (int c = 0; c < n; ++c) {
                    gx[c] = gx[c] + hb * lx[c];
#pragma unroll
                    for (int l = 0; l < S; ++l) gK[l][c] = gK[l][c] + hb * (h * L.a[3 * j + l]) * lx[c];
                }
                if (L.stagewise) { for (int c = 0; c < m; ++c) g[i * L.blk + n + j * m + c] = hb * lu[c]; }
                else { for (int c = 0; c < m; ++c) gu[c] = gu[c] + hb * lu[c]; }
                sum_bl = sum_bl + L.b[j] * val;
                for (int k = 0; k < nv; ++k) {
                    const double d0 = FREE ? dtime_of<P>(t0, k) : 0.0, dh = FREE ? dtime_of<P>(t1, k) - d0 : 0.0;
                    double e = P::LAG_V ? lv[k] : 0.0;
                    if (P::LAG_T && FREE) e = e + lt * (d0 + L.c[j] * dh);
                    if (FREE) for (int c = 0; c < n; ++c) e = e + lx[c] * (dh * sa[c]);
                    gv[k] = gv[k] + hb * e;
                }
            }
            for (int k = 0; k < nv; ++k) {
                const double dh = FREE ? dtime_of<P>(t1, k) - dtime_of<P>(t0, k) : 0.0;
                gv[k] = gv[k] + dh * sum_bl;
            }
            for (int c = 0; c < n; ++c) g[i * L.blk + c] = gx[c];
            if (!L.stagewise) for (int c = 0; c < m; ++c) g[i * L.blk + n + c] = gu[c];
#pragma unroll
            for (int l = 0; l < S; ++l)
                for (int c = 0; c < n; ++c) g[i * L.blk + n + L.cu + l * n + c] = gK[l][c];
        }
    }
    // deterministic reduction of the v-partials: wave shuffles, then one value per workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < nv; ++k) {
        double a = gv[k];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) wsum[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < nv; ++k) {
            double sacc = 0.0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) sacc += wsum[w][k];
            gp.partial[((size_t)mb * gp.nblocks + block) * kMaxNV + k] = sacc;
        }
}
template <class P, int SC, int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) grad_units_kernel(const GradParams gp, const double* __restrict__ xu) {
    __shared__ double wsum[4][kMaxNV];
    const int64_t mb = batch_member();
    grad_units_body<P, SC, S>(gp, xu + mb * gp.ldx, (int)blockIdx.x, wsum, mb);
}

template <class P>
__device__ __forceinline__ void grad_finish_body(const GradParams& gp, const double* __restrict__ xu, int64_t mb = 0) {
    if (threadIdx.x >= 64) return;
    constexpr int n = P::NX, nv = P::NV;
    const Layout& L = gp.L;
    const double* part = gp.partial + (size_t)mb * gp.nblocks * kMaxNV;
    double* const g = gp.g + mb * gp.ldg;
    double gvs[nv > 0 ? nv : 1];
    for (int k = 0; k < nv; ++k) {          // one wave, fixed order (see obj_finish_kernel)
        double sacc = 0.0;
        for (int b = threadIdx.x; b < gp.nblocks; b += 64) sacc += part[(size_t)b * kMaxNV + k];
        for (int off = 32; off > 0; off >>= 1) sacc += __shfl_down(sacc, off, 64);
        gvs[k] = sacc;
    }
    if (threadIdx.x != 0) return;
    if (P::HAS_MAYER && (gp.owns_first || gp.owns_last)) {
        double x0[n > 0 ? n : 1], xf[n > 0 ? n : 1], v[nv > 0 ? nv : 1], g0x[n > 0 ? n : 1], gfx[n > 0 ? n : 1], gmv[nv > 0 ? nv : 1];
        const double* b0 = grad_block(gp, xu, 0);
        const double* bf = grad_block(gp, xu, L.N);
        for (int c = 0; c < n; ++c) { x0[c] = b0[c]; xf[c] = bf[c]; g0x[c] = 0.0; gfx[c] = 0.0; }
        for (int k = 0; k < nv; ++k) { v[k] = xu[L.v_off + k]; gmv[k] = 0.0; }
        mayer_partials<P, 0>(x0, xf, v, g0x, gfx, gmv);
        for (int c = 0; c < n; ++c) {
            if (gp.owns_first) g[c] += g0x[c];
            if (gp.owns_last) g[L.N * (int64_t)L.blk + c] += gfx[c];
        }
        if (gp.owns_last) for (int k = 0; k < nv; ++k) gvs[k] += gmv[k];
    }
    for (int k = 0; k < nv; ++k) g[L.v_off + k] = gvs[k];
}
// (one workgroup per member of a batched launch: grid (1, batch))
template <class P>
__global__ void grad_finish_kernel(const GradParams gp, const double* __restrict__ xu) {
    if (blockIdx.x != 0) return;
    const int64_t mb = batch_member();
    grad_finish_body<P>(gp, xu + mb * gp.ldx, mb);
}

#if !defined(__HIPCC_RTC__)
// batch: members of a batched launch (the grid's second dimension; 1 for one iterate)
template <class P>
hipError_t launch_grad(const GradParams& gp, const double* xu, int grid, hipStream_t st, int batch) {
    const dim3 g(grid > 0 ? grid : 1, batch);
    if (grid > 0)          // (else a Mayer-only cost: nothing to integrate)
        for_scheme<false>(gp.L, [&](auto t) { grad_units_kernel<P, t.sc, t.s><<<g, 256, 0, st>>>(gp, xu); });
    grad_finish_kernel<P><<<dim3(1, batch), 64, 0, st>>>(gp, xu);
    return hipGetLastError();
}

#endif

#if !defined(__HIPCC_RTC__)
// ---- launchers ---------------------------------------------------------------------------------------------------
// Defined here as templates; each per-problem translation unit (ctd_kern_*.hip) explicitly instantiates them for one
// OCP so the registry compiles in parallel, and ctd_engine.hip only sees `extern template` declarations.
// Five kernel variants per OCP: (trapeze), (midpoint), (Gauss-Legendre s = 1, 2, 3); the stage count is a template
// parameter so every loop over stages unrolls.
template <class P, int SC, int S, bool DBG, bool LEAN>
hipError_t launch_variant_dbg(const KParams& kp, const double* xu, int grid, int block, size_t lds_bytes, hipStream_t st,
                              hipEvent_t e0, hipEvent_t e1) {
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)cons_jac_kernel<P, SC, S, DBG, LEAN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    // e0/e1 (optional): events recorded by the dispatch itself right before / after THIS kernel, so
    // hipEventElapsedTime(e0, e1) is the kernel's own duration on the stream it was launched on
    if (e0 || e1) hipExtLaunchKernelGGL((cons_jac_kernel<P, SC, S, DBG, LEAN>), dim3(grid), dim3(block), lds_bytes, st, e0, e1, 0, kp, xu);
    else cons_jac_kernel<P, SC, S, DBG, LEAN><<<grid, block, lds_bytes, st>>>(kp, xu);
    return hipGetLastError();
}
// Two variants of every instantiation: GENERAL (every mode of the handle) and LEAN (ctd_kernel_body.hpp: block_halo) for the
// launches that read the whole iterate from one buffer and emit everything behind the barrier -- every single-GPU evaluation
// unless early emission was asked for.  `lean_ok`: the handle allows the lean variant (env CTD_LEAN=0 at ctd_create forbids it).
// The static-emit variant of the lean kernel for NTHR lanes, when <P, SC, S> has one (StaticEmit::built) and the handle's periods are
// the static ones; `done`: it was launched (else the caller goes on with the lean / general kernel)
template <class P, int SC, int S, int NTHR>
hipError_t launch_static(const KParams& kp, const double* xu, int grid, size_t lds_bytes, hipStream_t st, hipEvent_t e0, hipEvent_t e1,
                         bool dbg, bool& done) {
    done = false;
    if constexpr (StaticEmit<P, SC, S>::template built<NTHR>()) {
        using SE = StaticEmit<P, SC, S>;
        if (kp.Lseg != SE::Lseg || kp.vr != SE::vr || (SC == SC_IRK && S >= 2 && !kp.L.stagewise)) return hipSuccess;
        const TileArgs ta = make_tile_args(kp, xu);       // (the tile workgroups' argument block: first kernel argument)
        if (!ta.valid) return hipSuccess;
        done = true;
        auto go = [&](auto kern) -> hipError_t {
            if (lds_bytes > 64 * 1024) {
                hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
                if (e != hipSuccess) return e;
            }
            if (e0 || e1) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(NTHR), lds_bytes, st, e0, e1, 0, ta, kp);
            else kern<<<grid, NTHR, lds_bytes, st>>>(ta, kp);
            return hipGetLastError();
        };
        if (dbg) return kp.wt_store ? go(cons_jac_static_kernel<P, SC, S, true, NTHR, true>) : go(cons_jac_static_kernel<P, SC, S, true, NTHR, false>);
        return kp.wt_store ? go(cons_jac_static_kernel<P, SC, S, false, NTHR, true>) : go(cons_jac_static_kernel<P, SC, S, false, NTHR, false>);
    }
    return hipSuccess;
}
// lean_ok: bit 0 -- the handle allows the lean variant; bit 1 -- and its static-emit form (ctd_create: manual pattern, CSC order,
// whole grid, periods checked against StaticEmit; env CTD_STATIC_EMIT=0 forbids it)
template <class P, int SC, int S>
hipError_t launch_variant(const KParams& kp, const double* xu, int grid, int block, size_t lds_bytes, hipStream_t st,
                          hipEvent_t e0, hipEvent_t e1, int lean_ok) {
    const bool dbg = kp.stamps || kp.debug_stop;
    if ((lean_ok & 3) == 3 && kp.halo == nullptr && kp.n_early == 0 && (block == 256 || block == 320)) {
        bool done = false;
        const hipError_t e = block == 256 ? launch_static<P, SC, S, 256>(kp, xu, grid, lds_bytes, st, e0, e1, dbg, done)
                                          : launch_static<P, SC, S, 320>(kp, xu, grid, lds_bytes, st, e0, e1, dbg, done);
        if (done) return e;
    }
    lean_ok &= 1;
    // The lean variant exists for the direct tiles and for the staged tiles of the Gauss-Legendre schemes, where it measured faster
    // (profiles/lean_kernel.md).  The staged tiles of the one-point schemes keep the general kernel: the 12-state quadrotor on
    // midpoint, N = 20 000, measured 15.74 us lean against 15.50; trapeze was not measured.
    constexpr bool kHasLean = DirectTile<P, SC>::value || SC == SC_IRK;
    if constexpr (kHasLean) {
        if (lean_ok && kp.halo == nullptr && kp.n_early == 0) {
            if (dbg) return launch_variant_dbg<P, SC, S, true, true>(kp, xu, grid, block, lds_bytes, st, e0, e1);
            return launch_variant_dbg<P, SC, S, false, true>(kp, xu, grid, block, lds_bytes, st, e0, e1);
        }
    }
    if (dbg) return launch_variant_dbg<P, SC, S, true, false>(kp, xu, grid, block, lds_bytes, st, e0, e1);
    return launch_variant_dbg<P, SC, S, false, false>(kp, xu, grid, block, lds_bytes, st, e0, e1);
}

template <class P>
hipError_t launch_cons_jac(const KParams& kp, const double* xu, int grid, int block, size_t lds_bytes, hipStream_t st,
                           hipEvent_t e0, hipEvent_t e1, int lean_ok) {
    hipError_t e = hipErrorInvalidValue;       // (midpoint: the template's stage count is control_steps -- 1 in collocation, up to 3 compiled in)
    for_scheme<true>(kp.L, [&](auto t) { e = launch_variant<P, t.sc, t.s>(kp, xu, grid, block, lds_bytes, st, e0, e1, lean_ok); });
    return e;
}

// resident workgroups per CU of the kernel launch_cons_jac would run (registers and LDS): sizes the multi-tile grid
template <class P, int SC, int S>
int occupancy_variant(int block, size_t lds_bytes) {
    int nb = 0;
    if (lds_bytes > 64 * 1024 &&
        hipFuncSetAttribute((const void*)cons_jac_kernel<P, SC, S, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
        return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, cons_jac_kernel<P, SC, S, false>, block, lds_bytes) != hipSuccess) return 0;
    return nb;
}
// Batched launch (ctd_cons_jac_batch_dev_async): cons_jac_batch_kernel on grid (grid, batch)
template <class P, int SC, int S>
hipError_t launch_variant_batch(const KParams& kp, const double* xu, const BatchLd& bl, int grid, int block, size_t lds_bytes, hipStream_t st,
                                int batch) {
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)cons_jac_batch_kernel<P, SC, S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    cons_jac_batch_kernel<P, SC, S><<<dim3(grid, batch), block, lds_bytes, st>>>(kp, xu, bl);
    return hipGetLastError();
}
template <class P>
hipError_t launch_cons_jac_batch(const KParams& kp, const double* xu, const BatchLd& bl, int grid, int block, size_t lds_bytes,
                                 hipStream_t st, int batch) {
    hipError_t e = hipErrorInvalidValue;
    for_scheme<true>(kp.L, [&](auto t) { e = launch_variant_batch<P, t.sc, t.s>(kp, xu, bl, grid, block, lds_bytes, st, batch); });
    return e;
}

// (0 for the midpoint scheme with more than 3 controls per step, which the launchers refuse: ctd_create refuses such a handle for a
// registry problem on a device, and the caller asks for Gauss-Legendre or control_steps = 1 only)
template <class P>
int occupancy_cons_jac(const KParams& kp, int block, size_t lds_bytes) {
    int nb = 0;
    for_scheme<true>(kp.L, [&](auto t) { nb = occupancy_variant<P, t.sc, t.s>(block, lds_bytes); });
    return nb;
}

template <class P>
hipError_t launch_obj(const ObjParams& op, const double* xu, int grid, int block, hipStream_t st, int batch) {
    const dim3 g(grid > 0 ? grid : 1, batch);
    if (grid > 0)          // (else a Mayer-only cost: nothing to integrate; the quadrature kernel has no stage count)
        for_scheme<false>(op.L, [&](auto t) { obj_partial_kernel<P, t.sc><<<g, block, 0, st>>>(op, xu); });
    obj_finish_kernel<P><<<dim3(1, batch), 64, 0, st>>>(op, xu);
    return hipGetLastError();
}

#define CTD_INSTANTIATE_LAUNCHERS(P)                                                                                       \
    template hipError_t launch_cons_jac<P>(const KParams&, const double*, int, int, size_t, hipStream_t, hipEvent_t, \
                                           hipEvent_t, int);                                                                 \
    template hipError_t launch_cons_jac_batch<P>(const KParams&, const double*, const BatchLd&, int, int, size_t, hipStream_t, int); \
    template hipError_t launch_obj<P>(const ObjParams&, const double*, int, int, hipStream_t, int);                  \
    template int occupancy_cons_jac<P>(const KParams&, int, size_t);                                                 \
    template hipError_t launch_grad<P>(const GradParams&, const double*, int, hipStream_t, int);
#define CTD_EXTERN_LAUNCHERS(P)                                                                                            \
    extern template hipError_t launch_cons_jac<P>(const KParams&, const double*, int, int, size_t, hipStream_t,      \
                                                  hipEvent_t, hipEvent_t, int);                                              \
    extern template hipError_t launch_cons_jac_batch<P>(const KParams&, const double*, const BatchLd&, int, int, size_t, hipStream_t, \
                                                        int);                                                                      \
    extern template hipError_t launch_obj<P>(const ObjParams&, const double*, int, int, hipStream_t, int);          \
    extern template int occupancy_cons_jac<P>(const KParams&, int, size_t);                                         \
    extern template hipError_t launch_grad<P>(const GradParams&, const double*, int, hipStream_t, int);

#endif  // !__HIPCC_RTC__

}  // namespace ctd
