// ctd_emit_static.hpp -- the emit phase of a tile with a STATIC geometry (included at the end of ctd_kernel_body.hpp).
//
// phase_emit_impl is generic: the periods of the three output streams (cb rows of c, Lseg CSC entries, vr entries of a V column),
// the workgroup size and the store flavour are run-time values, so every pass divides by a kernel argument (fast_div), both arms
// of every `par >= 1` choice and both store flavours are compiled, and every store sits behind an exec-mask branch.  For the
// MANUAL pattern in CSC order the periods follow from (OCP, scheme class, stages) alone -- the add_nonzero_block! calls of the
// reference (step_blocks, ctd_host.cpp) -- and ctd_create picks the workgroup size from a short list.  StaticEmit states the
// periods as constants, phase_emit_static<P, SC, S, NTHR, WT> is the tile's emit phase for them:
//   - lane -> (replica g, position k) of each stream is a division by a constant; lane -> address inside a pass is the identity
//   - ALL LDS reads of the lane's first chunk of every stream are issued before the first store (one LDS round trip)
//   - the stores of a chunk are `kf` unpredicated stores (kf: full passes, workgroup-uniform, selected once) plus one predicated
//     store for the pass that only the first `rem` replicas take part in
// The values and their places are those of phase_emit_impl (tests/test_static_emit_emu.py steps both over the same records).
#pragma once

namespace ctd {

// Periods of the output streams of a step of the Gauss-Legendre schemes, manual pattern, CSC order (irk.jl:330-380 /
// irk_stagewise.jl:483-524).  Columns of step i's block of variables: x_i: state + stage + path rows of step i, state rows of step
// i - 1; controls: stage + path rows; K_i: state + stage rows.  A V column holds every row of the step (cb).  Several stages: the
// control block of the STAGEWISE schemes (one control per stage) -- the constant-control variants keep the generic emit.
// The one-point schemes have no static form: the direct midpoint tiles measured no faster with it (profiles/static_emit.md).
template <class P, int SC, int S> struct StaticEmit {
    using SL = StaticLayout<P, SC, S>;
    static constexpr int n = SL::n, m = SL::m, nv = SL::nv, p = SL::p, s = SL::s, cb = SL::cb;
    static constexpr bool stagewise = SC == SC_IRK && S >= 2;
    static constexpr int cu = SL::cu(stagewise);
    static constexpr int Lseg = SC == SC_IRK ? n * (2 * n + s * n + p) + cu * (s * n + p) + s * n * (n + s * n) : 0;
    static constexpr int vr = nv > 0 ? cb : 0;
    // the direct tiles of the Gauss-Legendre schemes (the staged tiles keep the generic emit)
    static constexpr bool offered = DirectTile<P, SC>::value && SC == SC_IRK && Lseg > 0;
    // every period fits a workgroup of NTHR lanes: a lane owns one position of each stream
    template <int NTHR> static constexpr bool fits() { return offered && Lseg <= NTHR && cb <= NTHR; }
    // ctd_create's rule for a fifth wave (ctd_engine.hip): one more replica of the CSC period, at least 90 % of the lanes busy
    static constexpr bool wants320 = Lseg > 0 && 320 / (Lseg > 0 ? Lseg : 1) > 256 / (Lseg > 0 ? Lseg : 1) &&
                                     Lseg * (320 / (Lseg > 0 ? Lseg : 1)) * 10 >= 320 * 9;
    template <int NTHR> static constexpr bool built() { return fits<NTHR>() && P::MAXB >= NTHR && (NTHR == 256 || (NTHR == 320 && wants320)); }
};
// name of the first emit period of a manual / CSC model that differs from the static one, or null (host: ctd_create)
template <class P, int SC, int S> inline const char* static_emit_mismatch(const Layout& L, int Lseg, int vr) {
    using SE = StaticEmit<P, SC, S>;
    if (SC != SC_IRK) return nullptr;
    if (Lseg <= 0) return nullptr;                                             // (grids too short for a periodic range: all-edge mode)
    if (SC == SC_IRK && S >= 2 && !L.stagewise) return nullptr;               // (constant control: not described)
    if (Lseg != SE::Lseg) return "Lseg";
    if (vr != SE::vr) return "vr";
    return nullptr;
}

// codes of the lane's positions: position tid % period of the CSC segment and of every V column
template <class P, int SC, int S, int NTHR>
CTD_HD EmitPre emit_prefetch_static(const KParams& kp, int tid) {
    using SE = StaticEmit<P, SC, S>;
    EmitPre pre;
    pre.b = 0u; pre.eidx = 0; pre.have = 1; pre.kpos = 0; pre.eb = 0u; pre.ek = 0; pre.more[0] = 0u;
    pre.b = kp.tmpl[(uint32_t)tid % (uint32_t)SE::Lseg];
#pragma unroll
    for (int kk = 0; kk < kMaxNV; ++kk) {
        pre.v[kk] = 0u;
        if constexpr (SE::vr > 0) { if (kk < P::NV) pre.v[kk] = kp.vtmpl[kk * SE::vr + (int)((uint32_t)tid % (uint32_t)SE::vr)]; }
    }
    return pre;
}

// ---- one stream, one chunk of CH passes -------------------------------------------------------------------------------------
// PAR replicas of the period walk the steps: pass `it` has replica g at step g + it * PAR.  Reads: the lane's record fields of
// passes c0 .. c0 + CH - 1, the step clamped to the stream's last one (`jmax` = last - g, so no read leaves the tile's records).
template <int CH, int PAR, int STRIDE>
CTD_HD void se_load(const double* p, int c0, int jmax, double* v) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        int j = (c0 + u) * PAR;
        j = j < jmax ? j : jmax;
        v[u] = p[j * STRIDE];
    }
}
// Stores of a chunk: `out` points at the lane's entry of pass c0, passes are PITCH doubles apart.  kf: full passes left from c0 on
// (workgroup-uniform); tail: this lane also stores in the pass behind the full ones.
template <int K, int CH, int PITCH, bool WT>
CTD_HD void se_store_case(double* out, const double* v, int kf, bool tail) {
    if (kf == K) {
#pragma unroll
        for (int u = 0; u < K; ++u) emit_store(out + (int64_t)u * PITCH, v[u], WT);
        if (tail) emit_store(out + (int64_t)K * PITCH, v[K], WT);
        return;
    }
    if constexpr (K > 0) se_store_case<K - 1, CH, PITCH, WT>(out, v, kf, tail);
}
template <int CH, int PITCH, bool WT>
CTD_HD void se_store(double* out, const double* v, int kf, bool tail) {
    if (kf >= CH) {
#pragma unroll
        for (int u = 0; u < CH; ++u) emit_store(out + (int64_t)u * PITCH, v[u], WT);
        return;
    }
    se_store_case<CH - 1, CH, PITCH, WT>(out, v, kf, tail);
}

// The emit phase of a TILE (never the edge block).  `pre`: emit_prefetch_static of the same lane.
template <class P, int SC, int S, int NTHR, bool WT>
CTD_HD void phase_emit_static(const KParams& kp, const BlockCtx& cx, int tid, const EmitPre& pre) {
    using SE = StaticEmit<P, SC, S>;
    static_assert(SE::template fits<NTHR>(), "a period of this instantiation exceeds the workgroup");
    constexpr RecLayout R = RL<P, SC, S>::R;
    constexpr int stride = R.stride;
    constexpr int cb = SE::cb, Ls = SE::Lseg, vr = SE::vr, NV = P::NV;
    constexpr int parA = NTHR / cb, parB = NTHR / Ls, parC = vr > 0 ? NTHR / vr : 1;
    constexpr int CHA = 2, CHB = 8, CHC = 2;          // passes per chunk: registers 2 CHB + CHA + 2 NV CHC doubles
    static_assert(2 * CHB + CHA + 2 * kMaxNV * CHC <= 48, "the first chunk of every stream is held in registers at once");
    const int nsteps = (int)(cx.b - cx.a), slot0 = (int)(cx.a - cx.lo);
    // regular steps of the tile (the first and last steps of the grid belong to the edge block): clamps taken once
    const int64_t ra = cx.a > kp.reg_first ? cx.a : kp.reg_first, rb = cx.b < kp.reg_last ? cx.b : kp.reg_last;
    const int nreg = (int)(rb - ra), sl0 = (int)(ra - cx.lo);
    const bool doA = kp.c != nullptr && nsteps > 0, doB = kp.vals != nullptr && nreg > 0, doC = kp.vals != nullptr && vr > 0 && nsteps > 0;
    // lane -> (replica, position)
    const int gA = (int)((uint32_t)tid / (uint32_t)cb), rA = tid - gA * cb;
    const int gB = (int)((uint32_t)tid / (uint32_t)Ls);
    const int gC = vr > 0 ? (int)((uint32_t)tid / (uint32_t)(vr > 0 ? vr : 1)) : 0;
    const bool actA = tid < parA * cb, actB = tid < parB * Ls, actC = vr > 0 && tid < parC * vr;
    const int nfA = nsteps / parA, remA = nsteps - nfA * parA;
    const int nfB = nreg > 0 ? nreg / parB : 0, remB = nreg > 0 ? nreg - nfB * parB : 0;
    const int nfC = nsteps / parC, remC = nsteps - nfC * parC;
    // sources
    const double* srcA = cx.rec + (slot0 + gA) * stride + R.oR + rA;
    const uint32_t code = pre.b;
    const int bt = code_beta(code);
    const double beta = bt == 0 ? 0.0 : (bt == 1 ? 1.0 : -1.0);
    const double* pcB = cx.rec + (sl0 + gB - code_crec(code)) * stride + R.oC + code_ci(code);
    const double* pdB = cx.rec + (sl0 + gB - code_drec(code)) * stride + code_di(code);
    const double* pcC[NV > 0 ? NV : 1];
    const double* pdC[NV > 0 ? NV : 1];
#pragma unroll
    for (int kk = 0; kk < NV; ++kk) {
        pcC[kk] = cx.rec + (slot0 + gC) * stride + R.oC + code_ci(pre.v[kk]);
        pdC[kk] = cx.rec + (slot0 + gC) * stride + code_di(pre.v[kk]);
    }
    // destinations: the lane's entry of pass 0 (lane -> address is the identity inside a pass)
    double* outA = doA ? kp.c + cx.a * (int64_t)cb + tid : nullptr;
    double* outB = doB ? kp.vals + kp.seg_base + (ra - kp.reg_first) * (int64_t)Ls + tid : nullptr;
    double* outC[NV > 0 ? NV : 1];
#pragma unroll
    for (int kk = 0; kk < NV; ++kk) outC[kk] = doC ? kp.vals + kp.vcol_base[kk] + cx.a * (int64_t)vr + tid : nullptr;

    // ---- first chunk of every stream: all reads, then all stores
    double vA[CHA], aB[CHB], bB[CHB], aC[NV > 0 ? NV : 1][CHC], bC[NV > 0 ? NV : 1][CHC];
    if (doA) se_load<CHA, parA, stride>(srcA, 0, nsteps - 1 - gA, vA);
    if (doB) {
        se_load<CHB, parB, stride>(pcB, 0, nreg - 1 - gB, aB);
        se_load<CHB, parB, stride>(pdB, 0, nreg - 1 - gB, bB);
    }
    if (doC) {
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
            se_load<CHC, parC, stride>(pcC[kk], 0, nsteps - 1 - gC, aC[kk]);
            se_load<CHC, parC, stride>(pdC[kk], 0, nsteps - 1 - gC, bC[kk]);
        }
    }
    if (doA && actA) se_store<CHA, parA * cb, WT>(outA, vA, nfA, gA < remA);
    if (doB) {
#pragma unroll
        for (int u = 0; u < CHB; ++u) aB[u] = aB[u] * bB[u] + beta;
        if (actB) se_store<CHB, parB * Ls, WT>(outB, aB, nfB, gB < remB);
    }
    if (doC) {
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
#pragma unroll
            for (int u = 0; u < CHC; ++u) aC[kk][u] = aC[kk][u] * bC[kk][u];
            if (actC) se_store<CHC, parC * (vr > 0 ? vr : 1), WT>(outC[kk], aC[kk], nfC, gC < remC);
        }
    }
    // ---- long tiles: the remaining chunks, stream by stream
    if (doA)
        for (int c0 = CHA; c0 * parA < nsteps; c0 += CHA) {
            se_load<CHA, parA, stride>(srcA, c0, nsteps - 1 - gA, vA);
            if (actA) se_store<CHA, parA * cb, WT>(outA + (int64_t)c0 * (parA * cb), vA, nfA - c0, gA < remA);
        }
    if (doB)
        for (int c0 = CHB; c0 * parB < nreg; c0 += CHB) {
            se_load<CHB, parB, stride>(pcB, c0, nreg - 1 - gB, aB);
            se_load<CHB, parB, stride>(pdB, c0, nreg - 1 - gB, bB);
#pragma unroll
            for (int u = 0; u < CHB; ++u) aB[u] = aB[u] * bB[u] + beta;
            if (actB) se_store<CHB, parB * Ls, WT>(outB + (int64_t)c0 * (parB * Ls), aB, nfB - c0, gB < remB);
        }
    if (doC) {
#pragma unroll
        for (int kk = 0; kk < NV; ++kk)
            for (int c0 = CHC; c0 * parC < nsteps; c0 += CHC) {
                se_load<CHC, parC, stride>(pcC[kk], c0, nsteps - 1 - gC, aC[kk]);
                se_load<CHC, parC, stride>(pdC[kk], c0, nsteps - 1 - gC, bC[kk]);
#pragma unroll
                for (int u = 0; u < CHC; ++u) aC[kk][u] = aC[kk][u] * bC[kk][u];
                if (actC) se_store<CHC, parC * (vr > 0 ? vr : 1), WT>(outC[kk] + (int64_t)c0 * (parC * (vr > 0 ? vr : 1)), aC[kk], nfC - c0, gC < remC);
            }
    }
}

}  // namespace ctd
