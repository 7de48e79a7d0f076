// TEST INFRASTRUCTURE ONLY -- serial CPU stepping of the tile's emit phase in its two forms (tests/test_static_emit_emu.py).
//
// The same phase templates the HIP kernels wrap, compiled with g++ as tests/emu/ is: every workgroup evaluates its records once,
// then the GENERIC emit (phase_emit, ctd_kernel_body.hpp) streams them into (c, vals) and the STATIC emit (phase_emit_static,
// ctd_emit_static.hpp; the edge block: the generic one, as in cons_jac_static_kernel) into (c2, vals2).  The "LDS" is on the
// heap, exact size, NaN-filled.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../ctdirect.jl_amd/csrc/ctd_host.cpp"
#include "../ctdirect.jl_amd/csrc/ctd_jit.cpp"
#include "../ctdirect.jl_amd/csrc/ctd_kernel_body.hpp"
#define ST_OK ST_OK_HESS
#define ST_EPATTERN ST_EPATTERN_HESS
#include "../ctdirect.jl_amd/csrc/ctd_hess_host.cpp"          // (the model builder's dependency masks live there)
#undef ST_OK
#undef ST_EPATTERN

using namespace ctd;

static std::string g_err;

// 1: both forms ran; 0: <P, SC, S> has no static emit for NTHR lanes (or the handle's periods are not the static ones)
template <class P, int SC, int S, int NTHR>
static int run_both(const KParams& kp, const double* xu, double* c2, double* vals2) {
    using SE = StaticEmit<P, SC, S>;
    if constexpr (!SE::template fits<NTHR>()) return 0;
    else {
        if (kp.Lseg != SE::Lseg || kp.vr != SE::vr || (SC == SC_IRK && S >= 2 && !kp.L.stagewise)) return 0;
        const int nblocks = kp.ntiles + kp.has_edge;
        const int64_t nlds = lds_doubles(kp);
        KParams k2 = kp;
        k2.c = c2; k2.vals = vals2;
        for (int b = 0; b < nblocks; ++b) {
            std::vector<double> lds(nlds, std::numeric_limits<double>::quiet_NaN());
            BlockCtx cx = make_direct_ctx<true>(kp, b, lds.data(), xu, LV<P, SC, S, true>::blk(kp), P::NV);
            std::vector<EmitPre> pre(NTHR), pre2(NTHR);
            for (int t = 0; t < NTHR; ++t) pre[t] = emit_prefetch<P, 1, true>(kp, cx, t, NTHR);
            for (int t = 0; t < NTHR; ++t) phase_eval<P, SC, S, RegEval<P, SC, S>::value, 1, false, true>(kp, cx, t, NTHR, &pre[t]);
            for (int t = 0; t < NTHR; ++t) phase_emit<P, SC, S, 1, false, true>(kp, cx, t, NTHR, &pre[t]);
            if (cx.is_edge) {
                for (int t = 0; t < NTHR; ++t) phase_emit<P, SC, S, 1, false, true>(k2, cx, t, NTHR, &pre[t]);
                continue;
            }
            for (int t = 0; t < NTHR; ++t) pre2[t] = emit_prefetch_static<P, SC, S, NTHR>(k2, t);
            for (int t = 0; t < NTHR; ++t) phase_emit_static<P, SC, S, NTHR, false>(k2, cx, t, pre2[t]);
        }
        return 1;
    }
}

extern "C" {

const char* se_last_error() { return g_err.c_str(); }

// info[0..7] = ran, Lseg, vr, static Lseg, static vr, steps per tile, nnzj, ncon; the mismatch check's answer in g_err when it refuses
int se_cons_jac(int problem, int scheme, int64_t N, const double* tg, int64_t tglen, int control_steps, int tile, int nthr, const double* x,
                double* c, double* vals, double* c2, double* vals2, int64_t* info) {
    Model mo;
    HostDesc d{problem, scheme, 0, N, tg, tglen, control_steps < 1 ? 1 : control_steps, 0};
    int st = build_model(d, mo, g_err);
    if (st) return st;
    if (tile <= 0) {      // the tile of the engine's host-only launch plan
        LaunchPlan pl;
        std::string err;
        (void)plan_cons_jac(mo, 0, mo.L.N, plan_knobs_from_env(), Resident{}, 256, false, pl, err);
        tile = pl.tile;
    }
    KParams kp;
    mo.fill_kparams(kp, 0, mo.L.N, tile);
    kp.tau = mo.uniform ? nullptr : mo.tau.data();
    kp.tmpl = mo.tmpl.data();
    kp.vtmpl = mo.vtmpl.data();
    kp.edge_idx = mo.edge_idx.data();
    kp.edge_code = mo.edge_code.data();
    kp.c = c;
    kp.vals = vals;
    info[0] = 0; info[1] = mo.Lseg; info[2] = mo.vr; info[3] = info[4] = -1; info[5] = tile; info[6] = mo.nnzj; info[7] = mo.L.ncon;
    const char* bad = nullptr;
    bool ok = for_problem(problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        for_scheme<true>(mo.L, [&](auto t) {
            using SE = StaticEmit<P, t.sc, t.s>;
            info[3] = SE::Lseg; info[4] = SE::vr;
            bad = static_emit_mismatch<P, t.sc, t.s>(mo.L, mo.Lseg, mo.vr);
            if constexpr (DirectTile<P, t.sc>::value) {
                if (x) info[0] = nthr == 320 ? run_both<P, t.sc, t.s, 320>(kp, x, c2, vals2) : (nthr == 256 ? run_both<P, t.sc, t.s, 256>(kp, x, c2, vals2) : 0);
            }
        });
    });
    if (bad) { g_err = std::string("static emit mismatch: ") + bad; return 97; }
    return ok ? 0 : 5;
}

// the refusal itself: the check ctd_create runs, on periods that are NOT the model's; 1: refused (name of the field in se_last_error)
int se_mismatch(int problem, int scheme, int64_t N, int dLseg, int dvr) {
    Model mo;
    HostDesc d{problem, scheme, 0, N, nullptr, 0, 1, 0};
    if (build_model(d, mo, g_err)) return -1;
    const char* bad = nullptr;
    for_problem(problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        for_scheme<true>(mo.L, [&](auto t) { bad = static_emit_mismatch<P, t.sc, t.s>(mo.L, mo.Lseg + dLseg, mo.vr + dvr); });
    });
    g_err = bad ? bad : "";
    return bad ? 1 : 0;
}

}  // extern "C"
