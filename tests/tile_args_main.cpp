// TEST INFRASTRUCTURE ONLY -- stand-alone check of make_tile_args (csrc/ctd_layout.hpp) against the KParams of the launch plan
// (tests/test_tile_args_cpu.py builds this with g++ -fsanitize=address,undefined and runs it; host sources only, no GPU).
//
// For every case a host-only model and its plan are built as ctd_create builds them, the device pointers a handle would fill in
// are set to made-up addresses (nothing dereferences them), and every field of TileArgs must be the field of KParams it stands
// for.  `valid` must be 1 exactly for what a static tile can run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../ctdirect.jl_amd/csrc/ctd_host.cpp"
#include "../ctdirect.jl_amd/csrc/ctd_jit.cpp"
#define ST_OK ST_OK_HESS
#define ST_EPATTERN ST_EPATTERN_HESS
#include "../ctdirect.jl_amd/csrc/ctd_hess_host.cpp"          // (the model builder's dependency masks live there)
#undef ST_OK
#undef ST_EPATTERN

using namespace ctd;

static int g_bad = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_bad; } \
    } while (0)

template <class T> static T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }

static void one_case(int problem, int scheme, int64_t N, bool user_grid) {
    std::vector<double> tg;
    if (user_grid) {
        tg.resize(N + 1);
        double acc = 0.0;
        for (int64_t i = 0; i <= N; ++i) { tg[i] = acc; acc += 1.0 + 0.5 * std::sin((double)i); }
        for (int64_t i = 0; i <= N; ++i) tg[i] /= tg[N];
    }
    HostDesc d{problem, scheme, 0, N, user_grid ? tg.data() : nullptr, user_grid ? N + 1 : 0};
    Model mo;
    std::string err;
    if (build_model(d, mo, err)) { std::printf("FAIL build_model(%d, %d, %lld): %s\n", problem, scheme, (long long)N, err.c_str()); ++g_bad; return; }
    LaunchPlan plan;
    PlanKnobs knobs;
    knobs.tile = 21;
    if (plan_cons_jac(mo, 0, mo.L.N, knobs, Resident{}, 256, false, plan, err)) { std::printf("FAIL plan_cons_jac: %s\n", err.c_str()); ++g_bad; return; }
    KParams kp = plan.kp;
    const double* xu = fake<const double>(0x10000008);
    // a host-only plan has no device table: without one the static form must be refused
    CHECK(kp.tau == nullptr, "host-only plan with a device pointer");
    CHECK(make_tile_args(kp, xu).valid == 0, "no time-grid table, but valid");
    kp.tau = fake<const double>(0x20000000); kp.tmpl = fake<const uint32_t>(0x30000000); kp.vtmpl = fake<const uint32_t>(0x40000004);
    kp.c = fake<double>(0x50000008); kp.vals = fake<double>(0x60000010);
    const TileArgs ta = make_tile_args(kp, xu);
    const long long tag[3] = {problem, scheme, (long long)N};
#define SAME(field, want) CHECK(ta.field == (want), "%s (problem %lld scheme %lld N %lld)", #field, tag[0], tag[1], tag[2])
    SAME(xu, xu); SAME(tau, kp.tau); SAME(tmpl, kp.tmpl); SAME(vtmpl, kp.vtmpl); SAME(c, kp.c); SAME(vals, kp.vals);
    SAME(has_edge, kp.has_edge); SAME(T, kp.T); SAME(step_begin, kp.step_begin); SAME(step_end, kp.step_end);
    SAME(N, kp.L.N); SAME(v_off, kp.L.v_off); SAME(stagewise, kp.L.stagewise); SAME(t0, kp.L.t0); SAME(tf, kp.L.tf);
    SAME(seg_base, kp.seg_base); SAME(reg_first, kp.reg_first); SAME(reg_last, kp.reg_last);
    for (int k = 0; k < kMaxNV; ++k) SAME(vcol_base[k], kp.vcol_base[k]);
    SAME(valid, 1);
    CHECK(kp.L.N == N && kp.step_begin == 0 && kp.step_end == N && kp.T == 21, "the plan is not the one asked for");
    CHECK(kp.HL == 0 && kp.HH == 0 && kp.L.euler == 0 && kp.L.sc == SC_IRK, "a Gauss-Legendre tile with a halo record or an Euler flag");
    CHECK(reinterpret_cast<uintptr_t>(&ta) % 64 == 0, "a TileArgs object off its alignment");
    // what a static tile cannot run: each of these alone clears `valid` (and only `valid`)
    for (int what = 0; what < 6; ++what) {
        KParams k2 = kp;
        XHalo halo{};
        if (what == 0) k2.HL = 1;
        if (what == 1) k2.HH = 1;
        if (what == 2) k2.L.euler = 1;
        if (what == 3) k2.L.sc = SC_MIDPOINT;
        if (what == 4) k2.halo = &halo;
        if (what == 5) k2.n_early = 3;
        const TileArgs t2 = make_tile_args(k2, xu);
        CHECK(t2.valid == 0, "refusal %d", what);
        CHECK(t2.tau == kp.tau && t2.reg_last == kp.reg_last && t2.T == kp.T, "refusal %d changed other fields", what);
    }
#undef SAME
}

int main() {
    static_assert(sizeof(TileArgs) <= 192, "TileArgs is larger than three cache lines");
    static_assert(alignof(TileArgs) == 64, "TileArgs is not aligned to a cache line");
    static_assert(sizeof(TileArgs) % 64 == 0, "TileArgs does not end on a line");
    CHECK(sizeof(KParams) == 768, "KParams changed its size: %zu", sizeof(KParams));      // (it keeps every field and offset)
    int cases = 0;
    const int goddard = 0, free_t0_tf = 9, gl1 = 2, gl2 = 5, gl3 = 6;      // ids of include/ctdirect_hip.h
    for (int scheme : {gl1, gl2, gl3})
        for (int ug = 0; ug < 2; ++ug)
            for (int64_t N : {2, 7, 22, 43, 100}) { one_case(goddard, scheme, N, ug != 0); ++cases; }
    for (int ug = 0; ug < 2; ++ug)
        for (int64_t N : {7, 43}) { one_case(free_t0_tf, gl2, N, ug != 0); ++cases; }
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("ok: %d cases, sizeof(TileArgs) = %zu\n", cases, sizeof(TileArgs));
    return 0;
}
