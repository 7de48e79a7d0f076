// TEST INFRASTRUCTURE ONLY -- stand-alone check of the level helper of the log-depth exact Schur preconditioner (schur_cr_level,
// schur_cr_levels and the launch counts of csrc/ctd_schur_plan.hpp).  tests/test_kkt_schur_cr_cpu.py builds this with g++
// -fsanitize=address,undefined and runs it; the header is pure C++, no GPU.
//
// For every grid size: every block except 0 is eliminated exactly once; its neighbours are active at its level (multiples of 2^l
// that no earlier level eliminated); the last block of a level has no right neighbour exactly when i + 2^l >= N, and every other
// block of the level has one; after the last level block 0 alone is left.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ctdirect.jl_amd/csrc/ctd_schur_plan.hpp"

using namespace ctd;

static int g_bad = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++g_bad; } \
    } while (0)

static void one_grid(int64_t N) {
    const long long n = (long long)N;
    const int levels = schur_cr_levels(N);
    int want = 0;
    while (((int64_t)1 << want) < N) ++want;
    CHECK(levels == want, "N %lld: %d levels", n, levels);
    CHECK(N <= ((int64_t)1 << levels) && (levels == 0 || N > ((int64_t)1 << (levels - 1))), "N %lld: not ceil(log2 N)", n);
    CHECK(schur_cr_factor_launches(N) == 2 * levels + 2 && schur_cr_solve_launches(N) == 2 * levels + 1, "N %lld: launch counts", n);
    std::vector<int> level_of((size_t)N, -1);          // the level that eliminated a block
    for (int l = 0; l < levels; ++l) {
        const SchurCrLevel lv = schur_cr_level(N, l);
        const int64_t h = (int64_t)1 << l;
        CHECK(lv.first == h && lv.stride == 2 * h, "N %lld level %d: first %lld stride %lld", n, l, (long long)lv.first, (long long)lv.stride);
        CHECK(lv.count >= 1, "N %lld level %d: nothing to eliminate", n, l);
        for (int64_t q = 0; q < lv.count; ++q) {
            const int64_t i = lv.first + q * lv.stride;
            CHECK(i > 0 && i < N, "N %lld level %d: block %lld out of range", n, l, (long long)i);
            if (i <= 0 || i >= N) continue;
            CHECK(level_of[(size_t)i] < 0, "N %lld: block %lld eliminated twice", n, (long long)i);
            level_of[(size_t)i] = l;
            const int64_t lf = i - h, rt = i + h;
            CHECK(lf >= 0 && lf % h == 0 && level_of[(size_t)lf] < 0, "N %lld level %d: left neighbour of %lld not active", n, l, (long long)i);
            const bool has_right = rt < N;
            if (has_right) CHECK(rt % h == 0 && level_of[(size_t)rt] < 0, "N %lld level %d: right neighbour of %lld not active", n, l, (long long)i);
            if (q + 1 < lv.count) CHECK(has_right, "N %lld level %d: block %lld inside the level without a right neighbour", n, l, (long long)i);
            else CHECK((lv.last_has_right != 0) == has_right, "N %lld level %d: last_has_right %d", n, l, lv.last_has_right);
        }
        // the count covers every odd multiple of h below N
        CHECK(lv.first + lv.count * lv.stride >= N, "N %lld level %d: block %lld is missed", n, l, (long long)(lv.first + lv.count * lv.stride));
    }
    CHECK(level_of[0] < 0, "N %lld: block 0 eliminated", n);
    for (int64_t i = 1; i < N; ++i) CHECK(level_of[(size_t)i] >= 0, "N %lld: block %lld never eliminated", n, (long long)i);
    // past the last level nothing is left to eliminate
    CHECK(schur_cr_level(N, levels).count == 0, "N %lld: a level past the last", n);
    CHECK(schur_cr_workspace(N, 9) == kSchurFixed + N + 3 * N * 81 + 2 * N * 9, "N %lld: workspace", n);
}

int main() {
    const int64_t grids[] = {1, 2, 3, 4, 5, 7, 8, 9, 33, 1000};
    int cases = 0;
    for (int64_t N : grids) { one_grid(N); ++cases; }
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("ok: %d grids\n", cases);
    return 0;
}
