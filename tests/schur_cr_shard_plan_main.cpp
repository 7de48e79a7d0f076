// TEST INFRASTRUCTURE ONLY -- stand-alone check of the shard cut of the plan of the log-depth exact Schur preconditioner
// (schur_cr_shard_cut, schur_cr_shard_range_ok of csrc/ctd_schur_plan.hpp).  tests/test_kkt_schur_cr_shard_cpu.py builds this with
// g++ -fsanitize=address,undefined and runs it; the header is pure C++, no GPU.
//
// For every grid size and every way to cut it into up to four ranks of unequal lengths: the ranks' blocks partition [0, N); a rank's
// fields are those of the whole-grid plan of n_blocks blocks (levels, launch counts, workspace); its first row is step_begin m; the
// tail fields are the grid's; one rank is the grid itself; ranges outside the grid are refused.
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

static SchurCrPlan grid_plan(int64_t N, int64_t m) {
    SchurCrPlan g{};
    g.N = N;
    g.block_rows = m;
    g.first_tail_row = N * m;
    g.tail_rows = 3;
    g.tail_cols = 1;
    g.first_tail_col = 100 * N;
    g.n_levels = schur_cr_levels(N);
    g.factor_launches = schur_cr_factor_launches(N);
    g.solve_launches = schur_cr_solve_launches(N);
    g.workspace = schur_cr_workspace(N, m);
    return g;
}

static long g_cuts = 0;
static void one_cut(const SchurCrPlan& g, const std::vector<int64_t>& cuts) {
    const long long N = (long long)g.N;
    std::vector<int> seen((size_t)g.N, 0);
    for (size_t r = 0; r + 1 < cuts.size(); ++r) {
        const int64_t sb = cuts[r], se = cuts[r + 1];
        CHECK(schur_cr_shard_range_ok(g.N, sb, se), "N %lld: [%lld, %lld) refused", N, (long long)sb, (long long)se);
        const SchurCrShardPlan s = schur_cr_shard_cut(g, sb, se);
        CHECK(s.N == g.N && s.step_begin == sb && s.step_end == se && s.n_blocks == se - sb, "N %lld: range of rank %zu", N, r);
        CHECK(s.block_rows == g.block_rows && s.first_row == sb * g.block_rows, "N %lld: rows of rank %zu", N, r);
        CHECK(s.tail_rows == g.tail_rows && s.first_tail_row == g.first_tail_row && s.tail_cols == g.tail_cols &&
                  s.first_tail_col == g.first_tail_col, "N %lld: tail of rank %zu", N, r);
        CHECK(s.n_levels == schur_cr_levels(s.n_blocks) && s.factor_launches == 2 * s.n_levels + 2 && s.solve_launches == 2 * s.n_levels + 1,
              "N %lld: levels of rank %zu", N, r);
        CHECK(s.workspace == schur_cr_workspace(s.n_blocks, g.block_rows), "N %lld: workspace of rank %zu", N, r);
        CHECK(s.n_levels <= g.n_levels, "N %lld: rank %zu deeper than the grid", N, r);
        for (int64_t k = sb; k < se; ++k) ++seen[(size_t)k];
        // every level of the rank stays inside its blocks
        for (int l = 0; l < s.n_levels; ++l) {
            const SchurCrLevel lv = schur_cr_level(s.n_blocks, l);
            CHECK(lv.count >= 1 && lv.first + (lv.count - 1) * lv.stride < s.n_blocks, "N %lld: level %d of rank %zu leaves its blocks", N, l, r);
        }
    }
    for (int64_t k = 0; k < g.N; ++k) CHECK(seen[(size_t)k] == 1, "N %lld: block %lld covered %d times", N, (long long)k, seen[(size_t)k]);
    ++g_cuts;
}

static void one_grid(int64_t N, int64_t m) {
    const SchurCrPlan g = grid_plan(N, m);
    // one rank: the grid itself
    const SchurCrShardPlan one = schur_cr_shard_cut(g, 0, N);
    CHECK(one.n_blocks == N && one.first_row == 0 && one.n_levels == g.n_levels && one.factor_launches == g.factor_launches &&
              one.solve_launches == g.solve_launches && one.workspace == g.workspace, "N %lld: one rank is not the grid", (long long)N);
    one_cut(g, {0, N});
    // every cut into two, three and (for small grids) four ranks
    for (int64_t a = 1; a < N; ++a) {
        one_cut(g, {0, a, N});
        for (int64_t b = a + 1; b < N && N <= 33; ++b) {
            one_cut(g, {0, a, b, N});
            for (int64_t c = b + 1; c < N && N <= 9; ++c) one_cut(g, {0, a, b, c, N});
        }
    }
    // refused ranges
    CHECK(!schur_cr_shard_range_ok(N, -1, 1) && !schur_cr_shard_range_ok(N, 0, 0) && !schur_cr_shard_range_ok(N, 0, N + 1) &&
              !schur_cr_shard_range_ok(N, N, N) && !schur_cr_shard_range_ok(N, 1, 0), "N %lld: a range outside the grid accepted", (long long)N);
}

int main() {
    const int64_t grids[] = {1, 2, 3, 4, 5, 7, 8, 9, 20, 33, 1000};
    int cases = 0;
    for (int64_t N : grids) { one_grid(N, N % 2 ? 9 : 4); ++cases; }
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("ok: %d grids, %ld cuts\n", cases, g_cuts);
    return 0;
}
