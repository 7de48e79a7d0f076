// TEST INFRASTRUCTURE ONLY -- stand-alone check of the plan of the joined form of the log-depth Schur preconditioner
// (schur_cr_joint_cut, schur_cr_joint_range_ok of csrc/ctd_schur_plan.hpp).  tests/test_kkt_schur_cr_joint_cpu.py builds this with
// g++ -fsanitize=address,undefined and runs it; the header is pure C++, no GPU.
//
// For every grid size and every admissible way to cut it into up to four ranks (every rank but the first has at least two steps):
// separators and interiors partition [0, N); a rank's interior has the levels of the whole-grid plan of n_int blocks; the regions of
// the workspace follow each other in the documented order without overlap, every one of its documented size, and fill the
// workspace; the launch counts; one rank has no separator and no join launch; cuts with a one-step rank >= 1 and inconsistent
// (n_ranks, rank, range) triples are refused.
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

static long g_cuts = 0, g_refused = 0;
static void one_cut(const SchurCrPlan& g, const std::vector<int64_t>& cuts) {
    const long long N = (long long)g.N;
    const int64_t G = (int64_t)cuts.size() - 1, m = g.block_rows, mm = m * m;
    bool admissible = true;
    for (int64_t r = 1; r < G; ++r) admissible = admissible && cuts[(size_t)r + 1] - cuts[(size_t)r] >= 2;
    if (!admissible) {
        bool all_ok = true;
        for (int64_t r = 0; r < G; ++r) all_ok = all_ok && schur_cr_joint_range_ok(g.N, G, r, cuts[(size_t)r], cuts[(size_t)r + 1]);
        CHECK(!all_ok, "N %lld: a cut with a one-step rank >= 1 accepted", N);
        ++g_refused;
        return;
    }
    std::vector<int> seen((size_t)g.N, 0);
    for (int64_t r = 0; r < G; ++r) {
        const int64_t sb = cuts[(size_t)r], se = cuts[(size_t)r + 1];
        CHECK(schur_cr_joint_range_ok(g.N, G, r, sb, se), "N %lld: rank %lld [%lld, %lld) refused", N, (long long)r, (long long)sb, (long long)se);
        const SchurCrJointPlan s = schur_cr_joint_cut(g, G, r, sb, se);
        CHECK(s.N == g.N && s.n_ranks == G && s.rank == r && s.step_begin == sb && s.step_end == se, "N %lld: identity of rank %lld", N, (long long)r);
        CHECK(s.separator == (r > 0 ? sb : -1) && s.int_begin == sb + (r > 0) && s.n_int == se - s.int_begin && s.n_int >= 1,
              "N %lld: separator / interior of rank %lld", N, (long long)r);
        CHECK(s.block_rows == m && s.first_row == sb * m && s.tail_rows == g.tail_rows && s.first_tail_row == g.first_tail_row &&
                  s.tail_cols == g.tail_cols && s.first_tail_col == g.first_tail_col, "N %lld: rows / tail of rank %lld", N, (long long)r);
        CHECK(s.n_levels == schur_cr_levels(s.n_int) && s.n_sep == (G > 1 ? G - 1 : 1), "N %lld: levels of rank %lld", N, (long long)r);
        const int64_t L = s.n_levels;
        CHECK(s.factor_local_launches == 2 * L + 2 + (G > 1 ? 2 * L + 3 : 0) && s.factor_join_launches == (G > 1 ? 1 : 0) &&
                  s.solve_local_launches == 2 * L + 1 + (G > 1 ? 1 : 0) && s.solve_join_launches == (G > 1 ? 2 : 0),
              "N %lld: launches of rank %lld", N, (long long)r);
        CHECK(s.factor_slot == 16 + 4 * mm && s.solve_slot == 16 + 3 * 64, "N %lld: slots of rank %lld", N, (long long)r);
        // the regions in their order, each of its size, filling the workspace
        const int64_t off[] = {0, s.off_es, s.off_eb, s.off_ds, s.off_wl, s.off_wr, s.off_scratch, s.off_reduced, s.off_rs, s.off_xs, s.off_sigma,
                               s.workspace};
        const int64_t len[] = {schur_cr_workspace(s.n_int, m), mm, mm, mm, s.n_int * mm, s.n_int * mm, 4 * s.n_int * mm,
                               s.n_sep + 2 * s.n_sep * mm, s.n_sep * m, s.n_sep * m, 16};
        for (int i = 0; i < 11; ++i)
            CHECK(off[i + 1] - off[i] == len[i], "N %lld: region %d of rank %lld has %lld doubles, not %lld", N, i, (long long)r,
                  (long long)(off[i + 1] - off[i]), (long long)len[i]);
        if (r > 0) ++seen[(size_t)s.separator];
        for (int64_t k = s.int_begin; k < se; ++k) ++seen[(size_t)k];
        for (int l = 0; l < s.n_levels; ++l) {
            const SchurCrLevel lv = schur_cr_level(s.n_int, l);
            CHECK(lv.count >= 1 && lv.first + (lv.count - 1) * lv.stride < s.n_int, "N %lld: level %d of rank %lld leaves its interior", N, l,
                  (long long)r);
        }
        // the first and the last rank are tied to the ends of the grid
        CHECK((r == 0 || !schur_cr_joint_range_ok(g.N, G, 0, sb, se)) && (r == G - 1 || !schur_cr_joint_range_ok(g.N, G, G - 1, sb, se)),
              "N %lld: rank %lld accepted as the first or the last rank", N, (long long)r);
        CHECK(!schur_cr_joint_range_ok(g.N, G, -1, sb, se) && !schur_cr_joint_range_ok(g.N, 0, r, sb, se) &&
                  !schur_cr_joint_range_ok(g.N, kSchurJointMaxRanks + 1, r, sb, se), "N %lld: rank or n_ranks outside their ranges accepted", N);
    }
    for (int64_t k = 0; k < g.N; ++k) CHECK(seen[(size_t)k] == 1, "N %lld: block %lld covered %d times", N, (long long)k, seen[(size_t)k]);
    ++g_cuts;
}

static void one_grid(int64_t N, int64_t m) {
    const SchurCrPlan g = grid_plan(N, m);
    // one rank: the grid itself, the workspace of the log-depth form and the (unused) regions behind it
    const SchurCrJointPlan one = schur_cr_joint_cut(g, 1, 0, 0, N);
    CHECK(one.separator == -1 && one.int_begin == 0 && one.n_int == N && one.n_levels == g.n_levels && one.off_es == g.workspace &&
              one.factor_local_launches == g.factor_launches && one.solve_local_launches == g.solve_launches && one.factor_join_launches == 0 &&
              one.solve_join_launches == 0, "N %lld: one rank is not the grid", (long long)N);
    one_cut(g, {0, N});
    for (int64_t a = 1; a < N; ++a) {
        one_cut(g, {0, a, N});
        for (int64_t b = a + 1; b < N && N <= 33; ++b) {
            one_cut(g, {0, a, b, N});
            for (int64_t c = b + 1; c < N && N <= 9; ++c) one_cut(g, {0, a, b, c, N});
        }
    }
    CHECK(!schur_cr_joint_range_ok(N, 1, 0, -1, 1) && !schur_cr_joint_range_ok(N, 1, 0, 0, 0) && !schur_cr_joint_range_ok(N, 1, 0, 0, N + 1) &&
              !schur_cr_joint_range_ok(N, 2, 0, 0, N) && !schur_cr_joint_range_ok(N, 2, 1, 0, N), "N %lld: an inconsistent range accepted",
          (long long)N);
}

int main() {
    const int64_t grids[] = {1, 2, 3, 4, 5, 7, 8, 9, 20, 33, 1000};
    int cases = 0;
    for (int64_t N : grids) { one_grid(N, N % 2 ? 9 : 4); ++cases; }
    if (g_bad) { std::printf("%d checks failed\n", g_bad); return 1; }
    std::printf("ok: %d grids, %ld cuts, %ld refused\n", cases, g_cuts, g_refused);
    return 0;
}
