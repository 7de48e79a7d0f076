// ctd_schur_plan.hpp -- the host-side plan of the chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*,
// include/ctdirect_hip.h): block size, tail, chunks and workspace, derived from the model's layout; and the check of the model's own
// Jacobian pattern the block-tridiagonal form rests on; below it the plan of the log-depth exact form (ctd_kkt_schur_cr*): levels,
// launch counts, workspace.  Pure C++ (no HIP): ctd_host.cpp implements it, tested without a device.
// The kernels and the order of their sums: ctd_schur_kernels.hpp, ctd_schur_cr_kernels.hpp.
#pragma once
#include <cstdint>
#include <string>

namespace ctd {

struct Model;

constexpr int kSchurMaxBlock = 64;          // largest block_rows: one lane of a wave per row of a block
constexpr int64_t kSchurFixed = 512;        // doubles of the workspace before the per-chunk status words (CTD_KKT_SCHUR_FIXED)

// N blocks of m = block_rows rows (block k: the rows [k m, (k + 1) m) of step k), then tail_rows rows from first_tail_row on; the
// last tail_cols variables (from first_tail_col on) are the tail columns.  Chunk c: the blocks [c chunk_steps, min((c + 1)
// chunk_steps, N)); chunk_steps is the effective length min(requested, N).  workspace: doubles (schur_workspace)
struct SchurPlan {
    int64_t N, block_rows, tail_rows, first_tail_row, tail_cols, first_tail_col, n_chunks, chunk_steps, workspace;
};
inline int64_t schur_workspace(int64_t N, int64_t m) { return kSchurFixed + N + 2 * N * m * m; }

// Status codes as build_model; err receives the reason.  Refused: a CSC model (ST_EINVAL), block_rows > kSchurMaxBlock, chunk_steps
// < 1 (ST_EINVAL).  verify: walk the model's rows (gen_row) and refuse with ST_EPATTERN, naming the row, a pattern in which two rows
// that share a non-tail column lie more than one block apart (tail rows exempt) -- O(nnzj), so callers that plan repeatedly verify once
int plan_kkt_schur(const Model& m, int64_t chunk_steps, bool verify, SchurPlan& out, std::string& err);

// ---- the log-depth exact form (ctd_kkt_schur_cr*; kernels and orders: ctd_schur_cr_kernels.hpp) --------------------------------------
// The one-chunk matrix T, factored and applied by block odd-even (cyclic) reduction of the N blocks: n_levels = ceil(log2 N) levels
// (0 for N = 1).  At level l the active blocks are the multiples of 2^l; the eliminated ones are first + q stride, q = 0 .. count -
// 1, with first = 2^l and stride = 2^(l + 1).  An eliminated block i has the left neighbour i - 2^l (always) and the right neighbour
// i + 2^l when that is below N: every eliminated block of a level has one but possibly the last (last_has_right).
struct SchurCrLevel {
    int64_t first, stride, count;
    int32_t last_has_right, pad;
};
inline int schur_cr_levels(int64_t N) {
    int l = 0;
    while (((int64_t)1 << l) < N) ++l;
    return l;
}
inline SchurCrLevel schur_cr_level(int64_t N, int level) {
    SchurCrLevel v{};
    v.first = (int64_t)1 << level;
    v.stride = v.first * 2;
    v.count = N > v.first ? (N - v.first + v.stride - 1) / v.stride : 0;
    v.last_has_right = (v.count > 0 && v.first + (v.count - 1) * v.stride + v.first < N) ? 1 : 0;
    return v;
}
// Launches, functions of N alone.  Factor: assemble, per level eliminate + update, the root.  Solve: per level one launch down, the
// root, per level one launch up; inside MINRES one more, the partial sums of r2 . y
inline int64_t schur_cr_factor_launches(int64_t N) { return 2 * (int64_t)schur_cr_levels(N) + 2; }
inline int64_t schur_cr_solve_launches(int64_t N) { return 2 * (int64_t)schur_cr_levels(N) + 1; }
// doubles (CTD_KKT_SCHUR_CR_WORKSPACE): the fixed part, N status words, the blocks D -> L, E -> Gp / new couplings, Gm, and the
// solve's scratch: the running right-hand side and y
inline int64_t schur_cr_workspace(int64_t N, int64_t m) { return kSchurFixed + N + 3 * N * m * m + 2 * N * m; }

struct SchurCrPlan {
    int64_t N, block_rows, tail_rows, first_tail_row, tail_cols, first_tail_col, n_levels, factor_launches, solve_launches, workspace;
};
// The refusals and the pattern check of plan_kkt_schur (one chunk), then the fields above
int plan_kkt_schur_cr(const Model& m, bool verify, SchurCrPlan& out, std::string& err);

// ---- the shard form of the log-depth exact form (ctd_kkt_schur_cr_shard_*) ------------------------------------------------------------
// A rank holds the steps [step_begin, step_end): its matrix T_r is the principal submatrix of T on those n_blocks blocks, factored
// and applied by the recurrences above with the block index taken relative to step_begin and n_blocks in place of N (the coupling
// T(step_end, step_end - 1) to the next rank's first block is dropped).  first_row = step_begin block_rows.  The tail fields are the
// grid's.  The read set of the factor, half-open: [jvals_begin, jvals_end) the CSR range of the rank's block rows; [px_begin, px_end)
// the span of the non-tail columns of those rows (filled when `ranges` is set: a walk of the rank's rows)
struct SchurCrShardPlan {
    int64_t N, step_begin, step_end, n_blocks, block_rows, first_row, tail_rows, first_tail_row, tail_cols, first_tail_col, n_levels,
        factor_launches, solve_launches, workspace, jvals_begin, jvals_end, px_begin, px_end;
};
// the step range as a plan takes it: 0 <= step_begin < step_end <= N
inline bool schur_cr_shard_range_ok(int64_t N, int64_t step_begin, int64_t step_end) {
    return step_begin >= 0 && step_begin < step_end && step_end <= N;
}
// the fields that are functions of the grid's plan and the step range alone (no model): everything but the read set
inline SchurCrShardPlan schur_cr_shard_cut(const SchurCrPlan& g, int64_t step_begin, int64_t step_end) {
    SchurCrShardPlan s{};
    s.N = g.N;
    s.step_begin = step_begin;
    s.step_end = step_end;
    s.n_blocks = step_end - step_begin;
    s.block_rows = g.block_rows;
    s.first_row = step_begin * g.block_rows;
    s.tail_rows = g.tail_rows;
    s.first_tail_row = g.first_tail_row;
    s.tail_cols = g.tail_cols;
    s.first_tail_col = g.first_tail_col;
    s.n_levels = schur_cr_levels(s.n_blocks);
    s.factor_launches = schur_cr_factor_launches(s.n_blocks);
    s.solve_launches = schur_cr_solve_launches(s.n_blocks);
    s.workspace = schur_cr_workspace(s.n_blocks, g.block_rows);
    return s;
}
// The refusals and the pattern check of plan_kkt_schur_cr, a step range that is not inside the grid (ST_EINVAL), then the fields
int plan_kkt_schur_cr_shard(const Model& m, int64_t step_begin, int64_t step_end, bool verify, bool ranges, SchurCrShardPlan& out,
                            std::string& err);

}  // namespace ctd
