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

}  // namespace ctd
