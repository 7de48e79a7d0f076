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

// ---- the joined form (ctd_kkt_schur_cr_joint_*): the shard form with the couplings across the ranks restored ---------------------------
// Rank r of n_ranks holds the steps [step_begin, step_end).  Every rank but rank 0 gives up its first block as a separator; its
// interior, the blocks [int_begin, step_end) with int_begin = step_begin + (rank > 0), is factored exactly by the recurrences above
// (n_int blocks through offset pointers, as the shard form does), and the n_ranks - 1 separators are joined by a reduced block
// tridiagonal system that every rank factors redundantly (kernels, records and orders: ctd_schur_cr_joint_kernels.hpp).
constexpr int kSchurJointMaxRanks = 256;    // accepted n_ranks: the reduced sweep over n_ranks - 1 blocks is sequential, one wave
constexpr int64_t kSchurJointHead = 16;     // doubles of a record before its blocks / vectors
constexpr int64_t schur_cr_joint_factor_slot(int64_t m) { return kSchurJointHead + 4 * m * m; }       // (sb, se, m, rank; D_s, Cll, Crl, Crr)
constexpr int64_t kSchurJointSolveSlot = kSchurJointHead + 3 * kSchurMaxBlock;                     // (rank; r_s, qu, qd: 64 apart)

// Offsets in doubles into the workspace.  [0, off_es): the workspace of the log-depth form for the interior (with this family's tag
// in word 0 of the header and, behind the words of the shard form, step_begin, step_end, n_ranks and rank in the words 5 .. 8); then
// E[s] = T(int_begin, s), E[b] = T(step_end, step_end - 1) and D_s (m^2 each, zero where the rank has none); the spikes Wl and Wr
// (n_int m^2 each, block k row-major m x m); the scratch of the multi-column solve (2 m columns of n_int m running right-hand sides,
// then as many of y); the reduced factor (n_sep status words, n_sep blocks L_k, n_sep blocks F_k; n_sep = max(n_ranks - 1, 1)); rs~
// and x_s (n_sep m each); sigma (16, the first is used)
struct SchurCrJointPlan {
    int64_t N, n_ranks, rank, step_begin, step_end, separator, int_begin, n_int, block_rows, first_row, tail_rows, first_tail_row, tail_cols,
        first_tail_col, n_levels, n_sep, factor_local_launches, factor_join_launches, solve_local_launches, solve_join_launches, factor_slot,
        solve_slot, off_es, off_eb, off_ds, off_wl, off_wr, off_scratch, off_reduced, off_rs, off_xs, off_sigma, workspace, jvals_begin,
        jvals_end, jvals_halo_begin, jvals_halo_end, px_begin, px_end;
};
// what the step range and the rank must satisfy: inside the grid, able to be block `rank` of n_ranks ascending blocks, and at least
// one interior block behind the separator
inline bool schur_cr_joint_range_ok(int64_t N, int64_t n_ranks, int64_t rank, int64_t sb, int64_t se) {
    if (!schur_cr_shard_range_ok(N, sb, se) || n_ranks < 1 || n_ranks > kSchurJointMaxRanks || rank < 0 || rank >= n_ranks) return false;
    if ((rank == 0) != (sb == 0) || (rank == n_ranks - 1) != (se == N)) return false;
    return rank == 0 || se - sb >= 2;
}
// the fields that are functions of the grid's plan, the step range and the rank alone (no model): everything but the read set
inline SchurCrJointPlan schur_cr_joint_cut(const SchurCrPlan& g, int64_t n_ranks, int64_t rank, int64_t sb, int64_t se) {
    SchurCrJointPlan s{};
    const int64_t m = g.block_rows, mm = m * m;
    s.N = g.N;
    s.n_ranks = n_ranks;
    s.rank = rank;
    s.step_begin = sb;
    s.step_end = se;
    s.separator = rank > 0 ? sb : -1;
    s.int_begin = sb + (rank > 0 ? 1 : 0);
    s.n_int = se - s.int_begin;
    s.block_rows = m;
    s.first_row = sb * m;
    s.tail_rows = g.tail_rows;
    s.first_tail_row = g.first_tail_row;
    s.tail_cols = g.tail_cols;
    s.first_tail_col = g.first_tail_col;
    s.n_levels = schur_cr_levels(s.n_int);
    s.n_sep = n_ranks > 1 ? n_ranks - 1 : 1;
    // local factor: the interior's factor; with more than one rank the interface assemble, the multi-column solve, the contributions
    s.factor_local_launches = schur_cr_factor_launches(s.n_int) + (n_ranks > 1 ? schur_cr_solve_launches(s.n_int) + 2 : 0);
    s.factor_join_launches = n_ranks > 1 ? 1 : 0;       // the reduced matrix from the records and its block Cholesky, one wave
    s.solve_local_launches = schur_cr_solve_launches(s.n_int) + (n_ranks > 1 ? 1 : 0);        // ... and the record
    s.solve_join_launches = n_ranks > 1 ? 2 : 0;        // rs~, the reduced sweeps and sigma, one wave; the correction
    s.factor_slot = schur_cr_joint_factor_slot(m);
    s.solve_slot = kSchurJointSolveSlot;
    s.off_es = schur_cr_workspace(s.n_int, m);
    s.off_eb = s.off_es + mm;
    s.off_ds = s.off_eb + mm;
    s.off_wl = s.off_ds + mm;
    s.off_wr = s.off_wl + s.n_int * mm;
    s.off_scratch = s.off_wr + s.n_int * mm;
    s.off_reduced = s.off_scratch + 4 * s.n_int * mm;
    s.off_rs = s.off_reduced + s.n_sep + 2 * s.n_sep * mm;
    s.off_xs = s.off_rs + s.n_sep * m;
    s.off_sigma = s.off_xs + s.n_sep * m;
    s.workspace = s.off_sigma + 16;
    return s;
}
// The refusals and the pattern check of plan_kkt_schur_cr, then schur_cr_joint_range_ok (ST_EINVAL, with the reason), then the
// fields.  ranges: the read set of the factor.  jvals on [jvals_begin, jvals_end), the CSR range of the rank's own block rows (the
// separator's included), and on the halo [jvals_halo_begin, jvals_halo_end), the CSR range of the rows of block step_end, which
// E[b] reads (empty on the last rank; it lies right behind the rank's own range).  px on [px_begin, px_end), the span of the non-tail
// columns of the rank's own rows: E[b] adds over the columns that a row of block step_end shares with a row of block step_end - 1,
// which lie inside that span
int plan_kkt_schur_cr_joint(const Model& m, int64_t n_ranks, int64_t rank, int64_t step_begin, int64_t step_end, bool verify, bool ranges,
                            SchurCrJointPlan& out, std::string& err);

}  // namespace ctd
