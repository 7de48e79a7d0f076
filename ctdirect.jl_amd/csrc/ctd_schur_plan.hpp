// ctd_schur_plan.hpp -- the host-side plan of the chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*,
// include/ctdirect_hip.h): block size, tail, chunks and workspace, derived from the model's layout; and the check of the model's own
// Jacobian pattern the block-tridiagonal form rests on.  Pure C++ (no HIP): ctd_host.cpp implements it, tested without a device.
// The kernels and the order of their sums: ctd_schur_kernels.hpp.
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

}  // namespace ctd
