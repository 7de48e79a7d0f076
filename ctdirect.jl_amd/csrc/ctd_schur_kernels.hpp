// ctd_schur_kernels.hpp -- the kernels of the chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*, include/ctdirect_hip.h):
// workspace, arguments and launchers.  The kernels are in ctd_schur.hip; they do not depend on the OCP, so they are compiled once
// into the library, with strict rounding (-ffp-contract=off), like ctd_krylov.hip.  The host-side plan: ctd_schur_plan.hpp.
//
// THE MATRIX.  Rows in N blocks of m (block k = the rows [k m, (k + 1) m)); columns >= v_off (the tail columns) dropped; w_c = 1.0 /
// px[c].  With row(r) the CSR row r of the handle's pattern (columns ascending) and J its values:
//   D_k(a, b) = sum over the columns c < v_off common to row(k m + a) and row(k m + b)       of (J[k m + a, c] J[k m + b, c]) w_c
//   E_k(a, b) = sum over the columns c < v_off common to row((k + 1) m + a) and row(k m + b) of (J[(k + 1) m + a, c] J[k m + b, c]) w_c
// every sum in ascending column order starting from 0.0, each term the product of the two Jacobian values first (so D_k is symmetric
// bit for bit), then times w_c; sc[k m + a] is added to D_k(a, a) last.  E_k is formed where block k + 1 belongs to the chunk of
// block k, and is 0.0 elsewhere.  One thread per entry (ASSEMBLE, the first launch of the factor).
//
// THE FACTOR (second launch; one wave = one workgroup of 64 lanes per chunk, workgroup g serving the chunks g, g + G, g + 2 G, ...
// of G = min(n_chunks, kSchurMaxWg) workgroups).  Per chunk, blocks in ascending order, both results stored in place:
//   A = D_k - F_{k-1} F_{k-1}'   lower triangle: A(a, b) = D_k(a, b) - s, s = sum_j F_{k-1}(a, j) F_{k-1}(b, j), j ascending from 0.0
//                                (not for the first block of a chunk)
//   L_k L_k' = A                 column by column (j ascending): s = A(a, j); s -= L(a, p) L(j, p) for p = 0 .. j - 1 in that order;
//                                L(j, j) = sqrt(s), rho_j = 1.0 / L(j, j); L(a, j) = s rho_j for a > j.  The upper triangle is
//                                stored as 0.0
//   F_k = E_k L_k^-T             row by row: s = E(a, j); s -= F(a, p) L(j, p) for p = 0 .. j - 1; F(a, j) = s rho_j, j ascending
// (divisions by a pivot's root are products with its reciprocal rho_j, rounded once: one division per row instead of one per use)
// A pivot s that is not positive or not finite: the block's index goes into the chunk's status word (-1 otherwise) and L_k, F_k of
// that block and of every later block of the chunk are filled with NaN.  Blocks are staged in LDS; the loads of block k + 1 are
// issued into registers before the recurrence of block k.
//
// THE SOLVE (one launch, the same assignment of chunks to waves; G = min(N, kSchurMaxWg): the chunk length is read from the workspace)
//   forward, k ascending:   g(a) = r(a) - s, s = sum_j F_{k-1}(a, j) t_{k-1}(j), j ascending from 0.0 (not for the first block);
//                           then for j ascending: t(j) = g(j) rho_j, rho_j = 1.0 / L(j, j); g(a) -= L(a, j) t(j) for a > j
//   backward, k descending: g(a) = t_k(a) - s, s = sum_j F_k(j, a) y_{k+1}(j), j ascending from 0.0 (not for the last block);
//                           then for j descending: y(j) = g(j) rho_j; g(a) -= L(j, a) y(j) for a < j
// Inside MINRES the launch also leaves one partial sum of r . y per workgroup: lane a adds r(k m + a) y(k m + a) in the order it
// produces them (chunks g, g + G, ..., within a chunk k descending) starting from 0.0, then the shuffle tree of ctd_common.hpp (off =
// 32, ..., 1); a workgroup without a chunk stores 0.0.  The Krylov kernels add these G partial sums after their own, in ascending
// workgroup order (ctd_krylov.hip, the SCHUR instantiations).
//
// WORKSPACE (schur_workspace(N, m) doubles): [0, 16) the header -- 64-bit integers: a tag, N, m, the chunk length, the chunk count,
// written by the assemble launch --, [16, 16 + kSchurMaxWg) the partial sums, [512, 512 + N) the chunks' status words (64-bit
// integers; -1 past the chunk count), then the N blocks D_k -> L_k and the N blocks E_k -> F_k, row-major m x m.  The solve checks
// the header against its own N and m and stores nothing when it does not match.
// Kernel boundaries are the only synchronisation between workgroups; plain C++ stores only.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ctd_krylov_kernels.hpp"
#include "ctd_schur_plan.hpp"

namespace ctd {

constexpr int kSchurMaxWg = 256;            // cap of the workgroup count of the factor and the solve: the partial sums (C) adds
constexpr int kSchurPart = 16;              // offset of the partial sums in the workspace
constexpr int64_t kSchurTag = 0x5343485552303031;      // "SCHUR001"
static_assert(kSchurPart + kSchurMaxWg <= kSchurFixed, "the fixed part of the workspace");

struct SchurFactorParams {
    int64_t N, v_off, chunk_steps, n_chunks;
    int32_t m, pad;
    const int64_t *rowptr, *colind;
    const double *jvals, *px, *sc;          // sc may be null
    double* ws;
};

enum SchurSolveMode : int32_t { SCHUR_PLAIN = 0, SCHUR_START = 1, SCHUR_ITER = 2 };
// mode: SCHUR_PLAIN the solve alone; SCHUR_START also the partial sums; SCHUR_ITER also the freeze: nothing is stored unless
// cur->status is KRYLOV_RUNNING
struct SchurSolveParams {
    int64_t N;
    int32_t m, mode;
    const double* ws;
    const double* r;
    double* out;
    double* part;
    const KrylovState* cur;
};

inline int schur_solve_grid(int64_t N) { return (int)(N < 1 ? 1 : (N > kSchurMaxWg ? kSchurMaxWg : N)); }

// Launchers (ctd_schur.hip), enqueue-only on `st`
hipError_t schur_factor(const SchurFactorParams& fp, hipStream_t st);       // assemble, then the block Cholesky
hipError_t schur_solve(const SchurSolveParams& sp, hipStream_t st);

}  // namespace ctd
