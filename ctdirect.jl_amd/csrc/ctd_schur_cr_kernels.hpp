// ctd_schur_cr_kernels.hpp -- the kernels of the log-depth exact block-tridiagonal Schur preconditioner (ctd_kkt_schur_cr*,
// include/ctdirect_hip.h): workspace, arguments and launchers.  The kernels are in ctd_schur_cr.hip; they do not depend on the OCP,
// so they are compiled once into the library, with strict rounding (-ffp-contract=off), like ctd_schur.hip.  The host-side plan and
// the index sets of a level: ctd_schur_plan.hpp.
//
// THE MATRIX is T of ctd_schur_kernels.hpp with one chunk: diagonal blocks D_i and couplings E_i = T(i + 1, i), i + 1 < N, assembled
// by the same expressions in the same order (one thread per entry; the first launch of the factor).  No coupling is dropped.
//
// THE FACTOR is the block Cholesky of T in the nested-dissection (odd-even, cyclic reduction) order of the blocks.  Level l = 0 ..
// n_levels - 1, h = 2^l: the active blocks are the multiples of h, the eliminated ones the odd multiples i, with the left neighbour
// lf = i - h and, when i + h < N, the right neighbour rt = i + h.  The slot E[k] of an active block k holds the current coupling T(k',
// k) to the next active block k'.  Two launches per level:
//   ELIMINATE (one wave = one workgroup of 64 lanes per eliminated block, grid-stride; D_i, E[lf] and E[i] staged in LDS)
//     L_i L_i' = D_i          column by column as ctd_schur_kernels.hpp: s = A(a, j); s -= L(a, p) L(j, p), p = 0 .. j - 1; L(j, j) =
//                             sqrt(s), rho_j = 1.0 / L(j, j); L(a, j) = s rho_j for a > j; the upper triangle is stored as 0.0
//     Gm_i = L_i^-1 E[lf]     lane b owns column b: for j ascending, s = E(j, b); s -= L(j, p) Gm(p, b), p = 0 .. j - 1; Gm(j, b) = s
//                             rho_j.  Stored in the slot Gm[i]
//     Gp_i = E[i] L_i^-T      lane a owns row a (only when rt exists): for j ascending, s = E(a, j); s -= Gp(a, p) L(j, p), p = 0 .. j
//                             - 1; Gp(a, j) = s rho_j.  Stored in place, in the slot E[i]
//   UPDATE (one thread per entry of the survivors' D, lower triangle, and of the new couplings; a survivor k is an even multiple of h)
//     D_k(a, b) = (D_k(a, b) - s1) - s2      s1 = sum_j Gp_i(a, j) Gp_i(b, j) of the left eliminated neighbour i = k - h (if k >= h),
//                                            s2 = sum_j Gm_i(j, a) Gm_i(j, b) of the right one i = k + h (if k + h < N): the left
//                                            neighbour's term first
//     E[k](a, b) = -s                        s = sum_j Gp_i(a, j) Gm_i(j, b), i = k + h, when k + 2 h < N: the coupling T(k + 2 h, k)
//   every sum with j ascending from 0.0.  An entry is written by one thread, which reads both neighbours' blocks: no atomics.
// After the last level the ROOT launch factors D_0 (one wave).  2 n_levels + 2 launches in all, a function of N alone.
// A pivot s that is not positive or not finite: its column j goes into the status word of the block (one word per block index, -1
// otherwise) and L_i, Gm_i and Gp_i are filled with NaN, which reaches the later levels through the updates by ordinary arithmetic.
//
// THE SOLVE.  rhs_k is r(k) until block k has been a survivor, and the workspace's running right-hand side from then on.
//   DOWN, l ascending, one launch per level, one wave per ACTIVE block: an eliminated block i stores y_i = L_i^-1 rhs_i (for j
//     ascending: t = g(j) rho_j, rho_j = 1.0 / L(j, j); g(a) -= L(a, j) t for a > j); a survivor k forms y of its (up to) two
//     eliminated neighbours again -- the same bits: the same inputs in the same order -- and stores
//       rhs_k(a) = (rhs_k(a) - s1) - s2,  s1 = sum_j Gp_i(a, j) y_i(j), i = k - h;  s2 = sum_j Gm_i(j, a) y_i(j), i = k + h
//     (the left term first).  Forming y_i twice more costs two triangular solves of m^2 flops per survivor and saves one launch per
//     level: the solve is bound by the number of dependent launches, not by arithmetic.
//   ROOT, one wave: x_0 = L_0^-T L_0^-1 rhs_0.
//   UP, l descending, one launch per level, one wave per eliminated block:
//       g(a) = (y_i(a) - s1) - s2,  s1 = sum_j Gm_i(a, j) x_lf(j),  s2 = sum_j Gp_i(j, a) x_rt(j)  (if rt exists);  x_i = L_i^-T g
//     (for j descending: x(j) = g(j) rho_j; g(a) -= L(j, a) x(j) for a < j).
//   2 n_levels + 1 launches.  Inside MINRES one more launch leaves the partial sums of r . x: G = min(N, kSchurMaxWg) workgroups of
//   one wave, workgroup g adds for the blocks k = g, g + G, ... in that order, in lane a, r(k m + a) x(k m + a) starting from 0.0,
//   then the shuffle tree of ctd_common.hpp (off = 32, ..., 1).  (C) adds them as it adds the chunked solve's.
//
// WORKSPACE (schur_cr_workspace(N, m) doubles): [0, 16) the header -- 64-bit integers: the tag, N, m, n_levels --, [16, 16 +
// kSchurMaxWg) the partial sums, [512, 512 + N) the status words, N blocks D_k -> L_k, N slots E[k] (couplings -> Gp), N slots Gm[k],
// all row-major m x m, then the solve's scratch: N m running right-hand sides and N m entries of y.  The factor writes all of it;
// the solve writes the scratch (and the partial sums) only.  The solve checks the header against its own N and m and stores
// nothing when it does not match; in iteration mode every launch stores nothing unless cur->status is KRYLOV_RUNNING.
// Kernel boundaries are the only synchronisation between workgroups; plain C++ stores only.
//
// THE SHARD FORM (ctd_kkt_schur_cr_shard_*).  A rank's T_r -- the principal submatrix of T on its blocks [sb, se) -- is the whole-grid
// problem of N_r = se - sb blocks seen through offset pointers: the launchers are given rowptr + sb m (its entries stay absolute
// indices into colind and jvals), sc + sb m, r + sb m and out + sb m, N_r in place of N, and px indexed by global column.  The last
// local block has no coupling, so T(se, se - 1) is dropped.  The same kernels run, instantiated a second time for argument structs
// with two more fields (the whole-grid instantiations keep their instructions): `first` = sb goes into word 4 of the header (0 on
// the whole grid, as that word has always been) and is checked by every launch of the shard's solve like N, m and n_levels; `part`
// says where the partial sums of r . x go (the whole grid: the workspace's own, [16, 16 + kSchurMaxWg)).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ctd_krylov_kernels.hpp"
#include "ctd_schur_kernels.hpp"
#include "ctd_schur_plan.hpp"

namespace ctd {

constexpr int64_t kSchurCrTag = 0x5343485243523031;      // "SCHRCR01"

struct SchurCrFactorParams {
    int64_t N, v_off;
    int32_t m, n_levels;
    const int64_t *rowptr, *colind;
    const double *jvals, *px, *sc;          // sc may be null
    double* ws;
};
// ... of a shard: `first`, the global index of block 0 (the shard's step_begin), goes into word 4 of the header
struct SchurCrShardFactorParams : SchurCrFactorParams {
    int64_t first;
};

// mode: SchurSolveMode of ctd_schur_kernels.hpp
struct SchurCrSolveParams {
    int64_t N;
    int32_t m, mode, n_levels, pad;
    double* ws;
    const double* r;
    double* out;
    const KrylovState* cur;
};
// ... of a shard: `first` as above, checked against the header; part: where the partial sums of r . x go (modes other than
// SCHUR_PLAIN)
struct SchurCrShardSolveParams : SchurCrSolveParams {
    int64_t first;
    double* part;
};

// Launchers (ctd_schur_cr.hip), enqueue-only on `st`
hipError_t schur_cr_factor(const SchurCrFactorParams& fp, hipStream_t st);
hipError_t schur_cr_solve(const SchurCrSolveParams& sp, hipStream_t st);       // modes other than SCHUR_PLAIN: the partial sums too
hipError_t schur_cr_factor(const SchurCrShardFactorParams& fp, hipStream_t st);
hipError_t schur_cr_solve(const SchurCrShardSolveParams& sp, hipStream_t st);

}  // namespace ctd
