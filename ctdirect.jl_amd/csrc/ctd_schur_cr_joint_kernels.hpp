// ctd_schur_cr_joint_kernels.hpp -- the joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*,
// include/ctdirect_hip.h): the shard form of ctd_schur_cr_kernels.hpp with the G - 1 couplings across the ranks restored by
// separator elimination.  Arguments, records, launchers and the order of every sum; the kernels are in ctd_schur_cr.hip beside the
// ones they reuse, under CTD_SCHUR_CR_JOINT, and are compiled as a translation unit of their own, ctd_schur_cr_joint.hip (strict
// rounding, plain stores, no atomics, kernel boundaries are the only synchronisation between workgroups).
// The host-side plan (separator, interior, offsets into the workspace, launch counts): ctd_schur_plan.hpp.
//
// PARTITION.  Rank r of G holds the steps [sb, se).  Its separator is s = sb (r > 0), its interior I = [a, se), a = sb + (r > 0), of
// n_int blocks, b = se - 1 the last of them.  A = T on I is the whole-grid problem of n_int blocks through offset pointers, factored
// and applied by the kernels of ctd_schur_cr_kernels.hpp in a third instantiation (argument structs SchurCrJoint*Params): the same
// instructions but for the header, which carries this family's tag and in the words 4 .. 8 a, sb, se, G and r.  Every launch of this
// family checks all of them (and in SCHUR_ITER mode the freeze) and stores nothing on a mismatch.  Slots as there: E[k] = T(k + 1, k).
//
// LOCAL FACTOR (factor_local), launches in this order
//   INTERFACE  one thread per entry of D_s = T(s, s), E[s] = T(a, s) (both r > 0) and E[b] = T(se, b) (r < G - 1), by the expression
//              of the assemble launch of ctd_schur_cr_kernels.hpp in its order (the merge of the two rows' columns ascending, s +=
//              (J(ra, c) J(rb, c)) (1.0 / px(c)), then + sc on the diagonal); 0.0 where the rank has none.  E[b] reads the rows of
//              block se: the next rank's.  The same launch zeroes the rest of the workspace behind the interior's part.
//   the factor of A: 2 n_levels + 2 launches of ctd_schur_cr_kernels.hpp.
//   SPIKES     Wl = A^-1 (e_a E[s]) (r > 0), Wr = A^-1 (e_b E[b]') (r < G - 1), n_int m x m each: the DOWN / ROOT / UP chain of
//              ctd_schur_cr_kernels.hpp, 2 n_levels + 1 launches, with the column as the second grid dimension -- one wave per
//              (block, column), all (up to) 2 m columns in one chain, not batched.  Column c < m is column c of Wl, its right-hand
//              side E[s](:, c) in block a and 0.0 elsewhere; column m + c is column c of Wr, its right-hand side E[b](c, :)' in block
//              b.  A wave does what the wave of the single solve does, in its order: a column carries the bits of
//              ctd_kkt_schur_cr_shard_solve_dev_async on the steps I with that right-hand side.  Scratch: a running right-hand side
//              and a y of n_int m entries per column, 4 n_int m^2 doubles.
//   CONTRIBUTIONS  one thread per entry, p ascending from 0.0:
//              Cll(i, j) = sum_p E[s](p, i) Wl[a](p, j);   Crl(i, j) = sum_p E[b](i, p) Wl[b](p, j);   Crr(i, j) = sum_p E[b](i, p)
//              Wr[b](p, j), and THE FACTOR RECORD into the send slot: four 64-bit integers sb, se, m, r, twelve zero words, then D_s,
//              Cll, Crl, Crr (m^2 each, row-major): kSchurJointHead + 4 m^2 doubles.
// The caller gathers the G records (rank order).  JOIN (factor_join), one launch, one wave, the same on every rank:
//   block k = r - 1 of the reduced matrix, r = 1 .. G - 1:  S(k, k) = (D_s^(r) - Crr^(r-1)) - Cll^(r) (the left neighbour's term
//   first), S(k + 1, k) = -Crl^(r); then the block Cholesky sweep of ctd_schur_kernels.hpp, k ascending: A = S(k, k) - F_{k-1}
//   F_{k-1}' (lower triangle; sum over j ascending from 0.0, then one subtraction), L_k L_k' = A column by column as there, F_k =
//   S(k + 1, k) L_k^-T row by row as there.  A pivot that is not positive or not finite: the separator's global block index goes into
//   the status word of block k and of every later block (-1 before it), whose L and F are NaN.  Records that are not an ascending
//   cover of [0, N) by G ranks of block size m, or whose record r does not carry this rank's own steps, fill every block with NaN
//   and set every status word to 0.
//
// LOCAL SOLVE (solve_local): g = A^-1 r_I into out on the interior rows (2 n_levels + 1 launches of ctd_schur_cr_kernels.hpp), then
//   THE SOLVE RECORD, one wave: one 64-bit integer r, fifteen zero words, then three vectors 64 doubles apart: r_s (the rows of s),
//   qu(j) = sum_p E[s](p, j) g_a(p), qd(i) = sum_p E[b](i, p) g_b(p), p ascending from 0.0; 0.0 where the rank has none and behind m.
// The caller gathers the G records.  JOIN (solve_join), two launches:
//   REDUCED SOLVE, one wave, the same on every rank: rs~_k = (r_s^(r) - qd^(r-1)) - qu^(r), k = r - 1; forward t_k = L_k^-1 (rs~_k -
//   F_{k-1} t_{k-1}), backward x_k = L_k^-T (t_k - F_k' x_{k+1}), with the triangular solves and the products of
//   ctd_schur_cr_kernels.hpp (j ascending from 0.0, one subtraction); sigma = sum_k sum_a x_k(a) rs~_k(a), one running sum from 0.0,
//   k ascending, rows ascending.  rs~, x and sigma stay in the workspace.
//   CORRECTION, one thread per row of the rank's blocks: out_s = x_{r-1} on the separator; on the interior row (k, i)
//   out = (g - s1) - s2,  s1 = sum_j Wl[k](i, j) x_{r-1}(j) (r > 0),  s2 = sum_j Wr[k](i, j) x_r(j) (r < G - 1), j ascending from
//   0.0.  A thread reads its row of Wl[k] and Wr[k]: m consecutive doubles.  Rows are 8-byte aligned only when m is odd, so the loads
//   are single doubles for every m; the launch streams 2 n_int m^2 doubles once.
// One rank: no separator, no interface launch, no record, no join launch; factor_local and solve_local are the interior's alone,
// which is the whole grid: the launches and the bits of the shard form on the same steps.  The workspace behind the interior's part
// is then neither written nor read.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ctd_schur_cr_kernels.hpp"

namespace ctd {

constexpr int64_t kSchurCrJointTag = 0x5343484A4E543031;      // "SCHJNT01"

// what the header carries behind the words of the shard form
struct SchurCrJointId {
    int64_t sb, se;
    int32_t n_ranks, rank;
};
// the interior's factor and solve: the shard form's arguments (first = a) and the identity
struct SchurCrJointFactorParams : SchurCrShardFactorParams {
    SchurCrJointId id;
};
struct SchurCrJointSolveParams : SchurCrShardSolveParams {
    SchurCrJointId id;
};

// the kernels of this family proper.  rowptr, colind, jvals, px, sc, r, out: the grid's, not offset.  off_*: SchurCrJointPlan
struct SchurCrJointParams {
    int64_t N, n_int, v_off, int_begin;
    SchurCrJointId id;
    int32_t m, n_levels, mode, pad;
    const int64_t *rowptr, *colind;
    const double *jvals, *px, *sc;          // sc may be null
    double* ws;
    int64_t off_es, off_eb, off_ds, off_wl, off_wr, off_scratch, off_reduced, off_rs, off_xs, off_sigma, workspace;
    double* send;                           // factor_local, solve_local: the record
    const double* gathered;                 // the joins: n_ranks records, `slot` doubles apart
    int64_t slot;
    const double* r;
    double* out;
    const KrylovState* cur;                 // mode SCHUR_ITER: the freeze
};

// Launchers (ctd_schur_cr_joint.hip), enqueue-only on `st`
hipError_t schur_cr_factor(const SchurCrJointFactorParams& fp, hipStream_t st);
hipError_t schur_cr_solve(const SchurCrJointSolveParams& sp, hipStream_t st);
hipError_t schur_cr_joint_interface(const SchurCrJointParams& p, hipStream_t st);
hipError_t schur_cr_joint_spikes(const SchurCrJointParams& p, hipStream_t st);         // ... and the contributions, the record
hipError_t schur_cr_joint_factor_join(const SchurCrJointParams& p, hipStream_t st);
hipError_t schur_cr_joint_solve_record(const SchurCrJointParams& p, hipStream_t st);
hipError_t schur_cr_joint_solve_join(const SchurCrJointParams& p, hipStream_t st);

}  // namespace ctd
