// ctd_krylov_shard_kernels.hpp -- the shard form of the vector kernels of the device-resident MINRES solve
// (ctd_kkt_minres_shard_*, include/ctdirect_hip.h): ownership, send slots, workspace and the launchers.  The kernels are in
// ctd_krylov.hip beside the whole-grid ones.  The recurrences, the arithmetic of every expression, the cur / pend protocol of the
// state and the freeze are those of ctd_krylov_kernels.hpp; what differs is stated here.
//
// OWNERSHIP.  A rank's Krylov vectors are full-length (n = nvar + ncon entries, variables first).  The rank updates -- and stores to
// -- its OWNED entries only, in ascending global index (plan_krylov_shard, ctd_host.cpp):
//   [var_lo, var_hi)     the variables of its own steps (the last rank up to v_off),
//   [v_off, nvar)        the nv tail, replicated: every rank keeps and updates it with identical bits,
//   nvar + [r0, r1)      its own rows (the last rank also the tail rows).
// Position p of that compacted list maps to a global index through the three ranges (krylov_own_index): the ranges are kernel
// arguments, no index array exists.  The geometry is krylov_geom(n_own) over positions: workgroup b owns the positions
// [b chunk, (b + 1) chunk).  One shard of the whole grid: the list is 0 .. n - 1 and the geometry krylov_geom(n), every load,
// store and addition that of the whole-grid kernels.  In an inner product the tail terms are counted by the LAST rank only.
//
// SEND SLOT (kKrylovSlot doubles, the record a rank contributes to an all-gather).  One layout serves (A)'s one sum and (B)'s four:
//   [0, 4 kKrylovMaxWg)   the workgroups' partial sums, padded with +0.0: start and (A) write entry b for workgroup b (stride 1),
//                         (B) the entries 4 b .. 4 b + 3 (beta^2, z.z, z.u, u.u);
//   [kSlotTail, + 16)     (A): the rank's nv PARTIAL sums of the tail of kv, as ctd_kktprod_shard_dev_async left them;
//   [kSlotCount]          the number of workgroups that wrote partial sums, as a double.
// A rank has two send slots (A: start and (A); B: (B)) and two gathered areas of n_ranks slots each, rank-major, filled by the
// CALLER's all-gathers; with one rank the gathered areas ARE the send slots (krylov_shard_layout).  The library issues no collective.
//
// ORDER OF A CROSS-RANK SUM.  The reading kernel adds, in one running sum from 0.0: ranks 0 .. n_ranks - 1 ascending, within a rank
// the workgroups 0 .. count - 1 ascending (the padding is skipped by count).  Every thread of every workgroup of every rank does
// this redundantly: identical inputs in an identical order give identical scalars, decisions and KrylovState bytes on every rank.
// The sum has n_ranks x nwg terms (the cap of krylov_geom times the ranks): the known lever should it ever matter.
//
// THE TAIL OF K v.  kv's nv tail entries hold the rank's partial sums and are never completed in place.  (B) takes
// kv_tail[j] = the gathered partials of slot A added in rank order STARTING FROM RANK 0's VALUE (one rank: its own bits) wherever
// it needs kv at a tail entry.  alfa = v . y needs y = K v - .. at the tail before that value exists in (A): with more than one
// rank (A) leaves the tail terms out and (B) adds v_j y_j, j ascending, after the last rank's workgroups; with one rank kv is
// complete and (A) counts the tail terms where the whole-grid kernel does.  (A) keeps copies of the tail of v and r1 (kTailCopy)
// for that, because (B) overwrites r1 while other workgroups would read it.
//
// Per iteration: the two launches of kktprod_shard, (A), (B), (C), and three small all-gathers by the caller (the halo of v, slot A,
// slot B).  No all-reduce, no host synchronisation.
//
// THE SCHUR FORM (ctd_kkt_minres_schur_cr_shard_*): M = blkdiag(diag(1 / px), T_0^-1, .., T_{G-1}^-1, diag(1 / pc_tail)), T_r the rank's
// own block rows factored by ctd_kkt_schur_cr_shard_factor_dev_async (ctd_schur_cr_kernels.hpp).  Both send slots grow to
// kKrylovSchurSlot doubles: the slot above, then [kSlotSchur, + kSlotSchurMax) the partial sums of r2 . y over the rank's block rows,
// padded with +0.0, and [kSlotSchurCount] their number G_r = min(N_r, kSlotSchurMax).  The start's init kernel and (B) leave y and
// the terms of the inner product open on the rows [s_lo, s_hi) of the rank's blocks; the launches of the solve follow in the same
// phase, the last of which writes the G_r partial sums into the send slot (workgroup g: the local blocks g, g + G_r, ... in that
// order).  No gather is added: the partial sums travel in the slot.
// ORDER OF THE CROSS-RANK SUM of beta1^2 and beta^2 in the Schur form, one running sum from 0.0: first the terms above -- ranks
// ascending, within a rank the workgroups of the init kernel or of (B) ascending --, then the ranks ascending AGAIN, each rank's G_r
// partial sums of the solve in ascending workgroup order.  With one rank this is the order of the whole-grid (C) with the log-depth
// preconditioner.  The three other sums of (B), alfa and the tail of K v are as above.  (A) is the kernel above: it reads no slot.
#pragma once
#include "ctd_krylov_kernels.hpp"

namespace ctd {

constexpr int kKrylovTailMax = 16;                               // room for the nv tail entries in a slot
constexpr int kSlotTail = 4 * kKrylovMaxWg;                      // 2048
constexpr int kSlotCount = kSlotTail + kKrylovTailMax;           // 2064
constexpr int kKrylovSlot = kSlotCount + 16;                     // 2080 = CTD_KKT_MINRES_SHARD_SLOT
// the Schur form's slot: the slot above, the solve's partial sums, their count
constexpr int kSlotSchur = kKrylovSlot;                          // 2080
constexpr int kSlotSchurMax = 256;                               // = kSchurMaxWg (ctd_schur_kernels.hpp)
constexpr int kSlotSchurCount = kSlotSchur + kSlotSchurMax;      // 2336
constexpr int kKrylovSchurSlot = kSlotSchurCount + 16;           // 2352 = CTD_KKT_MINRES_SCHUR_SHARD_SLOT

// the joined form's slot (ctd_kkt_minres_schur_cr_joint_*): the slot above, then the rank's solve record of
// ctd_schur_cr_joint_kernels.hpp (kSchurJointSolveSlot = 16 + 3 * 64 doubles)
constexpr int kSlotJoint = kKrylovSchurSlot;                     // 2352
constexpr int kKrylovSchurJointSlot = kKrylovSchurSlot + 16 + 3 * 64;      // 2560 = CTD_KKT_MINRES_SCHUR_JOINT_SLOT

// what start records for begin and for (B): the handle keeps no per-solve state
struct KrylovShardMeta { double rtol; int64_t max_iter; int32_t precond, pad; };

// Offsets (doubles) into the caller's workspace: the eight vectors of n entries (r1, r2, y, v, kv, w, w2, minv), then the slots,
// then alfa, the tail copies, the meta block and the two states
struct KrylovShardLayout { int64_t v, kv, send_a, send_b, gathered_a, gathered_b, alfa, tail_copy, meta, cur, pend, total; };
inline KrylovShardLayout krylov_shard_layout(int64_t n, int64_t n_ranks, int64_t slot = kKrylovSlot) {
    KrylovShardLayout l{};
    l.v = 3 * n;
    l.kv = 4 * n;
    l.send_a = kKrylovVectors * n;
    l.send_b = l.send_a + slot;
    // one rank: nothing to gather, the kernels read the send slots
    l.gathered_a = n_ranks == 1 ? l.send_a : l.send_b + slot;
    l.gathered_b = n_ranks == 1 ? l.send_b : l.gathered_a + n_ranks * slot;
    l.alfa = n_ranks == 1 ? l.send_b + slot : l.gathered_b + n_ranks * slot;
    l.tail_copy = l.alfa + 16;
    l.meta = l.tail_copy + 2 * kKrylovTailMax;
    l.cur = l.meta + 16;
    l.pend = l.cur + 16;
    l.total = l.pend + 16;
    return l;
}
// CTD_KKT_MINRES_SHARD_WORKSPACE(n, n_ranks): an upper bound of krylov_shard_layout(n, n_ranks).total that is one formula
inline int64_t krylov_shard_workspace(int64_t n, int64_t n_ranks, int64_t slot = kKrylovSlot) {
    return kKrylovVectors * n + (2 + 2 * n_ranks) * slot + 96;
}

// the owned ranges as the kernels take them: positions [0, n_var) -> lo + p, [n_var, n_var + nv) -> v_off + .., then row0 + ..
struct KrylovOwn {
    int64_t lo, n_var, v_off, nv, row0;
    int32_t last, n_ranks;
};
__host__ __device__ __forceinline__ int64_t krylov_own_index(const KrylovOwn& o, int64_t p) {
    return p < o.n_var ? o.lo + p : (p < o.n_var + o.nv ? o.v_off + (p - o.n_var) : o.row0 + (p - o.n_var - o.nv));
}

// The kernels' arguments: a struct of its own (not KrylovParams: the shard kernels have no `part` and no `precond` -- the slots and
// the meta block take their place -- and the launch runs over n_own positions while the vectors are n entries apart)
struct KrylovShardParams {
    int64_t n_own, chunk;               // the positions of the compacted list; positions per workgroup
    int32_t nwg, pad;                   // krylov_geom(n_own)
    double *r1, *r2, *y, *v, *kv, *w, *w2, *minv;      // full-length vectors, global indexing
    double* z;                          // the caller's iterate
    double* alfa;                       // alfa of the iteration, stored by (B) for (C)
    KrylovState *cur, *pend;
    KrylovOwn own;
    double *send_a, *send_b;
    const double *gathered_a, *gathered_b;
    double* tail_copy;                  // v tail at [0, 16), r1 tail at [16, 32)
    KrylovShardMeta* meta;
};

// the workspace `ws` cut into the kernels' arguments; n: nvar + ncon, n_own: the rank's positions
inline KrylovShardParams krylov_shard_params(double* ws, int64_t n, int64_t n_own, const KrylovOwn& own, double* z,
                                             int64_t slot = kKrylovSlot) {
    KrylovShardParams sp{};
    const KrylovShardLayout l = krylov_shard_layout(n, own.n_ranks, slot);
    const KrylovGeom g = krylov_geom(n_own);
    sp.n_own = n_own; sp.chunk = g.chunk; sp.nwg = g.nwg;
    double** vec[] = {&sp.r1, &sp.r2, &sp.y, &sp.v, &sp.kv, &sp.w, &sp.w2, &sp.minv};
    for (int j = 0; j < kKrylovVectors; ++j) *vec[j] = ws + j * n;
    sp.z = z;
    sp.alfa = ws + l.alfa;
    sp.cur = (KrylovState*)(ws + l.cur);
    sp.pend = (KrylovState*)(ws + l.pend);
    sp.own = own;
    sp.send_a = ws + l.send_a; sp.send_b = ws + l.send_b;
    sp.gathered_a = ws + l.gathered_a; sp.gathered_b = ws + l.gathered_b;
    sp.tail_copy = ws + l.tail_copy;
    sp.meta = (KrylovShardMeta*)(ws + l.meta);
    static_assert(sizeof(KrylovShardMeta) <= 16 * sizeof(double), "the meta block has 16 doubles of the workspace");
    return sp;
}

// Launchers (ctd_krylov.hip), one launch each, enqueue-only on `st`.  start: the vectors on the owned entries, the meta block, the
// padding and the count of both send slots, the partial sums of beta1^2 into slot A; begin: beta1 from the gathered slots, v, both
// states; alfa / lanczos / update: (A), (B), (C)
hipError_t krylov_shard_start(const KrylovShardParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                              double rtol, int64_t max_iter, hipStream_t st);
hipError_t krylov_shard_begin(const KrylovShardParams& sp, hipStream_t st);
hipError_t krylov_shard_alfa(const KrylovShardParams& sp, hipStream_t st);
hipError_t krylov_shard_lanczos(const KrylovShardParams& sp, hipStream_t st);
hipError_t krylov_shard_update(const KrylovShardParams& sp, hipStream_t st);

// The Schur form: the arguments above cut with slots of kKrylovSchurSlot doubles, and the rows [s_lo, s_hi) of an n-vector that are
// the rank's block rows, s_nwg the number of partial sums its solve leaves.  New instantiations of the same kernels, one launch
// each; the caller enqueues the solve's launches behind start and behind lanczos, in the same phase.  (A) is krylov_shard_alfa
struct KrylovSchurShardParams : KrylovShardParams {
    int64_t s_lo, s_hi;
    int32_t s_nwg, s_pad;
};
hipError_t krylov_schur_shard_start(const KrylovSchurShardParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                                    double rtol, int64_t max_iter, hipStream_t st);
hipError_t krylov_schur_shard_begin(const KrylovSchurShardParams& sp, hipStream_t st);
hipError_t krylov_schur_shard_lanczos(const KrylovSchurShardParams& sp, hipStream_t st);
hipError_t krylov_schur_shard_update(const KrylovSchurShardParams& sp, hipStream_t st);

// THE JOINED FORM (ctd_kkt_minres_schur_cr_joint_*): M = blkdiag(diag(1 / px), T^-1, diag(1 / pc_tail)) with T^-1 applied by
// ctd_kkt_schur_cr_joint_* (ctd_schur_cr_joint_kernels.hpp).  The Schur form above on slots of kKrylovSchurJointSlot doubles: [s_lo,
// s_hi) are the rank's block rows, the separator's included; behind start's and (B)'s launch the caller enqueues the interior's
// solve, whose last launch writes the partial sums of r_I . g_r where the shard form's solve writes its own, and the record kernel,
// which writes the solve record at [kSlotJoint, kKrylovSchurJointSlot) of the same send slot: no gather is added.  begin and (C) are
// preceded, in the same phase, by the two join launches (the reduced solve from the gathered records, which leaves sigma = x_s . rs~
// at `sigma`; the correction of y on the rank's block rows).  ORDER OF beta1^2 AND beta^2: the running sum of the Schur form above --
// the own terms, ranks ascending; the partial sums of r_I . g_r, ranks ascending --, then + sigma, once, when n_ranks > 1.  With
// one rank there is no separator and sigma is not read: the order and the bits of the Schur form above.
struct KrylovSchurJointParams : KrylovSchurShardParams {
    const double* sigma;
};
hipError_t krylov_schur_joint_start(const KrylovSchurJointParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                                    double rtol, int64_t max_iter, hipStream_t st);
hipError_t krylov_schur_joint_begin(const KrylovSchurJointParams& sp, hipStream_t st);
hipError_t krylov_schur_joint_lanczos(const KrylovSchurJointParams& sp, hipStream_t st);
hipError_t krylov_schur_joint_update(const KrylovSchurJointParams& sp, hipStream_t st);

}  // namespace ctd
