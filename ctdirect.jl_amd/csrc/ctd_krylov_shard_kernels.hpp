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
#pragma once
#include "ctd_krylov_kernels.hpp"

namespace ctd {

constexpr int kKrylovTailMax = 16;                               // room for the nv tail entries in a slot
constexpr int kSlotTail = 4 * kKrylovMaxWg;                      // 2048
constexpr int kSlotCount = kSlotTail + kKrylovTailMax;           // 2064
constexpr int kKrylovSlot = kSlotCount + 16;                     // 2080 = CTD_KKT_MINRES_SHARD_SLOT

// what start records for begin and for (B): the handle keeps no per-solve state
struct KrylovShardMeta { double rtol; int64_t max_iter; int32_t precond, pad; };

// Offsets (doubles) into the caller's workspace: the eight vectors of n entries (r1, r2, y, v, kv, w, w2, minv), then the slots,
// then alfa, the tail copies, the meta block and the two states
struct KrylovShardLayout { int64_t v, kv, send_a, send_b, gathered_a, gathered_b, alfa, tail_copy, meta, cur, pend, total; };
inline KrylovShardLayout krylov_shard_layout(int64_t n, int64_t n_ranks) {
    KrylovShardLayout l{};
    l.v = 3 * n;
    l.kv = 4 * n;
    l.send_a = kKrylovVectors * n;
    l.send_b = l.send_a + kKrylovSlot;
    // one rank: nothing to gather, the kernels read the send slots
    l.gathered_a = n_ranks == 1 ? l.send_a : l.send_b + kKrylovSlot;
    l.gathered_b = n_ranks == 1 ? l.send_b : l.gathered_a + n_ranks * kKrylovSlot;
    l.alfa = n_ranks == 1 ? l.send_b + kKrylovSlot : l.gathered_b + n_ranks * kKrylovSlot;
    l.tail_copy = l.alfa + 16;
    l.meta = l.tail_copy + 2 * kKrylovTailMax;
    l.cur = l.meta + 16;
    l.pend = l.cur + 16;
    l.total = l.pend + 16;
    return l;
}
// CTD_KKT_MINRES_SHARD_WORKSPACE(n, n_ranks): an upper bound of krylov_shard_layout(n, n_ranks).total that is one formula
inline int64_t krylov_shard_workspace(int64_t n, int64_t n_ranks) { return kKrylovVectors * n + (2 + 2 * n_ranks) * kKrylovSlot + 96; }

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
inline KrylovShardParams krylov_shard_params(double* ws, int64_t n, int64_t n_own, const KrylovOwn& own, double* z) {
    KrylovShardParams sp{};
    const KrylovShardLayout l = krylov_shard_layout(n, own.n_ranks);
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

}  // namespace ctd
