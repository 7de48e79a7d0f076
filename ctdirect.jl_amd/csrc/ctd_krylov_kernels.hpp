// ctd_krylov_kernels.hpp -- the vector kernels of the device-resident preconditioned MINRES solve of K z = r (ctd_kkt_minres*,
// include/ctdirect_hip.h): geometry, state and the launchers.  The kernels themselves are in ctd_krylov.hip; they do not depend on
// the OCP, so they are compiled once into the library (registry and run-time OCPs are served alike, there is no hiprtc family).
//
// THE RECURRENCES are those of scipy.sparse.linalg.minres (Paige & Saunders): the same variables, the same initialisation, z0 = 0,
// every expression evaluated in scipy's order of operations under strict rounding (-ffp-contract=off), M = diag(1 / px, 1 / pc)
// applied as a product with the reciprocals (formed once, by the start).  One iteration, with v the Lanczos vector the operator is
// applied to (K v: ctd_kktprod's two launches, unchanged) and `done` the iterations completed before it:
//   (A) krylov_alfa_kernel    y = K v - (beta / oldb) r1  (done >= 1), the workgroups' partial sums of alfa = v . y.  Nothing but the
//                             partial sums is stored: (B) forms y again, the same bits.
//   (B) krylov_lanczos_kernel alfa from the partial sums; y -= (alfa / beta) r2; r1 = r2; r2 = y; y = M r2; with delta = cs dbar +
//                             sn alfa (the previous rotation) the direction u = v - oldeps w2 - delta w that (C) scales into the new
//                             w; the partial sums of beta^2 = r2 . y and of z . z, z . u, u . u.
//   (C) krylov_update_kernel  beta^2 and the three other sums from the partial sums, then the scalar recurrences (rotation, norms,
//                             stopping tests), redundantly in every thread of every workgroup: identical inputs in an identical
//                             order give identical decisions.  w2 = w; w = u / gamma; z += phi w; v = y / beta for the next
//                             operator call; one lane stores the state.
// |z| after the update -- scipy's ynorm = norm(x), a third inner product that would depend on (C)'s own update -- is taken as
// sqrt(z.z + 2 a z.u + a^2 u.u), a = phi / gamma, from sums over the vectors BEFORE the update: it only enters the stopping test
// test1, no iterate.
//
// SUMMATION ORDER (part of the contract: results are reproducible bit for bit; no floating-point atomics).  The geometry is a
// function of n = nvar + ncon alone (krylov_geom): nwg = min(kKrylovMaxWg, ceil(n / kKrylovSpan)) workgroups of 256 threads,
// workgroup b owns the elements [b chunk, min(n, (b + 1) chunk)), chunk = ceil(n / nwg) rounded up to a multiple of 256.  Every
// inner product is
//   1. per thread t of workgroup b: the terms of elements b chunk + t, + 256, + 512, ... added in that order starting from 0.0;
//   2. per wave, the shuffle tree of ctd_common.hpp (off = 32, 16, ..., 1); per workgroup, thread 0 adds the four waves' sums in
//      wave order starting from 0.0 (block_partial_sums) and writes the workgroup's partial sum;
//   3. in the next kernel every thread adds the partial sums of workgroups 0, 1, ..., nwg - 1 in that order starting from 0.0.
//
// STATE.  Two copies of KrylovState: `pend` is written by one lane of (C) -- and read by no workgroup of (C) --, `cur` is what (B)
// and (C) read.  (A) reads `pend` only, and its first lane commits it into `cur` when the two differ (no workgroup reads `cur` in
// (A)).  A kernel therefore never reads what a lane of the same launch writes, and no launch ordinal is baked into the arguments:
// a captured graph of iterations replays after any number of others.
//
// FREEZE.  Once the status is set (converged, breakdown, iteration cap) every kernel of every later iteration returns before any
// store to a vector, a partial sum or the pending state; the test is on a value every thread reads from the same word, so the exit
// is uniform.  The one store left is (A)'s commit of the pending state in the first frozen iteration, which is how (B) and (C)
// learn of the status.  The kktprod launches in between still run; their output (kv) is not consumed.  Breakdown: beta^2 negative
// or not finite (M not positive definite, or a NaN): no vector is touched by that iteration's (C), z stays the last iterate;
// beta^2 == 0 exactly after an iteration that did not converge (the Krylov space is exhausted): the iterate is updated first.
//
// Kernel boundaries are the only synchronisation between workgroups; plain C++ stores only.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ctd {

constexpr int kKrylovBlock = 256;       // threads per workgroup
constexpr int kKrylovSpan = 1024;       // elements per workgroup before the workgroup count is capped
constexpr int kKrylovMaxWg = 512;       // cap of the workgroup count (the length of the serial sum of step 3): two per compute unit
constexpr int kKrylovSums = 5;          // partial sums per workgroup: alfa, beta^2, z.z, z.u, u.u
constexpr int kKrylovVectors = 8;       // r1, r2, y, v, kv, w, w2, minv
// doubles of the workspace (CTD_KKT_MINRES_WORKSPACE of include/ctdirect_hip.h): the vectors, then the 512 partial sums of alfa (the
// start: of beta1^2) at 0, 512 rows of (B)'s four partial sums at 512, alfa at 2560, the two states at 2592 and 2608
constexpr int64_t kKrylovFixed = 3072;
inline int64_t krylov_workspace(int64_t n) { return kKrylovVectors * n + kKrylovFixed; }

enum KrylovStatus : int32_t { KRYLOV_RUNNING = 0, KRYLOV_CONVERGED = 1, KRYLOV_MAX_ITER = 2, KRYLOV_BREAKDOWN = 3 };

// scipy's names; itn: iterations done
struct KrylovState {
    double oldb, beta, dbar, epsln, phibar, cs, sn, tnorm2, ynorm, Anorm, beta1, rtol;
    int64_t itn, max_iter;
    int32_t status, pad;
};
static_assert(sizeof(KrylovState) <= 16 * sizeof(double), "a KrylovState has 16 doubles of the workspace");

struct KrylovGeom { int32_t nwg; int64_t chunk; };
inline KrylovGeom krylov_geom(int64_t n) {
    int64_t nwg = (n + kKrylovSpan - 1) / kKrylovSpan;
    nwg = nwg < 1 ? 1 : (nwg > kKrylovMaxWg ? kKrylovMaxWg : nwg);
    int64_t chunk = (n + nwg - 1) / nwg;
    chunk = (chunk + kKrylovBlock - 1) / kKrylovBlock * kKrylovBlock;
    return {(int32_t)nwg, chunk > 0 ? chunk : kKrylovBlock};
}

struct KrylovParams {
    int64_t n, chunk;
    int32_t nwg, precond;               // precond: y = minv o r2 (otherwise y = r2, scipy's identity)
    double *r1, *r2, *y, *v, *kv, *w, *w2, *minv;
    double* z;                          // the caller's iterate
    double* part;                       // kKrylovSums x kKrylovMaxWg partial sums
    double* alfa;                       // alfa of the iteration, stored by (B) for (C)
    KrylovState *cur, *pend;
    // the SCHUR instantiations only (ctd_schur_kernels.hpp): the block rows [s_lo, s_hi) of an n-vector, whose y the solve launch
    // writes, and its s_nwg partial sums of r2 . y
    int64_t s_lo, s_hi;
    const double* s_part;
    int32_t s_nwg;
};

// the workspace `ws` (krylov_workspace(n) doubles) cut into the kernels' arguments
inline KrylovParams krylov_params(double* ws, int64_t n, double* z, bool precond) {
    KrylovParams kp{};
    const KrylovGeom g = krylov_geom(n);
    kp.n = n; kp.chunk = g.chunk; kp.nwg = g.nwg; kp.precond = precond ? 1 : 0;
    double** vec[] = {&kp.r1, &kp.r2, &kp.y, &kp.v, &kp.kv, &kp.w, &kp.w2, &kp.minv};
    for (int j = 0; j < kKrylovVectors; ++j) *vec[j] = ws + j * n;
    double* fixed = ws + kKrylovVectors * n;
    kp.z = z;
    kp.part = fixed;
    kp.alfa = fixed + kKrylovSums * kKrylovMaxWg;
    kp.cur = (KrylovState*)(fixed + kKrylovSums * kKrylovMaxWg + 32);
    kp.pend = (KrylovState*)(fixed + kKrylovSums * kKrylovMaxWg + 48);
    static_assert(kKrylovSums * kKrylovMaxWg + 64 <= kKrylovFixed, "the fixed part of the workspace");
    return kp;
}

// Launchers (ctd_krylov.hip), enqueue-only on `st`.  krylov_start: two launches -- z = w = w2 = 0, r1 = r2 = rhs, minv = 1 / (px, pc),
// y = M rhs, beta1^2 = rhs . y; then v = y / beta1 and both states.  px, pc: nvar and n - nvar entries, or both null.
// krylov_alfa: (A), after the operator wrote kv = K v; krylov_step: (B) and (C).
hipError_t krylov_start(const KrylovParams& kp, const double* rhs, const double* px, const double* pc, int64_t nvar, double rtol,
                        int64_t max_iter, hipStream_t st);
hipError_t krylov_alfa(const KrylovParams& kp, hipStream_t st);
hipError_t krylov_step(const KrylovParams& kp, hipStream_t st);
// The same with the block-tridiagonal Schur preconditioner (kp.s_*): SCHUR instantiations of the same kernels, in which y = M r2
// and its term of the inner product are left to the solve launch on the block rows, and the kernel that adds the partial sums of
// beta^2 (beta1^2) adds the solve's after (B)'s (the init kernel's), in ascending workgroup order.  The caller enqueues the solve
// launch between krylov_schur_init and krylov_schur_first, and between krylov_schur_lanczos (B) and krylov_schur_update (C)
hipError_t krylov_schur_init(const KrylovParams& kp, const double* rhs, const double* px, const double* pc, int64_t nvar, hipStream_t st);
hipError_t krylov_schur_first(const KrylovParams& kp, double rtol, int64_t max_iter, hipStream_t st);
hipError_t krylov_schur_lanczos(const KrylovParams& kp, hipStream_t st);
hipError_t krylov_schur_update(const KrylovParams& kp, hipStream_t st);

}  // namespace ctd
