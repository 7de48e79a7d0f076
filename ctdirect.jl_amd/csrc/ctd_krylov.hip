// ctd_krylov.hip -- the vector kernels of the device-resident MINRES solve (ctd_kkt_minres*) and their launchers.  The recurrences,
// the launch cut, the summation order, the two copies of the state and the freeze are specified in ctd_krylov_kernels.hpp.
// Strict rounding like the products (the Makefile compiles this file with -ffp-contract=off): every expression below rounds as
// the NumPy expression of scipy.sparse.linalg.minres it transcribes.
#include <cfloat>
#include <type_traits>

#include "ctd_common.hpp"
#include "ctd_krylov_kernels.hpp"
#include "ctd_krylov_shard_kernels.hpp"

namespace ctd {
namespace {

constexpr int kWaves = kKrylovBlock / 64;
constexpr int kPartB = kKrylovMaxWg;      // offset of (B)'s rows of four partial sums; [0, kKrylovMaxWg): alfa (the start: beta1^2)

// step 3 of the summation order: every thread adds the workgroups' partial sums in ascending order from 0.0
__device__ __forceinline__ double ordered_sum(const double* part, int nwg, int stride) {
    double s = 0.0;
#pragma unroll 16
    for (int b = 0; b < nwg; ++b) s += part[(int64_t)b * stride];      // (unrolled: the loads of 16 partial sums are issued together)
    return s;
}
__device__ __forceinline__ bool first_lane() { return blockIdx.x == 0 && threadIdx.x == 0; }
__device__ __forceinline__ bool bad_beta2(double b2) { return !(b2 >= 0.0) || !__builtin_isfinite(b2); }

// start, first launch: the vectors and the partial sums of beta1^2 = rhs . M rhs
// SCHUR (every kernel below that has it): the instantiation for the block-tridiagonal Schur preconditioner; false compiles to the
// code without it
template <bool SCHUR>
__global__ void __launch_bounds__(kKrylovBlock) krylov_init_kernel(const KrylovParams kp, const double* rhs, const double* px,
                                                                   const double* pc, const int64_t nvar) {
    __shared__ double wsum[kWaves];
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n ? lo + kp.chunk : kp.n;
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kKrylovBlock) {
        const double r = rhs[i];
        double yv = r;
        if (kp.precond) {
            const double m = 1.0 / (i < nvar ? px[i] : pc[i - nvar]);
            kp.minv[i] = m;
            yv = m * r;
        }
        const bool solved = SCHUR && i >= kp.s_lo && i < kp.s_hi;        // y and its term: the solve launch's
        kp.r1[i] = r;
        kp.r2[i] = r;
        if (!solved) kp.y[i] = yv;
        kp.v[i] = 0.0;
        kp.kv[i] = 0.0;
        kp.w[i] = 0.0;
        kp.w2[i] = 0.0;
        kp.z[i] = 0.0;
        if (!solved) acc += r * yv;
    }
    block_partial_sums<1, 1>(&acc, wsum, kp.part + blockIdx.x);
}

// start, second launch: beta1, the first Lanczos vector v = y / beta1, both copies of the state
template <bool SCHUR>
__global__ void __launch_bounds__(kKrylovBlock) krylov_first_kernel(const KrylovParams kp, const double rtol, const int64_t max_iter) {
    double b2 = ordered_sum(kp.part, kp.nwg, 1);
    if (SCHUR)
        for (int b = 0; b < kp.s_nwg; ++b) b2 += kp.s_part[b];
    KrylovState t{};
    t.cs = -1.0;
    t.rtol = rtol;
    t.max_iter = max_iter;
    if (bad_beta2(b2)) t.status = KRYLOV_BREAKDOWN;             // M is not positive definite, or a NaN in rhs / px / pc
    else if (b2 == 0.0) t.status = KRYLOV_CONVERGED;            // rhs = 0: z = 0 is the solution
    else {
        t.beta1 = sqrt(b2);
        t.beta = t.phibar = t.beta1;
        const double s = 1.0 / t.beta1;
        const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n ? lo + kp.chunk : kp.n;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kKrylovBlock) kp.v[i] = s * kp.y[i];
    }
    if (first_lane()) {
        *kp.cur = t;
        *kp.pend = t;
    }
}

// y = K v - (beta / oldb) r1 of one element (the second term from the second iteration on), as (A) and (B) both form it
__device__ __forceinline__ double lanczos_y(double kv, double r1, bool ortho, double c1) { return ortho ? kv - c1 * r1 : kv; }

// The element loops: the vectors are distinct regions of the workspace, and z is the caller's buffer, refused when it is an input:
// the local pointers are __restrict__, so the loads of the next elements are issued ahead of the stores of this one (the loops are
// latency-bound otherwise); four elements per thread in flight.  The order of every thread's additions is the loop's.
#define CTD_KRYLOV_UNROLL _Pragma("unroll 4")

// (A)
__global__ void __launch_bounds__(kKrylovBlock) krylov_alfa_kernel(const KrylovParams kp) {
    __shared__ double wsum[kWaves];
    const int32_t status = kp.pend->status;
    const int64_t itn = kp.pend->itn;
    // the commit: no workgroup reads `cur` in this kernel
    if (first_lane() && (kp.cur->itn != itn || kp.cur->status != status)) {
        static_assert(sizeof(KrylovState) % sizeof(uint64_t) == 0, "copied word by word");
        const uint64_t* src = (const uint64_t*)kp.pend;
        uint64_t* dst = (uint64_t*)kp.cur;
        for (int j = 0; j < (int)(sizeof(KrylovState) / sizeof(uint64_t)); ++j) dst[j] = src[j];
    }
    if (status != KRYLOV_RUNNING) return;
    const bool ortho = itn >= 1;
    const double c1 = ortho ? kp.pend->beta / kp.pend->oldb : 0.0;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n ? lo + kp.chunk : kp.n;
    const double* __restrict__ v = kp.v;
    const double* __restrict__ kv = kp.kv;
    const double* __restrict__ r1 = kp.r1;
    double acc = 0.0;
    CTD_KRYLOV_UNROLL
    for (int64_t i = lo + threadIdx.x; i < hi; i += kKrylovBlock) acc += v[i] * lanczos_y(kv[i], r1[i], ortho, c1);
    block_partial_sums<1, 1>(&acc, wsum, kp.part + blockIdx.x);
}

// (B)
template <bool SCHUR>
__global__ void __launch_bounds__(kKrylovBlock) krylov_lanczos_kernel(const KrylovParams kp) {
    __shared__ double wsum[kWaves * 4];
    const KrylovState s = *kp.cur;
    if (s.status != KRYLOV_RUNNING) return;
    const double alfa = ordered_sum(kp.part, kp.nwg, 1);
    if (first_lane()) *kp.alfa = alfa;
    const bool ortho = s.itn >= 1;
    const double c1 = ortho ? s.beta / s.oldb : 0.0, c2 = alfa / s.beta;
    const double oldeps = s.epsln, delta = s.cs * s.dbar + s.sn * alfa;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n ? lo + kp.chunk : kp.n;
    double* __restrict__ r1 = kp.r1;
    double* __restrict__ r2 = kp.r2;
    double* __restrict__ y = kp.y;
    const double* __restrict__ kv = kp.kv;
    const double* __restrict__ minv = kp.minv;
    const double* __restrict__ z = kp.z;
    const double* __restrict__ v = kp.v;
    const double* __restrict__ w = kp.w;
    const double* __restrict__ w2 = kp.w2;
    const bool precond = kp.precond != 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    CTD_KRYLOV_UNROLL
    for (int64_t i = lo + threadIdx.x; i < hi; i += kKrylovBlock) {
        const double r2v = r2[i];
        const double yv = lanczos_y(kv[i], r1[i], ortho, c1) - c2 * r2v;
        r1[i] = r2v;
        r2[i] = yv;
        const double my = precond ? minv[i] * yv : yv;
        const bool solved = SCHUR && i >= kp.s_lo && i < kp.s_hi;
        if (!solved) y[i] = my;
        const double zv = z[i], u = (v[i] - oldeps * w2[i]) - delta * w[i];
        if (!solved) acc[0] += yv * my;
        acc[1] += zv * zv;
        acc[2] += zv * u;
        acc[3] += u * u;
    }
    block_partial_sums<4, 4>(acc, wsum, kp.part + kPartB + (int64_t)blockIdx.x * 4);
}

// (C)
template <bool SCHUR>
__global__ void __launch_bounds__(kKrylovBlock) krylov_update_kernel(const KrylovParams kp) {
    const KrylovState s = *kp.cur;
    if (s.status != KRYLOV_RUNNING) return;
    double b2 = 0.0, zz = 0.0, zu = 0.0, uu = 0.0;
#pragma unroll 8
    for (int b = 0; b < kp.nwg; ++b) {
        const double* p = kp.part + kPartB + (int64_t)b * 4;
        b2 += p[0];
        zz += p[1];
        zu += p[2];
        uu += p[3];
    }
    if (SCHUR) {
#pragma unroll 8
        for (int b = 0; b < kp.s_nwg; ++b) b2 += kp.s_part[b];
    }
    const double alfa = *kp.alfa;
    KrylovState t = s;
    if (bad_beta2(b2)) {
        t.status = KRYLOV_BREAKDOWN;
        if (first_lane()) *kp.pend = t;
        return;
    }
    const double eps = DBL_EPSILON;
    t.oldb = s.beta;
    t.beta = sqrt(b2);
    t.tnorm2 = s.tnorm2 + ((alfa * alfa + t.oldb * t.oldb) + t.beta * t.beta);
    // the previous rotation
    const double oldeps = s.epsln;
    const double delta = s.cs * s.dbar + s.sn * alfa;
    const double gbar = s.sn * s.dbar - s.cs * alfa;
    t.epsln = s.sn * t.beta;
    t.dbar = -s.cs * t.beta;
    const double root = sqrt(gbar * gbar + t.dbar * t.dbar);
    // the next one
    double gamma = sqrt(gbar * gbar + t.beta * t.beta);
    gamma = gamma > eps ? gamma : eps;
    t.cs = gbar / gamma;
    t.sn = t.beta / gamma;
    const double phi = t.cs * s.phibar;
    t.phibar = t.sn * s.phibar;
    const double denom = 1.0 / gamma;
    // norms and the stopping tests
    const double a = phi * denom, y2 = zz + 2.0 * a * zu + a * a * uu;
    t.Anorm = sqrt(t.tnorm2);
    t.ynorm = y2 > 0.0 ? sqrt(y2) : 0.0;
    const double inf = __builtin_huge_val();
    const double test1 = (t.ynorm == 0.0 || t.Anorm == 0.0) ? inf : t.phibar / (t.Anorm * t.ynorm);
    const double test2 = t.Anorm == 0.0 ? inf : root / t.Anorm;
    t.itn = s.itn + 1;
    if (test2 <= s.rtol || test1 <= s.rtol) t.status = KRYLOV_CONVERGED;
    else if (t.itn >= s.max_iter) t.status = KRYLOV_MAX_ITER;
    else if (t.beta == 0.0) t.status = KRYLOV_BREAKDOWN;
    const bool go_on = t.status == KRYLOV_RUNNING;
    const double sinv = go_on ? 1.0 / t.beta : 0.0;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n ? lo + kp.chunk : kp.n;
    double* __restrict__ v = kp.v;
    double* __restrict__ w = kp.w;
    double* __restrict__ w2 = kp.w2;
    double* __restrict__ z = kp.z;
    const double* __restrict__ y = kp.y;
    CTD_KRYLOV_UNROLL
    for (int64_t i = lo + threadIdx.x; i < hi; i += kKrylovBlock) {
        const double wv = w[i];
        const double wn = ((v[i] - oldeps * w2[i]) - delta * wv) * denom;
        w2[i] = wv;
        w[i] = wn;
        z[i] = z[i] + phi * wn;
        if (go_on) v[i] = sinv * y[i];
    }
    if (first_lane()) *kp.pend = t;
}

}  // namespace

hipError_t krylov_start(const KrylovParams& kp, const double* rhs, const double* px, const double* pc, int64_t nvar, double rtol,
                        int64_t max_iter, hipStream_t st) {
    hipLaunchKernelGGL(krylov_init_kernel<false>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rhs, px, pc, nvar);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(krylov_first_kernel<false>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rtol, max_iter);
    return hipGetLastError();
}

hipError_t krylov_alfa(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_alfa_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}

hipError_t krylov_step(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_lanczos_kernel<false>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(krylov_update_kernel<false>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}

hipError_t krylov_schur_init(const KrylovParams& kp, const double* rhs, const double* px, const double* pc, int64_t nvar, hipStream_t st) {
    hipLaunchKernelGGL(krylov_init_kernel<true>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rhs, px, pc, nvar);
    return hipGetLastError();
}
hipError_t krylov_schur_first(const KrylovParams& kp, double rtol, int64_t max_iter, hipStream_t st) {
    hipLaunchKernelGGL(krylov_first_kernel<true>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rtol, max_iter);
    return hipGetLastError();
}
hipError_t krylov_schur_lanczos(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_lanczos_kernel<true>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}
hipError_t krylov_schur_update(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_update_kernel<true>, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}

// ---- the shard form (ctd_krylov_shard_kernels.hpp): the same expressions over the rank's owned entries; every cross-rank sum is
// read from the gathered send slots in rank order ---------------------------------------------------------------------------------
namespace {

// the number of workgroups that wrote a slot; anything else than a count (a slot nobody filled) reads as none
__device__ __forceinline__ int slot_count(const double* slot) {
    const double c = slot[kSlotCount];
    return c >= 0.0 && c <= (double)kKrylovMaxWg ? (int)c : 0;
}
// P (here and in the kernels below): the kernels' arguments, KrylovShardParams or, for the Schur form (ctd_krylov_shard_kernels.hpp),
// KrylovSchurShardParams -- slots of kKrylovSchurSlot doubles, y and its term of the inner product left to the solve's launches on the
// rows [s_lo, s_hi).  The instantiations for KrylovShardParams compile to the code without it
template <class P> constexpr bool is_joint() { return std::is_same<P, KrylovSchurJointParams>::value; }      // (the joined form)
template <class P> constexpr bool is_schur() { return std::is_same<P, KrylovSchurShardParams>::value || is_joint<P>(); }
template <class P> constexpr int slot_len() { return is_joint<P>() ? kKrylovSchurJointSlot : (is_schur<P>() ? kKrylovSchurSlot : kKrylovSlot); }
// one running sum from 0.0: ranks ascending, within a rank the workgroups ascending; entry j of rows `stride` doubles apart; SLOT:
// the doubles of a slot
template <int SLOT> __device__ __forceinline__ double gathered_sum(const double* g, int n_ranks, int stride, int j) {
    double s = 0.0;
    for (int r = 0; r < n_ranks; ++r) {
        const double* slot = g + (int64_t)r * SLOT;
        const int cnt = slot_count(slot);
#pragma unroll 16
        for (int b = 0; b < cnt; ++b) s += slot[b * stride + j];
    }
    return s;
}
// the Schur form: the solves' partial sums of r2 . y added to the running sum s, ranks ascending, within a rank ascending
template <int SLOT> __device__ __forceinline__ double gathered_schur_sum(double s, const double* g, int n_ranks) {
    for (int r = 0; r < n_ranks; ++r) {
        const double* slot = g + (int64_t)r * SLOT;
        const double c = slot[kSlotSchurCount];
        const int cnt = c >= 0.0 && c <= (double)kSlotSchurMax ? (int)c : 0;
#pragma unroll 8
        for (int b = 0; b < cnt; ++b) s += slot[kSlotSchur + b];
    }
    return s;
}
// kv at tail entry j: the ranks' partial sums in rank order, starting from rank 0's value
template <int SLOT> __device__ __forceinline__ double gathered_kv_tail(const double* g, int n_ranks, int j) {
    double s = g[kSlotTail + j];
    for (int r = 1; r < n_ranks; ++r) s += g[(int64_t)r * SLOT + kSlotTail + j];
    return s;
}
__device__ __forceinline__ bool own_tail(const KrylovOwn& o, int64_t p) { return p >= o.n_var && p < o.n_var + o.nv; }

// start: the vectors on the owned entries, the meta block, the padding and the counts of both send slots, the partial sums of
// beta1^2 = rhs . M rhs (the tail terms on the last rank only) into slot A
template <class P>
__global__ void __launch_bounds__(kKrylovBlock) krylov_shard_init_kernel(const P sp, const double* rhs, const double* px,
                                                                         const double* pc, const int64_t nvar, const double rtol,
                                                                         const int64_t max_iter) {
    __shared__ double wsum[kWaves];
    const P& kp = sp;
    const bool precond = px != nullptr;
    if (blockIdx.x == 0) {
        for (int e = threadIdx.x; e < kKrylovSlot; e += kKrylovBlock) {
            const double c = e == kSlotCount ? (double)kp.nwg : 0.0;
            if (e >= kp.nwg) sp.send_a[e] = c;          // (the entries [0, nwg) are this launch's partial sums)
            sp.send_b[e] = c;
        }
        if constexpr (is_schur<P>()) {                  // (the solve's launches write their s_nwg partial sums behind this one)
            for (int e = kSlotSchur + threadIdx.x; e < slot_len<P>(); e += kKrylovBlock) {
                const double c = e == kSlotSchurCount ? (double)sp.s_nwg : 0.0;
                sp.send_a[e] = c;
                sp.send_b[e] = c;
            }
        }
        if (threadIdx.x == 0) {
            KrylovShardMeta m{};
            m.rtol = rtol;
            m.max_iter = max_iter;
            m.precond = precond ? 1 : 0;
            *sp.meta = m;
        }
    }
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n_own ? lo + kp.chunk : kp.n_own;
    double acc = 0.0;
    for (int64_t p = lo + threadIdx.x; p < hi; p += kKrylovBlock) {
        const int64_t i = krylov_own_index(sp.own, p);
        const double r = rhs[i];
        double yv = r;
        if (precond) {
            const double m = 1.0 / (i < nvar ? px[i] : pc[i - nvar]);
            kp.minv[i] = m;
            yv = m * r;
        }
        bool solved = false;                            // y and its term: the solve's launches'
        if constexpr (is_schur<P>()) solved = i >= sp.s_lo && i < sp.s_hi;
        kp.r1[i] = r;
        kp.r2[i] = r;
        if (!solved) kp.y[i] = yv;
        kp.v[i] = 0.0;
        kp.kv[i] = 0.0;
        kp.w[i] = 0.0;
        kp.w2[i] = 0.0;
        kp.z[i] = 0.0;
        if (!solved && (!own_tail(sp.own, p) || sp.own.last)) acc += r * yv;
    }
    block_partial_sums<1, 1>(&acc, wsum, sp.send_a + blockIdx.x);
}

// begin: beta1 from the gathered slots, the first Lanczos vector v = y / beta1 on the owned entries, both copies of the state
template <class P>
__global__ void __launch_bounds__(kKrylovBlock) krylov_shard_first_kernel(const P sp) {
    const P& kp = sp;
    double b2 = gathered_sum<slot_len<P>()>(sp.gathered_a, sp.own.n_ranks, 1, 0);
    if constexpr (is_schur<P>()) b2 = gathered_schur_sum<slot_len<P>()>(b2, sp.gathered_a, sp.own.n_ranks);
    if constexpr (is_joint<P>())
        if (sp.own.n_ranks > 1) b2 += *sp.sigma;
    KrylovState t{};
    t.cs = -1.0;
    t.rtol = sp.meta->rtol;
    t.max_iter = sp.meta->max_iter;
    if (bad_beta2(b2)) t.status = KRYLOV_BREAKDOWN;
    else if (b2 == 0.0) t.status = KRYLOV_CONVERGED;
    else {
        t.beta1 = sqrt(b2);
        t.beta = t.phibar = t.beta1;
        const double s = 1.0 / t.beta1;
        const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n_own ? lo + kp.chunk : kp.n_own;
        for (int64_t p = lo + threadIdx.x; p < hi; p += kKrylovBlock) {
            const int64_t i = krylov_own_index(sp.own, p);
            kp.v[i] = s * kp.y[i];
        }
    }
    if (first_lane()) {
        *kp.cur = t;
        *kp.pend = t;
    }
}

// (A): the partial sums of alfa = v . y into slot A, with it the rank's partial sums of the tail of kv; copies of the tail of v and r1
// for (B).  With several ranks kv is not complete at the tail yet: its terms are (B)'s to add
__global__ void __launch_bounds__(kKrylovBlock) krylov_shard_alfa_kernel(const KrylovShardParams sp) {
    __shared__ double wsum[kWaves];
    const KrylovShardParams& kp = sp;
    const int32_t status = kp.pend->status;
    const int64_t itn = kp.pend->itn;
    if (first_lane() && (kp.cur->itn != itn || kp.cur->status != status)) {
        const uint64_t* src = (const uint64_t*)kp.pend;
        uint64_t* dst = (uint64_t*)kp.cur;
        for (int j = 0; j < (int)(sizeof(KrylovState) / sizeof(uint64_t)); ++j) dst[j] = src[j];
    }
    if (status != KRYLOV_RUNNING) return;
    const bool ortho = itn >= 1;
    const double c1 = ortho ? kp.pend->beta / kp.pend->oldb : 0.0;
    const double* __restrict__ v = kp.v;
    const double* __restrict__ kv = kp.kv;
    const double* __restrict__ r1 = kp.r1;
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < sp.own.nv) {
        const int64_t i = sp.own.v_off + threadIdx.x;
        sp.send_a[kSlotTail + threadIdx.x] = kv[i];
        sp.tail_copy[threadIdx.x] = v[i];
        sp.tail_copy[kKrylovTailMax + threadIdx.x] = r1[i];
    }
    const bool count_tail = sp.own.last && sp.own.n_ranks == 1;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n_own ? lo + kp.chunk : kp.n_own;
    double acc = 0.0;
    CTD_KRYLOV_UNROLL
    for (int64_t p = lo + threadIdx.x; p < hi; p += kKrylovBlock) {
        const int64_t i = krylov_own_index(sp.own, p);
        if (!own_tail(sp.own, p) || count_tail) acc += v[i] * lanczos_y(kv[i], r1[i], ortho, c1);
    }
    block_partial_sums<1, 1>(&acc, wsum, sp.send_a + blockIdx.x);
}

// (B)
template <class P>
__global__ void __launch_bounds__(kKrylovBlock) krylov_shard_lanczos_kernel(const P sp) {
    __shared__ double wsum[kWaves * 4];
    const P& kp = sp;
    const KrylovState s = *kp.cur;
    if (s.status != KRYLOV_RUNNING) return;
    const int n_ranks = sp.own.n_ranks;
    const bool ortho = s.itn >= 1;
    const double c1 = ortho ? s.beta / s.oldb : 0.0;
    double alfa = gathered_sum<slot_len<P>()>(sp.gathered_a, n_ranks, 1, 0);
    if (n_ranks > 1)
        for (int j = 0; j < (int)sp.own.nv; ++j)
            alfa += sp.tail_copy[j] * lanczos_y(gathered_kv_tail<slot_len<P>()>(sp.gathered_a, n_ranks, j), sp.tail_copy[kKrylovTailMax + j], ortho, c1);
    if (first_lane()) *kp.alfa = alfa;
    const double c2 = alfa / s.beta;
    const double oldeps = s.epsln, delta = s.cs * s.dbar + s.sn * alfa;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n_own ? lo + kp.chunk : kp.n_own;
    double* __restrict__ r1 = kp.r1;
    double* __restrict__ r2 = kp.r2;
    double* __restrict__ y = kp.y;
    const double* __restrict__ kv = kp.kv;
    const double* __restrict__ minv = kp.minv;
    const double* __restrict__ z = kp.z;
    const double* __restrict__ v = kp.v;
    const double* __restrict__ w = kp.w;
    const double* __restrict__ w2 = kp.w2;
    const bool precond = sp.meta->precond != 0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    CTD_KRYLOV_UNROLL
    for (int64_t p = lo + threadIdx.x; p < hi; p += kKrylovBlock) {
        const int64_t i = krylov_own_index(sp.own, p);
        const bool tail = own_tail(sp.own, p);
        const double kvv = tail ? gathered_kv_tail<slot_len<P>()>(sp.gathered_a, n_ranks, (int)(p - sp.own.n_var)) : kv[i];
        const double r2v = r2[i];
        const double yv = lanczos_y(kvv, r1[i], ortho, c1) - c2 * r2v;
        r1[i] = r2v;
        r2[i] = yv;
        const double my = precond ? minv[i] * yv : yv;
        bool solved = false;
        if constexpr (is_schur<P>()) solved = i >= sp.s_lo && i < sp.s_hi;
        if (!solved) y[i] = my;
        const double zv = z[i], u = (v[i] - oldeps * w2[i]) - delta * w[i];
        if (!tail || sp.own.last) {
            if (!solved) acc[0] += yv * my;
            acc[1] += zv * zv;
            acc[2] += zv * u;
            acc[3] += u * u;
        }
    }
    block_partial_sums<4, 4>(acc, wsum, sp.send_b + (int64_t)blockIdx.x * 4);
}

// (C)
template <class P>
__global__ void __launch_bounds__(kKrylovBlock) krylov_shard_update_kernel(const P sp) {
    const P& kp = sp;
    const KrylovState s = *kp.cur;
    if (s.status != KRYLOV_RUNNING) return;
    double b2 = 0.0, zz = 0.0, zu = 0.0, uu = 0.0;
    for (int r = 0; r < sp.own.n_ranks; ++r) {
        const double* slot = sp.gathered_b + (int64_t)r * slot_len<P>();
        const int cnt = slot_count(slot);
#pragma unroll 8
        for (int b = 0; b < cnt; ++b) {
            const double* q = slot + b * 4;
            b2 += q[0];
            zz += q[1];
            zu += q[2];
            uu += q[3];
        }
    }
    if constexpr (is_schur<P>()) b2 = gathered_schur_sum<slot_len<P>()>(b2, sp.gathered_b, sp.own.n_ranks);
    if constexpr (is_joint<P>())
        if (sp.own.n_ranks > 1) b2 += *sp.sigma;
    const double alfa = *kp.alfa;
    KrylovState t = s;
    if (bad_beta2(b2)) {
        t.status = KRYLOV_BREAKDOWN;
        if (first_lane()) *kp.pend = t;
        return;
    }
    const double eps = DBL_EPSILON;
    t.oldb = s.beta;
    t.beta = sqrt(b2);
    t.tnorm2 = s.tnorm2 + ((alfa * alfa + t.oldb * t.oldb) + t.beta * t.beta);
    const double oldeps = s.epsln;
    const double delta = s.cs * s.dbar + s.sn * alfa;
    const double gbar = s.sn * s.dbar - s.cs * alfa;
    t.epsln = s.sn * t.beta;
    t.dbar = -s.cs * t.beta;
    const double root = sqrt(gbar * gbar + t.dbar * t.dbar);
    double gamma = sqrt(gbar * gbar + t.beta * t.beta);
    gamma = gamma > eps ? gamma : eps;
    t.cs = gbar / gamma;
    t.sn = t.beta / gamma;
    const double phi = t.cs * s.phibar;
    t.phibar = t.sn * s.phibar;
    const double denom = 1.0 / gamma;
    const double a = phi * denom, y2 = zz + 2.0 * a * zu + a * a * uu;
    t.Anorm = sqrt(t.tnorm2);
    t.ynorm = y2 > 0.0 ? sqrt(y2) : 0.0;
    const double inf = __builtin_huge_val();
    const double test1 = (t.ynorm == 0.0 || t.Anorm == 0.0) ? inf : t.phibar / (t.Anorm * t.ynorm);
    const double test2 = t.Anorm == 0.0 ? inf : root / t.Anorm;
    t.itn = s.itn + 1;
    if (test2 <= s.rtol || test1 <= s.rtol) t.status = KRYLOV_CONVERGED;
    else if (t.itn >= s.max_iter) t.status = KRYLOV_MAX_ITER;
    else if (t.beta == 0.0) t.status = KRYLOV_BREAKDOWN;
    const bool go_on = t.status == KRYLOV_RUNNING;
    const double sinv = go_on ? 1.0 / t.beta : 0.0;
    const int64_t lo = (int64_t)blockIdx.x * kp.chunk, hi = lo + kp.chunk < kp.n_own ? lo + kp.chunk : kp.n_own;
    double* __restrict__ v = kp.v;
    double* __restrict__ w = kp.w;
    double* __restrict__ w2 = kp.w2;
    double* __restrict__ z = kp.z;
    const double* __restrict__ y = kp.y;
    CTD_KRYLOV_UNROLL
    for (int64_t p = lo + threadIdx.x; p < hi; p += kKrylovBlock) {
        const int64_t i = krylov_own_index(sp.own, p);
        const double wv = w[i];
        const double wn = ((v[i] - oldeps * w2[i]) - delta * wv) * denom;
        w2[i] = wv;
        w[i] = wn;
        z[i] = z[i] + phi * wn;
        if (go_on) v[i] = sinv * y[i];
    }
    if (first_lane()) *kp.pend = t;
}

}  // namespace

hipError_t krylov_shard_start(const KrylovShardParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                              double rtol, int64_t max_iter, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_init_kernel<KrylovShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp, rhs, px, pc, nvar, rtol, max_iter);
    return hipGetLastError();
}
hipError_t krylov_shard_begin(const KrylovShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_first_kernel<KrylovShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_shard_alfa(const KrylovShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_shard_alfa_kernel, dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_shard_lanczos(const KrylovShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_lanczos_kernel<KrylovShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_shard_update(const KrylovShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_update_kernel<KrylovShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}

hipError_t krylov_schur_shard_start(const KrylovSchurShardParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                                    double rtol, int64_t max_iter, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_init_kernel<KrylovSchurShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp,
                       rhs, px, pc, nvar, rtol, max_iter);
    return hipGetLastError();
}
hipError_t krylov_schur_shard_begin(const KrylovSchurShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_first_kernel<KrylovSchurShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_schur_shard_lanczos(const KrylovSchurShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_lanczos_kernel<KrylovSchurShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_schur_shard_update(const KrylovSchurShardParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_update_kernel<KrylovSchurShardParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}

hipError_t krylov_schur_joint_start(const KrylovSchurJointParams& sp, const double* rhs, const double* px, const double* pc, int64_t nvar,
                                    double rtol, int64_t max_iter, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_init_kernel<KrylovSchurJointParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp,
                       rhs, px, pc, nvar, rtol, max_iter);
    return hipGetLastError();
}
hipError_t krylov_schur_joint_begin(const KrylovSchurJointParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_first_kernel<KrylovSchurJointParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_schur_joint_lanczos(const KrylovSchurJointParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_lanczos_kernel<KrylovSchurJointParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}
hipError_t krylov_schur_joint_update(const KrylovSchurJointParams& sp, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(krylov_shard_update_kernel<KrylovSchurJointParams>), dim3((unsigned)sp.nwg), dim3(kKrylovBlock), 0, st, sp);
    return hipGetLastError();
}

}  // namespace ctd
