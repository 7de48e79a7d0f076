// ctd_krylov.hip -- the vector kernels of the device-resident MINRES solve (ctd_kkt_minres*) and their launchers.  The recurrences,
// the launch cut, the summation order, the two copies of the state and the freeze are specified in ctd_krylov_kernels.hpp.
// Strict rounding like the products (the Makefile compiles this file with -ffp-contract=off): every expression below rounds as
// the NumPy expression of scipy.sparse.linalg.minres it transcribes.
#include <cfloat>

#include "ctd_common.hpp"
#include "ctd_krylov_kernels.hpp"

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
        kp.r1[i] = r;
        kp.r2[i] = r;
        kp.y[i] = yv;
        kp.v[i] = 0.0;
        kp.kv[i] = 0.0;
        kp.w[i] = 0.0;
        kp.w2[i] = 0.0;
        kp.z[i] = 0.0;
        acc += r * yv;
    }
    block_partial_sums<1, 1>(&acc, wsum, kp.part + blockIdx.x);
}

// start, second launch: beta1, the first Lanczos vector v = y / beta1, both copies of the state
__global__ void __launch_bounds__(kKrylovBlock) krylov_first_kernel(const KrylovParams kp, const double rtol, const int64_t max_iter) {
    const double b2 = ordered_sum(kp.part, kp.nwg, 1);
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
        y[i] = my;
        const double zv = z[i], u = (v[i] - oldeps * w2[i]) - delta * w[i];
        acc[0] += yv * my;
        acc[1] += zv * zv;
        acc[2] += zv * u;
        acc[3] += u * u;
    }
    block_partial_sums<4, 4>(acc, wsum, kp.part + kPartB + (int64_t)blockIdx.x * 4);
}

// (C)
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
    hipLaunchKernelGGL(krylov_init_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rhs, px, pc, nvar);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(krylov_first_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp, rtol, max_iter);
    return hipGetLastError();
}

hipError_t krylov_alfa(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_alfa_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}

hipError_t krylov_step(const KrylovParams& kp, hipStream_t st) {
    hipLaunchKernelGGL(krylov_lanczos_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(krylov_update_kernel, dim3((unsigned)kp.nwg), dim3(kKrylovBlock), 0, st, kp);
    return hipGetLastError();
}

}  // namespace ctd
