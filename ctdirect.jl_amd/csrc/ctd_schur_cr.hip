// ctd_schur_cr.hip -- the kernels of the log-depth exact block-tridiagonal Schur preconditioner (ctd_kkt_schur_cr*) and their
// launchers.  The matrix, the recurrences of a level, the order of every sum and the workspace are specified in
// ctd_schur_cr_kernels.hpp.  Strict rounding (the Makefile compiles this file with -ffp-contract=off): results are reproducible bit
// for bit.
#include <type_traits>

#include "ctd_common.hpp"
#include "ctd_schur_cr_kernels.hpp"

namespace ctd {
namespace {

constexpr int kWave = 64;
constexpr int64_t kCrMaxGrid = 1 << 16;     // cap of a level's workgroup count (grid-stride: it does not enter any result)

// FP / SP (the kernels below): the argument struct, SchurCrFactorParams / SchurCrSolveParams or their shard forms
// (ctd_schur_cr_kernels.hpp), which add the global index of block 0 -- word 4 of the header -- and the place of the partial sums.
// The instantiations for the whole-grid structs compile to the code without them
template <class P> constexpr bool is_shard() {
    return std::is_same<P, SchurCrShardFactorParams>::value || std::is_same<P, SchurCrShardSolveParams>::value;
}

// the regions of the workspace
struct CrWs {
    int64_t* status;
    double *D, *E, *Gm, *rhs, *y, *part;
};
__device__ __forceinline__ CrWs cr_ws(double* ws, int64_t N, int m) {
    const int64_t nd = N * (int64_t)m * m;
    CrWs w;
    w.status = (int64_t*)ws + kSchurFixed;
    w.D = ws + kSchurFixed + N;
    w.E = w.D + nd;
    w.Gm = w.E + nd;
    w.rhs = w.Gm + nd;
    w.y = w.rhs + N * (int64_t)m;
    w.part = ws + kSchurPart;
    return w;
}

// ASSEMBLE: one thread per entry of D_k and E_k (grid-stride), the header, the status words; everything else is zeroed.  The entries
// are those of the chunked factor's assemble launch with one chunk
template <class FP> __global__ void __launch_bounds__(256) schur_cr_assemble_kernel(const FP fp) {
    const int64_t m = fp.m, mm = m * m, nd = fp.N * mm, total = 2 * nd;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t* head = (int64_t*)fp.ws;
    if (tid == 0) {
        head[0] = kSchurCrTag;
        head[1] = fp.N;
        head[2] = m;
        head[3] = fp.n_levels;
        for (int j = 4; j < kSchurPart; ++j) head[j] = 0;
        if constexpr (is_shard<FP>()) head[4] = fp.first;
    }
    for (int64_t e = tid; e < kSchurFixed - kSchurPart; e += stride) fp.ws[kSchurPart + e] = 0.0;
    for (int64_t e = tid; e < fp.N; e += stride) head[kSchurFixed + e] = -1;
    const CrWs w = cr_ws(fp.ws, fp.N, fp.m);
    for (int64_t e = tid; e < nd + 2 * fp.N * m; e += stride) w.Gm[e] = 0.0;          // (Gm, and the solve's scratch behind it)
    for (int64_t e = tid; e < total; e += stride) {
        const bool coupling = e >= nd;
        const int64_t q = coupling ? e - nd : e, k = q / mm;
        const int a = (int)((q - k * mm) / m), b = (int)(q - k * mm - a * m);
        double s = 0.0;
        if (!coupling || k + 1 < fp.N) {
            const int64_t ra = (coupling ? k + 1 : k) * m + a, rb = k * m + b;
            int64_t pa = fp.rowptr[ra], pb = fp.rowptr[rb];
            const int64_t ea = fp.rowptr[ra + 1], eb = fp.rowptr[rb + 1];
            while (pa < ea && pb < eb) {
                const int64_t ca = fp.colind[pa], cb = fp.colind[pb];
                if (ca >= fp.v_off || cb >= fp.v_off) break;        // (columns ascend: the tail columns end a row)
                if (ca == cb) {
                    s += (fp.jvals[pa] * fp.jvals[pb]) * (1.0 / fp.px[ca]);
                    ++pa;
                    ++pb;
                } else if (ca < cb) ++pa;
                else ++pb;
            }
            if (!coupling && a == b && fp.sc) s += fp.sc[ra];
        }
        w.D[e] = s;
    }
}

__device__ __forceinline__ void stage(double* lds, const double* g, int mm, int lane) {
    for (int e = lane; e < mm; e += kWave) lds[e] = g[e];
}
__device__ __forceinline__ void fill_nan(double* g, int mm, int lane) {
    const double nan = __builtin_nan("");
    for (int e = lane; e < mm; e += kWave) g[e] = nan;
}

// ELIMINATE at level h = 2^l (h = 0: the root, block 0 alone, no neighbours): one wave per eliminated block
template <int MB, class FP> __global__ void __launch_bounds__(kWave) schur_cr_eliminate_kernel(const FP fp, const int64_t h) {
    __shared__ double lds[3 * MB * MB + MB];
    const int lane = threadIdx.x, m = fp.m, mm = m * m;
    double* A = lds;
    double* El = lds + MB * MB;
    double* Er = lds + 2 * MB * MB;
    double* dinv = lds + 3 * MB * MB;
    const CrWs w = cr_ws(fp.ws, fp.N, m);
    const int64_t count = h == 0 ? 1 : (fp.N > h ? (fp.N - h + 2 * h - 1) / (2 * h) : 0);
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int64_t i = (2 * q + 1) * h;
        const bool left = h > 0, right = h > 0 && i + h < fp.N;
        __syncthreads();                         // the previous block's reads of the staged blocks are done
        stage(A, w.D + i * mm, mm, lane);
        if (left) stage(El, w.E + (i - h) * mm, mm, lane);
        if (right) stage(Er, w.E + i * mm, mm, lane);
        __syncthreads();
        int bad = -1;
        for (int j = 0; j < m; ++j) {
            if (lane >= j && lane < m) {
                double s = A[lane * m + j];
                for (int p = 0; p < j; ++p) s -= A[lane * m + p] * A[j * m + p];
                A[lane * m + j] = s;
            }
            __syncthreads();
            const double d = A[j * m + j];
            if (!(d > 0.0) || !__builtin_isfinite(d)) {     // (every lane reads the same word: the exit is uniform)
                bad = j;
                break;
            }
            __syncthreads();                     // every lane has read the pivot before lane j replaces it by its root
            const double dj = sqrt(d), rj = 1.0 / dj;
            if (lane == j) {
                A[j * m + j] = dj;
                dinv[j] = rj;
            } else if (lane > j && lane < m) A[lane * m + j] = A[lane * m + j] * rj;
            __syncthreads();
        }
        if (lane == 0) w.status[i] = bad;
        if (bad >= 0) {
            fill_nan(w.D + i * mm, mm, lane);
            if (left) fill_nan(w.Gm + i * mm, mm, lane);
            if (right) fill_nan(w.E + i * mm, mm, lane);
            continue;
        }
        if (lane < m) {
            if (left) {                          // column `lane` of Gm = L^-1 E[lf]
                for (int j = 0; j < m; ++j) {
                    double s = El[j * m + lane];
                    for (int p = 0; p < j; ++p) s -= A[j * m + p] * El[p * m + lane];
                    El[j * m + lane] = s * dinv[j];
                }
            }
            if (right) {                         // row `lane` of Gp = E[i] L^-T
                for (int j = 0; j < m; ++j) {
                    double s = Er[lane * m + j];
                    for (int p = 0; p < j; ++p) s -= Er[lane * m + p] * A[j * m + p];
                    Er[lane * m + j] = s * dinv[j];
                }
            }
        }
        __syncthreads();
        for (int e = lane; e < mm; e += kWave) {
            const int a = e / m, b = e - a * m;
            w.D[i * mm + e] = b <= a ? A[e] : 0.0;
            if (left) w.Gm[i * mm + e] = El[e];
            if (right) w.E[i * mm + e] = Er[e];
        }
    }
}

// UPDATE at level h: one thread per entry of the survivors' D (lower triangle) and of their new couplings
template <class FP> __global__ void __launch_bounds__(256) schur_cr_update_kernel(const FP fp, const int64_t h) {
    const int m = fp.m;
    const int64_t mm = (int64_t)m * m, N = fp.N;
    const CrWs w = cr_ws(fp.ws, N, m);
    const int64_t survivors = (N + 2 * h - 1) / (2 * h), total = survivors * 2 * mm;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = tid; e < total; e += stride) {
        const int64_t sv = e / (2 * mm), k = sv * 2 * h;
        int64_t q = e - sv * 2 * mm;
        const bool coupling = q >= mm;
        if (coupling) q -= mm;
        const int a = (int)(q / m), b = (int)(q - (int64_t)a * m);
        if (!coupling) {
            if (b > a) continue;
            double v = w.D[k * mm + q];
            if (k >= h) {
                const double* Gp = w.E + (k - h) * mm;
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += Gp[a * m + j] * Gp[b * m + j];
                v = v - s;
            }
            if (k + h < N) {
                const double* Gm = w.Gm + (k + h) * mm;
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += Gm[j * m + a] * Gm[j * m + b];
                v = v - s;
            }
            w.D[k * mm + q] = v;
        } else if (k + 2 * h < N) {
            const double* Gp = w.E + (k + h) * mm;
            const double* Gm = w.Gm + (k + h) * mm;
            double s = 0.0;
            for (int j = 0; j < m; ++j) s += Gp[a * m + j] * Gm[j * m + b];
            w.E[k * mm + q] = -s;
        }
    }
}

// ---- the solve -------------------------------------------------------------------------------------------------------------------------
template <int MB> struct CrLds {
    double L[MB * MB], G[MB * MB], v[MB], dinv[MB];
};

// uniform: whether this launch stores anything (the header -- on a shard the step range too --, and in iteration mode the freeze)
template <class SP> __device__ __forceinline__ bool cr_go(const SP& sp) {
    const int64_t* head = (const int64_t*)sp.ws;
    if (head[0] != kSchurCrTag || head[1] != sp.N || head[2] != sp.m || head[3] != sp.n_levels) return false;
    if constexpr (is_shard<SP>())
        if (head[4] != sp.first) return false;
    return sp.mode != SCHUR_ITER || sp.cur->status == KRYLOV_RUNNING;
}

// L_i and the reciprocals of its diagonal into LDS
template <int MB> __device__ __forceinline__ void cr_stage_L(CrLds<MB>& s, const double* Lg, int m, int lane) {
    __syncthreads();                             // earlier reads of s.L and s.dinv are done
    stage(s.L, Lg, m * m, lane);
    __syncthreads();
    if (lane < m) s.dinv[lane] = 1.0 / s.L[lane * m + lane];
    __syncthreads();
}
// lane a: (L^-1 b)(a), through wave shuffles
template <int MB> __device__ __forceinline__ double cr_forward(const CrLds<MB>& s, double g, int m, int lane) {
    for (int j = 0; j < m; ++j) {
        const double tj = __shfl(g, j, kWave) * s.dinv[j];
        if (lane == j) g = tj;
        else if (lane > j && lane < m) g -= s.L[lane * m + j] * tj;
    }
    return g;
}
// lane a: (L^-T b)(a)
template <int MB> __device__ __forceinline__ double cr_backward(const CrLds<MB>& s, double g, int m, int lane) {
    for (int j = m - 1; j >= 0; --j) {
        const double yj = __shfl(g, j, kWave) * s.dinv[j];
        if (lane == j) g = yj;
        else if (lane < j) g -= s.L[j * m + lane] * yj;
    }
    return g;
}
// the block G and the vector v (this lane's entry) into LDS; lane a: sum_j G(a, j) v(j), or with TR sum_j G(j, a) v(j)
template <int MB, bool TR> __device__ __forceinline__ double cr_matvec(CrLds<MB>& s, const double* Gg, double v, int m, int lane) {
    __syncthreads();                             // earlier reads of s.G and s.v are done
    stage(s.G, Gg, m * m, lane);
    if (lane < m) s.v[lane] = v;
    __syncthreads();
    double sum = 0.0;
    if (lane < m)
        for (int j = 0; j < m; ++j) sum += (TR ? s.G[j * m + lane] : s.G[lane * m + j]) * s.v[j];
    return sum;
}

// DOWN at level h: one wave per active block
template <int MB, class SP> __global__ void __launch_bounds__(kWave) schur_cr_down_kernel(const SP sp, const int64_t h) {
    __shared__ CrLds<MB> s;
    if (!cr_go(sp)) return;
    const int lane = threadIdx.x, m = sp.m;
    const int64_t mm = (int64_t)m * m, N = sp.N;
    const bool row = lane < m;
    const CrWs w = cr_ws(sp.ws, N, m);
    const double* src = h == 1 ? sp.r : w.rhs;
    const int64_t active = (N + h - 1) / h;
    for (int64_t q = blockIdx.x; q < active; q += gridDim.x) {
        const int64_t k = q * h;
        if (q & 1) {
            cr_stage_L(s, w.D + k * mm, m, lane);
            const double y = cr_forward(s, row ? src[k * m + lane] : 0.0, m, lane);
            if (row) w.y[k * m + lane] = y;
            continue;
        }
        double g = row ? src[k * m + lane] : 0.0;
        if (k >= h) {
            const int64_t i = k - h;
            cr_stage_L(s, w.D + i * mm, m, lane);
            const double y = cr_forward(s, row ? src[i * m + lane] : 0.0, m, lane);
            g = g - cr_matvec<MB, false>(s, w.E + i * mm, y, m, lane);
        }
        if (k + h < N) {
            const int64_t i = k + h;
            cr_stage_L(s, w.D + i * mm, m, lane);
            const double y = cr_forward(s, row ? src[i * m + lane] : 0.0, m, lane);
            g = g - cr_matvec<MB, true>(s, w.Gm + i * mm, y, m, lane);
        }
        if (row) w.rhs[k * m + lane] = g;
    }
}

// ROOT: x_0 = L_0^-T L_0^-1 rhs_0
template <int MB, class SP> __global__ void __launch_bounds__(kWave) schur_cr_root_kernel(const SP sp) {
    __shared__ CrLds<MB> s;
    if (!cr_go(sp)) return;
    const int lane = threadIdx.x, m = sp.m;
    const CrWs w = cr_ws(sp.ws, sp.N, m);
    const double* src = sp.n_levels == 0 ? sp.r : w.rhs;
    cr_stage_L(s, w.D, m, lane);
    double g = cr_forward(s, lane < m ? src[lane] : 0.0, m, lane);
    g = cr_backward(s, g, m, lane);
    if (lane < m) sp.out[lane] = g;
}

// UP at level h: one wave per eliminated block
template <int MB, class SP> __global__ void __launch_bounds__(kWave) schur_cr_up_kernel(const SP sp, const int64_t h) {
    __shared__ CrLds<MB> s;
    if (!cr_go(sp)) return;
    const int lane = threadIdx.x, m = sp.m;
    const int64_t mm = (int64_t)m * m, N = sp.N;
    const bool row = lane < m;
    const CrWs w = cr_ws(sp.ws, N, m);
    const int64_t count = N > h ? (N - h + 2 * h - 1) / (2 * h) : 0;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int64_t i = (2 * q + 1) * h;
        double g = row ? w.y[i * m + lane] : 0.0;
        g = g - cr_matvec<MB, false>(s, w.Gm + i * mm, row ? sp.out[(i - h) * m + lane] : 0.0, m, lane);
        if (i + h < N) g = g - cr_matvec<MB, true>(s, w.E + i * mm, row ? sp.out[(i + h) * m + lane] : 0.0, m, lane);
        cr_stage_L(s, w.D + i * mm, m, lane);
        g = cr_backward(s, g, m, lane);
        if (row) sp.out[i * m + lane] = g;
    }
}

// the partial sums of r . x over the block rows, one per workgroup
template <class SP> __global__ void __launch_bounds__(kWave) schur_cr_dot_kernel(const SP sp) {
    if (!cr_go(sp)) return;
    const int lane = threadIdx.x, m = sp.m;
    double acc = 0.0;
    if (lane < m)
        for (int64_t k = blockIdx.x; k < sp.N; k += gridDim.x) acc += sp.r[k * m + lane] * sp.out[k * m + lane];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    if constexpr (is_shard<SP>()) {
        if (lane == 0) sp.part[blockIdx.x] = acc;
    } else {
        if (lane == 0) sp.ws[kSchurPart + blockIdx.x] = acc;
    }
}

template <class F> hipError_t for_block_size(int m, F&& f) {
    if (m <= 8) return f(std::integral_constant<int, 8>{});
    if (m <= 16) return f(std::integral_constant<int, 16>{});
    if (m <= 32) return f(std::integral_constant<int, 32>{});
    if (m <= kSchurMaxBlock) return f(std::integral_constant<int, 64>{});
    return hipErrorInvalidValue;
}

inline unsigned cr_grid(int64_t items) { return (unsigned)(items < 1 ? 1 : (items > kCrMaxGrid ? kCrMaxGrid : items)); }
// ... of the kernels with one thread per entry: workgroups of 256 threads, at most 4096 of them
inline unsigned cr_grid_threads(int64_t entries) { return cr_grid((entries + 255) / 256 > 4096 ? 4096 : (entries + 255) / 256); }

}  // namespace

namespace {

template <class FP> hipError_t cr_factor(const FP& fp, hipStream_t st) {
    if (fp.N < 1 || fp.m < 1 || fp.n_levels != schur_cr_levels(fp.N)) return hipErrorInvalidValue;
    const int64_t mm = (int64_t)fp.m * fp.m;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_assemble_kernel<FP>), dim3(cr_grid_threads(2 * fp.N * mm)), dim3(256), 0, st, fp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return for_block_size(fp.m, [&](auto mb) {
        constexpr int MB = decltype(mb)::value;
        for (int l = 0; l < fp.n_levels; ++l) {
            const SchurCrLevel lv = schur_cr_level(fp.N, l);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_eliminate_kernel<MB, FP>), dim3(cr_grid(lv.count)), dim3(kWave), 0, st, fp, lv.first);
            hipError_t le = hipGetLastError();
            if (le != hipSuccess) return le;
            const int64_t survivors = (fp.N + lv.stride - 1) / lv.stride;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_update_kernel<FP>), dim3(cr_grid_threads(survivors * 2 * mm)), dim3(256), 0, st, fp, lv.first);
            le = hipGetLastError();
            if (le != hipSuccess) return le;
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_eliminate_kernel<MB, FP>), dim3(1), dim3(kWave), 0, st, fp, (int64_t)0);
        return hipGetLastError();
    });
}

template <class SP> hipError_t cr_solve(const SP& sp, hipStream_t st) {
    if (sp.N < 1 || sp.m < 1 || sp.n_levels != schur_cr_levels(sp.N)) return hipErrorInvalidValue;
    const hipError_t e = for_block_size(sp.m, [&](auto mb) {
        constexpr int MB = decltype(mb)::value;
        for (int l = 0; l < sp.n_levels; ++l) {
            const int64_t h = (int64_t)1 << l;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_down_kernel<MB, SP>), dim3(cr_grid((sp.N + h - 1) / h)), dim3(kWave), 0, st, sp, h);
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return le;
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_root_kernel<MB, SP>), dim3(1), dim3(kWave), 0, st, sp);
        hipError_t le = hipGetLastError();
        if (le != hipSuccess) return le;
        for (int l = sp.n_levels - 1; l >= 0; --l) {
            const SchurCrLevel lv = schur_cr_level(sp.N, l);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_up_kernel<MB, SP>), dim3(cr_grid(lv.count)), dim3(kWave), 0, st, sp, lv.first);
            le = hipGetLastError();
            if (le != hipSuccess) return le;
        }
        return hipSuccess;
    });
    if (e != hipSuccess || sp.mode == SCHUR_PLAIN) return e;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_dot_kernel<SP>), dim3((unsigned)schur_solve_grid(sp.N)), dim3(kWave), 0, st, sp);
    return hipGetLastError();
}

}  // namespace

hipError_t schur_cr_factor(const SchurCrFactorParams& fp, hipStream_t st) { return cr_factor(fp, st); }
hipError_t schur_cr_solve(const SchurCrSolveParams& sp, hipStream_t st) { return cr_solve(sp, st); }
hipError_t schur_cr_factor(const SchurCrShardFactorParams& fp, hipStream_t st) { return cr_factor(fp, st); }
hipError_t schur_cr_solve(const SchurCrShardSolveParams& sp, hipStream_t st) {
    if (sp.mode != SCHUR_PLAIN && !sp.part) return hipErrorInvalidValue;
    return cr_solve(sp, st);
}

}  // namespace ctd
