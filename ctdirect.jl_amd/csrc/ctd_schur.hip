// ctd_schur.hip -- the kernels of the chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*) and their launchers.  The
// matrix, the recurrences, the order of every sum and the workspace are specified in ctd_schur_kernels.hpp.  Strict rounding (the
// Makefile compiles this file with -ffp-contract=off): results are reproducible bit for bit.
#include <type_traits>

#include "ctd_common.hpp"
#include "ctd_schur_kernels.hpp"

namespace ctd {
namespace {

constexpr int kWave = 64;

__device__ __forceinline__ double* schur_blocks_d(double* ws, int64_t N) { return ws + kSchurFixed + N; }
__device__ __forceinline__ const double* schur_blocks_d(const double* ws, int64_t N) { return ws + kSchurFixed + N; }

// ASSEMBLE: one thread per entry of D_k and E_k (grid-stride), the header and the status words
__global__ void __launch_bounds__(256) schur_assemble_kernel(const SchurFactorParams fp) {
    const int64_t m = fp.m, mm = m * m, nd = fp.N * mm, total = 2 * nd;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    int64_t* head = (int64_t*)fp.ws;
    if (tid == 0) {
        head[0] = kSchurTag;
        head[1] = fp.N;
        head[2] = m;
        head[3] = fp.chunk_steps;
        head[4] = fp.n_chunks;
        for (int j = 5; j < kSchurPart; ++j) head[j] = 0;
    }
    for (int64_t e = tid; e < kSchurFixed - kSchurPart; e += stride) fp.ws[kSchurPart + e] = 0.0;
    for (int64_t e = tid; e < fp.N; e += stride) head[kSchurFixed + e] = -1;
    double* blocks = schur_blocks_d(fp.ws, fp.N);
    for (int64_t e = tid; e < total; e += stride) {
        const bool coupling = e >= nd;
        const int64_t q = coupling ? e - nd : e, k = q / mm;
        const int a = (int)((q - k * mm) / m), b = (int)(q - k * mm - a * m);
        double s = 0.0;
        if (!coupling || (k + 1 < fp.N && (k + 1) % fp.chunk_steps != 0)) {
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
        blocks[e] = s;
    }
}

// a block of m x m doubles on its way from global memory to LDS: R values per lane, held in registers in between
template <int MB> struct Stage {
    static constexpr int R = (MB * MB + kWave - 1) / kWave;
    double v[R];
    __device__ __forceinline__ void load(const double* g, int mm, int lane) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int e = lane + kWave * i;
            v[i] = e < mm ? g[e] : 0.0;
        }
    }
    __device__ __forceinline__ void put(double* lds, int mm, int lane) const {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int e = lane + kWave * i;
            if (e < mm) lds[e] = v[i];
        }
    }
};

__device__ __forceinline__ void fill_nan(double* g, int mm, int lane) {
    const double nan = __builtin_nan("");
    for (int e = lane; e < mm; e += kWave) g[e] = nan;
}

// THE FACTOR: one wave per chunk
template <int MB> __global__ void __launch_bounds__(kWave) schur_factor_kernel(const SchurFactorParams fp) {
    __shared__ double lds[3 * MB * MB + MB];
    const int lane = threadIdx.x, m = fp.m, mm = m * m;
    double* A = lds;
    double* Eb = lds + MB * MB;
    double* Fp = lds + 2 * MB * MB;
    double* dinv = lds + 3 * MB * MB;
    double* Dg = schur_blocks_d(fp.ws, fp.N);
    double* Eg = Dg + fp.N * (int64_t)mm;
    int64_t* status = (int64_t*)fp.ws + kSchurFixed;
    for (int64_t c = blockIdx.x; c < fp.n_chunks; c += gridDim.x) {
        const int64_t k0 = c * fp.chunk_steps, k1 = k0 + fp.chunk_steps < fp.N ? k0 + fp.chunk_steps : fp.N;
        int64_t bad = -1;
        Stage<MB> sd, se;
        sd.load(Dg + k0 * mm, mm, lane);
        se.load(Eg + k0 * mm, mm, lane);
        for (int64_t k = k0; k < k1; ++k) {
            __syncthreads();                     // the previous block's reads of A, Eb, Fp are done
            sd.put(A, mm, lane);
            se.put(Eb, mm, lane);
            if (k + 1 < k1) {                    // the next block's loads, ahead of this block's recurrence
                sd.load(Dg + (k + 1) * mm, mm, lane);
                se.load(Eg + (k + 1) * mm, mm, lane);
            }
            __syncthreads();
            if (bad < 0) {
                if (k > k0) {
                    for (int e = lane; e < mm; e += kWave) {
                        const int a = e / m, b = e - a * m;
                        if (b <= a) {
                            double s = 0.0;
                            for (int j = 0; j < m; ++j) s += Fp[a * m + j] * Fp[b * m + j];
                            A[e] = A[e] - s;
                        }
                    }
                    __syncthreads();
                }
                for (int j = 0; j < m; ++j) {
                    if (lane >= j && lane < m) {
                        double s = A[lane * m + j];
                        for (int p = 0; p < j; ++p) s -= A[lane * m + p] * A[j * m + p];
                        A[lane * m + j] = s;
                    }
                    __syncthreads();
                    const double d = A[j * m + j];
                    if (!(d > 0.0) || !__builtin_isfinite(d)) {     // (every lane reads the same word: the exit is uniform)
                        bad = k;
                        break;
                    }
                    __syncthreads();             // every lane has read the pivot before lane j replaces it by its root
                    const double dj = sqrt(d), rj = 1.0 / dj;
                    if (lane == j) {
                        A[j * m + j] = dj;
                        dinv[j] = rj;
                    } else if (lane > j && lane < m) A[lane * m + j] = A[lane * m + j] * rj;
                    __syncthreads();
                }
            }
            if (bad >= 0) {
                fill_nan(Dg + k * mm, mm, lane);
                fill_nan(Eg + k * mm, mm, lane);
                continue;
            }
            if (lane < m) {
                for (int j = 0; j < m; ++j) {
                    double s = Eb[lane * m + j];
                    for (int p = 0; p < j; ++p) s -= Eb[lane * m + p] * A[j * m + p];
                    Eb[lane * m + j] = s * dinv[j];
                }
            }
            __syncthreads();
            for (int e = lane; e < mm; e += kWave) {
                const int a = e / m, b = e - a * m;
                Dg[k * mm + e] = b <= a ? A[e] : 0.0;
                Eg[k * mm + e] = Eb[e];
            }
            double* t = Eb;                      // F_k is the next block's F_{k-1}
            Eb = Fp;
            Fp = t;
        }
        if (lane == 0) status[c] = bad;
    }
}

// THE SOLVE: one wave per chunk, a forward and a backward sweep.  What does not depend on the recurrence -- the next block's L and F,
// its entries of r, and in the backward sweep its entries of t -- is loaded one block ahead
template <int MB> __global__ void __launch_bounds__(kWave) schur_solve_kernel(const SchurSolveParams sp) {
    __shared__ double lds[2 * MB * MB + 2 * MB];
    const int lane = threadIdx.x, m = sp.m, mm = m * m;
    const int64_t* head = (const int64_t*)sp.ws;
    if (head[0] != kSchurTag || head[1] != sp.N || head[2] != m) return;     // not a factor of this N and m: nothing is stored
    const int64_t L = head[3], n_chunks = head[4];
    if (L < 1 || L > sp.N || n_chunks != (sp.N + L - 1) / L) return;
    if (sp.mode == SCHUR_ITER && sp.cur->status != KRYLOV_RUNNING) return;   // the freeze
    double* Lb = lds;
    double* Fb = lds + MB * MB;
    double* tv = lds + 2 * MB * MB;
    double* dinv = tv + MB;
    const double* Lg = schur_blocks_d(sp.ws, sp.N);
    const double* Fg = Lg + sp.N * (int64_t)mm;
    const bool row = lane < m, sums = sp.mode != SCHUR_PLAIN;
    double acc = 0.0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t k0 = c * L, k1 = k0 + L < sp.N ? k0 + L : sp.N;
        Stage<MB> sl, sf;
        sl.load(Lg + k0 * mm, mm, lane);
        double rn = row ? sp.r[k0 * m + lane] : 0.0, g = 0.0;
        for (int64_t k = k0; k < k1; ++k) {
            __syncthreads();
            sl.put(Lb, mm, lane);
            if (k > k0) sf.put(Fb, mm, lane);
            g = rn;
            if (k + 1 < k1) {
                sl.load(Lg + (k + 1) * mm, mm, lane);
                sf.load(Fg + k * mm, mm, lane);
                rn = row ? sp.r[(k + 1) * m + lane] : 0.0;
            }
            __syncthreads();
            if (row) dinv[lane] = 1.0 / Lb[lane * m + lane];
            if (k > k0 && row) {
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += Fb[lane * m + j] * tv[j];
                g = g - s;
            }
            __syncthreads();                     // t_{k-1} has been read, the reciprocals are there
            for (int j = 0; j < m; ++j) {
                const double tj = __shfl(g, j, kWave) * dinv[j];
                if (lane == j) g = tj;
                else if (lane > j && row) g -= Lb[lane * m + j] * tj;
            }
            if (row) {
                tv[lane] = g;
                sp.out[k * m + lane] = g;
            }
        }
        // (g is t of the chunk's last block; the earlier blocks' t come back from `out`, where this lane stored them)
        sl.load(Lg + (k1 - 1) * mm, mm, lane);
        double tn = g, rb = (sums && row) ? sp.r[(k1 - 1) * m + lane] : 0.0;
        for (int64_t k = k1 - 1; k >= k0; --k) {
            __syncthreads();
            sl.put(Lb, mm, lane);
            if (k + 1 < k1) sf.put(Fb, mm, lane);
            g = tn;
            const double rk = rb;
            if (k > k0) {
                sl.load(Lg + (k - 1) * mm, mm, lane);
                sf.load(Fg + (k - 1) * mm, mm, lane);
                tn = row ? sp.out[(k - 1) * m + lane] : 0.0;
                rb = (sums && row) ? sp.r[(k - 1) * m + lane] : 0.0;
            }
            __syncthreads();
            if (row) dinv[lane] = 1.0 / Lb[lane * m + lane];
            if (k + 1 < k1 && row) {
                double s = 0.0;
                for (int j = 0; j < m; ++j) s += Fb[j * m + lane] * tv[j];
                g = g - s;
            }
            __syncthreads();                     // y_{k+1} has been read, the reciprocals are there
            for (int j = m - 1; j >= 0; --j) {
                const double yj = __shfl(g, j, kWave) * dinv[j];
                if (lane == j) g = yj;
                else if (lane < j) g -= Lb[j * m + lane] * yj;
            }
            if (row) {
                tv[lane] = g;
                sp.out[k * m + lane] = g;
                if (sums) acc += rk * g;
            }
        }
    }
    if (sums) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
        if (lane == 0) sp.part[blockIdx.x] = acc;
    }
}

template <class F> hipError_t for_block_size(int m, F&& f) {
    if (m <= 8) return f(std::integral_constant<int, 8>{});
    if (m <= 16) return f(std::integral_constant<int, 16>{});
    if (m <= 32) return f(std::integral_constant<int, 32>{});
    if (m <= kSchurMaxBlock) return f(std::integral_constant<int, 64>{});
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t schur_factor(const SchurFactorParams& fp, hipStream_t st) {
    if (fp.N < 1 || fp.m < 1 || fp.chunk_steps < 1 || fp.n_chunks != (fp.N + fp.chunk_steps - 1) / fp.chunk_steps) return hipErrorInvalidValue;
    const int64_t total = 2 * fp.N * (int64_t)fp.m * fp.m, want = (total + 255) / 256;
    const unsigned grid = (unsigned)(want > 4096 ? 4096 : (want < 1 ? 1 : want));
    hipLaunchKernelGGL(schur_assemble_kernel, dim3(grid), dim3(256), 0, st, fp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned wgs = (unsigned)(fp.n_chunks > kSchurMaxWg ? kSchurMaxWg : fp.n_chunks);
    return for_block_size(fp.m, [&](auto mb) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_factor_kernel<decltype(mb)::value>), dim3(wgs), dim3(kWave), 0, st, fp);
        return hipGetLastError();
    });
}

hipError_t schur_solve(const SchurSolveParams& sp, hipStream_t st) {
    if (sp.N < 1 || sp.m < 1) return hipErrorInvalidValue;
    return for_block_size(sp.m, [&](auto mb) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_solve_kernel<decltype(mb)::value>), dim3((unsigned)schur_solve_grid(sp.N)), dim3(kWave), 0, st, sp);
        return hipGetLastError();
    });
}

}  // namespace ctd
