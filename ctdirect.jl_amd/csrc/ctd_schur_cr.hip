// ctd_schur_cr.hip -- the kernels of the log-depth exact block-tridiagonal Schur preconditioner (ctd_kkt_schur_cr*) and their
// launchers.  The matrix, the recurrences of a level, the order of every sum and the workspace are specified in
// ctd_schur_cr_kernels.hpp.  Strict rounding (the Makefile compiles this file with -ffp-contract=off): results are reproducible bit
// for bit.
#include <type_traits>

#include "ctd_common.hpp"
#include "ctd_schur_cr_joint_kernels.hpp"
#include "ctd_schur_cr_kernels.hpp"

namespace ctd {
namespace {

constexpr int kWave = 64;
constexpr int64_t kCrMaxGrid = 1 << 16;     // cap of a level's workgroup count (grid-stride: it does not enter any result)

// FP / SP (the kernels below): the argument struct, SchurCrFactorParams / SchurCrSolveParams or their shard forms
// (ctd_schur_cr_kernels.hpp), which add the global index of block 0 -- word 4 of the header -- and the place of the partial sums.
// The instantiations for the whole-grid structs compile to the code without them
template <class P> constexpr bool is_joint() {
    return std::is_same<P, SchurCrJointFactorParams>::value || std::is_same<P, SchurCrJointSolveParams>::value;
}
template <class P> constexpr bool is_shard() {
    return std::is_same<P, SchurCrShardFactorParams>::value || std::is_same<P, SchurCrShardSolveParams>::value || is_joint<P>();
}
// ... and of the joined form (ctd_schur_cr_joint_kernels.hpp): the interior of a rank under that family's tag, with the identity of
// the rank in the words 5 .. 8 of the header
template <class P> __device__ __forceinline__ bool joint_id_ok(const int64_t* head, const P& p) {
    return head[5] == p.id.sb && head[6] == p.id.se && head[7] == p.id.n_ranks && head[8] == p.id.rank;
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
        if constexpr (is_joint<FP>()) {
            head[0] = kSchurCrJointTag;
            head[5] = fp.id.sb;
            head[6] = fp.id.se;
            head[7] = fp.id.n_ranks;
            head[8] = fp.id.rank;
        }
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
    if (head[0] != (is_joint<SP>() ? kSchurCrJointTag : kSchurCrTag) || head[1] != sp.N || head[2] != sp.m || head[3] != sp.n_levels) return false;
    if constexpr (is_shard<SP>())
        if (head[4] != sp.first) return false;
    if constexpr (is_joint<SP>())
        if (!joint_id_ok(head, sp)) return false;
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

#ifdef CTD_SCHUR_CR_JOINT
// ---- the joined form: interface, spikes, contributions, the reduced system, the correction (ctd_schur_cr_joint_kernels.hpp) ----------
// Compiled in a translation unit of its own (ctd_schur_cr_joint.hip defines CTD_SCHUR_CR_JOINT and includes this file), so that this
// file alone holds exactly the kernels it held before the joined form and they compile to the instructions they had
struct JointWs {
    int64_t* rstatus;
    double *Es, *Eb, *Ds, *Wl, *Wr, *srhs, *sy, *RL, *RF, *rs, *xs, *sigma;
};
__device__ __forceinline__ int64_t joint_n_sep(const SchurCrJointParams& p) { return p.id.n_ranks > 1 ? p.id.n_ranks - 1 : 1; }
__device__ __forceinline__ JointWs joint_ws(const SchurCrJointParams& p) {
    const int64_t mm = (int64_t)p.m * p.m, n_sep = joint_n_sep(p);
    JointWs w;
    w.Es = p.ws + p.off_es;
    w.Eb = p.ws + p.off_eb;
    w.Ds = p.ws + p.off_ds;
    w.Wl = p.ws + p.off_wl;
    w.Wr = p.ws + p.off_wr;
    w.srhs = p.ws + p.off_scratch;
    w.sy = w.srhs + 2 * p.n_int * mm;
    w.rstatus = (int64_t*)(p.ws + p.off_reduced);
    w.RL = p.ws + p.off_reduced + n_sep;
    w.RF = w.RL + n_sep * mm;
    w.rs = p.ws + p.off_rs;
    w.xs = p.ws + p.off_xs;
    w.sigma = p.ws + p.off_sigma;
    return w;
}
// uniform: whether this launch stores anything (the header of the rank's own local factor; in iteration mode the freeze)
__device__ __forceinline__ bool joint_go(const SchurCrJointParams& p) {
    const int64_t* head = (const int64_t*)p.ws;
    if (head[0] != kSchurCrJointTag || head[1] != p.n_int || head[2] != p.m || head[3] != p.n_levels || head[4] != p.int_begin) return false;
    if (!joint_id_ok(head, p)) return false;
    return p.mode != SCHUR_ITER || p.cur->status == KRYLOV_RUNNING;
}
__device__ __forceinline__ bool joint_left(const SchurCrJointParams& p) { return p.id.rank > 0; }
__device__ __forceinline__ bool joint_right(const SchurCrJointParams& p) { return p.id.rank < p.id.n_ranks - 1; }

// the entry T(row ra, row rb) of the assemble launch above, on the grid's own (not offset) arrays
__device__ __forceinline__ double joint_entry(const SchurCrJointParams& p, int64_t ra, int64_t rb, bool diag) {
    double s = 0.0;
    int64_t pa = p.rowptr[ra], pb = p.rowptr[rb];
    const int64_t ea = p.rowptr[ra + 1], eb = p.rowptr[rb + 1];
    while (pa < ea && pb < eb) {
        const int64_t ca = p.colind[pa], cb = p.colind[pb];
        if (ca >= p.v_off || cb >= p.v_off) break;
        if (ca == cb) {
            s += (p.jvals[pa] * p.jvals[pb]) * (1.0 / p.px[ca]);
            ++pa;
            ++pb;
        } else if (ca < cb) ++pa;
        else ++pb;
    }
    if (diag && p.sc) s += p.sc[ra];
    return s;
}

// INTERFACE: one thread per entry of D_s, E[s], E[b]; the rest of the workspace behind the interior's part is zeroed (the status
// words of the reduced factor: -1)
__global__ void __launch_bounds__(256) schur_cr_joint_interface_kernel(const SchurCrJointParams p) {
    const int64_t m = p.m, mm = m * m, n_sep = joint_n_sep(p);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const JointWs w = joint_ws(p);
    for (int64_t e = p.off_wl + tid; e < p.workspace; e += stride)
        if (e < p.off_reduced || e >= p.off_reduced + n_sep) p.ws[e] = 0.0;
    for (int64_t e = tid; e < n_sep; e += stride) w.rstatus[e] = -1;
    const int64_t sb = p.id.sb, se = p.id.se;
    for (int64_t e = tid; e < 3 * mm; e += stride) {
        const int which = (int)(e / mm);
        const int64_t q = e - which * mm, a = q / m, b = q - a * m;
        double v = 0.0;
        if (which == 0 && joint_left(p)) v = joint_entry(p, sb * m + a, sb * m + b, a == b);
        if (which == 1 && joint_left(p)) v = joint_entry(p, (sb + 1) * m + a, sb * m + b, false);
        if (which == 2 && joint_right(p)) v = joint_entry(p, se * m + a, (se - 1) * m + b, false);
        (which == 0 ? w.Ds : (which == 1 ? w.Es : w.Eb))[q] = v;
    }
}

// a column of the spikes: its right-hand side, its scratch and where its solution goes.  Column cc of the launch: cc < m is column
// cc of Wl, cc >= m column cc - m of Wr
struct SpikeCol {
    const double *Es, *Eb;
    double *rhs, *y, *W;
    int64_t N;
    int m, c;
    bool left;
    __device__ __forceinline__ double first(int64_t k, int a) const {
        return left ? (k == 0 ? Es[a * m + c] : 0.0) : (k == N - 1 ? Eb[c * m + a] : 0.0);
    }
    __device__ __forceinline__ double& out(int64_t k, int a) const { return W[(k * m + a) * (int64_t)m + c]; }
};
__device__ __forceinline__ SpikeCol spike_col(const SchurCrJointParams& p, const JointWs& w) {
    const int cc = (joint_left(p) ? 0 : p.m) + (int)blockIdx.y;
    SpikeCol s;
    s.Es = w.Es;
    s.Eb = w.Eb;
    s.N = p.n_int;
    s.m = p.m;
    s.left = cc < p.m;
    s.c = s.left ? cc : cc - p.m;
    s.rhs = w.srhs + cc * p.n_int * p.m;
    s.y = w.sy + cc * p.n_int * p.m;
    s.W = s.left ? w.Wl : w.Wr;
    return s;
}

// DOWN / ROOT / UP of the solve above for the columns of the spikes: blockIdx.y is the column, a wave does what the wave of the
// single solve does
template <int MB> __global__ void __launch_bounds__(kWave) schur_cr_joint_down_kernel(const SchurCrJointParams p, const int64_t h) {
    __shared__ CrLds<MB> s;
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m;
    const int64_t mm = (int64_t)m * m, N = p.n_int;
    const bool row = lane < m;
    const CrWs w = cr_ws(p.ws, N, m);
    const SpikeCol col = spike_col(p, joint_ws(p));
    auto src = [&](int64_t k) { return h == 1 ? col.first(k, lane) : col.rhs[k * m + lane]; };
    const int64_t active = (N + h - 1) / h;
    for (int64_t q = blockIdx.x; q < active; q += gridDim.x) {
        const int64_t k = q * h;
        if (q & 1) {
            cr_stage_L(s, w.D + k * mm, m, lane);
            const double y = cr_forward(s, row ? src(k) : 0.0, m, lane);
            if (row) col.y[k * m + lane] = y;
            continue;
        }
        double g = row ? src(k) : 0.0;
        if (k >= h) {
            const int64_t i = k - h;
            cr_stage_L(s, w.D + i * mm, m, lane);
            const double y = cr_forward(s, row ? src(i) : 0.0, m, lane);
            g = g - cr_matvec<MB, false>(s, w.E + i * mm, y, m, lane);
        }
        if (k + h < N) {
            const int64_t i = k + h;
            cr_stage_L(s, w.D + i * mm, m, lane);
            const double y = cr_forward(s, row ? src(i) : 0.0, m, lane);
            g = g - cr_matvec<MB, true>(s, w.Gm + i * mm, y, m, lane);
        }
        if (row) col.rhs[k * m + lane] = g;
    }
}
template <int MB> __global__ void __launch_bounds__(kWave) schur_cr_joint_root_kernel(const SchurCrJointParams p) {
    __shared__ CrLds<MB> s;
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m;
    const CrWs w = cr_ws(p.ws, p.n_int, m);
    const SpikeCol col = spike_col(p, joint_ws(p));
    cr_stage_L(s, w.D, m, lane);
    double g = cr_forward(s, lane < m ? (p.n_levels == 0 ? col.first(0, lane) : col.rhs[lane]) : 0.0, m, lane);
    g = cr_backward(s, g, m, lane);
    if (lane < m) col.out(0, lane) = g;
}
template <int MB> __global__ void __launch_bounds__(kWave) schur_cr_joint_up_kernel(const SchurCrJointParams p, const int64_t h) {
    __shared__ CrLds<MB> s;
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m;
    const int64_t mm = (int64_t)m * m, N = p.n_int;
    const bool row = lane < m;
    const CrWs w = cr_ws(p.ws, N, m);
    const SpikeCol col = spike_col(p, joint_ws(p));
    const int64_t count = N > h ? (N - h + 2 * h - 1) / (2 * h) : 0;
    for (int64_t q = blockIdx.x; q < count; q += gridDim.x) {
        const int64_t i = (2 * q + 1) * h;
        double g = row ? col.y[i * m + lane] : 0.0;
        g = g - cr_matvec<MB, false>(s, w.Gm + i * mm, row ? col.out(i - h, lane) : 0.0, m, lane);
        if (i + h < N) g = g - cr_matvec<MB, true>(s, w.E + i * mm, row ? col.out(i + h, lane) : 0.0, m, lane);
        cr_stage_L(s, w.D + i * mm, m, lane);
        g = cr_backward(s, g, m, lane);
        if (row) col.out(i, lane) = g;
    }
}

// CONTRIBUTIONS and the factor record: one thread per word of the record
__global__ void __launch_bounds__(256) schur_cr_joint_contrib_kernel(const SchurCrJointParams p) {
    if (!joint_go(p)) return;
    const int64_t m = p.m, mm = m * m, last = (p.n_int - 1) * mm;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const JointWs w = joint_ws(p);
    for (int64_t e = tid; e < kSchurJointHead + 4 * mm; e += stride) {
        if (e < kSchurJointHead) {
            ((int64_t*)p.send)[e] = e == 0 ? p.id.sb : (e == 1 ? p.id.se : (e == 2 ? m : (e == 3 ? (int64_t)p.id.rank : 0)));
            continue;
        }
        const int which = (int)((e - kSchurJointHead) / mm);
        const int64_t q = e - kSchurJointHead - which * mm, i = q / m, j = q - i * m;
        double s = 0.0;
        if (which == 0) s = w.Ds[q];
        else if (which == 1)
            for (int64_t t = 0; t < m; ++t) s += w.Es[t * m + i] * w.Wl[t * m + j];
        else if (which == 2)
            for (int64_t t = 0; t < m; ++t) s += w.Eb[i * m + t] * w.Wl[last + t * m + j];
        else
            for (int64_t t = 0; t < m; ++t) s += w.Eb[i * m + t] * w.Wr[last + t * m + j];
        p.send[e] = s;
    }
}

// JOIN of the factor: the reduced matrix from the gathered records and its block Cholesky sweep, one wave
template <int MB> __global__ void __launch_bounds__(kWave) schur_cr_joint_reduce_kernel(const SchurCrJointParams p) {
    __shared__ double lds[3 * MB * MB + MB];
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m, mm = m * m, G = p.id.n_ranks, n = G - 1;
    const JointWs w = joint_ws(p);
    bool ok = true;
    int64_t prev = 0;
    for (int r = 0; r < G; ++r) {                // (every lane reads the same words: uniform)
        const int64_t* rec = (const int64_t*)(p.gathered + r * p.slot);
        if (rec[0] != prev || rec[1] <= rec[0] || rec[2] != m || rec[3] != r) ok = false;
        if (r == p.id.rank && (rec[0] != p.id.sb || rec[1] != p.id.se)) ok = false;
        prev = rec[1];
    }
    if (prev != p.N) ok = false;
    if (!ok) {
        for (int k = 0; k < n; ++k) {
            fill_nan(w.RL + (int64_t)k * mm, mm, lane);
            fill_nan(w.RF + (int64_t)k * mm, mm, lane);
            if (lane == 0) w.rstatus[k] = 0;
        }
        return;
    }
    double* A = lds;
    double* Eb = lds + MB * MB;
    double* Fp = lds + 2 * MB * MB;
    double* dinv = lds + 3 * MB * MB;
    int64_t bad = -1;
    for (int k = 0; k < n; ++k) {
        const double* own = p.gathered + (k + 1) * p.slot + kSchurJointHead;
        const double* lft = p.gathered + k * p.slot + kSchurJointHead;
        __syncthreads();                         // the previous block's reads of A, Eb, Fp are done
        for (int e = lane; e < mm; e += kWave) {
            A[e] = (own[e] - lft[3 * mm + e]) - own[mm + e];
            Eb[e] = k + 1 < n ? -own[2 * mm + e] : 0.0;
        }
        __syncthreads();
        if (bad < 0) {
            if (k > 0) {
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
                    for (int q = 0; q < j; ++q) s -= A[lane * m + q] * A[j * m + q];
                    A[lane * m + j] = s;
                }
                __syncthreads();
                const double d = A[j * m + j];
                if (!(d > 0.0) || !__builtin_isfinite(d)) {     // (every lane reads the same word: the exit is uniform)
                    bad = ((const int64_t*)(p.gathered + (k + 1) * p.slot))[0];      // the separator's global block index
                    break;
                }
                __syncthreads();                 // every lane has read the pivot before lane j replaces it by its root
                const double dj = sqrt(d), rj = 1.0 / dj;
                if (lane == j) {
                    A[j * m + j] = dj;
                    dinv[j] = rj;
                } else if (lane > j && lane < m) A[lane * m + j] = A[lane * m + j] * rj;
                __syncthreads();
            }
        }
        if (lane == 0) w.rstatus[k] = bad;
        if (bad >= 0) {
            fill_nan(w.RL + (int64_t)k * mm, mm, lane);
            fill_nan(w.RF + (int64_t)k * mm, mm, lane);
            continue;
        }
        if (lane < m) {
            for (int j = 0; j < m; ++j) {
                double s = Eb[lane * m + j];
                for (int q = 0; q < j; ++q) s -= Eb[lane * m + q] * A[j * m + q];
                Eb[lane * m + j] = s * dinv[j];
            }
        }
        __syncthreads();
        for (int e = lane; e < mm; e += kWave) {
            const int a = e / m, b = e - a * m;
            w.RL[(int64_t)k * mm + e] = b <= a ? A[e] : 0.0;
            w.RF[(int64_t)k * mm + e] = Eb[e];
        }
        double* t = Eb;                          // F_k is the next block's F_{k-1}
        Eb = Fp;
        Fp = t;
    }
}

// THE SOLVE RECORD: one wave
__global__ void __launch_bounds__(kWave) schur_cr_joint_record_kernel(const SchurCrJointParams p) {
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m;
    const JointWs w = joint_ws(p);
    const bool left = joint_left(p) && lane < m, right = joint_right(p) && lane < m;
    if (lane < kSchurJointHead) ((int64_t*)p.send)[lane] = lane == 0 ? p.id.rank : 0;
    double qu = 0.0, qd = 0.0;
    if (left) {
        const double* g = p.out + p.int_begin * m;
        for (int t = 0; t < m; ++t) qu += w.Es[t * m + lane] * g[t];
    }
    if (right) {
        const double* g = p.out + (p.id.se - 1) * m;
        for (int t = 0; t < m; ++t) qd += w.Eb[lane * m + t] * g[t];
    }
    double* v = p.send + kSchurJointHead;
    v[lane] = left ? p.r[p.id.sb * m + lane] : 0.0;
    v[kSchurMaxBlock + lane] = qu;
    v[2 * kSchurMaxBlock + lane] = qd;
}

// REDUCED SOLVE: rs~ from the gathered records, the two sweeps, sigma; one wave
template <int MB> __global__ void __launch_bounds__(kWave) schur_cr_joint_reduced_solve_kernel(const SchurCrJointParams p) {
    __shared__ CrLds<MB> s;
    if (!joint_go(p)) return;
    const int lane = threadIdx.x, m = p.m, n = p.id.n_ranks - 1;
    const int64_t mm = (int64_t)m * m;
    const bool row = lane < m;
    const JointWs w = joint_ws(p);
    double t = 0.0;
    for (int k = 0; k < n; ++k) {
        const double* own = p.gathered + (k + 1) * p.slot + kSchurJointHead;
        const double* lft = p.gathered + k * p.slot + kSchurJointHead;
        double g = row ? (own[lane] - lft[2 * kSchurMaxBlock + lane]) - own[kSchurMaxBlock + lane] : 0.0;
        if (row) w.rs[k * m + lane] = g;
        if (k > 0) g = g - cr_matvec<MB, false>(s, w.RF + (k - 1) * mm, t, m, lane);
        cr_stage_L(s, w.RL + k * mm, m, lane);
        t = cr_forward(s, g, m, lane);
        if (row) w.xs[k * m + lane] = t;
    }
    double x = 0.0;
    for (int k = n - 1; k >= 0; --k) {
        double g = row ? w.xs[k * m + lane] : 0.0;           // (this lane's own store)
        if (k + 1 < n) g = g - cr_matvec<MB, true>(s, w.RF + k * mm, x, m, lane);
        cr_stage_L(s, w.RL + k * mm, m, lane);
        x = cr_backward(s, g, m, lane);
        if (row) w.xs[k * m + lane] = x;
    }
    __syncthreads();                             // the wave's stores to xs and rs~ are visible to lane 0
    if (lane == 0) {
        double sg = 0.0;
        for (int64_t e = 0; e < (int64_t)n * m; ++e) sg += w.xs[e] * w.rs[e];
        w.sigma[0] = sg;
    }
}

// CORRECTION: one thread per row of the rank's blocks
__global__ void __launch_bounds__(256) schur_cr_joint_correct_kernel(const SchurCrJointParams p) {
    if (!joint_go(p)) return;
    const int64_t m = p.m, mm = m * m, sb = p.id.sb, rows = (p.id.se - sb) * m;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const JointWs w = joint_ws(p);
    const bool left = joint_left(p), right = joint_right(p);
    const double* xl = w.xs + (int64_t)(p.id.rank - 1) * m;      // (read when left)
    const double* xr = w.xs + (int64_t)p.id.rank * m;            // (read when right)
    for (int64_t e = tid; e < rows; e += stride) {
        const int64_t k = e / m, i = e - k * m;
        if (left && k == 0) {
            p.out[sb * m + i] = xl[i];
            continue;
        }
        const int64_t kk = k - (left ? 1 : 0);
        double v = p.out[sb * m + e];
        if (left) {
            const double* wl = w.Wl + kk * mm + i * m;
            double s1 = 0.0;
            for (int64_t j = 0; j < m; ++j) s1 += wl[j] * xl[j];
            v = v - s1;
        }
        if (right) {
            const double* wr = w.Wr + kk * mm + i * m;
            double s2 = 0.0;
            for (int64_t j = 0; j < m; ++j) s2 += wr[j] * xr[j];
            v = v - s2;
        }
        p.out[sb * m + e] = v;
    }
}
#endif  // CTD_SCHUR_CR_JOINT

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

#ifndef CTD_SCHUR_CR_JOINT
hipError_t schur_cr_factor(const SchurCrFactorParams& fp, hipStream_t st) { return cr_factor(fp, st); }
hipError_t schur_cr_solve(const SchurCrSolveParams& sp, hipStream_t st) { return cr_solve(sp, st); }
hipError_t schur_cr_factor(const SchurCrShardFactorParams& fp, hipStream_t st) { return cr_factor(fp, st); }
hipError_t schur_cr_solve(const SchurCrShardSolveParams& sp, hipStream_t st) {
    if (sp.mode != SCHUR_PLAIN && !sp.part) return hipErrorInvalidValue;
    return cr_solve(sp, st);
}

#else
// ---- the joined form ---------------------------------------------------------------------------------------------------------------
hipError_t schur_cr_factor(const SchurCrJointFactorParams& fp, hipStream_t st) { return cr_factor(fp, st); }
hipError_t schur_cr_solve(const SchurCrJointSolveParams& sp, hipStream_t st) {
    if (sp.mode != SCHUR_PLAIN && !sp.part) return hipErrorInvalidValue;
    return cr_solve(sp, st);
}
namespace {
bool joint_ok(const SchurCrJointParams& p) {
    return p.n_int >= 1 && p.m >= 1 && p.m <= kSchurMaxBlock && p.n_levels == schur_cr_levels(p.n_int) && p.id.n_ranks >= 1 &&
           p.id.n_ranks <= kSchurJointMaxRanks && p.id.rank >= 0 && p.id.rank < p.id.n_ranks && p.ws;
}
}  // namespace
hipError_t schur_cr_joint_interface(const SchurCrJointParams& p, hipStream_t st) {
    if (!joint_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(schur_cr_joint_interface_kernel, dim3(cr_grid_threads(p.workspace - p.off_wl)), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t schur_cr_joint_spikes(const SchurCrJointParams& p, hipStream_t st) {
    if (!joint_ok(p) || p.id.n_ranks < 2 || !p.send) return hipErrorInvalidValue;
    const unsigned cols = (unsigned)((p.id.rank > 0 ? p.m : 0) + (p.id.rank < p.id.n_ranks - 1 ? p.m : 0));
    const hipError_t e = for_block_size(p.m, [&](auto mb) {
        constexpr int MB = decltype(mb)::value;
        for (int l = 0; l < p.n_levels; ++l) {
            const int64_t h = (int64_t)1 << l;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_joint_down_kernel<MB>), dim3(cr_grid((p.n_int + h - 1) / h), cols), dim3(kWave), 0, st, p, h);
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return le;
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_joint_root_kernel<MB>), dim3(1, cols), dim3(kWave), 0, st, p);
        hipError_t le = hipGetLastError();
        if (le != hipSuccess) return le;
        for (int l = p.n_levels - 1; l >= 0; --l) {
            const SchurCrLevel lv = schur_cr_level(p.n_int, l);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_joint_up_kernel<MB>), dim3(cr_grid(lv.count), cols), dim3(kWave), 0, st, p, lv.first);
            le = hipGetLastError();
            if (le != hipSuccess) return le;
        }
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(schur_cr_joint_contrib_kernel, dim3(cr_grid_threads(kSchurJointHead + 4 * (int64_t)p.m * p.m)), dim3(256), 0, st, p);
    return hipGetLastError();
}
hipError_t schur_cr_joint_factor_join(const SchurCrJointParams& p, hipStream_t st) {
    if (!joint_ok(p) || p.id.n_ranks < 2 || !p.gathered || p.slot < kSchurJointHead + 4 * (int64_t)p.m * p.m) return hipErrorInvalidValue;
    return for_block_size(p.m, [&](auto mb) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_joint_reduce_kernel<decltype(mb)::value>), dim3(1), dim3(kWave), 0, st, p);
        return hipGetLastError();
    });
}
hipError_t schur_cr_joint_solve_record(const SchurCrJointParams& p, hipStream_t st) {
    if (!joint_ok(p) || p.id.n_ranks < 2 || !p.send || !p.r || !p.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(schur_cr_joint_record_kernel, dim3(1), dim3(kWave), 0, st, p);
    return hipGetLastError();
}
hipError_t schur_cr_joint_solve_join(const SchurCrJointParams& p, hipStream_t st) {
    if (!joint_ok(p) || p.id.n_ranks < 2 || !p.gathered || p.slot < kSchurJointSolveSlot || !p.out) return hipErrorInvalidValue;
    const hipError_t e = for_block_size(p.m, [&](auto mb) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(schur_cr_joint_reduced_solve_kernel<decltype(mb)::value>), dim3(1), dim3(kWave), 0, st, p);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(schur_cr_joint_correct_kernel, dim3(cr_grid_threads((p.id.se - p.id.sb) * p.m)), dim3(256), 0, st, p);
    return hipGetLastError();
}
#endif  // CTD_SCHUR_CR_JOINT

}  // namespace ctd
