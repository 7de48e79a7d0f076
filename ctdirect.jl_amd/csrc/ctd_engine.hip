// ctd_engine.hip -- handle, device buffers, launches and the extern "C" entry points of include/ctdirect_hip.h.
//
// There is no CPU compute path in this library: every hot-path entry point launches the HIP kernels of
// ctd_kernels.hpp on the handle's device and fails with CTD_ENODEVICE when the handle has none.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>

#include <cstdio>
#include <functional>
#include <map>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/ctdirect_hip.h"
#include "ctd_host.hpp"
#include "ctd_kernels.hpp"
#include "ctd_hess_kernels.hpp"
#include "ctd_hess_step.hpp"
#include "ctd_iter_kernels.hpp"
#include "ctd_prod_kernels.hpp"
#include "ctd_hprod_kernels.hpp"
#include "ctd_kkt_kernels.hpp"
#include "ctd_diag_kernels.hpp"
#include "ctd_krylov_kernels.hpp"
#include "ctd_krylov_shard_kernels.hpp"
#include "ctd_schur_cr_joint_kernels.hpp"
#include "ctd_schur_cr_kernels.hpp"
#include "ctd_schur_kernels.hpp"
#include "ctd_jit.hpp"

using namespace ctd;

namespace ctd {
// the instantiations live in the per-problem translation units
#define CTD_EXTERN_ALL(ID, P) \
    CTD_EXTERN_LAUNCHERS(P) CTD_EXTERN_HESS(P) CTD_EXTERN_HESS_STEP(P) CTD_EXTERN_ITER(P) CTD_EXTERN_PROD(P) CTD_EXTERN_HPROD(P) CTD_EXTERN_KKT(P) CTD_EXTERN_DIAG(P)
CTD_REGISTRY(CTD_EXTERN_ALL)
}  // namespace ctd

// A device array the handle owns and frees when it is deleted; cap: the elements allocated.  ensure(n): at least n elements,
// allocated when the array is smaller (at first use: static tables, host-call staging and the partial sums of calls that are
// never captured); grow (below): the partial sums of the capturable calls.
template <class T = double> struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t ensure(int64_t n) {
        if (p && n <= cap) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void**)&p, sizeof(T) * (size_t)(n > 1 ? n : 1));      // (one element at least: never a null output)
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    int32_t grow(ctd_handle* h, int64_t need, const char* fn);
};

// the kernel families of a run-time OCP (ctd_register_ocp): one hiprtc module each -- two for the matrix-free families, whose
// shard form is a module of its own -- loaded at first use (jit_load)
enum JitFamily { JIT_FIRST, JIT_BATCH, JIT_PROD, JIT_HPROD, JIT_HESS, JIT_KKT, JIT_DIAG, kJitFamilies };
struct JitModule {
    hipModule_t mod = nullptr;
    hipFunction_t f[5] = {};        // in the order of the family's name expressions (kJit)
};

struct ctd_handle {
    Model model;
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t step_begin = 0, step_end = 0;
    LaunchPlan plan;            // constraint / Jacobian kernel (plan_cons_jac): plan.kp with the device pointers filled in, outputs set per call
    // static device data
    DevBuf<double> d_tau;
    DevBuf<uint32_t> d_tmpl, d_vtmpl;
    DevBuf<uint16_t> d_pos;
    DevBuf<int64_t> d_edge_idx;
    DevBuf<uint32_t> d_edge_code;
    // staging for the host-pointer entry points
    DevBuf<> d_x, d_c, d_vals;
    // objective
    DevBuf<> d_partial;         // per-workgroup partial sums (batched calls: one set per member)
    DevBuf<> d_obj;
    DevBuf<> d_g;               // staging for ctd_grad (host pointers)
    DevBuf<> d_gpartial;        // per-workgroup partial sums of dg/dv
    int obj_blocks = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // run-time defined OCP (ctd_register_ocp): kernels compiled with hiprtc and launched through the module API
    const RtOcp* rt = nullptr;
    JitModule jit[kJitFamilies][2];     // [family][shard form]
    // Hessian of the Lagrangian: tables are uploaded by the first Hessian call (hess_ready)
    bool hess_ready = false;
    HParams hp;
    int hess_tile = 0;
    size_t hess_lds_bytes = 0;
    DevBuf<uint32_t> d_htptr, d_hterms, d_hvptr, d_hvterms, d_heptr, d_hevptr, d_heterms;
    DevBuf<int64_t> d_hedge_idx;
    DevBuf<double> d_hpair_c;
    DevBuf<uint32_t> d_hcpos, d_hzpos;
    // lane-per-step Hessian kernel (ctd_hess_step.hpp): position tables, parameters, the tile kernel's parameters for its edge blocks
    DevBuf<int32_t> d_hssrc, d_hschunk;
    DevBuf<double> d_hsck;
    bool hess_step = false;
    SParams sp{};
    HParams hp_step{};
    size_t hess_step_lds = 0;
    DevBuf<uint32_t> d_htasks, d_hptasks, d_hbtasks;
    DevBuf<> d_hpartials, d_y, d_hvals;
    // sharded iterate read in place (ctd_set_x_shards): device table of the other shards' buffers, host copy of what it holds
    DevBuf<XHalo> d_halo;
    XHalo halo_host{};
    // ctd_stitch_c: padded send block and gathered blocks
    DevBuf<> d_stitch_send, d_stitch_recv;
    // batched callbacks (ctd_*_batch_dev_async): doubles of Hessian partial sums per member -- the partial-sum buffers grow with
    // the batch
    int64_t hpart_member = 0;
    // matrix-free Jacobian products (ctd_jprod*, ctd_jtprod*): per-workgroup partial sums of d/dv, host-call staging of the
    // direction and the product (nvar / ncon entries: nothing proportional to nnzj)
    DevBuf<> d_ppartial, d_pdir, d_pout;
    // matrix-free Hessian products (ctd_hprod*): their own partial sums (a graph captured over jtprod keeps its buffer), host-call
    // staging of v and Hv in d_pdir / d_pout and of y in d_y
    DevBuf<> d_hppartial;
    // matrix-free KKT products (ctd_kktprod*, the shard call included): their own partial sums again; the host call stages x, y, dx and rx as ctd_hprod does
    // and dy, sx, sc and rc here (nvar / ncon entries)
    DevBuf<> d_kktpartial, d_kdy, d_ksx, d_ksc, d_krc;
    // matrix-free KKT diagonals (ctd_hdiag*, ctd_jsq_cols*, the shard calls included; ctd_jsq_rows* has no reduction): a
    // partial-sum buffer per call, so a graph captured over any other product keeps its own; the host calls stage through d_x,
    // d_y, d_pdir and d_pout
    DevBuf<> d_hdpartial, d_jcpartial;
    // device-resident MINRES solve (ctd_kkt_minres*): the workspace of ctd_krylov_kernels.hpp (krylov_workspace(nvar + ncon) doubles),
    // the partial sums of its own kktprod launches (a graph captured over ctd_kktprod keeps its buffer), the host form's staging
    // of (px, pc), rhs and z; the iterate and the preconditioner flag of the solve started last (mr_z null: none yet)
    DevBuf<> d_mrws, d_mrkpartial, d_mrp, d_mrrhs, d_mrz;
    double* mr_z = nullptr;
    bool mr_precond = false;
    // chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur*): the CSR pattern on the device, uploaded by the first factor;
    // the pattern check of plan_kkt_schur passed (it is made once); the workspace of the factor the solve started last carries
    // (null: none, the diagonal or the plain solve) and its kind (mr_schur_cr: the log-depth exact form, ctd_kkt_schur_cr*)
    DevBuf<int64_t> d_schur_rowptr, d_schur_colind;
    bool schur_verified = false;
    double* mr_schur = nullptr;
    bool mr_schur_cr = false;
    std::string err;
};

// write-through stores of the Hessian kernel, as write_through (ctd_host.cpp) for the constraint / Jacobian kernel: outputs up to
// these many megabytes (gains up to ~10 MB, even at 16, losses from ~80)
constexpr double kHessWtMB = 16.0;

static thread_local std::string g_create_err;      // error of this thread's last failed handle-less call (ctd_last_error(NULL))

static int32_t fail(ctd_handle* h, int32_t code, const std::string& msg) {
    if (h) h->err = msg; else g_create_err = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(h, CTD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// The end of every enqueue: a launch that failed is CTD_EHIP, named by the entry point that was called (fn null: no name)
static int32_t launched(ctd_handle* h, const char* fn, hipError_t e) {
    if (e == hipSuccess) return CTD_OK;
    return fail(h, CTD_EHIP, (fn ? std::string(fn) + ": " : std::string()) + "kernel launch: " + hipGetErrorString(e));
}

// A struct of the caller's (`arg`: sys, info, layout): null, or laid out by another version of the header -- its struct_size is
// not sizeof(T) -- is CTD_EINVAL, set as the handle's error; false then
template <class T> static bool struct_ok(ctd_handle* h, const char* fn, const char* arg, const char* type, const T* p) {
    if (p && p->struct_size == sizeof(T)) return true;
    fail(h, CTD_EINVAL, std::string(fn) + ": " + arg + " is null or its struct_size is not sizeof(" + type + ") = " + std::to_string(sizeof(T)));
    return false;
}
#define STRUCT_OK(h, fn, arg, T, p) struct_ok<T>(h, fn, arg, #T, p)

// A device pointer the caller must give: null or not aligned to a double is CTD_EINVAL, by name
static int32_t check_ptr(ctd_handle* h, const char* fn, const char* name, const void* p) {
    if (!p) return fail(h, CTD_EINVAL, std::string(fn) + ": null argument (" + name + " is required)");
    if ((uintptr_t)p % sizeof(double)) return fail(h, CTD_EINVAL, std::string(fn) + ": " + name + " is not aligned to 8 bytes");
    return CTD_OK;
}
// [a, a + na) and [b, b + nb) share an entry (null: no range)
static bool ranges_overlap(const double* a, int64_t na, const double* b, int64_t nb) { return a && b && a < b + nb && b < a + na; }

// Every entry point that touches the device runs on the handle's device and leaves the caller's current device as it found
// it (a process driving several GPUs keeps its own notion of "current"); hipGetDevice is a thread-local read, and the
// hipSetDevice pair is only paid when the two differ.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    DeviceGuard() = default;
    explicit DeviceGuard(int dev) { (void)bind(dev); }
    hipError_t bind(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = (err == hipSuccess); }
        return err;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The prologue of every compute call: the handle, then its device -- a host-only handle is refused with CTD_ENODEVICE before
// any other check (the refusal starts with `fn` where given) -- then the handle's device is current until the end of the
// scope.  st: the first failure, CTD_OK if none.
struct OnDevice {
    DeviceGuard dg;
    int32_t st = CTD_OK;
    explicit OnDevice(ctd_handle* h, const char* fn = nullptr) {
        if (!h) st = CTD_EINVAL;
        else if (h->device < 0)
            st = fail(h, CTD_ENODEVICE, std::string(fn ? fn : "") + (fn ? ": " : "") +
                                            "compute call on a host-only handle (device = -1); there is no CPU fallback");
        else if (dg.bind(h->device) != hipSuccess) st = fail(h, CTD_EHIP, std::string("dg_.err: ") + hipGetErrorString(dg.err));
    }
};

// Grows a partial-sum buffer to `need` elements (batched calls: one set of partial sums per member).  The buffer may still be
// read by launches in flight, so the handle's stream is drained first -- which a capturing stream cannot do, and nothing may be
// allocated inside a capture either: the call is refused there.
template <class T> int32_t DevBuf<T>::grow(ctd_handle* h, int64_t need, const char* fn) {
    if (need <= cap && p) return CTD_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(h, CTD_EINVAL, std::string(fn) + ": this batch needs larger partial-sum buffers, which cannot be allocated while the "
                                   "stream is capturing; make one call with the same batch size before the capture");
    (void)hipGetLastError();
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, ensure(need));
    return CTD_OK;
}

template <class T> static hipError_t upload(DevBuf<T>& dst, const std::vector<T>& src) {
    dst.release();       // idempotent: a retry after a partial failure (ensure_hess) replaces, never leaks
    if (src.empty()) return hipSuccess;
    const hipError_t e = dst.ensure((int64_t)src.size());
    if (e != hipSuccess) return e;
    return hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

static int env_int(const char* name, int dflt) {
    const char* s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

// Frees the handle and what it holds on its device, on that device: the stream is drained first (enqueue-only calls may still be
// running on the buffers), the DevBufs free themselves with the handle
static void destroy_handle(ctd_handle* h) {
    DeviceGuard dg;
    if (h->device >= 0) {
        (void)dg.bind(h->device);
        (void)hipStreamSynchronize(h->stream);
        if (h->ev0) (void)hipEventDestroy(h->ev0);
        if (h->ev1) (void)hipEventDestroy(h->ev1);
        if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
        for (auto& fam : h->jit)
            for (JitModule& m : fam)
                if (m.mod) (void)hipModuleUnload(m.mod);
    }
    delete h;
}

// ---- run-time compilation of the kernel templates for a registered OCP -------------------------------------------------
namespace {
std::string jit_include_dir() {
    const char* env = std::getenv("CTD_JIT_INCLUDE");
    if (env && *env) return env;
    Dl_info info;
    if (dladdr((const void*)&destroy_handle, &info) && info.dli_fname) {
        std::string path(info.dli_fname);
        const size_t slash = path.find_last_of('/');
        return (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/csrc";
    }
    return "csrc";
}

std::mutex g_jit_mu;
std::map<std::string, std::pair<std::string, std::vector<std::string>>> g_jit_cache;   // key -> (code object, lowered names)

// compiles `header` + the OCP's functor for gfx950 and returns the code object and the lowered names of `exprs`
int32_t jit_compile(const RtOcp& ro, const char* header, const std::vector<std::string>& exprs, const char* fp_contract,
                    std::string& code, std::vector<std::string>& lowered, std::string& err) {
    std::string key = ro.name + "|" + std::to_string((size_t)&ro) + "|" + header;
    for (const std::string& e : exprs) key += "|" + e;
    // diagnostics: extra compiler options for the run-time kernels (e.g. CTD_JIT_EXTRA="-DCTD_ABL=2"), split at blanks
    std::vector<std::string> extra;
    if (const char* ex = std::getenv("CTD_JIT_EXTRA")) {
        std::string cur;
        for (const char* c = ex;; ++c) {
            if (*c == ' ' || *c == 0) { if (!cur.empty()) extra.push_back(cur); cur.clear(); if (*c == 0) break; }
            else cur += *c;
        }
        key += std::string("|") + ex;
    }
    {
        std::lock_guard<std::mutex> lk(g_jit_mu);
        auto it = g_jit_cache.find(key);
        if (it != g_jit_cache.end()) { code = it->second.first; lowered = it->second.second; return CTD_OK; }
    }
    const std::string src = std::string("#include \"") + header + "\"\n" + ro.functor_src;
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), "ctd_user_ocp.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        err = "hiprtcCreateProgram failed";
        return CTD_EHIP;
    }
    for (const std::string& e : exprs) (void)hiprtcAddNameExpression(prog, e.c_str());
    const std::string inc = "-I" + jit_include_dir();
    const std::string fpc = std::string("-ffp-contract=") + fp_contract;
    std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", fpc.c_str(), inc.c_str()};
    for (const std::string& e : extra) opts.push_back(e.c_str());
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (rc != HIPRTC_SUCCESS) {
        size_t ls = 0;
        (void)hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) (void)hiprtcGetProgramLog(prog, &log[0]);
        err = "run-time compilation of OCP '" + ro.name + "' failed: " + log.substr(0, 4000);
        (void)hiprtcDestroyProgram(&prog);
        return CTD_EHIP;
    }
    lowered.clear();
    for (const std::string& e : exprs) {
        const char* ln = nullptr;
        if (hiprtcGetLoweredName(prog, e.c_str(), &ln) != HIPRTC_SUCCESS || !ln) { err = "no lowered name for " + e; (void)hiprtcDestroyProgram(&prog); return CTD_EHIP; }
        lowered.emplace_back(ln);
    }
    size_t cs = 0;
    (void)hiprtcGetCodeSize(prog, &cs);
    code.assign(cs, '\0');
    (void)hiprtcGetCode(prog, &code[0]);
    (void)hiprtcDestroyProgram(&prog);
    std::lock_guard<std::mutex> lk(g_jit_mu);
    g_jit_cache[key] = {code, lowered};
    return CTD_OK;
}

// The name expressions of each family.  s: stages of a Gauss-Legendre scheme; for the midpoint scheme the controls per step
// (control_steps); sh: ", true" for the shard form of the matrix-free kernels (a module of its own, compiled by the first shard
// call), "" otherwise and for the families that have none
std::vector<std::string> jit_first_exprs(int sc, int s, const std::string&) {
    const std::string P = "ctd::UserOCP", a = std::to_string(sc), b = std::to_string((sc == SC_IRK || sc == SC_MIDPOINT) && s > 0 ? s : 1);
    return {"ctd::cons_jac_kernel<" + P + ", " + a + ", " + b + ", false>", "ctd::obj_partial_kernel<" + P + ", " + a + ">",
            "ctd::obj_finish_kernel<" + P + ">", "ctd::grad_units_kernel<" + P + ", " + a + ", " + b + ">",
            "ctd::grad_finish_kernel<" + P + ">"};
}
std::vector<std::string> jit_hess_exprs(int sc, int s, const std::string&) {
    const std::string P = "ctd::UserOCP", a = std::to_string(sc), b = std::to_string((sc == SC_IRK || sc == SC_MIDPOINT) && s > 0 ? s : 1);
    return {"ctd::hess_kernel<" + P + ", " + a + ", " + b + ", false>", "ctd::hess_finish_kernel<" + P + ">"};
}
std::vector<std::string> jit_batch_exprs(int sc, int s, const std::string&) {
    const std::string b = std::to_string((sc == SC_IRK || sc == SC_MIDPOINT) && s > 0 ? s : 1);
    return {"ctd::cons_jac_batch_kernel<ctd::UserOCP, " + std::to_string(sc) + ", " + b + ">"};
}
std::vector<std::string> prod_exprs(int sc, int s, const std::string& sh) {
    const std::string a = std::to_string(sc), b = std::to_string(sc == SC_IRK && s > 0 ? s : 1);
    return {"ctd::jprod_kernel<ctd::UserOCP, " + a + ", " + b + sh + ">", "ctd::jtprod_units_kernel<ctd::UserOCP, " + a + ", " + b + sh + ">",
            "ctd::jtprod_finish_kernel<ctd::UserOCP" + sh + ">"};
}
std::vector<std::string> hprod_exprs(int sc, int s, const std::string& sh) {
    const std::string a = std::to_string(sc), b = std::to_string(sc == SC_IRK && s > 0 ? s : 1);
    return {"ctd::hprod_units_kernel<ctd::UserOCP, " + a + ", " + b + sh + ">", "ctd::hprod_finish_kernel<ctd::UserOCP" + sh + ">"};
}
std::vector<std::string> kkt_exprs(int sc, int s, const std::string& sh) {
    const std::string a = std::to_string(sc), b = std::to_string(sc == SC_IRK && s > 0 ? s : 1);
    return {"ctd::kktprod_units_kernel<ctd::UserOCP, " + a + ", " + b + sh + ">", "ctd::kktprod_finish_kernel<ctd::UserOCP" + sh + ">"};
}
std::vector<std::string> diag_exprs(int sc, int s, const std::string& sh) {
    const std::string a = "<ctd::UserOCP, " + std::to_string(sc) + ", " + std::to_string(sc == SC_IRK && s > 0 ? s : 1) + sh + ">";
    return {"ctd::hdiag_units_kernel" + a, "ctd::hdiag_finish_kernel<ctd::UserOCP" + sh + ">", "ctd::jsq_cols_units_kernel" + a,
            "ctd::jsq_cols_finish_kernel<ctd::UserOCP" + sh + ">", "ctd::jsq_rows_kernel" + a};
}

// one row per JitFamily: the header, -ffp-contract, the name expressions
const struct { const char* header; const char* fp_contract; std::vector<std::string> (*exprs)(int sc, int s, const std::string& sh); }
kJit[kJitFamilies] = {
    {"ctd_kernels.hpp", "off", jit_first_exprs},        // cons_jac, obj_partial, obj_finish, grad_units, grad_finish
    {"ctd_kernels.hpp", "off", jit_batch_exprs},        // cons_jac_batch
    {"ctd_prod_kernels.hpp", "off", prod_exprs},        // jprod, jtprod_units, jtprod_finish
    {"ctd_hprod_kernels.hpp", "off", hprod_exprs},      // hprod_units, hprod_finish
    {"ctd_hess_kernels.hpp", "fast", jit_hess_exprs},   // hess, hess_finish
    {"ctd_kkt_kernels.hpp", "off", kkt_exprs},          // kktprod_units, kktprod_finish
    {"ctd_diag_kernels.hpp", "off", diag_exprs},        // hdiag_units, hdiag_finish, jsq_cols_units, jsq_cols_finish, jsq_rows
};

// batch: the grid's second dimension (members of a batched launch)
hipError_t jit_launch(hipFunction_t f, int grid, int block, size_t lds, hipStream_t st, void** args, hipEvent_t e0 = nullptr,
                      hipEvent_t e1 = nullptr, int batch = 1) {
    if (e0 || e1)
        return hipExtModuleLaunchKernel(f, (uint32_t)grid * (uint32_t)block, (uint32_t)batch, 1, (uint32_t)block, 1, 1, lds, st, args, nullptr, e0, e1, 0);
    return hipModuleLaunchKernel(f, (uint32_t)grid, (uint32_t)batch, 1, (uint32_t)block, 1, 1, (uint32_t)lds, st, args, nullptr);
}
}  // namespace

// The kernels of family `fam` of a run-time OCP, its shard form when `shard`: compiled (or taken from the cache) and loaded once,
// nothing for a registry problem.  The first family is loaded by ctd_create, whose errors go to ctd_last_error(NULL).
static int32_t jit_load(ctd_handle* h, JitFamily fam, bool shard = false) {
    JitModule& m = h->jit[fam][shard];
    if (!h->rt || m.mod) return CTD_OK;
    ctd_handle* eh = fam == JIT_FIRST ? nullptr : h;
    const Layout& L = h->model.L;
    std::string code, err;
    std::vector<std::string> names;
    const int32_t st = jit_compile(*h->rt, kJit[fam].header, kJit[fam].exprs(L.sc, L.sc == SC_MIDPOINT ? L.cs : L.s, shard ? ", true" : ""),
                                   kJit[fam].fp_contract, code, names, err);
    if (st) return fail(eh, st, err);
    hipError_t e = hipModuleLoadData(&m.mod, code.data());
    for (size_t i = 0; e == hipSuccess && i < names.size(); ++i) e = hipModuleGetFunction(&m.f[i], m.mod, names[i].c_str());
    if (e == hipSuccess) return CTD_OK;
    if (m.mod) (void)hipModuleUnload(m.mod);      // (loaded whole or not at all: a later call tries again)
    m = JitModule{};
    return fail(eh, CTD_EHIP, std::string(kJit[fam].header) + " module: " + hipGetErrorString(e));
}

// Workgroups of the handle's constraint / Jacobian kernel that one CU keeps resident, as the runtime computes it from the kernel's
// registers and `lds_bytes` of LDS at `block` lanes; 0: the query failed.  The Resident of the launch plan (plan_cons_jac) and
// ctd_launch_info's.  A registry problem is always asked about its GENERAL kernel (occupancy_cons_jac), also where the lean or
// the static-emit form is launched: the tile choices were measured with that answer.
static int resident_cons_jac(const ctd_handle* h, const KParams& kp, int block, size_t lds_bytes) {
    DeviceGuard dg(h->device);
    int per_cu = 0;
    if (dg.err == hipSuccess) {
        if (h->rt) { if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->jit[JIT_FIRST][0].f[0], block, lds_bytes) != hipSuccess) per_cu = 0; }
        else for_problem(h->model.problem, [&](auto tag) { per_cu = occupancy_cons_jac<typename decltype(tag)::type>(kp, block, lds_bytes); });
    }
    (void)hipGetLastError();
    return per_cu;
}

// A host array of a host-pointer call and the handle's buffer that stages it: n doubles (a null host pointer is not staged)
template <class T> struct Staged { T* host; DevBuf<>& buf; int64_t n; };

// The host-pointer entry points, after their prologue and checks: the staging buffers allocated at first use, the inputs copied
// in, the enqueue, the outputs copied back -- every copy on the handle's stream -- and one synchronisation
template <class Enqueue>
static int32_t host_call(ctd_handle* h, std::initializer_list<Staged<const double>> in, Enqueue&& enqueue,
                         std::initializer_list<Staged<double>> out) {
    for (const auto& a : in) if (a.host) HIP_TRY(h, a.buf.ensure(a.n));
    for (const auto& a : out) if (a.host) HIP_TRY(h, a.buf.ensure(a.n));
    for (const auto& a : in) if (a.host) HIP_TRY(h, hipMemcpyAsync(a.buf.p, a.host, sizeof(double) * a.n, hipMemcpyHostToDevice, h->stream));
    if (const int32_t st = enqueue()) return st;
    for (const auto& a : out) if (a.host) HIP_TRY(h, hipMemcpyAsync(a.host, a.buf.p, sizeof(double) * a.n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CTD_OK;
}

// ---- the matrix-free operators: one row each -----------------------------------------------------------------------------
// The three entry points of an operator: host pointers (ctd_X), device pointers (ctd_X_dev_async), device pointers on a shard of the
// grid (ctd_X_shard_dev_async)
enum MfForm { MF_HOST, MF_DEV, MF_SHARD };
// name: the entry points by MfForm; fam, f0: the kernels of a run-time OCP -- f[f0] of the family's module, and f[f0 + 1] unless
// one_launch: then there is no finish kernel; dir_ncon / out_ncon: the direction (v, w, dx, the weights) / the first output has
// ncon entries, not nvar (what the host form stages); required, outs: the pointers that must not be null and the outputs, as
// the messages name them
struct MfOp {
    const char* name[3];
    JitFamily fam;
    int f0;
    bool one_launch, dir_ncon, out_ncon;
    const char *required, *outs;
};
#define CTD_MF_OP(X, ...) {{"ctd_" #X, "ctd_" #X "_dev_async", "ctd_" #X "_shard_dev_async"}, __VA_ARGS__}
static constexpr MfOp kJprod = CTD_MF_OP(jprod, JIT_PROD, 0, true, false, true, "x, v and Jv", "Jv"),
                      kJtprod = CTD_MF_OP(jtprod, JIT_PROD, 1, false, true, false, "x, w and Jtw", "Jtw"),
                      kHprod = CTD_MF_OP(hprod, JIT_HPROD, 0, false, false, false, "x, v and Hv", "Hv"),
                      kKktprod = CTD_MF_OP(kktprod, JIT_KKT, 0, false, false, false, "x, dx, dy, rx and rc", "rx and rc"),
                      kHdiag = CTD_MF_OP(hdiag, JIT_DIAG, 0, false, false, false, "x and Hd", "Hd"),
                      kJsqCols = CTD_MF_OP(jsq_cols, JIT_DIAG, 2, false, true, false, "x and out", "out"),
                      kJsqRows = CTD_MF_OP(jsq_rows, JIT_DIAG, 4, true, false, true, "x and out", "out");
#undef CTD_MF_OP
// One call of an operator: every message carries fn(), the entry point that was called
struct MfCall {
    const MfOp& op;
    MfForm form;
    const char* fn() const { return op.name[form]; }
    bool shard() const { return form == MF_SHARD; }
    int32_t launched(ctd_handle* h, hipError_t e) const { return ::launched(h, fn(), e); }
};

// The directions a lane of a unit pass takes together: D<P>::JC of a registry problem, the same rule for a run-time OCP
template <template <class> class D>
static int prod_chunk(const ctd_handle* h, int (*rule)(int n, int dc)) {
    int jc = 1;
    if (h->rt) jc = rule(h->rt->info.n, h->rt->dc);
    for_problem(h->model.problem, [&](auto tag) { jc = D<typename decltype(tag)::type>::JC; });
    return jc;
}

// An operator of one launch (jprod, jsq_rows): f[f0] of the run-time OCP's module over the call's nodes, or launch(tag, SH) -- the
// launcher of registry problem `tag`, SH a std::bool_constant: the shard form.  pp: see enqueue_prod_units
template <class Launch>
static int32_t enqueue_prod_launch(ctd_handle* h, const MfCall& c, const ProdParams& pp, const double* x_dev, Launch&& launch) {
    hipError_t e = hipErrorInvalidValue;
    if (h->rt) {
        void* args[] = {(void*)&pp, &x_dev};
        e = jit_launch(h->jit[c.op.fam][c.shard()].f[c.op.f0], (int)((pp.unit_end - pp.unit_begin + 255) / 256), 256, 0, h->stream, args);
    }
    for_problem(h->model.problem, [&](auto tag) { e = c.shard() ? launch(tag, std::true_type{}) : launch(tag, std::false_type{}); });
    return c.launched(h, e);
}

// The unit pass and the finish of a transposed product (jtprod, hprod, kktprod, hdiag, jsq_cols): `dirs` directions per node in
// chunks of jc (prod_chunk) give the geometry and the size of the caller's partial buffer, written into a's ProdParams; then the two
// kernels: f[f0], f[f0 + 1] of the run-time OCP's module, or launch_prod_units.  a: the kernels' argument struct, its unit range
// set by the caller (prod_params): the grid and the partial sums cover those nodes -- all N + 1 of a whole-grid call
template <class K>
static int32_t enqueue_prod_units(ctd_handle* h, const MfCall& c, typename K::Params& a, int dirs, int jc, DevBuf<>& partial,
                                  const double* x_dev) {
    ProdParams& pp = K::prod(a);
    pp.nch = (int32_t)((dirs + jc - 1) / jc);
    const int64_t blocks = ((pp.unit_end - pp.unit_begin) * (int64_t)pp.nch + 255) / 256;
    if (blocks > 0x7fffffff) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": grid too large");
    pp.nblocks = (int32_t)blocks;
    const int32_t st = partial.grow(h, blocks * kMaxNV, c.fn());
    if (st) return st;
    pp.partial = partial.p;
    hipError_t e = hipErrorInvalidValue;
    if (h->rt) {
        const JitModule& jm = h->jit[c.op.fam][c.shard()];
        void* args[] = {&a, &x_dev};
        e = jit_launch(jm.f[c.op.f0], (int)blocks, 256, 0, h->stream, args);
        if (e == hipSuccess) e = jit_launch(jm.f[c.op.f0 + 1], 1, 64, 0, h->stream, args);
    }
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        e = c.shard() ? launch_prod_units<P, K, true>(a, x_dev, h->stream) : launch_prod_units<P, K, false>(a, x_dev, h->stream);
    });
    return c.launched(h, e);
}

extern "C" {

const char* ctd_strerror(int32_t st) {
    switch (st) {
        case CTD_OK: return "ok";
        case CTD_EINVAL: return "invalid argument";
        case CTD_EGRID: return "given time grid is not strictly increasing";
        case CTD_ESCHEME: return "unknown discretization method";
        case CTD_EPATTERN: return "sparsity pattern not available";
        case CTD_EPROBLEM: return "problem not in the compiled registry";
        case CTD_ENODEVICE: return "no HIP device bound to this handle (there is no CPU fallback)";
        case CTD_EHIP: return "HIP runtime error";
        case CTD_ENOMEM: return "out of memory";
        default: return "unknown status";
    }
}

const char* ctd_last_error(const ctd_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int32_t ctd_create(const ctd_desc* desc, ctd_handle** out) {
    if (!desc || !out) return fail(nullptr, CTD_EINVAL, "ctd_create: null argument");
    *out = nullptr;
    struct Del { void operator()(ctd_handle* p) const { if (p) destroy_handle(p); } };
    std::unique_ptr<ctd_handle, Del> h(new (std::nothrow) ctd_handle());
    if (!h) return fail(nullptr, CTD_ENOMEM, "ctd_create: out of memory");
    HostDesc hd{desc->problem, desc->scheme, desc->pattern_mode, desc->grid_size, desc->time_grid, desc->time_grid_len,
                desc->control_steps > 1 ? desc->control_steps : 1, desc->value_order};
    if (desc->reserved0 != 0) return fail(nullptr, CTD_EINVAL, "ctd_create: ctd_desc.reserved0 must be 0 (zero-initialise the descriptor: memset / ctd_desc d = {0})");
    std::string err;
    int st;
    try {
        st = build_model(hd, h->model, err);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, CTD_ENOMEM, "ctd_create: out of memory while building the model");
    }
    if (st) return fail(nullptr, st, err);
    const Model& mo = h->model;
    // The lean variant of the constraint / Jacobian kernel reads its block sizes, counts and Butcher tables from the static layout
    // of its instantiation (StaticLayout, ctd_kernel_body.hpp), not from the kernel arguments: a handle whose built layout differs
    // from it is refused here -- every handle, host-only ones included -- so a wrong constant never becomes a wrong Jacobian.
    // (Run-time OCPs have no registry instantiation; midpoint with more than 3 controls per step has no kernel at all.)
    if (!runtime_ocp(mo.problem)) {
        const char* bad = nullptr;
        for_problem(mo.problem, [&](auto tag) {
            using P = typename decltype(tag)::type;
            for_scheme<true>(mo.L, [&](auto t) { bad = static_layout_mismatch<P, t.sc, t.s>(mo.L); });
        });
        if (bad) return fail(nullptr, CTD_EINVAL, std::string("ctd_create: the static layout of the kernel instantiation differs from the model's layout in field '") + bad + "'");
        // The static-emit form of the lean kernel also takes the periods of the output streams (manual pattern, CSC order) from its
        // instantiation (StaticEmit, ctd_emit_static.hpp): the same check, the same refusal.
        if (mo.pattern_mode == 0 && mo.order == 0) {
            for_problem(mo.problem, [&](auto tag) {
                using P = typename decltype(tag)::type;
                for_scheme<true>(mo.L, [&](auto t) { bad = static_emit_mismatch<P, t.sc, t.s>(mo.L, mo.Lseg, mo.vr); });
            });
            if (bad) return fail(nullptr, CTD_EINVAL, std::string("ctd_create: the static emit geometry of the kernel instantiation differs from the model's in '") + bad + "'");
        }
    }
    if (mo.L.cs > 3 && desc->device >= 0 && !runtime_ocp(mo.problem))      // (host-only handles -- sizes, bounds, patterns -- take any)
        return fail(nullptr, CTD_EINVAL, "ctd_create: control_steps > 3 needs an OCP registered at run time (ctd_register_ocp); the compiled registry holds the midpoint kernels for 1, 2 and 3 controls per step");
    h->step_begin = desc->step_begin;
    h->step_end = desc->step_end;
    if (h->step_begin == 0 && h->step_end == 0) h->step_end = mo.L.N;
    if (h->step_begin < 0 || h->step_end > mo.L.N || h->step_begin >= h->step_end)
        return fail(nullptr, CTD_EINVAL, "ctd_create: shard [step_begin, step_end) is not inside [0, N)");
    h->rt = runtime_ocp(mo.problem);
    h->device = desc->device;
    Resident resident;
    int cus = 256;
    if (h->device >= 0) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || h->device >= ndev)
            return fail(nullptr, CTD_ENODEVICE, "ctd_create: HIP device not available");
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 256;
        resident = [hp = h.get()](const KParams& kp, int block, size_t lds_bytes) { return resident_cons_jac(hp, kp, block, lds_bytes); };
    }
    if (const int pst = plan_cons_jac(mo, h->step_begin, h->step_end, plan_knobs_from_env(), resident, cus, kMultiTileLoop, h->plan, err))
        return fail(nullptr, pst, err);
    if (h->device >= 0) {
        ctd_handle* hp = h.get();
        KParams& kp = hp->plan.kp;
        DeviceGuard dg_(hp->device); HIP_TRY(nullptr, dg_.err);
        if (desc->stream_mode == CTD_STREAM_GIVEN) { hp->stream = (hipStream_t)desc->stream; hp->own_stream = false; }
        else { HIP_TRY(nullptr, hipStreamCreateWithFlags(&hp->stream, hipStreamNonBlocking)); hp->own_stream = true; }
        // The normalized grid is always read from this table (N + 1 doubles, L2-resident): for a uniform grid the kernels
        // could compute tau_i = i / N themselves, but an FP64 division is ~35 dependent instructions on the evaluating lane's
        // critical path while the table load is issued together with the loads of x (the values are identical: the host
        // fills the table with the same division).
        HIP_TRY(nullptr, upload(hp->d_tau, mo.tau));
        HIP_TRY(nullptr, upload(hp->d_tmpl, mo.tmpl));
        HIP_TRY(nullptr, upload(hp->d_vtmpl, mo.vtmpl));
        HIP_TRY(nullptr, upload(hp->d_edge_idx, mo.edge_idx));
        HIP_TRY(nullptr, upload(hp->d_edge_code, mo.edge_code));
        kp.tau = hp->d_tau.p;
        kp.tmpl = hp->d_tmpl.p;
        kp.vtmpl = hp->d_vtmpl.p;
        if (hp->plan.early) {
            HIP_TRY(nullptr, upload(hp->d_pos, mo.pos_order));
            kp.pos = hp->d_pos.p;
        }
        kp.edge_idx = hp->d_edge_idx.p;
        kp.edge_code = hp->d_edge_code.p;
        hp->obj_blocks = 256;
        HIP_TRY(nullptr, hp->d_partial.ensure(hp->obj_blocks));
        HIP_TRY(nullptr, hp->d_obj.ensure(1));
        HIP_TRY(nullptr, hipEventCreate(&hp->ev0));
        HIP_TRY(nullptr, hipEventCreate(&hp->ev1));
        if (hp->rt) {
            const int32_t jst = jit_load(hp, JIT_FIRST);
            if (jst) return jst;
        }
    }
    *out = h.release();
    return CTD_OK;
}

int32_t ctd_register_ocp(const ctd_ocp_def* def, int32_t* problem_id) {
    if (!def || !problem_id) return fail(nullptr, CTD_EINVAL, "ctd_register_ocp: null argument");
    std::string err;
    int id = -1;
    const int st = register_runtime_ocp(def, &id, err);
    if (st) return fail(nullptr, st, "ctd_register_ocp: " + err);
    *problem_id = id;
    return CTD_OK;
}

int32_t ctd_ocp_source(int32_t problem_id, char* buf, int64_t cap) {
    const RtOcp* ro = runtime_ocp(problem_id);
    if (!ro) return fail(nullptr, CTD_EINVAL, "ctd_ocp_source: not a run-time problem id");
    const int64_t need = (int64_t)ro->functor_src.size() + 1;
    if (!buf || cap < need)        // never a silently truncated text: the message names the capacity to come back with
        return fail(nullptr, CTD_EINVAL, "ctd_ocp_source: buffer too small, needs " + std::to_string(need) + " bytes");
    std::memcpy(buf, ro->functor_src.c_str(), (size_t)need);
    return CTD_OK;
}

// compile-only check (no device needed): the kernels of `scheme` for a registered OCP build for gfx950
int32_t ctd_jit_check(int32_t problem_id, int32_t scheme) {
    const RtOcp* ro = runtime_ocp(problem_id);
    if (!ro) return fail(nullptr, CTD_EPROBLEM, "ctd_jit_check: not a run-time problem id");
    if (scheme < 0 || scheme > 8) return fail(nullptr, CTD_ESCHEME, "Unknown discretization method");
    const int sc = scheme == 0 ? SC_TRAPEZE : ((scheme == 1 || scheme >= 7) ? SC_MIDPOINT : SC_IRK);
    int s = (scheme < 2 || scheme >= 7) ? 0 : (scheme <= 4 ? scheme - 1 : scheme - 3);
    if (scheme == 1) s = env_int("CTD_JIT_CHECK_CS", 0);       // midpoint: controls per step of the kernels to build (default 1)
    std::string code, err;
    std::vector<std::string> names;
    int32_t st = jit_compile(*ro, "ctd_kernels.hpp", jit_first_exprs(sc, s, ""), "off", code, names, err);
    if (st == CTD_OK) st = jit_compile(*ro, "ctd_hess_kernels.hpp", jit_hess_exprs(sc, s, ""), "fast", code, names, err);
    if (st) return fail(nullptr, st, err);
    return CTD_OK;
}

int32_t ctd_destroy(ctd_handle* h) {
    if (!h) return CTD_EINVAL;
    destroy_handle(h);
    return CTD_OK;
}

int32_t ctd_sizes(const ctd_handle* h, int64_t* nvar, int64_t* ncon, int64_t* nnzj, int64_t* nnzh) {
    if (!h) return CTD_EINVAL;
    if (nvar) *nvar = h->model.L.nvar;
    if (ncon) *ncon = h->model.L.ncon;
    if (nnzj) *nnzj = h->model.nnzj;
    if (nnzh) *nnzh = h->model.H.nnzh;
    return CTD_OK;
}

int32_t ctd_dims(const ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    const Layout& L = h->model.L;
    const ProblemInfo& pi = h->model.info;
    o[0] = L.n; o[1] = L.m; o[2] = L.nv; o[3] = L.p; o[4] = L.bc; o[5] = L.N;
    o[6] = L.blk; o[7] = L.eqs; o[8] = L.p; o[9] = L.s; o[10] = L.final_control;
    o[11] = pi.it0 >= 0; o[12] = pi.itf >= 0; o[13] = pi.lagrange; o[14] = pi.mayer; o[15] = pi.maximize;
    return CTD_OK;
}

int32_t ctd_time_grid(const ctd_handle* h, double* normalized, double* fixed) {
    if (!h) return CTD_EINVAL;
    const Model& mo = h->model;
    if (normalized) std::memcpy(normalized, mo.tau.data(), sizeof(double) * (mo.L.N + 1));
    if (fixed) for (int64_t i = 0; i <= mo.L.N; ++i) fixed[i] = mo.fixed_time(i);
    return CTD_OK;
}

// get_time_grid(xu, docp), src/DOCP_data.jl:437-458 (host arithmetic on the tail of x: post-processing, not the hot path)
int32_t ctd_time_grid_at(const ctd_handle* h, const double* x, double* grid) {
    if (!h || !x || !grid) return CTD_EINVAL;
    const Model& mo = h->model;
    const Layout& L = mo.L;
    const double t0 = L.it0 >= 0 ? x[L.v_off + L.it0] : L.t0;
    const double tf = L.itf >= 0 ? x[L.v_off + L.itf] : L.tf;
    for (int64_t i = 0; i <= L.N; ++i) grid[i] = L.free_time ? t0 + mo.tau[i] * (tf - t0) : mo.fixed_time(i);
    return CTD_OK;
}

int32_t ctd_butcher(const ctd_handle* h, double* a, double* b, double* c) {
    if (!h) return CTD_EINVAL;
    const Layout& L = h->model.L;
    for (int i = 0; i < L.s; ++i) {
        if (b) b[i] = L.b[i];
        if (c) c[i] = L.c[i];
        if (a) for (int j = 0; j < L.s; ++j) a[i * L.s + j] = L.a[3 * i + j];
    }
    return CTD_OK;
}

int32_t ctd_bounds(const ctd_handle* h, double* lvar, double* uvar, double* lcon, double* ucon) {
    if (!h) return CTD_EINVAL;
    const Model& mo = h->model;
    mo.fill_bounds(lvar, uvar, lcon, ucon);
    return CTD_OK;
}

int32_t ctd_initial_guess(const ctd_handle* h, double* x0, const ctd_init* init) {
    if (!h || !x0) return CTD_EINVAL;
    if (init) {
        InitSamples sm;
        if (init->n_samples > 0) {
            if (!init->t_samples) return fail(const_cast<ctd_handle*>(h), CTD_EINVAL, "ctd_initial_guess: t_samples is NULL");
            for (int64_t k = 1; k < init->n_samples; ++k)
                if (!(init->t_samples[k] > init->t_samples[k - 1]))
                    return fail(const_cast<ctd_handle*>(h), CTD_EGRID, "ctd_initial_guess: t_samples must be strictly increasing");
            sm.n = init->n_samples; sm.t = init->t_samples; sm.state = init->state_samples; sm.control = init->control_samples;
        }
        model_initial_guess(h->model, x0, init->use_problem_default != 0, init->state, init->control, init->variable, sm);
    }
    else model_initial_guess(h->model, x0, false, nullptr, nullptr, nullptr);
    return CTD_OK;
}

int32_t ctd_jac_structure(const ctd_handle* h, int64_t* rows, int64_t* cols) {
    if (!h || !rows || !cols) return CTD_EINVAL;
    const Model& mo = h->model;
    std::vector<int64_t> r;
    int64_t nz = 0;
    if (mo.order == 1) {                 // CTD_ORDER_CSR: the k-th value belongs to the k-th entry read by rows
        for (int64_t i = 0; i < mo.L.ncon; ++i) {
            mo.gen_row(i, r);
            for (int64_t col : r) { rows[nz] = i + 1; cols[nz] = col + 1; ++nz; }
        }
        return nz == mo.nnzj ? CTD_OK : CTD_EPATTERN;
    }
    for (int64_t j = 0; j < mo.L.nvar; ++j) {
        mo.gen_column(j, r);
        for (int64_t row : r) { rows[nz] = row + 1; cols[nz] = j + 1; ++nz; }
    }
    return nz == mo.nnzj ? CTD_OK : CTD_EPATTERN;
}

int32_t ctd_jac_csc(const ctd_handle* h, int64_t* colptr, int64_t* rowval) {
    if (!h || !colptr || !rowval) return CTD_EINVAL;
    const Model& mo = h->model;
    std::vector<int64_t> r;
    int64_t nz = 0;
    for (int64_t j = 0; j < mo.L.nvar; ++j) {
        colptr[j] = nz;
        mo.gen_column(j, r);
        for (int64_t row : r) rowval[nz++] = row;
    }
    colptr[mo.L.nvar] = nz;
    return nz == mo.nnzj ? CTD_OK : CTD_EPATTERN;
}

int32_t ctd_jac_csr(const ctd_handle* h, int64_t* rowptr, int64_t* colind) {
    if (!h || !rowptr || !colind) return CTD_EINVAL;
    const Model& mo = h->model;
    std::vector<int64_t> c;
    int64_t nz = 0;
    for (int64_t i = 0; i < mo.L.ncon; ++i) {
        rowptr[i] = nz;
        if (mo.order == 1 && mo.row_start(i) != nz) return fail(const_cast<ctd_handle*>(h), CTD_EPATTERN, "internal: row_start disagrees with the generated rows");
        mo.gen_row(i, c);
        for (int64_t col : c) colind[nz++] = col;
    }
    rowptr[mo.L.ncon] = nz;
    return nz == mo.nnzj ? CTD_OK : CTD_EPATTERN;
}

int32_t ctd_value_order(const ctd_handle* h, int32_t* order) {
    if (!h || !order) return CTD_EINVAL;
    *order = h->model.order;
    return CTD_OK;
}

int32_t ctd_dropped_nonzeros(const ctd_handle* h, int64_t* count) {
    if (!h || !count) return CTD_EINVAL;
    *count = h->model.dropped;
    return CTD_OK;
}

int32_t ctd_shard_info(const ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    const Model& mo = h->model;
    const Layout& L = mo.L;
    const bool first = h->step_begin == 0, last = h->step_end == L.N;
    o[0] = h->step_begin; o[1] = h->step_end;
    o[2] = h->step_begin * L.cb;
    o[3] = h->step_end * L.cb;      // (+ the p + bc tail rows [N*cb, ncon), which every shard writes)
    o[4] = mo.shard_vals_begin(h->step_begin);
    o[5] = mo.shard_vals_end(h->step_end);
    o[6] = first; o[7] = last;
    return CTD_OK;
}

// Sharded iterate read in place: from now on the constraint / Jacobian kernels of this handle load the variables of OTHER
// shards -- the next shard's first node, the previous shard's last step block, X_1, X_{N+1} -- from x_bufs[k] (peer-mapped or
// IPC-mapped full-length buffers) instead of the x passed to the call.  The table is a few hundred bytes of device memory,
// rewritten only when the arguments change.
int32_t ctd_set_x_shards(ctd_handle* h, int32_t n_shards, const int64_t* step_begin, const double* const* x_bufs, int32_t self) {
    if (!h) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    if (n_shards <= 0 || !step_begin || !x_bufs) {         // back to "x holds everything this handle reads"
        h->plan.kp.halo = nullptr;
        h->halo_host.G = 0;
        return CTD_OK;
    }
    const Layout& L = h->model.L;
    if (n_shards > kMaxShards) return fail(h, CTD_EINVAL, "ctd_set_x_shards: more than 16 shards");
    if (self < 0 || self >= n_shards || step_begin[self] != h->step_begin || step_begin[self + 1] != h->step_end)
        return fail(h, CTD_EINVAL, "ctd_set_x_shards: step_begin[self], step_begin[self + 1] do not name this handle's shard");
    if (step_begin[0] != 0 || step_begin[n_shards] != L.N) return fail(h, CTD_EINVAL, "ctd_set_x_shards: the shards must cover [0, N)");
    XHalo t{};
    t.G = n_shards; t.self = self;
    for (int k = 0; k < n_shards; ++k) {
        if (step_begin[k + 1] <= step_begin[k]) return fail(h, CTD_EINVAL, "ctd_set_x_shards: empty shard");
        if (k != self && !x_bufs[k]) return fail(h, CTD_EINVAL, "ctd_set_x_shards: null buffer");
        t.vbegin[k] = step_begin[k] * (int64_t)L.blk;
        t.x[k] = k == self ? nullptr : x_bufs[k];
    }
    t.vbegin[n_shards] = L.v_off;       // the last shard also owns the final node; v is replicated
    if (h->plan.kp.halo && std::memcmp(&t, &h->halo_host, sizeof(XHalo)) == 0) return CTD_OK;
    DeviceGuard dg_(h->device); HIP_TRY(h, dg_.err);
    HIP_TRY(h, h->d_halo.ensure(1));
    HIP_TRY(h, hipStreamSynchronize(h->stream));           // launches in flight still read the old table
    HIP_TRY(h, hipMemcpy(h->d_halo.p, &t, sizeof(XHalo), hipMemcpyHostToDevice));
    h->halo_host = t;
    h->plan.kp.halo = h->d_halo.p;
    h->plan.kp.near = make_xnear(t, L.blk, L.N, L.v_off);
    return CTD_OK;
}

// ---- the stitched constraint vector for one-process-per-GPU hosts: RCCL all-gather inside the library --------------------
// RCCL is reached through the copy of librccl the host process already has (a Julia / Python host created the communicator
// with it): resolved with dlopen at first use, no link-time dependency.  CTD_RCCL_LIB names the library explicitly.
namespace {
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
typedef const char* (*nccl_errstr_fn)(int);
nccl_allgather_fn g_nccl_allgather = nullptr;
nccl_errstr_fn g_nccl_errstr = nullptr;
std::once_flag g_nccl_once;
void nccl_resolve() {
    std::call_once(g_nccl_once, [] {
        void* lib = nullptr;
        if (const char* p = std::getenv("CTD_RCCL_LIB")) lib = dlopen(p, RTLD_NOW);
        for (const char* nm : {"librccl.so.1", "librccl.so"})            // the copy already in the process, whoever loaded it
            if (!lib) lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
        for (const char* nm : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if (!lib) lib = dlopen(nm, RTLD_NOW);
        if (!lib) return;
        g_nccl_allgather = (nccl_allgather_fn)dlsym(lib, "ncclAllGather");
        g_nccl_errstr = (nccl_errstr_fn)dlsym(lib, "ncclGetErrorString");
    });
}
__global__ void stitch_pack_kernel(const double* __restrict__ c, double* __restrict__ send, int64_t row0, int64_t own, int64_t tail0, int64_t tail) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < own) send[e] = c[row0 + e];
    else if (e < own + tail) send[e] = c[tail0 + (e - own)];
}
__global__ void stitch_unpack_kernel(const double* __restrict__ recv, double* __restrict__ c, int64_t ncon, int64_t N, int cb, int G, int64_t smax) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < ncon) c[r] = recv[stitch_src(r, N, cb, G, smax)];
}
}  // namespace

int32_t ctd_shard_steps(int64_t N, int32_t n_shards, int32_t k, int64_t* begin, int64_t* end) {
    if (N < 1 || n_shards < 1 || n_shards > N || k < 0 || k >= n_shards || !begin || !end) return CTD_EINVAL;
    *begin = shard_begin(N, n_shards, k);
    *end = k + 1 == n_shards ? N : shard_begin(N, n_shards, k + 1);
    return CTD_OK;
}

int32_t ctd_stitch_c(ctd_handle* h, void* nccl_comm, int32_t n_ranks, int32_t rank, double* c_dev) {
    if (!h) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    if (!nccl_comm || !c_dev || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(h, CTD_EINVAL, "ctd_stitch_c: bad argument");
    const Layout& L = h->model.L;
    const int64_t N = L.N;
    const int G = n_ranks;
    if (G > N || h->step_begin != shard_begin(N, G, rank) || h->step_end != (rank + 1 == G ? N : shard_begin(N, G, rank + 1)))
        return fail(h, CTD_EINVAL, "ctd_stitch_c: the handle's shard is not block `rank` of the balanced split of the grid over n_ranks (ctd_shard_steps)");
    nccl_resolve();
    if (!g_nccl_allgather) return fail(h, CTD_ERCCL, "ctd_stitch_c: librccl (ncclAllGather) not found in this process; set CTD_RCCL_LIB");
    DeviceGuard dg_(h->device); HIP_TRY(h, dg_.err);
    const int64_t tail = L.ncon - N * L.cb;
    auto check = [&](int rc, const char* what) -> int32_t {
        if (rc == 0) return CTD_OK;
        return fail(h, CTD_ERCCL, std::string(what) + ": " + (g_nccl_errstr ? g_nccl_errstr(rc) : "RCCL error ") + " (" + std::to_string(rc) + ")");
    };
    constexpr int kNcclDouble = 8;       // ncclFloat64
    if (N % G == 0 && tail == 0) {       // equal blocks, nothing after them: gathered in place
        const int64_t S = (N / G) * L.cb;
        return check(g_nccl_allgather(c_dev + rank * S, c_dev, (size_t)S, kNcclDouble, nccl_comm, h->stream), "ncclAllGather");
    }
    const int64_t smax = ((N + G - 1) / G) * L.cb + tail;
    if (h->d_stitch_recv.cap < (int64_t)G * smax) {
        h->d_stitch_send.release();
        h->d_stitch_recv.release();
        HIP_TRY(h, h->d_stitch_send.ensure(smax));
        HIP_TRY(h, h->d_stitch_recv.ensure((int64_t)G * smax));
        HIP_TRY(h, hipMemsetAsync(h->d_stitch_send.p, 0, sizeof(double) * smax, h->stream));
    }
    const int64_t own = (h->step_end - h->step_begin) * L.cb, mytail = rank + 1 == G ? tail : 0;
    const int64_t np = own + mytail;
    stitch_pack_kernel<<<(unsigned)((np + 255) / 256), 256, 0, h->stream>>>(c_dev, h->d_stitch_send.p, h->step_begin * L.cb, own, N * L.cb, mytail);
    HIP_TRY(h, hipGetLastError());
    const int32_t st = check(g_nccl_allgather(h->d_stitch_send.p, h->d_stitch_recv.p, (size_t)smax, kNcclDouble, nccl_comm, h->stream), "ncclAllGather");
    if (st) return st;
    stitch_unpack_kernel<<<(unsigned)((L.ncon + 255) / 256), 256, 0, h->stream>>>(h->d_stitch_recv.p, c_dev, L.ncon, N, L.cb, G, smax);
    HIP_TRY(h, hipGetLastError());
    return CTD_OK;
}

// ---- device buffers shared between the processes of one node (one process per GPU) ------------------------------------
// hipIpcGetMemHandle names a whole allocation: the handle of the allocation that holds dev_ptr plus dev_ptr's offset in it
// (a torch tensor is a slice of the caching allocator's block).
int32_t ctd_ipc_export(int32_t device, const void* dev_ptr, void* handle64, int64_t* offset) {
    if (!dev_ptr || !handle64 || !offset) return CTD_EINVAL;
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "CTD_IPC_HANDLE_BYTES");
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (e == hipSuccess) e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dev_ptr);
    hipIpcMemHandle_t hd;
    if (e == hipSuccess) e = hipIpcGetMemHandle(&hd, (void*)base);
    if (e != hipSuccess) { g_create_err = std::string("ctd_ipc_export: ") + hipGetErrorString(e); (void)hipGetLastError(); return CTD_EHIP; }
    std::memcpy(handle64, &hd, sizeof(hd));
    *offset = (int64_t)((const char*)dev_ptr - (const char*)base);
    return CTD_OK;
}
int32_t ctd_ipc_open(int32_t device, const void* handle64, void** base) {
    if (!handle64 || !base) return CTD_EINVAL;
    *base = nullptr;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    hipIpcMemHandle_t hd;
    std::memcpy(&hd, handle64, sizeof(hd));
    if (e == hipSuccess) e = hipIpcOpenMemHandle(base, hd, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { g_create_err = std::string("ctd_ipc_open: ") + hipGetErrorString(e); (void)hipGetLastError(); return CTD_ERCCL; }
    return CTD_OK;
}
// reads `bytes` (<= 64) at a mapped pointer with a device-to-device copy on `device`: a mapping the device cannot reach comes back
// as an error code here instead of as a fault inside a kernel
int32_t ctd_ipc_probe(int32_t device, const void* ptr, size_t bytes) {
    if (!ptr || bytes == 0 || bytes > 64) return CTD_EINVAL;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    void* tmp = nullptr;
    if (e == hipSuccess) e = hipMalloc(&tmp, 64);
    if (e == hipSuccess) e = hipMemcpy(tmp, ptr, bytes, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess) { g_create_err = std::string("ctd_ipc_probe: ") + hipGetErrorString(e); (void)hipGetLastError(); return CTD_ERCCL; }
    return CTD_OK;
}
int32_t ctd_ipc_close(int32_t device, void* base) {
    if (!base) return CTD_OK;
    DeviceGuard dg(device);
    return (dg.err == hipSuccess && hipIpcCloseMemHandle(base) == hipSuccess) ? CTD_OK : CTD_EHIP;
}

int32_t ctd_launch_info(const ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    o[0] = h->plan.grid; o[1] = h->plan.block; o[2] = (int64_t)h->plan.lds_bytes; o[3] = h->plan.tile; o[4] = h->model.Lseg;
    o[5] = (int64_t)h->model.edge_idx.size();
    o[6] = (h->model.fused && h->model.L.sc != SC_TRAPEZE) ? 1 : 0;      // DirectTile<P, SC>
    // resident workgroups per CU of the kernel this handle launches, as the runtime computes it from the kernel's registers and
    // LDS (0: host-only handle / query failed): the tiles' rounds = grid / (o[7] * CUs)
    o[7] = h->device >= 0 ? resident_cons_jac(h, h->plan.kp, h->plan.block, h->plan.lds_bytes) : 0;
    return CTD_OK;
}

// ---- hot path ------------------------------------------------------------------------------------------------

// A batched call (ctd_*_batch_dev_async): n members, member b at x + b ldx, ... (leading dimensions in doubles, already checked)
struct Batch {
    int32_t n;
    int64_t ldx, ldy, ldc, ldv, ldg, ldh;
};

static int32_t enqueue_cons_jac(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev, hipEvent_t te0 = nullptr,
                                hipEvent_t te1 = nullptr, const Batch* bt = nullptr) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x_dev) return fail(h, CTD_EINVAL, "x is null");
    KParams kp = h->plan.kp;
    kp.c = c_dev;
    kp.vals = vals_dev;
    hipError_t e = hipErrorInvalidValue;
    if (bt) {      // the batched instantiation of the kernel: grid (tiles, members)
        BatchLd bl{bt->ldx, bt->ldc, bt->ldv};
        // write-through stores by the rule of the plan (plan_cons_jac), applied to what the whole LAUNCH writes (all members)
        kp.wt_store = write_through(h->plan.out_mb * bt->n);
        if (h->rt) {
            if (const int32_t jst = jit_load(h, JIT_BATCH)) return jst;
            void* args[] = {&kp, &x_dev, &bl};
            e = jit_launch(h->jit[JIT_BATCH][0].f[0], h->plan.grid, h->plan.block, h->plan.lds_bytes, h->stream, args, nullptr, nullptr, bt->n);
        }
        for_problem(h->model.problem, [&](auto tag) {
            using P = typename decltype(tag)::type;
            e = launch_cons_jac_batch<P>(kp, x_dev, bl, h->plan.grid, h->plan.block, h->plan.lds_bytes, h->stream, bt->n);
        });
        return launched(h, nullptr, e);
    }
    if (h->rt) {
        void* args[] = {&kp, &x_dev};
        e = jit_launch(h->jit[JIT_FIRST][0].f[0], h->plan.grid, h->plan.block, h->plan.lds_bytes, h->stream, args, te0, te1);
    }
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        e = launch_cons_jac<P>(kp, x_dev, h->plan.grid, h->plan.block, h->plan.lds_bytes, h->stream, te0, te1, h->plan.lean_ok);
    });
    return launched(h, nullptr, e);
}

int32_t ctd_cons_jac_dev_async(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev) {
    return enqueue_cons_jac(h, x_dev, c_dev, vals_dev);
}

// Launch on another stream from now on (e.g. the capturing stream while the caller records a HIP graph of a whole solver
// iteration).  The handle never owns a stream passed this way.
int32_t ctd_set_stream(ctd_handle* h, void* stream) {
    if (!h) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    if (h->own_stream && h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    return CTD_OK;
}

int32_t ctd_sync(ctd_handle* h) {
    if (!h) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CTD_OK;
}

int32_t ctd_cons_jac_dev(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev) {
    int32_t st = enqueue_cons_jac(h, x_dev, c_dev, vals_dev);
    if (st) return st;
    return ctd_sync(h);
}

static int32_t host_cons_jac(ctd_handle* h, const double* x, double* c, double* vals) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x) return fail(h, CTD_EINVAL, "x is null");
    const Model& mo = h->model;
    return host_call(h, {{x, h->d_x, mo.L.nvar}},
                     [&] { return enqueue_cons_jac(h, h->d_x.p, c ? h->d_c.p : nullptr, vals ? h->d_vals.p : nullptr); },
                     {{c, h->d_c, mo.L.ncon}, {vals, h->d_vals, mo.nnzj}});
}

int32_t ctd_host_alloc(void** ptr, size_t bytes) {
    if (!ptr) return CTD_EINVAL;
    *ptr = nullptr;
    const hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 8, hipHostMallocDefault);
    if (e != hipSuccess) { g_create_err = std::string("ctd_host_alloc: ") + hipGetErrorString(e); return CTD_EHIP; }
    return CTD_OK;
}
int32_t ctd_host_free(void* ptr) {
    if (!ptr) return CTD_OK;
    return hipHostFree(ptr) == hipSuccess ? CTD_OK : CTD_EHIP;
}

int32_t ctd_cons(ctd_handle* h, const double* x, double* c) {
    if (h && !c) return fail(h, CTD_EINVAL, "c is null");
    return host_cons_jac(h, x, c, nullptr);
}
int32_t ctd_jac_coord(ctd_handle* h, const double* x, double* vals) {
    if (h && !vals) return fail(h, CTD_EINVAL, "vals is null");
    return host_cons_jac(h, x, nullptr, vals);
}
int32_t ctd_cons_jac(ctd_handle* h, const double* x, double* c, double* vals) {
    if (h && (!c || !vals)) return fail(h, CTD_EINVAL, "c or vals is null");
    return host_cons_jac(h, x, c, vals);
}

// kernel parameters of the objective pass; returns the quadrature workgroups (0 for a Mayer-only cost)
static int fill_obj_params(ctd_handle* h, double* f_dev, ObjParams& op);

static int32_t enqueue_obj(ctd_handle* h, const double* x_dev, double* f_dev, const Batch* bt = nullptr) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x_dev || !f_dev) return fail(h, CTD_EINVAL, "null argument");
    const Layout& L = h->model.L;
    ObjParams op;
    const int blocks = fill_obj_params(h, f_dev, op);
    const bool lagrange = h->model.info.lagrange;
    const int nb = bt ? bt->n : 1;
    if (bt) {
        const int32_t st = h->d_partial.grow(h, (int64_t)nb * (blocks > 0 ? blocks : 1), "ctd_obj_batch_dev_async");
        if (st) return st;
        op.partial = h->d_partial.p;
        op.ldx = bt->ldx;
    }
    hipError_t e = hipErrorInvalidValue;
    if (h->rt) {
        void* args[] = {&op, &x_dev};
        e = lagrange ? jit_launch(h->jit[JIT_FIRST][0].f[1], blocks, 256, 0, h->stream, args, nullptr, nullptr, nb) : hipSuccess;
        if (e == hipSuccess) e = jit_launch(h->jit[JIT_FIRST][0].f[2], 1, 64, 0, h->stream, args, nullptr, nullptr, nb);
    }
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        e = launch_obj<P>(op, x_dev, lagrange ? blocks : 0, 256, h->stream, nb);
    });
    return launched(h, nullptr, e);
}

static int fill_obj_params(ctd_handle* h, double* f_dev, ObjParams& op) {
    const Layout& L = h->model.L;
    std::memset(&op, 0, sizeof(op));
    op.L = L;
    op.tau = h->d_tau.p;
    const bool last = h->step_end == L.N;
    // quadrature units: trapeze sums over nodes (node N belongs to the last shard), the others over steps
    op.unit_begin = h->step_begin;
    op.unit_end = (L.sc == SC_TRAPEZE && last) ? L.N + 1 : h->step_end;
    op.add_mayer = last ? 1 : 0;
    op.partial = h->d_partial.p;
    op.out = f_dev;
    op.halo = h->plan.kp.halo;
    op.near = h->plan.kp.near;
    const int64_t units = op.unit_end - op.unit_begin;
    int blocks = (int)((units + 255) / 256);
    if (blocks > h->obj_blocks) blocks = h->obj_blocks;
    if (blocks < 1) blocks = 1;
    const bool lagrange = h->model.info.lagrange;      // Mayer-only cost: no quadrature pass, the finish kernel alone
    op.nblocks = lagrange ? blocks : 0;
    return lagrange ? blocks : 0;
}

int32_t ctd_obj_dev_async(ctd_handle* h, const double* x_dev, double* f_dev) { return enqueue_obj(h, x_dev, f_dev); }

int32_t ctd_obj_dev(ctd_handle* h, const double* x_dev, double* f_host) {
    if (h && !f_host) return fail(h, CTD_EINVAL, "null argument");
    const OnDevice on(h);
    if (on.st) return on.st;
    return host_call(h, {}, [&] { return enqueue_obj(h, x_dev, h->d_obj.p); }, {{f_host, h->d_obj, 1}});
}

static int32_t enqueue_grad(ctd_handle* h, const double* x_dev, double* g_dev, GradParams* only_params = nullptr, bool shard = false,
                            const Batch* bt = nullptr);
int32_t ctd_grad_dev_async(ctd_handle* h, const double* x_dev, double* g_dev) { return enqueue_grad(h, x_dev, g_dev); }
// the shard's own entries of the gradient from a sharded iterate read in place (see include/ctdirect_hip.h)
int32_t ctd_grad_shard_dev_async(ctd_handle* h, const double* x_dev, double* g_dev) { return enqueue_grad(h, x_dev, g_dev, nullptr, true); }
int32_t ctd_grad_dev(ctd_handle* h, const double* x_dev, double* g_dev) {
    int32_t st = enqueue_grad(h, x_dev, g_dev);
    if (st) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CTD_OK;
}

// zeroes entries [0, len) of `rows` rows with leading dimension ld (the batched gradient's tails: one launch for all members)
__global__ void zero_rows_kernel(double* __restrict__ p, int64_t ld, int64_t len) {
    double* row = p + (int64_t)blockIdx.y * ld;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (int64_t)gridDim.x * blockDim.x) row[e] = 0.0;
}

static int32_t enqueue_grad(ctd_handle* h, const double* x_dev, double* g_dev, GradParams* only_params, bool shard, const Batch* bt) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x_dev || !g_dev) return fail(h, CTD_EINVAL, "null argument");
    // ctd_grad*: the gradient of the WHOLE objective (O(nvar) work on every rank), from the x it is given -- a whole iterate.
    // ctd_grad_shard_dev_async (shard = true): the quadrature units of this handle's steps only (the last shard also the final node),
    // neighbours' blocks through the shard table like the other callbacks: the shard's own entries of g + its partial d/dv
    const Layout& L = h->model.L;
    const bool last = h->step_end == L.N, first = h->step_begin == 0;
    const int64_t all_units = (L.sc == SC_IRK) ? L.N : L.N + 1;
    const int64_t ub = shard ? h->step_begin : 0, ue = shard ? ((L.sc != SC_IRK && last) ? L.N + 1 : h->step_end) : all_units;
    const int64_t units = ue - ub;
    const int blocks = (int)((units + 255) / 256);
    const int nb = bt ? bt->n : 1;
    if (bt) {
        const int32_t st = h->d_gpartial.grow(h, (int64_t)nb * blocks * kMaxNV, "ctd_grad_batch_dev_async");
        if (st) return st;
    } else HIP_TRY(h, h->d_gpartial.ensure((int64_t)blocks * kMaxNV));      // (neither drained nor refused inside a capture)
    GradParams gp;
    std::memset(&gp, 0, sizeof(gp));
    gp.L = L;
    gp.tau = h->d_tau.p;
    gp.g = g_dev;
    gp.partial = h->d_gpartial.p;
    gp.nblocks = blocks;
    gp.unit_begin = ub; gp.unit_end = ue;
    gp.owns_first = (!shard || first) ? 1 : 0;
    gp.owns_last = (!shard || last) ? 1 : 0;
    if (shard) { gp.halo = h->plan.kp.halo; gp.near = h->plan.kp.near; }
    if (only_params) { gp.nblocks = h->model.info.lagrange ? blocks : 0; *only_params = gp; return CTD_OK; }
    // With a Lagrange cost the per-step kernel writes every entry of the step blocks (owner computes), only the tail
    // (final state, variables) needs zeroing before the finish kernel adds the Mayer part; a Mayer-only gradient is zero
    // except at x_0, x_f, v: one memset and the finish kernel
    const bool lagrange = h->model.info.lagrange;
    if (bt) {
        // every member's g: the same entries as below (the tail, or all of g for a Mayer-only cost), zeroed by one launch
        gp.ldx = bt->ldx;
        gp.ldg = bt->ldg;
        const int64_t z0 = lagrange ? L.N * (int64_t)L.blk : 0, len = L.nvar - z0;
        if (len > 0) {
            zero_rows_kernel<<<dim3((unsigned)std::min<int64_t>(64, (len + 255) / 256), (unsigned)nb), 256, 0, h->stream>>>(g_dev + z0, bt->ldg, len);
            HIP_TRY(h, hipGetLastError());
        }
    } else if (shard) {
        // a shard touches its own entries only: zero what the unit kernel does not write (everything, for a Mayer-only cost), the
        // final-state entries on the last shard, and the nv variable entries (the finish kernel assigns them)
        const int64_t lo = h->step_begin * (int64_t)L.blk, hi = h->step_end * (int64_t)L.blk;
        if (!lagrange) HIP_TRY(h, hipMemsetAsync(g_dev + lo, 0, sizeof(double) * (hi - lo), h->stream));
        if (last && (!lagrange || L.sc == SC_IRK))
            HIP_TRY(h, hipMemsetAsync(g_dev + L.N * (int64_t)L.blk, 0, sizeof(double) * (L.v_off - L.N * (int64_t)L.blk), h->stream));
    } else if (lagrange) HIP_TRY(h, hipMemsetAsync(g_dev + L.N * (int64_t)L.blk, 0, sizeof(double) * (L.nvar - L.N * (int64_t)L.blk), h->stream));
    else HIP_TRY(h, hipMemsetAsync(g_dev, 0, sizeof(double) * L.nvar, h->stream));
    gp.nblocks = lagrange ? blocks : 0;
    hipError_t e = hipErrorInvalidValue;
    if (h->rt) {
        void* args[] = {&gp, &x_dev};
        e = lagrange ? jit_launch(h->jit[JIT_FIRST][0].f[3], blocks, 256, 0, h->stream, args, nullptr, nullptr, nb) : hipSuccess;
        if (e == hipSuccess) e = jit_launch(h->jit[JIT_FIRST][0].f[4], 1, 64, 0, h->stream, args, nullptr, nullptr, nb);
    }
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        e = launch_grad<P>(gp, x_dev, lagrange ? blocks : 0, h->stream, nb);
    });
    return launched(h, nullptr, e);
}

int32_t ctd_grad(ctd_handle* h, const double* x, double* g) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x || !g) return fail(h, CTD_EINVAL, "null argument");
    const int64_t nvar = h->model.L.nvar;
    return host_call(h, {{x, h->d_x, nvar}}, [&] { return enqueue_grad(h, h->d_x.p, h->d_g.p); }, {{g, h->d_g, nvar}});
}

// ---- the matrix-free operators (rows: kJprod ... kJsqRows above) ---------------------------------------------------------
// jprod!(nlp, x, v, Jv), jtprod!(nlp, x, w, Jtw): ctd_prod_kernels.hpp; hprod!(nlp, x, y, v, Hv; obj_weight): ctd_hprod_kernels.hpp;
// the KKT product rx = (sigma H_f + sum y_r H_{c_r}) dx + J' dy + sx o dx, rc = J dx - sc o dy: ctd_kkt_kernels.hpp; the KKT
// diagonals diag(H), diag(J W J') (row sums) and diag(J' W J) (column sums): ctd_diag_kernels.hpp.
//
// The checks of every entry point, in this order: handle (CTD_EINVAL), device (CTD_ENODEVICE) -- the prologue, OnDevice(h, fn) --,
// whole-grid handle (not for the shard calls, which take every handle), the required pointers -- `req` and `out`; `opt` may be
// null --, then every output against every input and against the other outputs (CTD_EINVAL).  The enqueue runs under the caller's
// prologue.
static int32_t mf_check(const OnDevice& on, ctd_handle* h, const MfCall& c, std::initializer_list<const double*> req,
                        std::initializer_list<const double*> opt, std::initializer_list<const double*> out) {
    if (on.st) return on.st;
    if (!c.shard() && (h->step_begin != 0 || h->step_end != h->model.L.N || h->plan.kp.halo))
        return fail(h, CTD_EINVAL, std::string(c.fn()) + ": this call needs a handle of the whole grid; a shard of the grid (step_begin / "
                                   "step_end, ctd_set_x_shards) is out of scope for this call: a shard handle calls " + c.op.name[MF_SHARD]);
    for (const auto& ptrs : {req, out})
        for (const double* p : ptrs)
            if (!p) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": null argument (" + c.op.required + " are required)");
    for (const double* const* o = out.begin(); o != out.end(); ++o) {
        for (const auto& ptrs : {req, opt})
            for (const double* p : ptrs)
                if (p == *o) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": the output (" + c.op.outs + ") must not be an input buffer");
        for (const double* const* o2 = out.begin(); o2 != o; ++o2)
            if (*o2 == *o) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": " + c.op.outs + " must be different buffers");
    }
    return CTD_OK;
}

// The kernels' common arguments: the inputs, and the nodes the launch evaluates.  Whole grid: all N + 1.  Shard call: the nodes of
// the handle's steps [step_begin, step_end), node N too on the last shard; the iterate's entries of other shards through the
// handle's table when one is set
static ProdParams prod_params(const ctd_handle* h, const MfCall& c, const double* dir_dev, double* out_dev) {
    ProdParams pp;
    std::memset(&pp, 0, sizeof(pp));
    const int64_t N = h->model.L.N;
    const bool shard = c.shard(), first = !shard || h->step_begin == 0, last = !shard || h->step_end == N;
    pp.L = h->model.L;
    pp.tau = h->d_tau.p;
    pp.dir = dir_dev;
    pp.out = out_dev;
    pp.unit_begin = shard ? h->step_begin : 0;
    pp.unit_end = last ? N + 1 : h->step_end;
    pp.owns_first = first ? 1 : 0;
    pp.owns_last = last ? 1 : 0;
    if (shard) { pp.halo = h->plan.kp.halo; pp.near = h->plan.kp.near; }
    return pp;
}

static int32_t enqueue_prod(ctd_handle* h, const MfCall& c, const double* x_dev, const double* d_dev, double* out_dev) {
    if (const int32_t st = jit_load(h, c.op.fam, c.shard())) return st;
    ProdParams pp = prod_params(h, c, d_dev, out_dev);
    if (c.op.one_launch)
        return enqueue_prod_launch(h, c, pp, x_dev, [&](auto tag, auto sh) {
            return launch_jprod<typename decltype(tag)::type, decltype(sh)::value>(pp, x_dev, h->stream);
        });
    return enqueue_prod_units<JtprodKernels>(h, c, pp, prod_dirs_per_node(pp.L), prod_chunk<ProdDirs>(h, jtprod_chunk), h->d_ppartial, x_dev);
}

static int32_t enqueue_hprod(ctd_handle* h, const MfCall& c, const double* x_dev, const double* y_dev, double obj_weight,
                             const double* v_dev, double* out_dev) {
    if (const int32_t st = jit_load(h, c.op.fam, c.shard())) return st;
    HProdParams hp;
    std::memset(&hp, 0, sizeof(hp));
    hp.p = prod_params(h, c, y_dev, out_dev);
    hp.vt = v_dev;
    hp.sigma = obj_weight;
    return enqueue_prod_units<HprodKernels>(h, c, hp, hprod_dirs_per_node(hp.p.L), prod_chunk<HProdDirs>(h, hprod_chunk), h->d_hppartial, x_dev);
}

static int32_t enqueue_kktprod(ctd_handle* h, const MfCall& c, const double* x_dev, const double* y_dev, double obj_weight,
                               const double* dx_dev, const double* dy_dev, const double* sx_dev, const double* sc_dev, double* rx_dev,
                               double* rc_dev, DevBuf<>& partial) {
    if (const int32_t st = jit_load(h, c.op.fam, c.shard())) return st;
    KktParams kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.h.p = prod_params(h, c, y_dev, rx_dev);
    kp.h.vt = dx_dev;
    kp.h.sigma = obj_weight;
    kp.dy = dy_dev;
    kp.sx = sx_dev;
    kp.sc = sc_dev;
    kp.rc = rc_dev;
    // the fused lanes keep the hprod chunk rule (profiles/kktprod_resources.md)
    return enqueue_prod_units<KktKernels>(h, c, kp, hprod_dirs_per_node(kp.h.p.L), prod_chunk<HProdDirs>(h, hprod_chunk), partial, x_dev);
}

static int32_t enqueue_hdiag(ctd_handle* h, const MfCall& c, const double* x_dev, const double* y_dev, double obj_weight, double* out_dev) {
    if (const int32_t st = jit_load(h, c.op.fam, c.shard())) return st;
    HProdParams hp;
    std::memset(&hp, 0, sizeof(hp));
    hp.p = prod_params(h, c, y_dev, out_dev);
    hp.sigma = obj_weight;
    // one direction per lane: tangent and seed are the same unit vector
    return enqueue_prod_units<HdiagKernels>(h, c, hp, hprod_dirs_per_node(hp.p.L), 1, h->d_hdpartial, x_dev);
}

// jsq_rows: out = diag(J diag(w) J') (ncon), one launch; jsq_cols: out = diag(J' diag(w) J) (nvar), units + finish
static int32_t enqueue_jsq(ctd_handle* h, const MfCall& c, const double* x_dev, const double* w_dev, double* out_dev) {
    if (const int32_t st = jit_load(h, c.op.fam, c.shard())) return st;
    ProdParams pp = prod_params(h, c, w_dev, out_dev);
    if (c.op.one_launch)
        return enqueue_prod_launch(h, c, pp, x_dev, [&](auto tag, auto sh) {
            return launch_jsq_rows<typename decltype(tag)::type, decltype(sh)::value>(pp, x_dev, h->stream);
        });
    // the general lane for every scheme: the node's block and v (hprod's directions, not the Gauss-Legendre shortcut's)
    return enqueue_prod_units<JsqColsKernels>(h, c, pp, hprod_dirs_per_node(pp.L), prod_chunk<JsqDirs>(h, jsq_chunk), h->d_jcpartial, x_dev);
}

// The entry points of each operator: prologue, checks, then the enqueue on the caller's device pointers -- or, for the host form, on
// the handle's staging buffers: x in d_x, y in d_y, the direction (v, w, dx, the weights) in d_pdir, the result in d_pout; dy, sx,
// sc and rc of ctd_kktprod in buffers of their own.  Vectors of nvar / ncon entries: nothing proportional to nnzj
static int32_t mf_prod(ctd_handle* h, const MfCall& c, const double* x, const double* d, double* out) {
    const OnDevice on(h, c.fn());
    if (const int32_t st = mf_check(on, h, c, {x, d}, {}, {out})) return st;
    if (c.form != MF_HOST) return enqueue_prod(h, c, x, d, out);
    const Layout& L = h->model.L;
    return host_call(h, {{x, h->d_x, L.nvar}, {d, h->d_pdir, c.op.dir_ncon ? L.ncon : L.nvar}},
                     [&] { return enqueue_prod(h, c, h->d_x.p, h->d_pdir.p, h->d_pout.p); },
                     {{out, h->d_pout, c.op.out_ncon ? L.ncon : L.nvar}});
}

// y may be null: the objective only
static int32_t mf_hprod(ctd_handle* h, const MfCall& c, const double* x, const double* y, double obj_weight, const double* v, double* Hv) {
    const OnDevice on(h, c.fn());
    if (const int32_t st = mf_check(on, h, c, {x, v}, {y}, {Hv})) return st;
    if (c.form != MF_HOST) return enqueue_hprod(h, c, x, y, obj_weight, v, Hv);
    const Layout& L = h->model.L;
    return host_call(h, {{x, h->d_x, L.nvar}, {v, h->d_pdir, L.nvar}, {y, h->d_y, L.ncon}},
                     [&] { return enqueue_hprod(h, c, h->d_x.p, y ? h->d_y.p : nullptr, obj_weight, h->d_pdir.p, h->d_pout.p); },
                     {{Hv, h->d_pout, L.nvar}});
}

// y, sx and sc may be null: no multipliers, no diagonal term
static int32_t mf_kktprod(ctd_handle* h, const MfCall& c, const double* x, const double* y, double obj_weight, const double* dx,
                          const double* dy, const double* sx, const double* sc, double* rx, double* rc) {
    const OnDevice on(h, c.fn());
    if (const int32_t st = mf_check(on, h, c, {x, dx, dy}, {y, sx, sc}, {rx, rc})) return st;
    if (c.form != MF_HOST) return enqueue_kktprod(h, c, x, y, obj_weight, dx, dy, sx, sc, rx, rc, h->d_kktpartial);
    const Layout& L = h->model.L;
    return host_call(h, {{x, h->d_x, L.nvar}, {dx, h->d_pdir, L.nvar}, {y, h->d_y, L.ncon}, {dy, h->d_kdy, L.ncon},
                         {sx, h->d_ksx, L.nvar}, {sc, h->d_ksc, L.ncon}},
                     [&] {
                         return enqueue_kktprod(h, c, h->d_x.p, y ? h->d_y.p : nullptr, obj_weight, h->d_pdir.p, h->d_kdy.p,
                                                sx ? h->d_ksx.p : nullptr, sc ? h->d_ksc.p : nullptr, h->d_pout.p, h->d_krc.p, h->d_kktpartial);
                     },
                     {{rx, h->d_pout, L.nvar}, {rc, h->d_krc, L.ncon}});
}

// y may be null: the objective only
static int32_t mf_hdiag(ctd_handle* h, const MfCall& c, const double* x, const double* y, double obj_weight, double* Hd) {
    const OnDevice on(h, c.fn());
    if (const int32_t st = mf_check(on, h, c, {x}, {y}, {Hd})) return st;
    if (c.form != MF_HOST) return enqueue_hdiag(h, c, x, y, obj_weight, Hd);
    const Layout& L = h->model.L;
    return host_call(h, {{x, h->d_x, L.nvar}, {y, h->d_y, L.ncon}},
                     [&] { return enqueue_hdiag(h, c, h->d_x.p, y ? h->d_y.p : nullptr, obj_weight, h->d_pout.p); }, {{Hd, h->d_pout, L.nvar}});
}

// w may be null: ones
static int32_t mf_jsq(ctd_handle* h, const MfCall& c, const double* x, const double* w, double* out) {
    const OnDevice on(h, c.fn());
    if (const int32_t st = mf_check(on, h, c, {x}, {w}, {out})) return st;
    if (c.form != MF_HOST) return enqueue_jsq(h, c, x, w, out);
    const Layout& L = h->model.L;
    return host_call(h, {{x, h->d_x, L.nvar}, {w, h->d_pdir, c.op.dir_ncon ? L.ncon : L.nvar}},
                     [&] { return enqueue_jsq(h, c, h->d_x.p, w ? h->d_pdir.p : nullptr, h->d_pout.p); },
                     {{out, h->d_pout, c.op.out_ncon ? L.ncon : L.nvar}});
}

// The shard calls write the shard's own rows (jprod, jsq_rows, rc) or the entries of its own variables + its partial sums of the nv
// tail entries, from full-length buffers (see include/ctdirect_hip.h)
int32_t ctd_jprod(ctd_handle* h, const double* x, const double* v, double* Jv) { return mf_prod(h, {kJprod, MF_HOST}, x, v, Jv); }
int32_t ctd_jprod_dev_async(ctd_handle* h, const double* x_dev, const double* v_dev, double* Jv_dev) {
    return mf_prod(h, {kJprod, MF_DEV}, x_dev, v_dev, Jv_dev);
}
int32_t ctd_jprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* v_dev, double* Jv_dev) {
    return mf_prod(h, {kJprod, MF_SHARD}, x_dev, v_dev, Jv_dev);
}
int32_t ctd_jtprod(ctd_handle* h, const double* x, const double* w, double* Jtw) { return mf_prod(h, {kJtprod, MF_HOST}, x, w, Jtw); }
int32_t ctd_jtprod_dev_async(ctd_handle* h, const double* x_dev, const double* w_dev, double* Jtw_dev) {
    return mf_prod(h, {kJtprod, MF_DEV}, x_dev, w_dev, Jtw_dev);
}
int32_t ctd_jtprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* w_dev, double* Jtw_dev) {
    return mf_prod(h, {kJtprod, MF_SHARD}, x_dev, w_dev, Jtw_dev);
}

int32_t ctd_hprod(ctd_handle* h, const double* x, const double* y, double obj_weight, const double* v, double* Hv) {
    return mf_hprod(h, {kHprod, MF_HOST}, x, y, obj_weight, v, Hv);
}
int32_t ctd_hprod_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* v_dev,
                            double* Hv_dev) {
    return mf_hprod(h, {kHprod, MF_DEV}, x_dev, y_dev, obj_weight, v_dev, Hv_dev);
}
int32_t ctd_hprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* v_dev,
                                  double* Hv_dev) {
    return mf_hprod(h, {kHprod, MF_SHARD}, x_dev, y_dev, obj_weight, v_dev, Hv_dev);
}

int32_t ctd_kktprod(ctd_handle* h, const double* x, const double* y, double obj_weight, const double* dx, const double* dy,
                    const double* sx, const double* sc, double* rx, double* rc) {
    return mf_kktprod(h, {kKktprod, MF_HOST}, x, y, obj_weight, dx, dy, sx, sc, rx, rc);
}
int32_t ctd_kktprod_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* dx_dev,
                              const double* dy_dev, const double* sx_dev, const double* sc_dev, double* rx_dev, double* rc_dev) {
    return mf_kktprod(h, {kKktprod, MF_DEV}, x_dev, y_dev, obj_weight, dx_dev, dy_dev, sx_dev, sc_dev, rx_dev, rc_dev);
}
int32_t ctd_kktprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* dx_dev,
                                    const double* dy_dev, const double* sx_dev, const double* sc_dev, double* rx_dev, double* rc_dev) {
    return mf_kktprod(h, {kKktprod, MF_SHARD}, x_dev, y_dev, obj_weight, dx_dev, dy_dev, sx_dev, sc_dev, rx_dev, rc_dev);
}

int32_t ctd_hdiag(ctd_handle* h, const double* x, const double* y, double obj_weight, double* Hd) {
    return mf_hdiag(h, {kHdiag, MF_HOST}, x, y, obj_weight, Hd);
}
int32_t ctd_hdiag_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* Hd_dev) {
    return mf_hdiag(h, {kHdiag, MF_DEV}, x_dev, y_dev, obj_weight, Hd_dev);
}
int32_t ctd_hdiag_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* Hd_dev) {
    return mf_hdiag(h, {kHdiag, MF_SHARD}, x_dev, y_dev, obj_weight, Hd_dev);
}
int32_t ctd_jsq_rows(ctd_handle* h, const double* x, const double* wx, double* out) { return mf_jsq(h, {kJsqRows, MF_HOST}, x, wx, out); }
int32_t ctd_jsq_rows_dev_async(ctd_handle* h, const double* x_dev, const double* wx_dev, double* out_dev) {
    return mf_jsq(h, {kJsqRows, MF_DEV}, x_dev, wx_dev, out_dev);
}
int32_t ctd_jsq_rows_shard_dev_async(ctd_handle* h, const double* x_dev, const double* wx_dev, double* out_dev) {
    return mf_jsq(h, {kJsqRows, MF_SHARD}, x_dev, wx_dev, out_dev);
}
int32_t ctd_jsq_cols(ctd_handle* h, const double* x, const double* wc, double* out) { return mf_jsq(h, {kJsqCols, MF_HOST}, x, wc, out); }
int32_t ctd_jsq_cols_dev_async(ctd_handle* h, const double* x_dev, const double* wc_dev, double* out_dev) {
    return mf_jsq(h, {kJsqCols, MF_DEV}, x_dev, wc_dev, out_dev);
}
int32_t ctd_jsq_cols_shard_dev_async(ctd_handle* h, const double* x_dev, const double* wc_dev, double* out_dev) {
    return mf_jsq(h, {kJsqCols, MF_SHARD}, x_dev, wc_dev, out_dev);
}

// ---- device-resident preconditioned MINRES solve of K z = rhs (kernels, state and freeze: ctd_krylov_kernels.hpp) -----------------
// One row per entry point (none has a shard form; the KKT family: what enqueue_kktprod launches for a run-time OCP)
#define CTD_MR_OP(X, REQ) {{X, X, X}, JIT_KKT, 0, false, false, false, REQ, "z"}
static constexpr MfOp kMrStart = CTD_MR_OP("ctd_kkt_minres_start_dev_async", "sys->x, rhs and z"),
                      kMrIters = CTD_MR_OP("ctd_kkt_minres_iters_dev_async", "sys->x and z"),
                      kMrDev = CTD_MR_OP("ctd_kkt_minres_dev", "sys->x, rhs and z"),
                      kMrHost = CTD_MR_OP("ctd_kkt_minres", "sys->x, rhs and z");
#undef CTD_MR_OP

// The checks of the solve's entry points, in the header's order.  Before the device: the handle and the layout of the caller's structs
// (*st = the status to return when the result is false)
static bool mr_structs_ok(ctd_handle* h, const char* fn, const ctd_kkt_system* sys, bool with_info, const ctd_minres_info* info, int32_t* st) {
    *st = CTD_EINVAL;
    return h && STRUCT_OK(h, fn, "sys", ctd_kkt_system, sys) && (!with_info || STRUCT_OK(h, fn, "info", ctd_minres_info, info));
}
// ... after it (OnDevice): whole-grid handle, the pointers (mf_check), the preconditioner pair
static int32_t mr_check(const OnDevice& on, ctd_handle* h, const MfCall& c, const ctd_kkt_system* sys, const double* rhs, const double* z,
                        bool with_rhs) {
    if (on.st) return on.st;
    if (h->step_begin != 0 || h->step_end != h->model.L.N || h->plan.kp.halo)
        return fail(h, CTD_EINVAL, std::string(c.fn()) + ": this call needs a handle of the whole grid; a shard of the grid (step_begin / "
                                   "step_end, ctd_set_x_shards) is out of scope: the solve has no shard form yet (it needs the "
                                   "all-reduce of ctd_kktprod_shard_dev_async's partial sums and of the inner products)");
    const int32_t st = with_rhs ? mf_check(on, h, c, {sys->x, rhs}, {sys->y, sys->sx, sys->sc, sys->px, sys->pc}, {z})
                                : mf_check(on, h, c, {sys->x}, {sys->y, sys->sx, sys->sc, sys->px, sys->pc}, {z});
    if (st) return st;
    if (!sys->px != !sys->pc)
        return fail(h, CTD_EINVAL, std::string(c.fn()) + ": px and pc are given both (M = diag(1 / px, 1 / pc)) or neither (no preconditioner)");
    return CTD_OK;
}
// (these two: the whole-grid solves and the start of every phase family on a shard)
static int32_t mr_check_count(ctd_handle* h, const char* fn, const char* name, int64_t v) {
    return v >= 1 ? CTD_OK : fail(h, CTD_EINVAL, std::string(fn) + ": " + name + " = " + std::to_string(v) + ", must be at least 1");
}
static int32_t mr_check_rtol(ctd_handle* h, const char* fn, double rtol) {
    return rtol >= 0.0 ? CTD_OK : fail(h, CTD_EINVAL, std::string(fn) + ": rtol must not be negative (or NaN)");
}

static KrylovParams mr_params(const ctd_handle* h) {
    KrylovParams kp = krylov_params(h->d_mrws.p, h->model.L.nvar + h->model.L.ncon, h->mr_z, h->mr_precond);
    if (h->mr_schur) {
        const Layout& L = h->model.L;
        kp.s_lo = L.nvar;
        kp.s_hi = L.nvar + L.N * (int64_t)L.cb;
        kp.s_part = h->mr_schur + kSchurPart;
        kp.s_nwg = schur_solve_grid(L.N);
    }
    return kp;
}
// the solve launch of the Schur preconditioner inside the solve: y = T^-1 r2 on the block rows, the partial sums of r2 . y
static SchurSolveParams mr_schur_params(const ctd_handle* h, const KrylovParams& kp, int32_t mode) {
    const Layout& L = h->model.L;
    return SchurSolveParams{L.N, L.cb, mode, h->mr_schur, kp.r2 + L.nvar, kp.y + L.nvar, h->mr_schur + kSchurPart, kp.cur};
}
// ... of either kind: the chunked form's one launch, or the launches of the log-depth form (the last one: its partial sums, which
// lie where the chunked solve leaves its own)
static hipError_t mr_schur_solve(const ctd_handle* h, const KrylovParams& kp, int32_t mode) {
    if (!h->mr_schur_cr) return schur_solve(mr_schur_params(h, kp, mode), h->stream);
    const Layout& L = h->model.L;
    return schur_cr_solve(SchurCrSolveParams{L.N, L.cb, mode, schur_cr_levels(L.N), 0, h->mr_schur, kp.r2 + L.nvar, kp.y + L.nvar, kp.cur},
                          h->stream);
}

// max_iter: the cap the device state carries
static int32_t mr_enqueue_start(ctd_handle* h, const MfCall& c, const ctd_kkt_system& sys, const double* rhs_dev, double* z_dev, double rtol,
                                int64_t max_iter, double* schur_ws = nullptr, bool schur_cr = false) {
    const Layout& L = h->model.L;
    const int64_t n = L.nvar + L.ncon;
    if (const int32_t st = h->d_mrws.grow(h, krylov_workspace(n), c.fn())) return st;
    h->mr_z = z_dev;
    h->mr_precond = sys.px != nullptr;
    h->mr_schur = schur_ws;
    h->mr_schur_cr = schur_ws && schur_cr;
    const KrylovParams kp = mr_params(h);
    if (!schur_ws) return c.launched(h, krylov_start(kp, rhs_dev, sys.px, sys.pc, L.nvar, rtol, max_iter, h->stream));
    hipError_t e = krylov_schur_init(kp, rhs_dev, sys.px, sys.pc, L.nvar, h->stream);
    if (e == hipSuccess) e = mr_schur_solve(h, kp, SCHUR_START);
    if (e == hipSuccess) e = krylov_schur_first(kp, rtol, max_iter, h->stream);
    return c.launched(h, e);
}

// k iterations: K v (v and kv are Krylov vectors: dx / dy and rx / rc are their halves), then (A), (B), (C)
static int32_t mr_enqueue_iters(ctd_handle* h, const MfCall& c, const ctd_kkt_system& sys, int64_t k) {
    const KrylovParams kp = mr_params(h);
    const int64_t nvar = h->model.L.nvar;
    for (int64_t it = 0; it < k; ++it) {
        if (const int32_t st = enqueue_kktprod(h, c, sys.x, sys.y, sys.obj_weight, kp.v, kp.v + nvar, sys.sx, sys.sc, kp.kv, kp.kv + nvar,
                                               h->d_mrkpartial))
            return st;
        hipError_t e = krylov_alfa(kp, h->stream);
        if (e == hipSuccess && !h->mr_schur) e = krylov_step(kp, h->stream);
        if (e == hipSuccess && h->mr_schur) {
            e = krylov_schur_lanczos(kp, h->stream);
            if (e == hipSuccess) e = mr_schur_solve(h, kp, SCHUR_ITER);
            if (e == hipSuccess) e = krylov_schur_update(kp, h->stream);
        }
        if (e != hipSuccess) return c.launched(h, e);
    }
    return CTD_OK;
}

// the state of a solve (state_dev: a KrylovState on the device) as the caller's info; waits for the handle's stream
static int32_t mr_read_info(ctd_handle* h, const void* state_dev, ctd_minres_info* info) {
    KrylovState s;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(&s, state_dev, sizeof(s), hipMemcpyDeviceToHost));
    info->status = s.status;
    info->iterations = s.itn;
    info->phibar = s.phibar;
    info->Anorm = s.Anorm;
    info->ynorm = s.ynorm;
    info->beta1 = s.beta1;
    return CTD_OK;
}

// start, then at most ceil(max_iter / check_every) chunks: the device freezes the solve at max_iter iterations
static int32_t mr_drive(ctd_handle* h, const MfCall& c, const ctd_kkt_system& sys, const double* rhs_dev, double* z_dev, double rtol,
                        int64_t max_iter, int64_t check_every, ctd_minres_info* info, double* schur_ws = nullptr, bool schur_cr = false) {
    if (const int32_t st = mr_enqueue_start(h, c, sys, rhs_dev, z_dev, rtol, max_iter, schur_ws, schur_cr)) return st;
    for (int64_t done = 0; done < max_iter; done += check_every) {
        if (const int32_t st = mr_enqueue_iters(h, c, sys, check_every)) return st;
        if (const int32_t st = mr_read_info(h, mr_params(h).pend, info)) return st;
        if (info->status != CTD_MINRES_RUNNING) return CTD_OK;
    }
    return mr_read_info(h, mr_params(h).pend, info);
}

int32_t ctd_kkt_minres_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev, double rtol) {
    const MfCall c{kMrStart, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, false, nullptr, &st)) return st;
    const OnDevice on(h, c.fn());
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol))) return st;
    return mr_enqueue_start(h, c, *sys, rhs_dev, z_dev, rtol, INT64_MAX);
}

int32_t ctd_kkt_minres_iters_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* z_dev, int64_t k) {
    const MfCall c{kMrIters, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, false, nullptr, &st)) return st;
    const OnDevice on(h, c.fn());
    if ((st = mr_check(on, h, c, sys, nullptr, z_dev, false))) return st;
    if ((st = mr_check_count(h, c.fn(), "k", k))) return st;
    if (!h->mr_z) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": no solve has been started on this handle (ctd_kkt_minres_start_dev_async)");
    if (z_dev != h->mr_z) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": z is not the iterate of the solve started last");
    return mr_enqueue_iters(h, c, *sys, k);
}

int32_t ctd_kkt_minres_info(ctd_handle* h, ctd_minres_info* info) {
    const char* fn = "ctd_kkt_minres_info";
    if (!h || !STRUCT_OK(h, fn, "info", ctd_minres_info, info)) return CTD_EINVAL;
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    if (!h->mr_z) return fail(h, CTD_EINVAL, std::string(fn) + ": no solve has been started on this handle (ctd_kkt_minres_start_dev_async)");
    return mr_read_info(h, mr_params(h).pend, info);
}

int32_t ctd_kkt_minres_dev(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev, double rtol, int64_t max_iter,
                           int64_t check_every, ctd_minres_info* info) {
    const MfCall c{kMrDev, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, true, info, &st)) return st;
    const OnDevice on(h, c.fn());
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol)) || (st = mr_check_count(h, c.fn(), "max_iter", max_iter)) ||
        (st = mr_check_count(h, c.fn(), "check_every", check_every)))
        return st;
    return mr_drive(h, c, *sys, rhs_dev, z_dev, rtol, max_iter, check_every, info);
}

int32_t ctd_kkt_minres(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs, double* z, double rtol, int64_t max_iter,
                       int64_t check_every, ctd_minres_info* info) {
    const MfCall c{kMrHost, MF_HOST};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, true, info, &st)) return st;
    const OnDevice on(h, c.fn());
    if ((st = mr_check(on, h, c, sys, rhs, z, true))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol)) || (st = mr_check_count(h, c.fn(), "max_iter", max_iter)) ||
        (st = mr_check_count(h, c.fn(), "check_every", check_every)))
        return st;
    // x, y, sx, sc where ctd_kktprod stages them; (px, pc), rhs and z in buffers of the solve's own
    const Layout& L = h->model.L;
    const int64_t n = L.nvar + L.ncon;
    HIP_TRY(h, h->d_mrp.ensure(n));
    ctd_kkt_system dev = *sys;  // (the device pointers are set once host_call has allocated the staging buffers)
    return host_call(h, {{sys->x, h->d_x, L.nvar}, {sys->y, h->d_y, L.ncon}, {sys->sx, h->d_ksx, L.nvar}, {sys->sc, h->d_ksc, L.ncon},
                         {rhs, h->d_mrrhs, n}},
                     [&]() -> int32_t {
                         if (sys->px) {
                             HIP_TRY(h, hipMemcpyAsync(h->d_mrp.p, sys->px, sizeof(double) * L.nvar, hipMemcpyHostToDevice, h->stream));
                             HIP_TRY(h, hipMemcpyAsync(h->d_mrp.p + L.nvar, sys->pc, sizeof(double) * L.ncon, hipMemcpyHostToDevice, h->stream));
                         }
                         dev.x = h->d_x.p;
                         dev.y = sys->y ? h->d_y.p : nullptr;
                         dev.sx = sys->sx ? h->d_ksx.p : nullptr;
                         dev.sc = sys->sc ? h->d_ksc.p : nullptr;
                         dev.px = sys->px ? h->d_mrp.p : nullptr;
                         dev.pc = sys->pc ? h->d_mrp.p + L.nvar : nullptr;
                         return mr_drive(h, c, dev, h->d_mrrhs.p, h->d_mrz.p, rtol, max_iter, check_every, info);
                     },
                     {{z, h->d_mrz, n}});
}

// ---- chunked block-tridiagonal Schur preconditioner (plan: ctd_schur_plan.hpp; kernels, sums and workspace: ctd_schur_kernels.hpp) -----
static_assert(kSchurFixed == CTD_KKT_SCHUR_FIXED, "the fixed part of the workspace of the header");
static constexpr int32_t kPlanStatus[] = {CTD_OK, CTD_EINVAL, CTD_EGRID, CTD_ESCHEME, CTD_EPATTERN, CTD_EPROBLEM};

// What the four Schur families share around their own plans, kernels and workspaces.  The end of a family's plan: its status `st`
// (ctd_schur_plan.hpp) as the C status with its text behind the entry point's name; a plan that passed has walked the pattern
static int32_t schur_planned(ctd_handle* h, const char* fn, int st, const std::string& err) {
    if (st) return fail(h, kPlanStatus[st], std::string(fn) + ": " + err);
    h->schur_verified = true;
    return CTD_OK;
}
// the arguments of a factor (sc may be null: zero) ...
static int32_t schur_check_factor_args(ctd_handle* h, const char* fn, const double* jvals, const double* px, const double* sc, const double* ws) {
    if (!jvals || !px || !ws) return fail(h, CTD_EINVAL, std::string(fn) + ": null argument (jvals, px and ws are required)");
    if (ws == jvals || ws == px || ws == sc) return fail(h, CTD_EINVAL, std::string(fn) + ": the output (ws) must not be an input buffer");
    return CTD_OK;
}
// ... and of a solve; ws_written: the solve uses a scratch region of the workspace (the log-depth forms), so r must not be it either
static int32_t schur_check_solve_args(ctd_handle* h, const char* fn, const double* ws, const double* r, const double* out, bool ws_written) {
    if (!ws || !r || !out) return fail(h, CTD_EINVAL, std::string(fn) + ": null argument (ws, r and out are required)");
    if (out == r || out == ws || (ws_written && r == ws))
        return fail(h, CTD_EINVAL, std::string(fn) + ": the output (out) " + (ws_written ? "and the workspace " : "") + "must not be an input buffer");
    return CTD_OK;
}
// The status words of a factor, for the families' info calls (ws, first_bad_block: their arguments): waits for the handle's
// stream, reads the header of the workspace and compares its first words with `expect` (the tag and the fields the factor wrote
// for this handle); then `status` gets the n words behind the fixed part -- one per block, -1: every pivot was positive --, or as
// many as header word count_word says (>= 0: the chunked form's count of chunks, at most n).  It stays empty when the header is
// another's: the caller words the refusal.  schur_first_set: the first word that is set (-1: none)
static int32_t schur_read_status(ctd_handle* h, const char* fn, const double* ws_dev, const int64_t* first_bad_block,
                                 std::initializer_list<int64_t> expect, int count_word, int64_t n, std::vector<int64_t>& status) {
    if (!ws_dev || !first_bad_block) return fail(h, CTD_EINVAL, std::string(fn) + ": null argument (ws and first_bad_block are required)");
    int64_t head[9];
    static_assert(sizeof(head) <= sizeof(double) * kSchurFixed, "the header lies in the fixed part of every family's workspace");
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(head, ws_dev, sizeof(head), hipMemcpyDeviceToHost));
    status.clear();
    if (!std::equal(expect.begin(), expect.end(), head)) return CTD_OK;
    if (count_word >= 0) n = head[count_word] <= n ? head[count_word] : 0;
    if (n < 1) return CTD_OK;
    status.resize((size_t)n);
    HIP_TRY(h, hipMemcpy(status.data(), ws_dev + kSchurFixed, sizeof(int64_t) * status.size(), hipMemcpyDeviceToHost));
    return CTD_OK;
}
static int64_t schur_first_set(const std::vector<int64_t>& status) {
    for (size_t k = 0; k < status.size(); ++k)
        if (status[k] >= 0) return (int64_t)k;
    return -1;
}

// The checks every entry point of the family shares once the handle (and its device) are known: whole grid, then the plan's own
// (CSR order, block_rows, chunk_steps, the pattern -- walked once per handle)
static int32_t schur_plan(ctd_handle* h, const char* fn, int64_t chunk_steps, SchurPlan& pl) {
    if (h->step_begin != 0 || h->step_end != h->model.L.N || h->plan.kp.halo)
        return fail(h, CTD_EINVAL, std::string(fn) + ": this call needs a handle of the whole grid; a shard of the grid (step_begin / "
                                   "step_end, ctd_set_x_shards) is refused: the Schur preconditioner has no shard form yet");
    std::string err;
    return schur_planned(h, fn, plan_kkt_schur(h->model, chunk_steps, !h->schur_verified, pl, err), err);
}

int32_t ctd_kkt_schur_layout(ctd_handle* h, int64_t chunk_steps, ctd_schur_layout* out) {
    const char* fn = "ctd_kkt_schur_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_schur_layout, out)) return CTD_EINVAL;
    SchurPlan pl;
    if (const int32_t st = schur_plan(h, fn, chunk_steps, pl)) return st;
    out->reserved = 0;
    out->N = pl.N;
    out->block_rows = pl.block_rows;
    out->tail_rows = pl.tail_rows;
    out->first_tail_row = pl.first_tail_row;
    out->tail_cols = pl.tail_cols;
    out->n_chunks = pl.n_chunks;
    out->chunk_steps = pl.chunk_steps;
    out->workspace = pl.workspace;
    return CTD_OK;
}

// the pattern on the device, at the first factor: refused inside a capture like the other first-use allocations
static int32_t schur_upload_pattern(ctd_handle* h, const char* fn) {
    if (h->d_schur_rowptr.p && h->d_schur_colind.p) return CTD_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(h, CTD_EINVAL, std::string(fn) + ": the first factor on a handle uploads the Jacobian pattern, which cannot be done "
                                   "while the stream is capturing; make one call before the capture");
    (void)hipGetLastError();
    const Model& mo = h->model;
    std::vector<int64_t> rowptr(mo.L.ncon + 1), colind, c;
    colind.reserve(mo.nnzj);
    for (int64_t i = 0; i < mo.L.ncon; ++i) {
        rowptr[i] = (int64_t)colind.size();
        mo.gen_row(i, c);
        colind.insert(colind.end(), c.begin(), c.end());
    }
    rowptr[mo.L.ncon] = (int64_t)colind.size();
    if ((int64_t)colind.size() != mo.nnzj) return fail(h, CTD_EPATTERN, std::string(fn) + ": internal: the generated rows disagree with nnzj");
    HIP_TRY(h, upload(h->d_schur_colind, colind));
    HIP_TRY(h, upload(h->d_schur_rowptr, rowptr));
    return CTD_OK;
}

int32_t ctd_kkt_schur_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev, int64_t chunk_steps,
                                       double* ws_dev) {
    const char* fn = "ctd_kkt_schur_factor_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurPlan pl;
    if (const int32_t st = schur_plan(h, fn, chunk_steps, pl)) return st;
    if (const int32_t st = schur_check_factor_args(h, fn, jvals_dev, px_dev, sc_dev, ws_dev)) return st;
    if (const int32_t st = schur_upload_pattern(h, fn)) return st;
    const SchurFactorParams fp{pl.N, pl.first_tail_col, pl.chunk_steps, pl.n_chunks, (int32_t)pl.block_rows, 0,
                               h->d_schur_rowptr.p, h->d_schur_colind.p, jvals_dev, px_dev, sc_dev, ws_dev};
    return launched(h, fn, schur_factor(fp, h->stream));
}

int32_t ctd_kkt_schur_solve_dev_async(ctd_handle* h, const double* ws_dev, const double* r_dev, double* out_dev) {
    const char* fn = "ctd_kkt_schur_solve_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurPlan pl;
    if (const int32_t st = schur_plan(h, fn, 1, pl)) return st;
    if (const int32_t st = schur_check_solve_args(h, fn, ws_dev, r_dev, out_dev, false)) return st;
    const SchurSolveParams sp{pl.N, (int32_t)pl.block_rows, SCHUR_PLAIN, ws_dev, r_dev, out_dev, nullptr, nullptr};
    return launched(h, fn, schur_solve(sp, h->stream));
}

int32_t ctd_kkt_schur_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block) {
    const char* fn = "ctd_kkt_schur_info";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurPlan pl;
    if (const int32_t st = schur_plan(h, fn, 1, pl)) return st;
    std::vector<int64_t> status;       // one word per chunk (the factor's count: header word 4), each the chunk's first bad block
    if (const int32_t st = schur_read_status(h, fn, ws_dev, first_bad_block, {kSchurTag, pl.N, pl.block_rows}, 4, pl.N, status)) return st;
    if (status.empty())
        return fail(h, CTD_EINVAL, std::string(fn) + ": the workspace holds no factor of this handle (ctd_kkt_schur_factor_dev_async)");
    *first_bad_block = -1;
    for (int64_t b : status)
        if (b >= 0 && (*first_bad_block < 0 || b < *first_bad_block)) *first_bad_block = b;
    return CTD_OK;
}

// The solve with the factor as its preconditioner: the checks of ctd_kkt_minres_dev, then the family's own
static constexpr MfOp kMrSchurStart = {{"ctd_kkt_minres_schur_start_dev_async", "ctd_kkt_minres_schur_start_dev_async", "ctd_kkt_minres_schur_start_dev_async"},
                                       JIT_KKT, 0, false, false, false, "sys->x, rhs and z", "z"},
                      kMrSchurDev = {{"ctd_kkt_minres_schur_dev", "ctd_kkt_minres_schur_dev", "ctd_kkt_minres_schur_dev"},
                                     JIT_KKT, 0, false, false, false, "sys->x, rhs and z", "z"};
static int32_t mr_schur_check(ctd_handle* h, const MfCall& c, const ctd_kkt_system* sys, const double* ws, const double* rhs, const double* z) {
    if (!sys->px || !sys->pc || !ws)
        return fail(h, CTD_EINVAL, std::string(c.fn()) + ": null argument (sys->px, sys->pc and schur_ws are required)");
    for (const double* p : {sys->x, sys->y, sys->sx, sys->sc, sys->px, sys->pc, rhs, z})
        if (p == ws) return fail(h, CTD_EINVAL, std::string(c.fn()) + ": the workspace (schur_ws) must not be another argument's buffer");
    return CTD_OK;
}

int32_t ctd_kkt_minres_schur_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                             double* z_dev, double rtol) {
    const MfCall c{kMrSchurStart, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, false, nullptr, &st)) return st;
    const OnDevice on(h, c.fn());
    if (on.st) return on.st;
    SchurPlan pl;
    if ((st = schur_plan(h, c.fn(), 1, pl))) return st;             // (whole grid, CSR order, the block size)
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_schur_check(h, c, sys, schur_ws_dev, rhs_dev, z_dev))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol))) return st;
    return mr_enqueue_start(h, c, *sys, rhs_dev, z_dev, rtol, INT64_MAX, schur_ws_dev);
}

int32_t ctd_kkt_minres_schur_dev(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev, double* z_dev,
                                 double rtol, int64_t max_iter, int64_t check_every, ctd_minres_info* info) {
    const MfCall c{kMrSchurDev, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, true, info, &st)) return st;
    const OnDevice on(h, c.fn());
    if (on.st) return on.st;
    SchurPlan pl;
    if ((st = schur_plan(h, c.fn(), 1, pl))) return st;             // (whole grid, CSR order, the block size)
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_schur_check(h, c, sys, schur_ws_dev, rhs_dev, z_dev))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol)) || (st = mr_check_count(h, c.fn(), "max_iter", max_iter)) ||
        (st = mr_check_count(h, c.fn(), "check_every", check_every)))
        return st;
    return mr_drive(h, c, *sys, rhs_dev, z_dev, rtol, max_iter, check_every, info, schur_ws_dev);
}

// ---- log-depth exact block-tridiagonal Schur preconditioner (plan: ctd_schur_plan.hpp; kernels, sums and workspace:
// ctd_schur_cr_kernels.hpp): the entry points of the chunked one, with the same checks in the same order ----------------------------
static int32_t schur_cr_plan(ctd_handle* h, const char* fn, SchurCrPlan& pl) {
    if (h->step_begin != 0 || h->step_end != h->model.L.N || h->plan.kp.halo)
        return fail(h, CTD_EINVAL, std::string(fn) + ": this call needs a handle of the whole grid; a shard of the grid (step_begin / "
                                   "step_end, ctd_set_x_shards) is refused: this entry point has no shard form (the shard form of the "
                                   "log-depth preconditioner is ctd_kkt_schur_cr_shard_*)");
    std::string err;
    return schur_planned(h, fn, plan_kkt_schur_cr(h->model, !h->schur_verified, pl, err), err);
}

int32_t ctd_kkt_schur_cr_layout(ctd_handle* h, ctd_schur_cr_layout* out) {
    const char* fn = "ctd_kkt_schur_cr_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_schur_cr_layout, out)) return CTD_EINVAL;
    SchurCrPlan pl;
    if (const int32_t st = schur_cr_plan(h, fn, pl)) return st;
    static_assert(CTD_KKT_SCHUR_CR_WORKSPACE(7, 9) == kSchurFixed + 7 + 3 * 7 * 81 + 2 * 7 * 9, "the workspace of the header");
    out->reserved = 0;
    out->N = pl.N;
    out->block_rows = pl.block_rows;
    out->tail_rows = pl.tail_rows;
    out->first_tail_row = pl.first_tail_row;
    out->tail_cols = pl.tail_cols;
    out->n_levels = pl.n_levels;
    out->factor_launches = pl.factor_launches;
    out->solve_launches = pl.solve_launches;
    out->workspace = pl.workspace;
    return CTD_OK;
}

int32_t ctd_kkt_schur_cr_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev, double* ws_dev) {
    const char* fn = "ctd_kkt_schur_cr_factor_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrPlan pl;
    if (const int32_t st = schur_cr_plan(h, fn, pl)) return st;
    if (const int32_t st = schur_check_factor_args(h, fn, jvals_dev, px_dev, sc_dev, ws_dev)) return st;
    if (const int32_t st = schur_upload_pattern(h, fn)) return st;
    const SchurCrFactorParams fp{pl.N, pl.first_tail_col, (int32_t)pl.block_rows, (int32_t)pl.n_levels,
                                 h->d_schur_rowptr.p, h->d_schur_colind.p, jvals_dev, px_dev, sc_dev, ws_dev};
    return launched(h, fn, schur_cr_factor(fp, h->stream));
}

int32_t ctd_kkt_schur_cr_solve_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev) {
    const char* fn = "ctd_kkt_schur_cr_solve_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrPlan pl;
    if (const int32_t st = schur_cr_plan(h, fn, pl)) return st;
    if (const int32_t st = schur_check_solve_args(h, fn, ws_dev, r_dev, out_dev, true)) return st;
    const SchurCrSolveParams sp{pl.N, (int32_t)pl.block_rows, SCHUR_PLAIN, (int32_t)pl.n_levels, 0, ws_dev, r_dev, out_dev, nullptr};
    return launched(h, fn, schur_cr_solve(sp, h->stream));
}

int32_t ctd_kkt_schur_cr_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block) {
    const char* fn = "ctd_kkt_schur_cr_info";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrPlan pl;
    if (const int32_t st = schur_cr_plan(h, fn, pl)) return st;
    std::vector<int64_t> status;       // one word per block
    if (const int32_t st = schur_read_status(h, fn, ws_dev, first_bad_block, {kSchurCrTag, pl.N, pl.block_rows, pl.n_levels},
                                             -1, pl.N, status))
        return st;
    if (status.empty())
        return fail(h, CTD_EINVAL, std::string(fn) + ": the workspace holds no factor of this handle (ctd_kkt_schur_cr_factor_dev_async)");
    *first_bad_block = schur_first_set(status);
    return CTD_OK;
}

static constexpr MfOp kMrSchurCrStart = {{"ctd_kkt_minres_schur_cr_start_dev_async", "ctd_kkt_minres_schur_cr_start_dev_async", "ctd_kkt_minres_schur_cr_start_dev_async"},
                                         JIT_KKT, 0, false, false, false, "sys->x, rhs and z", "z"},
                      kMrSchurCrDev = {{"ctd_kkt_minres_schur_cr_dev", "ctd_kkt_minres_schur_cr_dev", "ctd_kkt_minres_schur_cr_dev"},
                                       JIT_KKT, 0, false, false, false, "sys->x, rhs and z", "z"};

int32_t ctd_kkt_minres_schur_cr_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                                double* z_dev, double rtol) {
    const MfCall c{kMrSchurCrStart, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, false, nullptr, &st)) return st;
    const OnDevice on(h, c.fn());
    if (on.st) return on.st;
    SchurCrPlan pl;
    if ((st = schur_cr_plan(h, c.fn(), pl))) return st;             // (whole grid, CSR order, the block size)
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_schur_check(h, c, sys, schur_ws_dev, rhs_dev, z_dev))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol))) return st;
    return mr_enqueue_start(h, c, *sys, rhs_dev, z_dev, rtol, INT64_MAX, schur_ws_dev, true);
}

int32_t ctd_kkt_minres_schur_cr_dev(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev, double* z_dev,
                                    double rtol, int64_t max_iter, int64_t check_every, ctd_minres_info* info) {
    const MfCall c{kMrSchurCrDev, MF_DEV};
    int32_t st;
    if (!mr_structs_ok(h, c.fn(), sys, true, info, &st)) return st;
    const OnDevice on(h, c.fn());
    if (on.st) return on.st;
    SchurCrPlan pl;
    if ((st = schur_cr_plan(h, c.fn(), pl))) return st;             // (whole grid, CSR order, the block size)
    if ((st = mr_check(on, h, c, sys, rhs_dev, z_dev, true))) return st;
    if ((st = mr_schur_check(h, c, sys, schur_ws_dev, rhs_dev, z_dev))) return st;
    if ((st = mr_check_rtol(h, c.fn(), rtol)) || (st = mr_check_count(h, c.fn(), "max_iter", max_iter)) ||
        (st = mr_check_count(h, c.fn(), "check_every", check_every)))
        return st;
    return mr_drive(h, c, *sys, rhs_dev, z_dev, rtol, max_iter, check_every, info, schur_ws_dev, true);
}

// ---- the solve on a shard of the grid (ownership, slots and summation order: ctd_krylov_shard_kernels.hpp) ------------------------
// The phases between which the caller exchanges the send slots: one launch each, no collective, no per-solve state in the handle.
static_assert(kKrylovSlot == CTD_KKT_MINRES_SHARD_SLOT, "the slot length of the header");
static_assert(kMaxNV <= kKrylovTailMax, "the nv tail entries fit a slot");
static void mrs_geom(int64_t n, int32_t* nwg, int64_t* chunk) {
    const KrylovGeom g = krylov_geom(n);
    *nwg = g.nwg;
    *chunk = g.chunk;
}
static KrylovShardPlan mrs_plan(const ctd_handle* h) { return plan_krylov_shard(h->model.L, h->step_begin, h->step_end, mrs_geom); }

// n_ranks, rank and the handle's steps: the steps must be able to be block `rank` of n_ranks ascending blocks of the grid
static int32_t check_ranks(ctd_handle* h, const char* fn, int32_t n_ranks, int32_t rank, bool with_rank) {
    const int64_t N = h->model.L.N, sb = h->step_begin, se = h->step_end;
    if (n_ranks < 1) return fail(h, CTD_EINVAL, std::string(fn) + ": n_ranks = " + std::to_string(n_ranks) + ", must be at least 1");
    if (n_ranks > N)
        return fail(h, CTD_EINVAL, std::string(fn) + ": n_ranks = " + std::to_string(n_ranks) + " exceeds the " + std::to_string(N) + " steps of the grid");
    if (!with_rank) return CTD_OK;
    if (rank < 0 || rank >= n_ranks)
        return fail(h, CTD_EINVAL, std::string(fn) + ": rank = " + std::to_string(rank) + " is outside [0, n_ranks = " + std::to_string(n_ranks) + ")");
    if ((rank == 0) != (sb == 0) || (rank == n_ranks - 1) != (se == N) || sb < rank || N - se < n_ranks - 1 - rank)
        return fail(h, CTD_EINVAL, std::string(fn) + ": the handle's steps [" + std::to_string(sb) + ", " + std::to_string(se) + ") of " +
                                       std::to_string(N) + " cannot be block rank = " + std::to_string(rank) + " of n_ranks = " +
                                       std::to_string(n_ranks) + " ascending blocks of the grid");
    return CTD_OK;
}

// What the phase families share (this one, ctd_kkt_minres_schur_cr_shard_* and ctd_kkt_minres_schur_cr_joint_* below); a family is
// data here: the length of its slots and, where it carries a factor, the length of the factor's workspace.
// The buffers of one call: the solve's workspace, cut with slots of `slot` doubles; z (n entries) and the factor's workspace where
// the call takes them (with_z, with_schur; null otherwise), so that a null pointer is refused by name
struct PhaseBufs {
    int64_t slot;
    const double* ws;
    bool with_z;
    const double* z;
    bool with_schur;
    const double* schur_ws;
};
// ... checked, for every phase and for start: the pointers by name (null, alignment), z against the workspace
// (CTD_KKT_MINRES_SHARD_WORKSPACE doubles for the family's slot), the factor's workspace (schur_len doubles) against both
static int32_t check_phase_buffers(ctd_handle* h, const char* fn, const PhaseBufs& b, int32_t n_ranks, int64_t schur_len) {
    int32_t st;
    if (b.with_z && (st = check_ptr(h, fn, "z", b.z))) return st;
    if ((st = check_ptr(h, fn, "ws", b.ws))) return st;
    if (b.with_schur && (st = check_ptr(h, fn, "schur_ws", b.schur_ws))) return st;
    const int64_t n = h->model.L.nvar + h->model.L.ncon, wlen = krylov_shard_workspace(n, n_ranks, b.slot);
    if (ranges_overlap(b.z, n, b.ws, wlen)) return fail(h, CTD_EINVAL, std::string(fn) + ": z and ws must be different buffers: z overlaps the workspace");
    if (ranges_overlap(b.schur_ws, schur_len, b.ws, wlen) || ranges_overlap(b.schur_ws, schur_len, b.z, n))
        return fail(h, CTD_EINVAL, std::string(fn) + ": schur_ws must not overlap z or the workspace");
    return CTD_OK;
}
// The prologue of a phase is, in every family: phase_rank -- the handle and its device (on), n_ranks / rank / the handle's steps --,
// the family's plan (the one step that is its own; it gives the length of the factor's workspace), check_phase_buffers
static int32_t phase_rank(const OnDevice& on, ctd_handle* h, const char* fn, int32_t n_ranks, int32_t rank) {
    return on.st ? on.st : check_ranks(h, fn, n_ranks, rank, true);
}
// start's own, behind its pointers and the buffers, in the header's order: the inputs (rhs, px, pc; null: none) as ranges against
// every output range; (the diagonal form's rule for px / pc, which its start has between the two;) then rtol and max_iter
static int32_t check_start_inputs(ctd_handle* h, const char* fn, const ctd_kkt_system* sys, const double* rhs, const PhaseBufs& b,
                                  int32_t n_ranks, int64_t schur_len) {
    const Layout& L = h->model.L;
    const int64_t n = L.nvar + L.ncon, wlen = krylov_shard_workspace(n, n_ranks, b.slot);
    const std::pair<const double*, int64_t> ins[] = {{rhs, n}, {sys->px, L.nvar}, {sys->pc, L.ncon}};
    for (const auto& in : ins)
        if (ranges_overlap(in.first, in.second, b.z, n) || ranges_overlap(in.first, in.second, b.ws, wlen) ||
            ranges_overlap(in.first, in.second, b.schur_ws, schur_len))
            return fail(h, CTD_EINVAL, std::string(fn) + ": the outputs (" + (b.with_schur ? "z, ws and schur_ws" : "z and ws") +
                                           ") must not overlap an input buffer");
    return CTD_OK;
}
static int32_t check_start_scalars(ctd_handle* h, const char* fn, double rtol, int64_t max_iter) {
    if (const int32_t st = mr_check_rtol(h, fn, rtol)) return st;
    return mr_check_count(h, fn, "max_iter", max_iter);
}
// the Krylov arguments of a call on the handle's shard: what the rank owns (mrs_plan), the workspace cut with `slot`
static KrylovShardParams shard_krylov_params(const ctd_handle* h, double* ws, double* z, int32_t n_ranks, int64_t slot) {
    const KrylovShardPlan pl = mrs_plan(h);
    const KrylovOwn own{pl.var_lo, pl.var_hi - pl.var_lo, pl.tail_lo, pl.tail_hi - pl.tail_lo, pl.row_lo, pl.last, n_ranks};
    return krylov_shard_params(ws, pl.n, pl.n_own, own, z, slot);
}
// the layout query behind the family's own checks
static int32_t fill_shard_layout(const ctd_handle* h, int32_t n_ranks, int64_t slot, ctd_minres_shard_layout* out) {
    const KrylovShardPlan pl = mrs_plan(h);
    const KrylovShardLayout l = krylov_shard_layout(pl.n, n_ranks, slot);
    out->reserved = 0;
    out->n = pl.n; out->n_ranks = n_ranks;
    out->var_begin = pl.var_lo; out->var_end = pl.var_hi;
    out->tail_begin = pl.tail_lo; out->tail_end = pl.tail_hi;
    out->row_begin = pl.row_lo; out->row_end = pl.row_hi;
    out->n_own = pl.n_own; out->n_dot = pl.n_dot; out->nwg = pl.nwg; out->chunk = pl.chunk;
    out->slot = slot;
    out->off_v = l.v; out->off_kv = l.kv;
    out->off_send_a = l.send_a; out->off_send_b = l.send_b;
    out->off_gathered_a = l.gathered_a; out->off_gathered_b = l.gathered_b;
    out->off_state = l.pend;
    out->workspace = krylov_shard_workspace(pl.n, n_ranks, slot);
    return CTD_OK;
}
// the info call of a family: the state words of its workspace
static int32_t shard_info(ctd_handle* h, const char* fn, const double* ws_dev, int32_t n_ranks, int64_t slot, ctd_minres_info* info) {
    if (!h || !STRUCT_OK(h, fn, "info", ctd_minres_info, info)) return CTD_EINVAL;
    const OnDevice on(h, fn);
    int32_t st;
    if ((st = on.st) || (st = check_ranks(h, fn, n_ranks, 0, false)) || (st = check_ptr(h, fn, "ws", ws_dev))) return st;
    return mr_read_info(h, ws_dev + krylov_shard_layout(h->model.L.nvar + h->model.L.ncon, n_ranks, slot).pend, info);
}

int32_t ctd_kkt_minres_shard_layout(ctd_handle* h, int32_t n_ranks, ctd_minres_shard_layout* out) {
    const char* fn = "ctd_kkt_minres_shard_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_minres_shard_layout, out)) return CTD_EINVAL;
    if (const int32_t st = check_ranks(h, fn, n_ranks, 0, false)) return st;
    return fill_shard_layout(h, n_ranks, kKrylovSlot, out);
}

int32_t ctd_kkt_minres_shard_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev,
                                             double* ws_dev, int32_t n_ranks, int32_t rank, double rtol, int64_t max_iter) {
    const char* fn = "ctd_kkt_minres_shard_start_dev_async";
    int32_t st;
    if (!mr_structs_ok(h, fn, sys, false, nullptr, &st)) return st;
    const OnDevice on(h, fn);
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = check_ptr(h, fn, "rhs", rhs_dev))) return st;
    if ((sys->px && (st = check_ptr(h, fn, "px", sys->px))) || (sys->pc && (st = check_ptr(h, fn, "pc", sys->pc)))) return st;
    const PhaseBufs b{kKrylovSlot, ws_dev, true, z_dev, false, nullptr};
    if ((st = check_phase_buffers(h, fn, b, n_ranks, 0)) || (st = check_start_inputs(h, fn, sys, rhs_dev, b, n_ranks, 0))) return st;
    if (!sys->px != !sys->pc)
        return fail(h, CTD_EINVAL, std::string(fn) + ": px and pc are given both (M = diag(1 / px, 1 / pc)) or neither (no preconditioner)");
    if ((st = check_start_scalars(h, fn, rtol, max_iter))) return st;
    return launched(h, fn, krylov_shard_start(shard_krylov_params(h, ws_dev, z_dev, n_ranks, kKrylovSlot), rhs_dev, sys->px, sys->pc,
                                              h->model.L.nvar, rtol, max_iter, h->stream));
}

// begin and the phases: one launch each; z is absent in begin
static int32_t mrs_phase(ctd_handle* h, const char* fn, double* z_dev, bool with_z, double* ws_dev, int32_t n_ranks, int32_t rank,
                         hipError_t (*launch)(const KrylovShardParams&, hipStream_t)) {
    const OnDevice on(h, fn);
    int32_t st;
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = check_phase_buffers(h, fn, {kKrylovSlot, ws_dev, with_z, z_dev, false, nullptr}, n_ranks, 0)))
        return st;
    return launched(h, fn, launch(shard_krylov_params(h, ws_dev, z_dev, n_ranks, kKrylovSlot), h->stream));
}
int32_t ctd_kkt_minres_shard_begin_dev_async(ctd_handle* h, double* ws_dev, int32_t n_ranks, int32_t rank) {
    return mrs_phase(h, "ctd_kkt_minres_shard_begin_dev_async", nullptr, false, ws_dev, n_ranks, rank, krylov_shard_begin);
}
int32_t ctd_kkt_minres_shard_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    return mrs_phase(h, "ctd_kkt_minres_shard_alfa_dev_async", z_dev, true, ws_dev, n_ranks, rank, krylov_shard_alfa);
}
int32_t ctd_kkt_minres_shard_lanczos_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    return mrs_phase(h, "ctd_kkt_minres_shard_lanczos_dev_async", z_dev, true, ws_dev, n_ranks, rank, krylov_shard_lanczos);
}
int32_t ctd_kkt_minres_shard_update_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    return mrs_phase(h, "ctd_kkt_minres_shard_update_dev_async", z_dev, true, ws_dev, n_ranks, rank, krylov_shard_update);
}

int32_t ctd_kkt_minres_shard_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info) {
    return shard_info(h, "ctd_kkt_minres_shard_info", ws_dev, n_ranks, kKrylovSlot, info);
}

// ---- the shard form of the log-depth exact Schur preconditioner (plan: ctd_schur_plan.hpp; the kernels of the whole-grid form
// through offset pointers: ctd_schur_cr_kernels.hpp) and of the solve that carries it (ctd_krylov_shard_kernels.hpp) -----------------
static_assert(kKrylovSchurSlot == CTD_KKT_MINRES_SCHUR_SHARD_SLOT, "the slot length of the header");
static_assert(kSlotSchurMax == kSchurMaxWg, "a slot has room for the solve's partial sums");
static_assert(CTD_KKT_MINRES_SCHUR_SHARD_WORKSPACE(10, 3) == kKrylovVectors * 10 + 8 * kKrylovSchurSlot + 96, "the workspace of the header");

// every handle is accepted; the plan's own refusals (CSR order, block_rows, the pattern -- walked once per handle)
static int32_t schur_crs_plan(ctd_handle* h, const char* fn, bool ranges, SchurCrShardPlan& pl) {
    std::string err;
    return schur_planned(h, fn, plan_kkt_schur_cr_shard(h->model, h->step_begin, h->step_end, !h->schur_verified, ranges, pl, err), err);
}
// the rank's blocks as the whole-grid problem of n_blocks blocks: the solve's arguments
static SchurCrShardSolveParams schur_crs_solve_params(const SchurCrShardPlan& pl, int32_t mode, double* ws, const double* r, double* out,
                                                      const KrylovState* cur, double* part) {
    SchurCrShardSolveParams sp{};
    static_cast<SchurCrSolveParams&>(sp) =
        SchurCrSolveParams{pl.n_blocks, (int32_t)pl.block_rows, mode, (int32_t)pl.n_levels, 0, ws, r + pl.first_row, out + pl.first_row, cur};
    sp.first = pl.step_begin;
    sp.part = part;
    return sp;
}

int32_t ctd_kkt_schur_cr_shard_layout(ctd_handle* h, ctd_schur_cr_shard_layout* out) {
    const char* fn = "ctd_kkt_schur_cr_shard_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_schur_cr_shard_layout, out)) return CTD_EINVAL;
    SchurCrShardPlan pl;
    if (const int32_t st = schur_crs_plan(h, fn, true, pl)) return st;
    out->reserved = 0;
    out->N = pl.N;
    out->step_begin = pl.step_begin;
    out->step_end = pl.step_end;
    out->n_blocks = pl.n_blocks;
    out->block_rows = pl.block_rows;
    out->first_row = pl.first_row;
    out->tail_rows = pl.tail_rows;
    out->first_tail_row = pl.first_tail_row;
    out->tail_cols = pl.tail_cols;
    out->n_levels = pl.n_levels;
    out->factor_launches = pl.factor_launches;
    out->solve_launches = pl.solve_launches;
    out->workspace = pl.workspace;
    out->jvals_begin = pl.jvals_begin;
    out->jvals_end = pl.jvals_end;
    out->px_begin = pl.px_begin;
    out->px_end = pl.px_end;
    return CTD_OK;
}

int32_t ctd_kkt_schur_cr_shard_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                                double* ws_dev) {
    const char* fn = "ctd_kkt_schur_cr_shard_factor_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrShardPlan pl;
    if (const int32_t st = schur_crs_plan(h, fn, false, pl)) return st;
    if (const int32_t st = schur_check_factor_args(h, fn, jvals_dev, px_dev, sc_dev, ws_dev)) return st;
    if (const int32_t st = schur_upload_pattern(h, fn)) return st;
    SchurCrShardFactorParams fp{};
    static_cast<SchurCrFactorParams&>(fp) =
        SchurCrFactorParams{pl.n_blocks, pl.first_tail_col, (int32_t)pl.block_rows, (int32_t)pl.n_levels, h->d_schur_rowptr.p + pl.first_row,
                            h->d_schur_colind.p, jvals_dev, px_dev, sc_dev ? sc_dev + pl.first_row : nullptr, ws_dev};
    fp.first = pl.step_begin;
    return launched(h, fn, schur_cr_factor(fp, h->stream));
}

int32_t ctd_kkt_schur_cr_shard_solve_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev) {
    const char* fn = "ctd_kkt_schur_cr_shard_solve_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrShardPlan pl;
    if (const int32_t st = schur_crs_plan(h, fn, false, pl)) return st;
    if (const int32_t st = schur_check_solve_args(h, fn, ws_dev, r_dev, out_dev, true)) return st;
    return launched(h, fn, schur_cr_solve(schur_crs_solve_params(pl, SCHUR_PLAIN, ws_dev, r_dev, out_dev, nullptr, nullptr), h->stream));
}

int32_t ctd_kkt_schur_cr_shard_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block) {
    const char* fn = "ctd_kkt_schur_cr_shard_info";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrShardPlan pl;
    if (const int32_t st = schur_crs_plan(h, fn, false, pl)) return st;
    std::vector<int64_t> status;       // one word per block of the rank
    if (const int32_t st = schur_read_status(h, fn, ws_dev, first_bad_block, {kSchurCrTag, pl.n_blocks, pl.block_rows, pl.n_levels, pl.step_begin},
                                             -1, pl.n_blocks, status))
        return st;
    if (status.empty())
        return fail(h, CTD_EINVAL, std::string(fn) + ": the workspace holds no factor of this handle's steps (ctd_kkt_schur_cr_shard_factor_dev_async)");
    const int64_t k = schur_first_set(status);
    *first_bad_block = k < 0 ? -1 : pl.step_begin + k;
    return CTD_OK;
}

// The phases of ctd_kkt_minres_shard_* with slots of kKrylovSchurSlot doubles
static KrylovSchurShardParams mrss_params(const ctd_handle* h, const SchurCrShardPlan& sc, double* ws, double* z, int32_t n_ranks) {
    KrylovSchurShardParams sp{};
    static_cast<KrylovShardParams&>(sp) = shard_krylov_params(h, ws, z, n_ranks, kKrylovSchurSlot);
    sp.s_lo = h->model.L.nvar + sc.first_row;
    sp.s_hi = sp.s_lo + sc.n_blocks * sc.block_rows;
    sp.s_nwg = schur_solve_grid(sc.n_blocks);
    return sp;
}

int32_t ctd_kkt_minres_schur_cr_shard_layout(ctd_handle* h, int32_t n_ranks, ctd_minres_shard_layout* out) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_minres_shard_layout, out)) return CTD_EINVAL;
    if (const int32_t st = check_ranks(h, fn, n_ranks, 0, false)) return st;
    SchurCrShardPlan sp;
    if (const int32_t st = schur_crs_plan(h, fn, false, sp)) return st;
    return fill_shard_layout(h, n_ranks, kKrylovSchurSlot, out);
}

int32_t ctd_kkt_minres_schur_cr_shard_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                                      double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank, double rtol,
                                                      int64_t max_iter) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_start_dev_async";
    int32_t st;
    if (!mr_structs_ok(h, fn, sys, false, nullptr, &st)) return st;
    const OnDevice on(h, fn);
    SchurCrShardPlan pl;
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = schur_crs_plan(h, fn, false, pl))) return st;
    if ((st = check_ptr(h, fn, "rhs", rhs_dev)) || (st = check_ptr(h, fn, "px", sys->px)) || (st = check_ptr(h, fn, "pc", sys->pc))) return st;
    const PhaseBufs b{kKrylovSchurSlot, ws_dev, true, z_dev, true, schur_ws_dev};
    if ((st = check_phase_buffers(h, fn, b, n_ranks, pl.workspace)) ||
        (st = check_start_inputs(h, fn, sys, rhs_dev, b, n_ranks, pl.workspace)) || (st = check_start_scalars(h, fn, rtol, max_iter)))
        return st;
    const KrylovSchurShardParams sp = mrss_params(h, pl, ws_dev, z_dev, n_ranks);
    const int64_t nvar = h->model.L.nvar;
    hipError_t e = krylov_schur_shard_start(sp, rhs_dev, sys->px, sys->pc, nvar, rtol, max_iter, h->stream);
    if (e == hipSuccess)
        e = schur_cr_solve(schur_crs_solve_params(pl, SCHUR_START, schur_ws_dev, sp.r2 + nvar, sp.y + nvar, sp.cur, sp.send_a + kSlotSchur),
                           h->stream);
    return launched(h, fn, e);
}

// the prologue of the phases, with this family's plan
static int32_t mrss_phase(const OnDevice& on, ctd_handle* h, const char* fn, const PhaseBufs& b, int32_t n_ranks, int32_t rank,
                          SchurCrShardPlan& pl) {
    int32_t st;
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = schur_crs_plan(h, fn, false, pl))) return st;
    return check_phase_buffers(h, fn, b, n_ranks, pl.workspace);
}
int32_t ctd_kkt_minres_schur_cr_shard_begin_dev_async(ctd_handle* h, double* ws_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_begin_dev_async";
    const OnDevice on(h, fn);
    SchurCrShardPlan pl;
    if (const int32_t st = mrss_phase(on, h, fn, {kKrylovSchurSlot, ws_dev, false, nullptr, false, nullptr}, n_ranks, rank, pl)) return st;
    return launched(h, fn, krylov_schur_shard_begin(mrss_params(h, pl, ws_dev, nullptr, n_ranks), h->stream));
}
int32_t ctd_kkt_minres_schur_cr_shard_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_alfa_dev_async";
    const OnDevice on(h, fn);
    SchurCrShardPlan pl;
    if (const int32_t st = mrss_phase(on, h, fn, {kKrylovSchurSlot, ws_dev, true, z_dev, false, nullptr}, n_ranks, rank, pl)) return st;
    return launched(h, fn, krylov_shard_alfa(mrss_params(h, pl, ws_dev, z_dev, n_ranks), h->stream));
}
int32_t ctd_kkt_minres_schur_cr_shard_lanczos_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev, int32_t n_ranks,
                                                        int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_lanczos_dev_async";
    const OnDevice on(h, fn);
    SchurCrShardPlan pl;
    if (const int32_t st = mrss_phase(on, h, fn, {kKrylovSchurSlot, ws_dev, true, z_dev, true, schur_ws_dev}, n_ranks, rank, pl)) return st;
    const KrylovSchurShardParams sp = mrss_params(h, pl, ws_dev, z_dev, n_ranks);
    const int64_t nvar = h->model.L.nvar;
    hipError_t e = krylov_schur_shard_lanczos(sp, h->stream);
    if (e == hipSuccess)
        e = schur_cr_solve(schur_crs_solve_params(pl, SCHUR_ITER, schur_ws_dev, sp.r2 + nvar, sp.y + nvar, sp.cur, sp.send_b + kSlotSchur),
                           h->stream);
    return launched(h, fn, e);
}
int32_t ctd_kkt_minres_schur_cr_shard_update_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_shard_update_dev_async";
    const OnDevice on(h, fn);
    SchurCrShardPlan pl;
    if (const int32_t st = mrss_phase(on, h, fn, {kKrylovSchurSlot, ws_dev, true, z_dev, false, nullptr}, n_ranks, rank, pl)) return st;
    return launched(h, fn, krylov_schur_shard_update(mrss_params(h, pl, ws_dev, z_dev, n_ranks), h->stream));
}

int32_t ctd_kkt_minres_schur_cr_shard_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info) {
    return shard_info(h, "ctd_kkt_minres_schur_cr_shard_info", ws_dev, n_ranks, kKrylovSchurSlot, info);
}

// ---- the joined form of the log-depth Schur preconditioner (plan: ctd_schur_plan.hpp; kernels: ctd_schur_cr_joint_kernels.hpp) ---------
static_assert(kSchurJointMaxRanks == CTD_KKT_SCHUR_CR_JOINT_MAX_RANKS, "the largest n_ranks of the header");
static_assert(kSchurJointSolveSlot == CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT, "the solve record of the header");
static_assert(schur_cr_joint_factor_slot(9) == CTD_KKT_SCHUR_CR_JOINT_FACTOR_SLOT(9), "the factor record of the header");

// every handle is accepted; the plan's own refusals (CSR order, block_rows, the pattern -- walked once per handle --, the split)
static int32_t schur_crj_plan(ctd_handle* h, const char* fn, int32_t n_ranks, int32_t rank, bool ranges, SchurCrJointPlan& pl) {
    std::string err;
    return schur_planned(h, fn, plan_kkt_schur_cr_joint(h->model, n_ranks, rank, h->step_begin, h->step_end, !h->schur_verified, ranges, pl, err), err);
}
static SchurCrJointId schur_crj_id(const SchurCrJointPlan& pl) {
    return SchurCrJointId{pl.step_begin, pl.step_end, (int32_t)pl.n_ranks, (int32_t)pl.rank};
}
// the arguments of the family's own kernels; the pattern must have been uploaded for the factor (the solves do not read it)
static SchurCrJointParams schur_crj_params(const ctd_handle* h, const SchurCrJointPlan& pl, double* ws) {
    SchurCrJointParams p{};
    p.N = pl.N;
    p.n_int = pl.n_int;
    p.v_off = pl.first_tail_col;
    p.int_begin = pl.int_begin;
    p.id = schur_crj_id(pl);
    p.m = (int32_t)pl.block_rows;
    p.n_levels = (int32_t)pl.n_levels;
    p.mode = SCHUR_PLAIN;
    p.rowptr = h->d_schur_rowptr.p;
    p.colind = h->d_schur_colind.p;
    p.ws = ws;
    p.off_es = pl.off_es; p.off_eb = pl.off_eb; p.off_ds = pl.off_ds; p.off_wl = pl.off_wl; p.off_wr = pl.off_wr;
    p.off_scratch = pl.off_scratch; p.off_reduced = pl.off_reduced; p.off_rs = pl.off_rs; p.off_xs = pl.off_xs; p.off_sigma = pl.off_sigma;
    p.workspace = pl.workspace;
    return p;
}
// the interior as the whole-grid problem of n_int blocks: the solve's arguments
static SchurCrJointSolveParams schur_crj_solve_params(const SchurCrJointPlan& pl, int32_t mode, double* ws, const double* r, double* out,
                                                      const KrylovState* cur, double* part) {
    SchurCrJointSolveParams sp{};
    const int64_t row0 = pl.int_begin * pl.block_rows;
    static_cast<SchurCrSolveParams&>(sp) =
        SchurCrSolveParams{pl.n_int, (int32_t)pl.block_rows, mode, (int32_t)pl.n_levels, 0, ws, r + row0, out + row0, cur};
    sp.first = pl.int_begin;
    sp.part = part;
    sp.id = schur_crj_id(pl);
    return sp;
}
// [p, p + n) against the workspace
static int32_t schur_crj_disjoint(ctd_handle* h, const char* fn, const char* name, const double* p, int64_t n, const double* ws,
                                  const SchurCrJointPlan& pl) {
    if (ranges_overlap(p, n, ws, pl.workspace)) return fail(h, CTD_EINVAL, std::string(fn) + ": " + name + " overlaps the workspace");
    return CTD_OK;
}

int32_t ctd_kkt_schur_cr_joint_layout(ctd_handle* h, int32_t n_ranks, int32_t rank, ctd_schur_cr_joint_layout* out) {
    const char* fn = "ctd_kkt_schur_cr_joint_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_schur_cr_joint_layout, out)) return CTD_EINVAL;
    SchurCrJointPlan pl;
    if (const int32_t st = schur_crj_plan(h, fn, n_ranks, rank, true, pl)) return st;
    out->reserved = 0;
    out->N = pl.N; out->n_ranks = pl.n_ranks; out->rank = pl.rank;
    out->step_begin = pl.step_begin; out->step_end = pl.step_end;
    out->separator = pl.separator; out->int_begin = pl.int_begin; out->n_int = pl.n_int;
    out->block_rows = pl.block_rows; out->first_row = pl.first_row;
    out->tail_rows = pl.tail_rows; out->first_tail_row = pl.first_tail_row; out->tail_cols = pl.tail_cols;
    out->n_levels = pl.n_levels; out->n_sep = pl.n_sep;
    out->factor_local_launches = pl.factor_local_launches; out->factor_join_launches = pl.factor_join_launches;
    out->solve_local_launches = pl.solve_local_launches; out->solve_join_launches = pl.solve_join_launches;
    out->factor_slot = pl.factor_slot; out->solve_slot = pl.solve_slot;
    out->off_es = pl.off_es; out->off_eb = pl.off_eb; out->off_ds = pl.off_ds; out->off_wl = pl.off_wl; out->off_wr = pl.off_wr;
    out->off_scratch = pl.off_scratch; out->off_reduced = pl.off_reduced; out->off_rs = pl.off_rs; out->off_xs = pl.off_xs;
    out->off_sigma = pl.off_sigma;
    out->workspace = pl.workspace;
    out->jvals_begin = pl.jvals_begin; out->jvals_end = pl.jvals_end;
    out->jvals_halo_begin = pl.jvals_halo_begin; out->jvals_halo_end = pl.jvals_halo_end;
    out->px_begin = pl.px_begin; out->px_end = pl.px_end;
    return CTD_OK;
}

int32_t ctd_kkt_schur_cr_joint_factor_local_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                                      double* ws_dev, double* send_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_schur_cr_joint_factor_local_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrJointPlan pl;
    int32_t st;
    if ((st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    if ((st = check_ptr(h, fn, "jvals", jvals_dev)) || (st = check_ptr(h, fn, "px", px_dev)) || (st = check_ptr(h, fn, "ws", ws_dev)))
        return st;
    if (sc_dev && (st = check_ptr(h, fn, "sc", sc_dev))) return st;
    if (n_ranks > 1 && (st = check_ptr(h, fn, "send", send_dev))) return st;
    const Layout& L = h->model.L;
    if ((st = schur_crj_disjoint(h, fn, "jvals", jvals_dev, h->model.nnzj, ws_dev, pl)) || (st = schur_crj_disjoint(h, fn, "px", px_dev, L.nvar, ws_dev, pl)) ||
        (st = schur_crj_disjoint(h, fn, "sc", sc_dev, L.ncon, ws_dev, pl)) ||
        (n_ranks > 1 && (st = schur_crj_disjoint(h, fn, "send", send_dev, pl.factor_slot, ws_dev, pl))))
        return st;
    if (n_ranks > 1 && (ranges_overlap(send_dev, pl.factor_slot, jvals_dev, h->model.nnzj) || ranges_overlap(send_dev, pl.factor_slot, px_dev, L.nvar) ||
                        ranges_overlap(send_dev, pl.factor_slot, sc_dev, L.ncon)))
        return fail(h, CTD_EINVAL, std::string(fn) + ": the outputs (ws and send) must not overlap an input buffer");
    if ((st = schur_upload_pattern(h, fn))) return st;
    SchurCrJointParams p = schur_crj_params(h, pl, ws_dev);
    p.jvals = jvals_dev;
    p.px = px_dev;
    p.sc = sc_dev;
    p.send = send_dev;
    const int64_t row0 = pl.int_begin * pl.block_rows;
    SchurCrJointFactorParams fp{};
    static_cast<SchurCrFactorParams&>(fp) =
        SchurCrFactorParams{pl.n_int, pl.first_tail_col, (int32_t)pl.block_rows, (int32_t)pl.n_levels, h->d_schur_rowptr.p + row0,
                            h->d_schur_colind.p, jvals_dev, px_dev, sc_dev ? sc_dev + row0 : nullptr, ws_dev};
    fp.first = pl.int_begin;
    fp.id = p.id;
    hipError_t e = n_ranks > 1 ? schur_cr_joint_interface(p, h->stream) : hipSuccess;      // (one rank: no interface, nothing behind the interior's part is read)
    if (e == hipSuccess) e = schur_cr_factor(fp, h->stream);
    if (e == hipSuccess && n_ranks > 1) e = schur_cr_joint_spikes(p, h->stream);
    return launched(h, fn, e);
}

int32_t ctd_kkt_schur_cr_joint_factor_join_dev_async(ctd_handle* h, double* ws_dev, const double* gathered_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_schur_cr_joint_factor_join_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrJointPlan pl;
    int32_t st;
    if ((st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    if ((st = check_ptr(h, fn, "ws", ws_dev))) return st;
    if (n_ranks == 1) return CTD_OK;
    if ((st = check_ptr(h, fn, "gathered", gathered_dev))) return st;
    if ((st = schur_crj_disjoint(h, fn, "gathered", gathered_dev, n_ranks * pl.factor_slot, ws_dev, pl))) return st;
    SchurCrJointParams p = schur_crj_params(h, pl, ws_dev);
    p.gathered = gathered_dev;
    p.slot = pl.factor_slot;
    return launched(h, fn, schur_cr_joint_factor_join(p, h->stream));
}

int32_t ctd_kkt_schur_cr_joint_solve_local_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev, double* send_dev,
                                                     int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_schur_cr_joint_solve_local_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrJointPlan pl;
    int32_t st;
    if ((st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    if ((st = check_ptr(h, fn, "ws", ws_dev)) || (st = check_ptr(h, fn, "r", r_dev)) || (st = check_ptr(h, fn, "out", out_dev)))
        return st;
    if (n_ranks > 1 && (st = check_ptr(h, fn, "send", send_dev))) return st;
    const int64_t ncon = h->model.L.ncon;
    if (ranges_overlap(out_dev, ncon, r_dev, ncon)) return fail(h, CTD_EINVAL, std::string(fn) + ": the output (out) must not overlap r");
    if ((st = schur_crj_disjoint(h, fn, "r", r_dev, ncon, ws_dev, pl)) || (st = schur_crj_disjoint(h, fn, "out", out_dev, ncon, ws_dev, pl)))
        return st;
    if (n_ranks > 1 && (ranges_overlap(send_dev, pl.solve_slot, r_dev, ncon) || ranges_overlap(send_dev, pl.solve_slot, out_dev, ncon) ||
                        ranges_overlap(send_dev, pl.solve_slot, ws_dev, pl.workspace)))
        return fail(h, CTD_EINVAL, std::string(fn) + ": send must not overlap r, out or the workspace");
    hipError_t e = schur_cr_solve(schur_crj_solve_params(pl, SCHUR_PLAIN, ws_dev, r_dev, out_dev, nullptr, nullptr), h->stream);
    if (e == hipSuccess && n_ranks > 1) {
        SchurCrJointParams p = schur_crj_params(h, pl, ws_dev);
        p.r = r_dev;
        p.out = out_dev;
        p.send = send_dev;
        e = schur_cr_joint_solve_record(p, h->stream);
    }
    return launched(h, fn, e);
}

int32_t ctd_kkt_schur_cr_joint_solve_join_dev_async(ctd_handle* h, double* ws_dev, const double* gathered_dev, double* out_dev, int32_t n_ranks,
                                                    int32_t rank) {
    const char* fn = "ctd_kkt_schur_cr_joint_solve_join_dev_async";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrJointPlan pl;
    int32_t st;
    if ((st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    if ((st = check_ptr(h, fn, "ws", ws_dev)) || (st = check_ptr(h, fn, "out", out_dev))) return st;
    if (n_ranks == 1) return CTD_OK;
    if ((st = check_ptr(h, fn, "gathered", gathered_dev))) return st;
    const int64_t ncon = h->model.L.ncon, glen = n_ranks * pl.solve_slot;
    if ((st = schur_crj_disjoint(h, fn, "gathered", gathered_dev, glen, ws_dev, pl)) || (st = schur_crj_disjoint(h, fn, "out", out_dev, ncon, ws_dev, pl)))
        return st;
    if (ranges_overlap(gathered_dev, glen, out_dev, ncon)) return fail(h, CTD_EINVAL, std::string(fn) + ": the output (out) must not overlap gathered");
    SchurCrJointParams p = schur_crj_params(h, pl, ws_dev);
    p.gathered = gathered_dev;
    p.slot = pl.solve_slot;
    p.out = out_dev;
    return launched(h, fn, schur_cr_joint_solve_join(p, h->stream));
}

int32_t ctd_kkt_schur_cr_joint_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, int32_t rank, int64_t* first_bad_block) {
    const char* fn = "ctd_kkt_schur_cr_joint_info";
    const OnDevice on(h, fn);
    if (on.st) return on.st;
    SchurCrJointPlan pl;
    if (const int32_t st = schur_crj_plan(h, fn, n_ranks, rank, false, pl)) return st;
    std::vector<int64_t> status;       // one word per block of the interior
    if (const int32_t st = schur_read_status(h, fn, ws_dev, first_bad_block,
                                             {kSchurCrJointTag, pl.n_int, pl.block_rows, pl.n_levels, pl.int_begin, pl.step_begin, pl.step_end,
                                              pl.n_ranks, pl.rank},
                                             -1, pl.n_int, status))
        return st;
    if (status.empty())
        return fail(h, CTD_EINVAL, std::string(fn) + ": the workspace holds no factor of this handle's steps as rank " + std::to_string(rank) + " of " +
                                       std::to_string(n_ranks) + " (ctd_kkt_schur_cr_joint_factor_local_dev_async)");
    std::vector<int64_t> red((size_t)pl.n_sep);       // ... and per separator of the reduced factor
    HIP_TRY(h, hipMemcpy(red.data(), ws_dev + pl.off_reduced, sizeof(int64_t) * red.size(), hipMemcpyDeviceToHost));
    int64_t bad = schur_first_set(status);
    if (bad >= 0) bad += pl.int_begin;
    for (int64_t k = 0; k < pl.n_ranks - 1; ++k)
        if (red[(size_t)k] >= 0 && (bad < 0 || red[(size_t)k] < bad)) bad = red[(size_t)k];
    *first_bad_block = bad;
    return CTD_OK;
}

// The phases of ctd_kkt_minres_schur_cr_shard_* with M of the joined form: slots of kKrylovSchurJointSlot doubles
static_assert(kKrylovSchurJointSlot == CTD_KKT_MINRES_SCHUR_JOINT_SLOT, "the slot length of the header");
static_assert(kKrylovSchurJointSlot - kSlotJoint == kSchurJointSolveSlot, "the solve record fits behind the Schur form's slot");
static_assert(CTD_KKT_MINRES_SCHUR_JOINT_WORKSPACE(10, 3) == kKrylovVectors * 10 + 8 * kKrylovSchurJointSlot + 96, "the workspace of the header");

static KrylovSchurJointParams mrsj_params(const ctd_handle* h, const SchurCrJointPlan& sc, double* ws, double* z, const double* schur_ws) {
    KrylovSchurJointParams sp{};
    static_cast<KrylovShardParams&>(sp) = shard_krylov_params(h, ws, z, (int32_t)sc.n_ranks, kKrylovSchurJointSlot);
    sp.s_lo = h->model.L.nvar + sc.first_row;
    sp.s_hi = h->model.L.nvar + sc.step_end * sc.block_rows;
    sp.s_nwg = schur_solve_grid(sc.n_int);
    sp.sigma = schur_ws ? schur_ws + sc.off_sigma : nullptr;
    return sp;
}
// the prologue of the phases, with this family's plan
static int32_t mrsj_phase(const OnDevice& on, ctd_handle* h, const char* fn, const PhaseBufs& b, int32_t n_ranks, int32_t rank,
                          SchurCrJointPlan& pl) {
    int32_t st;
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    return check_phase_buffers(h, fn, b, n_ranks, pl.workspace);
}
// behind start's and (B)'s launch: the interior's solve with its partial sums into the send slot, then the solve record behind them
static hipError_t mrsj_local(const ctd_handle* h, const SchurCrJointPlan& pl, const KrylovSchurJointParams& sp, int32_t mode, double* schur_ws,
                             double* send) {
    const int64_t nvar = h->model.L.nvar;
    hipError_t e = schur_cr_solve(schur_crj_solve_params(pl, mode, schur_ws, sp.r2 + nvar, sp.y + nvar, sp.cur, send + kSlotSchur), h->stream);
    if (e != hipSuccess || pl.n_ranks == 1) return e;
    SchurCrJointParams p = schur_crj_params(h, pl, schur_ws);
    p.mode = mode;
    p.cur = sp.cur;
    p.r = sp.r2 + nvar;
    p.out = sp.y + nvar;
    p.send = send + kSlotJoint;
    return schur_cr_joint_solve_record(p, h->stream);
}
// ahead of begin's and (C)'s launch: the reduced solve from the gathered records (sigma), the correction of y on the rank's block rows
static hipError_t mrsj_join(const ctd_handle* h, const SchurCrJointPlan& pl, const KrylovSchurJointParams& sp, int32_t mode, double* schur_ws,
                            const double* gathered) {
    if (pl.n_ranks == 1) return hipSuccess;
    SchurCrJointParams p = schur_crj_params(h, pl, schur_ws);
    p.mode = mode;
    p.cur = sp.cur;
    p.out = sp.y + h->model.L.nvar;
    p.gathered = gathered + kSlotJoint;
    p.slot = kKrylovSchurJointSlot;
    return schur_cr_joint_solve_join(p, h->stream);
}

int32_t ctd_kkt_minres_schur_cr_joint_layout(ctd_handle* h, int32_t n_ranks, int32_t rank, ctd_minres_shard_layout* out) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_layout";
    if (!h || !STRUCT_OK(h, fn, "layout", ctd_minres_shard_layout, out)) return CTD_EINVAL;
    int32_t st;
    SchurCrJointPlan sp;
    if ((st = check_ranks(h, fn, n_ranks, rank, true)) || (st = schur_crj_plan(h, fn, n_ranks, rank, false, sp))) return st;
    return fill_shard_layout(h, n_ranks, kKrylovSchurJointSlot, out);
}

int32_t ctd_kkt_minres_schur_cr_joint_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                                      double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank, double rtol,
                                                      int64_t max_iter) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_start_dev_async";
    int32_t st;
    if (!mr_structs_ok(h, fn, sys, false, nullptr, &st)) return st;
    const OnDevice on(h, fn);
    SchurCrJointPlan pl;
    if ((st = phase_rank(on, h, fn, n_ranks, rank)) || (st = schur_crj_plan(h, fn, n_ranks, rank, false, pl))) return st;
    if ((st = check_ptr(h, fn, "rhs", rhs_dev)) || (st = check_ptr(h, fn, "px", sys->px)) || (st = check_ptr(h, fn, "pc", sys->pc))) return st;
    const PhaseBufs b{kKrylovSchurJointSlot, ws_dev, true, z_dev, true, schur_ws_dev};
    if ((st = check_phase_buffers(h, fn, b, n_ranks, pl.workspace)) ||
        (st = check_start_inputs(h, fn, sys, rhs_dev, b, n_ranks, pl.workspace)) || (st = check_start_scalars(h, fn, rtol, max_iter)))
        return st;
    const KrylovSchurJointParams sp = mrsj_params(h, pl, ws_dev, z_dev, schur_ws_dev);
    hipError_t e = krylov_schur_joint_start(sp, rhs_dev, sys->px, sys->pc, h->model.L.nvar, rtol, max_iter, h->stream);
    if (e == hipSuccess) e = mrsj_local(h, pl, sp, SCHUR_START, schur_ws_dev, sp.send_a);
    return launched(h, fn, e);
}
int32_t ctd_kkt_minres_schur_cr_joint_begin_dev_async(ctd_handle* h, double* schur_ws_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_begin_dev_async";
    const OnDevice on(h, fn);
    SchurCrJointPlan pl;
    if (const int32_t st = mrsj_phase(on, h, fn, {kKrylovSchurJointSlot, ws_dev, false, nullptr, true, schur_ws_dev}, n_ranks, rank, pl)) return st;
    const KrylovSchurJointParams sp = mrsj_params(h, pl, ws_dev, nullptr, schur_ws_dev);
    hipError_t e = mrsj_join(h, pl, sp, SCHUR_START, schur_ws_dev, sp.gathered_a);
    if (e == hipSuccess) e = krylov_schur_joint_begin(sp, h->stream);
    return launched(h, fn, e);
}
int32_t ctd_kkt_minres_schur_cr_joint_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_alfa_dev_async";
    const OnDevice on(h, fn);
    SchurCrJointPlan pl;
    if (const int32_t st = mrsj_phase(on, h, fn, {kKrylovSchurJointSlot, ws_dev, true, z_dev, false, nullptr}, n_ranks, rank, pl)) return st;
    return launched(h, fn, krylov_shard_alfa(mrsj_params(h, pl, ws_dev, z_dev, nullptr), h->stream));
}
int32_t ctd_kkt_minres_schur_cr_joint_lanczos_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev, int32_t n_ranks,
                                                        int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_lanczos_dev_async";
    const OnDevice on(h, fn);
    SchurCrJointPlan pl;
    if (const int32_t st = mrsj_phase(on, h, fn, {kKrylovSchurJointSlot, ws_dev, true, z_dev, true, schur_ws_dev}, n_ranks, rank, pl)) return st;
    const KrylovSchurJointParams sp = mrsj_params(h, pl, ws_dev, z_dev, schur_ws_dev);
    hipError_t e = krylov_schur_joint_lanczos(sp, h->stream);
    if (e == hipSuccess) e = mrsj_local(h, pl, sp, SCHUR_ITER, schur_ws_dev, sp.send_b);
    return launched(h, fn, e);
}
int32_t ctd_kkt_minres_schur_cr_joint_update_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev, int32_t n_ranks,
                                                       int32_t rank) {
    const char* fn = "ctd_kkt_minres_schur_cr_joint_update_dev_async";
    const OnDevice on(h, fn);
    SchurCrJointPlan pl;
    if (const int32_t st = mrsj_phase(on, h, fn, {kKrylovSchurJointSlot, ws_dev, true, z_dev, true, schur_ws_dev}, n_ranks, rank, pl)) return st;
    const KrylovSchurJointParams sp = mrsj_params(h, pl, ws_dev, z_dev, schur_ws_dev);
    hipError_t e = mrsj_join(h, pl, sp, SCHUR_ITER, schur_ws_dev, sp.gathered_b);
    if (e == hipSuccess) e = krylov_schur_joint_update(sp, h->stream);
    return launched(h, fn, e);
}
int32_t ctd_kkt_minres_schur_cr_joint_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info) {
    return shard_info(h, "ctd_kkt_minres_schur_cr_joint_info", ws_dev, n_ranks, kKrylovSchurJointSlot, info);
}

int32_t ctd_obj(ctd_handle* h, const double* x, double* f) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x || !f) return fail(h, CTD_EINVAL, "null argument");
    return host_call(h, {{x, h->d_x, h->model.L.nvar}}, [&] { return enqueue_obj(h, h->d_x.p, h->d_obj.p); }, {{f, h->d_obj, 1}});
}

int32_t ctd_debug_stamps(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev, uint64_t* out, int64_t cap) {
    if (!h || !out) return CTD_EINVAL;
    const OnDevice on(h);
    if (on.st) return on.st;
    int64_t words = (int64_t)h->plan.grid * 12;
    if (cap < words) return fail(h, CTD_EINVAL, "stamp buffer too small");
    if (cap >= (int64_t)h->plan.grid * 28) words = (int64_t)h->plan.grid * 28;      // + sub-stamps of experiment builds (CTD_SUBSTAMPS)
    unsigned long long* d_st = nullptr;
    HIP_TRY(h, hipMalloc((void**)&d_st, sizeof(unsigned long long) * words));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * words, h->stream));
    int32_t st = enqueue_cons_jac(h, x_dev, c_dev, vals_dev);     // warm, no stamps
    if (st == CTD_OK) {
        h->plan.kp.stamps = d_st;
        st = enqueue_cons_jac(h, x_dev, c_dev, vals_dev);
        h->plan.kp.stamps = nullptr;
    }
    if (st == CTD_OK) {
        hipError_t e = hipMemcpyAsync(out, d_st, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) st = fail(h, CTD_EHIP, hipGetErrorString(e));
    }
    (void)hipFree(d_st);
    return st;
}

// Mean duration of one dispatch of a kernel, measured the way the timed region of bench.py runs it: the launches are
// enqueued back to back in batches (the GPU stays busy, clocks stay up), every launch carries its own pair of dispatch
// events (start / stop timestamps taken by the dispatch of THAT kernel on the handle's stream), one synchronisation per batch
static int32_t time_dispatches(ctd_handle* h, int32_t iters, double* mean_ms,
                               const std::function<int32_t(hipEvent_t, hipEvent_t)>& launch) {
    constexpr int kBatch = 32;
    DeviceGuard dg_(h->device); HIP_TRY(h, dg_.err);
    static thread_local std::map<int, std::vector<hipEvent_t>> ev_by_device;    // events belong to the device they were created on
    std::vector<hipEvent_t>& ev = ev_by_device[h->device];
    if (ev.empty()) ev.assign(2 * kBatch, nullptr);
    for (hipEvent_t& e : ev)
        if (!e) HIP_TRY(h, hipEventCreate(&e));
    int32_t st = launch(nullptr, nullptr);   // warm
    if (st) return st;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double total = 0.0;
    for (int done = 0; done < iters;) {
        const int nb = iters - done < kBatch ? iters - done : kBatch;
        for (int i = 0; i < nb; ++i) {
            st = launch(ev[2 * i], ev[2 * i + 1]);
            if (st) return st;
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < nb; ++i) {
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            total += (double)ms;
        }
        done += nb;
    }
    *mean_ms = total / iters;
    return CTD_OK;
}

int32_t ctd_time_cons_jac_dev(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev, int32_t iters, double* mean_ms) {
    if (!h || !mean_ms || iters < 1) return CTD_EINVAL;
    const OnDevice on(h);
    if (on.st) return on.st;
    return time_dispatches(h, iters, mean_ms, [&](hipEvent_t a, hipEvent_t b) { return enqueue_cons_jac(h, x_dev, c_dev, vals_dev, a, b); });
}

// ---- Hessian of the Lagrangian ----------------------------------------------------------------------------------------

int32_t ctd_hess_structure(const ctd_handle* h, int64_t* rows, int64_t* cols) {
    if (!h || !rows || !cols) return CTD_EINVAL;
    const Model& mo = h->model;
    std::vector<int64_t> r;
    int64_t k = 0;
    for (int64_t j = 0; j < mo.L.nvar; ++j) {
        mo.hess_gen_column(j, r);
        for (int64_t row : r) { rows[k] = row + 1; cols[k] = j + 1; ++k; }
    }
    return CTD_OK;
}

int32_t ctd_hess_csc(const ctd_handle* h, int64_t* colptr, int64_t* rowval);
// upper triangle by rows = lower triangle by columns (symmetric matrix): the same arrays, the same value order
int32_t ctd_hess_csr(const ctd_handle* h, int64_t* rowptr, int64_t* colind) { return ctd_hess_csc(h, rowptr, colind); }

int32_t ctd_hess_csc(const ctd_handle* h, int64_t* colptr, int64_t* rowval) {
    if (!h || !colptr || !rowval) return CTD_EINVAL;
    const Model& mo = h->model;
    std::vector<int64_t> r;
    int64_t k = 0;
    for (int64_t j = 0; j < mo.L.nvar; ++j) {
        colptr[j] = k;
        mo.hess_gen_column(j, r);
        for (int64_t row : r) rowval[k++] = row;
    }
    colptr[mo.L.nvar] = k;
    return k == mo.H.nnzh ? CTD_OK : CTD_EPATTERN;
}

static int32_t ensure_hess(ctd_handle* h) {
    if (h->hess_ready) return CTD_OK;
    const Model& mo = h->model;
    const HessModel& H = mo.H;
    DeviceGuard dg_(h->device); HIP_TRY(h, dg_.err);
    h->hess_tile = env_int("CTD_HESS_TILE", 0);
    if (h->hess_tile <= 0) h->hess_tile = default_hess_tile(mo);
    mo.fill_hparams(h->hp, h->hess_tile, h->step_begin, h->step_end);
    h->hess_lds_bytes = (size_t)hess_lds_doubles(h->hp) * sizeof(double);
    const size_t hess_cap = h->rt ? 64 * 1024 : 96 * 1024;
    while (h->hess_lds_bytes > hess_cap && h->hess_tile > 1) {
        h->hess_tile = (h->hess_tile + 1) / 2;
        mo.fill_hparams(h->hp, h->hess_tile, h->step_begin, h->step_end);
        h->hess_lds_bytes = (size_t)hess_lds_doubles(h->hp) * sizeof(double);
    }
    if (h->hess_lds_bytes > (h->rt ? 64u : 160u) * 1024) return fail(h, CTD_EINVAL, "Hessian records of one step do not fit the LDS");
    if (const int32_t jst = jit_load(h, JIT_HESS)) return jst;
    HIP_TRY(h, upload(h->d_htptr, H.ctptr));
    HIP_TRY(h, upload(h->d_hcpos, H.cpos));
    HIP_TRY(h, upload(h->d_hzpos, H.zpos));
    HIP_TRY(h, upload(h->d_hterms, H.tcode));
    HIP_TRY(h, upload(h->d_hpair_c, H.pair_c));
    HIP_TRY(h, upload(h->d_hvptr, H.vptr));
    HIP_TRY(h, upload(h->d_hvterms, H.vterms));
    HIP_TRY(h, upload(h->d_hedge_idx, H.edge_idx));
    HIP_TRY(h, upload(h->d_heptr, H.eptr));
    HIP_TRY(h, upload(h->d_hevptr, H.evptr));
    HIP_TRY(h, upload(h->d_heterms, H.eterms));
    HIP_TRY(h, upload(h->d_htasks, H.tasks));
    HIP_TRY(h, upload(h->d_hptasks, H.ptasks));
    HIP_TRY(h, upload(h->d_hbtasks, H.btasks));
    // Gauss-Legendre schemes with 2 / 3 stages of registry OCPs: the lane-per-step kernel takes the regular steps (CTD_HESS_STEP=0:
    // the tile kernel everywhere)
    std::vector<int32_t> ssrc, schunk;
    int snout = -1;
    const int64_t sb = std::max<int64_t>(h->hp.step_begin, H.reg_first), se = std::min<int64_t>(h->hp.step_end, H.reg_last);
    // CTD_HESS_STEP: 0 never, 2 whenever the OCP has assembly functions, 1 (default) from the grid size on where it wins: a wave
    // of the step kernel needs ~17 us for its 64 steps whatever the grid, the tile kernel's time grows with it (MI355X, Goddard:
    // 3 stages 18.5 vs 19.9 us at 32 000 steps, 28.7 vs 37.7 at 80 000; 2 stages 10.4 vs 10.9 us at 10 000, 14.0 vs 17.8 at 50 000)
    const int step_mode = env_int("CTD_HESS_STEP", 1);
    const int64_t step_min = mo.L.s == 3 ? 28000 : 9000;
    if (!h->rt && mo.L.sc == SC_IRK && (mo.L.s == 2 || mo.L.s == 3) && se > sb && step_mode != 0 && (step_mode == 2 || se - sb >= step_min)) {
        const short* prs = nullptr;
        for_problem(mo.problem, [&](auto tag) { prs = hess_step_pairs<typename decltype(tag)::type>(mo.L.s, mo.L.stagewise != 0, &snout); });
        h->hess_step = prs && snout >= 0 && build_hess_step_tables(mo, prs, snout, kSymStepChunk, ssrc, schunk);
    }
    const int step_wgs = h->hess_step ? (int)((h->hp.step_end - h->hp.step_begin + kStepBlock - 1) / kStepBlock) : 0;
    const int edge_step = 32;      // (upper bound of the edge workgroups of the step launch)
    h->hpart_member = (int64_t)(std::max(h->hp.ntiles, step_wgs) + std::max(h->hp.n_edge_blocks, edge_step)) * (H.nvv > 0 ? H.nvv : 1);
    HIP_TRY(h, h->d_hpartials.ensure(h->hpart_member));
    HParams& hp = h->hp;
    hp.tau = h->d_tau.p;
    hp.tptr = h->d_htptr.p; hp.terms = h->d_hterms.p; hp.pair_c = h->d_hpair_c.p;
    hp.cpos = h->d_hcpos.p; hp.zpos = h->d_hzpos.p;
    hp.vptr = h->d_hvptr.p; hp.vterms = h->d_hvterms.p;
    hp.edge_idx = h->d_hedge_idx.p; hp.eptr = h->d_heptr.p; hp.evptr = h->d_hevptr.p; hp.eterms = h->d_heterms.p;
    hp.tasks = h->d_htasks.p; hp.ptasks = h->d_hptasks.p; hp.btasks = h->d_hbtasks.p;
    hp.partials = h->d_hpartials.p;
    // V x V partials: added in a fixed order by a second, one-workgroup kernel (a last-workgroup finish inside the main
    // kernel measured 2-7x slower on MI355X, profiles/r01_hessian_kernel.md: device-scope release per workgroup)
    hp.debug_stop = env_int("CTD_HESS_STOP", 0);
    // write-through value stores for small Hessians (as for the constraint / Jacobian kernel, plan_cons_jac)
    hp.wt_store = 8.0 * (double)(h->hp.step_end - h->hp.step_begin) * (double)H.Lseg / 1.0e6 <= kHessWtMB ? 1 : 0;
    if (h->hess_step) {
        HIP_TRY(h, upload(h->d_hssrc, ssrc));
        HIP_TRY(h, upload(h->d_hschunk, schunk));
        SParams& sp = h->sp;
        sp = SParams{};
        sp.L = mo.L;
        sp.tau = h->d_tau.p;
        sp.step_begin = h->hp.step_begin; sp.step_end = h->hp.step_end;
        sp.reg_lo = sb; sp.reg_hi = se;
        sp.seg_base = H.seg_base; sp.reg_first = H.reg_first;
        sp.Lseg = H.Lseg; sp.nout = snout; sp.nchunk = (int)schunk.size() - 1; sp.nvv = H.nvv;
        sp.src = h->d_hssrc.p; sp.chunk_pos = h->d_hschunk.p;
        {   // constant parts of the chain-rule coefficients (HC_*, ctd_hess.hpp) and of their pairs
            const Layout& L = mo.L;
            double kc[kHC];
            for (int ci = 0; ci < kHC; ++ci) {
                if (ci == HC_ONE) kc[ci] = 1.0;
                else if (ci == HC_HALF) kc[ci] = 0.5;
                else if (ci < HC_A) kc[ci] = L.a[ci - HC_HA];
                else if (ci < HC_B) kc[ci] = L.a[ci - HC_A];
                else if (ci < HC_NBH) kc[ci] = L.b[ci - HC_B];
                else kc[ci] = -L.b[(ci - HC_NBH) % 3];
            }
            std::vector<double> ck((size_t)kHC * kHC);
            for (int c1 = 0; c1 < kHC; ++c1)
                for (int c2 = 0; c2 < kHC; ++c2) ck[(size_t)c1 * kHC + c2] = kc[c1] * kc[c2];
            HIP_TRY(h, upload(h->d_hsck, ck));
            sp.ck = h->d_hsck.p;
        }
        sp.partials = h->d_hpartials.p;
        // the tile kernel's edge path rides in the same launch on kStepBlock lanes: one edge workgroup per 64 edge entries
        h->hp_step = hp;
        const int ntot = (hp.edge_end - hp.edge_begin) + (hp.edge2_end - hp.edge2_begin);
        h->hp_step.n_edge_blocks = std::max(1, std::min(edge_step, (ntot + kStepBlock - 1) / kStepBlock));
        h->hp_step.ntiles = step_wgs;                 // (partials the finish kernel adds)
        sp.part_base = h->hp_step.n_edge_blocks;
        sp.wt_store = hp.wt_store;
        h->hess_step_lds = std::max(hess_step_lds_bytes(snout, mo.L.nv, H.Lseg), (size_t)hess_edge_lds_doubles(h->hp_step) * sizeof(double));
    }
    h->hess_ready = true;
    return CTD_OK;
}

static int32_t enqueue_hess(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev,
                            hipEvent_t te0 = nullptr, hipEvent_t te1 = nullptr, const Batch* bt = nullptr) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x_dev || !y_dev || !vals_dev) return fail(h, CTD_EINVAL, "null argument");
    int32_t st = ensure_hess(h);
    if (st) return st;
    const int nb = bt ? bt->n : 1;
    if (bt) {      // one set of V x V partial sums per member
        st = h->d_hpartials.grow(h, (int64_t)nb * h->hpart_member, "ctd_hess_coord_batch_dev_async");
        if (st) return st;
        h->hp.partials = h->hp_step.partials = h->sp.partials = h->d_hpartials.p;
    }
    HParams hp = h->hp;
    if (bt) { hp.ldx = bt->ldx; hp.ldy = bt->ldy; hp.ldh = bt->ldh; hp.part_stride = h->hpart_member; }
    hp.obj_weight = obj_weight;
    hp.vals = vals_dev;
    hp.halo = h->plan.kp.halo;
    hp.near = h->plan.kp.near;
    if (hp.halo) { hp.own_lo = h->halo_host.vbegin[h->halo_host.self]; hp.own_hi = h->halo_host.vbegin[h->halo_host.self + 1]; }
    hipError_t e = hipErrorInvalidValue;
    if (h->rt) {
        void* args[] = {&hp, &x_dev, &y_dev};
        e = jit_launch(h->jit[JIT_HESS][0].f[0], hp.ntiles + hp.n_edge_blocks, kHessBlock, h->hess_lds_bytes, h->stream, args, te0, te1, nb);
        if (e == hipSuccess && hp.nvv > 0) e = jit_launch(h->jit[JIT_HESS][0].f[1], 1, kHessBlock, 0, h->stream, args, nullptr, nullptr, nb);
    }
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        if (h->hess_step && !hp.stamps && !hp.debug_stop) {
            HParams he = h->hp_step;
            he.obj_weight = obj_weight;
            he.vals = vals_dev;
            he.halo = hp.halo; he.near = hp.near; he.own_lo = hp.own_lo; he.own_hi = hp.own_hi;       // (its edge blocks; a step lane reads its own step only)
            he.ldx = hp.ldx; he.ldy = hp.ldy; he.ldh = hp.ldh; he.part_stride = hp.part_stride;
            SParams sp = h->sp;
            sp.obj_weight = obj_weight;
            sp.vals = vals_dev;
            sp.ldh = hp.ldh; sp.part_stride = hp.part_stride;
            e = launch_hess_step<P>(he, sp, x_dev, y_dev, h->hess_step_lds, h->stream, te0, te1, nb);
        } else {
            e = launch_hess<P>(hp, x_dev, y_dev, h->hess_lds_bytes, h->stream, te0, te1, nb);
        }
    });
    return launched(h, nullptr, e);
}

int32_t ctd_hess_coord_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev) {
    return enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev);
}

int32_t ctd_hess_coord_dev(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev) {
    int32_t st = enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev);
    if (st) return st;
    return ctd_sync(h);
}

int32_t ctd_hess_coord(ctd_handle* h, const double* x, const double* y, double obj_weight, double* vals) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x || !y || !vals) return fail(h, CTD_EINVAL, "null argument");
    const Model& mo = h->model;
    return host_call(h, {{x, h->d_x, mo.L.nvar}, {y, h->d_y, mo.L.ncon}},
                     [&] { return enqueue_hess(h, h->d_x.p, h->d_y.p, obj_weight, h->d_hvals.p); }, {{vals, h->d_hvals, mo.H.nnzh}});
}

// ---- batched callbacks: K iterates of one transcription per launch ---------------------------------------------------
// The same kernels on a grid whose second dimension is the member (include/ctdirect_hip.h).  Checks in this order: handle,
// device (CTD_ENODEVICE) -- the prologue, OnDevice(h, fn) --, batch size, whole-grid handle, then pointers and leading dimensions
// (CTD_EINVAL).
constexpr int32_t kMaxBatch = 65535;       // the grid's y limit

static int32_t batch_check(const OnDevice& on, ctd_handle* h, const char* fn, int32_t batch, const double* x_dev, int64_t ldx) {
    if (on.st) return on.st;
    if (batch < 1 || batch > kMaxBatch) return fail(h, CTD_EINVAL, std::string(fn) + ": batch must be in [1, 65535], got " + std::to_string(batch));
    if (h->step_begin != 0 || h->step_end != h->model.L.N || h->plan.kp.halo)
        return fail(h, CTD_EINVAL, std::string(fn) + ": batched calls need a handle of the whole grid; a shard handle (step_begin / step_end, "
                                   "ctd_set_x_shards) evaluates one iterate per call");
    if (!x_dev) return fail(h, CTD_EINVAL, std::string(fn) + ": x is null");
    if (ldx < h->model.L.nvar) return fail(h, CTD_EINVAL, std::string(fn) + ": ldx = " + std::to_string(ldx) + " < nvar = " + std::to_string(h->model.L.nvar));
    return CTD_OK;
}
static int32_t ld_check(ctd_handle* h, const char* fn, const char* name, int64_t ld, int64_t n) {
    if (ld < n) return fail(h, CTD_EINVAL, std::string(fn) + ": " + name + " = " + std::to_string(ld) + " is below the vector length " + std::to_string(n));
    return CTD_OK;
}

int32_t ctd_cons_jac_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* c_dev, int64_t ldc,
                                     double* vals_dev, int64_t ldv) {
    static const char* fn = "ctd_cons_jac_batch_dev_async";
    const OnDevice on(h, fn);
    int32_t st = batch_check(on, h, fn, batch, x_dev, ldx);
    if (!st && c_dev) st = ld_check(h, fn, "ldc", ldc, h->model.L.ncon);
    if (!st && vals_dev) st = ld_check(h, fn, "ldv", ldv, h->model.nnzj);
    if (st) return st;
    const Batch bt{batch, ldx, 0, c_dev ? ldc : 0, vals_dev ? ldv : 0, 0, 0};
    return enqueue_cons_jac(h, x_dev, c_dev, vals_dev, nullptr, nullptr, &bt);
}

int32_t ctd_obj_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* f_dev) {
    static const char* fn = "ctd_obj_batch_dev_async";
    const OnDevice on(h, fn);
    const int32_t st = batch_check(on, h, fn, batch, x_dev, ldx);
    if (st) return st;
    if (!f_dev) return fail(h, CTD_EINVAL, std::string(fn) + ": f is null");
    const Batch bt{batch, ldx, 0, 0, 0, 0, 0};
    return enqueue_obj(h, x_dev, f_dev, &bt);
}

int32_t ctd_grad_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* g_dev, int64_t ldg) {
    static const char* fn = "ctd_grad_batch_dev_async";
    const OnDevice on(h, fn);
    int32_t st = batch_check(on, h, fn, batch, x_dev, ldx);
    if (st) return st;
    if (!g_dev) return fail(h, CTD_EINVAL, std::string(fn) + ": g is null");
    if ((st = ld_check(h, fn, "ldg", ldg, h->model.L.nvar))) return st;
    const Batch bt{batch, ldx, 0, 0, 0, ldg, 0};
    return enqueue_grad(h, x_dev, g_dev, nullptr, false, &bt);
}

int32_t ctd_hess_coord_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, const double* y_dev, int64_t ldy,
                                       double obj_weight, double* vals_dev, int64_t ldh) {
    static const char* fn = "ctd_hess_coord_batch_dev_async";
    const OnDevice on(h, fn);
    int32_t st = batch_check(on, h, fn, batch, x_dev, ldx);
    if (st) return st;
    if (!y_dev || !vals_dev) return fail(h, CTD_EINVAL, std::string(fn) + ": y or vals is null");
    if ((st = ld_check(h, fn, "ldy", ldy, h->model.L.ncon))) return st;
    if ((st = ld_check(h, fn, "ldh", ldh, h->model.H.nnzh))) return st;
    const Batch bt{batch, ldx, ldy, 0, 0, 0, ldh};
    return enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev, nullptr, nullptr, &bt);
}

// ---- one solver iteration in one call --------------------------------------------------------------------------------
// obj(x), grad(x), cons(x) + jac_coord(x) and hess_coord(x, y; obj_weight) only depend on (x, y).  Registry problems: the
// horizontally fused kernel of ctd_iter_kernels.hpp (+ its finish kernel): two launches per iteration.  Run-time OCPs (their
// kernels are compiled by hiprtc per callback): the same callbacks one after the other on the handle's stream.
int32_t ctd_eval_all_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* f_dev, double* g_dev,
                               double* c_dev, double* vals_dev, double* hvals_dev) {
    const OnDevice on(h);
    if (on.st) return on.st;
    if (!x_dev) return fail(h, CTD_EINVAL, "x is null");
    if (hvals_dev && !y_dev) return fail(h, CTD_EINVAL, "y is null");
    int32_t st = CTD_OK;
    if (hvals_dev) { st = ensure_hess(h); if (st) return st; }      // first use uploads the tables (not capturable)
    if (h->rt || h->model.L.cs > 1) {
        if (f_dev) st = enqueue_obj(h, x_dev, f_dev);
        if (!st && g_dev) st = enqueue_grad(h, x_dev, g_dev);
        if (!st && (c_dev || vals_dev)) st = enqueue_cons_jac(h, x_dev, c_dev, vals_dev);
        if (!st && hvals_dev) st = enqueue_hess(h, x_dev, y_dev, obj_weight, hvals_dev);
        return st;
    }
    IterParams ip;
    std::memset(&ip, 0, sizeof(ip));
    size_t lds = 4 * kMaxNV * sizeof(double) + 64;
    ip.kp = h->plan.kp;       // (Layout is read from kp / hp / gp / op by the respective bodies)
    ip.hp = h->hp;
    ip.hp.halo = h->plan.kp.halo;
    ip.hp.near = h->plan.kp.near;
    if (ip.hp.halo) { ip.hp.own_lo = h->halo_host.vbegin[h->halo_host.self]; ip.hp.own_hi = h->halo_host.vbegin[h->halo_host.self + 1]; }
    // The fused grid always carries the TILE body of the Hessian, also on handles whose stand-alone hess_coord runs the
    // lane-per-step kernel (Gauss-Legendre 2 from 9 000 steps, 3 from 28 000: ensure_hess).  Measured with the fused first-order
    // grid, then the step kernel and its finish as two more launches: Goddard GL2 N = 10 000 22.9 us against 14-16, GL3 N = 80 000
    // 64.0 against 62.6 -- the two extra launches cost what the faster kernel gains
    if (hvals_dev) {
        ip.hp.obj_weight = obj_weight;
        ip.hp.vals = hvals_dev;
        ip.nb_h = ip.hp.ntiles + ip.hp.n_edge_blocks;
        lds = std::max(lds, h->hess_lds_bytes);
    }
    if (c_dev || vals_dev) {
        ip.kp.c = c_dev;
        ip.kp.vals = vals_dev;
        ip.nb_cj = h->plan.grid;
        lds = std::max(lds, h->plan.lds_bytes);
    }
    if (g_dev) {
        st = enqueue_grad(h, x_dev, g_dev, &ip.gp);          // fills the parameters only (and sizes the partials buffer)
        if (st) return st;
        ip.zero_g = h->model.info.lagrange ? 0 : 1;
        const Layout& L = h->model.L;
        ip.nb_g = ip.zero_g ? (int)std::min<int64_t>(64, (L.nvar + 4095) / 4096) : ip.gp.nblocks;
        if (ip.nb_g < 1) ip.nb_g = 1;
    }
    if (f_dev) ip.nb_o = fill_obj_params(h, f_dev, ip.op);
    hipError_t e = hipErrorInvalidValue;
    for_problem(h->model.problem, [&](auto tag) {
        using P = typename decltype(tag)::type;
        e = launch_iter<P>(ip, x_dev, y_dev, lds, h->stream);
    });
    return launched(h, nullptr, e);
}

// out[0..9]: grid (workgroups), block, LDS bytes, steps per tile, CSC period of the lower triangle, edge entries, eval lanes
// per stage point / path point / boundary point, terms of the periodic segment
int32_t ctd_hess_launch_info(ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    int32_t st = ensure_hess(h);
    if (st) return st;
    o[0] = h->hp.ntiles + h->hp.n_edge_blocks; o[1] = kHessBlock; o[2] = (int64_t)h->hess_lds_bytes; o[3] = h->hess_tile; o[4] = h->hp.Lseg; o[5] = h->hp.n_edge;
    o[6] = h->hp.ntask; o[7] = h->hp.nptask; o[8] = h->hp.nbtask; o[9] = h->hp.nterms;
    return CTD_OK;
}

int32_t ctd_hess_kernel_info(ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    if (h->device < 0) return fail(h, CTD_ENODEVICE, "host-only handle");
    int32_t st = ensure_hess(h);
    if (st) return st;
    o[0] = h->hess_step ? 1 : 0;
    o[1] = h->hess_step ? h->hp_step.n_edge_blocks + h->hp_step.ntiles : h->hp.ntiles + h->hp.n_edge_blocks;
    return CTD_OK;
}

int32_t ctd_hess_debug_stamps(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev,
                              uint64_t* out, int64_t cap) {
    if (!h || !out) return CTD_EINVAL;
    int32_t st = enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev);     // warm, no stamps
    if (st) return st;
    const int64_t words = (int64_t)(h->hp.ntiles + h->hp.n_edge_blocks) * 10;
    if (cap < words) return fail(h, CTD_EINVAL, "stamp buffer too small");
    unsigned long long* d_st = nullptr;
    HIP_TRY(h, hipMalloc((void**)&d_st, sizeof(unsigned long long) * words));
    HIP_TRY(h, hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * words, h->stream));
    h->hp.stamps = d_st;
    st = enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev);
    h->hp.stamps = nullptr;
    if (st == CTD_OK) {
        hipError_t e = hipMemcpyAsync(out, d_st, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) st = fail(h, CTD_EHIP, hipGetErrorString(e));
    }
    (void)hipFree(d_st);
    return st;
}

// out[0..3 + nvv): vals_main_begin, vals_main_end (contiguous CSC range of the shard's step columns), nvv, then the nvv
// positions of the V x V entries -- after ctd_hess_coord_dev on a shard they hold the shard's PARTIAL sums and must be
// added over the shards (one all-reduce of nvv doubles)
int32_t ctd_hess_shard_info(const ctd_handle* h, int64_t* o) {
    if (!h || !o) return CTD_EINVAL;
    const Model& mo = h->model;
    const HessModel& H = mo.H;
    const int64_t a = h->step_begin > H.reg_first ? h->step_begin : H.reg_first;
    const int64_t b = h->step_end < H.reg_last ? h->step_end : H.reg_last;
    o[0] = H.seg_base + (a - H.reg_first) * (int64_t)H.Lseg;
    o[1] = b > a ? H.seg_base + (b - H.reg_first) * (int64_t)H.Lseg : o[0];
    int nvv = 0;                                     // (optimized pattern: entries no evaluation point feeds are not in the pattern)
    for (int e = 0; e < H.nvv; ++e)
        if (H.vv_idx[e] >= 0) o[3 + nvv++] = H.vv_idx[e];
    o[2] = nvv;
    return CTD_OK;
}

int32_t ctd_time_hess_dev(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev, int32_t iters,
                          double* mean_ms) {
    if (!h || !mean_ms || iters < 1) return CTD_EINVAL;
    return time_dispatches(h, iters, mean_ms,
                           [&](hipEvent_t a, hipEvent_t b) { return enqueue_hess(h, x_dev, y_dev, obj_weight, vals_dev, a, b); });
}

// ---- one transcription on several GPUs of one process --------------------------------------------------------------------
}  // extern "C"

struct ctd_sharded {
    std::vector<ctd_handle*> h;
    std::vector<int> dev;
    std::vector<hipEvent_t> x_ready;     // recorded on shard k's stream when this call's reads of x_dev[k] by OTHER shards may start
    std::vector<hipEvent_t> done;        // recorded on shard k's stream after its kernel (its rows of c are final)
    std::vector<hipEvent_t> pulled;      // recorded on shard k's stream after it has pulled the others' row blocks (stitching)
    bool pulls_pending = false;          // the last call stitched: the next kernels must not overwrite rows still being pulled
    std::vector<char> peer_ok;           // [a * G + b]: device of shard a can load from device of shard b (same device, or peer access enabled)
    int64_t N = 0;
    std::string err;
    ~ctd_sharded() {
        for (size_t k = 0; k < h.size(); ++k) {
            if (h[k]) { DeviceGuard dg(dev[k]); if (x_ready[k]) (void)hipEventDestroy(x_ready[k]); if (done[k]) (void)hipEventDestroy(done[k]); if (pulled[k]) (void)hipEventDestroy(pulled[k]); }
            if (h[k]) (void)ctd_destroy(h[k]);
        }
    }
};

static int32_t sfail(ctd_sharded* s, int32_t code, const std::string& msg) {
    if (s) s->err = msg; else g_create_err = msg;
    return code;
}
// a copy between two shards' buffers on shard k's stream: peer-to-peer over xGMI (or a plain device copy when both shards
// sit on one device)
static hipError_t shard_copy(ctd_sharded* s, int k, double* dst, int from, const double* src, int64_t count) {
    if (count <= 0) return hipSuccess;
    if (s->dev[k] == s->dev[from]) return hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToDevice, s->h[k]->stream);
    return hipMemcpyPeerAsync(dst, s->dev[k], src, s->dev[from], sizeof(double) * count, s->h[k]->stream);
}
#define SH_TRY(s, expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return sfail(s, CTD_ERCCL, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

extern "C" {

int32_t ctd_create_sharded(const ctd_desc* desc, const int32_t* devices, int32_t n_devices, ctd_sharded** out) {
    if (!desc || !devices || !out || n_devices < 1) return sfail(nullptr, CTD_EINVAL, "ctd_create_sharded: bad argument");
    *out = nullptr;
    if (desc->step_begin != 0 || desc->step_end != 0) return sfail(nullptr, CTD_EINVAL, "ctd_create_sharded: the descriptor must name the whole grid");
    const int64_t N = desc->time_grid ? desc->time_grid_len - 1 : desc->grid_size;
    if (N < n_devices) return sfail(nullptr, CTD_EINVAL, "ctd_create_sharded: fewer time steps than devices");
    std::unique_ptr<ctd_sharded> s(new (std::nothrow) ctd_sharded());
    if (!s) return sfail(nullptr, CTD_ENOMEM, "ctd_create_sharded: out of memory");
    s->N = N;
    s->h.assign(n_devices, nullptr); s->dev.assign(devices, devices + n_devices);
    s->x_ready.assign(n_devices, nullptr); s->done.assign(n_devices, nullptr); s->pulled.assign(n_devices, nullptr);
    const int64_t base = N / n_devices, rem = N % n_devices;
    for (int k = 0; k < n_devices; ++k) {
        ctd_desc dk = *desc;
        dk.device = devices[k];
        dk.step_begin = k * base + (k < rem ? k : rem);
        dk.step_end = dk.step_begin + base + (k < rem ? 1 : 0);
        dk.stream = nullptr;
        dk.stream_mode = CTD_STREAM_OWN;
        const int32_t st = ctd_create(&dk, &s->h[k]);
        if (st) return st;                                   // message in ctd_last_error(NULL)
        DeviceGuard dg(devices[k]);
        if (dg.err != hipSuccess || hipEventCreateWithFlags(&s->x_ready[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->done[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->pulled[k], hipEventDisableTiming) != hipSuccess)
            return sfail(nullptr, CTD_EHIP, "ctd_create_sharded: event creation failed");
    }
    // peer access between every pair of distinct devices (xGMI); hipMemcpyPeerAsync works without it, through the host.  Which
    // pairs can load from each other is RECORDED: CTD_X_SHARDED_IN_PLACE dereferences the other shards' buffers inside the kernels
    // and falls back to the copying protocol when a pair it needs is not peer-capable (a fault inside a kernel otherwise)
    s->peer_ok.assign((size_t)n_devices * n_devices, 0);
    for (int a = 0; a < n_devices; ++a)
        for (int b = 0; b < n_devices; ++b) {
            if (devices[a] == devices[b]) { s->peer_ok[(size_t)a * n_devices + b] = (a == b || !env_int("CTD_TEST_NO_PEER", 0)) ? 1 : 0; continue; }      // (test knob: pretend distinct shards cannot reach each other)
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can) {
                DeviceGuard dg(devices[a]);
                const hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return sfail(nullptr, CTD_ERCCL, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
                (void)hipGetLastError();
                s->peer_ok[(size_t)a * n_devices + b] = 1;
            }
        }
    *out = s.release();
    return CTD_OK;
}

int32_t ctd_sharded_destroy(ctd_sharded* s) {
    if (!s) return CTD_EINVAL;
    delete s;
    return CTD_OK;
}

const char* ctd_sharded_last_error(const ctd_sharded* s) { return s ? s->err.c_str() : g_create_err.c_str(); }

int32_t ctd_sharded_handle(ctd_sharded* s, int32_t k, ctd_handle** h) {
    if (!s || !h || k < 0 || k >= (int32_t)s->h.size()) return CTD_EINVAL;
    *h = s->h[k];
    return CTD_OK;
}

int32_t ctd_sharded_shard_info(const ctd_sharded* s, int32_t k, int64_t* o) {
    if (!s || !o || k < 0 || k >= (int32_t)s->h.size()) return CTD_EINVAL;
    o[0] = (int64_t)s->h.size();
    o[1] = s->dev[k];
    return ctd_shard_info(s->h[k], o + 2);
}

int32_t ctd_sharded_sync(ctd_sharded* s) {
    if (!s) return CTD_EINVAL;
    for (size_t k = 0; k < s->h.size(); ++k) {
        const int32_t st = ctd_sync(s->h[k]);
        if (st) return sfail(s, st, ctd_last_error(s->h[k]));
    }
    return CTD_OK;
}

int32_t ctd_dev_alloc(int32_t device, size_t bytes, void** ptr) {
    if (!ptr) return CTD_EINVAL;
    *ptr = nullptr;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e == hipSuccess) e = hipMalloc(ptr, bytes ? bytes : 8);
    if (e != hipSuccess) { g_create_err = std::string("ctd_dev_alloc: ") + hipGetErrorString(e); return CTD_EHIP; }
    return CTD_OK;
}
int32_t ctd_dev_free(int32_t device, void* ptr) {
    if (!ptr) return CTD_OK;
    DeviceGuard dg(device);
    return (dg.err == hipSuccess && hipFree(ptr) == hipSuccess) ? CTD_OK : CTD_EHIP;
}
int32_t ctd_dev_copy(int32_t device, void* dst, const void* src, size_t bytes, int32_t kind) {
    if (!dst || !src || (kind != 0 && kind != 1)) return CTD_EINVAL;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, kind == 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    if (e != hipSuccess) { g_create_err = std::string("ctd_dev_copy: ") + hipGetErrorString(e); return CTD_EHIP; }
    return CTD_OK;
}

int32_t ctd_cons_jac_sharded_dev_async(ctd_sharded* s, double* const* x_dev, double* const* c_dev, double* const* vals_dev,
                                       int32_t x_mode, int32_t stitch) {
    if (!s || !x_dev) return CTD_EINVAL;
    const int G = (int)s->h.size();
    for (int k = 0; k < G; ++k)
        if (!x_dev[k] || (stitch && (!c_dev || !c_dev[k]))) return sfail(s, CTD_EINVAL, "ctd_cons_jac_sharded_dev_async: null buffer");
    if (x_mode != CTD_X_IN_PLACE && x_mode != CTD_X_SHARDED && x_mode != CTD_X_FROM_DEVICE0 && x_mode != CTD_X_SHARDED_COPY &&
        x_mode != CTD_X_SHARDED_IN_PLACE)
        return sfail(s, CTD_EINVAL, "ctd_cons_jac_sharded_dev_async: unknown x_mode");
    const Layout& L = s->h[0]->model.L;
    const int64_t N = L.N;
    // shards whose buffers shard k reads besides its own: its neighbours, the first (X_1) and the last (X_{N+1})
    auto reads = [&](int k, int j) { return j != k && (j == k - 1 || j == k + 1 || j == 0 || j == G - 1); };
    // (0) CTD_X_SHARDED_IN_PLACE: the kernels read the neighbours' entries in place through the peer mappings -- nothing is copied;
    // the table of buffers is rewritten only when the caller passes other pointers than last time.  A pair of devices that cannot
    // load from each other (no peer access: hipDeviceCanAccessPeer said no at creation) would fault inside the kernel: the call then
    // takes the copying protocol of CTD_X_SHARDED instead (same results; ctd_sharded_last_error says so)
    if (x_mode == CTD_X_SHARDED_IN_PLACE && G > 1) {
        if (G > kMaxShards) return sfail(s, CTD_EINVAL, "ctd_cons_jac_sharded_dev_async: CTD_X_SHARDED_IN_PLACE supports at most 16 shards");
        for (int k = 0; k < G && x_mode == CTD_X_SHARDED_IN_PLACE; ++k)
            for (int j = 0; j < G; ++j)
                if (reads(k, j) && !s->peer_ok[(size_t)k * G + j]) {
                    s->err = "CTD_X_SHARDED_IN_PLACE: device " + std::to_string(s->dev[k]) + " has no peer access to device " + std::to_string(s->dev[j]) +
                             "; the halo entries are copied instead (CTD_X_SHARDED)";
                    x_mode = CTD_X_SHARDED;
                    break;
                }
    }
    {
        int64_t sb[kMaxShards + 1];
        const bool peer = x_mode == CTD_X_SHARDED_IN_PLACE && G > 1;
        if (peer) {
            for (int k = 0; k < G; ++k) sb[k] = s->h[k]->step_begin;
            sb[G] = N;
        }
        for (int k = 0; k < G; ++k) {
            const int32_t st = peer ? ctd_set_x_shards(s->h[k], G, sb, x_dev, k) : (s->h[k]->plan.kp.halo ? ctd_set_x_shards(s->h[k], 0, nullptr, nullptr, 0) : CTD_OK);
            if (st) return sfail(s, st, ctd_last_error(s->h[k]));
        }
        // ... and the cheap half of the copying protocol stays: every shard marks the point of ITS stream behind which its buffer holds
        // this iterate (work the caller queued there -- e.g. its update of x on that device's stream -- included), and a shard's kernel
        // waits for the marks of the shards it reads.  No copy; two event operations per neighbour
        if (peer) {
            for (int k = 0; k < G; ++k) {
                DeviceGuard dg(s->dev[k]);
                SH_TRY(s, hipEventRecord(s->x_ready[k], s->h[k]->stream));
            }
            for (int k = 0; k < G; ++k) {
                DeviceGuard dg(s->dev[k]);
                for (int j = 0; j < G; ++j)
                    if (reads(k, j)) SH_TRY(s, hipStreamWaitEvent(s->h[k]->stream, s->x_ready[j], 0));
            }
        }
    }
    // (1) iterate distribution.  Every shard first marks the point of its stream behind which its x buffer may be read by
    // the others (its own previous kernel has finished with it; the caller's writes are complete by contract).
    if ((x_mode == CTD_X_SHARDED || x_mode == CTD_X_SHARDED_COPY || x_mode == CTD_X_FROM_DEVICE0) && G > 1) {
        for (int k = 0; k < G; ++k) {
            DeviceGuard dg(s->dev[k]);
            SH_TRY(s, hipEventRecord(s->x_ready[k], s->h[k]->stream));
        }
        const int64_t w = L.n + (L.final_control ? L.m : 0);
        // (whatever the Jacobian's value order needs: the gradient and the Hessian of a one-point scheme read the previous block too)
        const int64_t lo = (L.sc == SC_IRK) ? 0 : L.blk;
        for (int k = 0; k < G; ++k) {
            DeviceGuard dg(s->dev[k]);
            ctd_handle* hk = s->h[k];
            if (x_mode == CTD_X_FROM_DEVICE0) {
                if (k == 0) continue;
                SH_TRY(s, hipStreamWaitEvent(hk->stream, s->x_ready[0], 0));
                SH_TRY(s, shard_copy(s, k, x_dev[k], 0, x_dev[0], L.nvar));
                continue;
            }
            const int64_t b = hk->step_begin, e = hk->step_end;
            if (k + 1 < G) {      // next shard's first node; the final state (boundary rows, Mayer cost)
                SH_TRY(s, hipStreamWaitEvent(hk->stream, s->x_ready[k + 1], 0));
                SH_TRY(s, shard_copy(s, k, x_dev[k] + e * L.blk, k + 1, x_dev[k + 1] + e * L.blk, w));
                if (k + 1 != G - 1) SH_TRY(s, hipStreamWaitEvent(hk->stream, s->x_ready[G - 1], 0));
                SH_TRY(s, shard_copy(s, k, x_dev[k] + N * L.blk, G - 1, x_dev[G - 1] + N * L.blk, L.n));
            }
            if (k > 0) {          // previous shard's last block (one-point schemes); the first state (boundary rows)
                SH_TRY(s, hipStreamWaitEvent(hk->stream, s->x_ready[k - 1], 0));
                if (lo) SH_TRY(s, shard_copy(s, k, x_dev[k] + (b - 1) * L.blk, k - 1, x_dev[k - 1] + (b - 1) * L.blk, lo));
                if (k - 1 != 0) SH_TRY(s, hipStreamWaitEvent(hk->stream, s->x_ready[0], 0));
                SH_TRY(s, shard_copy(s, k, x_dev[k], 0, x_dev[0], L.n));
            }
        }
    }
    // (2) the shards' kernels (after every other device has finished pulling this shard's rows of the previous stitched call)
    if (s->pulls_pending) {
        for (int k = 0; k < G; ++k) {
            DeviceGuard dg(s->dev[k]);
            for (int j = 0; j < G; ++j)
                if (j != k) SH_TRY(s, hipStreamWaitEvent(s->h[k]->stream, s->pulled[j], 0));
        }
        s->pulls_pending = false;
    }
    for (int k = 0; k < G; ++k) {
        const int32_t st = enqueue_cons_jac(s->h[k], x_dev[k], c_dev ? c_dev[k] : nullptr, vals_dev ? vals_dev[k] : nullptr);
        if (st) return sfail(s, st, ctd_last_error(s->h[k]));
    }
    // (3) stitching: every device pulls the other shards' row blocks of c once those shards' kernels are done
    if (stitch && G > 1) {
        for (int k = 0; k < G; ++k) {
            DeviceGuard dg(s->dev[k]);
            SH_TRY(s, hipEventRecord(s->done[k], s->h[k]->stream));
        }
        for (int k = 0; k < G; ++k) {
            DeviceGuard dg(s->dev[k]);
            for (int j = 0; j < G; ++j) {
                if (j == k) continue;
                SH_TRY(s, hipStreamWaitEvent(s->h[k]->stream, s->done[j], 0));
                // (the p + bc tail rows come from the last shard: the only one that holds everything they read when x is sharded)
                const int64_t r0 = s->h[j]->step_begin * L.cb, r1 = (j == G - 1) ? L.ncon : s->h[j]->step_end * L.cb;
                SH_TRY(s, shard_copy(s, k, c_dev[k] + r0, j, c_dev[j] + r0, r1 - r0));
            }
            SH_TRY(s, hipEventRecord(s->pulled[k], s->h[k]->stream));
        }
        s->pulls_pending = true;
    }
    return CTD_OK;
}

}  // extern "C"
