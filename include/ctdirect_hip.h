/*
 * ctdirect_hip.h -- C ABI of the MI355X-native collocation engine (libctdirect_hip.so).
 *
 * This is the drop-in boundary for CTDirect.jl's NLP-callback hot path.  In the reference the boundary is the call
 *     ADNLPModels.ADNLPModel!(f, x0, lvar, uvar, c!, lcon, ucon; minimize, backends...)   src/collocation.jl:137-149
 * inside build_adnlp_model (src/collocation.jl:90-153), after which ADNLPModels serves the NLPModels API
 * (obj, cons!, jac_structure!, jac_coord!, ...) to Ipopt/MadNLP by calling the two Julia closures
 *     f  = x -> CTDirect.__objective(x, docp)          src/collocation.jl:97,  src/DOCP_functions.jl:23-54
 *     c! = (c, x) -> CTDirect.__constraints!(c, x, docp)  src/collocation.jl:98,  src/DOCP_functions.jl:80-115
 * and differentiating c! with coloured ForwardDiff passes over DOCP_Jacobian_pattern(docp) (src/collocation.jl:116-120).
 * A Julia shim subtypes NLPModels.AbstractNLPModel and forwards each NLPModels method to ONE entry
 * point below through `ccall`; every entry point states the reference interface it replaces.
 *
 * Conventions
 *   - all functions return an int32 status (CTD_OK == 0); no C++ exception crosses this boundary;
 *   - the caller owns every buffer passed in; the engine owns its device buffers and staging inside the handle;
 *   - host-pointer calls copy H2D / D2H and return when the result is in the caller's buffer;
 *     `_dev` calls take device pointers (hipMalloc'ed, on the handle's device) and are synchronous;
 *     `_dev_async` calls only enqueue on the handle's stream (ctd_sync waits);
 *   - external layouts are the reference's: variables step-major [X_i, U_i.., K_i..]..., X_{N+1}, [U_{N+1}], V
 *     (src/ode/trapeze.jl:1-4, midpoint.jl:1-7, irk.jl:1-9, irk_stagewise.jl:6-11); constraints
 *     [C_i^x, C_i^{k,1..s}, G_i]..., G_{N+1}, B (src/ode/irk_stagewise.jl:13-30, src/DOCP_functions.jl:92-111);
 *     Jacobian values in the CSC order of SparseArrays.sparse(Is, Js, ...) as DOCP_Jacobian_pattern returns it (default), or by rows
 *     (ctd_desc.value_order = CTD_ORDER_CSR);
 *   - all arithmetic is FP64; there is NO CPU fallback: compute entry points on a handle without a device fail
 *     with CTD_ENODEVICE.
 *   - a handle is not thread-safe; distinct handles are independent (one HIP stream each).
 */
#ifndef CTDIRECT_HIP_H
#define CTDIRECT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctd_handle ctd_handle;

/* status codes; the Julia shim rethrows CTD_EGRID as ArgumentError (src/DOCP_data.jl:186-189), CTD_ESCHEME as
 * error("Unknown discretization method") (src/DOCP_data.jl:342-349), CTD_EPATTERN as the error of the
 * DOCP_Jacobian_pattern stubs (src/ode/common.jl:252-272) */
enum {
    CTD_OK = 0,
    CTD_EINVAL = 1,     /* null pointer / bad argument */
    CTD_EGRID = 2,      /* time grid not strictly increasing */
    CTD_ESCHEME = 3,    /* unknown discretization scheme */
    CTD_EPATTERN = 4,   /* sparsity pattern not available / not step-periodic */
    CTD_EPROBLEM = 5,   /* problem id not in the compiled registry */
    CTD_ENODEVICE = 6,  /* compute call on a host-only handle, or no usable HIP device */
    CTD_EHIP = 7,       /* a HIP runtime call failed (message in ctd_last_error) */
    CTD_ENOMEM = 8,
    CTD_ERCCL = 9       /* an exchange between the devices of a multi-device handle failed (peer access / peer copy) */
};

/* scheme symbols of the reference, src/DOCP_data.jl:307-349 */
enum {
    CTD_SCHEME_TRAPEZE = 0,                          /* :trapeze                              */
    CTD_SCHEME_MIDPOINT = 1,                         /* :midpoint                             */
    CTD_SCHEME_GAUSS_LEGENDRE_1 = 2,                 /* Gauss_Legendre_1 (test only, irk.jl:20) */
    CTD_SCHEME_GAUSS_LEGENDRE_2_CONSTANT_CONTROL = 3,/* :gauss_legendre_2_constant_control    */
    CTD_SCHEME_GAUSS_LEGENDRE_3_CONSTANT_CONTROL = 4,/* :gauss_legendre_3_constant_control    */
    CTD_SCHEME_GAUSS_LEGENDRE_2 = 5,                 /* :gauss_legendre_2 (stagewise controls) */
    CTD_SCHEME_GAUSS_LEGENDRE_3 = 6,                 /* :gauss_legendre_3 (stagewise controls) */
    CTD_SCHEME_EULER = 7,                            /* :euler | :euler_explicit | :euler_forward (src/DOCP_data.jl:315-317, src/ode/euler.jl) */
    CTD_SCHEME_EULER_IMPLICIT = 8                    /* :euler_implicit | :euler_backward (:318-320)                                           */
};

/* compiled OCP registry (the reference takes arbitrary Julia closures from CTModels; a GPU engine behind a C ABI
 * cannot -- see DESIGN.md "the unavoidable gap") */
enum {
    CTD_PROBLEM_GODDARD = 0,                    /* test/problems/goddard.jl:18-49                  */
    CTD_PROBLEM_GODDARD_ALL = 1,                /* test/problems/goddard.jl:87-158                 */
    CTD_PROBLEM_DOUBLE_INTEGRATOR_PATH = 2,     /* double_integrator.jl:42-58 + build-defined path */
    CTD_PROBLEM_QUADROTOR = 3,                  /* test/problems/quadrotor.jl:7-105 (8 states)     */
    CTD_PROBLEM_QUADROTOR12 = 4,                /* build-defined 12-state rigid body               */
    CTD_PROBLEM_STAGEWISE_SCALAR = 5,           /* test/ci/test_discretization_stagewise.jl:1-14   */
    CTD_PROBLEM_ESTIMATE_INITIAL_CONDITION = 6, /* test/problems/autonomous_system.jl:6-43         */
    CTD_PROBLEM_ESTIMATE_ROTATION_RATE = 7,     /* test/problems/autonomous_system.jl:46-87        */
    CTD_PROBLEM_LEAST_SQUARES_CONSTRAINT = 8,   /* test/problems/autonomous_system.jl:90-138       */
    CTD_PROBLEM_DOUBLE_INTEGRATOR_FREET0TF = 9  /* test/problems/double_integrator.jl:79-99        */
};

enum {
    CTD_PATTERN_REFERENCE_MANUAL = 0, /* DOCP_Jacobian_pattern exactly as written (bug-compatible, SURVEY hazards H1/H2) */
    CTD_PATTERN_STRUCTURAL = 1,       /* = manual + the dynamics-row x V block trapeze.jl:203 omits */
    CTD_PATTERN_OPTIMIZED = 2         /* the sparsity ADNLPModels' default backend detects itself (src/collocation.jl:131-134:
                                         SparseConnectivityTracer over c! and the Lagrangian): operator-level dependence of every
                                         row, e.g. nnzj 4504 / nnzh 5259 instead of 6028 / 6519 for Goddard, midpoint, N = 250
                                         (test/ci/test_modeler_solver.jl:32,37).  Fewer entries = fewer bytes per evaluation */
};

/* replaces the arguments of CTDirect.DOCP(ocp, grid_size, control_steps, scheme, time_grid), src/DOCP_data.jl:293-365,
 * as selected by Collocation(; grid_size, scheme, time_grid), src/collocation.jl:16-48,57-73 */
typedef struct ctd_desc {
    int32_t problem;          /* CTD_PROBLEM_*                                                        */
    int32_t scheme;           /* CTD_SCHEME_*                                                         */
    int32_t pattern_mode;     /* CTD_PATTERN_*                                                        */
    int32_t device;           /* HIP device ordinal; -1 = host-only handle (sizes, bounds, x0, patterns) */
    int64_t grid_size;        /* N; used when time_grid == NULL (uniform grid, src/DOCP_data.jl:179-183) */
    const double* time_grid;  /* optional strictly increasing grid of time_grid_len = N+1 points (:184-199) */
    int64_t time_grid_len;
    int64_t step_begin;       /* shard of the time grid this handle evaluates: steps [step_begin, step_end),  */
    int64_t step_end;         /*   0-based; 0,0 = all N steps (single GPU)                                    */
    void* stream;             /* hipStream_t to launch on when stream_mode == CTD_STREAM_GIVEN                */
    int32_t stream_mode;      /* CTD_STREAM_OWN: the handle creates a private non-blocking stream (default);  */
                              /* CTD_STREAM_GIVEN: launch on `stream` (NULL = the device's default stream),   */
                              /* so launches are ordered with the caller's other work on that stream          */
    int32_t control_steps;    /* controls per time step: DOCP(ocp, grid_size, control_steps, scheme, time_grid), src/DOCP_data.jl:293.
                               * 0 or 1: collocation (src/collocation.jl:65).  > 1: the direct-shooting layout of
                               * src/direct_shooting.jl:55-71 -- step block [X_i, U_i^1 .. U_i^cs] (midpoint.jl:20), dynamics summed over
                               * the control sub-steps (midpoint.jl:47-72,137-155), cost midpoint.jl:99-116, bounds / initial guess for
                               * every control (DOCP_variables.jl:44,138); path constraints see U_i^1 (common.jl:140-155).  CTD_SCHEME_MIDPOINT
                               * only.  KNOWN DEVIATION (decided, not an omission): the reference accepts control_steps > 1 with every scheme --
                               * it sizes the step block with it (trapeze.jl:20, euler.jl:22, irk.jl:141) and bounds / initialises the extra
                               * controls (DOCP_variables.jl:44-47,138-140) -- but only midpoint.jl integrates over them, and elsewhere its own
                               * layout is incoherent: the stage-variable getter of the IRK schemes keeps the offset n + m (common.jl:166-170),
                               * so K_i^j ALIASES the controls U_i^2.. it has just bounded; the trapeze `:manual` pattern addresses X_{i+1} at
                               * n + m behind X_i (trapeze.jl:180-186), i.e. inside the extra controls, and misses the real X_{i+1} columns;
                               * the stagewise schemes ignore control_steps altogether (irk_stagewise.jl:138-146); Euler is coherent (extra
                               * controls that nothing reads).  The engine returns CTD_ESCHEME for all of them instead of reproducing aliased or
                               * dead variables (direct shooting, the only caller that sets
                               * control_steps, advertises :midpoint and :trapeze, src/direct_shooting.jl:33-37; its default is :midpoint).
                               * Compiled problems: control_steps <= 3; problems registered at run time: any.  Constraints, Jacobian (all three
                               * patterns), objective, gradient, hess_structure and hess_coord (one second-order evaluation point per control). */
    int32_t value_order;      /* CTD_ORDER_CSC (0): Jacobian values in the order of SparseArrays.sparse(Is, Js, ...) as DOCP_Jacobian_pattern
                               * returns it (src/ode/midpoint.jl:229-232, irk_stagewise.jl:555-558) -- what ADNLPModels' jac_coord! fills.
                               * CTD_ORDER_CSR (1): the same entries by ROWS -- what GPU KKT consumers (rocSPARSE / hipSOLVER) take, and what
                               * BASELINE north_star names ("assembled ... in CSR on device").  Same kernel, same bytes; the rows of a time step,
                               * V entries inline, are one contiguous run of the value array, so a shard of the grid owns ONE range
                               * (ctd_shard_info).  ctd_jac_structure / ctd_jac_coord / ctd_cons_jac* follow the order chosen here. */
    int32_t reserved0;        /* must be 0.  ZERO-INITIALISE the whole struct (memset / `ctd_desc d = {0}` / Ref{ctd_desc}(zeros)): fields that were
                               * reserved in an earlier version of this header get a meaning later (control_steps was one), and a nonzero
                               * reserved field is refused with CTD_EINVAL */
} ctd_desc;

enum { CTD_ORDER_CSC = 0, CTD_ORDER_CSR = 1 };

enum { CTD_STREAM_OWN = 0, CTD_STREAM_GIVEN = 1 };

/* replaces the `init` tuple handed to __initial_guess(docp, CTModels.build_initial_guess(ocp, init)),
 * src/collocation.jl:101-102, src/DOCP_variables.jl:122-145, src/ode/irk_stagewise.jl:302-335.
 * NULL pointers mean "not provided" (entries stay at the 0.1 default, src/DOCP_variables.jl:126). */
typedef struct ctd_init {
    int32_t use_problem_default; /* nonzero: use the init tuple of the problem file (e.g. goddard.jl:48)    */
    const double* state;         /* constant state guess  [n]  or NULL                                      */
    const double* control;       /* constant control guess [m] or NULL                                      */
    const double* variable;      /* variable guess [nv] or NULL                                             */
    /* time-dependent guesses -- the functional / interpolated / warm-start forms of CTModels' init.state(t), init.control(t)
     * (test/ci/test_initial_guess.jl): n_samples > 0 gives trajectories sampled at the increasing times t_samples[k];
     * state_samples is row-major [n_samples][n], control_samples [n_samples][m] (either may be NULL).  They are evaluated
     * where the reference evaluates the functions (node times t_i; stage times t_ij for stagewise controls) by linear
     * interpolation, end values held outside the sampled span, and take precedence over the constant entries above. */
    int64_t n_samples;
    const double* t_samples;
    const double* state_samples;
    const double* control_samples;
} ctd_init;

/* ---- OCPs defined at run time ----------------------------------------------------------------------------------
 * The reference obtains the OCP functions as Julia closures from CTModels (CTModels.dynamics(ocp)(dx, t, x, u, v) called
 * at src/ode/trapeze.jl:66, midpoint.jl:64, irk.jl:291, irk_stagewise.jl:441; lagrange / mayer src/DOCP_functions.jl:35-48;
 * path / boundary constraints :108-110,136-138).  A closure cannot cross a C ABI, so an OCP that is not in the compiled
 * registry is handed over as TEXT: one arithmetic expression per output.  Grammar: + - * / parentheses, numbers, ^ with a CONSTANT
 * exponent (small non-negative integers multiply out; any other real exponent is pow), exp log sin cos tan atan tanh sqrt abs asin acos
 * sinh cosh floor, max(a, b) min(a, b) (derivative of the selected operand: ForwardDiff's rule, at a tie max follows b and min a;
 * floor has derivative 0) -- everything the reference's problem folder (test/problems, every .jl file) uses --, the names t, x1..xn, u1..um,
 * v1..vnv (dynamics, lagrange, path) or x0_1.., xf_1.., v1.. (mayer, boundary), and what `constants` declares: "Cd=310; beta=500"
 * (numbers) and "aux = 543 + 186*cos(x4); g13 = -(105 + 2*cos(2*x4)) / (2*aux)" (ALIASES: named sub-expressions, the `aux = ...`
 * lines of a CTParser @def block such as test/problems/swimmer.jl:39-53; substituted where they are used, may use each other).
 * No C++ is accepted.  ctd_register_ocp parses
 * the expressions, generates a functor of the registry's shape and returns a problem id (>= 1000) for ctd_desc.problem;
 * ctd_create then compiles the SAME kernel templates for it with hiprtc (gfx950) -- same code path as a built-in problem.
 * dims, flags and bounds restate DOCPdims / DOCPFlags (src/DOCP_data.jl:24-30,88-94) and the boxes of CTModels
 * (src/DOCP_variables.jl:88-98).  Bound arrays may be NULL (boxes: free; path / boundary: equality with 0). */
typedef struct ctd_ocp_def {
    const char* name;
    int32_t n, m, nv, npath, nbc;        /* state, control, variable, path-constraint, boundary-constraint dimensions */
    int32_t it0, itf;                    /* 0-based index of t0 / tf inside v, -1 = fixed                             */
    double t0, tf;                       /* fixed values when the index is -1                                          */
    int32_t maximize;                    /* DOCPFlags.max                                                              */
    int32_t reserved;
    const char* const* dynamics;         /* n expressions                                                              */
    const char* lagrange;                /* running cost or NULL                                                       */
    const char* mayer;                   /* terminal cost or NULL                                                      */
    const char* const* path;             /* npath expressions                                                          */
    const char* const* boundary;         /* nbc expressions                                                            */
    const char* constants;               /* "name=value; ..." or NULL                                                  */
    const double *state_lb, *state_ub, *control_lb, *control_ub, *variable_lb, *variable_ub;
    const double *path_lb, *path_ub, *boundary_lb, *boundary_ub;
} ctd_ocp_def;
int32_t ctd_register_ocp(const ctd_ocp_def* def, int32_t* problem_id);
/* the functor text generated for a registered OCP (diagnostics / tests).  cap too small: CTD_EINVAL and ctd_last_error(NULL)
 * = "... needs <n> bytes" (nothing is written, never a truncated text) */
int32_t ctd_ocp_source(int32_t problem_id, char* buf, int64_t cap);
/* compile-only check, no device needed: the kernels of `scheme` build for gfx950 (ctd_last_error(NULL) holds the log) */
int32_t ctd_jit_check(int32_t problem_id, int32_t scheme);

/* ---- lifecycle ------------------------------------------------------------------------------------------ */
/* get_docp: DOCP(...) + __variables_bounds! + __constraints_bounds!   (src/collocation.jl:57-73) */
int32_t ctd_create(const ctd_desc* desc, ctd_handle** out);
int32_t ctd_destroy(ctd_handle* h);
const char* ctd_last_error(const ctd_handle* h);   /* h may be NULL: error of the last failed ctd_create */
/* Page-locked host memory for the vectors a caller hands to the host-pointer entry points (x, c, vals, g, y ...): the
 * copies then run as direct DMA at PCIe rate instead of through the runtime's bounce buffers.  Optional -- any host pointer
 * is accepted everywhere -- and independent of handles.  The reference's vectors are plain Julia arrays owned by the solver
 * (src/collocation.jl:137-149); a shim would wrap these with unsafe_wrap. */
int32_t ctd_host_alloc(void** ptr, size_t bytes);
int32_t ctd_host_free(void* ptr);
const char* ctd_strerror(int32_t status);

/* ---- sizes and static data (host) ------------------------------------------------------------------------ */
/* docp.dim_NLP_variables, docp.dim_NLP_constraints (src/DOCP_data.jl:285-286), nlp.meta.nnzj, nlp.meta.nnzh
 * (nnzh = entries of the lower triangle of DOCP_Hessian_pattern, e.g. 6519 for Goddard / midpoint / 250 steps,
 * test/archives/AD_backend.md:86) */
int32_t ctd_sizes(const ctd_handle* h, int64_t* nvar, int64_t* ncon, int64_t* nnzj, int64_t* nnzh);
/* out[0..15]: NLP_x, NLP_u, NLP_v, path_cons, boundary_cons (DOCPdims, src/DOCP_data.jl:88-94), steps,
 * _step_variables_block, _state_stage_eqs_block, _step_pathcons_block, stage, _final_control, freet0, freetf,
 * lagrange, mayer, max (DOCPFlags, :24-30) */
int32_t ctd_dims(const ctd_handle* h, int64_t* out16);
/* docp.time.normalized_grid / fixed_grid (src/DOCP_data.jl:147-152), each N+1 */
int32_t ctd_time_grid(const ctd_handle* h, double* normalized, double* fixed);
/* get_time_grid(xu, docp), src/DOCP_data.jl:437-458: grid[i] = t0 + tau_i (tf - t0) with t0 / tf fixed or read from the
 * tail of x (host pointers; post-processing helper for the solution rebuild, src/DOCP_data.jl:514-633) */
int32_t ctd_time_grid_at(const ctd_handle* h, const double* x, double* grid);
/* Butcher tables of the scheme struct (row-major a[stage*stage], b[stage], c[stage]), src/ode/irk_stagewise.jl:61-64,103-109 */
int32_t ctd_butcher(const ctd_handle* h, double* a, double* b, double* c);
/* docp.bounds.var_l/var_u/con_l/con_u : __variables_bounds! (src/DOCP_variables.jl:21-63, irk_stagewise.jl:250-300)
 * and __constraints_bounds! (src/DOCP_functions.jl:163-191) */
int32_t ctd_bounds(const ctd_handle* h, double* lvar, double* uvar, double* lcon, double* ucon);
/* __initial_guess (src/DOCP_variables.jl:122-145, irk_stagewise.jl:302-335) */
int32_t ctd_initial_guess(const ctd_handle* h, double* x0, const ctd_init* init);
/* jac_structure!(nlp, rows, cols): 1-based (row, col) of every entry of DOCP_Jacobian_pattern(docp) in CSC order
 * (src/ode/trapeze.jl:149-233, midpoint.jl:163-233, irk.jl:315-416, irk_stagewise.jl:468-558) */
int32_t ctd_jac_structure(const ctd_handle* h, int64_t* rows, int64_t* cols);
/* same pattern as 0-based CSC (colptr[nvar+1], rowval[nnzj]) -- the order of the values of a CTD_ORDER_CSC handle */
int32_t ctd_jac_csc(const ctd_handle* h, int64_t* colptr, int64_t* rowval);
/* same pattern as 0-based CSR (rowptr[ncon+1], colind[nnzj]) -- the order of the values of a CTD_ORDER_CSR handle: pass rowptr / colind and the
 * device array ctd_cons_jac_dev fills straight to rocsparse_create_csr_descr.  Available on every handle (the pattern is the same set). */
int32_t ctd_jac_csr(const ctd_handle* h, int64_t* rowptr, int64_t* colind);
/* ctd_desc.value_order of the handle */
int32_t ctd_value_order(const ctd_handle* h, int32_t* order);
/* number of structurally nonzero Jacobian entries that the selected pattern does not hold (0 except
 * REFERENCE_MANUAL + trapeze + a free time / v-dependent dynamics: hazard H1) */
int32_t ctd_dropped_nonzeros(const ctd_handle* h, int64_t* count);

/* ---- the hot path: host pointers -------------------------------------------------------------------------- */
/* obj(nlp, x)       = __objective(x, docp)                       src/DOCP_functions.jl:23-54 */
int32_t ctd_obj(ctd_handle* h, const double* x, double* f);
/* grad!(nlp, x, g): gradient of __objective with respect to the nvar NLP variables (the reference obtains it with
 * ReverseDiff over the objective closure: gradient_backend = ReverseDiffADGradient, src/collocation.jl:127).
 * Always the gradient of the whole objective, also on a sharded handle (it is O(nvar) work). */
int32_t ctd_grad(ctd_handle* h, const double* x, double* g);
/* cons!(nlp, x, c)  = __constraints!(c, x, docp)                 src/DOCP_functions.jl:80-115 */
int32_t ctd_cons(ctd_handle* h, const double* x, double* c);
/* jac_coord!(nlp, x, vals): values of dc/dx in the pattern's CSC order (ADNLPModels.SparseADJacobian,
 * call site src/collocation.jl:116-120) */
int32_t ctd_jac_coord(ctd_handle* h, const double* x, double* vals);
/* fused cons! + jac_coord! at one x: the benchmarked call (BASELINE.json metric) */
int32_t ctd_cons_jac(ctd_handle* h, const double* x, double* c, double* vals);

/* ---- the hot path: device pointers (inputs and outputs stay in HBM) --------------------------------------- */
/* POINTERS, for every entry point of this header whose name ends in _dev, _dev_async, _shard_dev_async or _batch_dev_async
 * (this section, the Hessian, the batched callbacks, the fused iteration, the matrix-free operators, the MINRES solve and their
 * shard forms):
 *   - no pointer needs more than 8-byte alignment -- inputs and outputs may be slices of one workspace at any offset that is a
 *     multiple of 8 bytes, the rows of a batched argument at any leading dimension the entry point accepts;
 *   - nothing outside the documented output ranges is written: not one double before or after an output, none of the padding
 *     between the rows of a batched output, and on a shard handle none of the entries the shard does not own;
 *   - inputs are never written.
 * The results do not depend on the addresses.  tests/test_gpu_write_sets.py holds every one of these entry points to that between
 * guard regions (tests/guarded.py), tests/test_gpu_kkt_minres.py the MINRES solve. */
/* c_dev has ncon entries and vals_dev nnzj entries (global indexing also for sharded handles: a shard writes only
 * its rows / its CSC ranges, see ctd_shard_info).  Either of c_dev / vals_dev may be NULL to skip that output. */
int32_t ctd_cons_jac_dev(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev);
int32_t ctd_cons_jac_dev_async(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev);
int32_t ctd_obj_dev(ctd_handle* h, const double* x_dev, double* f_host);
int32_t ctd_grad_dev(ctd_handle* h, const double* x_dev, double* g_dev);
/* enqueue-only variants for device-resident solver loops: the objective goes to f_dev[0] (device memory), nothing is
 * copied to the host and nothing waits; ctd_sync (or any later work on the handle's stream) orders the results */
/* Launch on `stream` (a hipStream_t, NULL = the device's default stream) from now on, e.g. the capturing stream while the
 * caller records a HIP graph of a whole solver iteration: every *_dev_async entry point only enqueues kernels (and one
 * memset) and is capturable.  Handles of run-time OCPs and the first Hessian call compile / upload on first use: call
 * each entry point once before capturing. */
int32_t ctd_set_stream(ctd_handle* h, void* stream);
int32_t ctd_obj_dev_async(ctd_handle* h, const double* x_dev, double* f_dev);
int32_t ctd_grad_dev_async(ctd_handle* h, const double* x_dev, double* g_dev);
/* The gradient of a SHARDED transcription without an all-gathered iterate (round 4): on a handle restricted to the steps
 * [step_begin, step_end) this writes ONLY the gradient entries of the shard's own variables -- its step blocks; the last shard also
 * the final state (and final control) -- into the full-length g_dev, and leaves the shard's PARTIAL sums of d/dv in the nv variable
 * entries (the caller adds them over the shards: one all-reduce of nv doubles, as for the V x V entries of the Hessian).  The Mayer
 * term's d/dx0 goes to the shard that owns X_1, its d/dxf and d/dv to the one that owns X_{N+1}.  Neighbours' entries (the next
 * shard's first node and the previous shard's last block for the midpoint / Euler quadrature, X_1 / X_{N+1} for the Mayer term) are read
 * through the table of ctd_set_x_shards like the other callbacks do, or from x_dev itself when no table is set (halos copied).  The
 * quadrature being differentiated: src/DOCP_functions.jl:23-54 with trapeze.jl:78-110, midpoint.jl:79-116, irk_stagewise.jl:344-384.
 * On an unsharded handle it equals ctd_grad_dev_async. */
int32_t ctd_grad_shard_dev_async(ctd_handle* h, const double* x_dev, double* g_dev);
int32_t ctd_sync(ctd_handle* h);

/* ---- multi-GPU shards (time-step partition) ------------------------------------------ */
/* out[0..7]: step_begin, step_end, c_row_begin, c_row_end (step rows this shard writes; in addition EVERY shard writes
 * the p + bc tail rows [N*cb, ncon) -- final-time path and boundary constraints, x being replicated -- so stitching c
 * is a single all-gather), vals_main_begin, vals_main_end, owns_first, owns_last.
 * CTD_ORDER_CSC: [vals_main_begin, vals_main_end) is the contiguous CSC range of the shard's step columns; the shard ALSO writes its
 * slice of every V column, the first shard the irregular first-step columns and the last shard the final-state columns (SURVEY 8e
 * "CSC caveat").  CTD_ORDER_CSR: [vals_main_begin, vals_main_end) is EVERYTHING the shard writes: its step rows, V entries inline
 * (the last shard's range runs to nnzj: the p + bc tail rows follow the step rows) -- one range per rank, the ranges of the ranks
 * partition the value array. */
int32_t ctd_shard_info(const ctd_handle* h, int64_t* out8);

/* ---- measurement ------------------------------------------------------------------------------------------ */
/* Launches the fused kernel `iters` times back-to-back on the handle's stream between two hipEvents (recorded on
 * that same stream) and returns the mean duration of one launch in milliseconds.  Used by bench.py for the
 * roofline figure; the outputs are the normal outputs of ctd_cons_jac_dev. */
int32_t ctd_time_cons_jac_dev(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev,
                              int32_t iters, double* mean_ms);
/* Diagnostics: one launch of the fused kernel with in-kernel phase stamps.  out receives, per workgroup, 6 pairs
 * {100 MHz realtime counter, shader cycle counter} taken by lane 0 at: start, after load, after eval, after fin, after
 * emit issue, after the workgroup's stores drained.  cap = capacity of out in uint64 words (needs grid * 12). */
int32_t ctd_debug_stamps(ctd_handle* h, const double* x_dev, double* c_dev, double* vals_dev, uint64_t* out, int64_t cap);
/* kernel launch geometry: out[0..7] = grid blocks, block threads, dynamic LDS bytes, steps per tile, interior
 * CSC period L (entries per regular step), number of edge entries, 1 when the tiles run the direct driver (x read
 * straight from global memory by the evaluating lanes, one workgroup barrier) and 0 for the staged one, resident workgroups
 * per CU of that kernel (the runtime's occupancy query for its registers and LDS; 0 on a host-only handle) */
int32_t ctd_launch_info(const ctd_handle* h, int64_t* out8);


/* ---- Hessian of the Lagrangian --------------------------------------------------------------------------------
 * Replaces hess_structure!(nlp, rows, cols) / hess_coord!(nlp, x, y, vals; obj_weight) of the ADNLPModel built at
 * src/collocation.jl:137-149 (sparse Hessian backend selected at :121-125).  The sparsity pattern is the lower triangle
 * (row >= col, NLPModels convention) of DOCP_Hessian_pattern(docp) -- src/ode/trapeze.jl:240-303, midpoint.jl:240-300,
 * irk.jl:423-496, irk_stagewise.jl:565-638 -- in CSC order; CTD_PATTERN_STRUCTURAL adds the final-state x variable
 * block whose add_nonzero_block! call has an empty range in the reference (irk.jl:483 / irk_stagewise.jl:625).
 * Values:  vals[k] = obj_weight * d2 f/dx_i dx_j + sum_r y[r] * d2 c_r/dx_i dx_j  at (i, j) = (rows[k], cols[k]),
 * f = __objective (src/DOCP_functions.jl:23-54), c = __constraints! (:80-115); entries of the pattern that are
 * structurally zero receive 0.0.  A sharded handle (step_begin, step_end) writes the entries of its step columns (one
 * contiguous CSC range), the first / last shard also the irregular first-step / final-state entries, and leaves its PARTIAL
 * sums in the nv (nv+1)/2 variable x variable entries (they sum over every step): ctd_hess_shard_info names them for the
 * one all-reduce the caller has to do. */
/* One solver iteration in one call: obj(nlp, x) -> f_dev[0], grad!(nlp, x, g), cons!(nlp, x, c) + jac_coord!(nlp, x, vals) and
 * hess_coord!(nlp, x, y, hvals; obj_weight) -- the NLPModels calls an interior-point iteration makes on the ADNLPModel of
 * src/collocation.jl:137-149 -- in TWO launches for registry problems: one grid whose workgroups take the bodies of the four
 * evaluation kernels by index range (all resident together: the launch costs about what the longest of them, the Hessian,
 * costs instead of their sum), then the fixed-order cross-workgroup sums.  Any output may be NULL to skip that callback.
 * Enqueue-only, like the *_dev_async entry points. */
/* (single-iterate: ctd_eval_all_dev_async has no batched form -- batching it is out of scope; the *_batch_dev_async calls below
 * batch the callbacks one by one) */
int32_t ctd_eval_all_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* f_dev,
                               double* g_dev, double* c_dev, double* vals_dev, double* hvals_dev);

/* ---- batched callbacks: K iterates of ONE transcription per launch -------------------------------------------------------
 * No NLPModels counterpart (one iterate per call there): for hosts that hold many iterates of the same transcription at once --
 * multistart, MPC scenarios / warm starts, parameter sweeps, line-search trial points, finite-difference checks.  One launch of
 * the same kernels evaluates all `batch` members instead of `batch` launches: each launch of a single callback costs ~4 us of
 * dispatch whatever its size.
 * Layout: member b (0 <= b < batch) reads x_dev + b*ldx (and y_dev + b*ldy) and writes c_dev + b*ldc, vals_dev + b*ldv,
 * g_dev + b*ldg, vals_dev + b*ldh (Hessian) and f_dev[b].  Leading dimensions are in doubles (not bytes) and at least the vector
 * length: ldx >= nvar, ldy >= ncon, ldc >= ncon, ldv >= nnzj, ldg >= nvar, ldh >= nnzh; entries between a row's end and the next
 * row are never touched (row slices of wider buffers work).  c_dev / vals_dev may be NULL to skip that output (as in
 * ctd_cons_jac_dev_async; its leading dimension is then not checked).  All members share the handle's transcription, pattern,
 * value order, tables and stream; obj_weight is shared by the members of a Hessian call.
 * Contract: member b's results are BIT-IDENTICAL to one *_dev_async call on member b alone -- the same arithmetic per member and
 * the same fixed-order cross-workgroup sums (one finish workgroup per member).
 * Enqueue-only, like the *_dev_async calls (ctd_sync waits).  The partial-sum buffers of the objective, gradient and Hessian grow
 * with the batch: a call that needs them larger drains the handle's stream first, and is refused (CTD_EINVAL) while the stream is
 * capturing -- make one call with the batch size before a capture.  A run-time OCP compiles its batched constraint / Jacobian
 * kernel at the first batched call.
 * Checks, in this order: h NULL -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE (whatever the other arguments); batch < 1 or
 * > 65535 (the grid's second dimension) -> CTD_EINVAL; a shard handle (step_begin / step_end not the whole grid, or a
 * ctd_set_x_shards table) -> CTD_EINVAL: batched sharded evaluation is out of scope; then null pointers and leading dimensions
 * that are too small -> CTD_EINVAL.  ctd_last_error names the reason. */
int32_t ctd_cons_jac_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* c_dev, int64_t ldc,
                                     double* vals_dev, int64_t ldv);
int32_t ctd_obj_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* f_dev);   /* f_dev[batch] */
int32_t ctd_grad_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, double* g_dev, int64_t ldg);
int32_t ctd_hess_coord_batch_dev_async(ctd_handle* h, int32_t batch, const double* x_dev, int64_t ldx, const double* y_dev, int64_t ldy,
                                       double obj_weight, double* vals_dev, int64_t ldh);

/* Matrix-free Jacobian products at x (NLPModels jprod! / jtprod!; the reference leaves both backends empty,
 * jprod_backend = jtprod_backend = EmptyADbackend, src/collocation.jl:104-110):
 *   Jv  = J(x) v   (ncon entries, the row order of ctd_cons: [C_i^x, C_i^{k,1..s}, G_i].., G_N+1, B)
 *   Jtw = J(x)' w  (nvar entries, the variable layout of the transcription).
 * J is the exact derivative of what ctd_cons computes: the Jacobian of the STRUCTURAL pattern, whatever the handle's
 * pattern_mode or value_order.  On a REFERENCE_MANUAL handle with ctd_dropped_nonzeros > 0 the products therefore include the
 * entries the manual pattern drops, as ADNLPModels' ForwardDiff product backends do.  Results are reproducible bit for bit
 * (fixed summation order, no floating-point atomics) and equal for every pattern_mode / value_order of one transcription.
 * No device memory proportional to nnzj is allocated: the products never assemble J (scratch: one row of kMaxNV partial sums
 * per workgroup; the host calls stage x, the direction and the result).
 * Run-time OCPs (ctd_register_ocp) compile their product kernels on the first call: make one call before capturing a graph.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE; shard handle (step_begin / step_end not
 * the whole grid, or a ctd_set_x_shards table) -> CTD_EINVAL (a shard handle calls ctd_jprod_shard_dev_async /
 * ctd_jtprod_shard_dev_async below); null pointers or an output that equals an input -> CTD_EINVAL. */
/* host pointers: return when the result is in the caller's buffer */
int32_t ctd_jprod(ctd_handle* h, const double* x, const double* v, double* Jv);
int32_t ctd_jtprod(ctd_handle* h, const double* x, const double* w, double* Jtw);
/* device pointers on the handle's device: enqueue-only on the handle's stream (ctd_sync waits), capturable after one warm call */
int32_t ctd_jprod_dev_async(ctd_handle* h, const double* x_dev, const double* v_dev, double* Jv_dev);
int32_t ctd_jtprod_dev_async(ctd_handle* h, const double* x_dev, const double* w_dev, double* Jtw_dev);

/* Matrix-free Hessian-of-the-Lagrangian products at (x, y) (NLPModels hprod!; the reference leaves the backend empty,
 * hprod_backend = EmptyADbackend, src/collocation.jl:104-110):
 *   Hv = (obj_weight H_f(x) + sum_r y_r H_{c_r}(x)) v   (nvar entries, the variable layout of the transcription)
 * x, v and Hv have nvar entries, y has ncon entries in the row order of ctd_cons.  y == NULL: every multiplier is zero (the
 * objective-only hprod!(nlp, x, v, Hv; obj_weight)), bit-identical to passing a zero vector.
 * H is the exact second derivative of what ctd_obj and ctd_cons compute: the Hessian of the STRUCTURAL pattern, whatever the
 * handle's pattern_mode or value_order -- Mayer and Lagrange terms, boundary and path rows, and the second-order terms through a
 * free t0 / tf (time grid, step length h, the h K products of the Gauss-Legendre steps) included; kinks (abs, floor, max, min)
 * follow the conventions of ctd_hess_coord.  On a REFERENCE_MANUAL handle the product therefore includes the entries the manual
 * pattern drops.  Results are reproducible bit for bit (fixed summation order, no floating-point atomics) and equal for every
 * pattern_mode / value_order of one transcription.  No device memory proportional to nnzh or nnzj is allocated (scratch: one row
 * of kMaxNV partial sums per workgroup; the host call stages x, y, v and the result).
 * Run-time OCPs (ctd_register_ocp) compile their hprod kernels on the first hprod call: make one call before capturing a graph.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE; shard handle (step_begin / step_end not
 * the whole grid, or a ctd_set_x_shards table) -> CTD_EINVAL (a shard handle calls ctd_hprod_shard_dev_async below); null x, v
 * or Hv, or Hv equal to x, y or v -> CTD_EINVAL. */
/* host pointers: return when the result is in the caller's buffer */
int32_t ctd_hprod(ctd_handle* h, const double* x, const double* y, double obj_weight, const double* v, double* Hv);
/* device pointers on the handle's device: enqueue-only on the handle's stream (ctd_sync waits), capturable after one warm call */
int32_t ctd_hprod_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* v_dev,
                            double* Hv_dev);

/* Matrix-free product with the regularised augmented (KKT) matrix at (x, y): the operator a Krylov solver applies once per inner
 * iteration of an interior-point or SQP step.  There is no NLPModels counterpart.
 *   rx = (obj_weight H_f(x) + sum_r y_r H_{c_r}(x)) dx + J(x)' dy + sx o dx   (nvar entries)
 *   rc = J(x) dx - sc o dy                                                    (ncon entries)
 * NOTE THE SIGN of sc: the bottom block is J dx MINUS sc o dy, the quasi-definite form that Ipopt and MadNLP regularise to
 * (sx, sc >= 0 make K symmetric quasi-definite).  x, dx, sx and rx have nvar entries; y, dy, sc and rc have ncon entries in the row
 * order of ctd_cons.  H and J are the structural ones, exactly as documented for ctd_hprod and ctd_jprod above: the exact
 * derivatives of what ctd_obj / ctd_cons compute whatever the handle's pattern_mode or value_order, kinks by the conventions of
 * ctd_hess_coord, second-order terms through a free t0 / tf included.
 * y == NULL: every multiplier is zero.  sx == NULL or sc == NULL: that diagonal term is absent.  Each gives results value-equal to
 * passing a vector of zeros.  dy is required.
 * rx / rc, and dx / dy, may be the two halves of one (nvar + ncon)-long buffer (a Krylov vector): no pointer needs more than
 * 8-byte alignment.
 * Two kernel launches per call (a unit pass and a finish, like ctd_hprod) instead of the seven dispatches of hprod + jtprod +
 * jprod + two element-wise updates: the second-order lanes of hprod already hold the first derivatives of every row along their
 * own directions (J' dy) and along dx (J dx).  The results differ from that composition by rounding only; they are NOT its bits.
 * Results are reproducible bit for bit (fixed summation order, no floating-point atomics) and equal for every pattern_mode /
 * value_order of one transcription.  No device memory proportional to nnzj or nnzh is allocated; the partial-sum buffer (one row of
 * kMaxNV doubles per workgroup) is this call's own, so a graph captured over ctd_hprod or ctd_jtprod keeps its buffer; the host call
 * stages its eight vectors through buffers the handle owns.
 * Run-time OCPs (ctd_register_ocp) compile their KKT kernels on the first ctd_kktprod* call: make one call before capturing a
 * graph.
 * OUT OF SCOPE: a batched form and several right-hand sides per call.  The diagonals a scaling preconditioner of this operator
 * is built from are ctd_hdiag, ctd_jsq_rows and ctd_jsq_cols below; block and Riccati-type preconditioners are not provided.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE, whatever the other arguments; shard handle
 * (step_begin / step_end not the whole grid, or a ctd_set_x_shards table) -> CTD_EINVAL (a shard handle calls
 * ctd_kktprod_shard_dev_async below); null x, dx, dy, rx or rc -> CTD_EINVAL;
 * an output equal to any input, or rx == rc -> CTD_EINVAL.  ctd_last_error names the reason. */
/* host pointers: returns when rx, rc are in the caller's buffers */
int32_t ctd_kktprod(ctd_handle* h, const double* x, const double* y, double obj_weight, const double* dx, const double* dy,
                    const double* sx, const double* sc, double* rx, double* rc);
/* device pointers on the handle's device: enqueue-only on the handle's stream (ctd_sync waits), capturable after one warm call */
int32_t ctd_kktprod_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* dx_dev,
                              const double* dy_dev, const double* sx_dev, const double* sc_dev, double* rx_dev, double* rc_dev);

/* Matrix-free diagonals of the blocks of the KKT matrix K = [[H + Sx, J'], [J, -Sc]] at (x, y): what a first-level (scaling)
 * preconditioner of ctd_kktprod is built from, and the row / column norms of J that gradient-based NLP scaling uses.  There is no
 * NLPModels counterpart; without them the only route is ctd_hess_coord + ctd_jac_coord, the assembly the products avoid.
 *   ctd_hdiag:     Hd_j  = (obj_weight H_f(x) + sum_r y_r H_{c_r}(x))_jj     (nvar entries; y == NULL: objective only, bit-identical
 *                                                                            to a zero vector)
 *   ctd_jsq_rows:  out_r = sum_j wx_j J_rj^2 = diag(J diag(wx) J')_r          (ncon entries; wx: nvar weights, NULL = ones)
 *   ctd_jsq_cols:  out_j = sum_r wc_r J_rj^2 = diag(J' diag(wc) J)_j          (nvar entries; wc: ncon weights, NULL = ones)
 * NULL weights are bit-identical to a vector of ones.  H and J are the structural ones, exactly as documented for ctd_hprod and
 * ctd_jprod above: entries a REFERENCE_MANUAL pattern drops and the terms through a free t0 / tf are included, kinks follow the
 * conventions of ctd_hess_coord.  A scaling preconditioner of K: px = |Hd + sx|, pc = jsq_rows(x, 1 / px) + sc, M = diag(1/px, 1/pc)
 * -- it needs |Hd_j + sx_j| away from zero, and it is no constraint preconditioner.
 * hdiag and jsq_cols are two kernel launches (a unit pass and a finish), jsq_rows is one.  Results are reproducible bit for bit
 * (fixed summation order, no floating-point atomics) and equal for every pattern_mode / value_order of one transcription.  No
 * device memory proportional to nnzj or nnzh is allocated, nothing is assembled; hdiag and jsq_cols each have a partial-sum buffer
 * of their own (one row of kMaxNV doubles per workgroup), so a graph captured over any other product keeps its buffer; the host
 * calls stage x, y / the weights and the result through buffers the handle owns.
 * Run-time OCPs (ctd_register_ocp) compile these kernels -- one family for the three calls -- on the first of these calls: make one
 * call before capturing a graph.
 * OUT OF SCOPE: batched forms, row / column max-norms.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE, whatever the other arguments; shard handle
 * (step_begin / step_end not the whole grid, or a ctd_set_x_shards table) -> CTD_EINVAL (a shard handle calls
 * ctd_hdiag_shard_dev_async / ctd_jsq_rows_shard_dev_async / ctd_jsq_cols_shard_dev_async below); null x or output -> CTD_EINVAL;
 * an output equal to an input -> CTD_EINVAL.  ctd_last_error names the reason. */
/* host pointers: return when the result is in the caller's buffer */
int32_t ctd_hdiag(ctd_handle* h, const double* x, const double* y, double obj_weight, double* Hd);
int32_t ctd_jsq_rows(ctd_handle* h, const double* x, const double* wx, double* out);
int32_t ctd_jsq_cols(ctd_handle* h, const double* x, const double* wc, double* out);
/* device pointers on the handle's device: enqueue-only on the handle's stream (ctd_sync waits), capturable after one warm call */
int32_t ctd_hdiag_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* Hd_dev);
int32_t ctd_jsq_rows_dev_async(ctd_handle* h, const double* x_dev, const double* wx_dev, double* out_dev);
int32_t ctd_jsq_cols_dev_async(ctd_handle* h, const double* x_dev, const double* wc_dev, double* out_dev);

/* ---- device-resident preconditioned MINRES solve of the KKT system ------------------------------------------------------
 * K z = rhs with K = [[H + Sx, J'], [J, -Sc]] the operator of ctd_kktprod at (x, y, obj_weight, sx, sc), z and rhs of
 * nvar + ncon entries (variables first), H and J assembled nowhere.  The recurrences are preconditioned MINRES (Paige & Saunders)
 * exactly as scipy.sparse.linalg.minres evaluates them -- the same variables, the same initialisation, z0 = 0, the stopping tests
 * test1 = phibar / (Anorm ynorm) <= rtol or test2 = root / Anorm <= rtol -- so iteration counts are comparable with scipy's.
 * The preconditioner is M = diag(1 / px, 1 / pc), applied element-wise (px: nvar entries, pc: ncon entries, e.g. the pair of
 * DOCP.kkt_diag_precond / ctd_hdiag + ctd_jsq_rows); px == NULL and pc == NULL: none.  M must be positive definite.
 * One iteration is the two launches of ctd_kktprod_dev_async plus three vector kernels, with no host synchronisation: the scalar
 * recurrences and the stopping tests run on the device, in a state block the handle owns.  Once the status is set -- converged,
 * breakdown (r2' M r2 negative or not finite: M is not positive definite, or a NaN appeared; or the Krylov space is exhausted
 * without convergence), iteration cap -- the kernels of every later iteration return before they store anything: iterations
 * enqueued past that point cost time and change no bit of z or of the state.  Every entry point enqueues a number of launches
 * fixed by its arguments; kernel boundaries are the only synchronisation between workgroups.
 * Results are reproducible bit for bit (fixed summation order of the inner products, documented in csrc/ctd_krylov_kernels.hpp; no
 * floating-point atomics), equal for the host and the device form and for every pattern_mode / value_order of one transcription.
 * No pointer needs more than 8-byte alignment.
 * WORKSPACE: CTD_KKT_MINRES_WORKSPACE(nvar + ncon) doubles of device memory the handle owns (the Krylov vectors, the partial sums,
 * the state), allocated by the first start and freed with the handle, plus a partial-sum buffer for its kktprod launches that is
 * not the one of ctd_kktprod* (a graph captured over ctd_kktprod keeps working); nothing nnzj- or nnzh-sized.  The host form also
 * stages its vectors (3 (nvar + ncon) doubles more).  One solve per handle at a time: a start discards the solve before it.
 * Capturable after one warm start on the handle (run-time OCPs compile their KKT kernels then).
 * OUT OF SCOPE: several right-hand sides, a nonzero initial guess.  Shard handles are refused by these entry points: the solve on a
 * shard of the grid is the ctd_kkt_minres_shard_* family below, whose collectives are the caller's.
 * Checks in this order: NULL handle -> CTD_EINVAL; sys (info) NULL or its struct_size not sizeof(ctd_kkt_system)
 * (sizeof(ctd_minres_info)) -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE; shard handle -> CTD_EINVAL (these entry points
 * have no shard form: ctd_kkt_minres_shard_* below is it); null x, rhs or z -> CTD_EINVAL; z equal to any input -> CTD_EINVAL; only one of px / pc -> CTD_EINVAL; k, max_iter or
 * check_every < 1, or rtol < 0 or NaN -> CTD_EINVAL; iters before any start, or with another z than the start -> CTD_EINVAL.
 * ctd_last_error names the reason, beginning with the entry point that was called. */
#define CTD_KKT_MINRES_WORKSPACE(n) (8 * (int64_t)(n) + 3072)
enum { CTD_MINRES_RUNNING = 0, CTD_MINRES_CONVERGED = 1, CTD_MINRES_MAX_ITER = 2, CTD_MINRES_BREAKDOWN = 3 };
/* the operator and the preconditioner: the arguments of ctd_kktprod (y, sx, sc may be NULL with its meaning) and px, pc (both or
 * neither).  struct_size = sizeof(ctd_kkt_system), set by the caller */
typedef struct ctd_kkt_system {
    uint32_t struct_size;
    uint32_t reserved;          /* 0 */
    const double* x;
    const double* y;
    double obj_weight;
    const double* sx;
    const double* sc;
    const double* px;
    const double* pc;
} ctd_kkt_system;
/* struct_size = sizeof(ctd_minres_info), set by the caller; iterations: completed ones (the iterate z is theirs); phibar: the
 * estimate of the M-norm of the residual, beta1 its initial value sqrt(rhs' M rhs); Anorm, ynorm: scipy's estimates of |K|, |z| */
typedef struct ctd_minres_info {
    uint32_t struct_size;
    int32_t status;             /* CTD_MINRES_* */
    int64_t iterations;
    double phibar, Anorm, ynorm, beta1;
} ctd_minres_info;
/* Enqueue-only on the handle's stream, device pointers.  start: the initialisation (two launches): z = 0, the state; reads rhs and
 * px, pc once (later calls do not read them again).  No iteration cap.  iters: k iterations (5 k launches) of the solve started
 * last, on the same z; x, y, sx, sc are read by every iteration. */
int32_t ctd_kkt_minres_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev, double rtol);
int32_t ctd_kkt_minres_iters_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* z_dev, int64_t k);
/* waits for the handle's stream and reads the state */
int32_t ctd_kkt_minres_info(ctd_handle* h, ctd_minres_info* info);
/* The drivers: start, then chunks of check_every iterations with one ctd_kkt_minres_info between chunks, until the status is set --
 * at most ceil(max_iter / check_every) chunks: the device sets CTD_MINRES_MAX_ITER after max_iter iterations.  z does not depend
 * on check_every.  Device pointers / host pointers (staged like the other host forms); both return when z is final. */
int32_t ctd_kkt_minres_dev(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev, double rtol,
                           int64_t max_iter, int64_t check_every, ctd_minres_info* info);
int32_t ctd_kkt_minres(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs, double* z, double rtol, int64_t max_iter,
                       int64_t check_every, ctd_minres_info* info);

/* ---- the MINRES solve on a shard of the grid ------------------------------------------------------------------------------
 * The solve above for a grid sharded by time step over `n_ranks` handles (processes, or handles of one process), rank r holding
 * the r-th block of steps in ascending order: the same recurrences, stopping tests, freeze and launch cut, every rank working on
 * its own entries of the Krylov vectors.  The LIBRARY ISSUES NO COLLECTIVE and never waits for the host: the entry points below
 * are the phases between which the CALLER exchanges data -- three small all-gathers per iteration, no all-reduce:
 *     start;  all-gather slot A;  begin;
 *     per iteration:  exchange the halo of (v_x, v_c);  ctd_kktprod_shard_dev_async on (v_x, v_c) -> (kv_x, kv_c);  alfa;
 *                     all-gather slot A;  lanczos;  all-gather slot B;  update
 * EVERY CROSS-RANK SUM is an all-gather followed by a sum on the device in rank order (csrc/ctd_krylov_shard_kernels.hpp states the
 * order), done redundantly by every rank: the bits of the iterate and of the state depend on the split of the grid only -- not on a
 * collective's algorithm, the backend, or whether the shards live in one process or several -- and every rank holds the same
 * state bytes, so all ranks stop after the same chunk without agreeing on it.  A single shard of the whole grid gives the bits of
 * ctd_kkt_minres_dev.
 * OWNED ENTRIES of a rank (ctd_kkt_minres_shard_layout), of every n-vector (n = nvar + ncon, variables first; z, rhs, the
 * workspace vectors): its variables [var_begin, var_end), the nv tail [tail_begin, tail_end) -- replicated: every rank keeps and
 * updates it with the same bits, the last rank counts it in the inner products --, its rows [row_begin, row_end).  Nothing else of
 * z or of a workspace vector is written.  rhs, px, pc must be valid on the owned entries (the tail on every rank).
 * WORKSPACE, caller-owned: CTD_KKT_MINRES_SHARD_WORKSPACE(n, n_ranks) doubles of device memory, cut by
 * ctd_kkt_minres_shard_layout: v and kv (n entries each; their halves are dx, dy / rx, rc of ctd_kktprod_shard_dev_async), the two
 * SEND SLOTS of CTD_KKT_MINRES_SHARD_SLOT doubles each -- what the rank contributes to an all-gather -- and the two GATHERED areas
 * of n_ranks slots, rank-major, which the caller's all-gather fills (n_ranks == 1: the gathered areas are the send slots, nothing
 * is to be gathered).  The handle keeps no state of the solve: two solves on two workspaces do not interfere.
 * Entries read and written per phase (owned entries only; K v at the nv tail is taken from the gathered partial sums of slot A):
 *   start    reads rhs, px, pc; writes z = 0, every workspace vector, send slot A (partial sums of beta1^2), the padding of both
 *   begin    reads gathered A; writes v, the state
 *   alfa     reads v, kv, r1; writes send slot A (partial sums of alfa, the rank's partial sums of the tail of kv)
 *   lanczos  reads gathered A, kv, z, v, w, w2, minv; writes r1, r2, y, send slot B
 *   update   reads gathered B, y; writes w, w2, z, v, the state
 * Once the status is set every phase returns before it stores anything (alfa still commits the state once).
 * Every handle is accepted: a whole-grid handle is the single shard of a one-rank split.
 * Checks in this order: NULL handle -> CTD_EINVAL; sys / info / layout NULL or struct_size wrong -> CTD_EINVAL; host-only handle
 * -> CTD_ENODEVICE (not the layout query, which needs no device); n_ranks < 1 or rank outside [0, n_ranks) -> CTD_EINVAL; a handle
 * whose steps cannot be block `rank` of a split into n_ranks blocks (n_ranks > N; rank 0 must begin at step 0 and no other rank
 * does, rank n_ranks - 1 must end at step N and no other rank does; at least rank steps before it and n_ranks - 1 - rank after
 * it) -> CTD_EINVAL; null or misaligned (8 bytes) pointers -> CTD_EINVAL; z (n entries) overlapping the workspace
 * (CTD_KKT_MINRES_SHARD_WORKSPACE doubles) anywhere -> CTD_EINVAL; start: z or the workspace overlapping rhs, px or pc, only one of
 * px / pc, rtol < 0 or NaN, max_iter < 1 -> CTD_EINVAL.  ctd_last_error names the entry point and the argument. */
#define CTD_KKT_MINRES_SHARD_SLOT 2080
#define CTD_KKT_MINRES_SHARD_WORKSPACE(n, n_ranks) (8 * (int64_t)(n) + (2 + 2 * (int64_t)(n_ranks)) * CTD_KKT_MINRES_SHARD_SLOT + 96)
/* struct_size = sizeof(ctd_minres_shard_layout), set by the caller.  Indices into an n-vector: var_*, tail_*, row_* (rows:
 * nvar + the row); n_own: the entries the rank updates, n_dot: those it counts in a sum; nwg, chunk: the launch geometry over the
 * compacted list of owned indices; off_*: offsets in doubles into the workspace; workspace: the doubles it needs */
typedef struct ctd_minres_shard_layout {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t n, n_ranks;
    int64_t var_begin, var_end, tail_begin, tail_end, row_begin, row_end;
    int64_t n_own, n_dot, nwg, chunk;
    int64_t slot;
    int64_t off_v, off_kv, off_send_a, off_send_b, off_gathered_a, off_gathered_b, off_state;
    int64_t workspace;
} ctd_minres_shard_layout;
int32_t ctd_kkt_minres_shard_layout(ctd_handle* h, int32_t n_ranks, ctd_minres_shard_layout* out);
/* Enqueue-only on the handle's stream, device pointers, one launch each; capturable (run-time OCPs after one warm
 * ctd_kktprod_shard_dev_async).  start reads sys->px / sys->pc (both or neither) and nothing else of sys */
int32_t ctd_kkt_minres_shard_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, const double* rhs_dev, double* z_dev,
                                             double* ws_dev, int32_t n_ranks, int32_t rank, double rtol, int64_t max_iter);
int32_t ctd_kkt_minres_shard_begin_dev_async(ctd_handle* h, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_shard_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_shard_lanczos_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_shard_update_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
/* waits for the handle's stream and reads the state out of the workspace: the one host read per chunk of iterations */
int32_t ctd_kkt_minres_shard_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info);

/* ---- chunked block-tridiagonal Schur preconditioner of the KKT MINRES solve ----------------------------------------------------
 * The constraint rows come in N consecutive blocks of block_rows = m rows (block k: the rows of step k -- state equation, stage
 * equations, path rows of node k), followed by tail_rows rows (final path rows, boundary rows); the last tail_cols = nv variables
 * (free t0 / tf, parameters) are the tail columns.  With Jt = J without the tail columns, w = 1 / px and a chunk length L >= 1
 * (chunk_steps), chunk c covers the blocks [c L, min((c + 1) L, N)) and
 *     T_c = Jt_c diag(w) Jt_c' + Sc_c            (Jt_c: the rows of chunk c; block tridiagonal, m x m blocks)
 *     M^-1 = blkdiag(diag(px), T_0, T_1, ..., diag(pc_tail)).
 * The preconditioner applied is M: variables divided by px, tail rows by their pc, the rows of chunk c solved with the Cholesky
 * factor of T_c.  Couplings between chunks are dropped: chunks are independent, each T_c is a principal submatrix of a positive
 * semidefinite matrix plus Sc.  L >= N is one chunk (the effective chunk_steps is min(L, N)).
 * The kernels do not depend on the OCP (compiled once, strict rounding); plain stores, no atomics, kernel boundaries are the only
 * synchronisation between workgroups, the number of launches is fixed by the arguments, results are reproducible bit for bit: the
 * order of every sum is stated in csrc/ctd_schur_kernels.hpp.
 * LAYOUT (ctd_kkt_schur_layout; works on host-only handles): derived from the handle's layout, and checked on the handle's own
 * Jacobian pattern: two rows that share a non-tail column lie in the same or in adjacent blocks (tail rows exempt), otherwise
 * CTD_EPATTERN with the row in the message.  Refused: block_rows > 64 (CTD_EINVAL), chunk_steps < 1 (CTD_EINVAL), shard handles
 * (CTD_EINVAL: the shard form is ctd_kkt_schur_cr_shard_* below), handles whose value_order is not CTD_ORDER_CSR (CTD_EINVAL).
 * WORKSPACE, caller-owned: CTD_KKT_SCHUR_WORKSPACE(N, m) doubles of device memory: 512 fixed (a header, the partial sums of the
 * solve inside MINRES), N words of per-chunk status, N m^2 for the diagonal blocks D_k -> L_k, N m^2 for the couplings E_k -> F_k.
 * Checks in this order: NULL handle -> CTD_EINVAL; struct sizes -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE (not the layout);
 * shard handle -> CTD_EINVAL; value_order not CSR -> CTD_EINVAL; block_rows > 64, chunk_steps < 1 -> CTD_EINVAL; the pattern ->
 * CTD_EPATTERN; null pointers -> CTD_EINVAL; aliasing (an output equal to an input) -> CTD_EINVAL.  ctd_last_error begins with
 * the entry point that was called. */
#define CTD_KKT_SCHUR_FIXED 512
#define CTD_KKT_SCHUR_WORKSPACE(N, m) (CTD_KKT_SCHUR_FIXED + (int64_t)(N) + 2 * (int64_t)(N) * (m) * (m))
/* struct_size = sizeof(ctd_schur_layout), set by the caller.  first_tail_row = N block_rows; chunk_steps: the effective one */
typedef struct ctd_schur_layout {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t N, block_rows, tail_rows, first_tail_row, tail_cols;
    int64_t n_chunks, chunk_steps;
    int64_t workspace;          /* doubles */
} ctd_schur_layout;
int32_t ctd_kkt_schur_layout(ctd_handle* h, int64_t chunk_steps, ctd_schur_layout* out);
/* Factor, enqueue-only, two launches (assemble; block Cholesky, one wave per chunk).  jvals_dev: the nnzj Jacobian values as
 * ctd_cons_jac_dev_async / ctd_jac_coord leave them on a CSR handle; px_dev: nvar entries; sc_dev: ncon entries or NULL (zero);
 * ws_dev: CTD_KKT_SCHUR_WORKSPACE doubles, written in full.  The first call on a handle uploads the pattern (rowptr / colind) and
 * is refused while the stream is capturing.  A pivot that is not positive or not finite is recorded in the workspace (the first
 * bad block of every chunk) and the rest of that chunk's factor is NaN: the solve then yields NaN there, which the breakdown
 * test of MINRES sees. */
int32_t ctd_kkt_schur_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                       int64_t chunk_steps, double* ws_dev);
/* out = blkdiag(T_c)^-1 r on the block rows; r, out: ncon entries, the tail rows of out are left untouched; out must not be r.
 * One launch: a forward and a backward sweep, one wave per chunk.  A workspace that holds no factor of this handle's N and m
 * is recognised on the device and nothing is stored. */
int32_t ctd_kkt_schur_solve_dev_async(ctd_handle* h, const double* ws_dev, const double* r_dev, double* out_dev);
/* waits for the handle's stream; *first_bad_block = -1 when every pivot was positive, otherwise the smallest bad block */
int32_t ctd_kkt_schur_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block);
/* The MINRES solve above with M of this section: sys->px and sys->pc are required (px: the one the factor was built from; pc is
 * read on the tail rows).  Per iteration (B) forms r2 as before and y = M r2 on the variables and the tail rows; ONE ADDED LAUNCH
 * solves the chunks for y on the block rows and writes one partial sum of r2 . y per workgroup (at most 256, a workgroup serves
 * several chunks); (C) -- and the start's last kernel, for beta1^2 -- adds (B)'s partial sums in their order and after them the
 * solve's in ascending workgroup order.  Six launches per iteration (the start: three), no host synchronisation; the freeze
 * covers the added kernel.  The handle remembers that the solve started last carries a factor: ctd_kkt_minres_iters_dev_async
 * and ctd_kkt_minres_info continue it unchanged.  The workspace must stay valid for the whole solve; the solve writes the partial sums in its fixed part and nothing else of it.  Checks as
 * for ctd_kkt_minres_dev, then CSR order, px / pc / schur_ws_dev null, z or the workspace equal to an input. */
int32_t ctd_kkt_minres_schur_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev,
                                             const double* rhs_dev, double* z_dev, double rtol);
int32_t ctd_kkt_minres_schur_dev(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                 double* z_dev, double rtol, int64_t max_iter, int64_t check_every, ctd_minres_info* info);

/* ---- log-depth exact block-tridiagonal Schur preconditioner of the KKT MINRES solve --------------------------------------------
 * The matrix of the section above with ONE chunk, T = Jt diag(1 / px) Jt' + Sc on the N blocks of m rows -- no coupling dropped, no
 * chunk length to choose --, factored and applied by block odd-even (cyclic) reduction: a block Cholesky of T in the
 * nested-dissection order of the time axis.  n_levels = ceil(log2 N) levels (0 for N = 1) stand in place of a chain of N blocks:
 * at level l the blocks that are odd multiples of 2^l are eliminated, all of them in parallel, one wave per block.  The number of
 * launches is a function of N alone: the factor 2 n_levels + 2 (assemble; per level eliminate and update; the root), the solve
 * solve_launches = 2 n_levels + 1 (per level one launch down, the root, per level one launch up).  Compiled once, strict rounding,
 * plain stores, no atomics, kernel boundaries are the only synchronisation between workgroups, results reproducible bit for bit:
 * the recurrences and the order of every sum are stated in csrc/ctd_schur_cr_kernels.hpp.
 * LAYOUT, refusals and the order of the checks: those of the section above (there is no chunk_steps).
 * WORKSPACE, caller-owned: CTD_KKT_SCHUR_CR_WORKSPACE(N, m) doubles of device memory: 512 fixed (a header with a tag of its own, the
 * partial sums of the solve inside MINRES), N status words (one per block), 3 N m^2 for the blocks, 2 N m of scratch for the solve.
 * A workspace of one family handed to the other's solve is recognised on the device and nothing is stored; the other's info call
 * returns CTD_EINVAL. */
#define CTD_KKT_SCHUR_CR_WORKSPACE(N, m) \
    (CTD_KKT_SCHUR_FIXED + (int64_t)(N) + 3 * (int64_t)(N) * (m) * (m) + 2 * (int64_t)(N) * (m))
/* struct_size = sizeof(ctd_schur_cr_layout), set by the caller */
typedef struct ctd_schur_cr_layout {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t N, block_rows, tail_rows, first_tail_row, tail_cols;
    int64_t n_levels, factor_launches, solve_launches;
    int64_t workspace;          /* doubles */
} ctd_schur_cr_layout;
/* works on host-only handles */
int32_t ctd_kkt_schur_cr_layout(ctd_handle* h, ctd_schur_cr_layout* out);
/* Factor, enqueue-only, factor_launches launches.  Arguments as ctd_kkt_schur_factor_dev_async; ws_dev is written in full.  The
 * pattern upload is shared with the chunked factor: the first factor of either kind on a handle is refused while the stream is
 * capturing.  A pivot that is not positive or not finite: its column is recorded in the block's status word, the block's factors
 * are NaN, and the NaN reaches the later levels by ordinary arithmetic: the solve then yields NaN on the block rows. */
int32_t ctd_kkt_schur_cr_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                          double* ws_dev);
/* out = T^-1 r on the block rows, solve_launches launches; r, out: ncon entries, the tail rows of out are left untouched, r is not
 * modified; out must not be r.  ws_dev is not const: the solve keeps the running right-hand side and y in its scratch region.  The
 * factor part of the workspace is only read. */
int32_t ctd_kkt_schur_cr_solve_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev);
/* waits for the handle's stream; *first_bad_block = -1 when every pivot was positive, otherwise the smallest block index with a
 * recorded pivot */
int32_t ctd_kkt_schur_cr_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block);
/* ctd_kkt_minres_schur_start_dev_async / ctd_kkt_minres_schur_dev with this preconditioner: the same Krylov kernels; between (B) and
 * (C) stand the solve_launches launches of the solve and one small launch that writes at most 256 partial sums of r2 . y over the
 * block rows (workgroup g of G = min(N, 256): the blocks g, g + G, ... in that order), which (C) adds as it adds the chunked
 * solve's.  In an iteration every one of these launches stores nothing unless the status is running.  The handle remembers which
 * kind of factor the solve started last carries: ctd_kkt_minres_iters_dev_async and ctd_kkt_minres_info continue it unchanged.
 * Capturable in a graph after one warm call. */
int32_t ctd_kkt_minres_schur_cr_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev,
                                                const double* rhs_dev, double* z_dev, double rtol);
int32_t ctd_kkt_minres_schur_cr_dev(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev, const double* rhs_dev,
                                    double* z_dev, double rtol, int64_t max_iter, int64_t check_every, ctd_minres_info* info);

/* ---- the shard form of the log-depth exact Schur preconditioner ------------------------------------------------------------------
 * Rank r of G holds the steps [sb, se), N_r = se - sb blocks.  With T of the sections above, T_r is the principal submatrix of T on
 * the blocks [sb, se) and
 *     M^-1 = blkdiag(diag(px), T_0, ..., T_{G-1}, diag(pc_tail)):
 * exact inside a rank (block cyclic reduction over the rank's own blocks, schur_cr_levels(N_r) = ceil(log2 N_r) levels, factor
 * 2 n_levels + 2 launches, solve 2 n_levels + 1), cut at the rank boundaries: each of the G - 1 cuts drops one coupling block
 * T(se, se - 1) of the matrix.  It is the chunked matrix of ctd_kkt_schur_* with the ranks' step ranges -- of any lengths -- as
 * chunks.  No collective is needed: a rank's factor and solve touch its own blocks only.  The kernels are those of the section
 * above, given the rank's blocks through offset pointers (csrc/ctd_schur_cr_kernels.hpp): every sum is in their order, and a
 * whole-grid handle -- the single shard -- leaves the bits of ctd_kkt_schur_cr_factor_dev_async in the factor's part of the
 * workspace (header, status words, blocks) and the bits of ctd_kkt_schur_cr_solve_dev_async in out.
 * Every handle is accepted.  Buffers are full-length with global indexing (jvals: nnzj, px: nvar, sc / r / out: ncon entries).
 * LAYOUT (works on host-only handles): N the grid's steps; n_blocks = N_r; first_row = sb block_rows; tail_rows, first_tail_row,
 * tail_cols: the grid's (the tail rows are the last rank's in the MINRES solve, none of this family touches them); workspace =
 * CTD_KKT_SCHUR_CR_WORKSPACE(n_blocks, block_rows).  THE READ SET OF THE FACTOR, half-open ranges derived from the handle's own
 * pattern: jvals on [jvals_begin, jvals_end), the CSR range of the rank's block rows (inside ctd_shard_info's range; on the last
 * rank without the tail rows behind it); px on [px_begin, px_end), the span of the non-tail columns of those rows: the rank's own
 * variables and the first node of block se -- the entries ctd_jsq_rows_shard_dev_async reads of its weight --; sc on the rows
 * [first_row, first_row + n_blocks block_rows).  Anything else of the three buffers may hold anything.
 * Refusals: value_order not CTD_ORDER_CSR, block_rows > 64 (CTD_EINVAL), the pattern (CTD_EPATTERN), in the order of the sections
 * above; null pointers, an output equal to an input -> CTD_EINVAL.  ctd_last_error begins with the entry point that was called.
 * A workspace factored for another step range, another N_r or m, or by the chunked family is recognised on the device by the
 * solve (the header: tag, N_r, m, n_levels, sb) and nothing is stored; the info call returns CTD_EINVAL for it. */
/* struct_size = sizeof(ctd_schur_cr_shard_layout), set by the caller */
typedef struct ctd_schur_cr_shard_layout {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t N, step_begin, step_end, n_blocks, block_rows;
    int64_t first_row, tail_rows, first_tail_row, tail_cols;
    int64_t n_levels, factor_launches, solve_launches;
    int64_t workspace;          /* doubles */
    int64_t jvals_begin, jvals_end, px_begin, px_end;
} ctd_schur_cr_shard_layout;
int32_t ctd_kkt_schur_cr_shard_layout(ctd_handle* h, ctd_schur_cr_shard_layout* out);
/* Factor of T_r, enqueue-only, factor_launches launches; reads the read set above, writes the whole workspace.  The pattern upload
 * is shared with the other factors: the first factor of any kind on a handle is refused while the stream is capturing. */
int32_t ctd_kkt_schur_cr_shard_factor_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                                double* ws_dev);
/* out = T_r^-1 r on the rank's block rows [first_row, first_row + n_blocks block_rows): reads r there, writes out there and nothing
 * else of out (not the tail rows, not another rank's rows); solve_launches launches; out must not be r */
int32_t ctd_kkt_schur_cr_shard_solve_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev);
/* waits for the handle's stream; *first_bad_block = -1, or the smallest GLOBAL block index in [sb, se) with a recorded pivot */
int32_t ctd_kkt_schur_cr_shard_info(ctd_handle* h, const double* ws_dev, int64_t* first_bad_block);
/* The shard form of the MINRES solve (ctd_kkt_minres_shard_* above: the same phases, the same three all-gathers by the caller, the
 * same checks) with M of this section.  sys->px and sys->pc are required (px: the one the factor was built from; pc is read on the
 * tail rows).  Both send slots grow to CTD_KKT_MINRES_SCHUR_SHARD_SLOT doubles: the slot above, then room for the solve's at most
 * 256 partial sums of r2 . y over the rank's block rows, padded with +0.0, and their count; the workspace is cut by
 * ctd_kkt_minres_schur_cr_shard_layout (the struct of ctd_kkt_minres_shard_layout; slot = CTD_KKT_MINRES_SCHUR_SHARD_SLOT).  No
 * fourth gather: the partial sums travel in the slots.  start and lanczos take the factor's workspace (the handle keeps no state of
 * the solve): behind their own launch -- which leaves y and its term of the inner product open on the rank's block rows -- they
 * enqueue the solve_launches launches of the solve and one launch that writes min(N_r, 256) partial sums into the send slot
 * (workgroup g: the local blocks g, g + G_r, ... in that order); in lanczos every one of them reads the status (B) read and stores
 * nothing unless it is running.  begin, alfa, update: one launch each.  beta1^2 and beta^2 are one running sum from 0.0: the terms
 * of the diagonal form in their order (ranks ascending, workgroups ascending), then the ranks ascending again, each rank's solve
 * partial sums in ascending workgroup order; with one rank that is the order of ctd_kkt_minres_schur_cr_dev, whose bits a single
 * shard of the whole grid gives.  A failed pivot on one rank is NaN in its partial sums, which reaches beta^2 on every rank: all
 * ranks end with "breakdown" after the same chunk.  Further checks: px / pc / schur_ws null or misaligned, schur_ws overlapping z
 * or the workspace -> CTD_EINVAL. */
#define CTD_KKT_MINRES_SCHUR_SHARD_SLOT (CTD_KKT_MINRES_SHARD_SLOT + 256 + 16)
#define CTD_KKT_MINRES_SCHUR_SHARD_WORKSPACE(n, n_ranks) \
    (8 * (int64_t)(n) + (2 + 2 * (int64_t)(n_ranks)) * CTD_KKT_MINRES_SCHUR_SHARD_SLOT + 96)
int32_t ctd_kkt_minres_schur_cr_shard_layout(ctd_handle* h, int32_t n_ranks, ctd_minres_shard_layout* out);
int32_t ctd_kkt_minres_schur_cr_shard_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev,
                                                      const double* rhs_dev, double* z_dev, double* ws_dev, int32_t n_ranks,
                                                      int32_t rank, double rtol, int64_t max_iter);
int32_t ctd_kkt_minres_schur_cr_shard_begin_dev_async(ctd_handle* h, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_shard_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_shard_lanczos_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev,
                                                        int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_shard_update_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_shard_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info);

/* ---- the joined form of the log-depth exact Schur preconditioner: the couplings across the ranks restored ----------------------------
 * The shard form above is exact inside a rank and drops the G - 1 coupling blocks T(se, se - 1) at the rank boundaries.  This family
 * applies T^-1 itself on the N blocks, on any ascending split of the steps over G ranks, by separator elimination: every rank but
 * rank 0 gives up its first block s = sb as a separator; its interior I = [sb + (rank > 0), se) -- at least one block: se - sb >= 2 for
 * rank >= 1 -- is factored exactly by the block cyclic reduction of the sections above (the same kernels through offset pointers); the
 * G - 1 separators are joined by a reduced block tridiagonal system of G - 1 blocks of m rows, the Schur complement of T on the
 * separators, which every rank assembles from the gathered records and factors redundantly (one wave, a sequential block Cholesky
 * sweep: n_ranks <= CTD_KKT_SCHUR_CR_JOINT_MAX_RANKS).  SPD throughout.  Two collectives by the caller: ONE ALL-GATHER of the factor
 * records at factor time (CTD_KKT_SCHUR_CR_JOINT_FACTOR_SLOT(m) doubles per rank) and ONE ALL-GATHER of the solve records per
 * application (CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT doubles per rank); gathered buffers hold the n_ranks records in rank order, one slot
 * apart.  Identical gathered records give identical bits of the reduced factor, x_s and sigma on every rank.
 *   factor_local   the interface blocks D_s, E[s] = T(s + 1, s), E[b] = T(se, se - 1) by the assemble expression of the sections above;
 *                  the factor of the interior; the spikes Wl = A^-1 (e_a E[s]) and Wr = A^-1 (e_b E[b]') -- all (up to) 2 m columns
 *                  through ONE chain of 2 n_levels + 1 launches, the column as the second grid dimension, each column with the bits of
 *                  a single solve --; the contributions Cll, Crl, Crr and the record (sb, se, m, rank; D_s, Cll, Crl, Crr) into send_dev.
 *   factor_join    S(r, r) = (D_s^(r) - Crr^(r-1)) - Cll^(r), S(r + 1, r) = -Crl^(r) and its block Cholesky sweep: one launch.  Records
 *                  that are not an ascending cover of [0, N) make the reduced factor NaN.
 *   solve_local    g = A^-1 r on the interior rows of out (2 n_levels + 1 launches), then the record (r_s, qu = E[s]' g_a, qd = E[b] g_b).
 *   solve_join     rs~_r = (r_s^(r) - qd^(r-1)) - qu^(r); x_s = S^-1 rs~ (one wave; it also leaves sigma = x_s . rs~ in the workspace at
 *                  off_sigma: r' T^-1 r = sum_r r_I . g_r + sigma); then out_s = x_s on the rank's separator and out = (g - Wl x_s,r) -
 *                  Wr x_s,r+1 on its interior: two launches.  out then holds T^-1 r on the rank's block rows, nothing else is written.
 * With one rank there is no separator, no record and no join launch (send_dev and gathered_dev may be NULL, the joins do nothing):
 * the bits of ctd_kkt_schur_cr_shard_* on the same handle.  The recurrences and the order of every sum:
 * csrc/ctd_schur_cr_joint_kernels.hpp.  Enqueue-only on the handle's stream, plain stores, no atomics, strict rounding.
 * LAYOUT (works on host-only handles): the separator (-1 on rank 0), the interior, the launch counts, the slots and the offsets (in
 * doubles) into the workspace of `workspace` doubles.  THE READ SET OF THE FACTOR: that of the shard form on [sb, se) and, of jvals,
 * the halo [jvals_halo_begin, jvals_halo_end) -- the CSR range of the rows of block se, the next rank's first, right behind the
 * rank's own range; empty on the last rank -- which the caller fills.  px needs nothing more: E[b] adds over the columns that block
 * se shares with block se - 1, inside [px_begin, px_end).
 * Refusals as in the section above, then: n_ranks outside [1, 256], rank outside [0, n_ranks), steps that cannot be block `rank` of
 * n_ranks ascending blocks, a rank >= 1 of one step -> CTD_EINVAL; null or misaligned pointers, an output that overlaps an input ->
 * CTD_EINVAL.  The workspace carries a tag of its own and the rank's identity (interior, steps, n_ranks, rank) in its header: a
 * workspace of the sections above given to this family, or the reverse, or one factored for another split, is recognised on the
 * device and nothing is stored; the info call returns CTD_EINVAL for it. */
#define CTD_KKT_SCHUR_CR_JOINT_MAX_RANKS 256
#define CTD_KKT_SCHUR_CR_JOINT_FACTOR_SLOT(m) (16 + 4 * (int64_t)(m) * (m))
#define CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT (16 + 3 * 64)
/* struct_size = sizeof(ctd_schur_cr_joint_layout), set by the caller */
typedef struct ctd_schur_cr_joint_layout {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t N, n_ranks, rank, step_begin, step_end, separator, int_begin, n_int, block_rows;
    int64_t first_row, tail_rows, first_tail_row, tail_cols;
    int64_t n_levels, n_sep;
    int64_t factor_local_launches, factor_join_launches, solve_local_launches, solve_join_launches;
    int64_t factor_slot, solve_slot;      /* doubles */
    int64_t off_es, off_eb, off_ds, off_wl, off_wr, off_scratch, off_reduced, off_rs, off_xs, off_sigma;
    int64_t workspace;                    /* doubles */
    int64_t jvals_begin, jvals_end, jvals_halo_begin, jvals_halo_end, px_begin, px_end;
} ctd_schur_cr_joint_layout;
int32_t ctd_kkt_schur_cr_joint_layout(ctd_handle* h, int32_t n_ranks, int32_t rank, ctd_schur_cr_joint_layout* out);
/* writes the whole workspace and the factor record (factor_slot doubles) into send_dev; with one rank only the interior's part of the
 * workspace, [0, off_es), and no record (factor_local_launches counts exactly what is launched).  The pattern upload is
 * shared with the other factors: the first factor of any kind on a handle is refused while the stream is capturing */
int32_t ctd_kkt_schur_cr_joint_factor_local_dev_async(ctd_handle* h, const double* jvals_dev, const double* px_dev, const double* sc_dev,
                                                      double* ws_dev, double* send_dev, int32_t n_ranks, int32_t rank);
/* gathered_dev: n_ranks records, factor_slot doubles apart; writes the reduced factor in the workspace */
int32_t ctd_kkt_schur_cr_joint_factor_join_dev_async(ctd_handle* h, double* ws_dev, const double* gathered_dev, int32_t n_ranks,
                                                     int32_t rank);
/* r, out: ncon entries; reads r on the rank's block rows, writes out on its interior rows and the solve record (solve_slot doubles)
 * into send_dev; out must not be r */
int32_t ctd_kkt_schur_cr_joint_solve_local_dev_async(ctd_handle* h, double* ws_dev, const double* r_dev, double* out_dev, double* send_dev,
                                                     int32_t n_ranks, int32_t rank);
/* gathered_dev: n_ranks records, solve_slot doubles apart; out: the one solve_local wrote */
int32_t ctd_kkt_schur_cr_joint_solve_join_dev_async(ctd_handle* h, double* ws_dev, const double* gathered_dev, double* out_dev,
                                                    int32_t n_ranks, int32_t rank);
/* waits for the handle's stream; *first_bad_block = -1, or the smallest GLOBAL block index with a recorded pivot among the rank's
 * interior and the separators (a reduced factor made NaN by records that do not cover the grid reports block 0) */
int32_t ctd_kkt_schur_cr_joint_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, int32_t rank, int64_t* first_bad_block);
/* The shard form of the MINRES solve (ctd_kkt_minres_schur_cr_shard_* above: the same phases, the same THREE all-gathers by the caller,
 * the same checks) with M of this section, T^-1 on the block rows.  No fourth gather: both send slots grow to
 * CTD_KKT_MINRES_SCHUR_JOINT_SLOT doubles -- the slot of the shard form, whose solve partial sums are now those of r_I . g_r over the
 * rank's interior, then the rank's solve record (CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT doubles).  start and lanczos enqueue, behind their own
 * launch, the interior's solve, its partial sums and the record kernel (solve_local_launches + 1 launches); begin and update START
 * with the two join launches (the reduced solve from the gathered records, the correction of y on the rank's own block rows), then
 * their kernel adds sigma = x_s . rs~ -- read from the factor's workspace -- after all gathered partial sums:
 *     beta^2 = [the terms of the diagonal form, ranks ascending] + [the partial sums of r_I . g_r, ranks ascending] + sigma,
 * one running sum from 0.0 (r' T^-1 r split by the block elimination: both parts are non-negative).  v = y / beta in (C) sees the
 * corrected y.  Identical gathered slots give identical sigma, states and decisions on every rank; a failed pivot anywhere reaches
 * every rank's beta^2 as NaN through the records: all ranks end with "breakdown" after the same chunk.  In lanczos and update every
 * added launch reads the status (B) read and stores nothing unless it is running.  With one rank no join launch is enqueued and
 * sigma is not read: the bits of ctd_kkt_minres_schur_cr_shard_* on the same handle, hence of ctd_kkt_minres_schur_cr_dev.  begin
 * and update take the factor's workspace (the handle keeps no state of the solve).  Capturable after one warm call. */
#define CTD_KKT_MINRES_SCHUR_JOINT_SLOT (CTD_KKT_MINRES_SCHUR_SHARD_SLOT + 3 * 64 + 16)
#define CTD_KKT_MINRES_SCHUR_JOINT_WORKSPACE(n, n_ranks) \
    (8 * (int64_t)(n) + (2 + 2 * (int64_t)(n_ranks)) * CTD_KKT_MINRES_SCHUR_JOINT_SLOT + 96)
int32_t ctd_kkt_minres_schur_cr_joint_layout(ctd_handle* h, int32_t n_ranks, int32_t rank, ctd_minres_shard_layout* out);
int32_t ctd_kkt_minres_schur_cr_joint_start_dev_async(ctd_handle* h, const ctd_kkt_system* sys, double* schur_ws_dev,
                                                      const double* rhs_dev, double* z_dev, double* ws_dev, int32_t n_ranks,
                                                      int32_t rank, double rtol, int64_t max_iter);
int32_t ctd_kkt_minres_schur_cr_joint_begin_dev_async(ctd_handle* h, double* schur_ws_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_joint_alfa_dev_async(ctd_handle* h, double* z_dev, double* ws_dev, int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_joint_lanczos_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev,
                                                        int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_joint_update_dev_async(ctd_handle* h, double* schur_ws_dev, double* z_dev, double* ws_dev,
                                                       int32_t n_ranks, int32_t rank);
int32_t ctd_kkt_minres_schur_cr_joint_info(ctd_handle* h, const double* ws_dev, int32_t n_ranks, ctd_minres_info* info);

/* ---- matrix-free products on a shard of the grid ------------------------------------------------------------------------
 * The products above for a handle restricted to the steps [sb, se) = [step_begin, step_end) of its ctd_desc (handles of
 * ctd_sharded_handle included), modelled on ctd_grad_shard_dev_async: enqueue-only on the handle's stream, capturable after one
 * warm call, reproducible bit for bit; run-time OCPs compile the shard form of their product kernels at the first shard call (a
 * family of its own: the whole-grid calls compile nothing more than before).  Every buffer is full-length with global indexing
 * (nvar or ncon entries).  "First" shard: sb == 0; "last" shard: se == N.  blk: variables per step block, cb: rows per step,
 * eqs: state + stage rows per step, p: path rows per node, v_off = nvar - nv.
 * WRITES -- nothing else of the output is touched:
 *   jprod   the rows [sb cb, se cb); the last shard also the tail rows [N cb, ncon) (final path rows and boundary rows): the row
 *           ownership of ctd_stitch_c;
 *   jtprod, hprod   the variable entries [sb blk, se blk), the last shard up to v_off (node N included), and the nv entries
 *           [v_off, nvar) with the shard's PARTIAL sums of d/dv: the caller adds them over the shards (one all-reduce of nv
 *           doubles).  The boundary rows' and the Mayer term's contributions go to X_1 on the first shard, to X_{N+1} and to v on
 *           the last one (the convention of ctd_grad_shard_dev_async).
 *   kktprod rx: the entries of jtprod / hprod above, the nv entries again the shard's PARTIAL sums, which the caller adds over the
 *           shards (one all-reduce of nv doubles); sx o dx of the v entries is in the last shard's partial sum only.  rc: the rows
 *           of jprod above.
 * On a whole-grid handle each call is bit-identical to its *_dev_async counterpart (kktprod: the v entries included).
 * READS of x: through the table of ctd_set_x_shards when one is set (the call contains no exchange); otherwise from x_dev, whose
 * halo entries must have been copied in.  The directions v, w and y (kktprod: dx, dy, y, sx and sc) are ALWAYS read from the
 * pointer passed: their halo entries are the caller's to fill (as for y of the sharded ctd_hess_coord).  Upper bounds of what a
 * call reads -- nothing outside them is read, so those entries need not be valid:
 *   variable layout (x without a table, v; kktprod: dx):  the shard's own entries (as in the write set above); [v_off, nvar); the
 *     whole block sb - 1 if sb > 0; if se < N the first n entries of block se, plus the m controls behind them on the trapeze;
 *     [0, n) and [N blk, N blk + n);
 *   constraint layout (w, y; kktprod: dy):  the shard's own rows (the tail included on the last shard); the eqs state / stage rows
 *     of step sb - 1 if sb > 0; the p path rows of node se, [se cb + eqs, (se + 1) cb), if se < N; the tail [N cb, ncon);
 *   the diagonals of kktprod:  sx the shard's own variable entries, on the last shard also [v_off, nvar); sc the shard's own rows.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE; null pointers (y_dev may be NULL: objective
 * only) -> CTD_EINVAL; an output that equals an input -> CTD_EINVAL. */
int32_t ctd_jprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* v_dev, double* Jv_dev);
int32_t ctd_jtprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* w_dev, double* Jtw_dev);
int32_t ctd_hprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* v_dev,
                                  double* Hv_dev);
/* ctd_kktprod_dev_async on a shard: the same arguments with the same meaning (y_dev, sx_dev, sc_dev may be NULL), two launches, the
 * partial-sum buffer of ctd_kktprod* (not hprod's or jtprod's).  A Krylov iteration of a sharded solver costs these two launches, one exchange of the halos of
 * (dx, dy) and one all-reduce of nv doubles; x (read in place or with its halo copied once) and y (its halo rows copied once) do not
 * change over the inner iterations of one outer step.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE; null x, dx, dy, rx or rc -> CTD_EINVAL; an
 * output equal to any input, or rx == rc -> CTD_EINVAL. */
int32_t ctd_kktprod_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, const double* dx_dev,
                                    const double* dy_dev, const double* sx_dev, const double* sc_dev, double* rx_dev, double* rc_dev);
/* ctd_hdiag_dev_async, ctd_jsq_rows_dev_async and ctd_jsq_cols_dev_async on a shard: the same arguments with the same meaning
 * (y_dev NULL: objective only; NULL weights: ones, bit-identical to a vector of ones), the same launches (two, two, one) and the
 * partial-sum buffers of ctd_hdiag* and ctd_jsq_cols*; run-time OCPs compile one more family at the first of these three calls.
 * WRITES -- nothing else of the output is touched:
 *   hdiag, jsq_cols   the write set of jtprod / hprod above: the shard's own variable entries, the last shard up to v_off, and
 *           [v_off, nvar) with the shard's PARTIAL sums, which the caller adds over the shards (one all-reduce of nv doubles).  The
 *           boundary rows' (hdiag: and the Mayer term's) contributions go to X_1 on the first shard, to X_{N+1} and to v on the last.
 *   jsq_rows   the write set of jprod above: the rows [sb cb, se cb), on the last shard also the tail [N cb, ncon).  Every row sum is
 *           complete: no reduction over the shards.
 * On a whole-grid handle each call is bit-identical to its *_dev_async counterpart, the v entries included.
 * READS: x as above (through the table when one is set, else from x_dev with its halo copied in); y (hdiag) and wc (jsq_cols) the
 * constraint-layout read set above, wx (jsq_rows) the variable-layout read set above, always from the pointer passed.
 * A scaling preconditioner of ctd_kktprod_shard_dev_async per outer iteration: hdiag, an all-reduce of the nv partial sums (the last
 * shard adds the tail of sx first), px = |Hd + sx|, an exchange of the halo of wx = 1 / px, jsq_rows, pc = out + sc on the own rows.
 * Checks in this order: NULL handle -> CTD_EINVAL; host-only handle -> CTD_ENODEVICE, whatever the other arguments; null x or
 * output -> CTD_EINVAL; an output equal to an input -> CTD_EINVAL.  Every handle is accepted, shard or whole grid. */
int32_t ctd_hdiag_shard_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* Hd_dev);
int32_t ctd_jsq_rows_shard_dev_async(ctd_handle* h, const double* x_dev, const double* wx_dev, double* out_dev);
int32_t ctd_jsq_cols_shard_dev_async(ctd_handle* h, const double* x_dev, const double* wc_dev, double* out_dev);

/* 1-based (rows[k], cols[k]), k < nnzh, CSC order */
int32_t ctd_hess_structure(const ctd_handle* h, int64_t* rows, int64_t* cols);
/* same pattern as 0-based CSC (colptr[nvar + 1], rowval[nnzh]) */
int32_t ctd_hess_csc(const ctd_handle* h, int64_t* colptr, int64_t* rowval);
/* The Hessian values in CSR: the Hessian is symmetric, so the value array of ctd_hess_coord* (lower triangle by columns) IS the CSR value
 * array of the UPPER triangle (row j of the upper triangle = column j of the lower one).  rowptr[nvar + 1], colind[nnzh], 0-based,
 * colind >= row: hand them with the values to a CSR consumer as a symmetric matrix stored by its upper triangle
 * (rocsparse_fill_mode_upper).  No second value order is needed for the Hessian -- nothing is permuted, no extra bytes move. */
int32_t ctd_hess_csr(const ctd_handle* h, int64_t* rowptr, int64_t* colind);
/* host pointers: x[nvar], y[ncon] (constraint multipliers), vals[nnzh]; includes the PCIe copies */
int32_t ctd_hess_coord(ctd_handle* h, const double* x, const double* y, double obj_weight, double* vals);
/* device pointers on the handle's device; the first returns after the handle's stream has drained, the second only
 * enqueues (ctd_sync waits) */
int32_t ctd_hess_coord_dev(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev);
int32_t ctd_hess_coord_dev_async(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev);
/* measurement: mean duration (ms) of the Hessian kernel over `iters` launches, per-dispatch events on the handle's stream */
int32_t ctd_time_hess_dev(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev,
                          int32_t iters, double* mean_ms);
/* launch geometry of the Hessian kernel: out[0..9] = grid blocks, block threads, dynamic LDS bytes, steps per tile,
 * CSC period of the lower triangle (entries per regular step), number of edge entries, second-order eval lanes per
 * stage point / path point / boundary point (after the structural-sparsity probe), terms of the periodic segment */
int32_t ctd_hess_launch_info(ctd_handle* h, int64_t* out10);
/* Which kernel ctd_hess_coord* launches for the regular steps of this handle: out[0] = 0 tile kernel (every scheme), 1 lane-per-step
 * kernel (Gauss-Legendre schemes with 2 / 3 stages of the light registry OCPs on large grids); out[1] = its grid. */
int32_t ctd_hess_kernel_info(ctd_handle* h, int64_t* out2);
/* out[0..3 + nvv): vals_main_begin, vals_main_end (0-based contiguous range of the shard's step columns in the CSC value
 * array), nvv = nv (nv+1)/2, then the 0-based positions of the variable x variable entries (partial sums on a shard) */
int32_t ctd_hess_shard_info(const ctd_handle* h, int64_t* out13);
/* Diagnostics: one launch of the Hessian kernel with in-kernel phase stamps: per workgroup 5 pairs {100 MHz realtime
 * counter, shader cycle counter} at start, after load, after eval, after emit issue, after the stores drained.
 * cap = capacity of out in uint64 words (needs grid * 10). */
int32_t ctd_hess_debug_stamps(ctd_handle* h, const double* x_dev, const double* y_dev, double obj_weight, double* vals_dev,
                              uint64_t* out, int64_t cap);


/* ---- one transcription on several GPUs of ONE process (SURVEY.md section 8b "device list", 8e) ------------------------------
 * The reference has no counterpart (it is single-threaded): this serves a Julia host that owns all GPUs of a node from one
 * process -- the same `ccall` shim, one multi-device handle instead of one handle.  The N time steps are split into
 * n_devices contiguous blocks (block k = steps [k N / n, (k+1) N / n), the ceil / floor rule of a balanced split; the loop
 * being partitioned is src/DOCP_functions.jl:92-98); shard k lives on devices[k] with a stream of its own.  Buffers are
 * FULL-LENGTH on every device (global indexing): x_dev[k] (nvar), c_dev[k] (ncon), vals_dev[k] (nnzj) are device pointers on
 * devices[k]; shard k writes its rows of c, its contiguous CSC range and its slices of the V columns
 * (ctd_sharded_shard_info).  The same device may appear several times (tests on a one-GPU box).  Exchanges between the
 * devices are peer-to-peer copies over xGMI (hipMemcpyPeerAsync on the shards' streams, ordered by events); a failure of one
 * of them is reported as CTD_ERCCL.
 * Single-iterate only: the batched callbacks (ctd_*_batch_dev_async) are out of scope for sharded evaluation -- they refuse a
 * shard handle. */
typedef struct ctd_sharded ctd_sharded;

enum {
    CTD_X_IN_PLACE = 0,      /* every x_dev[k] already holds what shard k reads (e.g. the solver replicates x)               */
    CTD_X_SHARDED = 1,       /* x_dev[k] holds shard k's own variables (+ the replicated v).  The few entries a shard needs    */
                             /*   from its neighbours -- next shard's first node, previous shard's last block (midpoint /      */
                             /*   Euler), X_1, X_{N+1} -- are COPIED into x_dev[k] (hipMemcpyPeerAsync on the shards' streams, */
                             /*   ordered by events: a shard's buffer is read behind the work already queued on ITS stream);   */
                             /*   afterwards every callback of shard k's handle can run on x_dev[k].  Works on any topology    */
                             /*   (without peer access the copies go through the host).  The meaning this value has had since  */
                             /*   round 2; round 3 had given it to the in-place mode below                                      */
    CTD_X_FROM_DEVICE0 = 2,  /* x_dev[0] holds the whole iterate: the engine copies all of it to the other devices          */
    CTD_X_SHARDED_COPY = 3,  /* = CTD_X_SHARDED (kept for callers of round 3)                                                 */
    CTD_X_SHARDED_IN_PLACE = 4 /* as CTD_X_SHARDED, but nothing is copied: the kernels LOAD those entries in place from the   */
                             /*   owner's buffer through the peer mappings (xGMI; ctd_set_x_shards).  Ordering: every shard's  */
                             /*   stream records an event, the shards that read its buffer wait for it -- so work the caller   */
                             /*   queued on x_dev[k]'s device stream (ctd_set_stream) before this call is ordered before the   */
                             /*   neighbours' reads; writes from anywhere else must be complete.  The other callbacks of a     */
                             /*   shard handle then read the neighbours' entries through the same table (objective, Hessian)   */
                             /*   -- except ctd_grad*, which needs a whole iterate.  Needs peer access between the devices of  */
                             /*   neighbouring shards, of the first and of the last shard (recorded by ctd_create_sharded): a  */
                             /*   pair without it makes the call take the CTD_X_SHARDED protocol instead of faulting inside    */
                             /*   the kernel, and ctd_sharded_last_error names the pair                                         */
};

/* desc->device, step_begin / step_end and stream are ignored (must be 0 / NULL); devices[k] are HIP ordinals */
int32_t ctd_create_sharded(const ctd_desc* desc, const int32_t* devices, int32_t n_devices, ctd_sharded** out);
int32_t ctd_sharded_destroy(ctd_sharded* s);
const char* ctd_sharded_last_error(const ctd_sharded* s);
/* the k-th shard's single-device handle (owned by s): sizes, patterns, bounds, ctd_shard_info, ctd_set_stream, and every
 * single-device callback (objective, gradient, Hessian) on that shard */
int32_t ctd_sharded_handle(ctd_sharded* s, int32_t k, ctd_handle** h);
/* out[0..9] = n_devices, devices[k], then ctd_shard_info(shard k)[0..7] */
int32_t ctd_sharded_shard_info(const ctd_sharded* s, int32_t k, int64_t* out10);
/* Enqueue one fused evaluation on every device: [iterate distribution per x_mode] -> shard kernels -> [stitch != 0: every
 * device receives the other shards' row blocks of c (the p + bc tail rows from the last shard), so each c_dev[k] ends up
 * whole].  Nothing waits on the host.  The
 * caller's writes to x_dev must be complete (or ordered before the shards' streams) when this is called. */
int32_t ctd_cons_jac_sharded_dev_async(ctd_sharded* s, double* const* x_dev, double* const* c_dev, double* const* vals_dev,
                                       int32_t x_mode, int32_t stitch);
/* ---- sharded iterate read in place ------------------------------------------------------------------------------------------
 * One shard handle (ctd_desc.step_begin / step_end) usually finds everything it reads in the x passed to the call.  With the
 * iterate sharded like the steps (a shard holds its own steps' variables and the replicated v in a
 * full-length buffer) a few entries belong to other shards: the next shard's first node, the previous shard's last step block
 * (one-point schemes), X_1 and X_{N+1} (boundary rows).  After ctd_set_x_shards the constraint / Jacobian, objective and Hessian kernels of `h` load
 * those entries straight from x_bufs[k], the full-length buffer of shard k = steps [step_begin[k], step_begin[k+1]) -- a
 * peer-mapped pointer of another device of this process, or the mapping of another process' buffer (ctd_ipc_open below) --
 * so the evaluation of a shard contains no exchange step at all: the loop being split is src/DOCP_functions.jl:92-98, and
 * step i reads only X_i, U_i, K_i, X_{i+1}, v.  `self` = this handle's shard (x_bufs[self] is ignored: its x is the call's
 * argument); n_shards <= 16; n_shards = 0 switches back.  The writers' updates of x must be complete (or ordered before this
 * handle's stream) when an evaluation is enqueued -- the acceptance test of a solver iteration is a collective already.
 * The objective (src/DOCP_functions.jl:23-54: its quadrature over the shard's steps, the Mayer term on the last shard) and the
 * Hessian callbacks (ctd_hess_coord*, ctd_eval_all_dev_async; the multipliers y are replicated) follow the same table since
 * round 3.  ctd_grad* is the gradient of the WHOLE objective on every rank (see there) and ignores the table: it reads only the
 * x it is given, which must then hold every variable (an all-gathered copy); ctd_grad_shard_dev_async (round 4) is the sharded
 * form that follows the table. */
int32_t ctd_set_x_shards(ctd_handle* h, int32_t n_shards, const int64_t* step_begin, const double* const* x_bufs, int32_t self);
/* One process per GPU (e.g. a Julia host under MPI): the "RCCL all-gather over xGMI for the stitched constraint vector" of the
 * north star, inside the library.  comm is an ncclComm_t of n_ranks ranks created by the host with ITS copy of librccl (found
 * with dlopen at first use; no link-time dependency; CTD_RCCL_LIB overrides); rank r evaluates block r of the balanced split
 * (ctd_shard_steps gives the [begin, end) to put into ctd_desc).  c_dev is the full-length constraint vector in which this
 * rank's rows are already written (ctd_cons_jac_dev_async); on return of the stream every rank holds all N cb step rows, and the
 * p + bc tail rows as computed by the LAST rank.  Equal blocks without tail rows: ONE in-place ncclAllGather; otherwise padded
 * blocks + one index kernel.  Enqueue-only on the handle's stream.  A failing collective returns CTD_ERCCL. */
int32_t ctd_stitch_c(ctd_handle* h, void* nccl_comm, int32_t n_ranks, int32_t rank, double* c_dev);
/* block k of the balanced split of N steps over n_shards (the first N % n_shards blocks hold one step more) */
int32_t ctd_shard_steps(int64_t N, int32_t n_shards, int32_t k, int64_t* begin, int64_t* end);

/* One process per GPU: export a device buffer (any pointer inside a hipMalloc'ed allocation, e.g. a tensor of a caching
 * allocator: `handle64` names the allocation, `offset` the pointer's byte offset in it) and map it in another process of the
 * node (ctd_ipc_open returns the allocation's base in this process; add the offset).  hipIpcGetMemHandle / hipIpcOpenMemHandle. */
#define CTD_IPC_HANDLE_BYTES 64
int32_t ctd_ipc_export(int32_t device, const void* dev_ptr, void* handle64, int64_t* offset);
int32_t ctd_ipc_open(int32_t device, const void* handle64, void** base);
int32_t ctd_ipc_close(int32_t device, void* base);
/* reads `bytes` (<= 64) at a mapped pointer with a device-to-device copy: CTD_ERCCL if `device` cannot reach it (an error code
 * here instead of a fault inside a kernel); hosts call it once per mapping before ctd_set_x_shards */
int32_t ctd_ipc_probe(int32_t device, const void* ptr, size_t bytes);

/* waits for every shard's stream */
int32_t ctd_sharded_sync(ctd_sharded* s);
/* Device memory for hosts without a HIP binding of their own (examples/cabi_demo.c; a Julia host passes AMDGPU.jl arrays
 * instead): hipMalloc / hipFree / hipMemcpy on the given device.  kind: 0 = host -> device, 1 = device -> host. */
int32_t ctd_dev_alloc(int32_t device, size_t bytes, void** ptr);
int32_t ctd_dev_free(int32_t device, void* ptr);
int32_t ctd_dev_copy(int32_t device, void* dst, const void* src, size_t bytes, int32_t kind);

#ifdef __cplusplus
}
#endif
#endif /* CTDIRECT_HIP_H */
