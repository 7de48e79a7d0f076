"""ctypes binding of libctdirect_hip.so -- the C ABI declared in include/ctdirect_hip.h.

The library is the product: if it is missing or fails to load, importing the engine fails loudly.  There is no
Python / NumPy / PyTorch compute fallback anywhere in this package.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTD_LIB_PATH") or os.path.join(_HERE, "libctdirect_hip.so")      # (override: A/B runs of experiment builds)
CSRC = os.path.join(_HERE, "csrc")

# status codes (include/ctdirect_hip.h)
CTD_OK, CTD_EINVAL, CTD_EGRID, CTD_ESCHEME, CTD_EPATTERN, CTD_EPROBLEM, CTD_ENODEVICE, CTD_EHIP, CTD_ENOMEM, CTD_ERCCL = range(10)


class ctd_desc(C.Structure):
    _fields_ = [("problem", C.c_int32), ("scheme", C.c_int32), ("pattern_mode", C.c_int32), ("device", C.c_int32),
                ("grid_size", C.c_int64), ("time_grid", C.POINTER(C.c_double)), ("time_grid_len", C.c_int64),
                ("step_begin", C.c_int64), ("step_end", C.c_int64), ("stream", C.c_void_p),
                ("stream_mode", C.c_int32), ("control_steps", C.c_int32), ("value_order", C.c_int32), ("reserved0", C.c_int32)]


class ctd_init(C.Structure):
    _fields_ = [("use_problem_default", C.c_int32), ("state", C.POINTER(C.c_double)),
                ("control", C.POINTER(C.c_double)), ("variable", C.POINTER(C.c_double)),
                ("n_samples", C.c_int64), ("t_samples", C.POINTER(C.c_double)),
                ("state_samples", C.POINTER(C.c_double)), ("control_samples", C.POINTER(C.c_double))]


class ctd_ocp_def(C.Structure):
    _fields_ = [("name", C.c_char_p), ("n", C.c_int32), ("m", C.c_int32), ("nv", C.c_int32), ("npath", C.c_int32),
                ("nbc", C.c_int32), ("it0", C.c_int32), ("itf", C.c_int32), ("t0", C.c_double), ("tf", C.c_double),
                ("maximize", C.c_int32), ("reserved", C.c_int32), ("dynamics", C.POINTER(C.c_char_p)),
                ("lagrange", C.c_char_p), ("mayer", C.c_char_p), ("path", C.POINTER(C.c_char_p)),
                ("boundary", C.POINTER(C.c_char_p)), ("constants", C.c_char_p)] + \
               [(k, C.POINTER(C.c_double)) for k in ("state_lb", "state_ub", "control_lb", "control_ub", "variable_lb",
                                                     "variable_ub", "path_lb", "path_ub", "boundary_lb", "boundary_ub")]


# status of the device-resident MINRES solve (ctd_minres_info.status), by CTD_MINRES_* value
MINRES_STATUS = ("running", "converged", "max_iter", "breakdown")


class ctd_kkt_system(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("x", C.c_void_p), ("y", C.c_void_p),
                ("obj_weight", C.c_double), ("sx", C.c_void_p), ("sc", C.c_void_p), ("px", C.c_void_p), ("pc", C.c_void_p)]


class ctd_minres_info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("status", C.c_int32), ("iterations", C.c_int64), ("phibar", C.c_double),
                ("Anorm", C.c_double), ("ynorm", C.c_double), ("beta1", C.c_double)]


# CTD_KKT_MINRES_SHARD_SLOT and the layout query of the shard form of the solve (ctd_kkt_minres_shard_layout)
KKT_MINRES_SHARD_SLOT = 2080


class ctd_minres_shard_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(nm, C.c_int64) for nm in (
        "n", "n_ranks", "var_begin", "var_end", "tail_begin", "tail_end", "row_begin", "row_end", "n_own", "n_dot", "nwg", "chunk",
        "slot", "off_v", "off_kv", "off_send_a", "off_send_b", "off_gathered_a", "off_gathered_b", "off_state", "workspace")]


# the layout of the chunked block-tridiagonal Schur preconditioner (ctd_kkt_schur_layout); CTD_KKT_SCHUR_FIXED
KKT_SCHUR_FIXED = 512


class ctd_schur_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(nm, C.c_int64) for nm in (
        "N", "block_rows", "tail_rows", "first_tail_row", "tail_cols", "n_chunks", "chunk_steps", "workspace")]


# ... and of its log-depth exact form (ctd_kkt_schur_cr_layout)
class ctd_schur_cr_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(nm, C.c_int64) for nm in (
        "N", "block_rows", "tail_rows", "first_tail_row", "tail_cols", "n_levels", "factor_launches", "solve_launches", "workspace")]


# the shard form of that (ctd_kkt_schur_cr_shard_layout): the rank's blocks and the read set of its factor
class ctd_schur_cr_shard_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(nm, C.c_int64) for nm in (
        "N", "step_begin", "step_end", "n_blocks", "block_rows", "first_row", "tail_rows", "first_tail_row", "tail_cols", "n_levels",
        "factor_launches", "solve_launches", "workspace", "jvals_begin", "jvals_end", "px_begin", "px_end")]


# the joined form (ctd_kkt_schur_cr_joint_layout): separator, interior, launch counts, record slots, workspace offsets, read set
class ctd_schur_cr_joint_layout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(nm, C.c_int64) for nm in (
        "N", "n_ranks", "rank", "step_begin", "step_end", "separator", "int_begin", "n_int", "block_rows", "first_row", "tail_rows",
        "first_tail_row", "tail_cols", "n_levels", "n_sep", "factor_local_launches", "factor_join_launches", "solve_local_launches",
        "solve_join_launches", "factor_slot", "solve_slot", "off_es", "off_eb", "off_ds", "off_wl", "off_wr", "off_scratch", "off_reduced",
        "off_rs", "off_xs", "off_sigma", "workspace", "jvals_begin", "jvals_end", "jvals_halo_begin", "jvals_halo_end", "px_begin",
        "px_end")]


# CTD_KKT_MINRES_SCHUR_JOINT_SLOT: the slot of the sharded solve that carries the joined form
KKT_MINRES_SCHUR_JOINT_SLOT = KKT_MINRES_SHARD_SLOT + 256 + 16 + 3 * 64 + 16

# CTD_KKT_SCHUR_CR_JOINT_MAX_RANKS, CTD_KKT_SCHUR_CR_JOINT_SOLVE_SLOT
KKT_SCHUR_CR_JOINT_MAX_RANKS = 256
KKT_SCHUR_CR_JOINT_SOLVE_SLOT = 16 + 3 * 64


def kkt_schur_cr_joint_factor_slot(m):
    """CTD_KKT_SCHUR_CR_JOINT_FACTOR_SLOT(m)"""
    return 16 + 4 * m * m


# CTD_KKT_MINRES_SCHUR_SHARD_SLOT: the slot of the sharded solve that carries it
KKT_MINRES_SCHUR_SHARD_SLOT = KKT_MINRES_SHARD_SLOT + 256 + 16


def kkt_schur_cr_workspace(N, m):
    """CTD_KKT_SCHUR_CR_WORKSPACE(N, m)"""
    return KKT_SCHUR_FIXED + N + 3 * N * m * m + 2 * N * m


# every symbol include/ctdirect_hip.h declares: name -> (restype, argtypes)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_vp = C.c_void_p
SYMBOLS = {
    "ctd_create": (C.c_int32, [C.POINTER(ctd_desc), C.POINTER(_vp)]),
    "ctd_destroy": (C.c_int32, [_vp]),
    "ctd_last_error": (C.c_char_p, [_vp]),
    "ctd_strerror": (C.c_char_p, [C.c_int32]),
    "ctd_host_alloc": (C.c_int32, [C.POINTER(C.c_void_p), C.c_size_t]),
    "ctd_host_free": (C.c_int32, [C.c_void_p]),
    "ctd_sizes": (C.c_int32, [_vp, _ip, _ip, _ip, _ip]),
    "ctd_dims": (C.c_int32, [_vp, _ip]),
    "ctd_time_grid": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_time_grid_at": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_butcher": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_bounds": (C.c_int32, [_vp, _dp, _dp, _dp, _dp]),
    "ctd_initial_guess": (C.c_int32, [_vp, _dp, C.POINTER(ctd_init)]),
    "ctd_jac_structure": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_jac_csc": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_jac_csr": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_value_order": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "ctd_dropped_nonzeros": (C.c_int32, [_vp, _ip]),
    "ctd_obj": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_grad": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_grad_dev": (C.c_int32, [_vp, _vp, _vp]),
    "ctd_cons": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_jac_coord": (C.c_int32, [_vp, _dp, _dp]),
    "ctd_cons_jac": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_cons_jac_dev": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_cons_jac_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_obj_dev": (C.c_int32, [_vp, _vp, _dp]),
    "ctd_obj_dev_async": (C.c_int32, [_vp, _vp, _vp]),
    "ctd_grad_dev_async": (C.c_int32, [_vp, _vp, _vp]),
    "ctd_grad_shard_dev_async": (C.c_int32, [_vp, _vp, _vp]),
    "ctd_sync": (C.c_int32, [_vp]),
    "ctd_set_stream": (C.c_int32, [_vp, _vp]),
    "ctd_shard_info": (C.c_int32, [_vp, _ip]),
    "ctd_time_cons_jac_dev": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, _dp]),
    "ctd_launch_info": (C.c_int32, [_vp, _ip]),
    "ctd_debug_stamps": (C.c_int32, [_vp, _vp, _vp, _vp, C.POINTER(C.c_uint64), C.c_int64]),
    "ctd_register_ocp": (C.c_int32, [C.POINTER(ctd_ocp_def), C.POINTER(C.c_int32)]),
    "ctd_ocp_source": (C.c_int32, [C.c_int32, C.c_char_p, C.c_int64]),
    "ctd_jit_check": (C.c_int32, [C.c_int32, C.c_int32]),
    "ctd_hess_structure": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_hess_csc": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_hess_csr": (C.c_int32, [_vp, _ip, _ip]),
    "ctd_hess_coord": (C.c_int32, [_vp, _dp, _dp, C.c_double, _dp]),
    "ctd_hess_coord_dev": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp]),
    "ctd_hess_coord_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp]),
    "ctd_time_hess_dev": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, C.c_int32, _dp]),
    "ctd_hess_launch_info": (C.c_int32, [_vp, _ip]),
    "ctd_hess_kernel_info": (C.c_int32, [_vp, _ip]),
    "ctd_hess_shard_info": (C.c_int32, [_vp, _ip]),
    "ctd_hess_debug_stamps": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, C.POINTER(C.c_uint64), C.c_int64]),
    "ctd_eval_all_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    # batched callbacks: K iterates of one transcription per launch (member b at x + b ldx, ...)
    "ctd_cons_jac_batch_dev_async": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "ctd_obj_batch_dev_async": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _vp]),
    "ctd_grad_batch_dev_async": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64]),
    "ctd_jprod": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_jtprod": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_jprod_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_jtprod_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_hprod": (C.c_int32, [_vp, _dp, _dp, C.c_double, _dp, _dp]),
    "ctd_hprod_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, _vp]),
    "ctd_kktprod": (C.c_int32, [_vp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ctd_kktprod_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    # matrix-free KKT diagonals: diag(H), row sums and column sums of J o J
    "ctd_hdiag": (C.c_int32, [_vp, _dp, _dp, C.c_double, _dp]),
    "ctd_hdiag_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp]),
    "ctd_jsq_rows": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_jsq_rows_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_jsq_cols": (C.c_int32, [_vp, _dp, _dp, _dp]),
    "ctd_jsq_cols_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    # device-resident preconditioned MINRES solve of the KKT system
    "ctd_kkt_minres_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, C.c_double]),
    "ctd_kkt_minres_iters_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, C.c_int64]),
    "ctd_kkt_minres_info": (C.c_int32, [_vp, C.POINTER(ctd_minres_info)]),
    "ctd_kkt_minres_dev": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, C.c_double, C.c_int64, C.c_int64,
                                       C.POINTER(ctd_minres_info)]),
    "ctd_kkt_minres": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _dp, _dp, C.c_double, C.c_int64, C.c_int64,
                                   C.POINTER(ctd_minres_info)]),
    # chunked block-tridiagonal Schur preconditioner: layout, factor, solve, status, and the solve that carries it
    "ctd_kkt_schur_layout": (C.c_int32, [_vp, C.c_int64, C.POINTER(ctd_schur_layout)]),
    "ctd_kkt_schur_factor_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "ctd_kkt_schur_solve_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_kkt_schur_info": (C.c_int32, [_vp, _vp, _ip]),
    "ctd_kkt_minres_schur_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, C.c_double]),
    "ctd_kkt_minres_schur_dev": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, C.c_double, C.c_int64, C.c_int64,
                                             C.POINTER(ctd_minres_info)]),
    # log-depth exact block-tridiagonal Schur preconditioner (block cyclic reduction): the same family without a chunk length
    "ctd_kkt_schur_cr_layout": (C.c_int32, [_vp, C.POINTER(ctd_schur_cr_layout)]),
    "ctd_kkt_schur_cr_factor_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, _vp]),
    "ctd_kkt_schur_cr_solve_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_kkt_schur_cr_info": (C.c_int32, [_vp, _vp, _ip]),
    "ctd_kkt_minres_schur_cr_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, C.c_double]),
    "ctd_kkt_minres_schur_cr_dev": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, C.c_double, C.c_int64, C.c_int64,
                                                C.POINTER(ctd_minres_info)]),
    # ... and the shard form of the solve: the phases between the caller's all-gathers
    "ctd_kkt_minres_shard_layout": (C.c_int32, [_vp, C.c_int32, C.POINTER(ctd_minres_shard_layout)]),
    "ctd_kkt_minres_shard_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double,
                                                         C.c_int64]),
    "ctd_kkt_minres_shard_begin_dev_async": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_shard_alfa_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_shard_lanczos_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_shard_update_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_shard_info": (C.c_int32, [_vp, _vp, C.c_int32, C.POINTER(ctd_minres_info)]),
    # the shard form of the log-depth Schur preconditioner, and the phases of the sharded solve that carries it
    "ctd_kkt_schur_cr_shard_layout": (C.c_int32, [_vp, C.POINTER(ctd_schur_cr_shard_layout)]),
    "ctd_kkt_schur_cr_shard_factor_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, _vp]),
    "ctd_kkt_schur_cr_shard_solve_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_kkt_schur_cr_shard_info": (C.c_int32, [_vp, _vp, _ip]),
    "ctd_kkt_minres_schur_cr_shard_layout": (C.c_int32, [_vp, C.c_int32, C.POINTER(ctd_minres_shard_layout)]),
    "ctd_kkt_minres_schur_cr_shard_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, _vp, C.c_int32, C.c_int32,
                                                                  C.c_double, C.c_int64]),
    "ctd_kkt_minres_schur_cr_shard_begin_dev_async": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_shard_alfa_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_shard_lanczos_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_shard_update_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_shard_info": (C.c_int32, [_vp, _vp, C.c_int32, C.POINTER(ctd_minres_info)]),
    # the joined form of the log-depth Schur preconditioner: local phases and joins around the caller's all-gathers
    "ctd_kkt_schur_cr_joint_layout": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.POINTER(ctd_schur_cr_joint_layout)]),
    "ctd_kkt_schur_cr_joint_factor_local_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_schur_cr_joint_factor_join_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_schur_cr_joint_solve_local_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_schur_cr_joint_solve_join_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_schur_cr_joint_info": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _ip]),
    "ctd_kkt_minres_schur_cr_joint_layout": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.POINTER(ctd_minres_shard_layout)]),
    "ctd_kkt_minres_schur_cr_joint_start_dev_async": (C.c_int32, [_vp, C.POINTER(ctd_kkt_system), _vp, _vp, _vp, _vp, C.c_int32, C.c_int32,
                                                                  C.c_double, C.c_int64]),
    "ctd_kkt_minres_schur_cr_joint_begin_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_joint_alfa_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_joint_lanczos_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_joint_update_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32]),
    "ctd_kkt_minres_schur_cr_joint_info": (C.c_int32, [_vp, _vp, C.c_int32, C.POINTER(ctd_minres_info)]),
    "ctd_jprod_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_jtprod_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_hprod_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, _vp]),
    "ctd_kktprod_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctd_hdiag_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, C.c_double, _vp]),
    "ctd_jsq_rows_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_jsq_cols_shard_dev_async": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "ctd_hess_coord_batch_dev_async": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64, C.c_double, _vp, C.c_int64]),
    # one transcription on several GPUs of one process
    "ctd_create_sharded": (C.c_int32, [C.POINTER(ctd_desc), C.POINTER(C.c_int32), C.c_int32, C.POINTER(_vp)]),
    "ctd_sharded_destroy": (C.c_int32, [_vp]),
    "ctd_sharded_last_error": (C.c_char_p, [_vp]),
    "ctd_sharded_handle": (C.c_int32, [_vp, C.c_int32, C.POINTER(_vp)]),
    "ctd_sharded_shard_info": (C.c_int32, [_vp, C.c_int32, _ip]),
    "ctd_cons_jac_sharded_dev_async": (C.c_int32, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.c_int32, C.c_int32]),
    "ctd_sharded_sync": (C.c_int32, [_vp]),
    "ctd_dev_alloc": (C.c_int32, [C.c_int32, C.c_size_t, C.POINTER(_vp)]),
    "ctd_dev_free": (C.c_int32, [C.c_int32, _vp]),
    "ctd_dev_copy": (C.c_int32, [C.c_int32, _vp, _vp, C.c_size_t, C.c_int32]),
    # sharded iterate read in place + buffers shared between the processes of a node
    "ctd_set_x_shards": (C.c_int32, [_vp, C.c_int32, _ip, C.POINTER(_vp), C.c_int32]),
    "ctd_ipc_export": (C.c_int32, [C.c_int32, _vp, _vp, _ip]),
    "ctd_ipc_open": (C.c_int32, [C.c_int32, _vp, C.POINTER(_vp)]),
    "ctd_ipc_close": (C.c_int32, [C.c_int32, _vp]),
    "ctd_ipc_probe": (C.c_int32, [C.c_int32, _vp, C.c_size_t]),
    "ctd_stitch_c": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp]),
    "ctd_shard_steps": (C.c_int32, [C.c_int64, C.c_int32, C.c_int32, _ip, _ip]),
}


def build(jobs=8):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC, "-s", f"-j{jobs}"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built (run `python -c 'import "
                "__graft_entry__ as g; g.build()'` or `make -C ctdirect.jl_amd/csrc`). There is no fallback path.")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same soname as /opt/rocm's).  If torch is
        # going to be used in this process it must be loaded first so that this library binds to the same runtime
        # (two runtimes in one process do not see each other's devices, streams or allocations).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("CTD_LIB_PATH") and not hasattr(L, name):
                continue                  # (A/B runs against an older experiment build: it may lack the newest entry points)
            f = getattr(L, name)          # AttributeError if the library does not export the symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib
