"""ctypes binding of libfoship.so (include/foship.h).  No fallback: a missing library is an ImportError-class failure."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["FOSHIP_LIB"]) if os.environ.get("FOSHIP_LIB") else _HERE / "csrc" / "libfoship.so"      # (FOSHIP_LIB: as in julia/FOSHip.jl)

# error codes / enums (mirror of include/foship.h)
FOS_OK = 0
CONE_CODES = {"Free": 0, "Zero": 1, "NonNeg": 2, "NonPos": 3, "SOC": 4, "SOCRotated": 5, "SDP": 6,
              "ExpPrimal": 7, "ExpDual": 8}
SET_CODES = {"IndFree": 0, "IndBallL2": 1, "IndBallL1": 2, "IndSimplex": 3, "IndHalfspace": 4, "IndHyperslab": 5, "IndPoint": 6, "IndBox": 7}      # FOS_SET_*
FN_CODES = {"NormL1": 32, "SqrNormL2": 33, "ElasticNet": 34, "Linear": 35, "NormL2": 36, "HuberLoss": 37, "NormLinf": 38}      # FOS_FN_*: further kinds of fos_feas_set_blocks
# FOS_FN_BLK_QUADRATIC, FOS_SET_BLK_AFFINE, FOS_FN_BLK_LEAST_SQUARES: the dense blocks of fos_feas_set_blocks2, by the class whose block they are (a table of
# its own: tests pin SET_CODES and FN_CODES to the vector kinds)
BLK_CODES = {"Quadratic": 48, "IndAffine": 49, "LeastSquares": 50}
LS_FORM_CODES = {"sparse_factored": 0, "normal": 1}      # FOS_LS_FORM_*
ALG_GAP, ALG_GAPA, ALG_FISTA, ALG_DYKSTRA = 0, 1, 2, 3
CG_REFERENCE, CG_FUSED_P, CG_MERGED_SWEEP, CG_MERGED_UPDATE, CG_RESIDENT = 0, 1, 2, 3, 4
DEBUG_PUPDATE_DELAY = 1
STATUS_NAMES = {0: "Continue", 1: "Optimal", 2: "Unbounded", 3: "Infeasible"}


class FosError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libfoship error %d: %s" % (code, msg))
        self.code = code


class CheckResult(C.Structure):
    _fields_ = [("p", C.c_double), ("d", C.c_double), ("g", C.c_double), ("ctx", C.c_double), ("bty", C.c_double),
                ("kappa", C.c_double), ("tau", C.c_double), ("norm_axs", C.c_double), ("norm_aty", C.c_double),
                ("norm_b", C.c_double), ("norm_c", C.c_double), ("cgiter", C.c_int64), ("status", C.c_int32),
                ("cg_maxiter_hit", C.c_int32)]


_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_h = C.c_void_p
_dpp = C.POINTER(_dp)

# name -> (restype, argtypes): every symbol include/foship.h declares
PROTOTYPES = {
    "fos_abi_version": (C.c_int, []),
    "fos_last_error": (C.c_char_p, []),
    "fos_device_count": (C.c_int, [_i32p]),
    "fos_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "fos_create": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                             C.c_int64, _i32p, _i64p, _i64p, C.c_int64, _i32p, _i64p, _i64p, C.c_int, C.POINTER(_h)]),
    "fos_create2": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                              C.c_int64, _i32p, _i64p, _i64p, C.c_int64, _i32p, _i64p, _i64p, C.c_int, C.c_int32, C.POINTER(_h)]),
    "fos_create3": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                              C.c_int64, _i32p, _i64p, _i64p, C.c_int64, _i32p, _i64p, _i64p, C.c_int, C.c_int32, C.c_int32, C.POINTER(_h)]),
    "fos_get_equilibration": (C.c_int, [_h, _i32p, _dp, _dp, _dp]),
    "fos_host_equilibrate": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp,
                                       C.c_int64, _i32p, _i64p, _i64p, C.c_int64, _i32p, _i64p, _i64p, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]),
    "fos_destroy": (C.c_int, [_h]),
    "fos_sizes": (C.c_int, [_h, _i64p, _i64p, _i64p, _i64p]),
    "fos_get_cg_total": (C.c_int, [_h, _i64p]),
    "fos_operator_stats": (C.c_int, [_h, _i64p]),
    "fos_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "fos_set_linesearch": (C.c_int, [_h, C.c_int64]),
    "fos_linesearch_log": (C.c_int, [_h, _dp]),
    "fos_set_longstep": (C.c_int, [_h, C.c_int64, C.c_int64]),
    "fos_longstep_log": (C.c_int, [_h, _dp]),
    "fos_host_long_project": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp]),
    "fos_comm_init": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p]),
    "fos_comm_init_host": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fos_peer_export": (C.c_int, [_h, C.c_void_p]),
    "fos_peer_open": (C.c_int, [_h, C.c_int, C.c_int, C.c_void_p, C.c_double]),
    "fos_peer_open_host": (C.c_int, [_h, C.c_int, C.c_int, C.c_char_p, C.c_double]),
    "fos_peer_close": (C.c_int, [_h]),
    "fos_peer_selftest": (C.c_int, [_h, C.c_int, C.POINTER(C.c_int32)]),
    "fos_exchange_bench": (C.c_int, [_h, C.c_int, _dp]),
    "fos_peer_vec_export": (C.c_int, [_h, C.c_void_p]),
    "fos_peer_vec_open": (C.c_int, [_h, C.c_void_p]),
    "fos_peer_enable": (C.c_int, [_h, C.c_int32]),
    "fos_set_alg": (C.c_int, [_h, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "fos_reset_affine": (C.c_int, [_h]),
    "fos_enable_direct": (C.c_int, [_h, _i64p, _i64p, _dp]),
    "fos_disable_direct": (C.c_int, [_h]),
    "fos_get_direct_mode": (C.c_int, [_h, _i32p]),
    "fos_enable_direct2": (C.c_int, [_h, _i64p, _i64p, _dp, C.c_int32]),
    "fos_get_direct_stats": (C.c_int, [_h, _dp]),
    "fos_enable_direct3": (C.c_int, [_h, _i64p, _i64p, _dp, C.c_int32, C.c_int32]),
    "fos_get_direct_stats2": (C.c_int, [_h, _dp]),
    "fos_dense_spd_inverse": (C.c_int, [C.c_int32, C.c_int64, _dp, _dp, C.c_int32, _dp]),
    "fos_host_chol_inverse": (C.c_int, [C.c_int64, _dp, _dp, _i64p]),
    "fos_host_reduced_symm": (C.c_int, [C.c_int64, _dp, _dp, _dp, _i32p]),
    "fos_set_iterate": (C.c_int, [_h, _dp]),
    "fos_get_iterate": (C.c_int, [_h, _dp]),
    "fos_get_checked": (C.c_int, [_h, _dp]),
    "fos_step": (C.c_int, [_h, C.c_int64, C.c_int64, C.c_int64, C.c_double, _i64p, _i32p, C.POINTER(CheckResult)]),
    "fos_getsol": (C.c_int, [_h, _dp, C.c_int32, C.c_double, C.POINTER(CheckResult)]),
    "fos_get_affine_state": (C.c_int, [_h, _dp, _i64p, _i32p]),
    "fos_set_affine_state": (C.c_int, [_h, _dp, C.c_int64]),
    "fos_get_alg_state": (C.c_int, [_h, _dp, _dp, _dp]),
    "fos_set_alg_state": (C.c_int, [_h, _dp, _dp, _dp]),
    "fos_get_cgiter": (C.c_int, [_h, _i64p]),
    "fos_get_alpha12": (C.c_int, [_h, _dp]),
    "fos_get_prox_count": (C.c_int, [_h, _i64p]),
    "fos_q_apply": (C.c_int, [_h, _dp, _dp, C.c_int32]),
    "fos_kkt_apply": (C.c_int, [_h, _dp, _dp]),
    "fos_cg_kkt": (C.c_int, [_h, _dp, _dp, C.c_double, C.c_int64, _i64p]),
    "fos_prox_affine": (C.c_int, [_h, _dp, _dp]),
    "fos_hsdematrix_prox": (C.c_int, [_h, _dp, _dp]),
    "fos_prox_cones": (C.c_int, [_h, _dp, _dp]),
    "fos_check": (C.c_int, [_h, _dp, C.c_double, C.POINTER(CheckResult)]),
    "fos_profile": (C.c_int, [_h, C.c_int32]),
    "fos_profile_read": (C.c_int, [_h, _i64p, _dp, _dp]),
    "fos_profile_read_classes": (C.c_int, [_h, _i64p, _dp]),
    "fos_bench_cg_chain": (C.c_int, [_h, C.c_int32, C.c_int32, C.c_int32, _dp]),
    "fos_bench_kkt": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_psd_debug": (C.c_int, [_h, C.c_int32, C.c_int32]),
    "fos_psd_stats": (C.c_int, [_h, _i32p, C.c_int64, _i64p]),
    "fos_psd_fused_steps": (C.c_int, [_h, _i64p]),
    "fos_sync": (C.c_int, [_h]),
    "fos_host_stacked_spmv": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, C.c_int32, C.c_int32, _i64p]),
    "fos_host_resident_cg": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, C.c_int32, _dp, _dp, C.c_double, C.c_int64, _i64p, _i64p]),
    "fos_host_resident_plan": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, C.c_int32, _i64p, _i32p, C.c_int64, _i64p, C.c_int64]),
    "fos_host_stacked_spmv_mode": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, C.c_int32, _i64p]),
    "fos_window_stats": (C.c_int, [_h, _i64p]),
    "fos_set_tuning": (C.c_int, [_h, C.c_int32, C.c_int32, C.c_int32]),
    "fos_set_cg_variant": (C.c_int, [_h, C.c_int32]),
    "fos_get_cg_variant": (C.c_int, [_h, _i32p]),
    "fos_host_cg_variant": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _i32p]),
    "fos_host_cg_windows": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p]),
    "fos_resident_stats": (C.c_int, [_h, _i64p]),
    "fos_resident_lowp_stats": (C.c_int, [_h, _dp]),
    "fos_resident_lowp_cache_stats": (C.c_int, [_h, _i64p]),
    "fos_host_lowp_cached": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, _i32p, _i64p]),
    "fos_debug_set": (C.c_int, [_h, C.c_int32, C.c_int64]),
    "fos_set_gapp": (C.c_int, [_h, C.c_int64]),
    "fos_gapp_log": (C.c_int, [_h, _dp]),
    # Feasibility form (src/problemforms/Feasibility/*.jl)
    "fos_feas_create": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(_h)]),
    "fos_feas_destroy": (C.c_int, [_h]),
    "fos_feas_set_affine": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _dp]),
    "fos_feas_set_affine_sparse": (C.c_int, [_h, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp]),
    "fos_feas_affine_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_feas_set_affine_factored": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _dp, C.c_int32, C.c_int32]),
    "fos_feas_affine_factored_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_feas_affine_factored_plan": (C.c_int, [_h, C.c_int32, _i64p]),
    "fos_host_affine_factored": (C.c_int, [C.c_int64, C.c_int64, _dp, _dp, C.c_int32, _dp, _dp]),
    "fos_feas_set_least_squares": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _dp, C.c_double, C.c_int32]),
    "fos_host_least_squares": (C.c_int, [C.c_int64, C.c_int64, _dp, _dp, C.c_double, _dp, _dp]),
    "fos_feas_set_affine_sparse_factored": (C.c_int, [_h, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_int32, C.c_int32]),
    "fos_feas_affine_sparse_factored_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_feas_affine_sparse_factored_plan": (C.c_int, [_h, C.c_int32, _i64p]),
    "fos_host_affine_sparse_factored": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_int32, _dp, _dp]),
    "fos_feas_set_quadratic": (C.c_int, [_h, C.c_int32, _dp, _dp, C.c_int32]),
    "fos_feas_set_least_squares_normal": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _dp, C.c_double, C.c_int32]),
    "fos_feas_set_least_squares_sparse": (C.c_int, [_h, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_double, C.c_int32, C.c_int32]),
    "fos_feas_nspace_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_host_quadratic": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp]),
    "fos_host_least_squares_normal": (C.c_int, [C.c_int64, C.c_int64, _dp, _dp, C.c_double, _dp, _dp]),
    "fos_host_least_squares_sparse": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_double, C.c_int32, _dp, _dp]),
    "fos_host_symv_packed": (C.c_int, [C.c_int64, _dp, _dp, _dp, _i32p]),
    "fos_feas_set_quadratic_sparse": (C.c_int, [_h, C.c_int32, _i64p, _i64p, _dp, _dp, C.c_double]),
    "fos_feas_set_least_squares_cg": (C.c_int, [_h, C.c_int32, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_double, C.c_double]),
    "fos_feas_nspace_cg_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_host_quadratic_cg": (C.c_int, [C.c_int64, _i64p, _i64p, _dp, _dp, C.c_double, _dp, _dp, _i32p]),
    "fos_host_least_squares_cg": (C.c_int, [C.c_int64, C.c_int64, _i64p, _i64p, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _i32p]),
    "fos_bench_symv_packed": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, _dp]),
    "fos_feas_set_box": (C.c_int, [_h, C.c_int32, C.c_double, C.c_double]),
    "fos_feas_set_box_arrays": (C.c_int, [_h, C.c_int32, _dp, _dp]),
    "fos_feas_set_cones": (C.c_int, [_h, C.c_int32, C.c_int64, _i32p, _i64p]),
    "fos_feas_set_callback": (C.c_int, [_h, C.c_int32, C.c_void_p, C.c_void_p]),
    "fos_feas_set_blocks": (C.c_int, [_h, C.c_int32, C.c_int64, _i32p, _i64p, _dp, _dp]),
    "fos_feas_set_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_host_set_project": (C.c_int, [C.c_int32, C.c_int64, _dp, _dp, _dp, _dp, _i32p]),
    "fos_feas_set_blocks2": (C.c_int, [_h, C.c_int32, C.c_int64, _i32p, _i64p, _dp, _dp, C.c_int64, _i64p, _i64p, _dpp, _i64p, _dpp]),
    "fos_feas_dense_block_stats": (C.c_int, [_h, C.c_int32, _dp]),
    "fos_feas_dense_block_get": (C.c_int, [_h, C.c_int32, C.c_int64, _dp, _dp]),
    "fos_host_dense_block": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp]),
    "fos_feas_set_alg": (C.c_int, [_h, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double]),
    "fos_feas_set_gapp": (C.c_int, [_h, C.c_double, C.c_double, C.c_double, C.c_int64]),
    "fos_feas_gapp_log": (C.c_int, [_h, _dp]),
    "fos_feas_set_linesearch": (C.c_int, [_h, C.c_int64]),
    "fos_feas_linesearch_log": (C.c_int, [_h, _dp]),
    "fos_feas_set_longstep": (C.c_int, [_h, C.c_int64, C.c_int64]),
    "fos_feas_longstep_log": (C.c_int, [_h, _dp]),
    "fos_feas_set_iterate": (C.c_int, [_h, _dp]),
    "fos_feas_step": (C.c_int, [_h, C.c_int64, C.c_int64, C.c_int64, C.c_double, _i64p, _i32p, _dp, _i32p]),
    "fos_feas_getsol": (C.c_int, [_h, _dp, C.c_int32, C.c_double, _i32p, _dp]),
    "fos_feas_get_iterate": (C.c_int, [_h, _dp]),
    "fos_feas_prox": (C.c_int, [_h, C.c_int32, _dp, _dp]),
    "fos_feas_info": (C.c_int, [_h, _dp, _i32p, _dp]),
}

_lib = None


def load(check_symbols=False):
    """dlopen csrc/libfoship.so and bind every prototype.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and not check_symbols:
        return _lib
    if not LIB_PATH.exists():
        raise FosError(-100, "%s not found: build it with `make -C %s` (hipcc, gfx950); there is no CPU fallback"
                       % (LIB_PATH, LIB_PATH.parent))
    lib = C.CDLL(str(LIB_PATH), mode=getattr(os, "RTLD_NOW", 2) | getattr(os, "RTLD_GLOBAL", 0x100))
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.fos_abi_version() != 1:
        raise FosError(-101, "ABI version mismatch")
    _lib = lib
    return lib


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)     # fos_allreduce_fn


def header_symbols():
    """The function names declared in include/foship.h (parsed, so the test notices a header/binding drift)."""
    import re
    text = (_HERE.parent / "include" / "foship.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fos_[a-z0-9_]+)\s*\(", text)))


def check(code):
    if code != FOS_OK:
        msg = load().fos_last_error()
        raise FosError(code, msg.decode("utf-8", "replace") if msg else "")


def dptr(a):
    return a.ctypes.data_as(_dp)


def as_f64(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if n is not None and a.shape[0] != n:
        raise ValueError("expected %d entries, got %d" % (n, a.shape[0]))
    return a


def device_count():
    n = C.c_int32(0)
    check(load().fos_device_count(C.byref(n)))
    return n.value
