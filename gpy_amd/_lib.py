"""ctypes binding of libmi355gp.so (C-ABI declared in include/mi355gp.h).

No PyTorch, no CPU fallback: if the library is missing it is built with hipcc (gfx950) on first use, and
every compute entry point raises when no MI355X is visible.  The CPU oracle under `oracle/` is never
imported from here.
"""
import ctypes
import os
import subprocess

import numpy as np
from numpy.ctypeslib import ndpointer

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355GP_LIB") or os.path.join(_HERE, "libmi355gp.so")
CSRC = os.path.join(_HERE, "csrc")

KIND_IDS = {"rbf": 0, "matern52": 1, "matern32": 2, "exponential": 3, "white": 4, "bias": 5, "ratquad": 6, "stdperiodic": 7,
            "coregionalize": 8, "linear": 9, "mlp": 10, "poly": 11, "cosine": 12, "sinc": 13, "expquadcosine": 14}


def ard_id(kind, ARD):
    """`ard` of the C-ABI: a flag, for StdPeriodic the bitmask ARD1 | ARD2 << 1, for Coregionalize the number of outputs"""
    if kind == "coregionalize":
        return int(ARD)
    return int(ARD) & 3 if kind == "stdperiodic" else int(bool(ARD))


class Part(ctypes.Structure):
    """`mi355gp_part` of include/mi355gp.h: one part of a sum-of-products kernel expression."""
    _fields_ = [("kind", ctypes.c_int), ("ard", ctypes.c_int), ("n_active", ctypes.c_int),
                ("active_dims", ctypes.POINTER(ctypes.c_int)), ("theta", ctypes.POINTER(ctypes.c_double)),
                ("term", ctypes.c_int)]


def make_parts(specs):
    """specs: [(kind_name, ARD, theta array, active_dims array or None[, term])] -> (ctypes array, keep-alive list,
    n_theta).  term (optional, default 0): parts with the same non-zero term id are multiplied (product kernels)."""
    arr = (Part * len(specs))()
    keep, ntheta = [], 0
    for i, spec in enumerate(specs):
        kind, ARD, theta, dims = spec[:4]
        arr[i].term = int(spec[4]) if len(spec) > 4 else 0
        th = np.ascontiguousarray(theta, dtype=np.float64)
        keep.append(th)
        arr[i].kind = KIND_IDS[kind]
        arr[i].ard = ard_id(kind, ARD)
        arr[i].theta = th.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        if dims is None:
            arr[i].n_active = 0
            arr[i].active_dims = None
        else:
            d = np.ascontiguousarray(dims, dtype=np.int32)
            keep.append(d)
            arr[i].n_active = d.size
            arr[i].active_dims = d.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        ntheta += th.size
    return arr, keep, ntheta
FETCH_L, FETCH_KINV, FETCH_DLDK, FETCH_K = 0, 1, 2, 3
EP_BERNOULLI_PROBIT = 0
OUT_LML, OUT_LOGDET, OUT_DATAFIT, OUT_DNOISE, OUT_TRKINV, NUM_OUT = 0, 1, 2, 3, 4, 8
STAGE_NAMES = ("kbuild", "potrf", "trtri", "lauum", "solve", "grad", "total")
NUM_T = 8
PROFILE_FAMILIES = ("update_nt", "trtri", "lauum", "diag128", "trsm128", "update_nt64", "potrf_persist", "trtri_early")

_lib = None


class MI355GPError(RuntimeError):
    pass


DIAG_LIB_PATH = os.path.join(_HERE, "libmi355gp_diag.so")


def build(force=False):
    """Compile every HIP translation unit for gfx950 and link, in-tree (make -C gpy_amd/csrc): libmi355gp.so, the product, and
    libmi355gp_diag.so, the same sources with -DMI355GP_DIAG (schedule overrides, fault injectors and bounding experiments that
    the product build compiles out; loaded only by the tests / tools that ask for it through MI355GP_LIB)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) or f == "Makefile"]
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug_lauum.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug_tileops.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_epdtc.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_sparse_diag.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_sparse_coreg.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug_sparse_coreg.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_psi_lin.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug_psi_lin.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_psi_ss.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_sparse_missing.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_debug_sparse_missing.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_vargauss.h"))
    srcs.append(os.path.join(_HERE, "..", "include", "mi355gp_kron.h"))
    product = os.path.join(_HERE, "libmi355gp.so")
    if not force and os.path.exists(product) and os.path.exists(DIAG_LIB_PATH):
        t = min(os.path.getmtime(product), os.path.getmtime(DIAG_LIB_PATH))
        if all(os.path.getmtime(s) <= t for s in srcs if os.path.exists(s)):
            return product
    r = subprocess.run(["make", "-C", CSRC, "-j8", "all", "diag"], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(product) or not os.path.exists(DIAG_LIB_PATH):
        raise MI355GPError("building libmi355gp.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return product


_ci, _i64, _cd, _vp, _str = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_char_p
_dp = ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")              # a double array that must be there
_c_dp = ctypes.POINTER(ctypes.c_double)                               # a double array or scalar that may be NULL
_ip, _hp, _parts = ctypes.POINTER(_ci), ctypes.POINTER(_vp), ctypes.POINTER(Part)
_i32a, _i64a = (ndpointer(dtype=t, flags="C_CONTIGUOUS") for t in (np.int32, np.int64))
_EXACT = [_vp, _ci, _ci, _dp, _dp, _i64, _cd, _cd, _dp] + [_c_dp] * 4   # (ctx, kind, ard, theta, array, length, 2 scalars, out, 4 optional)
_KERN_X2 = [_dp, _i64, _c_dp, _i64, _ci, _dp]                           # (X, N, X2 or NULL, M, D, out)

# The C-ABI, once: every function of include/mi355gp.h and include/mi355gp_debug.h, in their order, with its parameter types.
# All return int except the two `const char*` ones (`lib()`); tests/test_abi.py holds each entry against the headers' prototypes.
ABI = {
    "mi355gp_last_error": [],
    "mi355gp_version": [],
    "mi355gp_device_count": [_ip],
    "mi355gp_device_synchronize": [_ci],
    "mi355gp_create": [_ci, _hp],
    "mi355gp_destroy": [_vp],
    "mi355gp_set_data": [_vp, _dp, _i64, _ci, _dp, _ci],
    "mi355gp_set_targets": [_vp, _dp, _ci],
    "mi355gp_kern_K": [_ci, _ci, _ci, _dp] + _KERN_X2,
    "mi355gp_kern_Kdiag": [_ci, _dp, _i64, _dp],
    "mi355gp_update_gradients_full": [_ci, _ci, _ci, _dp, _dp] + _KERN_X2,
    "mi355gp_gradients_X": [_ci, _ci, _ci, _dp, _dp] + _KERN_X2,
    "mi355gp_exact_inference": _EXACT,
    "mi355gp_exact_inference_sum": [_vp, _ci, _parts, _dp, _i64, _cd, _cd, _dp] + [_c_dp] * 4,
    "mi355gp_exact_studentt_sum": [_vp, _ci, _parts, _cd, _cd, _cd, _dp] + [_c_dp] * 3,
    "mi355gp_inference_given_K": [_vp, _dp, _dp, _i64, _cd, _cd, _dp] + [_c_dp] * 3,
    "mi355gp_fetch": [_vp, _ci, _dp, _ci],
    "mi355gp_predict": [_vp, _ci, _ci, _dp, _dp, _i64, _c_dp, _c_dp, _ci],
    "mi355gp_predict_sum": [_vp, _ci, _parts, _dp, _i64, _c_dp, _c_dp, _ci],
    "mi355gp_predictive_gradients_sum": [_vp, _ci, _parts, _dp, _i64, _c_dp, _c_dp],
    "mi355gp_laplace_begin": [_vp, _ci, _parts],
    "mi355gp_laplace_newton": [_vp, _dp, _dp, _cd, _dp, _dp, _c_dp],
    "mi355gp_laplace_finish": [_vp, _dp, _cd, _dp, _c_dp],
    "mi355gp_laplace_gradients": [_vp, _dp, _dp, _dp],
    "mi355gp_laplace_implicit": [_vp, _dp, _dp],
    "mi355gp_laplace_predict": [_vp, _ci, _parts, _dp, _i64, _dp, _c_dp, _c_dp, _ci],
    "mi355gp_ep_recompute": [_vp, _dp, _dp, _cd, _cd, _ci, _dp, _dp, _c_dp, _c_dp],
    "mi355gp_ep_sweep": [_vp, _ci, _i64a, _dp, _cd, _cd] + [_dp] * 7 + [_c_dp],
    "mi355gp_covariance_between_points": [_vp, _ci, _parts, _dp, _i64, _dp, _i64, _dp],
    "mi355gp_potrf": [_ci, _dp, _i64, _c_dp],
    "mi355gp_pdinv": [_ci, _dp, _i64] + [_c_dp] * 4,
    "mi355gp_pdinv_full": [_ci, _dp, _i64] + [_c_dp] * 5,
    "mi355gp_set_option": [_vp, _ci, _ci],
    "mi355gp_get_option": [_vp, _ci, _ip],
    "mi355gp_get_profile": [_vp, _dp, _dp, _i32a],
    "mi355gp_grid_unique_id": [_str],
    "mi355gp_grid_create": [_ci] * 6 + [_str, _hp],
    "mi355gp_grid_destroy": [_vp],
    "mi355gp_grid_set_data": [_vp, _dp, _i64, _ci, _dp, _ci],
    "mi355gp_grid_exact_inference": _EXACT,
    "mi355gp_grid_fetch": [_vp, _ci, _dp],
    "mi355gp_grid_set_option": [_vp, _ci, _ci],
    "mi355gp_grid_get_option": [_vp, _ci, _ip],
    "mi355gp_grid_coll_log": [_vp, _ci, _dp],
    "mi355gp_sparse_create": [_ci, _hp],
    "mi355gp_sparse_destroy": [_vp],
    "mi355gp_sparse_set_data": [_vp, _dp, _i64, _ci, _dp, _ci],
    "mi355gp_vardtc_inference": _EXACT,
    "mi355gp_vardtc_inference_sum": [_vp, _ci, _parts, _dp, _i64, _dp, _i64, _cd, _dp] + [_c_dp] * 6,
    "mi355gp_sparse_set_input_variance": [_vp, _dp, _i64, _ci],
    "mi355gp_sparse_set_inputs": [_vp, _dp, _c_dp, _i64, _ci],
    "mi355gp_vardtc_inference_uncertain": [_vp, _ci, _parts, _dp, _i64, _dp, _i64, _cd, _dp] + [_c_dp] * 6,
    "mi355gp_sparse_predict": [_vp, _ci, _parts, _dp, _i64, _c_dp, _c_dp, _ci],
    "mi355gp_sparse_predict_uncertain": [_vp, _ci, _parts, _dp, _dp, _i64, _dp, _c_dp],
    "mi355gp_sparse_get_predict_ms": [_vp, _c_dp],
    "mi355gp_sparse_fetch_dLdKnm": [_vp, _i64, _i64, _dp],
    "mi355gp_sparse_attach_comm": [_vp, _ci, _ci, _str],
    "mi355gp_sparse_attach_loopback": [_vp, _ci, _ci, _ci],
    "mi355gp_sparse_fetch": [_vp, _ci, _dp],
    "mi355gp_sparse_get_profile": [_vp, _dp],
    "mi355gp_svgp_forward": [_vp, _ci, _parts, _dp, _i64, _dp, _dp, _ci, _cd, _dp, _dp, _dp, _c_dp],
    "mi355gp_svgp_backward": [_vp, _dp, _dp] + [_c_dp] * 5,
    "mi355gp_svgp_predict": [_vp, _ci, _parts, _c_dp, _i64, _ci] + [_c_dp] * 4,
    "mi355gp_pep_inference": [_vp, _ci, _parts, _dp, _i64, _cd, _cd, _cd, _dp] + [_c_dp] * 5,
    "mi355gp_pep_check_sigma": [_dp, _i64, _i64, _cd, _cd],
    "mi355gp_rbf_psi": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci] + [_c_dp] * 3,
    "mi355gp_rbf_psi_grad": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci] + [_c_dp] * 4 + [_dp] * 5,
    # ---- include/mi355gp_debug.h ----
    "mi355gp_bench_factor": [_ci, _i64, _ci, _c_dp, _c_dp, _c_dp],
    "mi355gp_dbg_ipc_selftest": [_str, _ci, _ci, _ci, _ci, _i64, _dp],
    "mi355gp_dbg_comm_selftest": [_ci, _str, _ci, _ci, _ci, _ci, _i64, _ci, _dp],
    "mi355gp_dbg_grid_multi": [_ci, _ci, _ci, _ci, _dp],
    "mi355gp_dbg_update_nt": [_ci, _ci, _ip, _ci, _ci, _dp],
    "mi355gp_dbg_update_rect": [_ci, _ci, _ci, _ip, _ci, _ci, _dp],
    "mi355gp_dbg_mfma": [_ci, _dp, _dp, _dp],
    "mi355gp_dbg_gemm": [_ci, _ci, _ci, _i64, _i64, _i64, _dp, _dp, _dp, _cd, _cd, _ci, _c_dp],
    "mi355gp_dbg_peaks": [_ci, _dp],
    "mi355gp_dbg_gemm_clock": [_c_dp, _c_dp],
    "mi355gp_dbg_cu_map": [_ci, _ci, _ci, ctypes.POINTER(ctypes.c_uint)],
    "mi355gp_dbg_pipe_share": [_ci, _dp],
    "mi355gp_dbg_graph_factor": [_ci, _i64, _ci, _dp],
    "mi355gp_dbg_persist": [_ci, _i64, _ci, _ci, _dp],
    "mi355gp_dbg_lauum_plan": [_ci, _ip, _ci, _ip],
    "mi355gp_dbg_persist_owners": [_ci, _ci, _ci, _ip, _ip],
    "mi355gp_dbg_mask_probe": [_ci, _ci, _ci, _dp],
}
EXPORTED = tuple(ABI)
# include/mi355gp_debug_lauum.h: the diagnostics of X^T X on the 128 x 256 tile, in its order (tests/test_lauum_wide_map.py holds the
# table against that header's prototypes)
DEBUG_LAUUM_ABI = {
    "mi355gp_dbg_lauum_wide_map": [_ci, _ip, _ci, _ip],
    "mi355gp_dbg_lauum": [_ci, _i64, _c_dp, _c_dp, _ci, _ci, _c_dp],
}
# include/mi355gp_debug_tileops.h: one launcher of the tile-GEMM family alone (tests/test_oracle_tileops.py holds the table against
# that header's prototype)
DEBUG_TILEOPS_ABI = {
    "mi355gp_dbg_tileop": [_ci, _ci, ctypes.POINTER(_i64), _c_dp, _c_dp, _c_dp, _cd],
}
# include/mi355gp_epdtc.h: EPDTC on the sparse context, in its order (tests/test_oracle_epdtc.py holds the table against that
# header's prototypes)
EPDTC_ABI = {
    "mi355gp_epdtc_begin": [_vp, _ci, _parts, _dp, _i64, _cd],
    "mi355gp_epdtc_recompute": [_vp, _dp, _dp, _dp, _dp, _c_dp],
    "mi355gp_epdtc_sweep": [_vp, _i64a, _dp, _cd, _cd, _ci] + [_dp] * 7 + [_c_dp],
    "mi355gp_epdtc_inference": [_vp, _ci, _parts, _dp, _i64, _dp, _dp, _cd, _dp] + [_c_dp] * 5,
}
# include/mi355gp_sparse_diag.h: the per-point diagonal of an expression on the sparse context (tests/test_sparse_lin_host.py holds
# the table against that header's prototype)
SPARSE_DIAG_ABI = {
    "mi355gp_sparse_set_linear": [_vp, _ci],
    "mi355gp_sparse_kdiag": [_vp, _ci, _parts] + [_c_dp] * 4,
}
# include/mi355gp_sparse_coreg.h: Coregionalize parts on the sparse context (tests/test_sparse_coreg_host.py holds the table
# against that header's prototype)
SPARSE_COREG_ABI = {
    "mi355gp_sparse_set_coregionalize": [_vp, _ci],
}
# include/mi355gp_debug_sparse_coreg.h: the A/B switch of the sparse context's fused gradient passes, a diagnostic (held by the
# same test)
DEBUG_SPARSE_COREG_ABI = {
    "mi355gp_dbg_sparse_set_fuse_cols": [_vp, _ci],
}
# include/mi355gp_psi_lin.h: Linear and Bias psi-statistics on the sparse context (tests/test_psi_lin_host.py holds the table
# against that header's prototype)
PSI_LIN_ABI = {
    "mi355gp_sparse_set_psi_lin_bias": [_vp, _ci],
}
# include/mi355gp_debug_psi_lin.h: the row kernel of a Linear part on its own, a diagnostic (held by the same test)
DEBUG_PSI_LIN_ABI = {
    "mi355gp_dbg_psi_lin_rows": [_ci, _ci, _dp] + [_c_dp] * 3 + [_cd, _cd, _dp, _dp, _dp, _cd, _i64, _i64, _ci, _ci, _dp, _ci, _c_dp],
}
# include/mi355gp_psi_ss.h: the RBF psi-statistics for spike-and-slab inputs, in its order (tests/test_oracle_psi_ss.py holds the
# table against that header's prototypes)
PSI_SS_ABI = {
    "mi355gp_ssrbf_psi": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _dp, _i64, _ci] + [_c_dp] * 3,
    "mi355gp_ssrbf_psi_grad": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _dp, _i64, _ci] + [_c_dp] * 4 + [_dp] * 6,
    "mi355gp_sparse_set_binary_prob": [_vp, _c_dp, _i64, _ci],
    "mi355gp_sparse_set_inputs_ss": [_vp, _dp, _dp, _dp, _i64, _ci],
    "mi355gp_vardtc_inference_ss": [_vp, _ci, _parts, _dp, _i64, _dp, _i64, _cd, _dp] + [_c_dp] * 7,
}
# include/mi355gp_vargauss.h: the variational Gaussian approximation inside the Laplace session of an exact context, in its order
# (tests/test_oracle_vargauss.py holds the table against that header's prototypes)
VARGAUSS_ABI = {
    "mi355gp_vargauss_forward": [_vp, _dp, _dp, _cd, _dp, _dp, _dp],
    "mi355gp_vargauss_backward": [_vp, _dp, _dp, _dp, _dp, _dp],
    "mi355gp_vargauss_backward_exact": [_vp, _dp, _dp, _dp, _dp, _dp],
}
# include/mi355gp_kron.h: exact GP regression on a full Cartesian grid (Kronecker-structured covariance), in its order
# (tests/test_oracle_kron.py holds the table against that header's prototypes)
KRON_ABI = {
    "mi355gp_kron_create": [_ci, _hp],
    "mi355gp_kron_destroy": [_vp],
    "mi355gp_kron_set_data": [_vp, _ci, _i64a, _dp],
    "mi355gp_kron_solve": [_vp, _dp, _dp, _cd, _dp],
    "mi355gp_kron_quadforms": [_vp, _ci, _dp, _dp, _dp],
    "mi355gp_kron_predict": [_vp, _i64, _dp, _c_dp, _cd, _dp, _c_dp],
    "mi355gp_kron_fetch": [_vp, _ci, _dp],
    "mi355gp_kron_mode_probe": [_vp, _i64, _i64, _i64, _ci, _dp, _dp, _dp, _ci, _c_dp],
    "mi355gp_kron_get_ms": [_vp, _c_dp],
}
# include/mi355gp_sparse_missing.h: psi2 and its chain rule for several row masks at once (missing data), in its order
# (tests/test_oracle_missing.py holds the table against that header's prototypes)
MISSING_ABI = {
    "mi355gp_psi_groups_batch": [],
    "mi355gp_rbf_psi2_groups": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci, _dp, _ci, _dp],
    "mi355gp_rbf_psi_grad_groups": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci, _dp, _ci, _dp] + [_dp] * 5,
    "mi355gp_sparse_set_output_groups": [_vp, _ci, _ip, _c_dp],
    "mi355gp_vardtc_inference_missing": [_vp, _ci, _parts, _dp, _i64, _dp, _i64, _cd, _dp] + [_c_dp] * 6,
    "mi355gp_sparse_select_output_group": [_vp, _ci],
    "mi355gp_sparse_fetch_group_scalars": [_vp, _dp],
}
# include/mi355gp_debug_sparse_missing.h: the stateless pair with the replaced route and the kernels' stream time, diagnostics
# (held by the same test)
DEBUG_MISSING_ABI = {
    "mi355gp_dbg_rbf_psi2_groups": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci, _dp, _ci, _ci, _dp, _c_dp],
    "mi355gp_dbg_rbf_psi_grad_groups": [_ci, _cd, _dp, _ci, _dp, _i64, _dp, _dp, _i64, _ci, _dp, _ci, _dp, _ci] + [_dp] * 5 + [_c_dp],
}
TILEOPS = {"trmm_lower": 0, "trmm_lower_T": 1, "trmm64": 2, "gram_splitk": 3, "update_nt": 4}    # MI355GP_TILEOP_*


def _opt(a):
    """optional output array -> pointer or NULL"""
    return None if a is None else a.ctypes.data_as(_c_dp)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        for table in (ABI, DEBUG_LAUUM_ABI, DEBUG_TILEOPS_ABI, EPDTC_ABI, SPARSE_DIAG_ABI, SPARSE_COREG_ABI, DEBUG_SPARSE_COREG_ABI, PSI_LIN_ABI, DEBUG_PSI_LIN_ABI,
                      PSI_SS_ABI, VARGAUSS_ABI, KRON_ABI, MISSING_ABI, DEBUG_MISSING_ABI):
            for name, argtypes in table.items():
                getattr(L, name).argtypes = argtypes
        L.mi355gp_last_error.restype = L.mi355gp_version.restype = _str
        _lib = L
    return _lib


# mi355gp_set_option / mi355gp_get_option ids (include/mi355gp.h, MI355GP_OPT_*)
OPTIONS = {"profile": 0, "lookahead": 1, "tri_overlap": 2, "tri_min_nt": 3, "tri_h": 4, "tri_wgs": 5, "tri_half": 6,
           "part1_on_panel": 7, "nbo": 8, "solve_overlap": 9, "diag_excl_first": 10, "graph": 11, "persist": 12, "agg2": 13,
           "persist_test": 14, "persist_aborts": 15, "persist_skip": 16, "persist_sched": 17}


def last_error():
    return lib().mi355gp_last_error().decode()


def check(rc, what):
    """negative rc -> exception; positive rc (LAPACK info) is returned to the caller"""
    if rc < 0:
        raise MI355GPError("%s failed (rc=%d): %s" % (what, rc, last_error()))
    return rc


def device_count():
    n = ctypes.c_int(0)
    lib().mi355gp_device_count(ctypes.byref(n))
    return n.value


def device_synchronize(device=0):
    """hipDeviceSynchronize through the library (no second HIP runtime user in the process)."""
    require_device(device)
    check(lib().mi355gp_device_synchronize(int(device)), "mi355gp_device_synchronize")


def require_device(device=0):
    n = device_count()
    if device >= n:
        raise MI355GPError("no MI355X visible to HIP (device %d requested, %d present): the gpy_amd backend has "
                           "no CPU fallback" % (device, n))


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def theta_vec(variance, lengthscale, ARD, D):
    ls = np.atleast_1d(np.asarray(lengthscale, dtype=np.float64)).ravel()
    if ARD:
        if ls.size == 1:
            ls = np.full(D, ls[0])
        assert ls.size == D, "ARD kernel needs one lengthscale per input dimension"
    else:
        assert ls.size == 1, "isotropic kernel has a single lengthscale"
    return np.concatenate([[float(np.asarray(variance).ravel()[0])], ls])


def _exact_result(out, ms, **arrays):
    """the result dict of the exact-inference entries from their scalar block, stage times and output arrays"""
    res = dict(lml=out[OUT_LML], logdet=out[OUT_LOGDET], datafit=out[OUT_DATAFIT], dnoise=out[OUT_DNOISE],
               trKinv=out[OUT_TRKINV], **arrays)
    if ms is not None:
        res["stage_ms"] = dict(zip(STAGE_NAMES, ms[:len(STAGE_NAMES)]))
    return res


def _predict(entry, head, Xnew, D, Dy, full_cov, want_var, between=()):
    """the shared part of the predict entries, which all end (..., Xnew, M, [between,] mu, var, full_cov):
    (mu (M x Dy), var (M x 1) or cov (M x M) or None)"""
    Xnew = f64(Xnew)
    M = Xnew.shape[0]
    assert Xnew.shape[1] == D
    mu = np.empty((M, Dy))
    var = (np.empty((M, M)) if full_cov else np.empty(M)) if want_var else None
    check(getattr(lib(), entry)(*(tuple(head) + (Xnew, M) + tuple(between) + (mu.ctypes.data_as(_c_dp), _opt(var),
                                                                              int(bool(full_cov))))), entry)
    if var is not None and not full_cov:
        var = var[:, None]
    return mu, var


class _Handle(object):
    """Owner of one context handle of the C-ABI: made by the entry `_create` on construction, given to `_destroy` once, by
    `close()` or when the object is collected."""
    _create = _destroy = None

    def __init__(self, device=0):
        require_device(device)
        self._h = ctypes.c_void_p()
        check(getattr(lib(), self._create)(device, ctypes.byref(self._h)), self._create)
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One device context = one uploaded data set (X, R = Y - mean) with its N x N buffers in HBM."""
    _create, _destroy = "mi355gp_create", "mi355gp_destroy"

    def __init__(self, device=0):
        super(Context, self).__init__(device)
        self.N = self.D = self.Dy = 0

    def set_data(self, X, R):
        X, R = f64(X), f64(R)
        assert X.ndim == 2 and R.ndim == 2 and X.shape[0] == R.shape[0]
        self.N, self.D = X.shape
        self.Dy = R.shape[1]
        check(lib().mi355gp_set_data(self._h, X, self.N, self.D, R, self.Dy), "mi355gp_set_data")

    def set_targets(self, R):
        R = f64(R)
        check(lib().mi355gp_set_targets(self._h, R, R.shape[1]), "mi355gp_set_targets")

    def _exact(self, entry, head, ntheta, noise, jitter, extra_jitter, want_alpha, want_diag, want_stage_ms):
        """the shared part of `exact_inference` / `exact_inference_sum`: (info, dict)"""
        noise = f64(np.atleast_1d(noise))
        out = np.zeros(NUM_OUT)
        alpha = np.empty((self.N, self.Dy)) if want_alpha else None
        dtheta = np.zeros(ntheta)
        diag = np.empty(self.N) if want_diag else None
        ms = np.zeros(NUM_T) if want_stage_ms else None
        rc = check(getattr(lib(), entry)(self._h, *(tuple(head) + (noise, noise.size, jitter, extra_jitter, out, _opt(alpha),
                                                                   _opt(dtheta), _opt(diag), _opt(ms)))), entry)
        return rc, _exact_result(out, ms, alpha=alpha, dtheta=dtheta, diag_dL_dK=diag)

    def exact_inference(self, kind, ARD, theta, noise, jitter=1e-8, extra_jitter=0.0, want_alpha=True,
                        want_diag=False, want_stage_ms=False):
        """Returns (info, dict).  info > 0: not positive definite (the caller runs GPy's jitter ladder)."""
        theta = f64(theta)
        return self._exact("mi355gp_exact_inference", (KIND_IDS[kind], ard_id(kind, ARD), theta), theta.size, noise, jitter,
                           extra_jitter, want_alpha, want_diag, want_stage_ms)

    def exact_inference_sum(self, specs, noise, jitter=1e-8, extra_jitter=0.0, want_alpha=True, want_diag=False,
                            want_stage_ms=False):
        """Sum kernel: specs = [(kind, ARD, theta, active_dims or None)]; dtheta is the concatenation over the parts."""
        arr, keep, ntheta = make_parts(specs)
        return self._exact("mi355gp_exact_inference_sum", (len(specs), arr), ntheta, noise, jitter, extra_jitter, want_alpha,
                           want_diag, want_stage_ms)

    def predict_sum(self, specs, Xnew, full_cov=False, want_var=True):
        arr, keep, _ = make_parts(specs)
        return _predict("mi355gp_predict_sum", (self._h, len(specs), arr), Xnew, self.D, self.Dy, full_cov, want_var)

    def exact_studentt_sum(self, specs, nu, jitter=1e-8, extra_jitter=0.0):
        """Student-t process: (info, dict(lml, logdet, beta, scale, alpha, dtheta))"""
        arr, keep, ntheta = make_parts(specs)
        out = np.zeros(NUM_OUT)
        alpha = np.empty((self.N, self.Dy))
        dtheta = np.zeros(ntheta)
        rc = check(lib().mi355gp_exact_studentt_sum(self._h, len(specs), arr, float(nu), jitter, extra_jitter, out,
                                                    _opt(alpha), _opt(dtheta), None), "mi355gp_exact_studentt_sum")
        return rc, dict(lml=out[OUT_LML], logdet=out[OUT_LOGDET], beta=out[OUT_DATAFIT], scale=out[5], alpha=alpha,
                        dtheta=dtheta)

    def predictive_gradients(self, specs, Xnew, want_var=True):
        """(dmu (M x D x Dy), dvar (M x D)) of GP.predictive_gradients (core/gp.py:418-474), reduced on the device."""
        arr, keep, _ = make_parts(specs)
        Xnew = f64(Xnew)
        M = Xnew.shape[0]
        assert Xnew.shape[1] == self.D
        dmu = np.empty((M, self.D, self.Dy))
        dvar = np.empty((M, self.D)) if want_var else None
        check(lib().mi355gp_predictive_gradients_sum(self._h, len(specs), arr, Xnew, M, dmu.ctypes.data_as(_c_dp), _opt(dvar)),
              "mi355gp_predictive_gradients_sum")
        return dmu, dvar

    def covariance_between_points(self, specs, X1, X2):
        arr, keep, _ = make_parts(specs)
        X1, X2 = f64(X1), f64(X2)
        out = np.empty((X1.shape[0], X2.shape[0]))
        check(lib().mi355gp_covariance_between_points(self._h, len(specs), arr, X1, X1.shape[0], X2, X2.shape[0], out),
              "mi355gp_covariance_between_points")
        return out

    def inference_given_K(self, K, noise, jitter=1e-8, extra_jitter=0.0, want_diag=False, want_stage_ms=False):
        K = f64(K)
        assert K.shape == (self.N, self.N)
        noise = f64(np.atleast_1d(noise))
        out = np.zeros(NUM_OUT)
        alpha = np.empty((self.N, self.Dy))
        diag = np.empty(self.N) if want_diag else None
        ms = np.zeros(NUM_T) if want_stage_ms else None
        rc = check(lib().mi355gp_inference_given_K(self._h, K, noise, noise.size, jitter, extra_jitter, out,
                                                   _opt(alpha), _opt(diag), _opt(ms)), "mi355gp_inference_given_K")
        return rc, _exact_result(out, ms, alpha=alpha, diag_dL_dK=diag)

    # ---- Laplace session (include/mi355gp.h: begin, newton per mode-search iteration, finish, gradients, predict / fetch) ----
    def laplace_begin(self, specs):
        """K = kern.K(X) for the part list, resident for the session (reference `laplace.py:129`)."""
        arr, keep, ntheta = make_parts(specs)
        check(lib().mi355gp_laplace_begin(self._h, len(specs), arr), "mi355gp_laplace_begin")
        self._lap_ntheta = ntheta

    def laplace_newton(self, W, b, extra_jitter=0.0):
        """One iteration of `rasm_mode` (reference `laplace.py:184-199`): (info, a = full-step Ki_f, K a, logdet B)."""
        W, b = f64(np.ravel(W)), f64(np.ravel(b))
        assert W.size == self.N and b.size == self.N
        a, Ka = np.empty(self.N), np.empty(self.N)
        ld = ctypes.c_double(0.0)
        rc = check(lib().mi355gp_laplace_newton(self._h, W, b, float(extra_jitter), a, Ka, ctypes.byref(ld)),
                   "mi355gp_laplace_newton")
        return rc, a, Ka, ld.value

    def laplace_finish(self, W, extra_jitter=0.0):
        """The B statistics at the mode (reference `laplace.py:247,333-351`): (info, diag(Ki_W_i), logdet_I_KW)."""
        W = f64(np.ravel(W))
        assert W.size == self.N
        d = np.empty(self.N)
        ld = ctypes.c_double(0.0)
        rc = check(lib().mi355gp_laplace_finish(self._h, W, float(extra_jitter), d, ctypes.byref(ld)), "mi355gp_laplace_finish")
        return rc, d, ld.value

    def laplace_gradients(self, Ki_f, dL_dfhat):
        """dL/dtheta of every part (concatenated) from the device-resident dL_dK (reference `laplace.py:257-272`)."""
        Ki_f, s = f64(np.ravel(Ki_f)), f64(np.ravel(dL_dfhat))
        assert Ki_f.size == self.N and s.size == self.N
        dtheta = np.zeros(self._lap_ntheta)
        check(lib().mi355gp_laplace_gradients(self._h, Ki_f, s, dtheta), "mi355gp_laplace_gradients")
        return dtheta

    def laplace_implicit(self, dL_dfhat):
        """s = K (dL_dfhat - K_Wi_i K dL_dfhat): the implicit term of every likelihood-parameter gradient is s . g_i
        (reference `laplace.py:293-295`, where it is dL_dfhat^T (I - K K_Wi_i) K g_i)."""
        d = f64(np.ravel(dL_dfhat))
        assert d.size == self.N
        s = np.empty(self.N)
        check(lib().mi355gp_laplace_implicit(self._h, d, s), "mi355gp_laplace_implicit")
        return s

    def laplace_predict(self, specs, Xnew, wv, full_cov=False, want_var=True):
        """`Posterior._raw_predict` for the Laplace posterior (reference `laplace.py:146`, `posterior.py:198-262`)."""
        arr, keep, _ = make_parts(specs)
        wv = f64(np.ravel(wv))
        assert wv.size == self.N
        return _predict("mi355gp_laplace_predict", (self._h, len(specs), arr), Xnew, self.D, 1, full_cov, want_var,
                        between=(wv,))

    # ---- VarGauss inside a Laplace session (include/mi355gp_vargauss.h: begin, then forward / backward per evaluation) ----
    def vargauss_forward(self, alpha, beta, extra_jitter=0.0):
        """The N x N half of reference `var_gauss.py:34-41,54`: (info, m = K alpha, diag Sigma, log det A, tr A^-1, m^T alpha)
        for A = I + diag(beta) K diag(beta); beta is signed."""
        alpha, beta = f64(np.ravel(alpha)), f64(np.ravel(beta))
        assert alpha.size == self.N and beta.size == self.N
        m, var, scal = np.empty(self.N), np.empty(self.N), np.zeros(3)
        rc = check(lib().mi355gp_vargauss_forward(self._h, alpha, beta, float(extra_jitter), m, var, scal),
                   "mi355gp_vargauss_forward")
        return rc, m, var, scal[0], scal[1], scal[2]

    def vargauss_backward(self, dF_dm, dF_dv, exact=False):
        """Reference `var_gauss.py:48-65`: (alpha.gradient, beta.gradient, dL/dtheta of every part) from the symmetrised
        dL_dK, which stays on the device.  `exact`: the dF_dv term of dL_dK as the derivative of the bound, T diag(dF_dv) T^T,
        instead of the reference's row-scaled (T o dF_dv) T^T (`mi355gp_vargauss_backward_exact`)."""
        g, v = f64(np.ravel(dF_dm)), f64(np.ravel(dF_dv))
        assert g.size == self.N and v.size == self.N
        da, db, dtheta = np.empty(self.N), np.empty(self.N), np.zeros(self._lap_ntheta)
        entry = "mi355gp_vargauss_backward_exact" if exact else "mi355gp_vargauss_backward"
        check(getattr(lib(), entry)(self._h, g, v, da, db, dtheta), entry)
        return da, db, dtheta

    # ---- EP inside a Laplace session (include/mi355gp.h: recompute, sweep; the final pass is newton / finish / gradients) ----
    def ep_recompute(self, tau, v, extra_jitter=0.0, add_diag=0.0, want_sigma=True, want_ms=False):
        """`posteriorParams._recompute` (reference `expectation_propagation.py:129-143`): (info, mu, diag(Sigma), logdet B[, ms]);
        with `want_sigma` the full Sigma stays on the device for `ep_sweep`."""
        tau, v = f64(np.ravel(tau)), f64(np.ravel(v))
        assert tau.size == self.N and v.size == self.N
        mu, sd = np.empty(self.N), np.empty(self.N)
        ld, ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = check(lib().mi355gp_ep_recompute(self._h, tau, v, float(extra_jitter), float(add_diag), int(bool(want_sigma)), mu, sd,
                                              ctypes.byref(ld), ctypes.byref(ms)), "mi355gp_ep_recompute")
        return (rc, mu, sd, ld.value) + ((ms.value,) if want_ms else ())

    def ep_sweep(self, order, ysign, tau, v, eta=1.0, delta=1.0, lik=EP_BERNOULLI_PROBIT, want_ms=False):
        """One sequential pass of `_local_updates` (reference `expectation_propagation.py:330-351`) on the device:
        dict(tau, v (updated copies), cav_tau, cav_v, log_Z_hat, mu, Sigma_diag[, ms])."""
        order = np.ascontiguousarray(np.ravel(order), dtype=np.int64)
        ysign = f64(np.ravel(ysign))
        tau, v = f64(np.ravel(tau)).copy(), f64(np.ravel(v)).copy()
        assert order.size == self.N and ysign.size == self.N and tau.size == self.N and v.size == self.N
        o = [np.empty(self.N) for _ in range(5)]
        ms = ctypes.c_double(0.0)
        check(lib().mi355gp_ep_sweep(self._h, int(lik), order, ysign, float(eta), float(delta), tau, v, o[0], o[1], o[2], o[3], o[4],
                                     ctypes.byref(ms)), "mi355gp_ep_sweep")
        r = dict(tau=tau, v=v, cav_tau=o[0], cav_v=o[1], log_Z_hat=o[2], mu=o[3], Sigma_diag=o[4])
        if want_ms:
            r["ms"] = ms.value
        return r

    def set_option(self, name, value):
        """Options of THIS context through the C-ABI (`mi355gp_set_option`; the MI355GP_* environment variables only give the
        process-wide defaults).  'profile': 0 = off, 1 = every kernel family, or a tuple of family names; 'lookahead': 0/1;
        the schedule switches of OPTIONS take an int, -1 = back to the process default."""
        if name == "profile" and not isinstance(value, (int, bool)):
            value = sum(1 << PROFILE_FAMILIES.index(f) for f in value) << 1
        check(lib().mi355gp_set_option(self._h, OPTIONS[name], int(value)), "mi355gp_set_option")

    def get_option(self, name):
        v = ctypes.c_int(0)
        check(lib().mi355gp_get_option(self._h, OPTIONS[name], ctypes.byref(v)), "mi355gp_get_option")
        return int(v.value)

    def get_profile(self):
        """{family: (ms, algorithmic flops, launches)} of the last inference call made with option 'profile' on."""
        ms, fl, n = np.zeros(8), np.zeros(8), np.zeros(8, dtype=np.int32)
        check(lib().mi355gp_get_profile(self._h, ms, fl, n), "mi355gp_get_profile")
        return {k: (ms[i], fl[i], int(n[i])) for i, k in enumerate(PROFILE_FAMILIES)}

    def predict(self, kind, ARD, theta, Xnew, full_cov=False, want_var=True):
        """(mu (M x Dy), var (M x 1) or cov (M x M)) of the latent function at Xnew, computed on the device."""
        return _predict("mi355gp_predict", (self._h, KIND_IDS[kind], ard_id(kind, ARD), f64(theta)), Xnew, self.D, self.Dy,
                        full_cov, want_var)

    def fetch(self, which, fortran_order=False):
        out = np.empty((self.N, self.N))
        check(lib().mi355gp_fetch(self._h, which, out, int(fortran_order)), "mi355gp_fetch")
        if fortran_order:
            return out.T      # same memory viewed as an F-contiguous array
        return out


class SparseContext(_Handle):
    """One device context of the sparse (VarDTC) path = one uploaded (X, Y); Z and theta change per call."""
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = 0, 1, 2, 3, 4, 5
    sharded = False
    _create, _destroy = "mi355gp_sparse_create", "mi355gp_sparse_destroy"

    def __init__(self, device=0):
        super(SparseContext, self).__init__(device)
        self.N = self.D = self.Dy = self.M = 0

    def attach_comm(self, rank, world, id_bytes):
        """Row-sharded multi-GPU mode: this rank will upload only its slice of (X, Y) (see gpy_amd.grid.shard_rows)."""
        check(lib().mi355gp_sparse_attach_comm(self._h, rank, world, id_bytes), "mi355gp_sparse_attach_comm")
        self.sharded = True

    def set_data(self, X, Y):
        X, Y = f64(X), f64(Y)
        self.N, self.D = X.shape
        self.Dy = Y.shape[1]
        check(lib().mi355gp_sparse_set_data(self._h, X, self.N, self.D, Y, self.Dy), "mi355gp_sparse_set_data")

    def get_profile(self):
        """Launch timing of the two MFMA kernels of the LAST vardtc call (hipEvent pairs on the launching stream):
        {"gemm_T": (ms, algorithmic flops, launches), "gram_psi2": (...)} (`mi355gp_sparse_get_profile`)."""
        o = np.zeros(6)
        check(lib().mi355gp_sparse_get_profile(self._h, o), "mi355gp_sparse_get_profile")
        return {"gemm_T": (o[0], o[1], int(o[2])), "gram_psi2": (o[3], o[4], int(o[5]))}

    def _fit(self, entry, head, ntheta, Z, scalars, extras, want_stage_ms, wv_cols=None):
        """the shared part of the four fit entries, which all run (ctx, *head, Z, M, *scalars, out, dtheta, dZ, woodbury_vector,
        *extras (optional outputs), ms): (info, out, dict(lml, dnoise, dtheta, dZ, woodbury_vector[, stage_ms]))"""
        Z = f64(Z)
        self.M = Z.shape[0]
        assert Z.shape[1] == self.D
        out = np.zeros(NUM_OUT)
        dtheta = np.zeros(ntheta)
        dZ = np.zeros((self.M, self.D))
        wv = np.zeros((self.M, self.Dy if wv_cols is None else wv_cols))
        ms = np.zeros(4) if want_stage_ms else None
        args = tuple(head) + (Z, self.M) + tuple(scalars) + (out, _opt(dtheta), _opt(dZ), _opt(wv))
        rc = check(getattr(lib(), entry)(self._h, *(args + tuple(_opt(e) for e in extras) + (_opt(ms),))), entry)
        res = dict(lml=out[0], dnoise=out[1], dtheta=dtheta, dZ=dZ, woodbury_vector=wv)
        if ms is not None:
            res["stage_ms"] = dict(pass1=ms[0], mxm=ms[1], pass2=ms[2], total=ms[3])
        return rc, out, res

    def vardtc(self, kind, ARD, theta, Z, noise_var, extra_jitter=0.0, want_stage_ms=False):
        """(info, dict(lml, dnoise, dtheta, dZ, woodbury_vector[, stage_ms]))"""
        theta = f64(theta)
        rc, out, res = self._fit("mi355gp_vardtc_inference", (KIND_IDS[kind], int(bool(ARD)), theta), theta.size, Z,
                                 (float(noise_var), float(extra_jitter)), (), want_stage_ms)
        res.update(trA=out[2], data_fit=out[3])
        return rc, res

    def fetch(self, which):
        out = np.empty((self.M, self.M))
        check(lib().mi355gp_sparse_fetch(self._h, which, out), "mi355gp_sparse_fetch")
        return out

    def attach_loopback(self, rank, world, group_key):
        """Row-sharded mode over the in-process loopback transport (one host thread per logical rank)."""
        check(lib().mi355gp_sparse_attach_loopback(self._h, rank, world, int(group_key)), "mi355gp_sparse_attach_loopback")
        self.sharded = True

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, want_dL_dm=False, want_stage_ms=False):
        """Sum-of-parts kernel (specs as for `Context.exact_inference_sum`), scalar or per-point noise variances.
        (info, dict(lml, dnoise (scalar; per-point noise: the N-vector dL_dR, N x Dy for several output columns), dtheta
        (concatenated), dZ, woodbury_vector[, dL_dm, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        noise = f64(np.atleast_1d(noise)).ravel()
        rows = np.zeros((self.N, self.Dy)) if noise.size > 1 else None   # dL_dR per point and output column (var_dtc.py:240-256)
        dm = np.zeros((self.N, self.Dy)) if want_dL_dm else None
        rc, out, res = self._fit("mi355gp_vardtc_inference_sum", (len(specs), arr), ntheta, Z,
                                 (noise, noise.size, float(extra_jitter)), (rows, dm), want_stage_ms)
        if rows is not None:
            res["dnoise"] = rows[:, 0] if self.Dy == 1 else rows
        res.update(trA=out[2], data_fit=out[3], dL_dm=dm)
        return rc, res

    def set_input_variance(self, S):
        """Input variances (N x D, positive and finite) for the data of `set_data`, whose X is then the mean of q(x_n)."""
        S = f64(S)
        assert S.ndim == 2, "S must be N x D"
        check(lib().mi355gp_sparse_set_input_variance(self._h, S, S.shape[0], S.shape[1]), "mi355gp_sparse_set_input_variance")

    def set_inputs(self, X, S=None):
        """Replaces the inputs of `set_data` (and, with S, their variances); Y stays resident on the device."""
        X = f64(X)
        S = None if S is None else f64(S)
        assert X.ndim == 2 and (S is None or S.shape == X.shape), "X and S must be N x D"
        check(lib().mi355gp_sparse_set_inputs(self._h, X, _opt(S), X.shape[0], X.shape[1]), "mi355gp_sparse_set_inputs")

    def predict_uncertain(self, specs, mu_new, S_new, want_var=True):
        """(mean (M* x Dy), var (M* x Dy) or None) of the sparse posterior of the last call at points N(mu_new, diag S_new)."""
        arr, keep, _ = make_parts(specs)
        mu_new, S_new = f64(mu_new), f64(S_new)
        assert mu_new.ndim == 2 and mu_new.shape[1] == self.D and S_new.shape == mu_new.shape, "mu_new and S_new must be M* x D"
        Mn = mu_new.shape[0]
        mean = np.empty((Mn, self.Dy))
        var = np.empty((Mn, self.Dy)) if want_var else None
        check(lib().mi355gp_sparse_predict_uncertain(self._h, len(specs), arr, mu_new, S_new, Mn, mean, _opt(var)),
              "mi355gp_sparse_predict_uncertain")
        return mean, var

    def predict_ms(self):
        """HIP-event time (ms) of the stream work of the last `predict_uncertain` call"""
        out = np.zeros(1)
        check(lib().mi355gp_sparse_get_predict_ms(self._h, out.ctypes.data_as(_c_dp)), "mi355gp_sparse_get_predict_ms")
        return float(out[0])

    def vardtc_uncertain(self, specs, Z, noise, extra_jitter=0.0, want_dmu_dS=True, want_stage_ms=False):
        """One evaluation with uncertain inputs (one RBF part alone or with White parts, ONE noise variance).
        (info, dict(lml, dnoise, dtheta (concatenated), dZ, woodbury_vector, dmu, dS[, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        noise = f64(np.atleast_1d(noise)).ravel()
        dmu = np.zeros((self.N, self.D)) if want_dmu_dS else None
        dS = np.zeros((self.N, self.D)) if want_dmu_dS else None
        rc, out, res = self._fit("mi355gp_vardtc_inference_uncertain", (len(specs), arr), ntheta, Z,
                                 (noise, noise.size, float(extra_jitter)), (dmu, dS), want_stage_ms)
        res.update(trA=out[2], data_fit=out[3], dmu=dmu, dS=dS)
        return rc, res

    def set_output_groups(self, group_of_output, W):
        """The row masks of Y's columns for a fit with missing data (`mi355gp_sparse_set_output_groups`; `output_groups(Y)` makes
        them): group_of_output (Dy ints) and W (N x G, 0 / 1).  The Y of `set_data` holds 0 where unobserved.  None clears them."""
        if group_of_output is None:
            check(lib().mi355gp_sparse_set_output_groups(self._h, 0, None, None), "mi355gp_sparse_set_output_groups")
            self.G = 0
            return
        gof, W = np.ascontiguousarray(group_of_output, dtype=np.int32), f64(W)
        assert gof.shape == (self.Dy,) and W.ndim == 2 and W.shape[0] == self.N, "group_of_output has Dy entries, W is N x G"
        check(lib().mi355gp_sparse_set_output_groups(self._h, W.shape[1], gof.ctypes.data_as(_ip), _opt(W)), "mi355gp_sparse_set_output_groups")
        self.G, self.group_of_output = W.shape[1], gof.copy()

    def vardtc_missing(self, specs, Z, noise, extra_jitter=0.0, want_dmu_dS=True, want_stage_ms=False):
        """One evaluation with uncertain inputs and missing entries of Y (`set_output_groups` first; one RBF part alone or with
        White parts, ONE noise variance).  (info, dict(lml, dnoise, dtheta (concatenated), dZ, woodbury_vector, dmu, dS,
        group_scalars (G x 8: lml, dnoise, trA, data_fit, ... per group)[, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        noise = f64(np.atleast_1d(noise)).ravel()
        dmu = np.zeros((self.N, self.D)) if want_dmu_dS else None
        dS = np.zeros((self.N, self.D)) if want_dmu_dS else None
        rc, out, res = self._fit("mi355gp_vardtc_inference_missing", (len(specs), arr), ntheta, Z,
                                 (noise, noise.size, float(extra_jitter)), (dmu, dS), want_stage_ms)
        gs = np.zeros((self.G, NUM_OUT))
        check(lib().mi355gp_sparse_fetch_group_scalars(self._h, gs), "mi355gp_sparse_fetch_group_scalars")
        res.update(trA=out[2], data_fit=out[3], dmu=dmu, dS=dS, group_scalars=gs)
        return rc, res

    def select_output_group(self, g):
        """group g's woodbury_inv and psi2 become the context's current ones: `predict`, `predict_uncertain` and `fetch` then
        serve the outputs of that group (`mi355gp_sparse_select_output_group`)"""
        check(lib().mi355gp_sparse_select_output_group(self._h, int(g)), "mi355gp_sparse_select_output_group")

    def predict_missing(self, specs, Xnew, S_new=None):
        """(mean, variance), both M* x Dy, of the posterior of the last `vardtc_missing` call at certain points or at
        N(Xnew, diag S_new): the mean from all Woodbury columns, output d's variance from its group's woodbury_inv
        (`posterior.py:243-246`, `:268`) -- one device contraction per group"""
        mean, var = None, None
        for g in range(self.G):
            self.select_output_group(g)
            m, v = self.predict(specs, Xnew) if S_new is None else self.predict_uncertain(specs, Xnew, S_new)
            if var is None:
                mean, var = m, np.empty_like(m)
            d = np.nonzero(self.group_of_output == g)[0]
            var[:, d] = v if v.shape[1] == 1 else v[:, d]
        return mean, var

    def set_binary_prob(self, gamma):
        """Slab probabilities (N x D, strictly inside (0, 1)) next to the means and variances: spike-and-slab inputs
        (`mi355gp_sparse_set_binary_prob`).  None takes the context back to Gaussian inputs."""
        if gamma is None:
            check(lib().mi355gp_sparse_set_binary_prob(self._h, None, 0, 0), "mi355gp_sparse_set_binary_prob")
            return
        gamma = f64(gamma)
        assert gamma.ndim == 2, "gamma must be N x D"
        check(lib().mi355gp_sparse_set_binary_prob(self._h, _opt(gamma), gamma.shape[0], gamma.shape[1]),
              "mi355gp_sparse_set_binary_prob")

    def set_inputs_ss(self, X, S, gamma):
        """Replaces means, variances and slab probabilities (`mi355gp_sparse_set_inputs_ss`); Y stays resident on the device."""
        X, S, gamma = f64(X), f64(S), f64(gamma)
        assert X.ndim == 2 and S.shape == X.shape and gamma.shape == X.shape, "X, S and gamma must be N x D"
        check(lib().mi355gp_sparse_set_inputs_ss(self._h, X, S, gamma, X.shape[0], X.shape[1]), "mi355gp_sparse_set_inputs_ss")

    def vardtc_ss(self, specs, Z, noise, extra_jitter=0.0, want_dq=True, want_stage_ms=False):
        """One evaluation with spike-and-slab inputs (one RBF part alone or with White parts, ONE noise variance).
        (info, dict(lml, dnoise, dtheta (concatenated), dZ, woodbury_vector, dmu, dS, dgamma[, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        noise = f64(np.atleast_1d(noise)).ravel()
        dmu, dS, dg = (np.zeros((self.N, self.D)) if want_dq else None for _ in range(3))
        rc, out, res = self._fit("mi355gp_vardtc_inference_ss", (len(specs), arr), ntheta, Z,
                                 (noise, noise.size, float(extra_jitter)), (dmu, dS, dg), want_stage_ms)
        res.update(trA=out[2], data_fit=out[3], dmu=dmu, dS=dS, dgamma=dg)
        return rc, res

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        """(mu (M* x Dy), var (M* x 1) or cov) of the sparse posterior of the last call, on the device."""
        arr, keep, _ = make_parts(specs)
        return _predict("mi355gp_sparse_predict", (self._h, len(specs), arr), Xnew, self.D, self.Dy, full_cov, want_var)

    def fetch_dL_dKnm(self, row0, nrows):
        out = np.empty((nrows, self.M))
        check(lib().mi355gp_sparse_fetch_dLdKnm(self._h, int(row0), int(nrows), out), "mi355gp_sparse_fetch_dLdKnm")
        return out

    def set_linear(self, on=True):
        """Linear parts on this context's inference and prediction entry points (`mi355gp_sparse_set_linear`); off at first"""
        check(lib().mi355gp_sparse_set_linear(self._h, int(bool(on))), "mi355gp_sparse_set_linear")

    def set_coregionalize(self, on=True):
        """Coregionalize parts on this context's `vardtc_sum`, `predict` and `kdiag` (`mi355gp_sparse_set_coregionalize`); off at
        first.  Switch it on before `set_data`: the rows' output indices are checked against a host copy that set_data keeps."""
        check(lib().mi355gp_sparse_set_coregionalize(self._h, int(bool(on))), "mi355gp_sparse_set_coregionalize")

    def set_fuse_cols(self, on=True):
        """A/B switch of the second pass (`mi355gp_dbg_sparse_set_fuse_cols`, a diagnostic): off, the unfused routes -- for a
        stationary x Coregionalize term the product route in place of k_grad_cols_icm"""
        check(lib().mi355gp_dbg_sparse_set_fuse_cols(self._h, int(bool(on))), "mi355gp_dbg_sparse_set_fuse_cols")

    def set_psi_lin_bias(self, on=True):
        """One RBF or Linear part with Bias and White parts on this context's uncertain-input entry points
        (`mi355gp_sparse_set_psi_lin_bias`); off at first.  On also switches Linear on."""
        check(lib().mi355gp_sparse_set_psi_lin_bias(self._h, int(bool(on))), "mi355gp_sparse_set_psi_lin_bias")

    def kdiag(self, specs, w=None):
        """Kdiag of the expression at the context's rows (`mi355gp_sparse_kdiag`): kd (N), and with weights w (N) also
        (sum w kd, sum w^2 kd) and the gradient of sum w kd in the parts' parameters, concatenated in theta order --
        what `update_gradients_diag(w, X)` installs.  Returns kd, or (kd, sums, ddiag)."""
        arr, keep, ntheta = make_parts(specs)
        kd = np.empty(self.N)
        if w is None:
            check(lib().mi355gp_sparse_kdiag(self._h, len(specs), arr, None, _opt(kd), None, None), "mi355gp_sparse_kdiag")
            return kd
        w = f64(np.asarray(w)).ravel()
        assert w.size == self.N, "w must have one entry per row of X"
        sums, ddiag = np.zeros(2), np.zeros(ntheta)
        check(lib().mi355gp_sparse_kdiag(self._h, len(specs), arr, _opt(w), _opt(kd), _opt(sums), _opt(ddiag)), "mi355gp_sparse_kdiag")
        return kd, sums, ddiag

    # ---- EPDTC (epdtc.hip, include/mi355gp_epdtc.h) -------------------------------------------------------------------------
    def epdtc_begin(self, specs, Z, jitter=0.0):
        """The part list, Z and Kmm + jitter I, factored: (info, {})."""
        arr, keep, _ = make_parts(specs)
        Z = f64(Z)
        self.M = Z.shape[0]
        assert Z.shape[1] == self.D
        return check(lib().mi355gp_epdtc_begin(self._h, len(specs), arr, Z, self.M, float(jitter)), "mi355gp_epdtc_begin"), {}

    def epdtc_recompute(self, tau, v, want_ms=False):
        """`posteriorParamsDTC._recompute` for the site parameters (tau, v): (info, mu, Sigma_diag[, ms])."""
        mu, sd, ms = np.empty(self.N), np.empty(self.N), np.zeros(1)
        rc = check(lib().mi355gp_epdtc_recompute(self._h, f64(tau), f64(v), mu, sd, _opt(ms)), "mi355gp_epdtc_recompute")
        return (rc, mu, sd, float(ms[0])) if want_ms else (rc, mu, sd)

    def epdtc_sweep(self, order, ysign, tau, v, eta=1.0, delta=1.0, first=False, want_ms=False):
        """One sequential pass over the sites in `order`, from the P and gamma of the last recompute: dict(tau, v, cav_tau,
        cav_v, log_Z_hat, mu_hat, sigma2_hat[, ms])."""
        order = np.ascontiguousarray(order, dtype=np.int64)
        assert order.shape == (self.N,), "order must have N entries"
        tau, v = f64(tau).copy(), f64(v).copy()
        out = [np.empty(self.N) for _ in range(5)]
        ms = np.zeros(1)
        check(lib().mi355gp_epdtc_sweep(self._h, order, f64(ysign), float(eta), float(delta), int(bool(first)), tau, v, *out,
                                        _opt(ms)), "mi355gp_epdtc_sweep")
        r = dict(zip(("cav_tau", "cav_v", "log_Z_hat", "mu_hat", "sigma2_hat"), out), tau=tau, v=v)
        if want_ms:
            r["ms"] = float(ms[0])
        return r

    def epdtc_inference(self, specs, Z, tau, v, jitter=0.0, want_stage_ms=False):
        """The VarDTC evaluation of the sites (targets v / tau, precisions tau, `jitter` the whole term on Kmm's diagonal):
        (info, dict(lml (without log Z_tilde), dL_dR (N), dtheta (concatenated), dZ, woodbury_vector[, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        dR = np.zeros(self.N)
        rc, out, res = self._fit("mi355gp_epdtc_inference", (len(specs), arr), ntheta, Z, (f64(tau), f64(v), float(jitter)), (dR,),
                                 want_stage_ms)
        res["dL_dR"] = dR
        return rc, res

    # ---- PEP / FITC (pep.hip) ---------------------------------------------------------------------------------------------
    def pep(self, specs, Z, noise_variance, alpha, jitter, want_stage_ms=False):
        """One `PEP.inference` (alpha = 1: `FITC.inference`) with one noise variance; `jitter` is the whole term on Kmm's
        diagonal.  (info, dict(lml, dnoise (= dL_dthetaL), dL_dR (N), dtheta (concatenated), dZ, woodbury_vector[, stage_ms]))"""
        arr, keep, ntheta = make_parts(specs)
        dR = np.zeros(self.N)
        rc, out, res = self._fit("mi355gp_pep_inference", (len(specs), arr), ntheta, Z,
                                 (float(noise_variance), float(alpha), float(jitter)), (dR,), want_stage_ms, wv_cols=1)
        res.update(sum_dL_dR=out[2], dL_dR=dR)
        return rc, res

    # ---- SVGP: forward -> the likelihood's quadrature on the host -> backward (svgp.hip) ------------------------------------
    def svgp_forward(self, specs, Z, q_mean, q_chol, extra_jitter=0.0, want_stage_ms=False):
        """q_mean: M x L; q_chol: L x M x M lower-triangular factors.  (info, dict(mu (N x L), v (N x L), KL, logdet_Kmm,
        logdet_S (L)[, stage_ms])); info > 0: Kmm is not positive definite, retry with `extra_jitter`."""
        arr, keep, ntheta = make_parts(specs)
        Z, q_mean, q_chol = f64(Z), f64(q_mean), f64(q_chol)
        self.M = Z.shape[0]
        assert Z.shape[1] == self.D
        assert q_mean.ndim == 2 and q_mean.shape[0] == self.M, "q_mean must be M x L"
        L = q_mean.shape[1]
        assert q_chol.shape == (L, self.M, self.M), "q_chol must be L x M x M"
        self.L, self._svgp_ntheta = L, ntheta
        mu, v = np.zeros((self.N, L)), np.zeros((self.N, L))
        sc = np.zeros(2 + L)
        ms = np.zeros(3) if want_stage_ms else None
        rc = check(lib().mi355gp_svgp_forward(self._h, len(specs), arr, Z, self.M, q_mean, q_chol, L, float(extra_jitter), mu, v,
                                              sc, _opt(ms)), "mi355gp_svgp_forward")
        res = dict(mu=mu, v=v, KL=sc[0], logdet_Kmm=sc[1], logdet_S=sc[2:2 + L].copy())
        if ms is not None:
            res["stage_ms"] = dict(mxm=ms[0], rows=ms[1], total=ms[2])
        return rc, res

    def svgp_backward(self, dF_dmu, dF_dv, want_stage_ms=False):
        """dF_dmu, dF_dv: N x L, already times batch_scale.  dict(dtheta (concatenated), dZ, dL_dm (M x L), dL_dchol
        (L x M x M, lower triangles)[, stage_ms]) after `svgp_forward` on the same data."""
        L = getattr(self, "L", 0)
        dF_dmu, dF_dv = f64(dF_dmu), f64(dF_dv)
        if L:
            assert dF_dmu.shape == (self.N, L) and dF_dv.shape == (self.N, L), "dF_dmu and dF_dv must be N x L"
        dtheta = np.zeros(getattr(self, "_svgp_ntheta", 0))
        dZ, dm, dchol = np.zeros((self.M, self.D)), np.zeros((self.M, L)), np.zeros((L, self.M, self.M))
        ms = np.zeros(3) if want_stage_ms else None
        check(lib().mi355gp_svgp_backward(self._h, dF_dmu, dF_dv, _opt(dtheta), _opt(dZ), _opt(dm), _opt(dchol), _opt(ms)),
              "mi355gp_svgp_backward")
        res = dict(dtheta=dtheta, dZ=dZ, dL_dm=dm, dL_dchol=dchol)
        if ms is not None:
            res["stage_ms"] = dict(rows=ms[0], mxm=ms[1], total=ms[2])
        return res

    def svgp_predict(self, specs, Xnew, full_cov=False, want_var=True):
        """(mu (M* x L), var (M* x L) or cov (M* x M* x L) or None) of the SVGP posterior of the last `svgp_forward`."""
        arr, keep, _ = make_parts(specs)
        Xnew = f64(Xnew)
        Mn, L = Xnew.shape[0], getattr(self, "L", 1)
        assert Xnew.shape[1] == self.D
        mu = np.empty((Mn, L))
        var = (np.empty((Mn, Mn, L)) if full_cov else np.empty((Mn, L))) if want_var else None
        check(lib().mi355gp_svgp_predict(self._h, len(specs), arr, Xnew.ctypes.data_as(_c_dp), Mn, int(bool(full_cov)),
                                         mu.ctypes.data_as(_c_dp), _opt(var), None, None), "mi355gp_svgp_predict")
        return mu, var

    def svgp_woodbury(self, want_inv=True):
        """(woodbury_vector = Kmm^-1 m (M x L), woodbury_inv (M x M x L, the reference's axis order) or None) of the last
        `svgp_forward`"""
        L = getattr(self, "L", 1)
        wv = np.empty((self.M, L))
        wi = np.empty((L, self.M, self.M)) if want_inv else None
        check(lib().mi355gp_svgp_predict(self._h, 0, None, None, 0, 0, None, None, wv.ctypes.data_as(_c_dp), _opt(wi)),
              "mi355gp_svgp_predict")
        return wv, (None if wi is None else np.ascontiguousarray(np.transpose(wi, (1, 2, 0))))


def _point_sets(X, X2, dL_dK=None):
    """the (X, N, X2 or NULL, M, D) run of the three kernel functions, X2 = None standing for X itself; with `dL_dK`, that
    matrix checked against N x M comes first"""
    X = f64(X)
    N, D = X.shape
    if X2 is None:
        M, p2 = N, None
    else:
        X2 = f64(X2)
        M, p2 = X2.shape[0], X2.ctypes.data_as(_c_dp)        # (the pointer keeps the converted X2 alive)
        assert X2.shape[1] == D
    if dL_dK is None:
        return X, N, p2, M, D
    G = f64(dL_dK)
    assert G.shape == (N, M), "dL_dK must be N x M"
    return G, X, N, p2, M, D


def kern_K(kind, ARD, theta, X, X2=None, device=0):
    require_device(device)
    sets = _point_sets(X, X2)
    out = np.empty((sets[1], sets[3]))
    check(lib().mi355gp_kern_K(device, KIND_IDS[kind], ard_id(kind, ARD), f64(theta), *(sets + (out,))), "mi355gp_kern_K")
    return out


def kern_Kdiag(kind, theta, N):
    out = np.empty(N)
    check(lib().mi355gp_kern_Kdiag(KIND_IDS[kind], f64(theta), N, out), "mi355gp_kern_Kdiag")
    return out


def update_gradients_full(kind, ARD, theta, dL_dK, X, X2=None, device=0):
    require_device(device)
    theta = f64(theta)
    out = np.zeros(theta.size)
    check(lib().mi355gp_update_gradients_full(device, KIND_IDS[kind], ard_id(kind, ARD), theta,
                                              *(_point_sets(X, X2, dL_dK) + (out,))), "mi355gp_update_gradients_full")
    return out


def gradients_X(kind, ARD, theta, dL_dK, X, X2=None, device=0):
    """dL/dX (N x D) from dL_dK (N x M) (reference `Stationary.gradients_X`, stationary.py:245-252)."""
    require_device(device)
    sets = _point_sets(X, X2, dL_dK)
    out = np.zeros(sets[1].shape)
    check(lib().mi355gp_gradients_X(device, KIND_IDS[kind], ard_id(kind, ARD), f64(theta), *(sets + (out,))),
          "mi355gp_gradients_X")
    return out


def _psi_args(variance, lengthscale, ARD, Z, mu, S, weights):
    Z, mu, S = f64(Z), f64(mu), f64(S)
    N, D = mu.shape
    assert S.shape == mu.shape and Z.ndim == 2 and Z.shape[1] == D, "Z is M x D, mu and S are N x D"
    ls = theta_vec(variance, lengthscale, ARD, D)[1:]
    w = None if weights is None else f64(np.ravel(weights))
    assert w is None or w.size == N
    return (float(np.ravel(variance)[0]), f64(ls), int(bool(ARD)), Z, Z.shape[0], mu, S, N, D, _opt(w)), w


def rbf_psi(variance, lengthscale, ARD, Z, mu, S, weights=None, want_psi1=True, want_psi2=True, device=0):
    """(psi1 (N x M) or None, psi2 = sum_n w_n psi2n (M x M) or None) of an RBF kernel for inputs N(mu, diag S)
    (reference `rbf_psi_comp.py:22-50`), on the device."""
    require_device(device)
    args, keep = _psi_args(variance, lengthscale, ARD, Z, mu, S, weights)
    M, N = args[4], args[7]
    p1 = np.empty((N, M)) if want_psi1 else None
    p2 = np.empty((M, M)) if want_psi2 else None
    check(lib().mi355gp_rbf_psi(device, *(args + (_opt(p1), _opt(p2)))), "mi355gp_rbf_psi")
    return p1, p2


def rbf_psi_grad(variance, lengthscale, ARD, Z, mu, S, dL_dpsi0=None, dL_dpsi1=None, dL_dpsi2=None, weights=None, device=0):
    """(dvariance, dlengthscale, dZ, dmu, dS) from dL_dpsi0 (N), dL_dpsi1 (N x M), dL_dpsi2 (M x M)
    (reference `rbf_psi_comp.py:70-133`), on the device."""
    require_device(device)
    args, keep = _psi_args(variance, lengthscale, ARD, Z, mu, S, weights)
    M, N, D = args[4], args[7], args[8]
    d0 = None if dL_dpsi0 is None else f64(np.ravel(dL_dpsi0))
    d1 = None if dL_dpsi1 is None else f64(dL_dpsi1)
    d2 = None if dL_dpsi2 is None else f64(dL_dpsi2)
    assert d0 is None or d0.size == N
    assert d1 is None or d1.shape == (N, M), "dL_dpsi1 must be N x M"
    assert d2 is None or d2.shape == (M, M), "dL_dpsi2 must be M x M"
    dvar, dl = np.zeros(1), np.zeros(D if ARD else 1)
    dZ, dmu, dS = np.zeros((M, D)), np.zeros((N, D)), np.zeros((N, D))
    check(lib().mi355gp_rbf_psi_grad(device, *(args + (_opt(d0), _opt(d1), _opt(d2), dvar, dl, dZ, dmu, dS))),
          "mi355gp_rbf_psi_grad")
    return dvar[0], dl, dZ, dmu, dS


def output_groups(Y):
    """(group_of_output (Dy ints), W (N x G, 0 / 1), Y with 0 for NaN) of an output matrix with NaN where unobserved: columns with
    the same observed rows share a group, groups in order of their first column (`stochastics.py:57-79`)"""
    Y = np.asarray(Y, dtype=np.float64)
    obs = ~np.isnan(Y)
    first, gof = {}, np.empty(Y.shape[1], dtype=np.int32)
    for d in range(Y.shape[1]):
        gof[d] = first.setdefault(obs[:, d].tobytes(), len(first))
    W = np.stack([obs[:, int(np.argmax(gof == g))] for g in range(len(first))], axis=1).astype(np.float64)
    return gof, W, np.where(obs, Y, 0.0)


def psi_groups_batch():
    """groups one launch of a group-batched psi2 kernel carries (PSI_GB of csrc/psi_missing.h)"""
    return int(lib().mi355gp_psi_groups_batch())


def _group_args(variance, lengthscale, ARD, Z, mu, S, W):
    args, _ = _psi_args(variance, lengthscale, ARD, Z, mu, S, None)
    W = f64(W)
    assert W.ndim == 2 and W.shape[0] == args[7] and W.shape[1] >= 1, "W is N x G, one 0/1 column per group"
    return args[:9] + (W, W.shape[1])


def rbf_psi2_groups(variance, lengthscale, ARD, Z, mu, S, W, loop=False, device=0, want_ms=False):
    """psi2_g = sum_n W[n, g] psi2n for every group g (G x M x M) of an RBF kernel for inputs N(mu, diag S): the psi2 side of a
    fit with missing data (reference `sparse_gp_minibatch.py:228-286`), every exponential evaluated once for a batch of groups.
    `loop=True` (a diagnostic): the single-mask kernel once per group instead, the route the batched kernel replaces; `want_ms`:
    also the stream time of the psi2 kernels."""
    require_device(device)
    args = _group_args(variance, lengthscale, ARD, Z, mu, S, W)
    M, G = args[4], args[10]
    out, ms = np.empty((G, M, M)), ctypes.c_double(0.0)
    if loop or want_ms:                                              # the diagnostic entry (include/mi355gp_debug_sparse_missing.h)
        check(lib().mi355gp_dbg_rbf_psi2_groups(device, *(args + (int(bool(loop)), out, ctypes.byref(ms)))), "mi355gp_dbg_rbf_psi2_groups")
    else:
        check(lib().mi355gp_rbf_psi2_groups(device, *(args + (out,))), "mi355gp_rbf_psi2_groups")
    return (out, ms.value) if want_ms else out


def rbf_psi_grad_groups(variance, lengthscale, ARD, Z, mu, S, W, dL_dpsi2, loop=False, device=0, want_ms=False):
    """(dvariance, dlengthscale, dZ, dmu, dS) of sum_g sum(dL_dpsi2[g] * psi2_g), psi2_g = sum_n W[n, g] psi2n: the chain rule of
    `rbf_psi_comp.py:70-133` with the per-row dL_dpsi2[n] = sum_g W[n, g] dL_dpsi2[g] (each G x M x M matrix symmetrised inside)."""
    require_device(device)
    args = _group_args(variance, lengthscale, ARD, Z, mu, S, W)
    M, N, D, G = args[4], args[7], args[8], args[10]
    d2 = f64(dL_dpsi2)
    assert d2.shape == (G, M, M), "dL_dpsi2 must be G x M x M"
    dvar, dl, ms = np.zeros(1), np.zeros(D if ARD else 1), ctypes.c_double(0.0)
    dZ, dmu, dS = np.zeros((M, D)), np.zeros((N, D)), np.zeros((N, D))
    if loop or want_ms:                                              # the diagnostic entry
        check(lib().mi355gp_dbg_rbf_psi_grad_groups(device, *(args + (d2, int(bool(loop)), dvar, dl, dZ, dmu, dS, ctypes.byref(ms)))),
              "mi355gp_dbg_rbf_psi_grad_groups")
    else:
        check(lib().mi355gp_rbf_psi_grad_groups(device, *(args + (d2, dvar, dl, dZ, dmu, dS))), "mi355gp_rbf_psi_grad_groups")
    r = (dvar[0], dl, dZ, dmu, dS)
    return r + (ms.value,) if want_ms else r


def _ss_args(variance, lengthscale, ARD, Z, mu, S, gamma, weights):
    args, w = _psi_args(variance, lengthscale, ARD, Z, mu, S, weights)
    gamma = f64(gamma)
    assert gamma.shape == args[5].shape, "gamma is N x D, as mu and S"
    return args[:7] + (gamma,) + args[7:], w


def ssrbf_psi(variance, lengthscale, ARD, Z, mu, S, gamma, weights=None, want_psi1=True, want_psi2=True, device=0):
    """(psi1 (N x M) or None, psi2 = sum_n w_n psi2n (M x M) or None) of an RBF kernel for spike-and-slab inputs
    gamma N(mu, diag S) + (1 - gamma) delta_0 (reference `ssrbf_psi_comp.py:209-288`), on the device."""
    require_device(device)
    args, keep = _ss_args(variance, lengthscale, ARD, Z, mu, S, gamma, weights)
    M, N = args[4], args[8]
    p1 = np.empty((N, M)) if want_psi1 else None
    p2 = np.empty((M, M)) if want_psi2 else None
    check(lib().mi355gp_ssrbf_psi(device, *(args + (_opt(p1), _opt(p2)))), "mi355gp_ssrbf_psi")
    return p1, p2


def ssrbf_psi_grad(variance, lengthscale, ARD, Z, mu, S, gamma, dL_dpsi0=None, dL_dpsi1=None, dL_dpsi2=None, weights=None,
                   device=0):
    """(dvariance, dlengthscale, dZ, dmu, dS, dgamma) from dL_dpsi0 (N), dL_dpsi1 (N x M), dL_dpsi2 (M x M, symmetrised inside)
    (reference `ssrbf_psi_comp.py:290-398`), on the device."""
    require_device(device)
    args, keep = _ss_args(variance, lengthscale, ARD, Z, mu, S, gamma, weights)
    M, N, D = args[4], args[8], args[9]
    d0 = None if dL_dpsi0 is None else f64(np.ravel(dL_dpsi0))
    d1 = None if dL_dpsi1 is None else f64(dL_dpsi1)
    d2 = None if dL_dpsi2 is None else f64(dL_dpsi2)
    assert d0 is None or d0.size == N
    assert d1 is None or d1.shape == (N, M), "dL_dpsi1 must be N x M"
    assert d2 is None or d2.shape == (M, M), "dL_dpsi2 must be M x M"
    dvar, dl = np.zeros(1), np.zeros(D if ARD else 1)
    dZ, dmu, dS, dg = np.zeros((M, D)), np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, D))
    check(lib().mi355gp_ssrbf_psi_grad(device, *(args + (_opt(d0), _opt(d1), _opt(d2), dvar, dl, dZ, dmu, dS, dg))),
          "mi355gp_ssrbf_psi_grad")
    return dvar[0], dl, dZ, dmu, dS, dg


def potrf(A, device=0):
    """Lower Cholesky factor of A (dpotrf equivalent) -> (L, info, ms)."""
    require_device(device)
    L = f64(A).copy()
    ms = ctypes.c_double(0.0)
    info = check(lib().mi355gp_potrf(device, L, L.shape[0], ctypes.byref(ms)), "mi355gp_potrf")
    return L, info, ms.value


def pdinv(A, device=0):
    """(Ainv, L, logdet, info, ms): pdinv equivalent (GPy/util/linalg.py:193-214)."""
    require_device(device)
    A = f64(A)
    n = A.shape[0]
    Ai, L = np.empty((n, n)), np.empty((n, n))
    ld, ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
    info = check(lib().mi355gp_pdinv(device, A, n, Ai.ctypes.data_as(_c_dp), L.ctypes.data_as(_c_dp),
                                     ctypes.byref(ld), ctypes.byref(ms)), "mi355gp_pdinv")
    return Ai, L, ld.value, info, ms.value


def pdinv_full(A, device=0):
    """(Ainv, L, Li, logdet, info): all four members of GPy's pdinv tuple (GPy/util/linalg.py:193-214)."""
    require_device(device)
    A = f64(A)
    n = A.shape[0]
    Ai, L, Li = np.empty((n, n)), np.empty((n, n)), np.empty((n, n))
    ld, ms = ctypes.c_double(0.0), ctypes.c_double(0.0)
    info = check(lib().mi355gp_pdinv_full(device, A, n, Ai.ctypes.data_as(_c_dp), L.ctypes.data_as(_c_dp),
                                          Li.ctypes.data_as(_c_dp), ctypes.byref(ld), ctypes.byref(ms)), "mi355gp_pdinv_full")
    return Ai, L, Li, ld.value, info


def bench_factor(N, reps=3, device=0):
    """Device-only timing of potrf / trtri / lauum on a synthetic SPD matrix: dict of ms and TFLOP/s (N^3/3 each)."""
    require_device(device)
    p, t, l = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(lib().mi355gp_bench_factor(device, N, reps, ctypes.byref(p), ctypes.byref(t), ctypes.byref(l)),
          "mi355gp_bench_factor")
    fl = float(N) ** 3 / 3.0
    return {"potrf_ms": p.value, "trtri_ms": t.value, "lauum_ms": l.value,
            "potrf_tflops": fl / p.value / 1e9, "trtri_tflops": fl / t.value / 1e9, "lauum_tflops": fl / l.value / 1e9}


def dbg_persist(N, reps=3, kcap=0, device=0):
    """The persistent dataflow Cholesky (persist.hip) next to the launch-per-step schedule on the same resident SPD matrix:
    dict(ms_steps, ms_persist, mismatches (doubles of the lower triangle of L that differ BITWISE), info, steps = per chain
    step the six wall-clock stamps in microseconds relative to the first)."""
    require_device(device)
    nt = (int(N) + 127) // 128
    out = np.zeros(8 + 32 * nt)
    check(lib().mi355gp_dbg_persist(device, int(N), int(reps), int(kcap), out), "mi355gp_dbg_persist")
    st = out[8:8 + 8 * nt].reshape(nt, 8)
    near = out[8 + 8 * nt:8 + 20 * nt].reshape(nt, 3, 4)   # [..., 3] of entry (j+1, 0): the chain published row j+1
    far = out[8 + 20 * nt:].reshape(nt, 12)                # far tile (i, i-3): last pass picked / done, solve picked / staged / solved / published
    return dict(ms_steps=out[0], ms_persist=out[1], mismatches=int(out[2]), info=int(out[3]), abort=int(out[4]), nt=nt,
                steps=(st - st[0, 0]) / 100.0, near=(near - st[0, 0]) / 100.0, far=(far - st[0, 0]) / 100.0)


def dbg_mask_probe(pct=75, order=0, device=0):
    """ms of a 4096^3 GEMM on (plain, CU-masked, CU-masked again) streams: is the mask in force?"""
    require_device(device)
    out = np.zeros(3)
    check(lib().mi355gp_dbg_mask_probe(device, pct, order, out), "mi355gp_dbg_mask_probe")
    return out


def dbg_mfma(a, b, device=0):
    require_device(device)
    d = np.zeros(256)
    check(lib().mi355gp_dbg_mfma(device, f64(a), f64(b), d), "dbg_mfma")
    return d.reshape(64, 4)


def dbg_gemm(A, B, C, a_mcontig, b_ncontig, alpha=1.0, beta=0.0, reps=0, device=0):
    """C = alpha*op(A) op(B) + beta*C.  A: (M,K) [k-contig] or (K,M) [m-contig]; B: (N,K) or (K,N)."""
    require_device(device)
    A, B, C = f64(A), f64(B), f64(C).copy()
    M, K = (A.shape[1], A.shape[0]) if a_mcontig else A.shape
    N = B.shape[1] if b_ncontig else B.shape[0]
    ms = ctypes.c_double(0.0)
    check(lib().mi355gp_dbg_gemm(device, int(a_mcontig), int(b_ncontig), M, N, K, A, B, C, alpha, beta, reps,
                                 ctypes.byref(ms)), "dbg_gemm")
    return C, ms.value


def dbg_gemm_clock():
    mhz, cyc = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(lib().mi355gp_dbg_gemm_clock(ctypes.byref(mhz), ctypes.byref(cyc)), "dbg_gemm_clock")
    return mhz.value, cyc.value


def dbg_peaks(device=0):
    require_device(device)
    out = np.zeros(8)
    check(lib().mi355gp_dbg_peaks(device, out), "dbg_peaks")
    return dict(mfma_f64_tflops=out[0], valu_f64_tflops=out[1], hbm_copy_gbs=out[2], hbm_fill_gbs=out[3],
                mfma_cycles_per_inst_1wave=out[4], shader_mhz_under_load=out[5], mfma_1wave_tflops=out[6],
                mfma_cycles_per_inst_loaded=out[7])


def dbg_grid_multi(T, nb=512, reps=3, device=0):
    """ms of the deep-K X^T X pass: [k_lauum row-major, grid kernel on two panel stores, on one panel store, grid kernel
    on the row-major matrix] (mi355gp_dbg_grid_multi)."""
    require_device(device)
    out = np.zeros(5)
    check(lib().mi355gp_dbg_grid_multi(device, int(T), int(nb), int(reps), out), "mi355gp_dbg_grid_multi")
    return out


def dbg_update_nt(nt, ks, reps=5, device=0):
    """ms per launch of the trailing-update kernel alone on the lower triangle of nt x nt tiles, one entry per panel depth."""
    require_device(device)
    ka = (ctypes.c_int * len(ks))(*[int(k) for k in ks])
    out = np.zeros(len(ks))
    check(lib().mi355gp_dbg_update_nt(device, int(nt), ka, len(ks), int(reps), out), "mi355gp_dbg_update_nt")
    return out


def dbg_update_rect(ntr, ntc, ks, reps=5, device=0):
    """the same for rows [ntc, ntr) x columns [0, ntc) of tiles (part 1 of a step: the next panel's columns)"""
    require_device(device)
    ka = (ctypes.c_int * len(ks))(*[int(k) for k in ks])
    out = np.zeros(len(ks))
    check(lib().mi355gp_dbg_update_rect(device, int(ntr), int(ntc), ka, len(ks), int(reps), out), "mi355gp_dbg_update_rect")
    return out


def persist_owners(nt, nw, tune=0):
    """Host only: the ownership map of a persistent launch (persist.hip): (owner matrix nt x nt as described in
    include/mi355gp_debug.h, near owners, half owners, far workers, most tiles one worker holds, tiles claimed twice)."""
    owner = (ctypes.c_int * (nt * nt))()
    out4 = (ctypes.c_int * 4)()
    dup = lib().mi355gp_dbg_persist_owners(nt, nw, tune, owner, out4)
    return np.frombuffer(owner, dtype=np.int32, count=nt * nt).reshape(nt, nt).copy(), out4[0], out4[1], out4[2], out4[3], dup


def lauum_plan(nt):
    """Host only: the X^T X work list for nt x nt tiles (gemm.hip): (items as an int array of rows (ti, tj, q, k0, klen, part),
    number of partial tiles, edge of an item's output tile, longest chunk in rows)."""
    out4 = (ctypes.c_int * 4)()
    lib().mi355gp_dbg_lauum_plan(nt, None, 0, out4)
    n = out4[0]
    buf = (ctypes.c_int * (6 * max(n, 1)))()
    check(lib().mi355gp_dbg_lauum_plan(nt, buf, n, out4), "mi355gp_dbg_lauum_plan")
    return np.frombuffer(buf, dtype=np.int32, count=6 * n).reshape(n, 6).copy(), out4[1], out4[2], out4[3]


def lauum_wide_map(nt):
    """Host only: the work list of X^T X on 128 x 256 tiles for nt x nt tiles (csrc/lauum_policy.h): (items as an int array of rows
    (ti, tj, column blocks, K), whether the policy gives this nt the wide tile, the policy's threshold in tiles)."""
    out4 = (ctypes.c_int * 4)()
    lib().mi355gp_dbg_lauum_wide_map(nt, None, 0, out4)
    n = out4[0]
    buf = (ctypes.c_int * (4 * max(n, 1)))()
    check(lib().mi355gp_dbg_lauum_wide_map(nt, buf, n, out4), "mi355gp_dbg_lauum_wide_map")
    return np.frombuffer(buf, dtype=np.int32, count=4 * n).reshape(n, 4).copy(), bool(out4[1]), out4[2]


def dbg_lauum(X, variant, reps=0, device=0, W0=None):
    """W = X^T X of a lower-triangular X (n x n, n % 128 == 0) as one whole-K launch on the 128 x 128 tile (variant 0) or the
    128 x 256 tile (variant 1), or as `lauum_device` launches it with a default workspace (variant 2; W then starts as W0):
    (W, ms per launch over `reps` further launches).  X an int n: a synthetic matrix made on the device, W is None."""
    require_device(device)
    ms = ctypes.c_double(0.0)
    if isinstance(X, (int, np.integer)):
        check(lib().mi355gp_dbg_lauum(device, int(X), None, None, int(variant), int(reps), ctypes.byref(ms)), "mi355gp_dbg_lauum")
        return None, ms.value
    X = f64(X)
    W = np.zeros_like(X) if W0 is None else f64(W0).copy()
    assert W.shape == X.shape and (W0 is None or variant == 2)
    check(lib().mi355gp_dbg_lauum(device, X.shape[0], X.ctypes.data_as(_c_dp), W.ctypes.data_as(_c_dp), int(variant), int(reps),
                                  ctypes.byref(ms)), "mi355gp_dbg_lauum")
    return W, ms.value


def dbg_tileop(op, dims, X, B, Out, alpha=1.0, device=0):
    """One launcher of the tile-GEMM family alone (include/mi355gp_debug_tileops.h): op a key of TILEOPS, dims its integers, X / B
    the operands (None where the op has none), Out what the output buffer holds before the launch.  Returns the buffer after it
    (same shape as Out); the shapes are checked here against what the entry point will read and write."""
    require_device(device)
    d = [int(v) for v in dims]
    if op in ("trmm_lower", "trmm_lower_T", "trmm64"):
        n, m = 128 * d[0], 128 * d[1]
        shapes = ((n, n), (m, n) if op == "trmm64" and d[2] >= 2 else (n, m))
        shapes += (shapes[1],)
    elif op == "gram_splitk":
        shapes = ((d[0], d[1]), None, (d[2], d[1], d[1]))
    else:
        n = d[0] + 128 * max(d[3] + d[1], d[4] + d[2])
        shapes = (None, None, (n, n))
    arrs = []
    for a, shp in zip((X, B, Out), shapes):
        assert (a is None) == (shp is None) and (a is None or np.shape(a) == shp), (op, d, shp)
        arrs.append(None if a is None else f64(a))
    out = arrs[2].copy()
    da = (ctypes.c_int64 * len(d))(*d)
    check(lib().mi355gp_dbg_tileop(device, TILEOPS[op], da, _opt(arrs[0]), _opt(arrs[1]), out.ctypes.data_as(_c_dp), float(alpha)),
          "mi355gp_dbg_tileop")
    return out


class KronContext(_Handle):
    """One device context of the Kronecker grid path (include/mi355gp_kron.h) = one uploaded y on a grid G_1 x ... x G_D: y, alpha
    and two work vectors of N = prod G_d doubles, nothing larger.  The flat index has the last dimension fastest."""
    _create, _destroy = "mi355gp_kron_create", "mi355gp_kron_destroy"
    FETCH_ALPHA = 0

    def __init__(self, device=0):
        super(KronContext, self).__init__(device)
        self.G, self.N = (), 0

    def set_data(self, G, y):
        G = np.ascontiguousarray(G, dtype=np.int64).ravel()
        y = f64(np.ravel(y))
        assert G.size >= 1 and y.size == int(np.prod(G)), "y must have prod(G) entries"
        check(lib().mi355gp_kron_set_data(self._h, G.size, G, y), "mi355gp_kron_set_data")
        self.G, self.N = tuple(int(g) for g in G), y.size

    def _mats(self, mats, what):
        assert len(mats) == len(self.G) and all(np.shape(m) == (g, g) for m, g in zip(mats, self.G)), what + " must be D matrices G_d x G_d"
        return f64(np.concatenate([np.ravel(f64(m)) for m in mats]))

    def _vecs(self, vecs, what):
        assert len(vecs) == len(self.G) and all(np.size(v) == g for v, g in zip(vecs, self.G)), what + " must be D vectors of G_d entries"
        return f64(np.concatenate([np.ravel(f64(v)) for v in vecs]))

    def solve(self, Qs, lams, noise):
        """alpha stays resident: (y^T alpha, sum log(V + noise)); `noise` is the whole term on the diagonal"""
        sc = np.zeros(2)
        check(lib().mi355gp_kron_solve(self._h, self._mats(Qs, "Qs"), self._vecs(lams, "lams"), float(noise), sc), "mi355gp_kron_solve")
        return float(sc[0]), float(sc[1])

    def quadforms(self, factors, gammas):
        """factors, gammas: one list of D matrices, resp. D vectors, per parameter: (q (nmat), s (nmat)) with
        q_t = alpha^T ((x)A_d) alpha and s_t = sum_i ((x)gamma_d)_i / (V_i + noise)"""
        assert len(factors) == len(gammas)
        nmat = len(factors)
        out = np.zeros(2 * max(nmat, 1))
        F = f64(np.concatenate([self._mats(f, "factors") for f in factors])) if nmat else np.zeros(1)
        g = f64(np.concatenate([self._vecs(v, "gammas") for v in gammas])) if nmat else np.zeros(1)
        check(lib().mi355gp_kron_quadforms(self._h, nmat, F, g, out), "mi355gp_kron_quadforms")
        return out[0:2 * nmat:2].copy(), out[1:2 * nmat:2].copy()

    def predict(self, kx, bx, noise_pred, want_var=True):
        """kx, bx: D blocks M x G_d (bx[d] = kx[d] Q_d): (mu (M), variance reduction (M) or None)"""
        M = np.shape(kx[0])[0]
        assert len(kx) == len(self.G) and all(np.shape(k) == (M, g) for k, g in zip(kx, self.G)), "kx must be D blocks M x G_d"
        K = f64(np.concatenate([np.ravel(f64(k)) for k in kx]))
        mu = np.empty(M)
        B = var = None
        if want_var:
            assert len(bx) == len(self.G) and all(np.shape(b) == (M, g) for b, g in zip(bx, self.G)), "bx must be D blocks M x G_d"
            B = f64(np.concatenate([np.ravel(f64(b)) for b in bx]))
            var = np.empty(M)
        check(lib().mi355gp_kron_predict(self._h, M, K, _opt(B), float(noise_pred), mu, _opt(var)), "mi355gp_kron_predict")
        return mu, var

    def fetch_alpha(self):
        out = np.empty(self.N)
        check(lib().mi355gp_kron_fetch(self._h, self.FETCH_ALPHA, out), "mi355gp_kron_fetch")
        return out

    def mode_probe(self, A, x, transA=False, reps=1):
        """One mode product alone: x (P x G), A (R x G, or G x R with transA) -> (out (R x P), ms per launch)"""
        A, x = f64(A), f64(x)
        P, G = x.shape
        R = A.shape[1] if transA else A.shape[0]
        assert A.shape == ((G, R) if transA else (R, G))
        out = np.empty((R, P))
        ms = ctypes.c_double(0.0)
        check(lib().mi355gp_kron_mode_probe(self._h, P, G, R, int(bool(transA)), A, x, out, int(reps), ctypes.byref(ms)),
              "mi355gp_kron_mode_probe")
        return out, ms.value

    def last_ms(self):
        """HIP-event time (ms) of the mode products and the scaling of the last solve + quadforms pair"""
        ms = ctypes.c_double(0.0)
        check(lib().mi355gp_kron_get_ms(self._h, ctypes.byref(ms)), "mi355gp_kron_get_ms")
        return ms.value


def psi_lin_rows_probe(W, X, Z, variances, c0=0.0, Y=None, V=None, rowscale=None, beta=0.0, gscale=1.0, fused=True, device=0,
                       time_reps=0):
    """The row-side kernel of a Linear part on its own (`mi355gp_dbg_psi_lin_rows`, include/mi355gp_debug_psi_lin.h):
    out[i][q] = variances_q (sum_j g[i][j] Z[j][q] + c0 X[i][q]), g = W, or rowscale_i (gscale W + beta Y V^T) formed on the fly.
    `fused`: the MFMA kernel (D <= 16); otherwise the weights in memory and the plain kernel.  time_reps > 0: returns
    (out, the milliseconds of each of that many further launches, by HIP events)."""
    W, X, Z = f64(W), f64(X), f64(Z)
    rows, M = W.shape
    D = X.shape[1]
    assert X.shape == (rows, D) and Z.shape == (M, D), "W is rows x M, X rows x D, Z M x D"
    var = f64(np.broadcast_to(np.asarray(variances, dtype=np.float64).ravel(), (D,)))
    Dy = 0
    if Y is not None:
        Y, V = f64(Y), f64(V)
        Dy = Y.shape[1]
        assert Y.shape == (rows, Dy) and V.shape == (M, Dy), "Y is rows x Dy, V M x Dy"
        rowscale = None if rowscale is None else f64(np.asarray(rowscale)).ravel()
        assert rowscale is None or rowscale.size == rows
    out, ms = np.empty((rows, D)), np.zeros(max(1, int(time_reps)))
    check(lib().mi355gp_dbg_psi_lin_rows(int(device), int(bool(fused)), W, _opt(Y), _opt(V if Y is not None else None),
                                           _opt(rowscale if Y is not None else None), float(beta), float(gscale), X, Z, var,
                                           float(c0), rows, M, D, Dy, out, int(time_reps), _opt(ms)), "mi355gp_dbg_psi_lin_rows")
    return (out, ms) if time_reps > 0 else out
