"""ctypes binding of the C-ABI in include/gpemu.h (lib/libgpemu_hip.so).

This is the same binding a reference maintainer would write for any FFI
(INTEGRATION.md); the tests and bench.py drive the device library through
it.  There is no CPU fallback: if the library is missing it is an error.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

POWEREXP, MATERN32, MATERN52 = 1, 2, 3

OK, ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_PD, ERR_REGRESSION, ERR_STATE = range(7)
PROF_NONE, PROF_GEMM, PROF_FILL, PROF_LEAF, PROF_POTRF, PROF_GEMM_BIG, PROF_GEMM_K512 = range(7)
PROF_LOO = 7
PROF_MEAN = 8
PROF_MEAN_GRAD = 9
PROF_VAR_GRAD = 10
PROF_COV = 11
PROF_JOINT = 12
PROF_LGO = 13
PROF_SENS = 14
PROF_SENS_POST = 15
PROF_CALIB = 16
PROF_DESIGN = 17
PROF_DESIGN_TARGET = 18
CALIB_MAX_R, CALIB_MAX_NT = 16, 1024
MODE_EXACT_GRAD, MODE_MATERN_LOG = 1, 2
MEASURE_UNIFORM, MEASURE_GAUSS = 0, 1
RESULT_RING = 4

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class GemmLaunchArgs(C.Structure):
    """gpemu_gemm_launch_args of include/gpemu.h (every field defaults to 0)"""
    _fields_ = ([(f, C.c_long) for f in ("offC", "offA", "offB", "ldc", "lda", "ldb", "bsC", "bsA", "bsB")] +
                [("alpha", C.c_double)] +
                [(f, C.c_int) for f in ("m", "n", "k0", "k1", "beta", "tri", "kstart_mode", "kstart_off", "kend_mode",
                                        "kend_off", "nbatch", "ksplit", "force_cfg", "fa", "fa_c0")])


class UpdateLaunchArgs(C.Structure):
    """gpemu_update_launch_args of include/gpemu.h"""
    _fields_ = ([(f, C.c_long) for f in ("off", "ld", "stride")] +
                [(f, C.c_int) for f in ("c0", "k", "ncols", "rp", "inv", "rhs_live", "nbatch", "ride")])


class LeafLaunchArgs(C.Structure):
    """gpemu_leaf_launch_args of include/gpemu.h"""
    _fields_ = ([(f, C.c_long) for f in ("off", "ld", "bstride")] +
                [(f, C.c_int) for f in ("nbatch", "c0", "m_below", "op", "staged", "pre", "c0b", "fa", "r_far", "m_far")])


LEAF_FACTOR, LEAF_SOLVE, LEAF_FACTOR_SOLVE, LEAF_PAIR, LEAF_PANEL_ROWS = 0, 1, 2, 3, 4


class GradSumsArgs(C.Structure):
    """gpemu_grad_sums_args of include/gpemu.h"""
    _fields_ = ([(f, _dp) for f in ("thetas", "a", "z", "gram", "alpha_out", "beta_out", "part_out", "sums_out")] +
                [(f, C.c_int) for f in ("nb", "nthetas", "form", "gram_dist", "clamp")])


class FillLaunchArgs(C.Structure):
    """gpemu_fill_launch_args of include/gpemu.h"""
    _fields_ = ([(f, _dp) for f in ("thetas", "rrows", "xq", "out", "norm2_out")] + [("form_out", _ip)] +
                [(f, C.c_long) for f in ("out_len", "rstride")] +
                [(f, C.c_int) for f in ("op", "form", "nb", "nthetas", "M", "Rp", "guard")])


FILL_STAGE, FILL_KVEC, FILL_FULL = 0, 1, 2


class ResidentLaunchArgs(C.Structure):
    """gpemu_resident_launch_args of include/gpemu.h"""
    _fields_ = ([(f, _dp) for f in ("lin", "kq", "vp", "part", "betaq", "y", "z", "t", "res", "mean", "var", "werr", "stat")] +
                [(f, _ip) for f in ("colrow", "members", "moff", "bsize", "info", "info_out")] +
                [(f, C.c_long) for f in ("lin_len", "ld", "kq_len", "ldk", "vp_len", "ldv", "part_len", "z_len", "t_len", "tstride", "out_len")] +
                [(f, C.c_int) for f in ("op", "K", "ntri", "ntot", "nslice", "klen", "vrows",
                                        "N", "Np", "nreg", "g0", "nbc", "bp", "ngroups", "nmembers")])


RES_SKINNY, RES_GEMV, RES_LOO_COLSQ, RES_LOO_FINISH, RES_LGO_GATHER, RES_LGO_STAGE, RES_LGO_FINISH, RES_LGO_TAIL = range(8)
_RES_LEN = dict(lin="lin_len", kq="kq_len", vp="vp_len", part="part_len", z="z_len", t="t_len", mean="out_len")


class SampleArgs(C.Structure):
    """gpemu_sample_args of include/gpemu.h"""
    _fields_ = ([(f, C.c_int) for f in ("nwalkers", "nsteps", "burn", "thin")] +
                [(f, C.c_ulonglong) for f in ("seed", "first_step")] + [("a", C.c_double)])


_up = C.POINTER(C.c_uint)

# every symbol include/gpemu.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gpemu_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "gpemu_ctx_destroy": (None, [C.c_void_p]),
    "gpemu_last_error": (C.c_char_p, [C.c_void_p]),
    "gpemu_version": (C.c_char_p, []),
    "gpemu_device_count": (C.c_int, []),
    "gpemu_device_memory": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "gpemu_rccl_allgather": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, _dp, C.c_int, _dp, C.c_char_p, C.c_size_t]),
    "gpemu_rccl_unique_id": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "gpemu_rccl_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "gpemu_rccl_comm_allgather": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, C.c_char_p, C.c_size_t]),
    "gpemu_rccl_comm_destroy": (None, [C.c_void_p]),
    "gpemu_set_model": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp]),
    "gpemu_set_training": (C.c_int, [C.c_void_p, _dp]),
    "gpemu_cov_matrix": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp]),
    "gpemu_kvectors": (C.c_int, [C.c_void_p, _dp, C.c_int, C.c_int, _dp, _dp]),
    "gpemu_loglik": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_loglik_enqueue": (C.c_int, [C.c_void_p, _dp, C.c_int]),
    "gpemu_loglik_collect": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_loglik_batch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_loglik_batch_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    "gpemu_loglik_batch_collect": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_loglik_batch_collect_back": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_grad": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _ip]),
    "gpemu_loglik_grad": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_loglik_grad_batch": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_loglik_grad_batch_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int]),
    "gpemu_loglik_grad_batch_collect": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_loglik_grad_batch_collect_back": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpemu_predict_setup": (C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _ip]),
    "gpemu_predict_setup_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, _dp, C.c_int, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gpemu_warm_start": (C.c_int, [C.c_int]),
    "gpemu_get_cinverse": (C.c_int, [C.c_void_p, _dp]),
    "gpemu_predict_batch": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "gpemu_predict_batch_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "gpemu_predict_batch_collect": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "gpemu_predict_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_predict_mean": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "gpemu_predict_mean_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "gpemu_predict_mean_collect": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "gpemu_predict_mean_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gpemu_predict_mean_grad": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "gpemu_predict_mean_grad_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "gpemu_predict_mean_grad_collect": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "gpemu_predict_mean_grad_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_predict_var_grad": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "gpemu_predict_var_grad_enqueue": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "gpemu_predict_var_grad_collect": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "gpemu_predict_var_grad_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_predict_cov": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp]),
    "gpemu_predict_cov_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_predict_joint_factor": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_predict_joint_factor_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_predict_joint_draw": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "gpemu_predict_joint_draw_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gpemu_predict_joint_release": (C.c_int, [C.c_void_p]),
    "gpemu_loo": (C.c_int, [C.c_void_p, _dp, _dp]),
    "gpemu_loo_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_lgo": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_lgo_dev": (C.c_int, [C.c_void_p, C.c_int, _ip, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_lgo_release": (C.c_int, [C.c_void_p]),
    "gpemu_sens_cov": (C.c_int, [C.c_void_p, C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpemu_sens_cov_dev": (C.c_int, [C.c_void_p, C.c_void_p, _dp, _dp, C.c_void_p]),
    "gpemu_sens_main": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp]),
    "gpemu_sens_release": (C.c_int, [C.c_void_p]),
    "gpemu_sens_post": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpemu_sens_post_dev": (C.c_int, [C.c_void_p, _dp, _dp, C.c_void_p]),
    "gpemu_sens_main_var": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpemu_test_sens_post_state": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "gpemu_design_gain": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpemu_design_gain_dev": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_test_design_state": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "gpemu_design_batch": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, _dp, C.c_int, C.c_void_p, _dp, _dp, _dp, _dp]),
    "gpemu_design_batch_dev": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_test_design_batch_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpemu_design_target_set": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "gpemu_design_target_set_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, _dp, C.c_void_p, C.c_void_p]),
    "gpemu_design_target_gain": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "gpemu_design_target_gain_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_design_target_release": (C.c_int, [C.c_void_p]),
    "gpemu_test_design_target_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpemu_sens_pairs": (C.c_int, [C.c_void_p, C.c_void_p, _dp, _dp, _dp]),
    "gpemu_sens_pairs_dev": (C.c_int, [C.c_void_p, C.c_void_p, _dp, _dp, C.c_void_p]),
    "gpemu_sens_pairs_post": (C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    "gpemu_sens_pairs_post_dev": (C.c_int, [C.c_void_p, _dp, _dp, C.c_void_p]),
    "gpemu_sens_joint": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "gpemu_sens_set_measure": (C.c_int, [C.c_void_p, _ip]),
    "gpemu_sens_get_measure": (C.c_int, [C.c_void_p, _ip]),
    "gpemu_calib_project": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_calib_setup": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpemu_calib_release": (C.c_int, [C.c_void_p]),
    "gpemu_calib_eval": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, _ip]),
    "gpemu_calib_eval_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gpemu_calib_grad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_long, _dp, _dp]),
    "gpemu_calib_grad_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long,
                                       C.c_void_p, C.c_void_p]),
    "gpemu_calib_select": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_double, C.c_int, C.c_double, _ip, _ip]),
    "gpemu_calib_select_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_void_p, _ip]),
    "gpemu_calib_gather_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_philox4x32": (C.c_int, [_up, _up, _up]),
    "gpemu_sample_uniforms": (C.c_int, [C.c_ulonglong, C.c_uint, C.c_ulonglong, _dp]),
    "gpemu_sample_set_prior": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _dp]),
    "gpemu_sample_release": (C.c_int, [C.c_void_p]),
    "gpemu_sample_propose_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_double,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_sample_accept_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_sample_logpost_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpemu_calib_sample": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(SampleArgs), _dp, _dp, _dp, _dp, _dp,
                                     _ip, _ip]),
    "gpemu_test_sample_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "gpemu_ctx_device": (C.c_int, [C.c_void_p]),
    "gpemu_chol_inverse": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, _dp, _ip]),
    "gpemu_symm_apply": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "gpemu_symm_invalidate": (C.c_int, [C.c_void_p]),
    "gpemu_symm_pin": (C.c_int, [C.c_void_p, C.c_int]),
    "gpemu_set_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "gpemu_get_mode": (C.c_int, [C.c_void_p]),
    "gpemu_derivative_gauss": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_double, _dp, C.c_int]),
    "gpemu_trace_product": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp]),
    "gpemu_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "gpemu_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gpemu_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gpemu_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gpemu_sync": (C.c_int, [C.c_void_p]),
    "gpemu_prof_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "gpemu_prof_end": (C.c_int, [C.c_void_p, _ip, _dp, _dp, _dp]),
    "gpemu_trace_dump": (C.c_int, [C.c_void_p, C.c_char_p]),
    "gpemu_test_gemm_nt": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp]),
    "gpemu_test_gemm_launch": (C.c_int, [C.c_void_p, _dp, C.c_long, C.POINTER(GemmLaunchArgs), _ip]),
    "gpemu_test_update_launch": (C.c_int, [C.c_void_p, _dp, C.c_long, C.POINTER(UpdateLaunchArgs), _ip]),
    "gpemu_test_leaf_launch": (C.c_int, [C.c_void_p, _dp, C.c_long, C.POINTER(LeafLaunchArgs), _ip]),
    "gpemu_test_grad_sums": (C.c_int, [C.c_void_p, C.POINTER(GradSumsArgs)]),
    "gpemu_test_fill_launch": (C.c_int, [C.c_void_p, C.POINTER(FillLaunchArgs)]),
    "gpemu_test_resident_launch": (C.c_int, [C.c_void_p, C.POINTER(ResidentLaunchArgs)]),
    "gpemu_test_pred_state": (C.c_int, [C.c_void_p, _dp, _dp]),
    "gpemu_test_gemm_bench": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, _dp, _dp]),
    "gpemu_test_potrf": (C.c_int, [C.c_void_p, C.c_int, _dp, _ip]),
    "gpemu_test_staged_matrix": (C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, C.c_int, _dp]),
    "gpemu_test_tile_table": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int]),
    "gpemu_test_row_table": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int]),
}

_lib = None


def lib_path():
    return _build.HIP_LIB


def load():
    """dlopen the device library and bind every declared symbol (fails loudly if absent)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -m madaiemulator_amd.build` (no CPU fallback exists)")
        L = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class GpemuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gpemu error {code}: {msg}")
        self.code = code


def _a(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


def nthetas_for(kind, d):
    return d + 2 if kind == POWEREXP else 3


def predict_setup_batch(ctxs, thetas):
    """gpemu_predict_setup_batch: the contexts of the components of a multi-output model (same design, own training vector)
    set up as ONE lock-step batch.  Returns (beta [n x nreg], info [n], status [n], rc)."""
    th = _a(thetas).reshape(len(ctxs), -1)
    n = len(ctxs)
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    beta = np.full((n, ctxs[0].nreg), np.nan)
    info = np.zeros(n, dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    rc = ctxs[0].L.gpemu_predict_setup_batch(hs, n, _p(th), th.shape[1], _p(beta), info.ctypes.data_as(C.POINTER(C.c_int)),
                                            status.ctypes.data_as(C.POINTER(C.c_int)))
    if rc not in (OK, ERR_NOT_PD, ERR_REGRESSION):
        raise GpemuError(rc, ctxs[0].L.gpemu_last_error(ctxs[0].h).decode())
    return beta, info, status, rc


def design_batch(ctxs, lo, hi, Xq, nbatch, weight=None):
    """gpemu_design_batch: nbatch greedy picks among the candidates Xq[M, d] for the contexts of one design (weight: one per context,
    None: all 1) -> dict(pick[nbatch], pick_gain[nbatch], pick_gain_ctx[nbatch, nctx], gain_first[M], gain_last[M])"""
    n, lead = len(ctxs), ctxs[0]
    lo, hi = lead._box("design_batch", lo, hi)
    Xq = _a(Xq).reshape(-1, lead.d)
    M = Xq.shape[0]
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    w = None if weight is None else _a(weight).ravel()
    if w is not None and w.size != n:
        raise ValueError("design_batch: one weight per context")
    pick = np.full(nbatch, -1, dtype=np.int32)
    out = dict(pick=pick, pick_gain=np.empty(nbatch), pick_gain_ctx=np.empty((nbatch, n)), gain_first=np.empty(M), gain_last=np.empty(M))
    rc = lead.L.gpemu_design_batch(hs, n, _po(w), _p(lo), _p(hi), M, _p(Xq), nbatch, pick.ctypes.data_as(C.c_void_p), _p(out["pick_gain"]),
                                   _p(out["pick_gain_ctx"]), _p(out["gain_first"]), _p(out["gain_last"]))
    if rc != OK:
        raise GpemuError(rc, lead.L.gpemu_last_error(lead.h).decode())
    return out


def design_batch_dev(ctxs, lo, hi, M, xq_dev, nbatch, pick_dev, pick_gain_dev, pick_gain_ctx_dev=None, gain_first_dev=None,
                     gain_last_dev=None, weight=None):
    """lo, hi, weight: HOST; everything else device memory (results complete behind ctxs[0]'s stream)"""
    n, lead = len(ctxs), ctxs[0]
    lo, hi = lead._box("design_batch_dev", lo, hi)
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    w = None if weight is None else _a(weight).ravel()
    rc = lead.L.gpemu_design_batch_dev(hs, n, _po(w), _p(lo), _p(hi), M, xq_dev, nbatch, pick_dev, pick_gain_dev, pick_gain_ctx_dev,
                                       gain_first_dev, gain_last_dev)
    if rc != OK:
        raise GpemuError(rc, lead.L.gpemu_last_error(lead.h).decode())


def _opt(x):
    return None if x is None else _a(x)


def _po(a):
    return None if a is None else _p(a)


def calib_project(ybar, A, z, S=None, sd=None, nt=None, nr=None):
    """gpemu_calib_project (host arithmetic, no device): the once-per-observation-set tables of the calibration entries
    -> dict(mhat[nr], sigz[nr, nr], c_perp, logdet_S, logdet_G, info, status); status is OK, ERR_NOT_PD (info = the 1-based
    pivot) or ERR_ARG.  nt, nr default to A's shape."""
    A = _a(A)
    nt = A.shape[0] if nt is None else nt
    nr = A.shape[1] if nr is None else nr
    ybar, z, S, sd = _opt(ybar), _opt(z), _opt(S), _opt(sd)
    mhat, sigz, consts = np.full(max(nr, 1), np.nan), np.full((max(nr, 1), max(nr, 1)), np.nan), np.full(3, np.nan)
    info = C.c_int(0)
    rc = load().gpemu_calib_project(nt, nr, _po(ybar), _p(A), _po(z), _po(S), _po(sd), _p(mhat), _p(sigz), _p(consts), C.byref(info))
    return dict(mhat=mhat, sigz=sigz, c_perp=consts[0], logdet_S=consts[1], logdet_G=consts[2], info=info.value, status=rc)


def philox4x32(ctr, key):
    """gpemu_philox4x32 (host, no device): the four output words of Philox4x32-10 for a counter of 4 and a key of 2 words"""
    c, k, o = (np.ascontiguousarray(ctr, dtype=np.uint32), np.ascontiguousarray(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32))
    if c.size != 4 or k.size != 2:
        raise GpemuError(ERR_ARG, "philox4x32: a counter of 4 words and a key of 2")
    rc = load().gpemu_philox4x32(c.ctypes.data_as(_up), k.ctypes.data_as(_up), o.ctypes.data_as(_up))
    if rc != OK:
        raise GpemuError(rc, "gpemu_philox4x32")
    return o


def sample_uniforms(seed, walker, step):
    """gpemu_sample_uniforms (host, no device): (u1, u2, u3) of a walker at a global step of the ensemble sampler"""
    u = np.zeros(3)
    rc = load().gpemu_sample_uniforms(seed, walker, step, _p(u))
    if rc != OK:
        raise GpemuError(rc, "gpemu_sample_uniforms")
    return u


def calib_sample(comps, obs, x0, nsteps, burn=0, thin=1, seed=0, first_step=0, a=2.0, trace=True):
    """gpemu_calib_sample: comps the component contexts (prediction set up), obs the context with the calibration set-up and
    the prior; x0[W, d].  -> dict(trace_x[nrec, W, d], trace_lp[nrec, W] (None without trace), x_end, lp_end, naccept, nrec)"""
    x0 = _a(x0)
    W, d = x0.shape
    args = SampleArgs(nwalkers=W, nsteps=nsteps, burn=burn, thin=thin, seed=seed, first_step=first_step, a=a)
    cap = sum(1 for g in range(first_step, first_step + max(nsteps, 0)) if g >= burn and (g + 1) % max(thin, 1) == 0)
    tx, tl = (np.full((cap, W, d), np.nan), np.full((cap, W), np.nan)) if trace else (None, None)
    x_end, lp_end, nacc, nrec = np.full((W, d), np.nan), np.full(W, np.nan), np.zeros(W, dtype=np.int32), C.c_int(-1)
    hs = (C.c_void_p * len(comps))(*[c.h for c in comps])
    obs._chk(obs.L.gpemu_calib_sample(hs, len(comps), obs.h, C.byref(args), _p(x0), _po(tx), _po(tl), _p(x_end), _p(lp_end),
                                      nacc.ctypes.data_as(_ip), C.byref(nrec)))
    assert nrec.value == cap
    return dict(trace_x=tx, trace_lp=tl, x_end=x_end, lp_end=lp_end, naccept=nacc, nrec=nrec.value)


class Context:
    """One gpemu_ctx: one HIP stream + its HBM workspace.  One per host thread."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.gpemu_ctx_create(C.byref(h), device)
        if rc != OK:
            raise GpemuError(rc, "gpemu_ctx_create failed (no usable HIP device?)")
        self.h = h
        self.N = self.d = self.nreg = 0
        self.kind = self.order = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.gpemu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != OK and rc not in allow:
            raise GpemuError(rc, self.L.gpemu_last_error(self.h).decode())
        return rc

    # -- model ---------------------------------------------------------
    def set_model(self, kind, order, X, y):
        X, y = _a(X), _a(y)
        N, d = X.shape
        self._chk(self.L.gpemu_set_model(self.h, kind, order, N, d, _p(X), _p(y)))
        self.kind, self.order, self.N, self.d, self.nreg = kind, order, N, d, 1 + order * d

    def set_training(self, y):
        y = _a(y)
        self._chk(self.L.gpemu_set_training(self.h, _p(y)))

    # -- a4 / a16 --------------------------------------------------------
    def cov_matrix(self, thetas):
        th = _a(thetas)
        out = np.empty((self.N, self.N))
        self._chk(self.L.gpemu_cov_matrix(self.h, _p(th), th.size, _p(out)))
        return out

    def kvectors(self, thetas, Xq):
        th, Xq = _a(thetas), _a(Xq).reshape(-1, self.d)
        out = np.empty((Xq.shape[0], self.N))
        self._chk(self.L.gpemu_kvectors(self.h, _p(th), th.size, Xq.shape[0], _p(Xq), _p(out)))
        return out

    # -- a11 ---------------------------------------------------------------
    def loglik(self, thetas):
        """-> dict(value=-logL, sigma2, beta, logdet, quad, info, status)"""
        th = _a(thetas)
        v, s2, ld, qd = (C.c_double(np.nan) for _ in range(4))
        info = C.c_int(0)
        beta = np.full(self.nreg, np.nan)
        rc = self.L.gpemu_loglik(self.h, _p(th), th.size, C.byref(v), C.byref(s2), _p(beta), C.byref(ld), C.byref(qd),
                                 C.byref(info))
        self._chk(rc, allow=(ERR_NOT_PD, ERR_REGRESSION))
        return dict(value=v.value, sigma2=s2.value, beta=beta, logdet=ld.value, quad=qd.value, info=info.value,
                    status=rc)

    def loglik_enqueue(self, thetas):
        th = _a(thetas)
        self._chk(self.L.gpemu_loglik_enqueue(self.h, _p(th), th.size))

    def loglik_collect(self):
        v, s2, ld, qd = (C.c_double(np.nan) for _ in range(4))
        info = C.c_int(0)
        beta = np.full(self.nreg, np.nan)
        rc = self.L.gpemu_loglik_collect(self.h, C.byref(v), C.byref(s2), _p(beta), C.byref(ld), C.byref(qd),
                                         C.byref(info))
        self._chk(rc, allow=(ERR_NOT_PD, ERR_REGRESSION))
        return dict(value=v.value, sigma2=s2.value, beta=beta, logdet=ld.value, quad=qd.value, info=info.value,
                    status=rc)

    def loglik_batch_enqueue(self, thetas):
        th = _a(thetas).reshape(-1, np.shape(thetas)[-1])
        self._nb = th.shape[0]
        self._chk(self.L.gpemu_loglik_batch_enqueue(self.h, th.shape[0], _p(th), th.shape[1]))

    def loglik_batch_collect(self):
        nb = self._nb
        v, s2, ld, qd = (np.full(nb, np.nan) for _ in range(4))
        beta = np.full((nb, self.nreg), np.nan)
        info = np.zeros(nb, dtype=np.int32)
        status = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.gpemu_loglik_batch_collect(self.h, nb, _p(v), _p(s2), _p(beta), _p(ld), _p(qd),
                                                    info.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
        return dict(value=v, sigma2=s2, beta=beta, logdet=ld, quad=qd, info=info, status=status)

    def loglik_batch_collect_back(self, back, nb):
        """results of the batch enqueued `back` batches before the newest (ring of RESULT_RING); waits for it only"""
        v, s2, ld, qd = (np.full(nb, np.nan) for _ in range(4))
        beta = np.full((nb, self.nreg), np.nan)
        info = np.zeros(nb, dtype=np.int32)
        status = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.gpemu_loglik_batch_collect_back(self.h, back, nb, _p(v), _p(s2), _p(beta), _p(ld), _p(qd),
                                                         info.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
        return dict(value=v, sigma2=s2, beta=beta, logdet=ld, quad=qd, info=info, status=status)

    def loglik_batch(self, thetas):
        """nb evaluations in lock-step (thetas: nb x nthetas) -> dict of arrays, as loglik() per element"""
        self.loglik_batch_enqueue(thetas)
        return self.loglik_batch_collect()

    def loglik_grad_batch(self, thetas):
        """value + gradient at nb thetas in lock-step -> dict(value, sigma2, beta, grad (nb x nthetas-1), info, status)"""
        th = _a(thetas).reshape(-1, np.shape(thetas)[-1])
        nb, nt = th.shape
        v, s2 = np.full(nb, np.nan), np.full(nb, np.nan)
        beta = np.full((nb, self.nreg), np.nan)
        g = np.full((nb, nt - 1), np.nan)
        info = np.zeros(nb, dtype=np.int32)
        status = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.gpemu_loglik_grad_batch(self.h, nb, _p(th), nt, _p(v), _p(s2), _p(beta), _p(g),
                                                 info.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
        return dict(value=v, sigma2=s2, beta=beta, grad=g, info=info, status=status)

    def loglik_grad_batch_enqueue(self, thetas):
        """puts a value+gradient batch on the context's stream and returns at once"""
        th = _a(thetas).reshape(-1, np.shape(thetas)[-1])
        self._gnb, self._gnt = th.shape
        self._chk(self.L.gpemu_loglik_grad_batch_enqueue(self.h, th.shape[0], _p(th), th.shape[1]))

    def loglik_grad_batch_collect_back(self, back, nb=None, nthetas=None):
        """results of the value+gradient batch enqueued `back` batches before the newest; waits for it only"""
        nb = self._gnb if nb is None else nb
        nt = self._gnt if nthetas is None else nthetas
        v, s2 = np.full(nb, np.nan), np.full(nb, np.nan)
        beta = np.full((nb, self.nreg), np.nan)
        g = np.full((nb, nt - 1), np.nan)
        info = np.zeros(nb, dtype=np.int32)
        status = np.zeros(nb, dtype=np.int32)
        self._chk(self.L.gpemu_loglik_grad_batch_collect_back(self.h, back, nb, _p(v), _p(s2), _p(beta), _p(g),
                                                              info.ctypes.data_as(_ip), status.ctypes.data_as(_ip)))
        return dict(value=v, sigma2=s2, beta=beta, grad=g, info=info, status=status)

    def loglik_grad_batch_collect(self):
        return self.loglik_grad_batch_collect_back(0)

    # -- a12 ---------------------------------------------------------------
    def grad(self, thetas):
        th = _a(thetas)
        g = np.full(th.size - 1, np.nan)
        info = C.c_int(0)
        rc = self._chk(self.L.gpemu_grad(self.h, _p(th), th.size, _p(g), C.byref(info)), allow=(ERR_NOT_PD,))
        return g, rc

    def loglik_grad(self, thetas):
        th = _a(thetas)
        g = np.full(th.size - 1, np.nan)
        beta = np.full(self.nreg, np.nan)
        v, s2 = C.c_double(np.nan), C.c_double(np.nan)
        info = C.c_int(0)
        rc = self._chk(self.L.gpemu_loglik_grad(self.h, _p(th), th.size, C.byref(v), C.byref(s2), _p(beta), _p(g),
                                                C.byref(info)), allow=(ERR_NOT_PD,))
        return dict(value=v.value, sigma2=s2.value, beta=beta, grad=g, info=info.value, status=rc)

    # -- a15 / a19 ---------------------------------------------------------
    def predict_setup(self, thetas):
        th = _a(thetas)
        beta = np.full(self.nreg, np.nan)
        info = C.c_int(0)
        rc = self._chk(self.L.gpemu_predict_setup(self.h, _p(th), th.size, _p(beta), C.byref(info)),
                       allow=(ERR_NOT_PD, ERR_REGRESSION))
        return beta, rc

    # the two halves of the four host-buffer prediction entries (gpemu_predict_<kind>_enqueue / _collect): one batch of any
    # kind is pending per context; _npred is its size, the collect's outputs are allocated by kind
    def _pred_enqueue(self, kind, Xq):
        Xq = _a(Xq).reshape(-1, self.d)
        self._npred = Xq.shape[0]
        self._chk(getattr(self.L, f"gpemu_predict_{kind}_enqueue")(self.h, Xq.shape[0], _p(Xq)))

    def _pred_collect(self, kind, outputs):
        """outputs: the collect's arrays in argument order, "m" / "v" (M values) or "g" (M x d) -> a tuple of them"""
        out = tuple(np.empty((self._npred, self.d) if o == "g" else self._npred) for o in outputs)
        self._chk(getattr(self.L, f"gpemu_predict_{kind}_collect")(self.h, self._npred, *map(_p, out)))
        return out

    def predict_enqueue(self, Xq):
        self._pred_enqueue("batch", Xq)

    def predict_collect(self):
        return self._pred_collect("batch", "mv")

    def loo(self):
        """leave-one-out mean and variance at every training point, from the resident prediction state -> (mean, var)"""
        m, v = np.empty(self.N), np.empty(self.N)
        self._chk(self.L.gpemu_loo(self.h, _p(m), _p(v)))
        return m, v

    def loo_dev(self, mean_dev, var_dev):
        self._chk(self.L.gpemu_loo_dev(self.h, mean_dev, var_dev))

    # K-fold / leave-group-out validation from the resident prediction state: every group left out as a
    # whole, its joint prediction and predictive density in closed form, all groups of a call in lock-step batches
    @staticmethod
    def _lgo_labels(group, ngroups):
        group = np.ascontiguousarray(group, dtype=np.int32).ravel()
        if ngroups is None:
            ngroups = int(group.max()) + 1 if group.size else 0
        return group, int(ngroups)

    def lgo(self, group, ngroups=None):
        """group[i] in 0 .. ngroups-1 or -1 (never left out), N labels; ngroups defaults to the largest label + 1
        -> dict(mean[N], var[N], werr[N] (design order, NaN for label -1), maha[ngroups], logdet[ngroups], logpdf[ngroups],
        info[ngroups], status); status is OK or ERR_NOT_PD (then info[g] != 0 names the group and the pivot, and that group's
        outputs are NaN)"""
        group, ngroups = self._lgo_labels(group, ngroups)
        if group.size != self.N:
            raise GpemuError(ERR_ARG, "lgo: one label per training point")
        ng = max(ngroups, 1)
        mean, var, werr = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        maha, logdet, logpdf = np.empty(ng), np.empty(ng), np.empty(ng)
        info = np.zeros(ng, dtype=np.int32)
        rc = self.L.gpemu_lgo(self.h, ngroups, group.ctypes.data_as(_ip), _p(mean), _p(var), _p(werr), _p(maha), _p(logdet),
                              _p(logpdf), info.ctypes.data_as(_ip))
        self._chk(rc, allow=(ERR_NOT_PD,))
        return dict(mean=mean, var=var, werr=werr, maha=maha, logdet=logdet, logpdf=logpdf, info=info, status=rc)

    def lgo_dev(self, group, ngroups, mean_dev, var_dev, werr_dev, stat_dev, info_dev):
        """group: HOST labels; the rest device pointers (werr_dev, stat_dev may be None); stat_dev: maha, logdet, logpdf, ngroups each"""
        group, ngroups = self._lgo_labels(group, ngroups)
        if group.size != self.N:
            raise GpemuError(ERR_ARG, "lgo_dev: one label per training point")
        self._chk(self.L.gpemu_lgo_dev(self.h, ngroups, group.ctypes.data_as(_ip), mean_dev, var_dev, werr_dev, stat_dev, info_dev))

    def lgo_release(self):
        self._chk(self.L.gpemu_lgo_release(self.h))

    # main effects and Sobol indices of the posterior mean in closed form: uniform inputs on the box [lo, hi]
    def sens_cov(self, lo, hi, other=None):
        """-> dict(e0[2], cov_all, cov_first[d], cov_rest[d]) of this context and `other` (default: itself) on one design"""
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_cov: one bound pair per coordinate")
        b = self if other is None else other
        e0, ca, cf, cr = np.empty(2), np.empty(1), np.empty(self.d), np.empty(self.d)
        self._chk(self.L.gpemu_sens_cov(self.h, b.h, _p(lo), _p(hi), _p(e0), _p(ca), _p(cf), _p(cr)))
        return dict(e0=e0, cov_all=ca[0], cov_first=cf, cov_rest=cr)

    def sens_cov_dev(self, lo, hi, out_dev, other=None):
        """lo, hi: HOST bounds; out_dev: 3 + 2 d doubles on the device (e0a, e0b, cov_all, first[d], rest[d])"""
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_cov_dev: one bound pair per coordinate")
        self._chk(self.L.gpemu_sens_cov_dev(self.h, (self if other is None else other).h, _p(lo), _p(hi), out_dev))

    def sens_main(self, lo, hi, grid):
        """grid[j][g]: values of x_j (d rows) -> (e0, main[d, G]) with main[j][g] = E[m | x_j = grid[j][g]]"""
        lo, hi, grid = _a(lo).ravel(), _a(hi).ravel(), _a(grid).reshape(self.d, -1)
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_main: one bound pair per coordinate")
        e0, main = np.empty(1), np.empty(grid.shape)
        self._chk(self.L.gpemu_sens_main(self.h, _p(lo), _p(hi), grid.shape[1], _p(grid), _p(e0), _p(main)))
        return e0[0], main

    def sens_release(self):
        self._chk(self.L.gpemu_sens_release(self.h))

    # implausibility and calibration likelihood against observations; the tables are the context's, not the model's
    def calib_setup(self, ybar, A, z, S=None, sd=None, rel=None, nt=None, nr=None, allow=()):
        """observations z with covariance S (or standard deviations sd) for outputs ybar + A m; rel: relative model error per
        output -> (status, info)"""
        A = _a(A)
        nt = A.shape[0] if nt is None else nt
        nr = A.shape[1] if nr is None else nr
        ybar, z, S, sd, rel = _opt(ybar), _opt(z), _opt(S), _opt(sd), _opt(rel)
        info = C.c_int(0)
        rc = self.L.gpemu_calib_setup(self.h, nt, nr, _po(ybar), _p(A), _po(z), _po(S), _po(sd), _po(rel), C.byref(info))
        self._chk(rc, allow=allow)
        if rc == OK:
            self.calib_nr = nr
        return rc, info.value

    def calib_release(self):
        self._chk(self.L.gpemu_calib_release(self.h))

    def calib_eval(self, mean, var, M=None):
        """mean, var: nr rows (component-major) of ld >= M columns -> (stat[5, M]: chi2, logpdf, top three I_t; worst[M])"""
        mean, var = np.atleast_2d(_a(mean)), np.atleast_2d(_a(var))
        ld = mean.shape[1]
        M = ld if M is None else M
        stat, worst = np.full((5, max(M, 1)), np.nan), np.full(max(M, 1), -2, dtype=np.int32)
        self._chk(self.L.gpemu_calib_eval(self.h, M, _p(mean), _p(var), ld, _p(stat), worst.ctypes.data_as(_ip)))
        return stat, worst

    def calib_eval_dev(self, M, mean_dev, var_dev, ld, stat_dev, worst_dev):
        self._chk(self.L.gpemu_calib_eval_dev(self.h, M, mean_dev, var_dev, ld, stat_dev, worst_dev))

    def calib_grad(self, mean, var, gmean, gvar, M=None, d=None, want=(True, True)):
        """mean, var as calib_eval takes them; gmean, gvar: nr blocks (component-major) of ldg >= M * d values, component c's
        M x d row-major gradients (or nr x M x d arrays) -> (gchi2[M, d], glogpdf[M, d]); want: which of the two are asked
        for (the other is None)"""
        mean, var = np.atleast_2d(_a(mean)), np.atleast_2d(_a(var))
        gmean, gvar = _a(gmean), _a(gvar)
        ld = mean.shape[1]
        M = ld if M is None else M
        d = gmean.shape[2] if d is None else d
        gmean, gvar = gmean.reshape(mean.shape[0], -1), gvar.reshape(mean.shape[0], -1)
        ldg = gmean.shape[1]
        out = [np.full((max(M, 1), max(d, 1)), np.nan) if w else None for w in want]
        self._chk(self.L.gpemu_calib_grad(self.h, M, d, _p(mean), _p(var), ld, _p(gmean), _p(gvar), ldg, _po(out[0]), _po(out[1])))
        return out[0], out[1]

    def calib_grad_dev(self, M, d, mean_dev, var_dev, ld, gmean_dev, gvar_dev, ldg, gchi2_dev, glogpdf_dev):
        self._chk(self.L.gpemu_calib_grad_dev(self.h, M, d, mean_dev, var_dev, ld, gmean_dev, gvar_dev, ldg, gchi2_dev, glogpdf_dev))

    def calib_select(self, stat, cut_chi2=np.inf, level=1, cut_I=np.inf):
        """stat[5, M] as calib_eval returns it -> the kept point indices, ascending"""
        stat = _a(stat).reshape(5, -1)
        M = stat.shape[1]
        idx, n = np.full(max(M, 1), -1, dtype=np.int32), C.c_int(0)
        self._chk(self.L.gpemu_calib_select(self.h, M, _p(stat), cut_chi2, level, cut_I, idx.ctypes.data_as(_ip), C.byref(n)))
        return idx[:n.value].copy()

    def calib_gather_dev(self, M, stat_dev, worst_dev, count, idx_dev, out_dev, worst_out_dev):
        self._chk(self.L.gpemu_calib_gather_dev(self.h, M, stat_dev, worst_dev, count, idx_dev, out_dev, worst_out_dev))

    def calib_select_dev(self, M, stat_dev, cut_chi2, level, cut_I, idx_dev):
        n = C.c_int(0)
        self._chk(self.L.gpemu_calib_select_dev(self.h, M, stat_dev, cut_chi2, level, cut_I, idx_dev, C.byref(n)))
        return n.value

    # the input measure of every sens_* entry: one kind per coordinate, MEASURE_UNIFORM (lo, hi: the bounds)
    # or MEASURE_GAUSS (lo: the mean, hi: the standard deviation)
    # the ensemble sampler's prior and primitives; the run itself is abi.calib_sample
    def sample_set_prior(self, lo, hi, kind=None, allow=()):
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        kp = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32).ravel()
        return self._chk(self.L.gpemu_sample_set_prior(self.h, lo.size, None if kp is None else kp.ctypes.data_as(_ip), _p(lo), _p(hi)),
                         allow=allow)

    def sample_release(self):
        self._chk(self.L.gpemu_sample_release(self.h))

    def sample_propose_dev(self, W, d, half, step, seed, a, x_dev, y_dev, aux_dev):
        self._chk(self.L.gpemu_sample_propose_dev(self.h, W, d, half, step, seed, a, x_dev, y_dev, aux_dev))

    def sample_accept_dev(self, W, d, half, step, seed, y_dev, aux_dev, loglik_dev, x_dev, lp_dev, naccept_dev):
        self._chk(self.L.gpemu_sample_accept_dev(self.h, W, d, half, step, seed, y_dev, aux_dev, loglik_dev, x_dev, lp_dev, naccept_dev))

    def sample_logpost_dev(self, M, d, x_dev, loglik_dev, lp_dev):
        self._chk(self.L.gpemu_sample_logpost_dev(self.h, M, d, x_dev, loglik_dev, lp_dev))

    def test_sample_chunk(self, records):
        self._chk(self.L.gpemu_test_sample_chunk(self.h, records))

    def sens_set_measure(self, kind=None):
        """kind: d values of MEASURE_UNIFORM / MEASURE_GAUSS, or None for all uniform; set_model resets it"""
        if kind is None:
            self._chk(self.L.gpemu_sens_set_measure(self.h, None))
            return
        kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
        if kind.size != self.d:
            raise GpemuError(ERR_ARG, "sens_set_measure: one kind per coordinate")
        self._chk(self.L.gpemu_sens_set_measure(self.h, kind.ctypes.data_as(_ip)))

    def sens_get_measure(self):
        kind = np.zeros(max(self.d, 1), dtype=np.int32)
        self._chk(self.L.gpemu_sens_get_measure(self.h, kind.ctypes.data_as(_ip)))
        return kind[:self.d].copy()

    # emulator uncertainty of the same quantities: S_u = E Var*[E[f | x_u]] of the posterior process f
    def sens_post(self, lo, hi):
        """-> dict(s_none, s_all, s_first[d], s_rest[d])"""
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_post: one bound pair per coordinate")
        sn, sa, sf, sr = np.empty(1), np.empty(1), np.empty(self.d), np.empty(self.d)
        self._chk(self.L.gpemu_sens_post(self.h, _p(lo), _p(hi), _p(sn), _p(sa), _p(sf), _p(sr)))
        return dict(s_none=sn[0], s_all=sa[0], s_first=sf, s_rest=sr)

    def sens_post_dev(self, lo, hi, out_dev):
        """lo, hi: HOST bounds; out_dev: 2 + 2 d doubles on the device (s_none, s_all, first[d], rest[d])"""
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_post_dev: one bound pair per coordinate")
        self._chk(self.L.gpemu_sens_post_dev(self.h, _p(lo), _p(hi), out_dev))

    def sens_main_var(self, lo, hi, grid):
        """grid[j][g]: values of x_j (d rows) -> (main[d, G], var[d, G], var_e0): the curves, Var*[E[f | x_j = grid[j][g]]], Var*[E0]"""
        lo, hi, grid = _a(lo).ravel(), _a(hi).ravel(), _a(grid).reshape(self.d, -1)
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, "sens_main_var: one bound pair per coordinate")
        main, var, ve0 = np.empty(grid.shape), np.empty(grid.shape), np.empty(1)
        self._chk(self.L.gpemu_sens_main_var(self.h, _p(lo), _p(hi), grid.shape[1], _p(grid), _p(main), _p(var), _p(ve0)))
        return main, var, ve0[0]

    def sens_post_state(self):
        """-> (P[N, N], G[N, nreg], Q[nreg, nreg]) bit for bit as the last sens_post read them (parity tests)"""
        P, G, Q = np.empty((self.N, self.N)), np.empty((self.N, self.nreg)), np.empty((self.nreg, self.nreg))
        self._chk(self.L.gpemu_test_sens_post_state(self.h, _p(P), _p(G), _p(Q)))
        return P, G, Q

    # second order: pairs j < k at p = j (2 d - j - 1) / 2 + (k - j - 1)
    def _box(self, what, lo, hi):
        lo, hi = _a(lo).ravel(), _a(hi).ravel()
        if lo.size != self.d or hi.size != self.d:
            raise GpemuError(ERR_ARG, f"{what}: one bound pair per coordinate")
        return lo, hi

    # expected reduction of the IMSE (s_all of sens_post) by one more run at each candidate
    def design_gain(self, lo, hi, Xq):
        """Xq[M, d] -> dict(gain[M], num[M], var[M]): gain = num / var = s_all(design) - s_all(design + {x*})"""
        lo, hi = self._box("design_gain", lo, hi)
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        gain, num, var = np.empty(M), np.empty(M), np.empty(M)
        self._chk(self.L.gpemu_design_gain(self.h, _p(lo), _p(hi), M, _p(Xq), _p(gain), _p(num), _p(var)))
        return dict(gain=gain, num=num, var=var)

    def design_gain_dev(self, lo, hi, M, xq_dev, gain_dev, num_dev=None, var_dev=None):
        """lo, hi: HOST bounds; xq_dev (M x d), gain_dev, num_dev, var_dev (M each; the last two may be None): device memory"""
        lo, hi = self._box("design_gain_dev", lo, hi)
        self._chk(self.L.gpemu_design_gain_dev(self.h, _p(lo), _p(hi), M, xq_dev, gain_dev, num_dev, var_dev))

    def design_state(self, M):
        """-> (a[M, N], b[M, nreg]) bit for bit as the last block of the last design_gain read them (parity tests)"""
        a, b = np.empty((M, self.N)), np.empty((M, self.nreg))
        self._chk(self.L.gpemu_test_design_state(self.h, M, _p(a), _p(b)))
        return a, b

    def design_batch_state(self, M, nbatch):
        """-> (lambda[M, nbatch], mu[M, nbatch], E[nbatch, nbatch]) of this context's part in the last design_batch, bit for bit"""
        lam, mu, E = np.empty((M, nbatch)), np.empty((M, nbatch)), np.empty((nbatch, nbatch))
        self._chk(self.L.gpemu_test_design_batch_state(self.h, M, nbatch, _p(lam), _p(mu), _p(E)))
        return lam, mu, E

    # gain over a weighted set of target points
    def design_target_set(self, Xt, weight=None):
        """Xt[S, d], weight[S] (None: 1 / S each) -> dict(target_var, var_t[S]): the resident target store of this context"""
        Xt = _a(Xt).reshape(-1, self.d)
        S = Xt.shape[0]
        w = None if weight is None else _a(weight).ravel()
        if w is not None and w.size != S:
            raise GpemuError(ERR_ARG, "design_target_set: one weight per target")
        tv, vt = np.empty(1), np.empty(S)
        self._chk(self.L.gpemu_design_target_set(self.h, S, _p(Xt), _po(w), _p(tv), _p(vt)))
        return dict(target_var=tv[0], var_t=vt)

    def design_target_set_dev(self, S, xt_dev, weight=None, target_var_dev=None, var_t_dev=None):
        """xt_dev (S x d), target_var_dev (1), var_t_dev (S): device memory, the last two may be None; weight: HOST or None"""
        w = None if weight is None else _a(weight).ravel()
        if w is not None and w.size != S:
            raise GpemuError(ERR_ARG, "design_target_set_dev: one weight per target")
        self._chk(self.L.gpemu_design_target_set_dev(self.h, S, xt_dev, _po(w), target_var_dev, var_t_dev))

    def design_target_gain(self, Xq):
        """Xq[M, d] -> dict(gain[M], num[M], var[M]): gain = num / var = the drop of the weighted variance over the targets"""
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        gain, num, var = np.empty(M), np.empty(M), np.empty(M)
        self._chk(self.L.gpemu_design_target_gain(self.h, M, _p(Xq), _p(gain), _p(num), _p(var)))
        return dict(gain=gain, num=num, var=var)

    def design_target_gain_dev(self, M, xq_dev, gain_dev, num_dev=None, var_dev=None):
        """xq_dev (M x d), gain_dev, num_dev, var_dev (M each; the last two may be None): device memory"""
        self._chk(self.L.gpemu_design_target_gain_dev(self.h, M, xq_dev, gain_dev, num_dev, var_dev))

    def design_target_release(self):
        self._chk(self.L.gpemu_design_target_release(self.h))

    def design_target_state(self, which, npoints):
        """-> (u[n, N], r[n, nreg], qr[n, nreg]) bit for bit as the sweep reads them: which = 0 the targets, 1 the last candidate block"""
        u, r, qr = np.empty((npoints, self.N)), np.empty((npoints, self.nreg)), np.empty((npoints, self.nreg))
        self._chk(self.L.gpemu_test_design_target_state(self.h, which, npoints, _p(u), _p(r), _p(qr)))
        return u, r, qr

    def sens_pairs(self, lo, hi, other=None):
        """-> cov_pair[d (d - 1) / 2] of this context and `other` (default: itself) on one design"""
        lo, hi = self._box("sens_pairs", lo, hi)
        out = np.empty(self.d * (self.d - 1) // 2)
        self._chk(self.L.gpemu_sens_pairs(self.h, (self if other is None else other).h, _p(lo), _p(hi), _p(out)))
        return out

    def sens_pairs_dev(self, lo, hi, out_dev, other=None):
        """lo, hi: HOST bounds; out_dev: d (d - 1) / 2 doubles on the device"""
        lo, hi = self._box("sens_pairs_dev", lo, hi)
        self._chk(self.L.gpemu_sens_pairs_dev(self.h, (self if other is None else other).h, _p(lo), _p(hi), out_dev))

    def sens_pairs_post(self, lo, hi):
        """-> s_pair[d (d - 1) / 2]"""
        lo, hi = self._box("sens_pairs_post", lo, hi)
        out = np.empty(self.d * (self.d - 1) // 2)
        self._chk(self.L.gpemu_sens_pairs_post(self.h, _p(lo), _p(hi), _p(out)))
        return out

    def sens_pairs_post_dev(self, lo, hi, out_dev):
        """lo, hi: HOST bounds; out_dev: d (d - 1) / 2 doubles on the device"""
        lo, hi = self._box("sens_pairs_post_dev", lo, hi)
        self._chk(self.L.gpemu_sens_pairs_post_dev(self.h, _p(lo), _p(hi), out_dev))

    def sens_joint(self, lo, hi, j, k, xj, xk):
        """-> (e0, joint[npts], inter[npts]) at the points (x_j, x_k) = (xj[g], xk[g])"""
        lo, hi = self._box("sens_joint", lo, hi)
        xj, xk = _a(xj).ravel(), _a(xk).ravel()
        if xj.size != xk.size:
            raise GpemuError(ERR_ARG, "sens_joint: one value of x_k per value of x_j")
        e0, joint, inter = np.empty(1), np.empty(xj.size), np.empty(xj.size)
        self._chk(self.L.gpemu_sens_joint(self.h, _p(lo), _p(hi), j, k, xj.size, _p(xj), _p(xk), _p(e0), _p(joint), _p(inter)))
        return e0[0], joint, inter

    def pred_state(self):
        """-> (beta[nreg], gamma[N]) bit for bit as the prediction state holds them (parity tests)"""
        beta, gamma = np.empty(self.nreg), np.empty(self.N)
        self._chk(self.L.gpemu_test_pred_state(self.h, _p(beta), _p(gamma)))
        return beta, gamma

    def chol_inverse(self, A):
        A = _a(A).copy()
        ld, info = C.c_double(np.nan), C.c_int(0)
        rc = self._chk(self.L.gpemu_chol_inverse(self.h, A.shape[0], _p(A), A.shape[1], C.byref(ld), C.byref(info)),
                       allow=(ERR_NOT_PD,))
        return A, ld.value, info.value, rc

    def symm_apply(self, A, V):
        A, V = _a(A), _a(V).reshape(-1, np.shape(A)[0])
        out = np.empty_like(V)
        self._chk(self.L.gpemu_symm_apply(self.h, A.shape[0], _p(A), A.shape[1], V.shape[0], _p(V), _p(out)))
        return out

    def set_mode(self, flags):
        self._chk(self.L.gpemu_set_mode(self.h, int(flags)))

    def get_mode(self):
        return self.L.gpemu_get_mode(self.h)

    def symm_invalidate(self):
        self._chk(self.L.gpemu_symm_invalidate(self.h))

    def symm_pin(self, pinned=True):
        self._chk(self.L.gpemu_symm_pin(self.h, 1 if pinned else 0))

    def derivative_gauss(self, xcol, theta_len):
        xcol = _a(xcol)
        out = np.empty((xcol.size, xcol.size))
        self._chk(self.L.gpemu_derivative_gauss(self.h, xcol.size, _p(xcol), float(theta_len), _p(out), xcol.size))
        return out

    def trace_product(self, A, B):
        A, B = _a(A), _a(B)
        t = C.c_double(np.nan)
        self._chk(self.L.gpemu_trace_product(self.h, A.shape[0], _p(A), A.shape[1], _p(B), B.shape[1], C.byref(t)))
        return t.value

    def cinverse(self):
        out = np.empty((self.N, self.N))
        self._chk(self.L.gpemu_get_cinverse(self.h, _p(out)))
        return out

    def predict(self, Xq):
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        mean, var = np.empty(M), np.empty(M)
        self._chk(self.L.gpemu_predict_batch(self.h, M, _p(Xq), _p(mean), _p(var)))
        return mean, var

    def predict_dev(self, M, xq_dev, mean_dev, var_dev):
        self._chk(self.L.gpemu_predict_batch_dev(self.h, M, xq_dev, mean_dev, var_dev))

    # the posterior mean alone: fused k-vector . gamma sweep, no product with L^-1 and no batch buffers
    def predict_mean(self, Xq):
        Xq = _a(Xq).reshape(-1, self.d)
        mean = np.empty(Xq.shape[0])
        self._chk(self.L.gpemu_predict_mean(self.h, Xq.shape[0], _p(Xq), _p(mean)))
        return mean

    def predict_mean_dev(self, M, xq_dev, mean_dev):
        self._chk(self.L.gpemu_predict_mean_dev(self.h, M, xq_dev, mean_dev))

    def predict_mean_enqueue(self, Xq):
        self._pred_enqueue("mean", Xq)

    def predict_mean_collect(self):
        return self._pred_collect("mean", "m")[0]

    # the posterior mean and its gradient with respect to the query point: one fused sweep
    def predict_mean_grad(self, Xq, want_mean=True):
        """-> (mean[M] or None, grad[M, d])"""
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        mean = np.empty(M) if want_mean else None
        grad = np.empty((M, self.d))
        self._chk(self.L.gpemu_predict_mean_grad(self.h, M, _p(Xq), _p(mean) if want_mean else None, _p(grad)))
        return mean, grad

    def predict_mean_grad_dev(self, M, xq_dev, mean_dev, grad_dev):
        self._chk(self.L.gpemu_predict_mean_grad_dev(self.h, M, xq_dev, mean_dev, grad_dev))

    def predict_mean_grad_enqueue(self, Xq):
        self._pred_enqueue("mean_grad", Xq)

    def predict_mean_grad_collect(self):
        return self._pred_collect("mean_grad", "mg")

    # mean, variance and the variance's gradient with respect to the query point: two N^2 products and a fused sweep
    # (DESIGN.md 4.10); uses the batch buffers of predict_batch
    def predict_var_grad(self, Xq, want_mean=True, want_var=True):
        """-> (mean[M] or None, var[M] or None, grad[M, d])"""
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        mean = np.empty(M) if want_mean else None
        var = np.empty(M) if want_var else None
        grad = np.empty((M, self.d))
        self._chk(self.L.gpemu_predict_var_grad(self.h, M, _p(Xq), _p(mean) if want_mean else None,
                                                _p(var) if want_var else None, _p(grad)))
        return mean, var, grad

    def predict_var_grad_dev(self, M, xq_dev, mean_dev, var_dev, grad_dev):
        self._chk(self.L.gpemu_predict_var_grad_dev(self.h, M, xq_dev, mean_dev, var_dev, grad_dev))

    def predict_var_grad_enqueue(self, Xq):
        self._pred_enqueue("var_grad", Xq)

    def predict_var_grad_collect(self):
        return self._pred_collect("var_grad", "mvg")

    # the joint posterior covariance between the query points of one call: the sweep of predict_batch plus
    # one symmetric M^2 N product; uses the batch buffers of predict_batch
    def predict_cov(self, Xq, want_mean=True):
        """-> (mean[M] or None, cov[M, M]); cov is the covariance itself, both triangles"""
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        mean = np.empty(M) if want_mean else None
        cov = np.empty((M, M))
        self._chk(self.L.gpemu_predict_cov(self.h, M, _p(Xq), _p(mean) if want_mean else None, _p(cov)))
        return mean, cov

    def predict_cov_dev(self, M, xq_dev, mean_dev, cov_dev):
        self._chk(self.L.gpemu_predict_cov_dev(self.h, M, xq_dev, mean_dev, cov_dev))

    # hold-out validation and joint draws at the query points of one call: S = Sigma + diag(noise) factored on
    # the device, the factor kept resident for predict_joint_draw
    def predict_joint_factor(self, Xq, noise=None, yobs=None):
        """-> dict(mean[M], var[M], werr[nobs, M], maha[nobs], logdet, logpdf[nobs], info, status); status is OK or ERR_NOT_PD
        (then info is the 1-based row of the failed pivot, mean and var are valid and the rest is NaN)"""
        Xq = _a(Xq).reshape(-1, self.d)
        M = Xq.shape[0]
        noise = None if noise is None else _a(noise).reshape(M)
        yobs = None if yobs is None else _a(yobs).reshape(-1, M)
        nobs = 0 if yobs is None else yobs.shape[0]
        mean, var = np.empty(M), np.empty(M)
        werr, maha, logpdf = np.empty((nobs, M)), np.empty(nobs), np.empty(nobs)
        logdet, info = C.c_double(np.nan), C.c_int(-1)
        rc = self.L.gpemu_predict_joint_factor(self.h, M, _p(Xq), None if noise is None else _p(noise), nobs,
                                               _p(yobs) if nobs else None, _p(mean), _p(var), _p(werr), _p(maha), C.byref(logdet),
                                               _p(logpdf), C.byref(info))
        self._chk(rc, allow=(ERR_NOT_PD,))
        return dict(mean=mean, var=var, werr=werr, maha=maha, logdet=logdet.value, logpdf=logpdf, info=info.value, status=rc)

    def predict_joint_factor_dev(self, M, xq_dev, noise_dev, nobs, yobs_dev, mean_dev, var_dev, werr_dev, stat_dev, info_dev):
        self._chk(self.L.gpemu_predict_joint_factor_dev(self.h, M, xq_dev, noise_dev, nobs, yobs_dev, mean_dev, var_dev, werr_dev,
                                                        stat_dev, info_dev))

    def predict_joint_draw(self, z):
        """z: ndraw rows of M standard normals -> out[ndraw, M] = mean + L_S z, from the factor the last predict_joint_factor left"""
        z = _a(z)
        z = z.reshape(1, -1) if z.ndim == 1 else z
        out = np.empty_like(z)
        self._chk(self.L.gpemu_predict_joint_draw(self.h, z.shape[0], _p(z), _p(out)))
        return out

    def predict_joint_draw_dev(self, ndraw, z_dev, out_dev):
        self._chk(self.L.gpemu_predict_joint_draw_dev(self.h, ndraw, z_dev, out_dev))

    def predict_joint_release(self):
        self._chk(self.L.gpemu_predict_joint_release(self.h))

    # -- memory / sync / profiling ------------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.gpemu_dev_alloc(self.h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        self._chk(self.L.gpemu_dev_free(self.h, p))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.gpemu_dev_upload(self.h, dptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, dptr, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        self._chk(self.L.gpemu_dev_download(self.h, out.ctypes.data_as(C.c_void_p), dptr, out.nbytes))
        return out

    def sync(self):
        self._chk(self.L.gpemu_sync(self.h))

    def prof_begin(self, cls):
        self._chk(self.L.gpemu_prof_begin(self.h, cls))

    def prof_end(self):
        n = C.c_int(0)
        ms, fl, by = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.L.gpemu_prof_end(self.h, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(n=n.value, ms=ms.value, flops=fl.value, bytes=by.value)

    # -- building blocks ------------------------------------------------------
    def test_gemm_nt(self, A, B, Cm, alpha=1.0, beta=0):
        A, B, Cm = _a(A), _a(B), _a(Cm).copy()
        m, k = A.shape
        n = B.shape[0]
        self._chk(self.L.gpemu_test_gemm_nt(self.h, m, n, k, alpha, beta, _p(A), _p(B), _p(Cm)))
        return Cm

    def test_gemm_launch(self, arena, **args):
        """one GEMM launch in any of its modes on operands inside `arena` (gpemu_test_gemm_launch; args: the fields of
        GemmLaunchArgs) -> (the arena after the launch, info word per matrix).  GpemuError(ERR_ARG) for a refused launch."""
        out = _a(arena).ravel().copy()
        a = GemmLaunchArgs(**{k: float(v) if k == "alpha" else int(v) for k, v in args.items()})
        info = np.zeros(max(a.nbatch, 1), dtype=np.int32)
        self._chk(self.L.gpemu_test_gemm_launch(self.h, _p(out), out.size, C.byref(a), info.ctypes.data_as(_ip)))
        return out, info

    def test_update_launch(self, arena, **args):
        """one trailing update of the factorisation, as production makes it, on tall matrices inside `arena`
        (gpemu_test_update_launch; args: the fields of UpdateLaunchArgs, default ride = 1) -> (the arena after the update, info
        word per matrix).  GpemuError(ERR_ARG) for a refused call."""
        out = _a(arena).ravel().copy()
        a = UpdateLaunchArgs(**{k: int(v) for k, v in dict(dict(ride=1), **args).items()})
        info = np.zeros(max(a.nbatch, 1), dtype=np.int32)
        self._chk(self.L.gpemu_test_update_launch(self.h, _p(out), out.size, C.byref(a), info.ctypes.data_as(_ip)))
        return out, info

    def test_leaf_launch(self, arena, **args):
        """one call of the Cholesky leaf launchers on a matrix inside `arena` (gpemu_test_leaf_launch; args: the fields of
        LeafLaunchArgs, defaults staged = -1, pre = 1, c0b = -1) -> (the arena after the launch, info word per matrix).
        GpemuError(ERR_ARG) for a refused launch."""
        out = _a(arena).ravel().copy()
        a = LeafLaunchArgs(**{k: int(v) for k, v in dict(dict(staged=-1, pre=1, c0b=-1), **args).items()})
        info = np.zeros(max(a.nbatch, 1), dtype=np.int32)
        self._chk(self.L.gpemu_test_leaf_launch(self.h, _p(out), out.size, C.byref(a), info.ctypes.data_as(_ip)))
        return out, info

    def test_grad_sums(self, thetas, a, z, gram=None, form=0, gram_dist=-1, clamp=-1):
        """the gradient's reduction kernels once on caller-chosen operands (gpemu_test_grad_sums), for the model and mode of
        the context.  thetas: nb x nthetas, a: nb x N x N (lower triangle read), z: nb x N x (1 + nreg), gram (exact form):
        nb x (1 + nreg) x (1 + nreg) -> dict(alpha (nb, N), beta (nb, nreg), part (nb, ntiles, 2d + 2), sums (nb, 2d + 2));
        what the form does not define is NaN.  GpemuError(ERR_ARG) for a refused call."""
        N, d, nreg = self.N, self.d, self.nreg
        th = _a(thetas)
        th = th.reshape(-1, th.shape[-1])
        nb = th.shape[0]
        a, z = _a(a).reshape(nb, N, N), _a(z).reshape(nb, N, 1 + nreg)
        g = None if gram is None else _a(gram).reshape(nb, 1 + nreg, 1 + nreg)
        nt = (N + 63) // 64
        out = dict(alpha=np.full((nb, N), np.nan), beta=np.full((nb, nreg), np.nan),
                   part=np.full((nb, nt * (nt + 1) // 2, 2 * d + 2), np.nan), sums=np.full((nb, 2 * d + 2), np.nan))
        args = GradSumsArgs(thetas=_p(th), a=_p(a), z=_p(z), gram=None if g is None else _p(g), alpha_out=_p(out["alpha"]),
                            beta_out=_p(out["beta"]), part_out=_p(out["part"]), sums_out=_p(out["sums"]), nb=nb,
                            nthetas=th.shape[1], form=int(form), gram_dist=int(gram_dist), clamp=int(clamp))
        self._chk(self.L.gpemu_test_grad_sums(self.h, C.byref(args)))
        return out

    def test_fill_launch(self, op, thetas, out, form=-1, rrows=None, rstride=0, Rp=64, guard=0, Xq=None):
        """one call of a covariance fill launcher for the context's model (gpemu_test_fill_launch): `out` is the caller's
        prefilled region (STAGE: nb x (Np + Rp + guard) x Np, KVEC: (Mp + guard) x Np, FULL: (Np + guard) x Np) -> (the
        region after the launch, form per matrix, norm2 per matrix).  Rp is always passed explicitly (production's is 64), so
        the length the entry reads from rrows, (nb - 1) * rstride + Rp * Np, is checked here against what was given.
        GpemuError(ERR_ARG) for a refused launch; the exception carries the region as the entry left it (`region`)."""
        th = _a(thetas)
        th = th.reshape(-1, th.shape[-1])
        nb = th.shape[0]
        res = _a(out).copy()
        rr = None if rrows is None else _a(rrows)
        xq = None if Xq is None else _a(Xq).reshape(-1, self.d)
        if Rp == 0:
            raise ValueError("Rp = 0 (the context's own) is not offered here: pass the number of rows")
        if rr is not None and op == FILL_STAGE and Rp > 0 and rstride >= 0:
            need = (nb - 1) * int(rstride) + int(Rp) * ((self.N + 63) // 64 * 64)
            if rr.size < need:
                raise ValueError(f"rrows holds {rr.size} values, the launch reads {need}")
        form_out, norm2 = np.full(nb, -1, dtype=np.int32), np.full(nb, np.nan)
        args = FillLaunchArgs(thetas=_p(th), rrows=None if rr is None else _p(rr), xq=None if xq is None else _p(xq),
                              out=_p(res), norm2_out=_p(norm2), form_out=form_out.ctypes.data_as(_ip), out_len=res.size,
                              rstride=int(rstride), op=int(op), form=int(form), nb=nb, nthetas=th.shape[1],
                              M=0 if xq is None else xq.shape[0], Rp=int(Rp), guard=int(guard))
        try:
            self._chk(self.L.gpemu_test_fill_launch(self.h, C.byref(args)))
        except GpemuError as e:
            e.region = res
            raise
        return res, form_out, norm2

    def test_resident_launch(self, op, allow=(), **args):
        """one call of a launcher that reads the resident factor (gpemu_test_resident_launch).  args: the fields of
        ResidentLaunchArgs; an array (float64 regions, int32 tables) is copied, passed with its length where the struct has
        one, and comes back as the entry left it -> (dict of the regions after the launch, status).  GpemuError for a status
        that is neither OK nor in `allow` (ERR_ARG for a refused launch, ERR_NOT_PD from RES_LGO_TAIL)."""
        ptrs = {f for f, t in ResidentLaunchArgs._fields_ if t in (_dp, _ip)}
        dbl = {f for f, t in ResidentLaunchArgs._fields_ if t is _dp}
        kw, out = dict(op=int(op)), {}
        for k, v in args.items():
            if k not in ptrs:
                kw[k] = int(v)
            elif v is not None:
                a = np.array(v, dtype=np.float64 if k in dbl else np.int32, order="C").ravel()
                out[k] = a
                kw[k] = a.ctypes.data_as(_dp if k in dbl else _ip)
                if k in _RES_LEN and _RES_LEN[k] not in args:
                    kw[_RES_LEN[k]] = a.size
        # the lengths the entry takes from the shape: what it would read from or write to a shorter host array is refused here
        g = lambda k: kw.get(k, 0)
        fixed = dict(betaq=g("nreg") + g("nreg") ** 2, y=g("N"), res=2 * g("nbc"), info=g("nbc"), stat=3 * g("ngroups"), info_out=g("ngroups"),
                     colrow=g("N"), members=g("nmembers"), moff=g("ngroups"), bsize=g("ngroups"), var=g("out_len"), werr=g("out_len"))
        for k, n in fixed.items():
            if k in out and out[k].size < n:
                raise ValueError(f"{k} holds {out[k].size} values, the entry takes {n}")
        rc = self._chk(self.L.gpemu_test_resident_launch(self.h, C.byref(ResidentLaunchArgs(**kw))), allow=allow)
        return out, rc

    def trace_dump(self, path):
        self._chk(self.L.gpemu_trace_dump(self.h, str(path).encode()))

    def gemm_bench(self, m, n, k, ld=0, cfg=0, tri=0, beta=1, reps=5):
        ms, fl = C.c_double(0), C.c_double(0)
        self._chk(self.L.gpemu_test_gemm_bench(self.h, m, n, k, ld, cfg, tri, beta, reps, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    def staged_matrix(self, thetas, b=0):
        """N x N block of matrix b as the batch staging launch (FILL_LOWER) leaves it; upper tiles are not written"""
        th = _a(thetas).reshape(-1, np.shape(thetas)[-1])
        out = np.zeros((self.N, self.N))
        self._chk(self.L.gpemu_test_staged_matrix(self.h, th.shape[0], _p(th), th.shape[1], int(b), _p(out)))
        return out

    def test_potrf(self, A):
        A = _a(A).copy()
        info = C.c_int(0)
        self._chk(self.L.gpemu_test_potrf(self.h, A.shape[0], _p(A), C.byref(info)))
        return A, info.value
