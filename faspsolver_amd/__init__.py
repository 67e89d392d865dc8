"""faspsolver_amd -- host-side mirror of the C-ABI in include/fasp_hip.h.

The product is libfasp_hip.so (C host code + hand-written HIP kernels for gfx950,
built by faspsolver_amd/csrc/Makefile).  This module only binds it with ctypes and
mirrors the reference's call signatures (same names, argument meaning and error
behaviour as base/src/SolCSR.c:476, AuxParam.c:431/572, ...), so that parity tests
read like the reference's own drivers.  It never computes anything itself and has no
CPU fallback: if the shared library is missing it raises; if there is no GPU the
library's compute entry points return ERROR_MISC.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _types as T
from ._types import *  # noqa: F401,F403  (constants + struct mirrors)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FASP_HIP_LIB") or os.path.join(_HERE, "libfasp_hip.so")   # (FASP_HIP_LIB: a development build beside the product one, tools/build_variant.sh)
_lib = None

EXPORTS = [  # every symbol include/fasp_hip.h declares
    "fasp_param_amg_init", "fasp_param_solver_init", "fasp_solver_dcsr_krylov_amg",
    "fasp_blas_dcsr_mxv", "fasp_blas_dcsr_aAxpy", "fasp_blas_darray_dotprod",
    "fasp_blas_darray_norm2", "fasp_blas_darray_norminf", "fasp_blas_darray_axpy",
    "fasp_blas_darray_axpby", "fasp_smoother_dcsr_jacobi",
    "fasp_blas_dbsr_mxv", "fasp_blas_dbsr_aAxpy", "fasp_dbsr_getdiaginv", "fasp_smoother_dbsr_jacobi1",
    "fasp_solver_dbsr_pcg", "fasp_solver_dbsr_pbcgs", "fasp_solver_dbsr_pgmres", "fasp_solver_dbsr_pvgmres",
    "fasp_solver_dbsr_pvfgmres", "fasp_hip_bsr_precond_setup", "fasp_hip_bsr_precond_fct", "fasp_hip_bsr_precond_free",
    "fasp_hip_param_input", "fasp_fwrapper_dcsr_krylov_amg_", "fasp_dcsrvec_read2", "fasp_dvec_read",
    "fasp_dbsr_read", "fasp_dcoo_read", "fasp_dcoo_read1", "fasp_dcoo_shift_read", "fasp_dmtx_read", "fasp_dmtxsym_read", "fasp_dvec_write", "fasp_dcsr_write_coo", "fasp_dcsrvec_write2", "fasp_fwrapper_dcsr_amg_", "fasp_fwrapper_dbsr_krylov_amg_", "fasp_hip_free_bsr", "fasp_hip_comm_selftest", "fasp_hip_amg_kernel_info", "fasp_hip_coarse_kernel_info", "fasp_hip_bsr_coarse_kernel_info", "fasp_hip_coding_selftest", "fasp_solver_amg", "fasp_solver_famg", "fasp_hip_amg_solve", "fasp_precond_diag", "fasp_precond_dbsr_diag", "fasp_solver_dcsr_itsolver", "fasp_solver_dcsr_krylov", "fasp_solver_dcsr_krylov_diag", "fasp_solver_dbsr_itsolver", "fasp_solver_dbsr_krylov", "fasp_solver_dbsr_krylov_diag", "fasp_hip_mxv_csr", "fasp_hip_mxv_bsr", "fasp_solver_matfree_init", "fasp_solver_pcg", "fasp_solver_pbcgs", "fasp_solver_pgcg", "fasp_solver_pminres", "fasp_solver_pgmres", "fasp_solver_pvgmres", "fasp_solver_pvfgmres", "fasp_solver_itsolver", "fasp_solver_krylov", "fasp_solver_dcsr_pcg", "fasp_solver_dcsr_pminres", "fasp_solver_dcsr_pgcg", "fasp_solver_dcsr_pgcr", "fasp_solver_dcsr_pbcgs", "fasp_solver_dcsr_pgmres", "fasp_solver_dcsr_pvgmres",
    "fasp_solver_dcsr_pvfgmres", "fasp_hip_precond_setup", "fasp_hip_precond_fct", "fasp_hip_precond_free",
    "fasp_hip_time_bsr_mxv", "fasp_solver_dbsr_krylov_amg", "fasp_hip_bsr_amg_create", "fasp_hip_bsr_amg_create_host",
    "fasp_hip_bsr_amg_destroy", "fasp_hip_bsr_amg_num_levels", "fasp_hip_bsr_amg_get_matrix",
    "fasp_hip_bsr_amg_get_diaginv", "fasp_hip_bsr_solve",
    "fasp_hip_set_device", "fasp_hip_device_count", "fasp_hip_device_identity", "fasp_hip_available",
    "fasp_hip_amg_create", "fasp_hip_amg_create_host", "fasp_hip_amg_upload",
    "fasp_hip_amg_destroy", "fasp_hip_amg_num_levels", "fasp_hip_amg_get_matrix",
    "fasp_hip_amg_get_cfmark", "fasp_hip_solve", "fasp_hip_set_rhs", "fasp_hip_set_guess",
    "fasp_hip_solve_resident", "fasp_hip_get_solution", "fasp_hip_device_synchronize",
    "fasp_hip_precond_amg",
    "fasp_hip_poisson7pt", "fasp_hip_aniso27pt", "fasp_hip_free_system", "fasp_hip_time_kernel", "fasp_hip_measure_ceilings", "fasp_hip_amg_publish", "fasp_hip_amg_attach", "fasp_hip_amg_unpublish",
    "fasp_precond_setup", "fasp_precond_amg", "fasp_precond_famg", "fasp_precond_amli", "fasp_precond_namli", "fasp_amg_data_create", "fasp_amg_data_free", "fasp_param_amg_to_prec", "fasp_param_prec_to_amg", "fasp_mem_free", "fasp_mem_calloc", "fasp_dvec_alloc", "fasp_dvec_set", "fasp_dvec_free", "fasp_dvec_create", "fasp_dcsr_create", "fasp_dcsr_free", "fasp_smoother_dcsr_gs", "fasp_smoother_dcsr_sor", "fasp_smoother_dcsr_L1diag",
    "fasp_hip_tune", "fasp_hip_comm_unique_id", "fasp_hip_comm_init", "fasp_hip_comm_finalize",
    "fasp_hip_comm_rank", "fasp_hip_comm_size", "fasp_hip_version", "fasp_hip_comm_init_shm",
    "fasp_hip_dist_plan", "fasp_hip_dist_level_info", "fasp_hip_dist_get_matrix",
    "fasp_hip_dist_get_list",
    "fasp_blas_dcsr_vmv", "fasp_blas_dcsr_mxv_agg", "fasp_blas_dcsr_aAxpy_agg", "fasp_blas_darray_ax",
    "fasp_blas_darray_axpyz", "fasp_blas_darray_norm1", "fasp_darray_cp", "fasp_darray_set", "fasp_dvec_isnan",
    "fasp_hip_time_matrix", "fasp_hip_bsr_dist_info", "fasp_hip_seq_schedule_selftest", "fasp_hip_seq_chain_selftest", "fasp_hip_cluster_order", "fasp_hip_permute_csr", "fasp_hip_comm_init_ipc", "fasp_hip_comm_stats", "fasp_hip_comm_timing", "fasp_hip_estream_selftest", "fasp_hip_sell_selftest", "fasp_hip_csr_plan", "fasp_hip_coarse_plan", "fasp_hip_bsr_coarse_plan", "fasp_hip_level_op", "fasp_hip_matrix_op", "fasp_hip_matrix_traits", "fasp_hip_matrix_traits2", "fasp_hip_csr_plan2", "fasp_hip_rgroup_selftest",
    "fasp_param_ilu_init", "fasp_ilu_data_create", "fasp_ilu_data_free", "fasp_mem_iludata_check", "fasp_ilu_dcsr_setup",
    "fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward", "fasp_solver_dcsr_krylov_ilu",
    "fasp_solver_dcsr_krylov_ilu_M", "fasp_smoother_dcsr_ilu", "fasp_fwrapper_dcsr_krylov_ilu_",
    "fasp_hip_ilu_resident_count", "fasp_hip_ilu_time", "fasp_hip_ilu_schedule",
    "fasp_ilu_dbsr_setup", "fasp_precond_dbsr_ilu", "fasp_solver_dbsr_krylov_ilu", "fasp_smoother_dbsr_ilu",
    "fasp_fwrapper_dbsr_krylov_ilu_",
    "fasp_hip_bsr_amg_get_ilu", "fasp_hip_bsr_amg_ilu_info", "fasp_hip_bsr_amg_ilu_smooth_time",
    "fasp_hip_bsr_sweep", "fasp_hip_csr_sweep",
    "fasp_blas_dcsr_rap", "fasp_hip_dcsr_rap", "fasp_hip_rap_info", "fasp_hip_rap_device_count", "fasp_hip_rap_time",
    "fasp_dstr_create", "fasp_dstr_alloc", "fasp_dstr_free", "fasp_dstr_cp", "fasp_format_dstr_dcsr", "fasp_dstr_read",
    "fasp_blas_dstr_aAxpy", "fasp_blas_dstr_mxv", "fasp_precond_dstr_diag", "fasp_solver_dstr_pcg", "fasp_solver_dstr_pbcgs",
    "fasp_solver_dstr_pminres", "fasp_solver_dstr_pgmres", "fasp_solver_dstr_pvgmres", "fasp_solver_dstr_itsolver",
    "fasp_solver_dstr_krylov", "fasp_solver_dstr_krylov_diag", "fasp_hip_mxv_str", "fasp_hip_str_form", "fasp_hip_time_str_mxv",
    "fasp_ilu_dstr_setup0", "fasp_ilu_dstr_setup1", "fasp_precond_dstr_ilu0", "fasp_precond_dstr_ilu1", "fasp_solver_dstr_krylov_ilu",
    "fasp_hip_str_ilu_form", "fasp_hip_str_ilu_apply", "fasp_hip_time_str_ilu",
    "fasp_smoother_dstr_jacobi", "fasp_smoother_dstr_jacobi1", "fasp_smoother_dstr_gs", "fasp_smoother_dstr_gs1",
    "fasp_smoother_dstr_gs_ascend", "fasp_smoother_dstr_gs_descend", "fasp_smoother_dstr_gs_order", "fasp_smoother_dstr_gs_cf",
    "fasp_smoother_dstr_sor", "fasp_smoother_dstr_sor1", "fasp_smoother_dstr_sor_ascend", "fasp_smoother_dstr_sor_descend",
    "fasp_smoother_dstr_sor_order", "fasp_smoother_dstr_sor_cf",
    "fasp_hip_str_sweep", "fasp_hip_str_sweep_form", "fasp_hip_str_sweep_levels", "fasp_hip_time_str_sweep",
    "fasp_generate_diaginv_block", "fasp_smoother_dstr_swz", "fasp_precond_dstr_blockgs", "fasp_solver_dstr_krylov_blockgs",
    "fasp_hip_str_swz", "fasp_hip_str_swz_levels", "fasp_hip_time_str_swz",
    "fasp_param_swz_init", "fasp_dcsr_sympart", "fasp_dcsr_shift", "fasp_sparse_mis", "fasp_swz_dcsr_setup", "fasp_dcsr_swz_forward",
    "fasp_dcsr_swz_backward", "fasp_precond_swz", "fasp_swz_data_free", "fasp_solver_dcsr_krylov_swz",
    "fasp_hip_csr_swz_levels", "fasp_hip_csr_swz", "fasp_hip_csr_swz_resident_count", "fasp_hip_time_csr_swz",
    "fasp_hip_csr_swz_runs", "fasp_hip_amg_get_swz", "fasp_hip_amg_swz_info", "fasp_hip_amg_swz_sweep_time", "fasp_hip_amg_swz_levels",
    "fasp_smoother_dbsr_jacobi", "fasp_smoother_dbsr_jacobi_setup", "fasp_smoother_dbsr_gs", "fasp_smoother_dbsr_gs1",
    "fasp_smoother_dbsr_gs_ascend", "fasp_smoother_dbsr_gs_ascend1", "fasp_smoother_dbsr_gs_descend", "fasp_smoother_dbsr_gs_descend1",
    "fasp_smoother_dbsr_gs_order1", "fasp_smoother_dbsr_gs_order2", "fasp_smoother_dbsr_sor", "fasp_smoother_dbsr_sor1",
    "fasp_smoother_dbsr_sor_ascend", "fasp_smoother_dbsr_sor_descend", "fasp_smoother_dbsr_sor_order",
    "fasp_hip_bsr_smoother_create", "fasp_hip_bsr_smoother_apply", "fasp_hip_bsr_smoother_destroy",
    "fasp_hip_bsr_smoother_info", "fasp_hip_bsr_sweep_plan", "fasp_hip_bsr_sweep_time",
    "fasp_solver_dcsr_spcg", "fasp_solver_dcsr_spbcgs", "fasp_solver_dcsr_spminres", "fasp_solver_dcsr_spgmres", "fasp_solver_dcsr_spvgmres",
    "fasp_solver_dcsr_itsolver_s", "fasp_solver_dcsr_krylov_s", "fasp_solver_dbsr_spbcgs", "fasp_solver_dbsr_spgmres",
    "fasp_solver_dbsr_spvgmres", "fasp_solver_dstr_spcg", "fasp_solver_dstr_spbcgs", "fasp_solver_dstr_spminres",
    "fasp_solver_dstr_spgmres", "fasp_solver_dstr_spvgmres", "fasp_hip_safe_update_selftest", "fasp_hip_plugin_solve_seconds",
    "fasp_hip_blas1_op", "fasp_hip_level_smooth",
]
SAFE_METHODS = ("spcg", "spbcgs", "spminres", "spgmres", "spvgmres")   # the safe-net Krylov methods (KrySP*.c) ...
SAFE_FORMATS = {"csr": SAFE_METHODS, "bsr": ("spbcgs", "spgmres", "spvgmres"), "str": SAFE_METHODS}   # ... the reference has per format


def build(verbose=False):
    """Compile libfasp_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)


def lib():
    """The loaded shared library (built on demand).  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    L = C.CDLL(LIB_PATH)  # RTLD_LOCAL: the reference-named symbols must not interpose other libraries
    P = C.POINTER
    L.fasp_param_amg_init.argtypes = [P(T.AMG_param)]
    L.fasp_param_solver_init.argtypes = [P(T.ITS_param)]
    L.fasp_solver_dcsr_krylov_amg.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector),
                                              P(T.ITS_param), P(T.AMG_param)]
    L.fasp_blas_dcsr_mxv.argtypes = [P(T.dCSRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dcsr_aAxpy.argtypes = [C.c_double, P(T.dCSRmat), T.c_double_p, T.c_double_p]
    for f in ("fasp_blas_darray_dotprod", "fasp_blas_darray_norm2", "fasp_blas_darray_norminf"):
        getattr(L, f).restype = C.c_double
    L.fasp_blas_darray_dotprod.argtypes = [C.c_int, T.c_double_p, T.c_double_p]
    L.fasp_blas_darray_norm2.argtypes = [C.c_int, T.c_double_p]
    L.fasp_blas_darray_norminf.argtypes = [C.c_int, T.c_double_p]
    L.fasp_blas_darray_axpy.argtypes = [C.c_int, C.c_double, T.c_double_p, T.c_double_p]
    L.fasp_blas_darray_axpby.argtypes = [C.c_int, C.c_double, T.c_double_p, C.c_double,
                                         T.c_double_p]
    L.fasp_blas_dcsr_vmv.restype = C.c_double
    L.fasp_blas_dcsr_vmv.argtypes = [P(T.dCSRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dcsr_mxv_agg.argtypes = [P(T.dCSRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dcsr_aAxpy_agg.argtypes = [C.c_double, P(T.dCSRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_darray_ax.argtypes = [C.c_int, C.c_double, T.c_double_p]
    L.fasp_blas_darray_axpyz.argtypes = [C.c_int, C.c_double, T.c_double_p, T.c_double_p, T.c_double_p]
    L.fasp_blas_darray_norm1.restype = C.c_double
    L.fasp_blas_darray_norm1.argtypes = [C.c_int, T.c_double_p]
    L.fasp_darray_cp.argtypes = [C.c_int, T.c_double_p, T.c_double_p]
    L.fasp_darray_set.argtypes = [C.c_int, T.c_double_p, C.c_double]
    L.fasp_hip_time_matrix.restype = C.c_double
    L.fasp_hip_time_matrix.argtypes = [P(T.dCSRmat), C.c_int, C.c_int, P(C.c_int)]
    L.fasp_dvec_isnan.restype = C.c_short
    L.fasp_dvec_isnan.argtypes = [P(T.dvector)]
    L.fasp_smoother_dcsr_jacobi.argtypes = [P(T.dvector), C.c_int, C.c_int, C.c_int,
                                            P(T.dCSRmat), P(T.dvector), C.c_int, C.c_double]
    L.fasp_blas_dbsr_mxv.argtypes = [P(T.dBSRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dbsr_aAxpy.argtypes = [C.c_double, P(T.dBSRmat), T.c_double_p, T.c_double_p]
    L.fasp_dbsr_getdiaginv.argtypes = [P(T.dBSRmat)]
    L.fasp_dbsr_getdiaginv.restype = T.dvector
    L.fasp_smoother_dbsr_jacobi1.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), T.c_double_p]
    L.fasp_hip_bsr_sweep.argtypes = [P(T.dBSRmat), T.c_double_p, T.c_double_p, T.c_double_p, C.c_int, C.c_int, C.c_double,
                                     P(C.c_int)]
    L.fasp_hip_csr_sweep.argtypes = [P(T.dCSRmat), P(C.c_int), C.c_int, C.c_int, C.c_double, C.c_int, T.c_double_p, T.c_double_p,
                                     P(C.c_int)]
    L.fasp_hip_time_bsr_mxv.argtypes = [P(T.dBSRmat), C.c_int]
    L.fasp_hip_time_bsr_mxv.restype = C.c_double
    L.fasp_solver_dcsr_pcg.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                       C.c_double, C.c_int, C.c_short, C.c_short]
    L.fasp_solver_dcsr_pbcgs.argtypes = L.fasp_solver_dcsr_pcg.argtypes
    L.fasp_solver_dcsr_pminres.argtypes = L.fasp_solver_dcsr_pcg.argtypes
    L.fasp_solver_dcsr_pgcg.argtypes = L.fasp_solver_dcsr_pcg.argtypes
    L.fasp_solver_dcsr_pvgmres.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                           C.c_double, C.c_int, C.c_short, C.c_short, C.c_short]
    L.fasp_solver_dcsr_pvfgmres.argtypes = L.fasp_solver_dcsr_pvgmres.argtypes
    L.fasp_solver_dcsr_pgmres.argtypes = L.fasp_solver_dcsr_pvgmres.argtypes
    L.fasp_solver_dcsr_pgcr.argtypes = L.fasp_solver_dcsr_pvgmres.argtypes
    L.fasp_hip_precond_setup.argtypes = [P(T.dCSRmat), P(T.AMG_param)]
    L.fasp_hip_precond_setup.restype = P(T.precond)
    L.fasp_hip_precond_free.argtypes = [P(T.precond)]
    L.fasp_hip_precond_free.restype = None
    L.fasp_hip_precond_fct.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_hip_precond_fct.restype = None
    L.fasp_solver_dbsr_pcg.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                       C.c_double, C.c_int, C.c_short, C.c_short]
    L.fasp_solver_dbsr_pbcgs.argtypes = L.fasp_solver_dbsr_pcg.argtypes
    L.fasp_solver_dbsr_pvgmres.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                           C.c_double, C.c_int, C.c_short, C.c_short, C.c_short]
    L.fasp_solver_dbsr_pgmres.argtypes = L.fasp_solver_dbsr_pvgmres.argtypes
    L.fasp_solver_dbsr_pvfgmres.argtypes = L.fasp_solver_dbsr_pvgmres.argtypes
    L.fasp_hip_bsr_precond_setup.argtypes = [P(T.dBSRmat), P(T.AMG_param)]
    L.fasp_hip_bsr_precond_setup.restype = P(T.precond)
    L.fasp_hip_bsr_precond_free.argtypes = [P(T.precond)]
    L.fasp_hip_bsr_precond_free.restype = None
    L.fasp_hip_bsr_precond_fct.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_hip_bsr_precond_fct.restype = None
    L.fasp_dcsrvec_read2.argtypes = [C.c_char_p, C.c_char_p, P(T.dCSRmat), P(T.dvector)]
    L.fasp_dvec_read.argtypes = [C.c_char_p, P(T.dvector)]
    L.fasp_dbsr_read.argtypes = [C.c_char_p, P(T.dBSRmat)]
    L.fasp_hip_free_bsr.argtypes = [P(T.dBSRmat)]
    L.fasp_hip_free_bsr.restype = None
    L.fasp_hip_param_input.argtypes = [C.c_char_p, P(T.ITS_param), P(T.AMG_param)]
    L.fasp_fwrapper_dcsr_krylov_amg_.argtypes = [P(C.c_int), P(C.c_int), T.c_int_p, T.c_int_p, T.c_double_p,
                                                 T.c_double_p, T.c_double_p, P(C.c_double), P(C.c_int), P(C.c_int)]
    L.fasp_fwrapper_dcsr_krylov_amg_.restype = None
    L.fasp_hip_coding_selftest.argtypes = [P(T.dCSRmat), P(C.c_int)]
    L.fasp_hip_amg_kernel_info.argtypes = [C.c_void_p, C.c_int, C.c_int, P(C.c_int), P(C.c_double)]
    L.fasp_hip_coarse_kernel_info.argtypes = [C.c_void_p, P(C.c_int)]
    L.fasp_hip_bsr_coarse_kernel_info.argtypes = [C.c_void_p, P(C.c_int)]
    L.fasp_solver_amg.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.AMG_param)]
    L.fasp_hip_amg_solve.argtypes = [C.c_void_p, P(T.dvector), P(T.dvector), P(T.AMG_param), T.c_double_p,
                                     C.c_int, P(T.fasp_hip_stats)]
    L.fasp_solver_dbsr_krylov_amg.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param),
                                              P(T.AMG_param)]
    L.fasp_hip_bsr_amg_create.argtypes = [P(C.c_void_p), P(T.dBSRmat), P(T.AMG_param)]
    L.fasp_hip_bsr_amg_create_host.argtypes = [P(C.c_void_p), P(T.dBSRmat), P(T.AMG_param)]
    L.fasp_hip_bsr_amg_destroy.argtypes = [C.c_void_p]
    L.fasp_hip_bsr_amg_destroy.restype = None
    L.fasp_hip_bsr_amg_num_levels.argtypes = [C.c_void_p]
    L.fasp_hip_bsr_amg_get_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, P(T.dBSRmat)]
    L.fasp_hip_bsr_amg_get_diaginv.argtypes = [C.c_void_p, C.c_int]
    L.fasp_hip_bsr_amg_get_diaginv.restype = T.c_double_p
    L.fasp_hip_bsr_solve.argtypes = [C.c_void_p, P(T.dvector), P(T.dvector), P(T.ITS_param), T.c_double_p,
                                     C.c_int, P(T.fasp_hip_stats)]
    L.fasp_hip_amg_create.argtypes = [P(C.c_void_p), P(T.dCSRmat), P(T.AMG_param)]
    L.fasp_hip_amg_create_host.argtypes = L.fasp_hip_amg_create.argtypes
    L.fasp_hip_amg_upload.argtypes = [C.c_void_p]
    L.fasp_hip_amg_destroy.argtypes = [C.c_void_p]
    L.fasp_hip_amg_destroy.restype = None
    L.fasp_hip_amg_num_levels.argtypes = [C.c_void_p]
    L.fasp_hip_amg_get_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, P(T.dCSRmat)]
    L.fasp_hip_amg_get_cfmark.argtypes = [C.c_void_p, C.c_int, P(T.ivector)]
    L.fasp_hip_level_smooth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                        T.c_double_p, T.c_double_p]
    L.fasp_hip_solve.argtypes = [C.c_void_p, P(T.dvector), P(T.dvector), P(T.ITS_param),
                                 T.c_double_p, C.c_int, P(T.fasp_hip_stats)]
    L.fasp_hip_set_rhs.argtypes = [C.c_void_p, P(T.dvector)]
    L.fasp_hip_set_guess.argtypes = [C.c_void_p, P(T.dvector)]
    L.fasp_hip_get_solution.argtypes = [C.c_void_p, P(T.dvector)]
    L.fasp_hip_solve_resident.argtypes = [C.c_void_p, P(T.ITS_param), T.c_double_p, C.c_int,
                                          P(T.fasp_hip_stats)]
    L.fasp_hip_precond_amg.argtypes = [C.c_void_p, T.c_double_p, T.c_double_p]
    L.fasp_hip_poisson7pt.argtypes = [C.c_int, C.c_int, C.c_int, P(T.dCSRmat), P(T.dvector),
                                      P(T.dvector)]
    L.fasp_hip_aniso27pt.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, P(T.dCSRmat), P(T.dvector)]
    L.fasp_hip_free_system.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector)]
    L.fasp_hip_free_system.restype = None
    L.fasp_hip_measure_ceilings.argtypes = [P(C.c_double), C.c_size_t, C.c_int]
    L.fasp_hip_amg_publish.argtypes = [C.c_void_p, C.c_char_p]
    L.fasp_hip_amg_attach.argtypes = [P(C.c_void_p), C.c_char_p]
    L.fasp_hip_amg_unpublish.argtypes = [C.c_char_p]
    L.fasp_hip_time_kernel.restype = C.c_double
    L.fasp_hip_time_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.fasp_hip_tune.argtypes = [C.c_char_p, C.c_int]
    L.fasp_hip_comm_unique_id.argtypes = [C.c_char_p]
    L.fasp_hip_comm_init.argtypes = [C.c_int, C.c_int, C.c_char_p]
    L.fasp_hip_version.restype = C.c_char_p
    L.fasp_hip_comm_init_shm.argtypes = [C.c_int, C.c_int, C.c_char_p]
    L.fasp_hip_dist_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.fasp_hip_dist_level_info.argtypes = [C.c_void_p, C.c_int, T.c_int_p]
    L.fasp_hip_dist_get_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, P(T.dCSRmat)]
    L.fasp_hip_dist_get_list.argtypes = [C.c_void_p, C.c_int, C.c_int, P(T.ivector)]
    # the block smoothers (ItrSmootherBSR.c) and the resident handle
    M, V, D, I = P(T.dBSRmat), P(T.dvector), T.c_double_p, T.c_int_p
    for name, args in (
            ("jacobi", [M, V, V]), ("jacobi_setup", [M, D]), ("gs", [M, V, V, C.c_int, I]), ("gs1", [M, V, V, C.c_int, I, D]),
            ("gs_ascend", [M, V, V, D]), ("gs_ascend1", [M, V, V]), ("gs_descend", [M, V, V, D]), ("gs_descend1", [M, V, V]),
            ("gs_order1", [M, V, V, D, I]), ("gs_order2", [M, V, V, I, D]), ("sor", [M, V, V, C.c_int, I, C.c_double]),
            ("sor1", [M, V, V, C.c_int, I, D, C.c_double]), ("sor_ascend", [M, V, V, D, C.c_double]),
            ("sor_descend", [M, V, V, D, C.c_double]), ("sor_order", [M, V, V, D, I, C.c_double])):
        f = getattr(L, "fasp_smoother_dbsr_" + name)
        f.argtypes, f.restype = args, None
    L.fasp_hip_bsr_smoother_create.argtypes = [P(C.c_void_p), M, D, C.c_int, I]
    L.fasp_hip_bsr_smoother_apply.argtypes = [C.c_void_p, C.c_int, C.c_double, V, V]
    L.fasp_hip_bsr_smoother_destroy.argtypes = [C.c_void_p]
    L.fasp_hip_bsr_smoother_destroy.restype = None
    L.fasp_hip_bsr_smoother_info.argtypes = [C.c_void_p, D]
    L.fasp_hip_bsr_sweep_plan.argtypes = [M, C.c_int, I, P(C.c_longlong), I, I, I, I, P(C.c_longlong), I]
    L.fasp_hip_bsr_sweep_time.argtypes = [M, C.c_int, I, C.c_int, C.c_double, C.c_int, C.c_int, D]
    L.fasp_hip_bsr_sweep_time.restype = C.c_double
    _lib = L
    # ILU preconditioner (csrc/ilu_setup.cpp, csrc/ilu.hip.h)
    L.fasp_param_ilu_init.argtypes = [P(T.ILU_param)]
    L.fasp_param_ilu_init.restype = None
    L.fasp_ilu_data_create.argtypes = [C.c_int, C.c_int, P(T.ILU_data)]
    L.fasp_ilu_data_create.restype = None
    L.fasp_ilu_data_free.argtypes = [P(T.ILU_data)]
    L.fasp_ilu_data_free.restype = None
    L.fasp_mem_iludata_check.argtypes = [P(T.ILU_data)]
    L.fasp_mem_iludata_check.restype = C.c_short
    L.fasp_ilu_dcsr_setup.argtypes = [P(T.dCSRmat), P(T.ILU_data), P(T.ILU_param)]
    L.fasp_ilu_dcsr_setup.restype = C.c_short
    for f in ("fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward"):
        getattr(L, f).argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        getattr(L, f).restype = None
    L.fasp_solver_dcsr_krylov_ilu.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    L.fasp_solver_dcsr_krylov_ilu_M.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param),
                                                P(T.ILU_param), P(T.dCSRmat)]
    L.fasp_smoother_dcsr_ilu.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), C.c_void_p]
    L.fasp_smoother_dcsr_ilu.restype = None
    L.fasp_fwrapper_dcsr_krylov_ilu_.argtypes = [P(C.c_int), P(C.c_int), T.c_int_p, T.c_int_p, T.c_double_p,
                                                 T.c_double_p, T.c_double_p, P(C.c_double), P(C.c_int), P(C.c_int)]
    L.fasp_fwrapper_dcsr_krylov_ilu_.restype = None
    L.fasp_hip_ilu_time.argtypes = [P(T.ILU_data), C.c_int, C.c_int, T.c_double_p]
    L.fasp_hip_ilu_time.restype = C.c_double
    L.fasp_hip_ilu_schedule.argtypes = [P(T.ILU_data), C.c_int, C.c_int, T.c_double_p]
    # block ILU (csrc/ilu_setup.cpp, csrc/ilu.hip.h)
    L.fasp_ilu_dbsr_setup.argtypes = [P(T.dBSRmat), P(T.ILU_data), P(T.ILU_param)]
    L.fasp_ilu_dbsr_setup.restype = C.c_short
    L.fasp_precond_dbsr_ilu.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dbsr_ilu.restype = None
    L.fasp_solver_dbsr_krylov_ilu.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    L.fasp_solver_dbsr_krylov_ilu.restype = C.c_int
    L.fasp_smoother_dbsr_ilu.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), C.c_void_p]
    L.fasp_smoother_dbsr_ilu.restype = None
    L.fasp_fwrapper_dbsr_krylov_ilu_.argtypes = [P(C.c_int), P(C.c_int), P(C.c_int), T.c_int_p, T.c_int_p, T.c_double_p,
                                                 T.c_double_p, T.c_double_p, P(C.c_double), P(C.c_int), P(C.c_int)]
    L.fasp_fwrapper_dbsr_krylov_ilu_.restype = None
    # ILU smoothing in the block AMG cycle (AMG_param.ILU_levels > 0): the factors a block hierarchy owns
    L.fasp_hip_bsr_amg_get_ilu.argtypes = [C.c_void_p, C.c_int, P(T.ILU_data)]
    L.fasp_hip_bsr_amg_ilu_info.argtypes = [C.c_void_p, C.c_int, T.c_double_p]
    L.fasp_hip_bsr_amg_ilu_smooth_time.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.fasp_hip_bsr_amg_ilu_smooth_time.restype = C.c_double
    # Galerkin product on the device (csrc/rap.hip.h)
    L.fasp_blas_dcsr_rap.argtypes = [P(T.dCSRmat), P(T.dCSRmat), P(T.dCSRmat), P(T.dCSRmat)]
    L.fasp_blas_dcsr_rap.restype = None
    L.fasp_hip_dcsr_rap.argtypes = L.fasp_blas_dcsr_rap.argtypes
    L.fasp_hip_rap_info.argtypes = [P(C.c_int)]
    L.fasp_hip_rap_device_count.argtypes = []
    L.fasp_hip_rap_device_count.restype = C.c_long
    L.fasp_hip_rap_time.argtypes = [P(T.dCSRmat), P(T.dCSRmat), P(T.dCSRmat), C.c_int, C.c_int]
    L.fasp_hip_rap_time.restype = C.c_double
    L.fasp_dcsr_free.argtypes = [P(T.dCSRmat)]
    L.fasp_dcsr_free.restype = None
    # structured (STR) matrices
    L.fasp_dstr_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, T.c_int_p]
    L.fasp_dstr_create.restype = T.dSTRmat
    L.fasp_dstr_alloc.argtypes = [C.c_int] * 7 + [T.c_int_p, P(T.dSTRmat)]
    L.fasp_dstr_alloc.restype = None
    L.fasp_dstr_free.argtypes = [P(T.dSTRmat)]
    L.fasp_dstr_free.restype = None
    L.fasp_dstr_cp.argtypes = [P(T.dSTRmat), P(T.dSTRmat)]
    L.fasp_dstr_cp.restype = None
    L.fasp_format_dstr_dcsr.argtypes = [P(T.dSTRmat), P(T.dCSRmat)]
    L.fasp_format_dstr_dcsr.restype = C.c_short
    L.fasp_dstr_read.argtypes = [C.c_char_p, P(T.dSTRmat)]
    L.fasp_hip_str_form.argtypes = [P(T.dSTRmat)]
    L.fasp_hip_time_str_mxv.argtypes = [P(T.dSTRmat), C.c_int]
    L.fasp_hip_time_str_mxv.restype = C.c_double
    L.fasp_blas_dstr_aAxpy.argtypes = [C.c_double, P(T.dSTRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dstr_aAxpy.restype = None
    L.fasp_blas_dstr_mxv.argtypes = [P(T.dSTRmat), T.c_double_p, T.c_double_p]
    L.fasp_blas_dstr_mxv.restype = None
    L.fasp_precond_dstr_diag.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dstr_diag.restype = None
    L.fasp_solver_dstr_pcg.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                       C.c_double, C.c_int, C.c_short, C.c_short]
    L.fasp_solver_dstr_pbcgs.argtypes = L.fasp_solver_dstr_pcg.argtypes
    L.fasp_solver_dstr_pminres.argtypes = L.fasp_solver_dstr_pcg.argtypes
    L.fasp_solver_dstr_pgmres.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double,
                                          C.c_double, C.c_int, C.c_short, C.c_short, C.c_short]
    L.fasp_solver_dstr_pvgmres.argtypes = L.fasp_solver_dstr_pgmres.argtypes
    L.fasp_solver_dstr_itsolver.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.precond), P(T.ITS_param)]
    L.fasp_solver_dstr_krylov.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param)]
    L.fasp_solver_dstr_krylov_diag.argtypes = L.fasp_solver_dstr_krylov.argtypes
    L.fasp_hip_mxv_str.argtypes = [C.c_void_p, T.c_double_p, T.c_double_p]
    L.fasp_hip_mxv_str.restype = None
    # structured ILU(0) / ILU(1)
    L.fasp_ilu_dstr_setup0.argtypes = [P(T.dSTRmat), P(T.dSTRmat)]
    L.fasp_ilu_dstr_setup0.restype = None
    L.fasp_ilu_dstr_setup1.argtypes = [P(T.dSTRmat), P(T.dSTRmat)]
    L.fasp_ilu_dstr_setup1.restype = None
    L.fasp_precond_dstr_ilu0.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dstr_ilu0.restype = None
    L.fasp_precond_dstr_ilu1.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dstr_ilu1.restype = None
    L.fasp_solver_dstr_krylov_ilu.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    L.fasp_hip_str_ilu_form.argtypes = [P(T.dSTRmat), C.c_int]
    L.fasp_hip_str_ilu_apply.argtypes = [P(T.dSTRmat), C.c_int, T.c_double_p, T.c_double_p]
    L.fasp_hip_time_str_ilu.argtypes = [P(T.dSTRmat), C.c_int, C.c_int]
    L.fasp_hip_time_str_ilu.restype = C.c_double
    # the structured smoothers (ItrSmootherSTR.c)
    A_, V_, D_, I_ = P(T.dSTRmat), P(T.dvector), T.c_double_p, T.c_int_p
    for name, args in (("jacobi", []), ("jacobi1", [D_]), ("gs", [C.c_int, I_]), ("gs1", [C.c_int, I_, D_]), ("gs_ascend", [D_]),
                       ("gs_descend", [D_]), ("gs_order", [D_, I_]), ("gs_cf", [D_, I_, C.c_int]), ("sor", [C.c_int, I_, C.c_double]),
                       ("sor1", [C.c_int, I_, D_, C.c_double]), ("sor_ascend", [D_, C.c_double]), ("sor_descend", [D_, C.c_double]),
                       ("sor_order", [D_, I_, C.c_double]), ("sor_cf", [D_, I_, C.c_int, C.c_double])):
        f = getattr(L, "fasp_smoother_dstr_" + name)
        f.argtypes = [A_, V_, V_] + args
        f.restype = None
    L.fasp_hip_str_sweep.argtypes = [A_, C.c_int, C.c_int, I_, C.c_double, D_, D_, D_, C.c_int, I_]
    L.fasp_hip_str_sweep_form.argtypes = [A_, C.c_int, I_]
    L.fasp_hip_str_sweep_levels.argtypes = [A_, C.c_int, I_, I_, I_, C.c_int]
    L.fasp_hip_time_str_sweep.argtypes = [A_, C.c_int, C.c_int, I_, C.c_double, C.c_int]
    L.fasp_hip_time_str_sweep.restype = C.c_double
    # the structured block Gauss-Seidel (Schwarz) smoother and preconditioner (ItrSmootherSTR.c:1543 / :1665, PreSTR.c:1715, SolSTR.c:323)
    IV_ = P(T.ivector)
    L.fasp_generate_diaginv_block.argtypes = [A_, IV_, V_, IV_]
    L.fasp_generate_diaginv_block.restype = None
    L.fasp_smoother_dstr_swz.argtypes = [A_, V_, V_, V_, IV_, IV_, IV_]
    L.fasp_smoother_dstr_swz.restype = None
    L.fasp_precond_dstr_blockgs.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dstr_blockgs.restype = None
    L.fasp_solver_dstr_krylov_blockgs.argtypes = [A_, V_, V_, P(T.ITS_param), IV_, IV_]
    L.fasp_hip_str_swz.argtypes = [A_, I_, C.c_int, I_, D_, D_, C.c_int, I_]
    L.fasp_hip_str_swz_levels.argtypes = [A_, I_, C.c_int, I_, I_, I_, C.c_int]
    L.fasp_hip_time_str_swz.argtypes = [A_, I_, C.c_int, I_, C.c_int, D_, D_, I_]
    # the CSR overlapping Schwarz method (BlaSchwarzSetup.c, PreCSR.c:371, PreDataInit.c:494, AuxParam.c:617, SolCSR.c:401)
    SD_, SP_, M_ = P(T.SWZ_data), P(T.SWZ_param), P(T.dCSRmat)
    L.fasp_param_swz_init.argtypes = [SP_]
    L.fasp_param_swz_init.restype = None
    L.fasp_dcsr_sympart.argtypes = [M_]
    L.fasp_dcsr_sympart.restype = T.dCSRmat
    L.fasp_dcsr_shift.argtypes = [M_, C.c_int]
    L.fasp_dcsr_shift.restype = None
    L.fasp_sparse_mis.argtypes = [M_]
    L.fasp_sparse_mis.restype = T.ivector
    L.fasp_swz_dcsr_setup.argtypes = [SD_, SP_]
    L.fasp_dcsr_swz_forward.argtypes = [SD_, SP_, V_, V_]
    L.fasp_dcsr_swz_forward.restype = None
    L.fasp_dcsr_swz_backward.argtypes = [SD_, SP_, V_, V_]
    L.fasp_dcsr_swz_backward.restype = None
    L.fasp_precond_swz.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_swz.restype = None
    L.fasp_swz_data_free.argtypes = [SD_]
    L.fasp_swz_data_free.restype = None
    L.fasp_solver_dcsr_krylov_swz.argtypes = [M_, V_, V_, P(T.ITS_param), SP_]
    L.fasp_hip_csr_swz_levels.argtypes = [SD_, C.c_int, I_, C.c_int]
    L.fasp_hip_csr_swz.argtypes = [SD_, C.c_int, D_, D_, C.c_int, I_, D_, I_]
    L.fasp_hip_csr_swz_resident_count.argtypes = []
    L.fasp_hip_time_csr_swz.argtypes = [SD_, C.c_int, D_, D_, I_]
    L.fasp_hip_csr_swz_runs.argtypes = [SD_, C.c_int, C.c_int, I_, C.c_int]
    L.fasp_hip_amg_get_swz.argtypes = [C.c_void_p, C.c_int, SD_]
    L.fasp_hip_amg_swz_info.argtypes = [C.c_void_p, C.c_int, I_]
    L.fasp_hip_amg_swz_levels.argtypes = [C.c_void_p, C.c_int, P(C.c_int)]
    L.fasp_hip_amg_swz_sweep_time.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.fasp_hip_amg_swz_sweep_time.restype = C.c_double
    for fmt, mat in (("csr", T.dCSRmat), ("bsr", T.dBSRmat), ("str", T.dSTRmat)):   # the safe-net solvers: no abstol (KrySP*.c)
        for m in SAFE_FORMATS[fmt]:
            rs = [C.c_short] if m.endswith("gmres") else []
            getattr(L, f"fasp_solver_d{fmt}_{m}").argtypes = [P(mat), V_, V_, P(T.precond), C.c_double, C.c_int] + rs + [C.c_short, C.c_short]
    L.fasp_solver_dcsr_itsolver_s.argtypes = [M_, V_, V_, P(T.precond), P(T.ITS_param)]
    L.fasp_solver_dcsr_krylov_s.argtypes = [M_, V_, V_, P(T.ITS_param)]
    L.fasp_hip_safe_update_selftest.argtypes = [C.c_int, C.c_int, C.c_int, D_]
    L.fasp_hip_plugin_solve_seconds.argtypes = []
    L.fasp_hip_plugin_solve_seconds.restype = C.c_double
    L.fasp_hip_blas1_op.argtypes = [C.c_int, C.c_int, C.c_int, I_, D_, P(D_), P(D_), D_, C.c_int, I_, D_, D_, I_, D_]
    return L


def solve_bsr_ilu(ia, ja, val, nb, b, x0=None, solver=None, tol=1e-8, maxit=500, lfil=0, print_level=0):
    """fasp_solver_dbsr_krylov_ilu on numpy arrays (BSR, row-major nb x nb blocks): block ILUk(lfil) set up on the host,
    the Krylov method (default BiCGstab) and both block triangular solves on the device.  Returns (status, x)."""
    L = lib()
    ia = np.ascontiguousarray(ia, dtype=np.int32); ja = np.ascontiguousarray(ja, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros(len(b)) if x0 is None else np.array(x0, dtype=np.float64)
    A = T.dBSRmat()
    A.ROW = A.COL = len(ia) - 1; A.NNZ = len(ja); A.nb = nb; A.storage_manner = 0
    A.IA = ia.ctypes.data_as(T.c_int_p); A.JA = ja.ctypes.data_as(T.c_int_p); A.val = val.ctypes.data_as(T.c_double_p)
    bv = T.dvector(len(b), b.ctypes.data_as(T.c_double_p)); xv = T.dvector(len(x), x.ctypes.data_as(T.c_double_p))
    it = T.ITS_param(); L.fasp_param_solver_init(C.byref(it))
    it.itsolver_type = T.SOLVER_BiCGstab if solver is None else solver
    it.tol, it.maxit, it.print_level = tol, maxit, print_level
    prm = T.ILU_param(); L.fasp_param_ilu_init(C.byref(prm))
    prm.ILU_lfil, prm.print_level = lfil, print_level
    st = L.fasp_solver_dbsr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm))
    return st, x


def available():
    """True when a HIP device is usable by the library."""
    return bool(lib().fasp_hip_available())


# --- parameter constructors (AuxParam.c:431 / :572) ------------------------------
def param_amg_init():
    p = T.AMG_param()
    lib().fasp_param_amg_init(C.byref(p))
    return p


def param_solver_init():
    p = T.ITS_param()
    lib().fasp_param_solver_init(C.byref(p))
    return p


def poisson7pt(nx, ny=None, nz=None):
    """P7 synthetic system (test/src/FdmPoisson.c:439 + :731) -> (ia, ja, a, f, u_exact)."""
    ny = nx if ny is None else ny
    nz = nx if nz is None else nz
    A = T.dCSRmat(); b = T.dvector(); u = T.dvector()
    st = lib().fasp_hip_poisson7pt(nx, ny, nz, C.byref(A), C.byref(b), C.byref(u))
    if st < 0:
        raise RuntimeError(f"fasp_hip_poisson7pt failed: {st}")
    ia, ja, a = T.csr_arrays(A)
    f = np.ctypeslib.as_array(b.val, (b.row,)).copy()
    ue = np.ctypeslib.as_array(u.val, (u.row,)).copy()
    lib().fasp_hip_free_system(C.byref(A), C.byref(b), C.byref(u))
    return ia, ja, a, f, ue


def poisson7pt_var(n, p7=None):
    """Variable-coefficient twin of P7(n): -div(kappa grad u) = f on the same grid and sparsity pattern,
    kappa = 1 + 0.8 sin(2 pi x) sin(2 pi y) sin(2 pi z) (contrast 9), face coefficients = mean of the two
    node values, Dirichlet boundary.  No two rows repeat, so no lossless matrix coding applies: the
    plain-CSR kernels serve every level.  Entry order = P7's (diagonal first).  -> (ia, ja, a, f)"""
    ia, ja, a, f, _ue = p7 if p7 is not None else poisson7pt(n)
    m = len(f)
    h = 1.0 / (n + 1)
    idx = np.arange(m, dtype=np.int64)
    xi = (idx % n + 1) * h
    yi = ((idx // n) % n + 1) * h
    zi = (idx // (n * n) + 1) * h
    kap = 1.0 + 0.8 * np.sin(2 * np.pi * xi) * np.sin(2 * np.pi * yi) * np.sin(2 * np.pi * zi)
    del xi, yi, zi
    cnt = np.diff(ia)
    rows = np.repeat(idx, cnt)
    off = ja != rows
    a2 = np.where(off, a * 0.5 * (kap[rows] + kap[ja]), 0.0)          # -kappa_face / h^2
    rowsum = np.bincount(rows, weights=a2, minlength=m)                # sum of the off-diagonals (negative)
    diag = -rowsum + (7 - cnt) * kap / (h * h)                         # + the faces that touch the boundary
    a2[ia[:-1]] = diag                                                 # P7 stores the diagonal first
    return ia, ja, a2, f.copy()


def aniso27pt(n, kx=1.0, ky=1.0, kz=0.01):
    """Config-5 synthetic system: Q1 FE, -div(diag(kx,ky,kz) grad u) = 1 -> (ia, ja, a, f)."""
    A = T.dCSRmat(); b = T.dvector()
    st = lib().fasp_hip_aniso27pt(n, kx, ky, kz, C.byref(A), C.byref(b))
    if st < 0:
        raise RuntimeError(f"fasp_hip_aniso27pt failed: {st}")
    ia, ja, a = T.csr_arrays(A)
    f = np.ctypeslib.as_array(b.val, (b.row,)).copy()
    lib().fasp_hip_free_system(C.byref(A), C.byref(b), None)
    return ia, ja, a, f


# --- Galerkin product on the device (csrc/rap.hip.h) --------------------------------
def _rap_operands(R, A, P):
    """R, A, P as (ia, ja, val, ncol) tuples -> the three dCSRmat structs + what keeps their arrays alive"""
    mats, keep = [], []
    for ia, ja, val, ncol in (R, A, P):
        M, k = T.as_csr(ia, ja, val, ncol=ncol)
        mats.append(M); keep.append(k)
    return mats, keep


def rap(R, A, P):
    """fasp_blas_dcsr_rap (BlaSpmvCSR.c:999) on the device: R, A, P = (ia, ja, val, ncol) -> (ia, ja, val) of R A P, the
    reference's bytes.  Raises on a status < 0 (fasp_hip_dcsr_rap)."""
    (r, a, p), _keep = _rap_operands(R, A, P)
    out = T.dCSRmat()
    st = lib().fasp_hip_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), C.byref(out))
    if st < 0:
        raise RuntimeError(f"fasp_hip_dcsr_rap failed with status {st}")
    res = T.csr_arrays(out)
    lib().fasp_dcsr_free(C.byref(out))
    return res


def rap_info():
    """The last device product: dict(form, batches, lds, rows) (fasp_hip_rap_info)."""
    info = (C.c_int * 4)()
    lib().fasp_hip_rap_info(info)
    return dict(zip(("form", "batches", "lds", "rows"), list(info)))


def rap_time(R, A, P, where, reps=3):
    """Seconds per product (fasp_hip_rap_time): where = 0 host, 1 device end to end, 2 device kernels alone."""
    (r, a, p), _keep = _rap_operands(R, A, P)
    return lib().fasp_hip_rap_time(C.byref(r), C.byref(a), C.byref(p), where, reps)


def solver_dcsr_krylov_amg(ia, ja, a, b, x, itparam, amgparam):
    """fasp_solver_dcsr_krylov_amg (SolCSR.c:476).  x is updated in place (numpy f64).
    Returns the iteration count or a negative ERROR_* code."""
    A, _keep = T.as_csr(ia, ja, a)
    bv, _b = T.as_vec(b)
    assert x.dtype == np.float64 and x.flags["C_CONTIGUOUS"]
    xv = T.dvector(x.shape[0], x.ctypes.data_as(T.c_double_p))
    return lib().fasp_solver_dcsr_krylov_amg(C.byref(A), C.byref(bv), C.byref(xv),
                                             C.byref(itparam), C.byref(amgparam))


class AMG:
    """Resident hierarchy (fasp_hip_amg).  host_only=True skips the GPU upload."""

    def __init__(self, ia, ja, a, amgparam, host_only=False):
        self._A, self._keep = T.as_csr(ia, ja, a)
        self.h = C.c_void_p()
        fn = lib().fasp_hip_amg_create_host if host_only else lib().fasp_hip_amg_create
        self.status = fn(C.byref(self.h), C.byref(self._A), C.byref(amgparam))
        if self.status < 0:
            self.h = C.c_void_p()
            raise RuntimeError(f"fasp_hip_amg_create failed with status {self.status}")
        self.n = self._A.row

    @classmethod
    def attach(cls, name):
        """Host-only handle on a hierarchy another process of this node published (fasp_hip_amg_attach)."""
        self = cls.__new__(cls)
        self._A = None; self._keep = None
        self.h = C.c_void_p()
        self.status = lib().fasp_hip_amg_attach(C.byref(self.h), name.encode())
        if self.status < 0:
            self.h = C.c_void_p()
            raise RuntimeError(f"fasp_hip_amg_attach({name}) failed with status {self.status}")
        v = T.dCSRmat()
        lib().fasp_hip_amg_get_matrix(self.h, 0, 0, C.byref(v))
        self.n = v.row
        return self

    def publish(self, name):
        st = lib().fasp_hip_amg_publish(self.h, name.encode())
        if st < 0:
            raise RuntimeError(f"fasp_hip_amg_publish({name}) failed with status {st}")

    @staticmethod
    def unpublish(name):
        lib().fasp_hip_amg_unpublish(name.encode())

    @property
    def num_levels(self):
        return lib().fasp_hip_amg_num_levels(self.h)

    def upload(self):
        st = lib().fasp_hip_amg_upload(self.h)
        if st < 0:
            raise RuntimeError(f"fasp_hip_amg_upload failed with status {st}")

    def matrix(self, level, which):
        """which: 0 A, 1 P, 2 R -> (nrow, ncol, ia, ja, val) copies."""
        v = T.dCSRmat()
        st = lib().fasp_hip_amg_get_matrix(self.h, level, which, C.byref(v))
        if st < 0:
            raise IndexError((level, which))
        ia, ja, val = T.csr_arrays(v)
        return v.row, v.col, ia, ja, val

    def cfmark(self, level):
        v = T.ivector()
        if lib().fasp_hip_amg_get_cfmark(self.h, level, C.byref(v)) < 0:
            raise IndexError(level)
        return np.ctypeslib.as_array(v.val, (v.row,)).copy()

    def solve(self, b, itparam, x0=None, hist_cap=600):
        """PCG on the resident hierarchy -> (status, x, hist, stats)."""
        x = np.zeros(self.n) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        bv, _b = T.as_vec(b)
        xv, x = T.as_vec(x)
        hist = np.zeros(hist_cap)
        stats = T.fasp_hip_stats()
        st = lib().fasp_hip_solve(self.h, C.byref(bv), C.byref(xv), C.byref(itparam),
                                  T.dp(hist), hist_cap, C.byref(stats))
        return st, x, hist[:max(stats.nhist, 0)].copy(), stats

    def amg_solve(self, b, amgparam=None, x0=None, hist_cap=600):
        """Multigrid cycles as a stand-alone solver (fasp_amg_solve) -> (status, x, hist, stats)."""
        x = np.zeros(self.n) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        bv, _b = T.as_vec(b)
        xv, x = T.as_vec(x)
        hist = np.zeros(hist_cap)
        stats = T.fasp_hip_stats()
        st = lib().fasp_hip_amg_solve(self.h, C.byref(bv), C.byref(xv),
                                      C.byref(amgparam) if amgparam is not None else None,
                                      T.dp(hist), hist_cap, C.byref(stats))
        return st, x, hist[:max(min(stats.nhist, hist_cap), 0)].copy(), stats

    def set_rhs(self, b):
        bv, _b = T.as_vec(b)
        st = lib().fasp_hip_set_rhs(self.h, C.byref(bv))
        if st < 0:
            raise RuntimeError(f"fasp_hip_set_rhs failed: {st}")

    def solve_resident(self, itparam, hist_cap=600):
        """Zero initial guess, b and x stay in HBM -> (status, hist, stats)."""
        st = lib().fasp_hip_set_guess(self.h, None)
        if st < 0:
            raise RuntimeError(f"fasp_hip_set_guess failed: {st}")
        hist = np.zeros(hist_cap)
        stats = T.fasp_hip_stats()
        st = lib().fasp_hip_solve_resident(self.h, C.byref(itparam), T.dp(hist), hist_cap,
                                           C.byref(stats))
        return st, hist[:max(stats.nhist, 0)].copy(), stats

    def get_solution(self):
        x = np.zeros(self.n)
        xv, x = T.as_vec(x)
        st = lib().fasp_hip_get_solution(self.h, C.byref(xv))
        if st < 0:
            raise RuntimeError(f"fasp_hip_get_solution failed: {st}")
        return x

    def kernel_info(self, level, which=0):
        """(kernel family, matrix bytes read per pass) of operator which (0 A, 1 P, 2 R) on a level."""
        k = C.c_int(0); b = C.c_double(0)
        if lib().fasp_hip_amg_kernel_info(self.h, level, which, C.byref(k), C.byref(b)) < 0:
            raise IndexError((level, which))
        return k.value, b.value

    def coarse_kernel_info(self):
        """The last coarsest-level solve: (family, instantiation, auxiliary, CG status, net ran, net status, compute units of the
        device, 0) -- fasp_hip_dev.h."""
        info = (C.c_int * 8)()
        if lib().fasp_hip_coarse_kernel_info(self.h, info) < 0:
            raise RuntimeError("fasp_hip_coarse_kernel_info failed")
        return tuple(info)

    def precond(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        st = lib().fasp_hip_precond_amg(self.h, T.dp(r), T.dp(z))
        if st < 0:
            raise RuntimeError(f"fasp_hip_precond_amg failed: {st}")
        return z

    def level_smooth(self, level, post, smoother, order, nsweeps, relax, ndeg, b, x=None):
        """One smoothing step of a resident level as a cycle takes it (fasp_hip_level_smooth) -> (status, iterate).
        x None: the step starts from the level's lazily zero iterate, and the buffer handed over is all NaN."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        zero = x is None
        x = np.full(len(b), np.nan) if zero else np.ascontiguousarray(x, dtype=np.float64).copy()
        st = lib().fasp_hip_level_smooth(self.h, level, int(post), smoother, order, nsweeps, relax, ndeg, int(zero), T.dp(b), T.dp(x))
        return st, x

    # --- row partition (host side) ---
    def dist_plan(self, rank, nranks, min_rows):
        st = lib().fasp_hip_dist_plan(self.h, rank, nranks, min_rows)
        if st < 0:
            raise RuntimeError(f"fasp_hip_dist_plan failed: {st}")

    def dist_info(self, level):
        info = (C.c_int * 8)()
        if lib().fasp_hip_dist_level_info(self.h, level, info) < 0:
            raise IndexError(level)
        keys = ("replicated", "nglobal", "row0", "nloc", "nghost", "nsend", "first_replicated", "nranks")
        return dict(zip(keys, list(info)))

    def dist_matrix(self, level, which):
        v = T.dCSRmat()
        if lib().fasp_hip_dist_get_matrix(self.h, level, which, C.byref(v)) < 0:
            raise IndexError((level, which))
        ia, ja, val = T.csr_arrays(v)
        return v.row, v.col, ia, ja, val

    def dist_list(self, level, which):
        v = T.ivector()
        if lib().fasp_hip_dist_get_list(self.h, level, which, C.byref(v)) < 0:
            raise IndexError((level, which))
        if v.row == 0:
            return np.zeros(0, np.int32)
        return np.ctypeslib.as_array(v.val, (v.row,)).copy()

    def time_kernel(self, kind, level=0, reps=20):
        return lib().fasp_hip_time_kernel(self.h, kind, level, reps)

    # --- Schwarz levels (SWZ_levels > 0) ---
    def swz(self, level):
        """The blocks level `level` is smoothed with, as copies: dict(nblk, maxbs, SWZ_type, iblock, jblock, A=(ia, ja, val) 1-based), or
        None when the level is no Schwarz level."""
        d = T.SWZ_data()
        st = lib().fasp_hip_amg_get_swz(self.h, level, C.byref(d))
        if st < 0:
            raise IndexError(level)
        if st == 0:
            return None
        iblock = np.ctypeslib.as_array(d.iblock, (d.nblk + 1,)).copy()
        jblock = np.ctypeslib.as_array(d.jblock, (int(iblock[-1]),)).copy()
        n, nnz = d.A.row, d.A.nnz
        ia = np.ctypeslib.as_array(d.A.IA, (n + 1,)).copy()
        ja = np.ctypeslib.as_array(d.A.JA, (max(nnz, 1),))[:nnz].copy()
        val = np.ctypeslib.as_array(d.A.val, (max(nnz, 1),))[:nnz].copy()
        return dict(nblk=d.nblk, maxbs=d.maxbs, SWZ_type=d.SWZ_type, iblock=iblock, jblock=jblock, A=(ia, ja, val))

    def swz_levels(self, level):
        """mgl[level].SWZ_levels as the reference's setup leaves it (host only)."""
        v = C.c_int(0)
        if lib().fasp_hip_amg_swz_levels(self.h, level, C.byref(v)) < 0:
            raise IndexError(level)
        return v.value

    def swz_info(self, level):
        """dict(levels_fwd, levels_bwd, launches_fwd, launches_bwd, nblk, maxbs, nswap, nfactor) of a Schwarz level of an uploaded
        hierarchy (the launches: of a sweep in the form the cycles take now), or None."""
        info = (C.c_int * 8)()
        st = lib().fasp_hip_amg_swz_info(self.h, level, info)
        if st < 0:
            raise IndexError(level)
        if st == 0:
            return None
        keys = ("levels_fwd", "levels_bwd", "launches_fwd", "launches_bwd", "nblk", "maxbs", "nswap", "nfactor")
        return dict(zip(keys, list(info)))

    def swz_sweep_time(self, level, dir=0, reps=20):
        """HIP-event milliseconds of one Schwarz sweep of a level (dir 0 forward, 1 backward) in the form the cycles take now."""
        ms = lib().fasp_hip_amg_swz_sweep_time(self.h, level, dir, reps)
        if ms < 0:
            raise RuntimeError(f"fasp_hip_amg_swz_sweep_time failed: {int(ms)}")
        return ms

    def close(self):
        if self.h:
            lib().fasp_hip_amg_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BSRAMG:
    """Resident block hierarchy (fasp_hip_amg_bsr, config 3).  host_only=True skips the GPU upload."""

    def __init__(self, ia, ja, val, nb, amgparam, host_only=False):
        self._A, self._keep = T.as_bsr(ia, ja, val, nb)
        self.h = C.c_void_p()
        fn = lib().fasp_hip_bsr_amg_create_host if host_only else lib().fasp_hip_bsr_amg_create
        self.status = fn(C.byref(self.h), C.byref(self._A), C.byref(amgparam))
        if self.status < 0:
            self.h = C.c_void_p()
            raise RuntimeError(f"fasp_hip_bsr_amg_create failed with status {self.status}")
        self.nb = nb
        self.n = self._A.ROW * nb

    @property
    def num_levels(self):
        return lib().fasp_hip_bsr_amg_num_levels(self.h)

    def matrix(self, level, which):
        """which: 0 A, 1 P, 2 R -> (ROW, COL, NNZ, ia, ja, val) copies."""
        v = T.dBSRmat()
        if lib().fasp_hip_bsr_amg_get_matrix(self.h, level, which, C.byref(v)) < 0:
            raise IndexError((level, which))
        ia = np.ctypeslib.as_array(v.IA, (v.ROW + 1,)).copy()
        ja = np.ctypeslib.as_array(v.JA, (max(v.NNZ, 1),))[:v.NNZ].copy()
        nv = v.NNZ * v.nb * v.nb
        val = np.ctypeslib.as_array(v.val, (max(nv, 1),))[:nv].copy()
        return v.ROW, v.COL, v.NNZ, ia, ja, val

    def diaginv(self, level):
        p = lib().fasp_hip_bsr_amg_get_diaginv(self.h, level)
        if not p:
            return None
        v = T.dBSRmat()
        lib().fasp_hip_bsr_amg_get_matrix(self.h, level, 0, C.byref(v))
        return np.ctypeslib.as_array(p, (v.ROW * v.nb * v.nb,)).copy()

    def ilu(self, level):
        """The host ILU factor of a level below AMG_param.ILU_levels (fasp_hip_bsr_amg_get_ilu) -> dict(nb, row, nzlu, ijlu,
        luval) of copies, or None when the level has none."""
        d = T.ILU_data()
        st = lib().fasp_hip_bsr_amg_get_ilu(self.h, level, C.byref(d))
        if st < 0:
            raise IndexError(level)
        if st == 0:
            return None
        return {"nb": d.nb, "row": d.row, "nzlu": d.nzlu,
                "ijlu": np.ctypeslib.as_array(d.ijlu, (d.nzlu,)).copy(),
                "luval": np.ctypeslib.as_array(d.luval, (d.nzlu * d.nb * d.nb,)).copy()}

    def ilu_info(self, level):
        """Schedule of the level's device factor (fasp_hip_bsr_amg_ilu_info): (levels of L, of U, form of the L solve, of the
        U solve -- 1 single launch, 0 level launches --, chunks of L, of U), or None when the level has no device factor."""
        info = np.zeros(6)
        st = lib().fasp_hip_bsr_amg_ilu_info(self.h, level, T.dp(info))
        if st < 0:
            raise IndexError(level)
        return tuple(int(v) for v in info) if st else None

    def ilu_smooth_time(self, level=0, reps=20):
        """Microseconds per ILU smoothing step of the cycle on `level` (fasp_hip_bsr_amg_ilu_smooth_time)."""
        return lib().fasp_hip_bsr_amg_ilu_smooth_time(self.h, level, reps)

    def solve(self, b, itparam, x0=None, hist_cap=1200):
        """Krylov solve on the resident block hierarchy -> (status, x, hist, stats)."""
        x = np.zeros(self.n) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        bv, _b = T.as_vec(b)
        xv, x = T.as_vec(x)
        hist = np.zeros(hist_cap)
        stats = T.fasp_hip_stats()
        st = lib().fasp_hip_bsr_solve(self.h, C.byref(bv), C.byref(xv), C.byref(itparam), T.dp(hist),
                                      hist_cap, C.byref(stats))
        return st, x, hist[:max(min(stats.nhist, hist_cap), 0)].copy(), stats

    def precond(self, r):
        """z = B r: maxit cycles of the resident block hierarchy from a zero guess (fasp_hip_bsr_precond_fct)."""
        r = np.ascontiguousarray(r, dtype=np.float64).copy()
        z = np.zeros_like(r)
        lib().fasp_hip_bsr_precond_fct(T.dp(r), T.dp(z), self.h)
        return z

    def coarse_kernel_info(self):
        """The last coarsest-level solve: (family, LV, cache2, GMRES status, iterations, 0, compute units, 0) -- fasp_hip_dev.h."""
        info = (C.c_int * 8)()
        if lib().fasp_hip_bsr_coarse_kernel_info(self.h, info) < 0:
            raise RuntimeError("fasp_hip_bsr_coarse_kernel_info failed")
        return tuple(info)

    def dist_info(self):
        """Row partition of level 0 (one process per GPU): owned block rows [row0, row0 + nloc)."""
        info = (C.c_int * 6)()
        lib().fasp_hip_bsr_dist_info(self.h, info)
        return {"replicated": info[0], "row0": info[1], "nloc": info[2], "nghost": info[3], "first_replicated": info[4], "nb": info[5]}

    def free(self):
        if self.h:
            lib().fasp_hip_bsr_amg_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


BSR_SWEEP_GS, BSR_SWEEP_SOR, BSR_SWEEP_IDENTITY = 0, 1, 2   # `kind` of fasp_hip_bsr_smoother_apply


def _mark_p(mark):
    if mark is None:
        return None, None
    m = np.ascontiguousarray(mark, dtype=np.int32)
    return m.ctypes.data_as(T.c_int_p), m


def bsr_sweep_plan(ia, ja, nb, order=T.ASCEND, mark=None):
    """fasp_hip_bsr_sweep_plan (host only): the slab plan of a block sweep as a dict, or None when nothing is swept.
    Raises ValueError(status) for a refused matrix or mark."""
    ia = np.ascontiguousarray(ia, dtype=np.int32); ja = np.ascontiguousarray(ja, dtype=np.int32)
    n = len(ia) - 1
    A = T.dBSRmat(n, n, int(ia[-1]), nb, 0, None, ia.ctypes.data_as(T.c_int_p), ja.ctypes.data_as(T.c_int_p))
    mp, _m = _mark_p(mark)
    info = (C.c_longlong * 6)()
    st = lib().fasp_hip_bsr_sweep_plan(C.byref(A), order, mp, info, None, None, None, None, None, None)
    if st < 0:
        raise ValueError(st)
    if st == 1:
        return None
    nlev, nchunk, nent = int(info[0]), int(info[1]), int(info[2])
    level = np.zeros(max(n, 1), dtype=np.int32); lvl_chunk = np.zeros(nlev + 1, dtype=np.int32)
    rows = np.zeros(max(64 * nchunk, 1), dtype=np.int32); ln = np.zeros(max(64 * nchunk, 1), dtype=np.int32)
    cbase = np.zeros(max(nchunk, 1), dtype=np.int64); cols = np.zeros(max(nent, 1), dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(T.c_int_p)
    st = lib().fasp_hip_bsr_sweep_plan(C.byref(A), order, mp, info, ip(level), ip(lvl_chunk), ip(rows), ip(ln),
                                       cbase.ctypes.data_as(C.POINTER(C.c_longlong)), ip(cols))
    assert st == 0, st
    return dict(levels=nlev, chunks=nchunk, nent=nent, nreal=int(info[3]), maxlen=int(info[4]), level=level[:n], lvl_chunk=lvl_chunk,
                rows=rows[:64 * nchunk], len=ln[:64 * nchunk], cbase=cbase[:nchunk], cols=cols[:nent])


class BSRSmoother:
    """Resident block smoother (fasp_hip_bsr_smoother): the sweep plan of (A, order, mark) uploaded once, one sweep per apply().
    diaginv=None: the inverse diagonal blocks are computed as fasp_smoother_dbsr_gs computes them."""

    def __init__(self, ia, ja, val, nb, order=T.ASCEND, mark=None, diaginv=None):
        A, _keep = T.as_bsr(ia, ja, val, nb)
        mp, _m = _mark_p(mark)
        d = None if diaginv is None else np.ascontiguousarray(diaginv, dtype=np.float64)
        self.h = C.c_void_p()
        self.status = lib().fasp_hip_bsr_smoother_create(C.byref(self.h), C.byref(A), None if d is None else T.dp(d), order, mp)
        if self.status < 0:
            self.h = C.c_void_p()
            raise RuntimeError(f"fasp_hip_bsr_smoother_create failed with status {self.status}")
        self.n = A.ROW * nb

    def apply(self, b, u, kind=BSR_SWEEP_GS, weight=1.0):
        """One sweep: u (float64, contiguous) is the iterate on entry and on exit.  Returns the status."""
        bv, _b = T.as_vec(b)
        assert u.dtype == np.float64 and u.flags.c_contiguous
        uv = T.dvector(len(u), T.dp(u))
        return lib().fasp_hip_bsr_smoother_apply(self.h, kind, weight, C.byref(bv), C.byref(uv))

    def info(self):
        """{levels, chunks, slab entries, padded entries, form of the last apply, form an apply would take now}"""
        out = np.zeros(6)
        lib().fasp_hip_bsr_smoother_info(self.h, T.dp(out))
        return dict(levels=int(out[0]), chunks=int(out[1]), nent=int(out[2]), padded=int(out[3]), last_form=int(out[4]), auto_form=int(out[5]))

    def free(self):
        if self.h:
            lib().fasp_hip_bsr_smoother_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def solver_dbsr_krylov_amg(ia, ja, val, nb, b, x, itparam, amgparam):
    """Drop-in call of fasp_solver_dbsr_krylov_amg (SolBSR.c:349): x is the guess on entry, solution on exit."""
    A, _keep = T.as_bsr(ia, ja, val, nb)
    bv, _b = T.as_vec(b)
    assert x.dtype == np.float64 and x.flags.c_contiguous
    xv = T.dvector(len(x), T.dp(x))
    return lib().fasp_solver_dbsr_krylov_amg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itparam),
                                             C.byref(amgparam))


def solver_amg(ia, ja, a, b, x, amgparam):
    """Drop-in call of fasp_solver_amg (SolAMG.c:49): x is the guess on entry, solution on exit."""
    A, _keep = T.as_csr(ia, ja, a)
    bv, _b = T.as_vec(b)
    assert x.dtype == np.float64 and x.flags.c_contiguous
    xv = T.dvector(len(x), T.dp(x))
    return lib().fasp_solver_amg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(amgparam))



def solver_safe(fmt, method, A, b, x, pc=None, tol=1e-8, maxit=500, restart=25, stop_type=T.STOP_REL_RES, print_level=0):
    """fasp_solver_d<fmt>_<method> (KrySP*.c: the Krylov methods with a safety net): fmt "csr" / "bsr" / "str", method one of
    SAFE_FORMATS[fmt], A the matching struct of _types (as_csr / as_bsr / as_str), pc a _types.precond or None.  x (numpy f64) is the
    guess on entry and the solution on exit.  Returns the iteration count or a negative ERROR_* code."""
    assert method in SAFE_FORMATS[fmt] and x.dtype == np.float64 and x.flags.c_contiguous
    bv, _b = T.as_vec(b)
    xv = T.dvector(len(x), T.dp(x))
    args = [C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc) if pc is not None else None, tol, maxit]
    if method.endswith("gmres"):
        args.append(restart)
    return getattr(lib(), f"fasp_solver_d{fmt}_{method}")(*args, stop_type, print_level)


def solver_dcsr_itsolver_s(ia, ja, a, b, x, itparam, pc=None):
    """fasp_solver_dcsr_itsolver_s (SolCSR.c:163): the safe-net method itparam.itsolver_type selects, with the caller's precond."""
    A, _keep = T.as_csr(ia, ja, a)
    bv, _b = T.as_vec(b)
    assert x.dtype == np.float64 and x.flags.c_contiguous
    xv = T.dvector(len(x), T.dp(x))
    return lib().fasp_solver_dcsr_itsolver_s(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc) if pc is not None else None, C.byref(itparam))


def solver_dcsr_krylov_s(ia, ja, a, b, x, itparam):
    """fasp_solver_dcsr_krylov_s (SolCSR.c:295): fasp_solver_dcsr_itsolver_s without a preconditioner."""
    A, _keep = T.as_csr(ia, ja, a)
    bv, _b = T.as_vec(b)
    assert x.dtype == np.float64 and x.flags.c_contiguous
    xv = T.dvector(len(x), T.dp(x))
    return lib().fasp_solver_dcsr_krylov_s(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itparam))


def safe_update_selftest(which, n, seed):
    """fasp_hip_safe_update_selftest -> (elementwise mismatches, scalars of the fused kernel, scalars of the BLAS-1 sequence)."""
    out = np.zeros(18)
    st = lib().fasp_hip_safe_update_selftest(which, n, seed, T.dp(out))
    if st < 0:
        raise RuntimeError(f"fasp_hip_safe_update_selftest failed with status {st}")
    nq = int(out[1])
    return int(out[0]), out[2:2 + nq].copy(), out[10:10 + nq].copy()


BLAS1_KERNELS = ("cg_update", "axpby_beta", "mgs_step", "finalize", "dot", "norms", "norm1_nan", "axpy", "axpby", "axpyz", "axpy_self",
                 "scale", "set", "poly_scale", "poly_start", "poly_step", "jacobi_zero", "l1_zero", "diag_precond", "bsr_dinv_apply", "pack")


def blas1_op(kernel, n, vectors=(), scal=(), ipar=(), variant=0, partials=None, idx=None):
    """fasp_hip_blas1_op (include/fasp_hip_dev.h): one launch of BLAS1_KERNELS[kernel] (or a name of it) on the caller's vectors, by slot.
    Returns (status, dict): "vec" the vectors as the kernel left them (copies; the inputs stay), "red" the finalised scalars, "partials"
    the raw per-block partials (quantities x grid), "grid", "pub" the published scalar.  status < 0: the dict holds what was passed in."""
    k = BLAS1_KERNELS.index(kernel) if isinstance(kernel, str) else int(kernel)
    vin = [np.ascontiguousarray(v, dtype=np.float64) for v in vectors]
    out = [v.copy() for v in vin]
    PA = T.c_double_p * 6
    pin = PA(*([T.dp(v) for v in vin] + [None] * (6 - len(vin))))
    pout = PA(*([T.dp(v) for v in out] + [None] * (6 - len(out))))
    sc = np.zeros(8); sc[:len(scal)] = scal
    ipr = np.zeros(4, dtype=np.int32); ipr[:len(ipar)] = ipar
    part = None if partials is None else np.ascontiguousarray(partials, dtype=np.float64).reshape(-1)
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    red = np.zeros(8); pout_part = np.zeros(8 * 2048); grid = np.zeros(2, dtype=np.int32); pub = np.zeros(1)
    st = lib().fasp_hip_blas1_op(k, variant, n, T.ip(ipr), T.dp(sc), pin, pout, None if part is None else T.dp(part),
                                 0 if part is None else len(part), None if ix is None else T.ip(ix), T.dp(red), T.dp(pout_part),
                                 T.ip(grid), T.dp(pub))
    G, nq = int(grid[0]), int(grid[1])
    return st, {"vec": out, "red": red[:nq].copy(), "partials": pout_part[:nq * G].reshape(nq, G).copy() if nq else np.zeros((0, G)),
                "grid": G, "pub": float(pub[0])}
