"""ctypes binding of the C ABI declared in include/sgp_hip.h.

The product path has no CPU fallback: if the library is missing or no gfx950 device is visible the
calls raise.  (`oracle/` is test infrastructure and is never imported from this package.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

SGP_FLAG_NO_GRAPH = 1          # no-op: launches are always eager
SGP_FLAG_KEEP_KUF = 2
SGP_FLAG_GRAPH = 4             # no-op: graph replay was measured slower and removed (DESIGN.md "Launch mode")
SGP_FLAG_PERSISTENT_CHAIN = 8
SGP_FLAG_REUSE_STATS = 16      # sgp_sweep reuses the resident statistics where the setters left them valid (sgp_sweep_kind)
SGP_SWEEP_FULL, SGP_SWEEP_TARGETS, SGP_SWEEP_REUSED, SGP_SWEEP_REWEIGHTED = 0, 1, 2, 3
SGP_S_YY, SGP_S_W, SGP_S_N, SGP_S_COUNT = 0, 1, 2, 8
(SGP_R_SUM_I1, SGP_R_SUM_I2, SGP_R_ENERGY, SGP_R_INFO_KUU, SGP_R_INFO_LAMBDA, SGP_R_INFO_PRIOR,
 SGP_R_LOGDET_KUU, SGP_R_LOGDET_LAMBDA, SGP_R_COUNT) = range(9)
SGP_T_SWEEP, SGP_T_GRAM, SGP_T_SYRK, SGP_T_FINISH1, SGP_T_FINISH2, SGP_T_GAP_LOCAL_FINISH, SGP_T_KUU, SGP_T_LOCAL = range(8)
SGP_T_COUNT = 8

EXPORTS = [
    "sgp_abi_version", "sgp_create", "sgp_destroy", "sgp_last_error", "sgp_set_inducing", "sgp_set_data",
    "sgp_set_kernel", "sgp_set_output_cov_sum", "sgp_set_prior", "sgp_set_noise", "sgp_sweep_local", "sgp_sweep_finish", "sgp_sweep",
    "sgp_stats_layout", "sgp_bind_stats", "sgp_get_posterior", "sgp_get_scalars", "sgp_get_stats",
    "sgp_get_kuu_chol", "sgp_get_wishart_invscale", "sgp_w_stats", "sgp_predict", "sgp_theta_objective", "sgp_carry_posterior", "sgp_set_posterior",
    "sgp_kernelmatrix", "sgp_potrf", "sgp_potri", "sgp_get_timestamps", "sgp_get_phase_totals", "sgp_time_kernel", "sgp_get_chain_trace", "sgp_set_allreduce", "sgp_use_rccl", "sgp_measure_sclk_mhz",
    "sgp_train_begin", "sgp_train_step", "sgp_train_end", "sgp_get_step_trace", "sgp_measure_clocks", "sgp_overlap_plan",
    "sgp_get_sweep_trace", "sgp_train_likelihood", "sgp_train_get_gamma", "sgp_wait", "sgp_set_targets", "sgp_sweep_kind",
    "sgp_predict_var", "sgp_set_kernel_family", "sgp_kernelmatrix_family", "sgp_in_message", "sgp_in_message_grad",
    "sgp_theta_descend", "sgp_out_message", "sgp_psi_stats", "sgp_sweep_local_psi",
    "sgp_theta_objective_psi", "sgp_theta_descend_psi", "sgp_psi_in_grad", "sgp_psi_predict",
    "sgp_theta_objective_xu", "sgp_theta_objective_psi_xu", "sgp_inducing_descend", "sgp_inducing_descend_psi",
    "sgp_sweep_plan", "sgp_select_inducing", "sgp_predict_joint", "sgp_sample_f", "sgp_vmp_run",
    "sgp_vmp_run_t", "sgp_vmp_run_w", "sgp_sample_path", "sgp_predict_grad",
]
# sgp_sweep_plan's bits (SGP_PLAN_* of include/sgp_hip.h), by name
PLAN_BITS = {"overlapped": 1, "pack": 2, "events": 4, "join_word": 8, "kuu_interleaved": 16, "stats_first": 32, "gate_side": 64,
             "resident": 128}
# kernel families (SGP_KERNEL_* of include/sgp_hip.h), by the names the Python layer accepts
SGP_KERNEL_SE, SGP_KERNEL_MATERN12, SGP_KERNEL_MATERN32, SGP_KERNEL_MATERN52 = 0, 1, 2, 3
KERNEL_FAMILIES = {"se": SGP_KERNEL_SE, "matern12": SGP_KERNEL_MATERN12, "matern32": SGP_KERNEL_MATERN32,
                   "matern52": SGP_KERNEL_MATERN52}


def family_id(family) -> int:
    """SGP_KERNEL_* id of a family name ("se", "matern12", "matern32", "matern52"); None is SE."""
    if family is None:
        return SGP_KERNEL_SE
    try:
        return KERNEL_FAMILIES[str(family).lower()]
    except KeyError:
        raise ValueError(f"unknown kernel family {family!r}: expected one of {sorted(KERNEL_FAMILIES)}") from None

SGP_TIME_GROUP0 = 100
SGP_TIME_QUADFORM = 120
SGP_PREDICT_NOISE = 1         # sgp_predict_var: add the observation noise W^-1
SGP_JOINT_MAX_ROWS = 8192     # sgp_predict_joint / sgp_sample_f: ns * d_out
SGP_PATH_MAX_FEATURES = 16384  # sgp_sample_path: L
SGP_PATH_MAX_COLUMNS = 2097152  # sgp_sample_path: d_out * n_samples
SGP_DESCEND_THETA, SGP_DESCEND_XU = 1, 2     # sgp_inducing_descend[_psi]: what the optimised vector holds
SGP_VMP_GAUSSIAN, SGP_VMP_PROBIT = 0, 1       # sgp_vmp_run: likelihood
SGP_VMP_HOLD_W = 1                            # sgp_vmp_run, sgp_vmp_run_t, sgp_vmp_run_w: flags
SGP_VMP_W_TERMS = 4                           # sgp_vmp_run_w: entries of `terms` per iteration


class SGPError(RuntimeError):
    """Negative status from the C ABI (bad argument, HIP error, no device)."""


class PosDefException(ArithmeticError):
    """Positive status k: leading minor k is not positive definite (Julia's PosDefException(k))."""

    def __init__(self, k, msg=""):
        super().__init__(f"matrix is not positive definite; Cholesky failed at minor {k}. {msg}")
        self.info = k


class Config(C.Structure):
    _fields_ = [("n_max", C.c_int64), ("m", C.c_int32), ("d", C.c_int32), ("d_out", C.c_int32),
                ("device", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


# int hook(void* ctx, void* stats_dev, int64_t count, void* stream): the all-reduce step of sgp_sweep (include/sgp_hip.h)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

_libs = {}


def library_path(variant=None) -> str:
    return _build.lib_path(variant)


def load(build_if_missing: bool = True, variant=None):
    """Load csrc/libsgp_hip.so -- or a variant library of the same ABI, see _build.VARIANTS -- building it first if hipcc is
    available.  Raises if it cannot."""
    if variant is None:
        variant = os.environ.get("SGP_LIB_VARIANT") or None      # diagnostics: run any script on a variant library (tools/step_trace.py)
    if variant in _libs:
        return _libs[variant]
    # PyTorch (used for streams / torch.distributed around this library) bundles its own libamdhip64.so.7.
    # A process must hold ONE HIP runtime: import torch first when it is installed so that this library's
    # DT_NEEDED libamdhip64.so.7 resolves to the copy torch already loaded (loading the system runtime
    # first leaves torch unable to see the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = _build.lib_path(variant)
    if not os.path.exists(path):
        if not build_if_missing:
            raise SGPError(f"{path} is missing: build it with `python -m gaussianprocessnode_amd._build`")
        _build.build(variant=variant)
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    lib.sgp_abi_version.restype = C.c_int
    lib.sgp_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.sgp_destroy.argtypes = [vp]
    lib.sgp_last_error.argtypes = [vp]
    lib.sgp_last_error.restype = C.c_char_p
    lib.sgp_set_inducing.argtypes = [vp, dp]
    lib.sgp_set_data.argtypes = [vp, dp, dp, dp, dp, C.c_int64, C.c_double]
    lib.sgp_set_output_cov_sum.argtypes = [vp, dp]
    lib.sgp_set_kernel.argtypes = [vp, C.c_double, dp, C.c_int32, C.c_double]
    lib.sgp_set_prior.argtypes = [vp, dp, dp, C.c_int32]
    lib.sgp_set_noise.argtypes = [vp, dp, C.c_double]
    for name in ("sgp_sweep_local", "sgp_sweep_finish", "sgp_sweep"):
        getattr(lib, name).argtypes = [vp, vp]
    lib.sgp_stats_layout.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.sgp_bind_stats.argtypes = [vp, vp]
    lib.sgp_get_posterior.argtypes = [vp, dp, dp, dp]
    lib.sgp_get_scalars.argtypes = [vp, dp]
    lib.sgp_get_stats.argtypes = [vp, dp, dp, dp]
    lib.sgp_get_kuu_chol.argtypes = [vp, dp]
    lib.sgp_get_wishart_invscale.argtypes = [vp, dp]
    lib.sgp_w_stats.argtypes = [vp, dp, dp, vp]
    lib.sgp_carry_posterior.argtypes = [vp, vp]
    lib.sgp_set_posterior.argtypes = [vp, dp, dp]
    lib.sgp_predict.argtypes = [vp, dp, C.c_int64, dp, dp]
    lib.sgp_predict_var.argtypes = [vp, dp, C.c_int64, dp, dp, C.c_int32, dp, dp]
    lib.sgp_predict_grad.argtypes = [vp, dp, C.c_int64, dp, dp, C.c_int32, dp, dp, dp, dp, dp]
    lib.sgp_predict_joint.argtypes = [vp, dp, C.c_int64, dp, dp, C.c_int32, dp, dp]
    lib.sgp_sample_f.argtypes = [vp, dp, C.c_int64, dp, dp, C.c_int32, C.c_double, dp, C.c_int64, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_sample_path.argtypes = [vp, dp, C.c_int64, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int64, C.c_int32, dp,
                                    C.POINTER(C.c_int64)]
    lib.sgp_in_message.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64), C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp]
    lib.sgp_in_message_grad.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64), C.c_int64, dp, dp, dp, dp, dp, dp]
    lib.sgp_out_message.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64), C.c_int64, dp, dp, dp, dp]
    lib.sgp_psi_stats.argtypes = [vp, dp, dp, C.c_int64, dp, dp, dp, dp, dp]
    lib.sgp_sweep_local_psi.argtypes = [vp, dp, dp, dp, dp, C.c_int64, vp]
    lib.sgp_theta_objective.argtypes = [vp, dp, dp]
    lib.sgp_theta_objective_xu.argtypes = [vp, dp, dp, dp]
    lib.sgp_kernelmatrix.argtypes = [C.c_int32, dp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_double, dp, C.c_int32, dp]
    lib.sgp_kernelmatrix_family.argtypes = [C.c_int32, C.c_int32, dp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_double, dp,
                                            C.c_int32, dp]
    lib.sgp_set_kernel_family.argtypes = [vp, C.c_int32]
    lib.sgp_potrf.argtypes = [C.c_int32, dp, C.c_int32, dp]
    lib.sgp_potri.argtypes = [C.c_int32, dp, C.c_int32, dp]
    lib.sgp_get_timestamps.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.sgp_get_phase_totals.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]
    lib.sgp_time_kernel.argtypes = [vp, C.c_int32, C.c_int32, vp, dp]
    lib.sgp_get_chain_trace.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
    lib.sgp_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    lib.sgp_use_rccl.argtypes = [vp, vp]
    lib.sgp_measure_sclk_mhz.argtypes = [C.c_int32, dp]
    lib.sgp_train_begin.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.sgp_train_step.argtypes = [vp, C.c_int64, C.c_int64, C.c_int32]
    lib.sgp_train_end.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    lib.sgp_theta_descend.argtypes = [vp, dp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, dp, dp,
                                      C.POINTER(C.c_int64)]
    lib.sgp_theta_objective_psi.argtypes = [vp, dp, dp, dp, C.c_int64, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_theta_objective_psi_xu.argtypes = [vp, dp, dp, dp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_psi_in_grad.argtypes = [vp, dp, dp, dp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_psi_predict.argtypes = [vp, dp, dp, C.c_int64, C.c_int32, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_theta_descend_psi.argtypes = [vp, dp, dp, dp, C.c_int64, dp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                          C.c_double, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_inducing_descend.argtypes = [vp, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                         dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_inducing_descend_psi.argtypes = [vp, dp, dp, dp, C.c_int64, dp, C.c_int32, dp, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                             C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_select_inducing.argtypes = [vp, dp, C.c_int64, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int64), dp,
                                        C.POINTER(C.c_int32)]
    lib.sgp_vmp_run.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, C.c_double, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_vmp_run_t.argtypes = [vp, C.c_double, dp, C.c_int32, C.c_int32, dp, dp, C.c_double, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_vmp_run_w.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, C.c_double, dp, dp, C.POINTER(C.c_int64)]
    lib.sgp_get_step_trace.argtypes = [C.POINTER(C.c_int64)]
    lib.sgp_measure_clocks.argtypes = [C.c_int32, dp]
    lib.sgp_overlap_plan.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sgp_sweep_plan.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.sgp_get_sweep_trace.argtypes =[C.POINTER(C.c_int64)]
    lib.sgp_train_likelihood.argtypes = [vp, C.c_int32, C.c_double, C.c_double]
    lib.sgp_train_get_gamma.argtypes = [vp, dp]
    lib.sgp_wait.argtypes = [vp]
    lib.sgp_set_targets.argtypes = [vp, dp, dp]
    lib.sgp_sweep_kind.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name != "sgp_last_error":
            fn.restype = C.c_int
    _libs[variant] = lib
    return lib


def as_f64(a, shape=None):
    """C-contiguous float64 view/copy (the memory layout the ABI expects: points along axis 0)."""
    arr = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and arr.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {arr.shape}")
    return arr


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def check(rc: int, handle=None, what: str = "", lib=None):
    if rc == 0:
        return
    lib = lib or load()
    msg = lib.sgp_last_error(handle)
    msg = msg.decode() if msg else ""
    if rc > 0:
        raise PosDefException(rc, f"{what} {msg}")
    raise SGPError(f"{what} failed with status {rc}: {msg}")
