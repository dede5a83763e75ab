"""ctypes binding of libgpsat_hip.so (C ABI declared in include/gpsat_hip.h).

The product path has no CPU fallback: if the shared library is missing or a symbol is
absent, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPSAT_LIB: developer override to load the diagnostic build (scripts/phase_profile.py); never a fallback
LIB_PATH = os.environ.get("GPSAT_LIB") or os.path.join(_HERE, "csrc", "libgpsat_hip.so")

# constants mirrored from include/gpsat_hip.h
ABI_VERSION = 4
F32, F64 = 0, 1
KERNEL_IDS = {"RBF": 0, "SquaredExponential": 0, "Matern12": 1, "Exponential": 1, "Matern32": 2, "Matern52": 3,
              "RationalQuadratic": 4}
KERNEL_RQ = 4      # GPSAT_KERNEL_RQ: one more hyper-parameter (alpha, last), fp64 and D <= 3 only
MEAN_ZERO, MEAN_CONSTANT = 0, 1      # GPSAT_MEAN_*: a trainable constant mean is one more hyper-parameter (c, last)
MEAN_IDS = {None: MEAN_ZERO, "zero": MEAN_ZERO, "constant": MEAN_CONSTANT}
OPT_NONE, OPT_LBFGS, OPT_ADAM = 0, 1, 2
OPT_IDS = {"none": OPT_NONE, None: OPT_NONE, "lbfgs": OPT_LBFGS, "L-BFGS-B": OPT_LBFGS, "adam": OPT_ADAM}
MEM_HOST, MEM_DEVICE = 0, 1
STATUS = {0: "converged", 1: "max_iter", 2: "not_pd", 3: "nan", 4: "skipped", 5: "not_optimised", 6: "ls_failed"}

EXPORTS = ["gpsat_version", "gpsat_last_error", "gpsat_device_count", "gpsat_create", "gpsat_device_name",
           "gpsat_destroy", "gpsat_fit_predict_batch", "gpsat_last_timing", "gpsat_select_batch",
           "gpsat_smooth_batch", "gpsat_glue_batch", "gpsat_max_tile_obs", "gpsat_sgpr_fit_predict_batch",
           "gpsat_max_inducing", "gpsat_select_batch_ex", "gpsat_fit_predict_batch_ms", "gpsat_bin_batch",
           "gpsat_fit_predict_batch_cv", "gpsat_max_cv_fold", "gpsat_cv_refit_count", "gpsat_fit_predict_batch_cv_refit",
           "gpsat_n_hyper", "gpsat_n_hyper_mean", "gpsat_fit_predict_batch_mean", "gpsat_fit_predict_batch_noise"]
# ABI additions that keep GPSAT_ABI_VERSION: callers detect them by their presence (engine: a clear error if absent)
OPTIONAL_EXPORTS = ["gpsat_fit_predict_batch_ms", "gpsat_bin_batch", "gpsat_fit_predict_batch_cv", "gpsat_max_cv_fold",
                    "gpsat_cv_refit_count", "gpsat_fit_predict_batch_cv_refit", "gpsat_n_hyper",
                    "gpsat_n_hyper_mean", "gpsat_fit_predict_batch_mean", "gpsat_fit_predict_batch_noise"]


class GpsatOpts(C.Structure):
    _fields_ = [("workgroups_per_cu", C.c_int32), ("reserved", C.c_int32 * 7)]


class GpsatBatch(C.Structure):
    _fields_ = [
        ("T", C.c_int32), ("D", C.c_int32), ("dtype", C.c_int32), ("kernel", C.c_int32),
        ("memory", C.c_int32), ("optimiser", C.c_int32), ("max_iter", C.c_int32), ("max_ls", C.c_int32),
        ("ftol", C.c_double), ("gtol", C.c_double), ("adam_lr", C.c_double),
        ("obs_off", C.c_void_p), ("pred_off", C.c_void_p), ("theta0", C.c_void_p), ("lo", C.c_void_p),
        ("hi", C.c_void_p), ("trainable", C.c_void_p),
        ("X", C.c_void_p), ("y", C.c_void_p), ("Xs", C.c_void_p),
        ("theta", C.c_void_p), ("nll", C.c_void_p), ("grad", C.c_void_p), ("status", C.c_void_p),
        ("n_eval", C.c_void_p), ("f_mean", C.c_void_p), ("f_var", C.c_void_p), ("y_var", C.c_void_p),
        ("cov_off", C.c_void_p), ("f_cov", C.c_void_p), ("n_iter", C.c_void_p),
    ]


class GpsatSparse(C.Structure):
    _fields_ = [("z_off", C.c_void_p), ("Z", C.c_void_p), ("jitter", C.c_double), ("reserved", C.c_int32 * 8)]


TRANSFORM_LOG = 1


class GpsatMultistart(C.Structure):
    _fields_ = [("n_starts", C.c_int32), ("transform", C.c_int32), ("starts", C.c_void_p), ("f_start", C.c_void_p),
                ("reserved", C.c_int32 * 8)]


class GpsatMean(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32 * 7)]


class GpsatNoise(C.Structure):
    _fields_ = [("obs_var", C.c_void_p), ("reserved", C.c_int32 * 8)]


class GpsatCv(C.Structure):
    _fields_ = [("fold", C.c_void_p), ("cv_mean", C.c_void_p), ("cv_f_var", C.c_void_p), ("cv_y_var", C.c_void_p),
                ("reserved", C.c_int32 * 8)]


class GpsatCvRefit(C.Structure):
    _fields_ = [("fold", C.c_void_p), ("start", C.c_int32), ("recentre", C.c_int32), ("min_obs", C.c_int32),
                ("fold_off", C.c_void_p), ("cv_mean", C.c_void_p), ("cv_f_var", C.c_void_p), ("cv_y_var", C.c_void_p),
                ("fold_theta", C.c_void_p), ("fold_nll", C.c_void_p), ("fold_shift", C.c_void_p),
                ("fold_status", C.c_void_p), ("fold_n_eval", C.c_void_p), ("fold_n_iter", C.c_void_p),
                ("fold_n_obs", C.c_void_p), ("fold_label", C.c_void_p), ("reserved", C.c_int32 * 8)]


CV_START_IDS = {"theta0": 0, "full": 1}

SEL_MAXCRIT = 4
COMP_IDS = {">=": 0, ">": 1, "==": 2, "<": 3, "<=": 4}


class GpsatSelectSpec(C.Structure):
    _fields_ = [("n_crit", C.c_int32), ("kind", C.c_int32 * SEL_MAXCRIT), ("comp", C.c_int32 * SEL_MAXCRIT),
                ("ncols", C.c_int32 * SEL_MAXCRIT), ("cols", (C.c_int32 * 3) * SEL_MAXCRIT),
                ("val", C.c_double * SEL_MAXCRIT)]


# statistics of gpsat_bin_batch (GPSAT_BIN_*), in the order of their bits = the order of the output rows
BIN_STATS = {"count": 1, "sum": 2, "mean": 4, "std": 8, "min": 16, "max": 32, "median": 64}


class LibraryMissing(ImportError):
    pass


def _one_hip_runtime():
    """A process must use ONE HIP runtime.  PyTorch wheels bundle their own libamdhip64 (same SONAME as the system ROCm's);
    whichever is loaded first serves both.  If this library came first with the system runtime, a later `import torch` +
    CUDA initialisation finds "No HIP GPUs"; the other way round works.  So when PyTorch is installed, its runtime is
    loaded first -- without importing torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError as e:
            import warnings
            warnings.warn(f"gpsat_amd: could not preload PyTorch's HIP runtime {cand}: {e}; if torch is imported later in this "
                          f"process it may not see the GPU")


def _check_one_hip_runtime():
    """After libgpsat_hip.so is loaded: the de-duplication above only works when PyTorch's bundled runtime has the SONAME
    this library was linked against (same ROCm major).  Two different libamdhip64 files mapped into the process = two
    runtimes: say so instead of failing later with 'No HIP GPUs'."""
    try:
        paths = set()
        for line in open("/proc/self/maps"):
            if "libamdhip64.so" in line:
                paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        return
    if len(paths) > 1:
        import warnings
        warnings.warn("gpsat_amd: two HIP runtimes are loaded (" + ", ".join(sorted(paths)) + "): libgpsat_hip.so was built "
                      "against a ROCm whose libamdhip64 SONAME differs from the one PyTorch bundles.  Build the library with "
                      "the ROCm release PyTorch was built for (INTEGRATION.md, 'One HIP runtime per process').")


def load():
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C gpsat_amd/csrc` (there is no CPU fallback)")
    _one_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    _check_one_hip_runtime()
    for name in EXPORTS:
        if name not in OPTIONAL_EXPORTS and not hasattr(lib, name):
            raise LibraryMissing(f"{LIB_PATH} does not export {name}")
    lib.gpsat_version.restype = C.c_int
    lib.gpsat_last_error.restype = C.c_char_p
    lib.gpsat_device_count.restype = C.c_int
    lib.gpsat_create.restype = C.c_int
    lib.gpsat_create.argtypes = [C.c_int, C.POINTER(GpsatOpts), C.POINTER(C.c_void_p)]
    lib.gpsat_device_name.restype = C.c_int
    lib.gpsat_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.gpsat_destroy.restype = C.c_int
    lib.gpsat_destroy.argtypes = [C.c_void_p]
    lib.gpsat_fit_predict_batch.restype = C.c_int
    lib.gpsat_fit_predict_batch.argtypes = [C.c_void_p, C.POINTER(GpsatBatch)]
    lib.gpsat_select_batch.restype = C.c_int
    lib.gpsat_select_batch.argtypes = [C.c_void_p, C.POINTER(GpsatSelectSpec), C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.gpsat_select_batch_ex.restype = C.c_int
    lib.gpsat_select_batch_ex.argtypes = [C.c_void_p, C.POINTER(GpsatSelectSpec), C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.gpsat_smooth_batch.restype = C.c_int
    lib.gpsat_smooth_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    lib.gpsat_glue_batch.restype = C.c_int
    lib.gpsat_glue_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.gpsat_max_tile_obs.restype = C.c_int
    lib.gpsat_max_tile_obs.argtypes = [C.c_int, C.c_int]
    lib.gpsat_sgpr_fit_predict_batch.restype = C.c_int
    lib.gpsat_sgpr_fit_predict_batch.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatSparse)]
    lib.gpsat_max_inducing.restype = C.c_int
    lib.gpsat_max_inducing.argtypes = [C.c_int, C.c_int]
    if hasattr(lib, "gpsat_fit_predict_batch_ms"):
        lib.gpsat_fit_predict_batch_ms.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatMultistart)]
        lib.gpsat_fit_predict_batch_ms.restype = C.c_int
    if hasattr(lib, "gpsat_fit_predict_batch_cv"):
        lib.gpsat_fit_predict_batch_cv.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatCv)]
        lib.gpsat_fit_predict_batch_cv.restype = C.c_int
        lib.gpsat_max_cv_fold.argtypes = [C.c_int, C.c_int]
        lib.gpsat_max_cv_fold.restype = C.c_int
    if hasattr(lib, "gpsat_fit_predict_batch_cv_refit"):
        lib.gpsat_cv_refit_count.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.gpsat_cv_refit_count.restype = C.c_int
        lib.gpsat_fit_predict_batch_cv_refit.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatCvRefit)]
        lib.gpsat_fit_predict_batch_cv_refit.restype = C.c_int
    if hasattr(lib, "gpsat_n_hyper"):
        lib.gpsat_n_hyper.argtypes = [C.c_int, C.c_int]
        lib.gpsat_n_hyper.restype = C.c_int
    if hasattr(lib, "gpsat_fit_predict_batch_mean"):
        lib.gpsat_n_hyper_mean.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.gpsat_n_hyper_mean.restype = C.c_int
        lib.gpsat_fit_predict_batch_mean.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatMean)]
        lib.gpsat_fit_predict_batch_mean.restype = C.c_int
    if hasattr(lib, "gpsat_fit_predict_batch_noise"):
        lib.gpsat_fit_predict_batch_noise.argtypes = [C.c_void_p, C.POINTER(GpsatBatch), C.POINTER(GpsatNoise)]
        lib.gpsat_fit_predict_batch_noise.restype = C.c_int
    if hasattr(lib, "gpsat_bin_batch"):
        lib.gpsat_bin_batch.restype = C.c_int
        lib.gpsat_bin_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_double, C.c_uint32,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gpsat_last_timing.restype = C.c_int
    lib.gpsat_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if lib.gpsat_version() != ABI_VERSION:
        raise LibraryMissing(f"ABI version mismatch: library {lib.gpsat_version()} != binding {ABI_VERSION}")
    return lib


def n_hyper(kernel, D: int, mean=None) -> int:
    """Hyper-parameters per tile (gpsat_n_hyper, gpsat_n_hyper_mean): D + 3 for "RationalQuadratic" (lengthscales, kernel
    variance, likelihood variance, alpha) and for ``mean="constant"`` with another kernel (..., likelihood variance, c), D + 2
    otherwise.  Host arithmetic, the same rule as the library's for the arguments it supports: shapes can be laid out without
    loading it."""
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    return int(D) + (3 if kid == KERNEL_RQ or MEAN_IDS[mean] == MEAN_CONSTANT else 2)


def max_tile_obs(dtype: str, D: int) -> int:
    """Largest tile (observations) the kernels take for this dtype / input dimension (gpsat_max_tile_obs)."""
    return int(get_lib().gpsat_max_tile_obs(F32 if dtype == "f32" else F64, int(D)))


def max_inducing(dtype: str, D: int) -> int:
    """Largest number of inducing points per sparse tile (gpsat_max_inducing); 0 for fp32 in this build."""
    return int(get_lib().gpsat_max_inducing(F32 if dtype == "f32" else F64, int(D)))


def max_cv_fold(dtype: str, D: int) -> int:
    """Largest fold (rows held out together) of gpsat_fit_predict_batch_cv; 0 for fp32."""
    lib = get_lib()
    if not hasattr(lib, "gpsat_max_cv_fold"):
        return 0
    return int(lib.gpsat_max_cv_fold(F32 if dtype == "f32" else F64, int(D)))


_lib = None


def get_lib():
    global _lib
    if _lib is None:
        _lib = load()
    return _lib
