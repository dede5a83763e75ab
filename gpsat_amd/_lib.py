"""ctypes binding of libgpsat_hip.so (C ABI declared in include/gpsat_hip.h).

The product path has no CPU fallback: if the shared library is missing or a symbol is
absent, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import variants

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


class GpsatPredGrad(C.Structure):
    _fields_ = [("f_grad", C.c_void_p), ("f_grad_var", C.c_void_p), ("reserved", C.c_int32 * 8)]


class GpsatPredHess(C.Structure):
    _fields_ = [("f_hess", C.c_void_p), ("f_hess_var", C.c_void_p), ("f_lap", C.c_void_p), ("f_lap_var", C.c_void_p),
                ("f_grad", C.c_void_p), ("f_grad_var", C.c_void_p), ("lap_weight", C.c_double * 4), ("dims", C.c_uint32),
                ("reserved", C.c_int32 * 7)]


class GpsatCv(C.Structure):
    _fields_ = [("fold", C.c_void_p), ("cv_mean", C.c_void_p), ("cv_f_var", C.c_void_p), ("cv_y_var", C.c_void_p),
                ("reserved", C.c_int32 * 8)]


class GpsatCvRefit(C.Structure):
    _fields_ = [("fold", C.c_void_p), ("start", C.c_int32), ("recentre", C.c_int32), ("min_obs", C.c_int32),
                ("fold_off", C.c_void_p), ("cv_mean", C.c_void_p), ("cv_f_var", C.c_void_p), ("cv_y_var", C.c_void_p),
                ("fold_theta", C.c_void_p), ("fold_nll", C.c_void_p), ("fold_shift", C.c_void_p),
                ("fold_status", C.c_void_p), ("fold_n_eval", C.c_void_p), ("fold_n_iter", C.c_void_p),
                ("fold_n_obs", C.c_void_p), ("fold_label", C.c_void_p), ("reserved", C.c_int32 * 8)]


class GpsatCvJoint(C.Structure):
    _fields_ = [("fold_off", C.c_void_p), ("fold_lpd", C.c_void_p), ("reserved", C.c_int32 * 8)]


PROJECT_IDS = {"forward": 0, "inverse": 1}      # GPSAT_PROJECT_*
TRACK_MODES = {"cut": 0, "runs": 1, "given": 2}             # GPSAT_TRACK_*


class GpsatProject(C.Structure):
    _fields_ = [("n", C.c_int64), ("direction", C.c_int32), ("memory", C.c_int32), ("lon_0", C.c_double), ("lat_0", C.c_double),
                ("in0", C.c_void_p), ("in1", C.c_void_p), ("out0", C.c_void_p), ("out1", C.c_void_p), ("reserved", C.c_int32 * 8)]


class GpsatTrack(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_cols", C.c_int32), ("memory", C.c_int32), ("cols", C.c_void_p * 3), ("group", C.c_void_p),
                ("cut_off", C.c_double), ("start_track", C.c_int32), ("mode", C.c_int32), ("out_delta", C.c_void_p),
                ("out_track", C.c_void_p), ("out_order", C.c_void_p), ("reserved", C.c_int32 * 8)]


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


_I, _I32, _I64, _U32, _D, _P, _S = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_double, C.c_void_p, C.c_char_p
_EXT = {v.entry: globals()[v.struct] for v in variants.VARIANTS.values() if v.entry}       # entry point -> its extension struct
_SELECT = [_P, C.POINTER(GpsatSelectSpec), _I64, _I32, _P, _I32, _P]
# name -> (restype, argtypes or None, required).  Not required: an ABI addition that keeps GPSAT_ABI_VERSION; callers detect
# it by its presence (engine: a clear error if absent).
SIGNATURES = {
    "gpsat_version": (_I, None, True),
    "gpsat_last_error": (_S, None, True),
    "gpsat_device_count": (_I, None, True),
    "gpsat_create": (_I, [_I, C.POINTER(GpsatOpts), C.POINTER(_P)], True),
    "gpsat_device_name": (_I, [_P, _S, _I], True),
    "gpsat_destroy": (_I, [_P], True),
    "gpsat_fit_predict_batch": (_I, [_P, C.POINTER(GpsatBatch)], True),
    "gpsat_last_timing": (_I, [_P, C.POINTER(_D), C.POINTER(_D)], True),
    "gpsat_select_batch": (_I, _SELECT + [_P, _P, _I64], True),
    "gpsat_select_batch_ex": (_I, _SELECT + [_I32, _P, _P, _P, _I64], True),
    "gpsat_smooth_batch": (_I, [_P, _I32, _P, _P, _P, _D, _D, _P], True),
    "gpsat_glue_batch": (_I, [_P, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _D, _P, _P], True),
    "gpsat_max_tile_obs": (_I, [_I, _I], True),
    "gpsat_max_inducing": (_I, [_I, _I], True),
    "gpsat_max_cv_fold": (_I, [_I, _I], False),
    "gpsat_cv_refit_count": (_I, [_I32, _P, _P, _P, C.POINTER(_I64)], False),
    "gpsat_n_hyper": (_I, [_I, _I], False),
    "gpsat_n_hyper_mean": (_I, [_I, _I, _I], False),
    "gpsat_bin_batch": (_I, [_P, _I64, _P, _P, _P, _P, _I32, _I32, _P, _D, _I32, _P, _D, _U32, _I64, _P, _P, _P], False),
    "gpsat_glue_keyed_batch": (_I, [_P, _I64, _I32, _I32, _P, _P, _P, _P, _D, _P, _D, _I64, C.POINTER(_I64), _P, _P, _P], False),
    "gpsat_glue_keyed_timing": (_I, [_P, _P], False),
    "gpsat_glue_keyed_grad_batch": (_I, [_P, _I64, _I32, _P, _P, _P, _P, _P, _D, _P, _D, _I64, C.POINTER(_I64), _P, _P, _P, _P], False),
    "gpsat_glue_keyed_hess_batch": (_I, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P, _D, _P, _D, _I64, C.POINTER(_I64), _P, _P, _P, _P, _P], False),
    "gpsat_project_batch": (_I, [_P, C.POINTER(GpsatProject)], False),
    "gpsat_track_batch": (_I, [_P, C.POINTER(GpsatTrack)], False),
    # the entry points of the variant table: (handle, batch, extension struct); the sparse one has been there since ABI 4
    **{name: (_I, [_P, C.POINTER(GpsatBatch), C.POINTER(st)], name == "gpsat_sgpr_fit_predict_batch") for name, st in _EXT.items()},
    # the joint density per fold: the cv row's call with its struct, and gpsat_cv_joint behind it
    **{name: (_I, [_P, C.POINTER(GpsatBatch), C.POINTER(_EXT[variants.VARIANTS[row].entry]),
                   C.POINTER(globals()[variants.JOINT_STRUCT])], False)
       for row, name in variants.JOINT_ENTRY.items()},
    # the gradient of the posterior mean: the plain call with gpsat_pred_grad behind the batch
    variants.PRED_GRAD_ENTRY: (_I, [_P, C.POINTER(GpsatBatch), C.POINTER(globals()[variants.PRED_GRAD_STRUCT])], False),
    # its second derivatives, with the gradient when asked for: gpsat_pred_hess behind the batch
    variants.PRED_HESS_ENTRY: (_I, [_P, C.POINTER(GpsatBatch), C.POINTER(globals()[variants.PRED_HESS_STRUCT])], False),
}
EXPORTS = list(SIGNATURES)
OPTIONAL_EXPORTS = [name for name, (_, _, required) in SIGNATURES.items() if not required]


def load():
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C gpsat_amd/csrc` (there is no CPU fallback)")
    _one_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    _check_one_hip_runtime()
    for name, (_, _, required) in SIGNATURES.items():
        if required and not hasattr(lib, name):
            raise LibraryMissing(f"{LIB_PATH} does not export {name}")
    for name, (restype, argtypes, _) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
    if lib.gpsat_version() != ABI_VERSION:
        raise LibraryMissing(f"ABI version mismatch: library {lib.gpsat_version()} != binding {ABI_VERSION}")
    return lib


def n_hyper(kernel, D: int, mean=None) -> int:
    """Hyper-parameters per tile (gpsat_n_hyper, gpsat_n_hyper_mean) of a kernel (name or id) and a mean: the layout of
    variants.n_hyper.  Host arithmetic, the same rule as the library's for the arguments it supports: shapes can be laid out
    without loading it."""
    return variants.n_hyper(D, theta_variants(kernel, mean))


def theta_variants(kernel, mean=None) -> list:
    """The rows of variants.VARIANTS that a kernel (name or id) and a mean ask for: those that change the layout of theta."""
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    return ["rq"] * (kid == KERNEL_RQ) + ["mean"] * (MEAN_IDS[mean] == MEAN_CONSTANT)


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
