"""The expert variants and call extensions of the host layer, as one table.

What a variant is built for -- which precision, up to which D, with which other variant it cannot be combined, which named
parameter it adds to theta, which C entry point carries it -- is stated here once.  engine.py, models.py and
local_experts.py ask this module; a new variant is one more row.  Host-only: no library and no torch are loaded.
The device-side counterpart is the variant table of the fp64 tile kernel.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

BASE_PARAMS = ("lengthscales", "kernel_variance", "likelihood_variance")
MAX_D = 4


@dataclass(frozen=True)
class Variant:
    arg: str                        # the argument that asks for it, as messages spell it
    label: str                      # what messages call it
    dtypes: tuple = ("f32", "f64")  # precisions it is built in
    max_D: int = MAX_D              # largest number of input dimensions
    stationary: bool = False        # needs a stationary kernel (every kernel built today is one)
    param: Optional[str] = None     # its named parameter, one more column of theta behind BASE_PARAMS
    excludes: frozenset = frozenset()   # rows it cannot be combined with (symmetric: checked on import)
    entry: Optional[str] = None     # the C entry point that carries it (None: a field of gpsat_batch) ...
    struct: Optional[str] = None    # ... and the ctypes struct of _lib that is its extension argument
    # Engine: two rows with entry points of their own cannot be expressed in one library call, so the wrapper refuses the
    # pair itself.  Anything else the library sees and refuses with its own message -- except the pairings named here,
    # which the wrapper refuses too ("f32": the precision).
    host_refuses: frozenset = frozenset()


_EXACT_ONLY = {"cv", "cv_refit", "multistart", "sgpr", "replacement"}      # what the three one-parameter-more kinds all exclude

VARIANTS = {
    "rq": Variant("kernel='RationalQuadratic'", "the RationalQuadratic kernel (kernel_alpha)", ("f64",), 3, False, "kernel_alpha",
                  frozenset(_EXACT_ONLY | {"mean", "noise"})),
    "mean": Variant("mean='constant'", "a trainable constant mean (mean_function 'Constant')", ("f64",), 3, True, "mean_constant",
                    frozenset(_EXACT_ONLY | {"rq", "noise"}), "gpsat_fit_predict_batch_mean", "GpsatMean", frozenset({"rq"})),
    "noise": Variant("obs_var", "noise variances per observation (obs_var_col)", ("f64",), 4, True, None,
                     frozenset(_EXACT_ONLY | {"rq", "mean"}), "gpsat_fit_predict_batch_noise", "GpsatNoise", frozenset({"rq", "f32"})),
    "cv": Variant("cv_fold", "held-out predictions (cv)", ("f64",), excludes=frozenset(
        {"rq", "mean", "noise", "cv_refit", "multistart", "sgpr", "full_cov"}), entry="gpsat_fit_predict_batch_cv", struct="GpsatCv"),
    "cv_refit": Variant("cv_refit", "held-out predictions from refitted folds (cv with refit)", excludes=frozenset(
        {"rq", "mean", "noise", "cv", "multistart", "sgpr", "full_cov"}), entry="gpsat_fit_predict_batch_cv_refit",
        struct="GpsatCvRefit", host_refuses=frozenset({"full_cov"})),
    "multistart": Variant("n_starts", "multi-start L-BFGS-B (the sklearn model)", excludes=frozenset(
        {"rq", "mean", "noise", "cv", "cv_refit", "sgpr"}), entry="gpsat_fit_predict_batch_ms", struct="GpsatMultistart"),
    "sgpr": Variant("SGPR", "sparse (SGPR) experts", ("f64",), excludes=frozenset(
        {"rq", "mean", "noise", "cv", "cv_refit", "multistart", "full_cov"}), entry="gpsat_sgpr_fit_predict_batch", struct="GpsatSparse"),
    "replacement": Variant("replacement_threshold", "a replacement model", excludes=frozenset({"rq", "mean", "noise"})),
    "full_cov": Variant("full_cov", "the full covariance (pred_kwargs.full_cov)", excludes=frozenset({"cv", "cv_refit", "sgpr"})),
}
PLAIN_ENTRY = "gpsat_fit_predict_batch"       # the call without any extension struct
# The joint log predictive density per fold (cv_joint) is an option of the two cv rows, not a row: the entry point that
# carries it takes the row's struct and, behind it, JOINT_STRUCT.
JOINT_ENTRY = {"cv": "gpsat_fit_predict_batch_cv_joint", "cv_refit": "gpsat_fit_predict_batch_cv_refit_joint"}
JOINT_STRUCT = "GpsatCvJoint"

# The gradient of the posterior mean at the prediction points, with its variance per component (pred_grad; DESIGN.md section
# 24), is an option of the plain call in the same way: its entry point takes PRED_GRAD_STRUCT behind the batch, and the rows
# below cannot be asked for beside it.  Matern12 is refused for what it is, not for what is built.
PRED_GRAD_ENTRY = "gpsat_fit_predict_batch_grad"
PRED_GRAD_STRUCT = "GpsatPredGrad"
PRED_GRAD_ARG = "pred_grad"
PRED_GRAD_LABEL = "the gradient of the posterior mean at the prediction points (pred_kwargs.gradient)"
PRED_GRAD_KERNELS = ("RBF", "SquaredExponential", "Matern32", "Matern52")
PRED_GRAD_EXCLUDES = ("rq", "mean", "noise", "cv", "cv_refit", "multistart", "sgpr", "full_cov")

for _k, _v in VARIANTS.items():
    assert all(_k in VARIANTS[_o].excludes for _o in _v.excludes), f"{_k}: excludes is not symmetric"
assert all(_k in VARIANTS for _k in PRED_GRAD_EXCLUDES)

# The second derivatives of the posterior mean at the prediction points, with their variances and a weighted Laplacian
# (pred_hess): an option of the plain call as pred_grad is, and the one that pred_grad can be combined
# with -- pred_grad then travels through PRED_HESS_ENTRY.  Matern12 and Matern32 are refused for what they are.
PRED_HESS_ENTRY = "gpsat_fit_predict_batch_hess"
PRED_HESS_STRUCT = "GpsatPredHess"
PRED_HESS_ARG = "pred_hess"
PRED_HESS_LABEL = "the second derivatives of the posterior mean at the prediction points (pred_kwargs.hessian)"
PRED_HESS_KERNELS = ("RBF", "SquaredExponential", "Matern52")
PRED_HESS_EXCLUDES = PRED_GRAD_EXCLUDES


def _param_rows(asked):
    return [VARIANTS[k] for k in VARIANTS if k in asked and VARIANTS[k].param]


def param_names(asked=()) -> list:
    """The named parameters of an expert with the variants ``asked``, in the order of theta."""
    return list(BASE_PARAMS) + [v.param for v in _param_rows(asked)]


def n_hyper(D: int, asked=()) -> int:
    """H: the columns of theta -- D lengthscales, the two variances and one per variant with a parameter of its own."""
    return int(D) + len(BASE_PARAMS) - 1 + len(_param_rows(asked))


def slots(D: int, asked=()) -> dict:
    """name -> (first column, width) of every named parameter in a tile's theta."""
    D = int(D)
    out = {"lengthscales": (0, D)}
    for name in param_names(asked)[1:]:
        out[name] = (D + len(out) - 1, 1)
    return out


def why_refused(asked, dtype: Optional[str], D: Optional[int], dims: str = "input dimensions", host_only: bool = False):
    """None when the variants ``asked`` can run together at ``dtype`` ("f32" / "f64"; None: not checked) and ``D`` (None: not
    checked), else the reason, one sentence.  ``dims``: what the caller's D counts.  ``host_only``: only what Engine refuses
    before a library call (see Variant.host_refuses)."""
    asked = [k for k in VARIANTS if k in asked]                      # table order, whatever the caller's
    for i, a in enumerate(asked):
        for b in asked[i + 1:]:
            va, vb = VARIANTS[a], VARIANTS[b]
            if b in va.excludes and (not host_only or (va.entry and vb.entry) or b in va.host_refuses or a in vb.host_refuses):
                return f"{va.arg} and {vb.arg} cannot be combined ({va.label}; {vb.label})"
    for k in asked:
        v = VARIANTS[k]
        if dtype is not None and dtype not in v.dtypes and (not host_only or dtype in v.host_refuses):
            only = " and ".join("fp" + d[1:] for d in v.dtypes)
            return f"{v.arg}: built in {only} only, not in {dtype!r} ({v.label}): pass dtype={v.dtypes[-1]!r}"
        if D is not None and D > v.max_D and not host_only:
            return f"{v.arg}: built for 1..{v.max_D} {dims} only, got {D} ({v.label})"
    return None


def why_refused_pred_grad(asked, dtype: Optional[str], kernel: Optional[str]):
    """None when the gradient of the posterior mean (pred_grad) can be asked for beside the rows ``asked`` at ``dtype`` ("f32" /
    "f64"; None: not checked) with ``kernel`` (a name; None: not checked), else the reason, one sentence."""
    if dtype is not None and dtype != "f64":
        return f"{PRED_GRAD_ARG}: built in fp64 only, not in {dtype!r} ({PRED_GRAD_LABEL}): pass dtype='f64'"
    if kernel in ("Matern12", "Exponential"):
        return (f"{PRED_GRAD_ARG}: kernel {kernel!r} has no gradient to return, a Matern-1/2 process is not mean-square "
                f"differentiable ({PRED_GRAD_LABEL})")
    for k in VARIANTS:                                               # table order, whatever the caller's
        if k in asked and k in PRED_GRAD_EXCLUDES:
            return f"{PRED_GRAD_ARG} and {VARIANTS[k].arg} cannot be combined ({PRED_GRAD_LABEL}; {VARIANTS[k].label})"
    if kernel is not None and kernel not in PRED_GRAD_KERNELS:
        return f"{PRED_GRAD_ARG}: not built for kernel {kernel!r}, only for {', '.join(PRED_GRAD_KERNELS)} ({PRED_GRAD_LABEL})"
    return None


def why_refused_pred_hess(asked, dtype: Optional[str], kernel: Optional[str]):
    """As why_refused_pred_grad, for the second derivatives of the posterior mean (pred_hess)."""
    if dtype is not None and dtype != "f64":
        return f"{PRED_HESS_ARG}: built in fp64 only, not in {dtype!r} ({PRED_HESS_LABEL}): pass dtype='f64'"
    if kernel in ("Matern12", "Exponential", "Matern32"):
        return (f"{PRED_HESS_ARG}: kernel {kernel!r} has no second derivatives to return, the derivative of a "
                f"{'Matern-3/2' if kernel == 'Matern32' else 'Matern-1/2'} process is not mean-square differentiable ({PRED_HESS_LABEL})")
    for k in VARIANTS:                                               # table order, whatever the caller's
        if k in asked and k in PRED_HESS_EXCLUDES:
            return f"{PRED_HESS_ARG} and {VARIANTS[k].arg} cannot be combined ({PRED_HESS_LABEL}; {VARIANTS[k].label})"
    if kernel is not None and kernel not in PRED_HESS_KERNELS:
        return f"{PRED_HESS_ARG}: not built for kernel {kernel!r}, only for {', '.join(PRED_HESS_KERNELS)} ({PRED_HESS_LABEL})"
    return None


def pred_hess_pairs(dims):
    """The pairs (a, b), a <= b, of the coordinate indices ``dims``: a ascending, then b -- the columns of f_hess."""
    dims = sorted(set(int(d) for d in dims))
    return [(a, b) for i, a in enumerate(dims) for b in dims[i:]]
