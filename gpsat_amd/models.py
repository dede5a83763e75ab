"""HipGPRModel -- per-tile model class with the reference's BaseGPRModel / GPflowGPRModel interface.

Drop-in hook: the reference selects its backend with ``model_config["oi_model"]``, either a
registry name or ``{"path_to_model": "gpsat_amd.models", "model_name": "HipGPRModel"}``
(GPSat/local_experts.py:319-325).  Every method the orchestrator calls on a model
(GPSat/local_experts.py:1043-1180) exists here with the same name, argument meaning and error
behaviour as GPSat/models/gpflow_models.py:26-663, but the arithmetic runs in the gfx950 HIP
kernels through the C ABI (include/gpsat_hip.h).  There is no CPU fallback.

Differences that are deliberate and documented in DESIGN.md:
  * compute dtype is fp32 on the GPU by default, ``dtype="f64"`` selects the fp64 kernels (host-side scaling /
    constraints are always fp64 like the reference);
  * of the mean functions, ``mean_function="Constant"`` is built (a trainable constant c, GPflow's
    mean_functions.Constant, ``mean_func_kwargs={"c": ...}``; fp64, at most 3 input dimensions, not with
    "RationalQuadratic"): one more parameter, ``mean_constant``, with its getter, setter and constraints, in the model's
    scaled observation units.  Other mean functions and custom likelihoods are not built
    (NotImplementedError);
  * of the likelihoods, a Gaussian one whose variance is a known function of the row is built: ``obs_var`` (an array beside
    ``obs``) or ``obs_var_col`` (a column of ``data``) gives every observation's noise variance in raw observation units,
    added to the diagonal of K beside ``likelihood_variance`` and not trained (fp64; not with "RationalQuadratic",
    ``mean_function="Constant"`` or ``cross_validate``).  ``likelihood=`` itself stays refused;
  * no TensorFlow import, no per-construction device probe (the engine knows its device).
"""
from __future__ import annotations

import platform
import re
import warnings
from typing import Dict, List

import numpy as np

try:  # pandas is optional at import time (arrays may be passed directly)
    import pandas as pd
except Exception:  # pragma: no cover
    pd = None

from . import _lib as L
from . import variants as V

LIKELIHOOD_VARIANCE_LOWER_BOUND = 1e-6   # GPflow Gaussian likelihood default (gpflow_models.py:404-409)

_cpu_name_cache = None


def _processor_name():
    # base_model.py:302-323 (Linux branch), cached: the reference shells out per construction
    global _cpu_name_cache
    if _cpu_name_cache is None:
        name = platform.processor() or "unknown"
        try:
            with open("/proc/cpuinfo") as f:
                for line in f:
                    if "model name" in line:
                        name = re.sub(".*model name.*:", "", line, 1).strip()
                        break
        except OSError:
            pass
        _cpu_name_cache = name
    return _cpu_name_cache


def clamp_within(vals, lo, hi, tol):
    """Pull values to at least ``tol`` inside the box [lo, hi] (the effect of gpflow_models.py:471-479): ``tol`` is
    capped at half the narrowest width; the upper side is applied first.  ``vals`` may carry leading batch axes."""
    margin = min(float(tol), float(np.min(hi - lo)) / 2)
    vals = np.where(vals > hi - margin, hi - margin, vals)
    return np.where(vals < lo + margin, lo + margin, vals)


def _as_name_list(c):
    return [c] if isinstance(c, str) else c


def _as_columns(a):
    a = np.array(a)
    return a[:, None] if a.ndim == 1 else a


def _as_scale_row(s):
    """None -> [[1]]; number -> [[s]]; list -> one row; arrays pass through (base_model.py:212-232)."""
    if s is None:
        return np.ones((1, 1))
    if isinstance(s, (int, float, list)):
        return np.atleast_2d(np.asarray(s, dtype=np.float64))
    return np.asarray(s, dtype=np.float64)


class HipGPRModel:
    """Exact GP regression for one expert tile on MI355X (mirror of GPflowGPRModel)."""

    def __init__(self, data=None, coords_col=None, obs_col=None, coords=None, obs=None,
                 coords_scale=None, obs_scale=None, obs_mean=None, verbose=True, *,
                 kernel="Matern32", kernel_kwargs=None, mean_function=None, mean_func_kwargs=None,
                 noise_variance=None, likelihood=None, engine=None, dtype="f32", obs_var=None, obs_var_col=None, **kwargs):
        # ---- known noise variances per observation: an array beside coords / obs, or a column of data
        if obs_var is not None and obs_var_col is not None:
            raise AssertionError("obs_var and obs_var_col were both provided, give one")
        if obs_var_col is not None:
            if data is None:
                raise AssertionError("obs_var_col names a column of data, but data was not provided")
            if not isinstance(obs_var_col, str):
                raise AssertionError(f"obs_var_col must be one column name, got {obs_var_col!r}")
            obs_var = data.loc[:, obs_var_col].to_numpy()
        # ---- data intake (behaviour of GPSat/models/base_model.py:134-189): a frame + column names, or bare arrays
        if data is not None:
            if coords_col is None or obs_col is None:
                missing = "coord_col" if coords_col is None else "obs_col"
                raise AssertionError(f"data was provided, but {missing} was not")
            coords_col, obs_col = _as_name_list(coords_col), _as_name_list(obs_col)
            raw_coords, raw_obs = data.loc[:, coords_col].to_numpy(), data.loc[:, obs_col].to_numpy()
        else:
            for label, arr in (("obs", obs), ("coords", coords)):
                if arr is None:
                    raise AssertionError(f"data is {data}, and so is {label}: {arr}, provide either")
                if not isinstance(arr, np.ndarray):
                    raise AssertionError(f"if {label} is provided directly it must be an np.array")
            raw_obs, raw_coords = _as_columns(obs), _as_columns(coords)
            if len(raw_obs) != len(raw_coords):
                raise AssertionError("obs and coords lengths don't match ")
            coords_col = list(range(raw_coords.shape[1])) if coords_col is None else coords_col
            obs_col = [0] if obs_col is None else obs_col
        self.coords_col, self.obs_col = coords_col, obs_col
        for label, arr in (("coords", raw_coords), ("obs", raw_obs)):
            if np.isnan(arr).any():
                raise AssertionError(f"nans found in {label}")
        if raw_obs.shape[1] != 1:
            raise AssertionError("HipGPRModel handles a single observation column")

        # ---- de-mean / scale (base_model.py:195-245): only the string "local" selects the column mean, every other
        #      obs_mean (numbers and lists included) means zero; scales become (1, k) rows
        self.obs_mean = raw_obs.mean(axis=0, keepdims=True).astype(np.float64) \
            if (isinstance(obs_mean, str) and obs_mean == "local") else np.zeros((1, 1))
        self.obs_scale = _as_scale_row(obs_scale)
        self.coords_scale = _as_scale_row(coords_scale)
        self.coords = np.array(raw_coords, dtype=np.float64) / self.coords_scale
        self.obs = (np.array(raw_obs, dtype=np.float64) - self.obs_mean) / self.obs_scale
        # variances in raw observation units -> the model's scaled units
        self.obs_var = None
        if obs_var is not None:
            raw_var = np.asarray(obs_var, dtype=np.float64).reshape(-1)
            if len(raw_var) != len(raw_obs):
                raise AssertionError(f"obs_var has {len(raw_var)} entries for {len(raw_obs)} observations")
            if np.isnan(raw_var).any():
                raise AssertionError("nans found in obs_var")
            if not np.isfinite(raw_var).all() or (raw_var < 0).any():
                raise AssertionError("obs_var must be finite and not negative")
            self.obs_var = raw_var / float(self.obs_scale[0, 0]) ** 2

        # ---- kernel / defaults: gpflow_models.py:113-157
        assert kernel is not None, "kernel was not provided"
        if not isinstance(kernel, str) or kernel not in L.KERNEL_IDS:
            raise NotImplementedError(f"kernel {kernel!r}: this backend builds {sorted(L.KERNEL_IDS)}")
        if likelihood is not None:
            raise NotImplementedError("mean_function / custom likelihood are not built in the HIP backend")
        if mean_function is not None and (not isinstance(mean_function, str) or mean_function not in ("Zero", "Constant")):
            raise NotImplementedError(f"mean_function {mean_function!r}: the HIP backend builds None, 'Zero' and 'Constant' "
                                      f"(Linear and the others would need 2 D + 3 > 6 parameters)")
        self.kernel = kernel
        if dtype not in ("f32", "f64"):
            raise ValueError("dtype must be 'f32' or 'f64'")
        self.dtype = dtype                                # device compute precision (the reference computes in fp64)
        D = self.coords.shape[1]
        if D > V.MAX_D:
            raise NotImplementedError(f"HIP backend is built for 1..{V.MAX_D} input dimensions")
        self.D = D
        # the rows of variants.VARIANTS this model asks for: RationalQuadratic's alpha and the constant of a trainable
        # constant mean (gpflow.mean_functions.Constant) are one more parameter each, last in the device's vector
        self._variants = L.theta_variants(kernel, "constant" if mean_function == "Constant" else None) \
            + ["noise"] * (self.obs_var is not None)
        why = V.why_refused(self._variants, dtype, D)
        if why:
            raise NotImplementedError(why)
        if "mean" in self._variants:
            mk = dict(mean_func_kwargs or {})
            if set(mk) - {"c"}:
                raise NotImplementedError(f"mean_func_kwargs {sorted(set(mk) - {'c'})}: 'Constant' takes 'c' only")
            c0 = np.asarray(0.0 if mk.get("c") is None else mk["c"], dtype=np.float64).reshape(-1)   # GPflow: c=None is 0
            assert len(c0) == 1, f"mean_func_kwargs['c'] must be a number or a sequence of one element, got {len(c0)}"
        kk = dict(kernel_kwargs or {})
        ls = np.broadcast_to(np.asarray(kk.get("lengthscales", np.ones(D)), dtype=np.float64), (D,)).copy()
        self._theta = np.concatenate([ls, [float(kk.get("variance", 1.0))],
                                      [1.0 if noise_variance is None else float(noise_variance)],
                                      [float(kk.get("alpha", 1.0))] if "rq" in self._variants else [],        # GPflow: alpha = 1
                                      [float(c0[0])] if "mean" in self._variants else []])
        H = V.n_hyper(D, self._variants)
        self._lo = np.full(H, np.nan)
        self._hi = np.full(H, np.nan)
        self._trainable = np.ones(H, dtype=bool)

        # ---- device info: base_model.py:259 (attributes the orchestrator reads at local_experts.py:1180)
        from .engine import default_engine
        self._engine = engine if engine is not None else default_engine()
        self.gpu_name = self._engine.device_name
        self.cpu_name = _processor_name()
        self.n_eval = 0
        self.status = None

        # base_model.py:270-277
        for pn in self.param_names:
            assert not bool(re.search(" ", pn)), f"param_name: '{pn}' has a space (' ') in it, which is prohibited"
            getattr(self, f"set_{pn}")
            getattr(self, f"get_{pn}")

    # ------------------------------------------------------------------ interface
    @property
    def param_names(self) -> List[str]:
        # the reference's three names (gpflow_models.py:179-184) would lose alpha in params_to_store and load_params
        # ... and likewise the constant of mean_function="Constant"
        return V.param_names(self._variants)

    def get_parameters(self, *args, return_dict=True):
        # base_model.py:370-403
        if len(args) == 0:
            args = self.param_names
        for a in args:
            assert a in self.param_names, f"cannot get parameters for: {a}, it's not in param_names: {self.param_names}"
        if return_dict:
            return {a: getattr(self, f"get_{a}")() for a in args}
        return [getattr(self, f"get_{a}")() for a in args]

    def set_parameters(self, **kwargs):
        # base_model.py:405-422
        for k, v in kwargs.items():
            assert k in self.param_names, f"cannot get parameters for: {k}, it's not in param_names: {self.param_names}"
            getattr(self, f"set_{k}")(v)

    def set_parameter_constraints(self, constraints_dict, **kwargs):
        # base_model.py:424-439
        for k, v in constraints_dict.items():
            assert k in self.param_names, f"cannot get parameters for: {k}, it's not in param_names: {self.param_names}"
            getattr(self, f"set_{k}_constraints")(**v, **kwargs)

    # -- getters / setters: gpflow_models.py:339-411
    def get_lengthscales(self) -> np.ndarray:
        return self._theta[self._slice("lengthscales")].copy()

    def get_kernel_variance(self) -> float:
        return float(self._theta[self._column("kernel_variance")])

    def get_likelihood_variance(self) -> float:
        return float(self._theta[self._column("likelihood_variance")])

    def _column(self, name):
        """The first column of theta with the parameter ``name``; AttributeError for a variant's parameter in a model without
        that variant."""
        if name not in self.param_names:
            row = next(v for v in V.VARIANTS.values() if v.param == name)
            raise AttributeError(f"{name} is the parameter of {row.label}, which this model (kernel {self.kernel!r}) does not have")
        return self._slice(name).start

    def _set_variant_param(self, name, value):
        col = self._column(name)
        v = np.asarray(value, dtype=np.float64).reshape(-1)
        assert len(v) == 1, f"set_{name} expected a float or an array of one element, got {len(v)}"
        self._theta[col] = float(v[0])

    def get_mean_constant(self) -> float:
        """c of the constant mean, in the model's scaled observation units, (y - obs_mean) / obs_scale."""
        return float(self._theta[self._column("mean_constant")])

    def set_mean_constant(self, mean_constant):
        self._column("mean_constant")
        assert np.isfinite(np.asarray(mean_constant, dtype=np.float64)).all(), "mean_constant must be finite"
        self._set_variant_param("mean_constant", mean_constant)

    def get_kernel_alpha(self) -> float:
        return float(self._theta[self._column("kernel_alpha")])

    def set_kernel_alpha(self, kernel_alpha):
        self._set_variant_param("kernel_alpha", kernel_alpha)

    def set_lengthscales(self, lengthscales):
        v = np.asarray(lengthscales, dtype=np.float64).reshape(-1)
        assert len(v) in (1, self.D), f"lengthscales must have length 1 or {self.D}"
        self._theta[self._slice("lengthscales")] = v

    def set_kernel_variance(self, kernel_variance):
        if isinstance(kernel_variance, np.ndarray):
            assert (len(kernel_variance) == 1) & (len(kernel_variance.shape) == 1), \
                f"set_kernel_variance expected to receive float, or np.array with len(1), shape:(1,), got" \
                f"len: {len(kernel_variance)}, shape: {kernel_variance.shape}"
            kernel_variance = kernel_variance[0]
        self._theta[self._column("kernel_variance")] = float(kernel_variance)

    def set_likelihood_variance(self, likelihood_variance):
        if isinstance(likelihood_variance, np.ndarray):
            assert (len(likelihood_variance) == 1) & (len(likelihood_variance.shape) == 1), \
                f"set_likelihood_variance expected to receive float, or np.array with len(1), shape:(1,), got" \
                f"len: {len(likelihood_variance)}, shape: {likelihood_variance.shape}"
            likelihood_variance = likelihood_variance[0]
        unconstrained = not np.isfinite(self._lo[self._column("likelihood_variance")])
        if unconstrained and likelihood_variance < LIKELIHOOD_VARIANCE_LOWER_BOUND:
            warnings.warn("\n***\ntrying to set likelihood_variance to value less than "
                          "model.likelihood.variance_lower_bound\nwill set to variance_lower_bound\n***\n")
            likelihood_variance = LIKELIHOOD_VARIANCE_LOWER_BOUND
        self._theta[self._column("likelihood_variance")] = float(likelihood_variance)

    # -- constraints: gpflow_models.py:416-590
    def _slice(self, name):
        start, width = V.slots(self.D, self._variants)[name]
        return slice(start, start + width)

    def _set_param_constraints(self, name, low, high, move_within_tol=True, tol=1e-8, scale=False,
                               scale_magnitude=None):
        """Box for one named parameter (behaviour of gpflow_models.py:416-494): bounds optionally divided by the
        coordinate scale, the current value pulled to at least ``tol`` inside the box; the sigmoid bijector itself
        runs on the GPU (lo / hi of the C ABI)."""
        sl = self._slice(name)
        n = sl.stop - sl.start
        bounds = []
        for label, b in (("low", low), ("high", high)):
            b = np.atleast_1d(np.asarray(b, dtype=np.float64))
            if b.ndim != 1:
                raise AssertionError(f"{label} constraint must be a scalar or 1-d")
            if len(b) != n:
                raise AssertionError(f"len of {label} constraint does not match param length")
            bounds.append(b)
        lo, hi = bounds
        if not np.all(lo <= hi):
            raise AssertionError("all values in high constraint must be greater than low")
        if scale:
            div = self.coords_scale[0, :] if scale_magnitude is None else scale_magnitude
            lo, hi = lo / div, hi / div
        cur = self._theta[sl]
        if move_within_tol:
            cur = clamp_within(cur, lo, hi, tol)
        self._theta[sl], self._lo[sl], self._hi[sl] = cur, lo, hi

    def set_lengthscales_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        self._set_param_constraints("lengthscales", low, high, move_within_tol, tol, scale, scale_magnitude)

    def set_kernel_variance_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        self._set_param_constraints("kernel_variance", low, high, move_within_tol, tol, scale, scale_magnitude)

    def set_likelihood_variance_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        self._set_param_constraints("likelihood_variance", low, high, move_within_tol, tol, scale, scale_magnitude)

    def set_kernel_alpha_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        self._column("kernel_alpha")
        self._set_param_constraints("kernel_alpha", low, high, move_within_tol, tol, scale, scale_magnitude)

    def set_mean_constant_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        """A box for c (without one it is unconstrained, as GPflow's Constant.c).  ``scale`` divides bounds by the COORDINATE
        scale, which means nothing for a level of the observations: refused."""
        self._column("mean_constant")
        if scale:
            raise NotImplementedError("set_mean_constant_constraints: scale=True divides by the coordinate scale, which "
                                      "does not apply to mean_constant; give the bounds in scaled observation units")
        self._set_param_constraints("mean_constant", low, high, move_within_tol, tol, False, None)

    # -- the three device calls
    def _tile_args(self, pred_coords=None) -> dict:
        """The engine arguments of this model's one tile: offsets, X, y, the prediction coordinates, theta0, the box, the
        trainable mask, the kernel and what the model's variants add."""
        N, D = self.coords.shape
        Xs = np.zeros((0, D)) if pred_coords is None else pred_coords
        return dict(D=D, obs_off=np.array([0, N]), X=self.coords, y=self.obs[:, 0], pred_off=np.array([0, len(Xs)]), Xs=Xs,
                    theta0=self._theta[None, :], lo=self._lo[None, :], hi=self._hi[None, :], trainable=self._trainable,
                    kernel=self.kernel, **self._variant_args())

    def _variant_args(self) -> dict:
        """The engine keywords that this model's variants add to a call."""
        kw = {"mean": "constant"} if "mean" in self._variants else {}
        if self.obs_var is not None:
            kw["obs_var"] = self.obs_var
        return kw

    def _run(self, *, optimiser, max_iter=0, pred_coords=None, **opt_kwargs):
        return self._engine.fit_predict_batch(dtype=self.dtype, optimiser=optimiser, max_iter=max_iter,
                                              **self._tile_args(pred_coords), **opt_kwargs)

    def _fix_hyperparameters(self, params_list):
        # gpflow_models.py:275-288
        for param in params_list:
            if param in self.param_names:
                self._trainable[self._slice(param)] = False
            else:
                print(f"{param} is not detected as a hyperparameter. Skipping...")

    def optimise_parameters(self, max_iter=10_000, fixed_params=None, **opt_kwargs):
        """L-BFGS on the unconstrained parameters, entirely on the GPU
        (replaces gpflow.optimizers.Scipy().minimize, gpflow_models.py:291-329).
        Returns True when the optimiser converged within ``max_iter`` (scipy ``success``)."""
        if fixed_params is None:
            fixed_params = []
        self._fix_hyperparameters(fixed_params)
        optimiser = opt_kwargs.pop("optimiser", "lbfgs")
        # engine tolerances may be passed through; SciPy-specific keys of the reference are ignored
        known = {k: opt_kwargs[k] for k in ("max_ls", "ftol", "gtol", "adam_lr") if k in opt_kwargs}
        r = self._run(optimiser=optimiser, max_iter=max_iter, **known)
        self.status = int(r.status[0])
        self.n_eval = int(r.n_eval[0])
        if self.status in (0, 1, 6):
            self._theta = r.theta[0].copy()
        success = self.status == 0
        if not success:
            print("*" * 10)
            print("optimization failed!")
        return success

    def get_objective_function_value(self):
        """Negative log marginal likelihood at the current parameters (gpflow_models.py:334-337)."""
        r = self._run(optimiser="none")
        return float(r.nll[0])

    def _why_no_gradient(self, full_cov=False):
        """Why predict(gradient=True) is refused for this model (variants.why_refused_pred_grad), or None."""
        return V.why_refused_pred_grad(self._variants + ["full_cov"] * bool(full_cov), self.dtype, self.kernel)

    def _why_no_hessian(self, full_cov=False):
        """Why predict(hessian=...) is refused for this model (variants.why_refused_pred_hess), or None."""
        return V.why_refused_pred_hess(self._variants + ["full_cov"] * bool(full_cov), self.dtype, self.kernel)

    def predict(self, coords, full_cov=False, apply_scale=True, gradient=False, hessian=False) -> Dict[str, np.ndarray]:
        """gpflow_models.py:187-273.  ``gradient=True`` (fp64; RBF, Matern32, Matern52): also the 1-D arrays
        ``f*_grad_<k>`` and ``f*_grad_var_<k>``, k = 0 .. D - 1 -- the derivative of the posterior mean with respect to
        coordinate k of the prediction point, and the posterior variance of that derivative.  With ``apply_scale`` they are in
        raw units, observation units per unit of the raw coordinate: obs_scale g_k / coords_scale_k and obs_scale^2 v_k /
        coords_scale_k^2; without it they are the scaled model's, as the coordinates given are.
        ``hessian=True`` or a list of coordinate indices (fp64; RBF, Matern52), alone or beside ``gradient``:
        also ``f*_hess_<a>_<b>`` and ``f*_hess_var_<a>_<b>`` for the pairs a <= b of those coordinates -- the second derivative
        of the posterior mean and its posterior variance -- and ``f*_lap`` / ``f*_lap_var``, the sum of the ``f*_hess_<a>_<a>``
        and its variance, which holds their covariances.  With ``apply_scale`` in raw units: obs_scale H_ab / (coords_scale_a
        coords_scale_b), the Laplacian weighted with 1 / coords_scale_a^2 so that it is the Laplacian in raw coordinates, and
        the variances with the squares; without it the scaled model's."""
        if hessian is not False and hessian is not None:
            why = self._why_no_hessian(full_cov)
            if why:
                raise NotImplementedError(why)
            hdims = list(range(self.D)) if hessian is True else sorted(set(int(a) for a in hessian))
            if not hdims or hdims[0] < 0 or hdims[-1] >= self.D:
                raise ValueError(f"hessian: True, or coordinate indices in 0..{self.D - 1}, got {hessian!r}")
        else:
            hdims = None
        if gradient and hdims is None:
            why = self._why_no_gradient(full_cov)
            if why:
                raise NotImplementedError(why)
        if pd is not None and isinstance(coords, (pd.Series, pd.DataFrame)):
            if self.coords_col is not None:
                coords = coords[self.coords_col].values
            else:
                coords = coords.values
        if isinstance(coords, list):
            coords = np.array(coords)
        if len(coords.shape) == 1:
            coords = coords[None, :]
        assert isinstance(coords, np.ndarray), "coords should be an ndarray (one can be converted from)"
        coords = coords.astype(self.coords.dtype)
        if apply_scale:
            coords = coords / self.coords_scale
        cs = np.broadcast_to(self.coords_scale, (1, self.D))[0] if apply_scale else np.ones(self.D)
        extra = {"pred_grad": True} if gradient else {}
        if hdims is not None:
            extra["pred_hess"] = {"dims": hdims, "lap_weight": [1.0 / cs[a] ** 2 if a in hdims else 0.0 for a in range(self.D)]}
        r = self._run(optimiser="none", pred_coords=coords, **(extra or {"full_cov": bool(full_cov)}))
        if r.status[0] in (2, 3):
            raise FloatingPointError("covariance matrix is not positive definite at the current parameters")
        if not full_cov:
            out = {"f*": r.f_mean.astype(np.float64), "f*_var": r.f_var.astype(np.float64),
                   "y_var": r.y_var.astype(np.float64)}
        else:
            # gpflow_models.py:245-263: marginal variance = diagonal of the full covariance; the predictive
            # covariance adds the likelihood variance on the diagonal
            P = len(coords)
            f_cov = np.asarray(r.f_cov, dtype=np.float64).reshape(P, P)
            f_var = np.diag(f_cov).copy()
            y_var = r.y_var.astype(np.float64)
            y_cov = f_cov.copy()
            y_cov[np.arange(P), np.arange(P)] += y_var - f_var
            out = {"f*": r.f_mean.astype(np.float64), "f*_var": f_var, "y_var": y_var, "f*_cov": f_cov, "y_cov": y_cov}
        osc = float(self.obs_scale[0, 0]) if apply_scale else 1.0
        if gradient:
            fg, fgv = np.asarray(r.f_grad, dtype=np.float64), np.asarray(r.f_grad_var, dtype=np.float64)
            for k in range(self.D):
                out[f"f*_grad_{k}"] = osc * fg[:, k] / cs[k]
                out[f"f*_grad_var_{k}"] = osc ** 2 * fgv[:, k] / cs[k] ** 2
        if hdims is not None:
            fh, fhv = np.asarray(r.f_hess, dtype=np.float64), np.asarray(r.f_hess_var, dtype=np.float64)
            for k, (a, b) in enumerate(r.hess_pairs):
                out[f"f*_hess_{a}_{b}"] = osc * fh[:, k] / (cs[a] * cs[b])
                out[f"f*_hess_var_{a}_{b}"] = osc ** 2 * fhv[:, k] / (cs[a] * cs[b]) ** 2
            out["f*_lap"] = osc * np.asarray(r.f_lap, dtype=np.float64)
            out["f*_lap_var"] = osc ** 2 * np.asarray(r.f_lap_var, dtype=np.float64)
        f_bar = self.obs_mean[:, 0]
        if len(f_bar) != len(out["f*"]):
            assert len(f_bar) == 1, f"'f_bar' did not match the length of 'f*' and f_bar len is not, got: {len(f_bar)}"
            out["f_bar"] = np.repeat(f_bar, len(out["f*"]))
        else:
            out["f_bar"] = f_bar
        return out

    def cross_validate(self, fold=None, apply_scale=True, refit=False, joint=False, **refit_kwargs) -> Dict[str, np.ndarray]:
        """Held-out predictions.  ``refit=False``: at the model's current parameters (no optimisation, nothing is fitted
        again without the fold; for that see ``refit`` below): every row predicted from the rows of all OTHER folds, from the tile's own factor (gpsat_fit_predict_batch_cv).
        ``fold``: None = leave-one-out; an array-like of N labels of any hashable kind, or a 2-D array whose equal rows form
        a fold; integer labels < 0 and None / NaN labels are never held out (NaN results).  Returns "f*", "f*_var" and
        "y_var", each [N] in the order of the model's rows, in the units ``predict`` returns its own (with "f_bar", the
        tile's own de-meaning constant: it is not recomputed per fold).  Always computed in fp64, whatever ``dtype``.
        ``apply_scale`` is accepted for symmetry with ``predict``: the model's coordinates are already scaled.
        ``refit=True``: every fold is fitted again without its rows (gpsat_fit_predict_batch_cv_refit), in the model's
        ``dtype``, from the model's current parameters ("start": "theta0") or from the tile's fitted ones ("full"); the
        model itself is not changed.  ``refit_kwargs``: ``start``, ``recentre``, ``min_obs``, ``max_expanded_rows`` as
        Engine.fit_predict_batch takes them in ``cv_refit``, and ``max_iter`` / ``optimiser`` / ``max_ls`` / ``ftol`` /
        ``gtol`` as ``optimise_parameters`` does.  "f*" is in the units of the tile's own "f_bar"; the result also holds,
        per fold in ascending order of the factorised label, "fold" (the code of factorise_folds), "theta" [F, H],
        "objective_value", "status", "num_obs" and "shift" (the mean of the rows the fold leaves, in the units of "f*").
        ``joint=True`` (either flavour; with ``refit`` fp64 only): also, per fold in ascending order of the factorised label
        (leave-one-out: per row), "fold" (the label's code), "fold_size" (its rows) and "lpd", the joint log predictive
        density log N(y_G; mean, covariance of the held-out fold) in the units of "f*" (Engine.fit_predict_batch
        ``cv_joint``); NaN where the fold's rows are NaN.  Without ``joint`` the result has exactly the keys above."""
        from .engine import factorise_folds
        N, D = self.coords.shape
        why = V.why_refused(self._variants + ["cv_refit" if refit else "cv"], None, None)
        if why:
            raise NotImplementedError(why)
        if refit:
            return self._cross_validate_refit(fold, joint=joint, **refit_kwargs)
        if refit_kwargs:
            raise TypeError(f"cross_validate: {sorted(refit_kwargs)} are options of refit=True")
        nmax = L.max_tile_obs("f64", D)
        if N > nmax:
            raise ValueError(f"tile of {N} observations: held-out predictions take at most {nmax} (gpsat_max_tile_obs, fp64, D={D})")
        labels = "loo"
        if fold is not None:
            labels = factorise_folds(fold, N)
            gmax = L.max_cv_fold("f64", D)
            counts = np.bincount(labels[labels >= 0]) if (labels >= 0).any() else np.zeros(1, dtype=int)
            if counts.max() > gmax:
                raise ValueError(f"a fold of {int(counts.max())} rows: at most {gmax} rows are held out together (gpsat_max_cv_fold)")
        more = {"cv_joint": True} if joint else {}
        r = self._engine.fit_predict_batch(dtype="f64", optimiser="none", max_iter=0, cv_fold=labels, **self._tile_args(), **more)
        if r.status[0] in (2, 3):
            raise FloatingPointError("covariance matrix is not positive definite at the current parameters")
        out = {"f*": np.asarray(r.cv_mean, dtype=np.float64), "f*_var": np.asarray(r.cv_f_var, dtype=np.float64),
               "y_var": np.asarray(r.cv_y_var, dtype=np.float64), "f_bar": np.repeat(self.obs_mean[:, 0], N)}
        if joint:
            out.update(self._joint_folds(np.arange(N, dtype=np.int32) if fold is None else labels, r.cv_lpd))
        return out

    @staticmethod
    def _joint_folds(labels, lpd):
        """The per-fold arrays of ``joint=True``: folds in ascending code, as the engine numbers them."""
        from .local_cv import fold_layout
        lay = fold_layout(labels)
        if len(lay.codes) != len(lpd):
            from .engine import GpsatError
            raise GpsatError(f"cross_validate(joint=True): {len(lay.codes)} folds counted here, {len(lpd)} by the engine")
        return {"fold": lay.codes.astype(np.int32), "fold_size": lay.size, "lpd": np.asarray(lpd, dtype=np.float64)}


    def _cross_validate_refit(self, fold, max_iter=10_000, optimiser="lbfgs", joint=False, **kw):
        from .engine import factorise_folds
        N = len(self.coords)
        labels = np.arange(N, dtype=np.int32) if fold is None else factorise_folds(fold, N)
        run = {k: kw.pop(k) for k in ("max_ls", "ftol", "gtol", "adam_lr") if k in kw}
        r = self._engine.fit_predict_batch(dtype=self.dtype, optimiser=optimiser, max_iter=max_iter, cv_fold=labels,
                                           cv_refit=kw or True, **self._tile_args(), **run, **({"cv_joint": True} if joint else {}))
        out = {"f*": np.asarray(r.cv_mean, dtype=np.float64), "f*_var": np.asarray(r.cv_f_var, dtype=np.float64),
               "y_var": np.asarray(r.cv_y_var, dtype=np.float64), "f_bar": np.repeat(self.obs_mean[:, 0], N),
               "fold": r.cv_label, "theta": r.cv_theta, "objective_value": r.cv_nll, "status": r.cv_status,
               "num_obs": r.cv_n_obs, "shift": r.cv_shift}
        if joint:
            jf = self._joint_folds(labels, r.cv_lpd)
            if not np.array_equal(jf["fold"], out["fold"]):
                from .engine import GpsatError
                raise GpsatError(f"cross_validate(joint=True): folds {jf['fold'].tolist()} counted here, "
                                 f"{np.asarray(out['fold']).tolist()} by the engine")
            out.update(fold_size=jf["fold_size"], lpd=jf["lpd"])
        return out


def select_inducing_points(coords: np.ndarray, num_inducing_points: int, seed: int = 0, expert_index: int = 0) -> np.ndarray:
    """Inducing points of one expert (GPflowSGPRModel.__init__, gpflow_models.py:836-847, made reproducible): all the
    coordinates when there are at most ``num_inducing_points`` of them, else a random subset of that many rows drawn
    with ``np.random.default_rng([seed, expert_index])`` (the reference shuffles with the unseeded global generator).
    The batched orchestrator and the per-tile model pick the same rows."""
    assert num_inducing_points is not None, "num_inducing_points is None, must be specified for SGPR"
    coords = np.asarray(coords, dtype=np.float64)
    M = int(num_inducing_points)
    if M < 1:
        raise ValueError("num_inducing_points must be at least 1")
    if len(coords) <= M:
        return coords.copy()
    rows = np.random.default_rng([int(seed), int(expert_index)]).permutation(len(coords))[:M]
    return coords[rows].copy()


class HipSGPRModel(HipGPRModel):
    """Sparse GP regression (SGPR, the collapsed Titsias bound) for one expert tile on MI355X, with fixed inducing points
    (mirror of GPflowSGPRModel, gpflow_models.py:666-901).  For tiles larger than the exact path takes
    (gpsat_max_tile_obs): cost O(N M^2) per evaluation, no limit on N.  fp64 only."""

    def __init__(self, data=None, coords_col=None, obs_col=None, coords=None, obs=None,
                 coords_scale=None, obs_scale=None, obs_mean=None, verbose=True, *,
                 kernel="Matern32", num_inducing_points=500, kernel_kwargs=None, mean_function=None,
                 mean_func_kwargs=None, noise_variance=None, likelihood=None, engine=None, dtype="f64",
                 inducing_seed=0, expert_index=0, obs_var=None, obs_var_col=None, **kwargs):
        why = V.why_refused(["sgpr"] + ["noise"] * (obs_var is not None or obs_var_col is not None)
                            + ["rq"] * (kernel == "RationalQuadratic"), dtype, None)
        if why:
            raise NotImplementedError(why)
        if mean_function is not None:
            raise NotImplementedError("mean_function is not built for sparse experts (HipSGPRModel)")
        super().__init__(data=data, coords_col=coords_col, obs_col=obs_col, coords=coords, obs=obs,
                         coords_scale=coords_scale, obs_scale=obs_scale, obs_mean=obs_mean, verbose=verbose,
                         kernel=kernel, kernel_kwargs=kernel_kwargs, mean_function=mean_function,
                         mean_func_kwargs=mean_func_kwargs, noise_variance=noise_variance, likelihood=likelihood,
                         engine=engine, dtype="f64", **kwargs)
        self.num_inducing_points = int(num_inducing_points)
        if self.num_inducing_points > L.max_inducing("f64", self.D):
            raise ValueError(f"num_inducing_points={num_inducing_points}: at most {L.max_inducing('f64', self.D)} "
                             f"are built (gpsat_max_inducing)")
        self.inducing_points = select_inducing_points(self.coords, self.num_inducing_points, inducing_seed, expert_index)

    @property
    def param_names(self) -> List[str]:
        return ["lengthscales", "kernel_variance", "likelihood_variance", "inducing_points"]

    def cross_validate(self, fold=None, apply_scale=True, **kwargs):
        raise NotImplementedError(V.why_refused(["sgpr", "cv"], None, None))

    def get_inducing_points(self) -> np.ndarray:
        """Inducing points [M, D] in the model's (scaled) coordinates."""
        return self.inducing_points.copy()

    def set_inducing_points(self, inducing_points):
        Z = np.atleast_2d(np.asarray(inducing_points, dtype=np.float64))
        if Z.shape[1] != self.D:
            raise AssertionError(f"inducing_points must have shape [M, {self.D}]")
        if not 1 <= len(Z) <= L.max_inducing("f64", self.D):
            raise ValueError(f"1..{L.max_inducing('f64', self.D)} inducing points are built")
        self.inducing_points = Z.copy()

    def set_inducing_points_constraints(self, *args, **kwargs):
        raise NotImplementedError("inducing points are fixed in the HIP backend (no constraints)")

    def _run(self, *, optimiser, max_iter=0, pred_coords=None, full_cov=False, **opt_kwargs):
        if full_cov:
            raise NotImplementedError("HipSGPRModel.predict(full_cov=True) is not built")
        Z = self.inducing_points
        return self._engine.sgpr_fit_predict_batch(z_off=np.array([0, len(Z)]), Z=Z, optimiser=optimiser, max_iter=max_iter,
                                                   **self._tile_args(pred_coords), **opt_kwargs)

    def optimise_parameters(self, train_inducing_points=False, max_iter=10_000, fixed_params=None, **opt_kwargs):
        """L-BFGS on the three hyper-parameters with Z fixed (gpflow_models.py:865-901)."""
        if train_inducing_points:
            raise NotImplementedError("train_inducing_points=True is not built: the inducing points stay fixed")
        return super().optimise_parameters(max_iter=max_iter, fixed_params=fixed_params, **opt_kwargs)

    def get_objective_function_value(self):
        """The ELBO at the current parameters (gpflow_models.py:860-862) -- not its negative."""
        r = self._run(optimiser="none")
        return -float(r.nll[0])

    def predict(self, coords, full_cov=False, apply_scale=True, gradient=False, hessian=False) -> Dict[str, np.ndarray]:
        if full_cov:
            raise NotImplementedError("HipSGPRModel.predict(full_cov=True) is not built")
        if gradient:
            raise NotImplementedError(V.why_refused_pred_grad(["sgpr"], None, None))
        if hessian is not False and hessian is not None:
            raise NotImplementedError(V.why_refused_pred_hess(["sgpr"], None, None))
        return super().predict(coords, full_cov=False, apply_scale=apply_scale)


SGPR_MODEL_NAMES = ("HipSGPRModel", "GPflowSGPRModel")


SKLEARN_MODEL_NAMES = ("HipSklearnGPRModel", "sklearnGPRModel")
SKLEARN_NU = {0.5: "Matern12", 1.5: "Matern32", 2.5: "Matern52", np.inf: "RBF"}
SKLEARN_BOUNDS = (1e-5, 1e5)              # sklearn's default hyperparameter bounds (length_scale, constant_value)


def sklearn_restart_starts(rng, log_lo, log_hi, n_restarts):
    """The further starts of sklearn's GaussianProcessRegressor.fit: ``n_restarts`` draws of
    ``rng.uniform(log_lo, log_hi)`` over the trainable hyperparameters (sklearn's order), returned in log space [n, k]."""
    return np.array([rng.uniform(log_lo, log_hi) for _ in range(int(n_restarts))]).reshape(int(n_restarts), len(log_lo))


class HipSklearnGPRModel(HipGPRModel):
    """Exact GP regression for one expert tile with the interface and behaviour of the reference's sklearnGPRModel
    (GPSat/models/sklearn_models.py): sklearn's GaussianProcessRegressor(kernel * ConstantKernel(sqrt(kernel_variance)),
    alpha=likelihood_variance, n_restarts_optimizer) fitted by multi-start bounded L-BFGS-B in log space on the GPU
    (gpsat_fit_predict_batch_ms).  fp64 by default, as sklearn."""

    def __init__(self, data=None, coords_col=None, obs_col=None, coords=None, obs=None,
                 coords_scale=None, obs_scale=None, obs_mean=None, verbose=True, *,
                 kernel="Matern", kernel_kwargs=None, mean_value=None, kernel_variance=1., likelihood_variance=None,
                 param_bounds=None, n_restarts_optimizer=2, random_state=None, engine=None, dtype="f64",
                 obs_var=None, obs_var_col=None, **kwargs):
        if obs_var is not None or obs_var_col is not None:
            raise NotImplementedError(V.why_refused(["multistart", "noise"], None, None))
        kk = dict(kernel_kwargs or {})
        if kernel == "Matern":
            nu = float(kk.pop("nu", 1.5))
            if nu not in SKLEARN_NU:
                raise NotImplementedError(f"Matern nu={nu}: this backend builds nu in {sorted(SKLEARN_NU)}")
            dev_kernel = SKLEARN_NU[nu]
        elif kernel == "RBF":
            dev_kernel = "RBF"
        else:
            raise NotImplementedError(f"kernel {kernel!r}: the sklearn model builds 'Matern' and 'RBF'")
        if mean_value is not None:
            raise NotImplementedError("mean_value (a trainable ConstantKernel summand) is not built")
        ls = kk.pop("length_scale", None)
        ls_bounds = kk.pop("length_scale_bounds", SKLEARN_BOUNDS)
        if kk:
            raise NotImplementedError(f"kernel_kwargs {sorted(kk)} are not built")
        super().__init__(data=data, coords_col=coords_col, obs_col=obs_col, coords=coords, obs=obs,
                         coords_scale=coords_scale, obs_scale=obs_scale, obs_mean=obs_mean, verbose=verbose,
                         kernel=dev_kernel, engine=engine, dtype=dtype)
        D = self.D
        if ls is None:
            ls = np.ones(D)
        ls = np.asarray(ls, dtype=np.float64)
        if ls.ndim != 1 or len(ls) != D:
            raise NotImplementedError("an isotropic (scalar) length_scale is not built: give one per dimension")
        # amplitude quirk of the reference: kernel * ConstantKernel(sqrt(kernel_variance)) -- the device sees sf2 = c
        self._has_constant = kernel_variance is not None
        c = float(np.sqrt(kernel_variance)) if self._has_constant else 1.0
        alpha = 1.0 if likelihood_variance is None else float(likelihood_variance)
        self._theta = np.concatenate([ls, [c], [alpha]])
        lsb = np.broadcast_to(np.asarray(ls_bounds, dtype=np.float64), (D, 2)) if np.ndim(ls_bounds) == 2 else \
            np.broadcast_to(np.asarray(ls_bounds, dtype=np.float64), (2,))[None, :].repeat(D, 0)
        self._lo = np.concatenate([lsb[:, 0], [SKLEARN_BOUNDS[0]], [np.nan]])
        self._hi = np.concatenate([lsb[:, 1], [SKLEARN_BOUNDS[1]], [np.nan]])
        self._trainable = np.array([True] * D + [self._has_constant, False])
        if param_bounds is not None:
            # the reference assigns to a Hyperparameter namedtuple field
            raise AttributeError("can't set attribute")
        self.n_restarts_optimizer = int(n_restarts_optimizer)
        self.random_state = random_state
        self._lml = None                   # +LML of the last fit (sklearn's log_marginal_likelihood_value_)
        self.f_start = None

    # -- getters / setters (sklearn_models.py:186-240)
    def get_kernel_variance(self) -> float:
        return float(self._theta[self._column("kernel_variance")]) ** 2 if self._has_constant else 1.0

    def set_kernel_variance(self, kernel_variance):
        if self._has_constant:
            self._theta[self._column("kernel_variance")] = float(np.sqrt(np.asarray(kernel_variance, dtype=np.float64).reshape(-1)[0]))

    def set_likelihood_variance(self, likelihood_variance):
        self._theta[self._column("likelihood_variance")] = float(np.asarray(likelihood_variance, dtype=np.float64).reshape(-1)[0])

    def set_lengthscales(self, lengthscales):
        v = np.asarray(lengthscales, dtype=np.float64).reshape(-1)
        assert len(v) == self.D, f"lengthscales must have length {self.D}"
        self._theta[self._slice("lengthscales")] = v

    # -- constraints (sklearn_models.py:282-360): only the length-scale bounds reach the kernel
    def set_lengthscales_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        lo = np.atleast_1d(np.asarray(low, dtype=np.float64))
        hi = np.atleast_1d(np.asarray(high, dtype=np.float64))
        assert len(lo) == self.D, "len of low constraint does not match size of parameter lengthscales"
        assert len(hi) == self.D, "len of high constraint does not match size of parameter lengthscales"
        assert np.all(lo <= hi), "all values in high constraint must be greater than low"
        if scale:
            div = self.coords_scale[0, :] if scale_magnitude is None else scale_magnitude
            lo, hi = lo / div, hi / div
        # move_within_tol edits a copy in the reference: the current values stay
        ls = self._slice("lengthscales")
        self._lo[ls], self._hi[ls] = lo, hi

    def set_kernel_variance_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        """No effect, as in the reference: it sets an attribute of the Product kernel that sklearn never reads."""

    def set_likelihood_variance_constraints(self, low, high, move_within_tol=True, tol=1e-8, scale=False, scale_magnitude=None):
        """No effect: alpha is fixed, never trained."""

    # -- fit / objective / predict
    def cross_validate(self, fold=None, apply_scale=True, **kwargs):
        raise NotImplementedError(V.why_refused(["multistart", "cv"], None, None))

    def restart_starts(self, rng=None):
        """The n_restarts_optimizer further starts, constrained space [n, D + 2], drawn as sklearn draws them from
        ``check_random_state(random_state)`` (or ``rng``)."""
        from sklearn.utils import check_random_state
        rng = check_random_state(self.random_state) if rng is None else rng
        tr = self._trainable
        log_lo, log_hi = np.log(self._lo[tr]), np.log(self._hi[tr])
        draws = sklearn_restart_starts(rng, log_lo, log_hi, self.n_restarts_optimizer)
        out = np.repeat(self._theta[None, :], self.n_restarts_optimizer, axis=0)
        out[:, tr] = np.exp(draws)
        return out

    def _run(self, *, optimiser, max_iter=0, pred_coords=None, starts=None, **opt_kwargs):
        S = 1 if starts is None else 1 + len(starts)
        return self._engine.fit_predict_batch(dtype=self.dtype, optimiser=optimiser, max_iter=max_iter, n_starts=S, starts=starts,
                                              **self._tile_args(pred_coords), **opt_kwargs)

    def optimise_parameters(self, opt=None, **kwargs):
        """sklearn's fit: L-BFGS-B from the current parameters and from n_restarts_optimizer random starts, the best
        optimum kept.  ``max_iter`` and ``fixed_params`` are ignored, as by the reference.  True unless the fit failed."""
        if self.n_restarts_optimizer > 0 and not (np.isfinite(self._lo[self._trainable]).all()
                                                  and np.isfinite(self._hi[self._trainable]).all()):
            raise ValueError("Multiple optimizer restarts (n_restarts_optimizer>0) requires that all bounds are finite.")
        starts = self.restart_starts() if self.n_restarts_optimizer > 0 else None
        # SciPy's L-BFGS-B defaults: maxiter 15000, maxls 20, ftol = factr * eps, pgtol 1e-5
        r = self._run(optimiser="lbfgs", max_iter=15000, starts=starts)
        self.status = int(r.status[0])
        self.n_eval = int(r.n_eval[0])
        self.f_start = r.f_start[0].copy()
        if self.status in (2, 3):
            print("*" * 10)
            print("optimization failed!")
            return False
        self._theta = r.theta[0].copy()
        self._lml = -float(r.nll[0])
        return True

    def get_objective_function_value(self):
        """+LML after a fit (sklearn's log_marginal_likelihood_value_); without one -LML at the current parameters
        (the reference's _fake_fit branch)."""
        if self._lml is not None:
            return self._lml
        r = self._run(optimiser="none")
        return float(r.nll[0])

    def predict(self, coords, full_cov=False, apply_scale=True, gradient=False, hessian=False) -> Dict[str, np.ndarray]:
        """f* and the latent variance f*_var (clipped at 0) as sklearn returns them: no y_var, no f_bar, no rescale by
        obs_scale (sklearn_models.py:116-178); ``full_cov`` adds f*_cov."""
        if gradient:
            raise NotImplementedError(V.why_refused_pred_grad(["multistart"], None, None))
        if hessian is not False and hessian is not None:
            raise NotImplementedError(V.why_refused_pred_hess(["multistart"], None, None))
        out = super().predict(coords, full_cov=full_cov, apply_scale=apply_scale)
        res = {"f*": np.atleast_1d(out["f*"]), "f*_var": np.maximum(np.atleast_1d(out["f*_var"]), 0.0)}
        if full_cov:
            res["f*_cov"] = out["f*_cov"]
        return res


def get_model(name):
    """Registry hook with the reference's semantics (GPSat/models/__init__.py:3-28): the exact-GP names resolve to
    HipGPRModel, the sparse ones to HipSGPRModel, the sklearn ones to HipSklearnGPRModel; anything else is
    NotImplementedError."""
    if name in ("HipGPRModel", "GPflowGPRModel"):
        return HipGPRModel
    if name in SGPR_MODEL_NAMES:
        return HipSGPRModel
    if name in SKLEARN_MODEL_NAMES:
        return HipSklearnGPRModel
    raise NotImplementedError(f"model with name: '{name}' is not implemented")
