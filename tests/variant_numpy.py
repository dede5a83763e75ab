"""fp64 NumPy / SciPy restatement of an exact-GP tile for the variants of the fp64 expert (test infrastructure, like
sgpr_numpy.py): objective, analytic gradient, predictions, full covariance, a SciPy L-BFGS-B fit in u-space with
oracle.gp_oracle's transforms, and the stand-in behind Engine.fit_predict_batch's packed interface.

A variant is one of the constants RQ, MEAN, NOISE below; every function takes it first.  Parameter vector of a tile:
    theta = (l_0 .. l_{D-1}, kernel variance s, likelihood variance sn2[, the variant's extra parameter]),   H = D + 2 + extra
so the first D + 2 entries are where the plain model keeps them.  Coordinates are the kernel's: already scaled.

    RQ      k(x, x') = s b^-alpha,  b = 1 + r^2 / (2 alpha),  r^2 = sum_d ((x_d - x'_d) / l_d)^2  (GPflow's and scikit-learn's
            RationalQuadratic);  extra: alpha
    MEAN    y ~ N(c 1, K + sn2 I): GPflow's GPR with gpflow.mean_functions.Constant(c), the oracle on the residual y - c;
            dnll/dc = -sum(K_y^-1 (y - c 1)),  f* = c + k*^T K_y^-1 (y - c 1), variances and covariance the zero-mean model's;
            extra: c
    NOISE   y ~ N(0, K + sn2 I + diag(v)),  v_i >= 0 given (obs_var) and not trained;  dK_y/dtheta does not involve v, and
            y_var = f*_var + sn2: a new point carries the homogeneous part only;  no extra parameter

What merges is the scaffolding and the factor-solve-predict path around a given K_y.  The arithmetic that would round
differently if merged stays a small function of its own: RQ's exp(-alpha log1p(.)) and its gradient, the mean's objective through
oracle.gp_oracle.nll_and_grad on the residual, the noise model's diagonal (K_ii + sn2) + v_i in this order.
"""
from dataclasses import dataclass

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular
from scipy.optimize import minimize

from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go


@dataclass(frozen=True)
class Variant:
    name: str
    extra: int                                             # H = D + 2 + extra
    what: str                                              # the extra parameter, last in theta


RQ = Variant("rq", 1, "alpha, the RationalQuadratic shape (positive: softplus, or its box)")
MEAN = Variant("mean", 1, "c, the constant mean (unconstrained: theta = u, or its box)")
NOISE = Variant("noise", 0, "none: obs_var is data, not a parameter")
RQ_KERNEL = "RationalQuadratic"


def _kid(kernel):
    return go.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)


def _args(variant, X, theta, obs_var):
    X, theta = np.asarray(X, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    D = X.shape[1]
    assert theta.shape == (D + 2 + variant.extra,), theta.shape
    assert (obs_var is not None) == (variant is NOISE), variant.name
    return X, D, theta


# ---- covariance functions
def _r2_and_sq(X, X2, ell):
    d = X[:, None, :] / ell - X2[None, :, :] / ell
    return np.einsum("ijk,ijk->ij", d, d), d * d


def rq_kernel_matrix(X, X2, ell, sf2, alpha):
    r2, _ = _r2_and_sq(np.asarray(X, dtype=np.float64), np.asarray(X2, dtype=np.float64), np.asarray(ell, dtype=np.float64))
    return sf2 * np.exp(-alpha * np.log1p(r2 / (2.0 * alpha)))


def kernel_matrix(variant, kernel, X, X2, theta):
    """k_theta(X, X2) without a noise term: the prior covariance."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    ell, sf2 = np.asarray(theta[:D], dtype=np.float64), float(theta[D])
    if variant is RQ:
        return rq_kernel_matrix(X, X2, ell, sf2, float(theta[D + 2]))
    return go.kernel_matrix(_kid(kernel), X, np.asarray(X2, dtype=np.float64), ell, sf2)


def K_y(variant, kernel, X, theta, obs_var=None):
    """K_theta + sn2 I at the first D + 2 entries of theta (and alpha); with obs_var, (K_ii + sn2) + v_i on the diagonal."""
    X = np.asarray(X, dtype=np.float64)
    K, sn2 = kernel_matrix(variant, kernel, X, X, theta), float(theta[X.shape[1] + 1])
    if variant is not NOISE:
        return K + sn2 * np.eye(len(X))
    i = np.arange(len(X))
    K[i, i] = (K[i, i] + sn2) + np.asarray(obs_var, dtype=np.float64).reshape(-1)
    return K


# ---- objective and gradient
def _rq_grad(kernel, X, theta, Q):
    D = X.shape[1]
    ell, sf2, alpha = theta[:D], float(theta[D]), float(theta[D + 2])
    r2, sq = _r2_and_sq(X, X, ell)
    x = r2 / (2.0 * alpha)                                  # b - 1
    kf = np.exp(-alpha * np.log1p(x))
    g = np.empty(D + 3)
    Qg = Q * (kf / (1.0 + x))                               # dk/dl_d = s (kf / b) (x_d - x'_d)^2 / l_d^3
    for d in range(D):
        g[d] = 0.5 * sf2 * np.sum(Qg * sq[:, :, d]) / ell[d]
    g[D] = 0.5 * np.sum(Q * kf)
    g[D + 1] = 0.5 * np.trace(Q)
    g[D + 2] = 0.5 * sf2 * np.sum(Q * kf * (x / (1.0 + x) - np.log1p(x)))
    return g


def _noise_grad(kernel, X, theta, Q):
    D = X.shape[1]
    ell, sf2 = theta[:D], float(theta[D])
    Kf = go.kernel_matrix(_kid(kernel), X, X, ell, sf2)
    QG = Q * go._g_over(_kid(kernel), go._scaled_sqdist(X, X, ell), sf2)
    g = np.empty(D + 2)
    for d in range(D):
        g[d] = 0.5 * np.sum(QG * (X[:, d][:, None] - X[:, d][None, :]) ** 2) / ell[d] ** 3
    g[D] = 0.5 * np.sum(Q * Kf) / sf2
    g[D + 1] = 0.5 * np.trace(Q)
    return g


def _mean_nll_and_grad(kernel, X, y, theta, want_grad):
    """The oracle's objective and gradient on y - c, and dnll/dc = -sum(alpha) behind them."""
    D = X.shape[1]
    th, c = theta[:D + 2], float(theta[D + 2])
    nll, g = go.nll_and_grad(_kid(kernel), X, y - c, th, want_grad=want_grad)
    if not want_grad:
        return nll, None
    if not np.isfinite(nll):
        return nll, np.full(D + 3, np.nan)
    alpha = cho_solve(cho_factor(K_y(MEAN, kernel, X, th), lower=True), y - c)
    return nll, np.concatenate([g, [-alpha.sum()]])


def nll_and_grad(variant, kernel, X, y, theta, obs_var=None, want_grad=True):
    """NLL = 1/2 r^T K_y^-1 r + sum log L_ii + N/2 log 2 pi (r = y, or y - c) and dNLL/dtheta = 1/2 sum_ab Q_ab dK_ab/dtheta,
    Q = K_y^-1 - a a^T.  (inf, NaN) when K_y is not positive definite, as the oracle."""
    X, D, theta = _args(variant, X, theta, obs_var)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if variant is MEAN:
        return _mean_nll_and_grad(kernel, X, y, theta, want_grad)
    N = len(y)
    try:
        L = np.linalg.cholesky(K_y(variant, kernel, X, theta, obs_var))
    except np.linalg.LinAlgError:
        return np.inf, np.full(len(theta), np.nan)
    z = solve_triangular(L, y, lower=True)
    nll = 0.5 * z @ z + np.log(np.diag(L)).sum() + 0.5 * N * np.log(2 * np.pi)
    if not want_grad:
        return nll, None
    a = solve_triangular(L, z, lower=True, trans="T")
    Q = cho_solve((L, True), np.eye(N)) - np.outer(a, a)
    return nll, (_rq_grad if variant is RQ else _noise_grad)(kernel, X, theta, Q)


# ---- predictions
def _solve(variant, kernel, X, Xs, theta, obs_var):
    X, D, theta = _args(variant, X, theta, obs_var)
    L = np.linalg.cholesky(K_y(variant, kernel, X, theta, obs_var))
    return X, D, theta, L, solve_triangular(L, kernel_matrix(variant, kernel, X, Xs, theta), lower=True)


def predict(variant, kernel, X, y, Xs, theta, obs_var=None):
    """f* (c included), f*_var, y_var = f*_var + sn2."""
    X, D, theta, L, V = _solve(variant, kernel, X, Xs, theta, obs_var)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    fvar = float(theta[D]) - np.sum(V * V, axis=0)
    if variant is MEAN:
        c = float(theta[D + 2])
        f = V.T @ solve_triangular(L, y - c, lower=True) + c
    else:
        f = V.T @ solve_triangular(L, y, lower=True)
    return f, fvar, fvar + float(theta[D + 1])


def predict_cov(variant, kernel, X, y, Xs, theta, obs_var=None):
    """f*_cov = K** - V^T V (whatever the mean)."""
    X, D, theta, L, V = _solve(variant, kernel, X, Xs, theta, obs_var)
    return kernel_matrix(variant, kernel, Xs, Xs, theta) - V.T @ V


def gls_sides(kernel, X, y, theta, dnll_dc):
    """MEAN: the two sides of the generalised-least-squares identity, for any theta:
        c - 1^T K_y^-1 y / 1^T K_y^-1 1  =  (dnll/dc) / (1^T K_y^-1 1)
    (dnll/dc = -1^T K_y^-1 (y - c 1) = c 1^T K_y^-1 1 - 1^T K_y^-1 y).  ``dnll_dc`` comes from the code under test; K_y is
    numpy's."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    cf = cho_factor(K_y(MEAN, kernel, X, theta), lower=True)
    one = np.ones(len(y))
    s11, s1y = one @ cho_solve(cf, one), one @ cho_solve(cf, y)
    return float(theta[-1]) - s1y / s11, float(dnll_dc) / s11


# ---- the fit
def transforms(variant, D, lo, hi):
    """(lo, hi, shift, ident): the oracle's transforms for every boxed or positive parameter -- the sigmoid box where both
    bounds are finite, else softplus, shifted by GPflow's lower bound for the likelihood variance only (alpha: GPflow's
    positive(), no shift) -- and ``ident``, true for MEAN's c without a box alone: GPflow's Constant.c is an unconstrained
    Parameter, theta = u."""
    H = D + 2 + variant.extra
    lo = np.full(H, np.nan) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(H, np.nan) if hi is None else np.asarray(hi, dtype=np.float64)
    box = np.isfinite(lo) & np.isfinite(hi)
    shift = np.zeros(H)
    shift[D + 1] = 0.0 if box[D + 1] else go.LIK_VAR_LOWER
    ident = np.zeros(H, dtype=bool)
    if variant is MEAN:
        ident[D + 2] = not box[D + 2]
    return np.where(box, lo, -np.inf), np.where(box, hi, np.inf), shift, ident


def fit(variant, kernel, X, y, theta0, lo=None, hi=None, trainable=None, max_iter=1000, obs_var=None, **opt_kwargs):
    """SciPy L-BFGS-B over the unconstrained u of the trainable entries (c itself where it has no box).  Returns
    (theta, nll, scipy result)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64)
    lo, hi, shift, ident = transforms(variant, D, lo, hi)
    tr = np.ones(len(theta0), dtype=bool) if trainable is None else np.asarray(trainable, dtype=bool)
    with np.errstate(all="ignore"):
        u_all = np.where(ident, theta0, go.u_from_theta(np.where(ident, 1.0, theta0), lo, hi, shift))

    def theta_of(u_tr):
        u = u_all.copy()
        u[tr] = u_tr
        th = np.where(ident, u, go.theta_from_u(u, lo, hi, shift))
        th[~tr] = theta0[~tr]
        return th

    def fun(u_tr):
        th = theta_of(u_tr)
        f, g = nll_and_grad(variant, kernel, X, y, th, obs_var)
        if not np.isfinite(f):
            return 1e300, np.zeros(int(tr.sum()))
        dth = np.where(ident, 1.0, go.dtheta_du(np.where(ident, 1.0, th), lo, hi, shift))
        return f, (g * dth)[tr]

    res = minimize(fun, u_all[tr], jac=True, method="L-BFGS-B", options=dict(maxiter=max_iter), **opt_kwargs)
    th = theta_of(res.x)
    return th, nll_and_grad(variant, kernel, X, y, th, obs_var, want_grad=False)[0], res


# ---- draws
def rq_prior_draw(rng, X, ell, sf2, sn2, alpha):
    """y ~ N(0, K_rq + sn2 I) at the rows of X."""
    K = rq_kernel_matrix(X, X, ell, sf2, alpha) + sn2 * np.eye(len(X))
    return np.linalg.cholesky(K) @ rng.standard_normal(len(X))


def fit_case(seeds=(900, 902, 905), N=150, P=16, D=3):
    """NOISE: three tiles of synthetic's Matern32 draw (true likelihood variance 0.004) with a further N(0, v_i) on every
    row, v ~ U(0, 0.001) with every seventh entry 0: small beside the homogeneous noise, so that sn2 is identified."""
    tiles = [syn.make_tile(s, N, P, D, kid=2)[:3] for s in seeds]
    T = len(seeds)
    rng = np.random.default_rng(77)
    v = rng.uniform(0.0, 0.001, T * N)
    v[::7] = 0.0
    b = dict(D=D, kernel="Matern32", obs_off=np.arange(T + 1) * N, pred_off=np.arange(T + 1) * P,
             X=np.concatenate([t[0] for t in tiles]), y=np.concatenate([t[1] for t in tiles]) + np.sqrt(v) * rng.standard_normal(T * N),
             Xs=np.concatenate([t[2] for t in tiles]), obs_var=v)
    lo, hi = syn.default_bounds(T, D)
    return b, np.ones((T, D + 2)), lo, hi


# ---- the engine stand-in
class NumpyEngine:
    """Engine stand-in for CPU tests: this module behind the packed-batch interface of Engine.fit_predict_batch."""
    device_id = 0

    def __init__(self, variant):
        self.variant, self.calls = variant, []
        self.device_name = f"cpu variant_numpy {variant.name} (tests only)"

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, mean=None, obs_var=None, **kw):
        var = self.variant
        asked = {RQ: kernel == RQ_KERNEL, MEAN: mean == "constant", NOISE: obs_var is not None}[var]
        assert asked and dtype == "f64" and not full_cov, (var.name, kernel, mean, dtype, full_cov)
        T, H = len(obs_off) - 1, D + 2 + var.extra
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        assert np.shape(trainable) == (H,) and (var is not NOISE or np.shape(obs_var) == (int(obs_off[-1]),))
        X, y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs))
        v = np.asarray(obs_var, dtype=np.float64) if var is NOISE else None
        self.calls.append(dict(T=T, theta0=theta0.copy(), lo=lo.copy(), hi=hi.copy(), optimiser=optimiser, obs_off=np.array(obs_off),
                               X=X.copy(), y=y.copy(), obs_var=None if v is None else v.copy()))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval = np.zeros(T, dtype=np.int32)
        fm, fv, yv = (np.zeros(int(pred_off[-1])) for _ in range(3))
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            vt = None if v is None else v[a:b]
            if optimiser != "none":
                theta[t], _, res = fit(var, kernel, X[a:b], y[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter, obs_var=vt)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = nll_and_grad(var, kernel, X[a:b], y[a:b], theta[t], vt, want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = predict(var, kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t], vt)
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32))
