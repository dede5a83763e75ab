"""fp64 NumPy / SciPy restatement of an exact-GP tile with known noise variances per observation (test infrastructure, like
mean_numpy.py): a Gaussian likelihood whose variance is a fixed function of the row.

    y ~ N(0, K_theta + sn2 I + diag(v)),   v_i >= 0 given and not trained
    nll and its gradient: the plain formulas with this K_y (dK_y/dtheta does not involve v)
    f* = k*^T K_y^-1 y,  f*_var = k** - k*^T K_y^-1 k*,  y_var = f*_var + sn2  (a new point carries the homogeneous part only)
Parameter vector of a tile, H = D + 2, as the plain model:   theta = (l_0 .. l_{D-1}, kernel variance, likelihood variance)
Coordinates are the kernel's: already scaled.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular
from scipy.optimize import minimize

from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go


def _kid(kernel):
    return go.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)


def _parts(X, theta):
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta = np.asarray(theta, dtype=np.float64)
    assert theta.shape == (D + 2,), theta.shape
    return X, D, theta[:D], float(theta[D]), float(theta[D + 1])


def K_y(kernel, X, theta, v):
    """K_theta + sn2 I + diag(v); on the diagonal (sf2 k + sn2) + v in this order."""
    X, D, ell, sf2, sn2 = _parts(X, theta)
    K = go.kernel_matrix(_kid(kernel), X, X, ell, sf2)
    i = np.arange(len(X))
    K[i, i] = (K[i, i] + sn2) + np.asarray(v, dtype=np.float64).reshape(-1)
    return K


def nll_and_grad(kernel, X, y, v, theta, want_grad=True):
    """(nll, gradient w.r.t. theta); (inf, NaN) when K_y is not positive definite, as the oracle."""
    X, D, ell, sf2, sn2 = _parts(X, theta)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = len(y)
    try:
        Lc = np.linalg.cholesky(K_y(kernel, X, theta, v))
    except np.linalg.LinAlgError:
        return np.inf, np.full(D + 2, np.nan)
    z = solve_triangular(Lc, y, lower=True)
    nll = 0.5 * z @ z + np.log(np.diag(Lc)).sum() + 0.5 * N * np.log(2 * np.pi)
    if not want_grad:
        return nll, None
    alpha = solve_triangular(Lc, z, lower=True, trans="T")
    Q = cho_solve((Lc, True), np.eye(N)) - np.outer(alpha, alpha)
    Kf = go.kernel_matrix(_kid(kernel), X, X, ell, sf2)
    QG = Q * go._g_over(_kid(kernel), go._scaled_sqdist(X, X, ell), sf2)
    g = np.empty(D + 2)
    for d in range(D):
        g[d] = 0.5 * np.sum(QG * (X[:, d][:, None] - X[:, d][None, :]) ** 2) / ell[d] ** 3
    g[D] = 0.5 * np.sum(Q * Kf) / sf2
    g[D + 1] = 0.5 * np.trace(Q)
    return nll, g


def _solve(kernel, X, Xs, v, theta):
    X, D, ell, sf2, sn2 = _parts(X, theta)
    Lc = np.linalg.cholesky(K_y(kernel, X, theta, v))
    Ks = go.kernel_matrix(_kid(kernel), X, np.asarray(Xs, dtype=np.float64), ell, sf2)
    return Lc, solve_triangular(Lc, Ks, lower=True), ell, sf2, sn2


def predict(kernel, X, y, v, Xs, theta):
    """f*, f*_var, y_var = f*_var + sn2."""
    Lc, V, ell, sf2, sn2 = _solve(kernel, X, Xs, v, theta)
    z = solve_triangular(Lc, np.asarray(y, dtype=np.float64).reshape(-1), lower=True)
    fvar = sf2 - np.sum(V * V, axis=0)
    return V.T @ z, fvar, fvar + sn2


def predict_cov(kernel, X, y, v, Xs, theta):
    """f*_cov = K** - k*^T K_y^-1 k*."""
    Lc, V, ell, sf2, sn2 = _solve(kernel, X, Xs, v, theta)
    Xs = np.asarray(Xs, dtype=np.float64)
    return go.kernel_matrix(_kid(kernel), Xs, Xs, ell, sf2) - V.T @ V


def transforms(D, lo, hi):
    """(lo, hi, shift) of the oracle's transforms: the sigmoid box where both bounds are finite, else softplus, shifted by
    GPflow's lower bound for the likelihood variance only."""
    lo = np.full(D + 2, np.nan) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(D + 2, np.nan) if hi is None else np.asarray(hi, dtype=np.float64)
    box = np.isfinite(lo) & np.isfinite(hi)
    shift = np.zeros(D + 2)
    shift[D + 1] = 0.0 if box[D + 1] else go.LIK_VAR_LOWER
    return np.where(box, lo, -np.inf), np.where(box, hi, np.inf), shift


def fit(kernel, X, y, v, theta0, lo=None, hi=None, trainable=None, max_iter=1000, **opt_kwargs):
    """SciPy L-BFGS-B over the unconstrained u of the trainable entries.  Returns (theta, nll, scipy result)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64)
    lo, hi, shift = transforms(D, lo, hi)
    tr = np.ones(D + 2, dtype=bool) if trainable is None else np.asarray(trainable, dtype=bool)
    u_all = go.u_from_theta(theta0, lo, hi, shift)

    def theta_of(u_tr):
        u = u_all.copy()
        u[tr] = u_tr
        th = go.theta_from_u(u, lo, hi, shift)
        th[~tr] = theta0[~tr]
        return th

    def fun(u_tr):
        th = theta_of(u_tr)
        f, g = nll_and_grad(kernel, X, y, v, th)
        if not np.isfinite(f):
            return 1e300, np.zeros(int(tr.sum()))
        return f, (g * go.dtheta_du(th, lo, hi, shift))[tr]

    res = minimize(fun, u_all[tr], jac=True, method="L-BFGS-B", options=dict(maxiter=max_iter), **opt_kwargs)
    th = theta_of(res.x)
    return th, nll_and_grad(kernel, X, y, v, th, want_grad=False)[0], res


def fit_case(seeds=(900, 902, 905), N=150, P=16, D=3):
    """Three tiles of synthetic's Matern32 draw (true likelihood variance 0.004) with a further N(0, v_i) on every row,
    v ~ U(0, 0.001) with every seventh entry 0: small beside the homogeneous noise, so that sn2 is identified."""
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


class NoiseNumpyEngine:
    """Engine stand-in for CPU tests: this module behind the packed-batch interface of Engine.fit_predict_batch."""
    device_name = "cpu noise_numpy (tests only)"
    device_id = 0

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, obs_var=None, **kw):
        assert obs_var is not None and dtype == "f64" and not full_cov, (dtype, full_cov)
        T, H = len(obs_off) - 1, D + 2
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        assert np.shape(trainable) == (H,) and np.shape(obs_var) == (int(obs_off[-1]),)
        X, y, Xs, v = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs, obs_var))
        self.calls.append(dict(T=T, theta0=theta0.copy(), optimiser=optimiser, obs_off=np.array(obs_off), X=X.copy(), y=y.copy(),
                               obs_var=v.copy()))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval = np.zeros(T, dtype=np.int32)
        fm, fv, yv = (np.zeros(int(pred_off[-1])) for _ in range(3))
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            if optimiser != "none":
                theta[t], _, res = fit(kernel, X[a:b], y[a:b], v[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = nll_and_grad(kernel, X[a:b], y[a:b], v[a:b], theta[t], want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = predict(kernel, X[a:b], y[a:b], v[a:b], Xs[pa:pb], theta[t])
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32))
