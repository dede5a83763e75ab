"""fp64 NumPy / SciPy restatement of an exact-GP tile with the RationalQuadratic covariance function (test infrastructure,
like sgpr_numpy.py): objective, analytic gradient, predictions, full covariance and a SciPy L-BFGS-B fit in u-space with
oracle.gp_oracle's transforms.

    k(x, x') = s b^-alpha,   b = 1 + r^2 / (2 alpha),   r^2 = sum_d ((x_d - x'_d) / l_d)^2
(GPflow's and scikit-learn's RationalQuadratic).  Parameter vector of a tile, H = D + 3:
    theta = (l_0 .. l_{D-1}, kernel variance s, likelihood variance, alpha)
alpha is last, so the first D + 2 entries are where the other kernels keep them.  Coordinates are the kernel's: already scaled.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular
from scipy.optimize import minimize

from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go

KERNEL = "RationalQuadratic"


def split(theta, D):
    theta = np.asarray(theta, dtype=np.float64)
    assert theta.shape == (D + 3,), theta.shape
    return theta[:D], float(theta[D]), float(theta[D + 1]), float(theta[D + 2])


def _r2_and_sq(X, X2, ell):
    d = X[:, None, :] / ell - X2[None, :, :] / ell
    return np.einsum("ijk,ijk->ij", d, d), d * d


def kernel_matrix(X, X2, ell, sf2, alpha):
    r2, _ = _r2_and_sq(np.asarray(X, dtype=np.float64), np.asarray(X2, dtype=np.float64), np.asarray(ell, dtype=np.float64))
    return sf2 * np.exp(-alpha * np.log1p(r2 / (2.0 * alpha)))


def nll_and_grad(X, y, theta, want_grad=True):
    """NLL = 1/2 y^T K^-1 y + sum log L_ii + N/2 log 2 pi and dNLL/dtheta = 1/2 sum_ab Q_ab dK_ab/dtheta, Q = K^-1 - a a^T.
    (inf, NaN) when K is not positive definite."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N, D = X.shape
    ell, sf2, sn2, alpha = split(theta, D)
    r2, sq = _r2_and_sq(X, X, ell)
    x = r2 / (2.0 * alpha)                                  # b - 1
    kf = np.exp(-alpha * np.log1p(x))
    K = sf2 * kf + sn2 * np.eye(N)
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return np.inf, np.full(D + 3, np.nan)
    z = solve_triangular(L, y, lower=True)
    nll = 0.5 * z @ z + np.log(np.diag(L)).sum() + 0.5 * N * np.log(2 * np.pi)
    if not want_grad:
        return nll, None
    a = solve_triangular(L, z, lower=True, trans="T")
    Q = cho_solve((L, True), np.eye(N)) - np.outer(a, a)
    g = np.empty(D + 3)
    Qg = Q * (kf / (1.0 + x))                               # dk/dl_d = s (kf / b) (x_d - x'_d)^2 / l_d^3
    for d in range(D):
        g[d] = 0.5 * sf2 * np.sum(Qg * sq[:, :, d]) / ell[d]
    g[D] = 0.5 * np.sum(Q * kf)
    g[D + 1] = 0.5 * np.trace(Q)
    g[D + 2] = 0.5 * sf2 * np.sum(Q * kf * (x / (1.0 + x) - np.log1p(x)))
    return nll, g


def _factor(X, y, theta):
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ell, sf2, sn2, alpha = split(theta, X.shape[1])
    L = np.linalg.cholesky(kernel_matrix(X, X, ell, sf2, alpha) + sn2 * np.eye(len(X)))
    return X, L, solve_triangular(L, y, lower=True), ell, sf2, sn2, alpha


def predict(X, y, Xs, theta):
    """f*, f*_var, y_var."""
    X, L, z, ell, sf2, sn2, alpha = _factor(X, y, theta)
    V = solve_triangular(L, kernel_matrix(X, np.asarray(Xs, dtype=np.float64), ell, sf2, alpha), lower=True)
    fvar = sf2 - np.sum(V * V, axis=0)
    return V.T @ z, fvar, fvar + sn2


def predict_cov(X, y, Xs, theta):
    """f*_cov = K** - V^T V."""
    X, L, z, ell, sf2, sn2, alpha = _factor(X, y, theta)
    Xs = np.asarray(Xs, dtype=np.float64)
    V = solve_triangular(L, kernel_matrix(X, Xs, ell, sf2, alpha), lower=True)
    return kernel_matrix(Xs, Xs, ell, sf2, alpha) - V.T @ V


def transforms(D, lo, hi):
    """(lo, hi, shift) as oracle.gp_oracle's transforms take them: the sigmoid box where both bounds are finite, else softplus,
    shifted by GPflow's lower bound for the likelihood variance only (alpha: GPflow's positive(), no shift)."""
    lo = np.full(D + 3, np.nan) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(D + 3, np.nan) if hi is None else np.asarray(hi, dtype=np.float64)
    box = np.isfinite(lo) & np.isfinite(hi)
    shift = np.zeros(D + 3)
    shift[D + 1] = 0.0 if box[D + 1] else go.LIK_VAR_LOWER
    return np.where(box, lo, -np.inf), np.where(box, hi, np.inf), shift


def fit(X, y, theta0, lo=None, hi=None, trainable=None, max_iter=1000, **opt_kwargs):
    """SciPy L-BFGS-B over the unconstrained u of the trainable entries.  Returns (theta, nll, scipy result)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64)
    lo, hi, shift = transforms(D, lo, hi)
    tr = np.ones(D + 3, dtype=bool) if trainable is None else np.asarray(trainable, dtype=bool)
    u_all = go.u_from_theta(theta0, lo, hi, shift)

    def theta_of(u_tr):
        u = u_all.copy()
        u[tr] = u_tr
        th = go.theta_from_u(u, lo, hi, shift)
        th[~tr] = theta0[~tr]
        return th

    def fun(u_tr):
        th = theta_of(u_tr)
        f, g = nll_and_grad(X, y, th)
        if not np.isfinite(f):
            return 1e300, np.zeros(int(tr.sum()))
        return f, (g * go.dtheta_du(th, lo, hi, shift))[tr]

    res = minimize(fun, u_all[tr], jac=True, method="L-BFGS-B", options=dict(maxiter=max_iter), **opt_kwargs)
    th = theta_of(res.x)
    return th, nll_and_grad(X, y, th, want_grad=False)[0], res


def rq_prior_draw(rng, X, ell, sf2, sn2, alpha):
    """y ~ N(0, K_rq + sn2 I) at the rows of X."""
    K = kernel_matrix(X, X, ell, sf2, alpha) + sn2 * np.eye(len(X))
    return np.linalg.cholesky(K) @ rng.standard_normal(len(X))


class RqNumpyEngine:
    """Engine stand-in for CPU tests: this module behind the packed-batch interface of Engine.fit_predict_batch."""
    device_name = "cpu rq_numpy (tests only)"
    device_id = 0

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, **kw):
        assert kernel == KERNEL and dtype == "f64" and not full_cov, (kernel, dtype, full_cov)
        T, H = len(obs_off) - 1, D + 3
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        assert np.shape(trainable) == (H,)
        self.calls.append(dict(T=T, theta0=theta0.copy(), optimiser=optimiser))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval = np.zeros(T, dtype=np.int32)
        fm, fv, yv = (np.zeros(int(pred_off[-1])) for _ in range(3))
        X, y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs))
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            if optimiser != "none":
                theta[t], _, res = fit(X[a:b], y[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = nll_and_grad(X[a:b], y[a:b], theta[t], want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = predict(X[a:b], y[a:b], Xs[pa:pb], theta[t])
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32))
