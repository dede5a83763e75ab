"""fp64 NumPy / SciPy restatement of an exact-GP tile with a trainable constant mean (test infrastructure, like rq_numpy.py):
GPflow's GPR with gpflow.mean_functions.Constant(c), stated through oracle.gp_oracle on the residual y - c.

    y ~ N(c 1, K_theta + sn2 I),   nll(theta, c; y) = nll_zero-mean(theta; y - c 1),   dnll/dc = -sum(K_y^-1 (y - c 1)),
    f*(x) = c + k*(x)^T K_y^-1 (y - c 1);  the variances and the full covariance are the zero-mean model's.
Parameter vector of a tile, H = D + 3:   theta = (l_0 .. l_{D-1}, kernel variance, likelihood variance, c)
c is last, so the first D + 2 entries are where the zero-mean model keeps them.  Coordinates are the kernel's: already scaled.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import minimize

from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go


def _kid(kernel):
    return go.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)


def _split(theta, D):
    theta = np.asarray(theta, dtype=np.float64)
    assert theta.shape == (D + 3,), theta.shape
    return theta[:D + 2], float(theta[D + 2])


def K_y(kernel, X, theta):
    """K_theta + sn2 I at the first D + 2 entries of theta."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    return go.kernel_matrix(_kid(kernel), X, X, np.asarray(theta[:D], dtype=np.float64), float(theta[D])) + float(theta[D + 1]) * np.eye(len(X))


def nll_and_grad(kernel, X, y, theta, want_grad=True):
    """The oracle's objective and gradient on y - c, and dnll/dc = -sum(alpha) behind them.  (inf, NaN) when K_y is not
    positive definite, as the oracle."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    D = X.shape[1]
    th, c = _split(theta, D)
    nll, g = go.nll_and_grad(_kid(kernel), X, y - c, th, want_grad=want_grad)
    if not want_grad:
        return nll, None
    if not np.isfinite(nll):
        return nll, np.full(D + 3, np.nan)
    alpha = cho_solve(cho_factor(K_y(kernel, X, th), lower=True), y - c)
    return nll, np.concatenate([g, [-alpha.sum()]])


def predict(kernel, X, y, Xs, theta):
    """f* (c included), f*_var, y_var."""
    X = np.asarray(X, dtype=np.float64)
    th, c = _split(theta, X.shape[1])
    f, fv, yv = go.predict(_kid(kernel), X, np.asarray(y, dtype=np.float64).reshape(-1) - c, Xs, th)[:3]
    return f + c, fv, yv


def predict_cov(kernel, X, y, Xs, theta):
    """f*_cov: the zero-mean model's."""
    X = np.asarray(X, dtype=np.float64)
    th, c = _split(theta, X.shape[1])
    out = go.predict_cov(_kid(kernel), X, np.asarray(y, dtype=np.float64).reshape(-1) - c, Xs, th)
    return out[0] if isinstance(out, tuple) else out


def gls_sides(kernel, X, y, theta, dnll_dc):
    """The two sides of the generalised-least-squares identity, for any theta:
        c - 1^T K_y^-1 y / 1^T K_y^-1 1  =  (dnll/dc) / (1^T K_y^-1 1)
    (dnll/dc = -1^T K_y^-1 (y - c 1) = c 1^T K_y^-1 1 - 1^T K_y^-1 y).  ``dnll_dc`` comes from the code under test; K_y is
    numpy's."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    cf = cho_factor(K_y(kernel, X, theta), lower=True)
    one = np.ones(len(y))
    s11, s1y = one @ cho_solve(cf, one), one @ cho_solve(cf, y)
    return float(theta[-1]) - s1y / s11, float(dnll_dc) / s11


def transforms(D, lo, hi):
    """(lo, hi, shift, ident): the oracle's transforms for every boxed or positive parameter -- the sigmoid box where both
    bounds are finite, else softplus, shifted by GPflow's lower bound for the likelihood variance only -- and ``ident``,
    true for c without a box: GPflow's Constant.c is an unconstrained Parameter, theta = u."""
    lo = np.full(D + 3, np.nan) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(D + 3, np.nan) if hi is None else np.asarray(hi, dtype=np.float64)
    box = np.isfinite(lo) & np.isfinite(hi)
    shift = np.zeros(D + 3)
    shift[D + 1] = 0.0 if box[D + 1] else go.LIK_VAR_LOWER
    ident = np.zeros(D + 3, dtype=bool)
    ident[D + 2] = not box[D + 2]
    return np.where(box, lo, -np.inf), np.where(box, hi, np.inf), shift, ident


def fit(kernel, X, y, theta0, lo=None, hi=None, trainable=None, max_iter=1000, **opt_kwargs):
    """SciPy L-BFGS-B over (u, c): the unconstrained u of the trainable entries, c itself where it has no box.  Returns
    (theta, nll, scipy result)."""
    X = np.asarray(X, dtype=np.float64)
    D = X.shape[1]
    theta0 = np.asarray(theta0, dtype=np.float64)
    lo, hi, shift, ident = transforms(D, lo, hi)
    tr = np.ones(D + 3, dtype=bool) if trainable is None else np.asarray(trainable, dtype=bool)
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
        f, g = nll_and_grad(kernel, X, y, th)
        if not np.isfinite(f):
            return 1e300, np.zeros(int(tr.sum()))
        dth = np.where(ident, 1.0, go.dtheta_du(np.where(ident, 1.0, th), lo, hi, shift))
        return f, (g * dth)[tr]

    res = minimize(fun, u_all[tr], jac=True, method="L-BFGS-B", options=dict(maxiter=max_iter), **opt_kwargs)
    th = theta_of(res.x)
    return th, nll_and_grad(kernel, X, y, th, want_grad=False)[0], res


class MeanNumpyEngine:
    """Engine stand-in for CPU tests: this module behind the packed-batch interface of Engine.fit_predict_batch."""
    device_name = "cpu mean_numpy (tests only)"
    device_id = 0

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, mean=None, **kw):
        assert mean == "constant" and dtype == "f64" and not full_cov, (mean, dtype, full_cov)
        T, H = len(obs_off) - 1, D + 3
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        assert np.shape(trainable) == (H,)
        self.calls.append(dict(T=T, theta0=theta0.copy(), lo=lo.copy(), hi=hi.copy(), optimiser=optimiser))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval = np.zeros(T, dtype=np.int32)
        fm, fv, yv = (np.zeros(int(pred_off[-1])) for _ in range(3))
        X, y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs))
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            if optimiser != "none":
                theta[t], _, res = fit(kernel, X[a:b], y[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = nll_and_grad(kernel, X[a:b], y[a:b], theta[t], want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = predict(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t])
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32))
