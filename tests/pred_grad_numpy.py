"""fp64 NumPy restatement of the gradient of the posterior mean at the prediction points and its variance per component
(test infrastructure, like variant_numpy.py), from K_y, its Cholesky factor and triangular solves:

    g_a[i] = dk(x*, x_i)/dx*_a = s gg(r^2) d_{i,a} / l_a,   d_i = (x_i - x*) / l,  r^2 = sum d_i^2,  gg = -k'(r) / r
    V_a = L^-1 g_a,   f_grad[a] = V_a^T z  (z = L^-1 y),   f_grad_var[a] = s gg(0) / l_a^2 - V_a^T V_a

with oracle.gp_oracle._g_over for s gg (the factor of dk/dl_d there), and the stand-in behind Engine.fit_predict_batch's packed
interface for the host-logic tests of the models and the orchestrator.  The plain model of variant_numpy is its NOISE variant
with obs_var = 0, which changes no bit of K_y.
"""
import numpy as np
from scipy.linalg import solve_triangular

import variant_numpy as vn
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go

KERNELS = ["RBF", "Matern32", "Matern52"]
GG0 = {"RBF": 1.0, "Matern32": 3.0, "Matern52": 5.0 / 3.0}                # gg at r = 0


def plain_predict(kernel, X, y, Xs, theta):
    return vn.predict(vn.NOISE, kernel, X, y, Xs, theta, np.zeros(len(X)))


def plain_predict_cov(kernel, X, y, Xs, theta):
    return vn.predict_cov(vn.NOISE, kernel, X, y, Xs, theta, np.zeros(len(X)))


def cross_gradient(kernel, X, Xs, theta):
    """G [D, N, P]: G[a, i, p] = dk(Xs_p, X_i) / dXs_{p,a}."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    D = X.shape[1]
    ell, sf2 = np.asarray(theta[:D], dtype=np.float64), float(theta[D])
    sgg = go._g_over(go.KERNEL_IDS[kernel], go._scaled_sqdist(X, Xs, ell), sf2)          # [N, P], s gg
    d = X[:, None, :] / ell - Xs[None, :, :] / ell                                         # [N, P, D]
    return np.stack([sgg * d[:, :, a] / ell[a] for a in range(D)])


def prior_grad(kernel, theta, P, D):
    """A tile without observations: gradient 0, variance s gg(0) / l_a^2, [P, D] each."""
    theta = np.asarray(theta, dtype=np.float64)
    return np.zeros((P, D)), np.tile(theta[D] * GG0[kernel] / theta[:D] ** 2, (P, 1))


def predict_grad(kernel, X, y, Xs, theta):
    """(f_grad, f_grad_var), [P, D] each."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    N, D = X.shape
    if N == 0:
        return prior_grad(kernel, theta, len(Xs), D)
    L = np.linalg.cholesky(vn.K_y(vn.NOISE, kernel, X, theta, np.zeros(N)))
    z = solve_triangular(L, np.asarray(y, dtype=np.float64).reshape(-1), lower=True)
    G = cross_gradient(kernel, X, Xs, theta)
    prior = prior_grad(kernel, theta, len(Xs), D)[1]
    fg, fgv = np.empty((len(Xs), D)), np.empty((len(Xs), D))
    for a in range(D):
        V = solve_triangular(L, G[a], lower=True)
        fg[:, a] = V.T @ z
        fgv[:, a] = prior[:, a] - np.sum(V * V, axis=0)
    return fg, fgv


class GradNumpyEngine:
    """Engine stand-in for CPU tests: the plain fp64 expert of variant_numpy behind the packed-batch interface of
    Engine.fit_predict_batch, with ``pred_grad``."""
    device_id = 0
    device_name = "cpu pred_grad_numpy (tests only)"

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, pred_grad=False, **kw):
        assert dtype == "f64" and not full_cov and not {k for k, v in kw.items() if v not in (None, False, 0, 0.0)} - \
            {"max_ls", "ftol", "gtol", "adam_lr", "want_grad"}, (dtype, full_cov, kw)
        T, H = len(obs_off) - 1, D + 2
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        X, y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs))
        self.calls.append(dict(T=T, pred_grad=bool(pred_grad), kernel=kernel, optimiser=optimiser, obs_off=np.array(obs_off),
                               pred_off=np.array(pred_off), X=X.copy(), y=y.copy(), Xs=Xs.copy()))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval, sumP = np.zeros(T, dtype=np.int32), int(pred_off[-1])
        fm, fv, yv = (np.zeros(sumP) for _ in range(3))
        fg, fgv = (np.zeros((sumP, D)), np.zeros((sumP, D))) if pred_grad else (None, None)
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            v0 = np.zeros(b - a)
            if optimiser != "none":
                theta[t], _, res = vn.fit(vn.NOISE, kernel, X[a:b], y[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter, obs_var=v0)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = vn.nll_and_grad(vn.NOISE, kernel, X[a:b], y[a:b], theta[t], v0, want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = plain_predict(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t])
                if pred_grad:
                    fg[pa:pb], fgv[pa:pb] = predict_grad(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t])
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32), f_grad=fg, f_grad_var=fgv)
