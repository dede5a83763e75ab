"""fp64 NumPy restatement of the second derivatives of the posterior mean at the prediction points, their variances and the
weighted Laplacian (test infrastructure, like pred_grad_numpy.py), from K_y, its Cholesky factor and triangular solves:

    h_ab[i] = d2k(x*, x_i)/dx*_a dx*_b = s (hh d_{i,a} d_{i,b} / (l_a l_b) - delta_ab gg / l_a^2),  d_i = (x_i - x*) / l
    V_ab = L^-1 h_ab,   f_hess[ab] = V_ab^T z  (z = L^-1 y),   f_hess_var[ab] = s hh(0) (1 + 2 delta_ab) / (l_a^2 l_b^2) - V_ab^T V_ab
    h_lap = sum_a c_a h_aa,   f_lap = V_lap^T z,   f_lap_var = s hh(0) (2 sum_a c_a^2 / l_a^4 + (sum_a c_a / l_a^2)^2) - V_lap^T V_lap

with gg = -k'(r) / r (oracle.gp_oracle._g_over gives s gg) and hh = -2 dgg/d(r^2), written out here.  The pairs a <= b run over
the chosen coordinates, a ascending, then b.  Also the stand-in behind Engine.fit_predict_batch's packed interface for the
host-logic tests of the models and the orchestrator.
"""
import numpy as np
from scipy.linalg import solve_triangular

import pred_grad_numpy as pg
import variant_numpy as vn
from gpsat_amd import variants as V
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go

KERNELS = [k for k in V.PRED_HESS_KERNELS if k != "SquaredExponential"]      # the row's kernels, RBF under one name: RBF, Matern52
HH0 = {"RBF": 1.0, "Matern52": 25.0 / 3.0}                                   # hh at r = 0


def pairs(dims):
    dims = sorted(set(int(a) for a in dims))
    return [(a, b) for i, a in enumerate(dims) for b in dims[i:]]


def hh(kernel, r2):
    """hh = -2 dgg/d(r^2) of the unit-variance kernel at squared scaled distance r2."""
    if kernel == "RBF":
        return np.exp(-0.5 * r2)
    assert kernel == "Matern52", kernel
    return (25.0 / 3.0) * np.exp(-np.sqrt(5.0 * r2))


def cross_hessian(kernel, X, Xs, theta):
    """Hm [D, D, N, P]: Hm[a, b, i, p] = d2k(Xs_p, X_i) / dXs_{p,a} dXs_{p,b}."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    D = X.shape[1]
    ell, sf2 = np.asarray(theta[:D], dtype=np.float64), float(theta[D])
    r2 = go._scaled_sqdist(X, Xs, ell)
    sgg = go._g_over(go.KERNEL_IDS[kernel], r2, sf2)                          # [N, P], s gg
    shh = sf2 * hh(kernel, r2)
    d = X[:, None, :] / ell - Xs[None, :, :] / ell                            # [N, P, D]
    out = np.empty((D, D) + r2.shape)
    for a in range(D):
        for b in range(D):
            out[a, b] = shh * d[:, :, a] * d[:, :, b] / (ell[a] * ell[b]) - (sgg / ell[a] ** 2 if a == b else 0.0)
    return out


def prior_pair(kernel, theta, D, a, b):
    theta = np.asarray(theta, dtype=np.float64)
    return theta[D] * HH0[kernel] * (3.0 if a == b else 1.0) / (theta[a] ** 2 * theta[b] ** 2)


def prior_lap(kernel, theta, D, w):
    """var of sum_a w_a d2f/dx_a^2 under the prior: s hh(0) (2 sum w_a^2 / l_a^4 + (sum w_a / l_a^2)^2)."""
    theta, w = np.asarray(theta, dtype=np.float64), np.asarray(w, dtype=np.float64)
    wl = w / theta[:D] ** 2
    return theta[D] * HH0[kernel] * (2.0 * np.sum(wl * wl) + np.sum(wl) ** 2)


def predict_hess(kernel, X, y, Xs, theta, dims=None, lap_weight=None, joint=False):
    """(f_hess, f_hess_var [P, npair], f_lap, f_lap_var [P]); ``lap_weight``: D weights (default: 1 on dims).  ``joint``: also
    the posterior covariance of (f_aa)_{a in dims} per point, [P, m, m], formed from the same V's."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    N, D = X.shape
    P = len(Xs)
    dims = list(range(D)) if dims is None else sorted(set(int(a) for a in dims))
    w = np.array([1.0 if a in dims else 0.0 for a in range(D)]) if lap_weight is None else np.asarray(lap_weight, dtype=np.float64)
    pr = pairs(dims)
    fh, fhv = np.zeros((P, len(pr))), np.empty((P, len(pr)))
    for k, (a, b) in enumerate(pr):
        fhv[:, k] = prior_pair(kernel, theta, D, a, b)
    fl, flv = np.zeros(P), np.full(P, prior_lap(kernel, theta, D, w))
    theta = np.asarray(theta, dtype=np.float64)
    # the prior covariance of f_aa and f_bb: s hh(0) (1 + 2 delta_ab) / (l_a^2 l_b^2)
    cov = np.array([[prior_pair(kernel, theta, D, a, b) for b in dims] for a in dims])[None].repeat(P, axis=0)
    if N > 0:
        L = np.linalg.cholesky(vn.K_y(vn.NOISE, kernel, X, theta, np.zeros(N)))
        z = solve_triangular(L, np.asarray(y, dtype=np.float64).reshape(-1), lower=True)
        Hm = cross_hessian(kernel, X, Xs, theta)
        for k, (a, b) in enumerate(pr):
            V = solve_triangular(L, Hm[a, b], lower=True)
            fh[:, k] = V.T @ z
            fhv[:, k] -= np.sum(V * V, axis=0)
        V = solve_triangular(L, sum(w[a] * Hm[a, a] for a in range(D)), lower=True)
        fl, flv = V.T @ z, flv - np.sum(V * V, axis=0)
        if joint:
            Vd = [solve_triangular(L, Hm[a, a], lower=True) for a in dims]
            for i in range(len(dims)):
                for j in range(len(dims)):
                    cov[:, i, j] -= np.sum(Vd[i] * Vd[j], axis=0)
    return (fh, fhv, fl, flv, cov) if joint else (fh, fhv, fl, flv)


class HessNumpyEngine:
    """Engine stand-in for CPU tests: the plain fp64 expert of variant_numpy behind the packed-batch interface of
    Engine.fit_predict_batch, with ``pred_grad`` and ``pred_hess``."""
    device_id = 0
    device_name = "cpu pred_hess_numpy (tests only)"

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", full_cov=False, pred_grad=False, pred_hess=False, **kw):
        assert dtype == "f64" and not full_cov and not {k for k, v in kw.items() if v not in (None, False, 0, 0.0)} - \
            {"max_ls", "ftol", "gtol", "adam_lr", "want_grad"}, (dtype, full_cov, kw)
        T, H = len(obs_off) - 1, D + 2
        theta0, lo, hi = (np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)) for a in (theta0, lo, hi))
        X, y, Xs = (np.asarray(a, dtype=np.float64) for a in (X, y, Xs))
        spec = None
        if pred_hess:
            spec = {} if pred_hess is True else dict(pred_hess)
            spec.setdefault("dims", list(range(D)))
            spec.setdefault("lap_weight", [1.0 if a in spec["dims"] else 0.0 for a in range(D)])
        self.calls.append(dict(T=T, pred_grad=bool(pred_grad), pred_hess=None if spec is None else dict(spec), kernel=kernel,
                               optimiser=optimiser, obs_off=np.array(obs_off), pred_off=np.array(pred_off), X=X.copy(),
                               y=y.copy(), Xs=Xs.copy()))
        theta, nll, status = np.array(theta0), np.zeros(T), np.full(T, 5, dtype=np.int32)
        n_eval, sumP = np.zeros(T, dtype=np.int32), int(pred_off[-1])
        fm, fv, yv = (np.zeros(sumP) for _ in range(3))
        fg, fgv = (np.zeros((sumP, D)), np.zeros((sumP, D))) if pred_grad else (None, None)
        pr = pairs(spec["dims"]) if spec else None
        fh, fhv, fl, flv = (np.zeros((sumP, len(pr))), np.zeros((sumP, len(pr))), np.zeros(sumP), np.zeros(sumP)) if spec else (None,) * 4
        for t in range(T):
            a, b, pa, pb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1]
            v0 = np.zeros(b - a)
            if optimiser != "none":
                theta[t], _, res = vn.fit(vn.NOISE, kernel, X[a:b], y[a:b], theta0[t], lo[t], hi[t], trainable, max_iter=max_iter, obs_var=v0)
                status[t], n_eval[t] = (0 if res.success else 1), res.nfev
            nll[t] = vn.nll_and_grad(vn.NOISE, kernel, X[a:b], y[a:b], theta[t], v0, want_grad=False)[0]
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = pg.plain_predict(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t])
                if pred_grad:
                    fg[pa:pb], fgv[pa:pb] = pg.predict_grad(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t])
                if spec:
                    fh[pa:pb], fhv[pa:pb], fl[pa:pb], flv[pa:pb] = predict_hess(kernel, X[a:b], y[a:b], Xs[pa:pb], theta[t],
                                                                                spec["dims"], spec["lap_weight"])
        return BatchResult(theta=theta, nll=nll, status=status, n_eval=n_eval, f_mean=fm, f_var=fv, y_var=yv,
                           n_iter=np.zeros(T, dtype=np.int32), f_grad=fg, f_grad_var=fgv, f_hess=fh, f_hess_var=fhv,
                           f_lap=fl, f_lap_var=flv, hess_pairs=pr)
