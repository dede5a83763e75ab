"""NumPy restatements of the joint log predictive density of a held-out fold, log N(y_G; mu_{G|-G}, Sigma_{G|-G}), used by
the cv_joint tests.  Two independent routes at fixed theta = (l_0 .. l_{D-1}, kernel_variance, likelihood_variance):
  * closed_form: from the full factor.  A = K_y^-1, alpha = A y, L_A = chol(A_GG), u = L_A^-1 alpha_G:
        lpd = -1/2 u^T u + sum log diag(L_A) - g/2 log 2 pi
    (Sigma_{G|-G} = A_GG^-1 and y_G - mu = A_GG^-1 alpha_G);
  * deletion: the rows are deleted, oracle.gp_oracle predicts them from the rest with the full covariance, and
    scipy.stats.multivariate_normal evaluates y_G under N(f*, f*_cov + sn2 I).  A fold that is the whole tile: the prior.
Both return one number per fold, folds in ascending label (labels None: every row its own fold, in row order) -- the
numbering of gpsat_cv_refit_count.  Rows with a label < 0 belong to no fold.
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.stats import multivariate_normal

from oracle import gp_oracle as go

LOG_2PI = float(np.log(2.0 * np.pi))


def folds(labels, N):
    labels = np.arange(N) if labels is None else np.asarray(labels)
    return [np.flatnonzero(labels == v) for v in np.unique(labels[labels >= 0])]


def closed_form(kid, X, y, theta, labels=None):
    N, D = X.shape
    if N == 0:
        return np.zeros(0)
    ell, sf2, sn2 = theta[:D], float(theta[D]), float(theta[D + 1])
    Ky = go.kernel_matrix(kid, X, X, ell, sf2) + sn2 * np.eye(N)
    Linv = np.linalg.solve(np.linalg.cholesky(Ky), np.eye(N))
    alpha = Linv.T @ (Linv @ y)
    out = []
    for G in folds(labels, N):
        LA = np.linalg.cholesky(Linv[:, G].T @ Linv[:, G])
        u = solve_triangular(LA, alpha[G], lower=True)
        out.append(-0.5 * float(u @ u) + float(np.log(np.diag(LA)).sum()) - 0.5 * len(G) * LOG_2PI)
    return np.array(out)


def deletion_fold(kid, X, y, theta, G, delta=0.0):
    """One fold: rows ``G`` deleted, the rest (and the fold's y) shifted by ``delta``."""
    N, D = X.shape
    sf2, sn2 = float(theta[D]), float(theta[D + 1])
    keep = np.setdiff1d(np.arange(N), G)
    if len(keep) == 0:
        f, cov = np.zeros(len(G)), go.kernel_matrix(kid, X[G], X[G], theta[:D], sf2)
    else:
        f = go.predict(kid, X[keep], y[keep] - delta, X[G], theta)[0]
        cov = go.predict_cov(kid, X[keep], y[keep] - delta, X[G], theta)[0]
    cov = 0.5 * (cov + cov.T) + sn2 * np.eye(len(G))
    return float(multivariate_normal.logpdf(y[G] - delta, mean=f, cov=cov, allow_singular=False))


def deletion(kid, X, y, theta, labels=None, recentre=False, thetas=None):
    """``recentre``: every fold's remaining rows are de-meaned by their own mean, the fold's rows shifted alike (the refit
    flavour's delta).  ``thetas`` [F, H]: the parameters of every fold (the refit flavour's cv_theta) instead of ``theta``."""
    N = len(y)
    out = []
    for k, G in enumerate(folds(labels, N)):
        keep = np.setdiff1d(np.arange(N), G)
        delta = float(np.mean(y[keep])) if recentre and len(keep) else 0.0
        out.append(deletion_fold(kid, X, y, theta if thetas is None else thetas[k], G, delta))
    return np.array(out)


def univariate(y, mean, y_var):
    """log N(y_i; mean_i, y_var_i): the joint density of a one-row fold."""
    return -0.5 * (y - mean) ** 2 / y_var - 0.5 * np.log(2.0 * np.pi * y_var)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0))
