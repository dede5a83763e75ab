"""NumPy restatements of held-out (cross-validation) prediction used by the held-out tests.

Two independent routes to the prediction of the rows G of a fold from all other rows of a tile, at fixed theta =
(l_0 .. l_{D-1}, kernel_variance, likelihood_variance):
  * closed_form: from the full factor.  A = K_y^-1, alpha = A y:  mean = y_G - A_GG^-1 alpha_G, cov(y_G) = A_GG^-1
    (one row: Rasmussen & Williams eq. 5.12);
  * deletion: the rows are deleted and oracle.gp_oracle.predict is called on the rest.
Rows with a label < 0 are never held out: NaN.
"""
import numpy as np

from oracle import gp_oracle as go


def _folds(labels, N):
    labels = np.arange(N) if labels is None else np.asarray(labels)
    return [np.flatnonzero(labels == v) for v in np.unique(labels[labels >= 0])]


def closed_form(kid, X, y, theta, labels=None):
    N, D = X.shape
    ell, sf2, sn2 = theta[:D], float(theta[D]), float(theta[D + 1])
    mean, fvar, yvar = (np.full(N, np.nan) for _ in range(3))
    if N == 0:
        return mean, fvar, yvar
    Ky = go.kernel_matrix(kid, X, X, ell, sf2) + sn2 * np.eye(N)
    Linv = np.linalg.solve(np.linalg.cholesky(Ky), np.eye(N))
    alpha = Linv.T @ (Linv @ y)
    for G in _folds(labels, N):
        AGG = Linv[:, G].T @ Linv[:, G]
        C = np.linalg.inv(AGG)
        C = 0.5 * (C + C.T)
        mean[G] = y[G] - C @ alpha[G]
        yvar[G] = np.diag(C)
        fvar[G] = np.diag(C) - sn2
    return mean, fvar, yvar


def deletion(kid, X, y, theta, labels=None):
    N, D = X.shape
    sf2, sn2 = float(theta[D]), float(theta[D + 1])
    mean, fvar, yvar = (np.full(N, np.nan) for _ in range(3))
    for G in _folds(labels, N):
        keep = np.setdiff1d(np.arange(N), G)
        if len(keep) == 0:                      # the fold is the whole tile: the prior
            mean[G], fvar[G], yvar[G] = 0.0, sf2, sf2 + sn2
            continue
        f, fv, yv = go.predict(kid, X[keep], y[keep], X[G], theta)
        mean[G], fvar[G], yvar[G] = f, fv, yv
    return mean, fvar, yvar


def run_labels(N, rng, lo=1, hi=64):
    """Contiguous runs of lo..hi rows: labels 0, 1, 2, ... along the tile."""
    out, f = np.empty(N, dtype=np.int32), 0
    i = 0
    while i < N:
        g = int(rng.integers(lo, hi + 1))
        out[i:i + g] = f
        i, f = i + g, f + 1
    return out
