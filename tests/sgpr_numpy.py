"""NumPy restatement of the SGPR (collapsed Titsias bound, as GPflow's SGPR computes it) used by the SGPR tests.

Written in the dense A / B form (the M x N matrix A = L^-1 Kuf / sigma is formed), not in the streaming form the HIP
kernel uses, so that it checks the kernel's algebra independently.  Coordinates are the kernel's: scaled and centred.
theta = (l_0 .. l_{D-1}, kernel_variance s, likelihood_variance sigma^2).
"""
import numpy as np

from oracle import gp_oracle as go

JITTER = 1e-6       # GPflow default_jitter


def _parts(kid, X, y, Z, theta, jitter):
    D = X.shape[1]
    ell, s, sn2 = theta[:D], float(theta[D]), float(theta[D + 1])
    M = len(Z)
    Kuu = go.kernel_matrix(kid, Z, Z, ell, s) + jitter * np.eye(M)
    Kuf = go.kernel_matrix(kid, Z, X, ell, s)
    L = np.linalg.cholesky(Kuu)
    A = np.linalg.solve(L, Kuf) / np.sqrt(sn2)
    B = np.eye(M) + A @ A.T
    LB = np.linalg.cholesky(B)
    c = np.linalg.solve(LB, A @ y) / np.sqrt(sn2)
    return ell, s, sn2, Kuu, Kuf, L, A, B, LB, c


def elbo(kid, X, y, Z, theta, jitter=JITTER):
    """ELBO = -N/2 log 2pi - sum log diag LB - N/2 log sn2 - y'y/(2 sn2) + c'c/2 - N s/(2 sn2) + tr(AA')/2."""
    N = len(y)
    ell, s, sn2, Kuu, Kuf, L, A, B, LB, c = _parts(kid, X, y, Z, theta, jitter)
    return (-0.5 * N * np.log(2 * np.pi) - np.sum(np.log(np.diag(LB))) - 0.5 * N * np.log(sn2)
            - 0.5 * (y @ y) / sn2 + 0.5 * (c @ c) - 0.5 * N * s / sn2 + 0.5 * np.sum(A * A))


def elbo_grad(kid, X, y, Z, theta, jitter=JITTER):
    """dELBO/dtheta, by the chain rule through Kuf, Kuu and kdiag with dense M x N matrices.  The jitter is a constant."""
    N, D = X.shape
    ell, s, sn2, Kuu, Kuf, L, A, B, LB, c = _parts(kid, X, y, Z, theta, jitter)
    Kinv = np.linalg.inv(Kuu)
    Sig = sn2 * Kuu + Kuf @ Kuf.T                      # S
    Sinv = np.linalg.inv(Sig)
    v = Sinv @ (Kuf @ y)
    alpha = (y - Kuf.T @ v) / sn2                       # Sigma^-1 y with Sigma = Qff + sn2 I (Woodbury)
    beta = Kuf @ alpha
    R = Kinv / sn2 - Sinv
    w = Kinv @ beta
    W = R @ Kuf + np.outer(w, alpha)                    # dELBO/dKuf
    Phi = Kuf @ Kuf.T
    C = 0.5 * np.outer(beta, beta) - 0.5 * Kuu @ Sinv @ Phi + Phi / (2 * sn2)
    G = -Kinv @ C @ Kinv                                # dELBO/dKuu
    trSigInv = (N - np.trace(Sinv @ Phi)) / sn2
    g = np.zeros(D + 2)
    # lengthscales: dk/dl_d = g(r) (x_d - z_d)^2 / l_d^3
    r2f = go._scaled_sqdist(Z, X, ell)
    r2u = go._scaled_sqdist(Z, Z, ell)
    gf = go._g_over(kid, r2f, s)
    gu = go._g_over(kid, r2u, s)
    for d in range(D):
        dKf = gf * (Z[:, d][:, None] - X[:, d][None, :]) ** 2 / ell[d] ** 3
        dKu = gu * (Z[:, d][:, None] - Z[:, d][None, :]) ** 2 / ell[d] ** 3
        g[d] = np.sum(W * dKf) + np.sum(G * dKu)
    g[D] = np.sum(W * Kuf) / s + np.sum(G * (Kuu - jitter * np.eye(len(Z)))) / s - N / (2 * sn2)
    g[D + 1] = 0.5 * (alpha @ alpha - trSigInv) + (N * s - np.trace(Kinv @ Phi)) / (2 * sn2 ** 2)
    return g


def grad_rounding_scale(kid, X, y, Z, theta, jitter=JITTER):
    """First-order size of the rounding that reaches the gradient through R = Kuu^-1 / sn2 - S^-1, whatever form computes
    it: R carries an error of about eps cond(Kuu) ||Kuu^-1||_2 / sn2 (spectral norm), and the data part of the gradient
    contracts R with Kuf and dKuf/dtheta, so the error is bounded by that times ||Kuf||_F ||dKuf/dtheta||_F.  Returns
    ||Kuu^-1||_2 / sn2 ||Kuf||_F ||dKuf/dtheta_i||_F per component (dKuf/ds = Kuf / s, dKuf/dsn2 taken as Kuf / sn2);
    multiply by eps cond(Kuu)."""
    N, D = X.shape
    ell, s, sn2, Kuu, Kuf, L, A, B, LB, c = _parts(kid, X, y, Z, theta, jitter)
    base = np.linalg.norm(np.linalg.inv(Kuu), 2) / sn2 * np.linalg.norm(Kuf)
    gf = go._g_over(kid, go._scaled_sqdist(Z, X, ell), s)
    out = np.zeros(D + 2)
    for d in range(D):
        out[d] = base * np.linalg.norm(gf * (Z[:, d][:, None] - X[:, d][None, :]) ** 2) / ell[d] ** 3
    out[D] = base * np.linalg.norm(Kuf) / s
    out[D + 1] = base * np.linalg.norm(Kuf) / sn2
    return out


def predict(kid, X, y, Z, Xs, theta, jitter=JITTER):
    """f*, f*_var, y_var at Xs (GPflow SGPR.predict_f, full_cov=False)."""
    D = X.shape[1]
    ell, s, sn2, Kuu, Kuf, L, A, B, LB, c = _parts(kid, X, y, Z, theta, jitter)
    Kus = go.kernel_matrix(kid, Z, Xs, ell, s)
    t1 = np.linalg.solve(L, Kus)
    t2 = np.linalg.solve(LB, t1)
    f = t2.T @ c
    fv = s + np.sum(t2 * t2, axis=0) - np.sum(t1 * t1, axis=0)
    return f, fv, fv + sn2


def fit_scipy(kid, X, y, Z, theta0, lo=None, hi=None, trainable=None, jitter=JITTER, maxiter=10_000):
    """Minimise -ELBO with SciPy L-BFGS-B in the kernel's unconstrained coordinates: a box where lo / hi are finite
    (sigmoid), else softplus, shifted by 1e-6 for the likelihood variance (GPflow's lower bound).  Fixed components stay at
    theta0.  Returns (theta, elbo, scipy result)."""
    from scipy.optimize import minimize
    H = len(theta0)
    lo = np.full(H, np.nan) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(H, np.nan) if hi is None else np.asarray(hi, dtype=np.float64)
    tr = np.ones(H, bool) if trainable is None else np.asarray(trainable, bool)
    box = np.isfinite(lo) & np.isfinite(hi)
    shift = np.where(~box & (np.arange(H) == H - 1), 1e-6, 0.0)
    u0 = go.u_from_theta(theta0, lo, hi, shift)

    def th_of(uf):
        u = u0.copy()
        u[tr] = uf
        return np.where(tr, go.theta_from_u(u, lo, hi, shift), theta0)

    def f(uf):
        th = th_of(uf)
        g = -elbo_grad(kid, X, y, Z, th, jitter) * go.dtheta_du(th, lo, hi, shift)
        return -elbo(kid, X, y, Z, th, jitter), g[tr]

    res = minimize(f, u0[tr], jac=True, method="L-BFGS-B", options=dict(maxiter=maxiter, ftol=1e-15, gtol=1e-8))
    th = th_of(res.x)
    return th, elbo(kid, X, y, Z, th, jitter), res
