"""Restatements (tests only) of gpsat_glue_keyed_hess_batch: the glued value F, the slope G_a and the second derivatives H_ab
of the glued map per key -- per group in mpmath at 50 digits (with the condition number kappa_ab the device bound is stated
in), a vectorised fp64 form for inputs with many keys, and an engine stand-in that answers without a device.

    w_i = prod_d normpdf(pred_d; xprt_d, sigma_i)      u_ia = (xprt_ia - pred_ia) / sigma_i^2      q_i = 1 / sigma_i^2
    c_iab = u_ia u_ib - delta_ab q_i                   (dw_i/dp_a = w_i u_ia,   d2w_i/dp_a dp_b = w_i c_iab)
    W = sum w_i     F = (sum_{f ok} w_i f_i) / W     U_a = sum w_i u_ia     S_a = sum_{f, g_a ok} w_i (g_ia + u_ia f_i)
    G_a = (S_a - F U_a) / W                          V_ab = sum w_i c_iab
    T_ab = sum_{f, g_a, g_b, h_ab ok} w_i (h_iab + u_ia g_ib + u_ib g_ia + c_iab f_i)
    H_ab = (T_ab - G_a U_b - G_b U_a - F V_ab) / W
    kappa_ab = sum w~_i (|h_iab| + |u_ia g_ib| + |u_ib g_ia| + |c_iab| (|f_i| + |F|)) + |G_a U_b| / W + |G_b U_a| / W

for the pairs a <= b in the order (0,0), (0,1), (1,1); w~ = w / W; a row outside a numerator adds |c_iab| |F| to kappa alone.
"""
import numpy as np

import glue_grad_numpy as gg

MP_DIGITS = gg.MP_DIGITS


def pairs(ndim):
    return [(a, b) for a in range(ndim) for b in range(a, ndim)]


def _prepare(key, pred, xprt, val, grad, hess, sigma, max_dist):
    key, pred, xprt, val, grad, sg, part = gg._prepare(key, pred, xprt, val, grad, sigma, max_dist)
    hess = np.atleast_2d(np.asarray(hess, dtype=np.float64))
    assert hess.shape == (len(pairs(pred.shape[0])), key.shape[0])
    return key, pred, xprt, val, grad, hess, sg, part


def glue_hess_mp(key, pred, xprt, val, grad, hess, sigma, max_dist=None):
    """key [R] (negative: ignored); pred, xprt, grad [ndim, R]; val [R]; hess [npair, R]; sigma scalar or [R]; max_dist as
    glue_keyed.  From the fp64 inputs in mpmath at MP_DIGITS digits (which rows take part is decided in fp64).  Returns
    (keys [G] ascending, counts [G], F [G], G [ndim, G], H [npair, G], kappa [npair, G]) as fp64 arrays rounded from the
    mpmath values; a key without a row that takes part: count 0 and NaN."""
    import mpmath as mp
    key, pred, xprt, val, grad, hess, sg, part = _prepare(key, pred, xprt, val, grad, hess, sigma, max_dist)
    ndim = pred.shape[0]
    pr = pairs(ndim)
    keys = np.unique(key[key >= 0])
    counts = np.zeros(len(keys), dtype=np.int32)
    F = np.full(len(keys), np.nan)
    G = np.full((ndim, len(keys)), np.nan)
    H = np.full((len(pr), len(keys)), np.nan)
    kappa = np.full((len(pr), len(keys)), np.nan)
    with mp.workdps(MP_DIGITS):
        m = lambda x: mp.mpf(float(x))
        for j, k in enumerate(keys):
            rows = np.nonzero((key == k) & part)[0]
            counts[j] = len(rows)
            if not len(rows):
                continue
            ws, us, qs = [], [], []
            for i in rows:
                s = m(sg[i])
                d = [m(xprt[a, i]) - m(pred[a, i]) for a in range(ndim)]
                wi = mp.mpf(1)
                for a in range(ndim):
                    wi *= mp.exp(-(d[a] / s) ** 2 / 2) / (s * mp.sqrt(2 * mp.pi))
                ws.append(wi)
                us.append([d[a] / (s * s) for a in range(ndim)])
                qs.append(1 / (s * s))
            W = mp.fsum(ws)
            fok = [not np.isnan(val[i]) for i in rows]
            f = [m(val[i]) if o else mp.mpf(0) for i, o in zip(rows, fok)]
            gok = [[o and not np.isnan(grad[a, i]) for i, o in zip(rows, fok)] for a in range(ndim)]
            g = [[m(grad[a, i]) if o else mp.mpf(0) for i, o in zip(rows, gok[a])] for a in range(ndim)]
            Fm = mp.fsum(wi * fi for wi, fi, o in zip(ws, f, fok) if o) / W
            U = [mp.fsum(wi * ui[a] for wi, ui in zip(ws, us)) for a in range(ndim)]
            Gm = []
            for a in range(ndim):
                S = mp.fsum(wi * (gi + ui[a] * fi) for wi, gi, ui, fi, o in zip(ws, g[a], us, f, gok[a]) if o)
                Gm.append((S - Fm * U[a]) / W)
            F[j] = float(Fm)
            G[:, j] = [float(x) for x in Gm]
            for p, (a, b) in enumerate(pr):
                T, V, kap = [], [], []
                for n, i in enumerate(rows):
                    c = us[n][a] * us[n][b] - (qs[n] if a == b else 0)
                    V.append(ws[n] * c)
                    kap.append(ws[n] * abs(c) * abs(Fm))
                    if gok[a][n] and gok[b][n] and not np.isnan(hess[p, i]):
                        h = m(hess[p, i])
                        T.append(ws[n] * (h + us[n][a] * g[b][n] + us[n][b] * g[a][n] + c * f[n]))
                        kap.append(ws[n] * (abs(h) + abs(us[n][a] * g[b][n]) + abs(us[n][b] * g[a][n]) + abs(c) * abs(f[n])))
                H[p, j] = float((mp.fsum(T) - Gm[a] * U[b] - Gm[b] * U[a] - Fm * mp.fsum(V)) / W)
                kappa[p, j] = float((mp.fsum(kap) + abs(Gm[a] * U[b]) + abs(Gm[b] * U[a])) / W)
    return keys, counts, F, G, H, kappa


def glue_hess_fast(key, pred, xprt, val, grad, hess, sigma, max_dist=None):
    """The same values in fp64 by np.bincount, for inputs with many keys.  Returns (keys, counts, F, G, H, kappa)."""
    key, pred, xprt, val, grad, hess, sg, part = _prepare(key, pred, xprt, val, grad, hess, sigma, max_dist)
    ndim, R = pred.shape
    pr = pairs(ndim)
    keys, counts, F, G, _ = gg.glue_grad_fast(key, pred, xprt, val, grad, sg, max_dist)
    w = np.prod(np.exp(-((pred - xprt) / sg) ** 2 / 2) / (sg * np.sqrt(2 * np.pi)), axis=0)
    u = (xprt - pred) / sg ** 2
    q = 1.0 / sg ** 2
    n = len(keys)
    pos = np.full(R, -1, dtype=np.int64)
    pos[key >= 0] = np.searchsorted(keys, key[key >= 0])
    use = part & (key >= 0)
    fok = use & ~np.isnan(val)
    gok = [fok & ~np.isnan(grad[a]) for a in range(ndim)]
    su = lambda rows, x: np.bincount(pos[rows], weights=x[rows], minlength=n)
    W = su(use, w)
    U = [su(use, w * u[a]) for a in range(ndim)]
    H, kappa = np.full((len(pr), n), np.nan), np.full((len(pr), n), np.nan)
    if n == 0:
        return keys, counts, F, G, H, kappa
    with np.errstate(invalid="ignore", divide="ignore"):
        Fr = np.where(use, F[pos], 0.0)                     # every row's own group's F
        for p, (a, b) in enumerate(pr):
            c = u[a] * u[b] - (q if a == b else 0.0)
            ok = gok[a] & gok[b] & ~np.isnan(hess[p])
            z = lambda x: np.where(ok, x, 0.0)              # NaN entries never reach a sum
            f0, ga, gb, h0 = z(val), z(grad[a]), z(grad[b]), z(hess[p])
            T = su(ok, w * (h0 + u[a] * gb + u[b] * ga + c * f0))
            V = su(use, w * c)
            H[p] = np.where(counts > 0, (T - G[a] * U[b] - G[b] * U[a] - F * V) / W, np.nan)
            k = su(use, w * np.abs(c) * np.abs(Fr))
            k += su(ok, w * (np.abs(h0) + np.abs(u[a] * gb) + np.abs(u[b] * ga) + np.abs(c) * np.abs(f0)))
            kappa[p] = np.where(counts > 0, (k + np.abs(G[a] * U[b]) + np.abs(G[b] * U[a])) / W, np.nan)
    return keys, counts, F, G, H, kappa


class GlueHessNumpyEngine(gg.GlueGradNumpyEngine):
    """Engine stand-in (tests only): ``glue_keyed_batch``, ``glue_keyed_grad_batch`` and ``glue_keyed_hess_batch`` from the
    restatements."""

    def glue_keyed_hess_batch(self, key, pred, xprt, val, grad, hess, sigma, max_dist=None):
        self.calls.append(dict(key=np.array(key), sigma=sigma, max_dist=max_dist, R=len(key), hess=True))
        self.last_hess = (key, pred, xprt, val, grad, hess, sigma, max_dist)
        return glue_hess_fast(*self.last_hess)[:5]
