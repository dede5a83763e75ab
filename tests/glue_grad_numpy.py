"""Restatements (tests only) of gpsat_glue_keyed_grad_batch: the glued value F and the exact slope G_a of the glued map per
key, as a plain per-group loop in fp64, the same in mpmath at 50 digits (with the condition number kappa_a the device bound
is stated in), a vectorised form for inputs with many keys, and an engine stand-in that answers without a device.

    w_i = prod_d normpdf(pred_d; xprt_d, sigma_i)      u_ia = (xprt_ia - pred_ia) / sigma_i^2      (dw_i/dp_a = w_i u_ia)
    W = sum w_i     F = (sum_{f ok} w_i f_i) / W     S_a = sum_{f, g_a ok} w_i (g_ia + u_ia f_i)     U_a = sum w_i u_ia
    G_a = (S_a - F U_a) / W
"""
import numpy as np

import glue_keyed_numpy as gk

MP_DIGITS = 50


def _prepare(key, pred, xprt, val, grad, sigma, max_dist):
    key = np.asarray(key, dtype=np.int64)
    pred, xprt, grad = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (pred, xprt, grad))
    val = np.asarray(val, dtype=np.float64).reshape(-1)
    R = key.shape[0]
    assert pred.shape == xprt.shape == grad.shape and val.shape == (R,) and pred.shape[1] == R
    sg = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (R,)))
    part = np.ones(R, dtype=bool)
    if max_dist is not None and np.isfinite(max_dist) and max_dist > 0:
        part = ((pred - xprt) ** 2).sum(axis=0) < float(max_dist) * float(max_dist)
    return key, pred, xprt, val, grad, sg, part


def glue_grad(key, pred, xprt, val, grad, sigma, max_dist=None):
    """key [R] (negative: ignored); pred, xprt, grad [ndim, R]; val [R]; sigma scalar or [R]; max_dist as glue_keyed.
    Returns (keys [G] ascending, counts [G], F [G], G [ndim, G]); a key without a row that takes part: count 0 and NaN."""
    key, pred, xprt, val, grad, sg, part = _prepare(key, pred, xprt, val, grad, sigma, max_dist)
    ndim = pred.shape[0]
    w = np.prod(np.exp(-((pred - xprt) / sg) ** 2 / 2) / (sg * np.sqrt(2 * np.pi)), axis=0)
    u = (xprt - pred) / sg ** 2
    keys = np.unique(key[key >= 0])
    counts = np.zeros(len(keys), dtype=np.int32)
    F = np.full(len(keys), np.nan)
    G = np.full((ndim, len(keys)), np.nan)
    for j, k in enumerate(keys):
        rows = np.nonzero((key == k) & part)[0]
        counts[j] = len(rows)
        if not len(rows):
            continue
        W = N = 0.0
        S, U = np.zeros(ndim), np.zeros(ndim)
        for i in rows:
            W += w[i]
            fok = not np.isnan(val[i])
            if fok:
                N += w[i] * val[i]
            for a in range(ndim):
                U[a] += w[i] * u[a, i]
                if fok and not np.isnan(grad[a, i]):
                    S[a] += w[i] * (grad[a, i] + u[a, i] * val[i])
        F[j] = N / W
        G[:, j] = (S - F[j] * U) / W
    return keys, counts, F, G


def glue_grad_mp(key, pred, xprt, val, grad, sigma, max_dist=None):
    """The same from the same fp64 inputs in mpmath at MP_DIGITS digits (which rows take part is decided in fp64, as above).
    Returns (keys, counts, F, G, kappa) as fp64 arrays rounded from the mpmath values, with
    kappa_a = sum w~_i (|g_ia| + |u_ia| (|f_i| + |F|)), w~ = w / W: the size of the terms G_a is the difference of."""
    import mpmath as mp
    key, pred, xprt, val, grad, sg, part = _prepare(key, pred, xprt, val, grad, sigma, max_dist)
    ndim = pred.shape[0]
    keys = np.unique(key[key >= 0])
    counts = np.zeros(len(keys), dtype=np.int32)
    F = np.full(len(keys), np.nan)
    G = np.full((ndim, len(keys)), np.nan)
    kappa = np.full((ndim, len(keys)), np.nan)
    with mp.workdps(MP_DIGITS):
        for j, k in enumerate(keys):
            rows = np.nonzero((key == k) & part)[0]
            counts[j] = len(rows)
            if not len(rows):
                continue
            ws, us = [], []
            for i in rows:
                s = mp.mpf(float(sg[i]))
                d = [mp.mpf(float(xprt[a, i])) - mp.mpf(float(pred[a, i])) for a in range(ndim)]
                wi = mp.mpf(1)
                for a in range(ndim):
                    wi *= mp.exp(-(d[a] / s) ** 2 / 2) / (s * mp.sqrt(2 * mp.pi))
                ws.append(wi)
                us.append([d[a] / (s * s) for a in range(ndim)])
            W = mp.fsum(ws)
            ok = [not np.isnan(val[i]) for i in rows]
            f = [mp.mpf(float(val[i])) if o else mp.mpf(0) for i, o in zip(rows, ok)]
            Fm = mp.fsum(wi * fi for wi, fi, o in zip(ws, f, ok) if o) / W
            F[j] = float(Fm)
            for a in range(ndim):
                gok = [o and not np.isnan(grad[a, i]) for i, o in zip(rows, ok)]
                g = [mp.mpf(float(grad[a, i])) if o else mp.mpf(0) for i, o in zip(rows, gok)]
                S = mp.fsum(wi * (gi + ui[a] * fi) for wi, gi, ui, fi, o in zip(ws, g, us, f, gok) if o)
                U = mp.fsum(wi * ui[a] for wi, ui in zip(ws, us))
                G[a, j] = float((S - Fm * U) / W)
                kappa[a, j] = float(mp.fsum(wi * (abs(ui[a]) * abs(Fm) + ((abs(gi) + abs(ui[a]) * abs(fi)) if o else 0))
                                            for wi, gi, ui, fi, o in zip(ws, g, us, f, gok)) / W)
    return keys, counts, F, G, kappa


def glue_grad_fast(key, pred, xprt, val, grad, sigma, max_dist=None):
    """The same values by np.bincount, for inputs with many keys (the loops above are quadratic).  Also returns kappa."""
    key, pred, xprt, val, grad, sg, part = _prepare(key, pred, xprt, val, grad, sigma, max_dist)
    ndim, R = pred.shape
    w = np.prod(np.exp(-((pred - xprt) / sg) ** 2 / 2) / (sg * np.sqrt(2 * np.pi)), axis=0)
    u = (xprt - pred) / sg ** 2
    keys, inv = np.unique(key[key >= 0], return_inverse=True)
    n = len(keys)
    pos = np.full(R, -1, dtype=np.int64)
    pos[key >= 0] = inv.reshape(-1)
    use = part & (key >= 0)
    counts = np.bincount(pos[use], minlength=n).astype(np.int32)
    W = np.bincount(pos[use], weights=w[use], minlength=n)
    fok = use & ~np.isnan(val)
    G, kappa = np.full((ndim, n), np.nan), np.full((ndim, n), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(counts > 0, np.bincount(pos[fok], weights=w[fok] * val[fok], minlength=n) / W, np.nan)
        for a in range(ndim):
            gok = fok & ~np.isnan(grad[a])
            S = np.bincount(pos[gok], weights=w[gok] * (grad[a][gok] + u[a][gok] * val[gok]), minlength=n)
            U = np.bincount(pos[use], weights=w[use] * u[a][use], minlength=n)
            G[a] = np.where(counts > 0, (S - F * U) / W, np.nan)
            k = np.bincount(pos[use], weights=w[use] * np.abs(u[a][use]) * np.abs(F[pos[use]]), minlength=n)
            k += np.bincount(pos[gok], weights=w[gok] * (np.abs(grad[a][gok]) + np.abs(u[a][gok] * val[gok])), minlength=n)
            kappa[a] = np.where(counts > 0, k / W, np.nan)
    return keys, counts, F, G, kappa


class GlueGradNumpyEngine(gk.GlueKeyedNumpyEngine):
    """Engine stand-in (tests only): ``glue_keyed_batch`` and ``glue_keyed_grad_batch`` from the restatements."""

    def glue_keyed_grad_batch(self, key, pred, xprt, val, grad, sigma, max_dist=None):
        self.calls.append(dict(key=np.array(key), sigma=sigma, max_dist=max_dist, R=len(key), grad=True))
        self.last = (key, pred, xprt, val, grad, sigma, max_dist)
        return glue_grad_fast(*self.last)[:4]
