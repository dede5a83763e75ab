"""NumPy restatement (tests only) of gpsat_glue_keyed_batch: the weighted average of the rows of every key >= 0, keys
ascending, and an engine stand-in that answers ``glue_keyed_batch`` from it without a device."""
import numpy as np


def glue_keyed(key, pred, xprt, vals, sigma, max_dist=None):
    """key [R] (negative: ignored); pred, xprt [ndim, R]; vals [nvars, R]; sigma scalar or [R]; max_dist: a row takes part
    only if sum_d (pred_d - xprt_d)^2 < max_dist^2 (None, +inf, <= 0: every row).  Returns (keys [G] ascending, counts [G],
    out [nvars, G]): out = sum w v / sum w with w = prod_d normpdf(pred_d; xprt_d, sigma); a NaN value is left out of the
    numerator, its weight stays in the denominator; a key without a row that takes part: count 0 and NaN."""
    key = np.asarray(key, dtype=np.int64)
    pred, xprt, vals = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (pred, xprt, vals))
    R = key.shape[0]
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (R,))
    diff = pred - xprt
    w = np.prod(np.exp(-(diff / sg) ** 2 / 2) / (sg * np.sqrt(2 * np.pi)), axis=0)
    part = np.ones(R, dtype=bool)
    if max_dist is not None and np.isfinite(max_dist) and max_dist > 0:
        part = (diff ** 2).sum(axis=0) < float(max_dist) * float(max_dist)
    keys = np.unique(key[key >= 0])
    counts = np.zeros(len(keys), dtype=np.int32)
    out = np.full((vals.shape[0], len(keys)), np.nan)
    for j, k in enumerate(keys):
        rows = np.nonzero((key == k) & part)[0]
        counts[j] = len(rows)
        if len(rows):
            ws = w[rows].sum()
            for v in range(vals.shape[0]):
                x = vals[v, rows]
                ok = ~np.isnan(x)
                out[v, j] = (w[rows][ok] * x[ok]).sum() / ws
    return keys, counts, out


def glue_keyed_fast(key, pred, xprt, vals, sigma, max_dist=None):
    """The same values by np.add.at, for inputs with many keys (the loop above is quadratic)."""
    key = np.asarray(key, dtype=np.int64)
    pred, xprt, vals = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (pred, xprt, vals))
    R = key.shape[0]
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (R,))
    diff = pred - xprt
    w = np.prod(np.exp(-(diff / sg) ** 2 / 2) / (sg * np.sqrt(2 * np.pi)), axis=0)
    part = np.ones(R, dtype=bool)
    if max_dist is not None and np.isfinite(max_dist) and max_dist > 0:
        part = (diff ** 2).sum(axis=0) < float(max_dist) * float(max_dist)
    keys, inv = np.unique(key[key >= 0], return_inverse=True)
    pos = np.full(R, -1, dtype=np.int64)
    pos[key >= 0] = inv.reshape(-1)
    use = part & (key >= 0)
    counts = np.bincount(pos[use], minlength=len(keys)).astype(np.int32)
    ws = np.bincount(pos[use], weights=w[use], minlength=len(keys))
    out = np.full((vals.shape[0], len(keys)), np.nan)
    for v in range(vals.shape[0]):
        ok = use & ~np.isnan(vals[v])
        num = np.bincount(pos[ok], weights=w[ok] * vals[v][ok], minlength=len(keys))
        with np.errstate(invalid="ignore", divide="ignore"):
            out[v] = np.where(counts > 0, num / ws, np.nan)
    return keys, counts, out


class GlueKeyedNumpyEngine:
    """Engine stand-in (tests only): ``glue_keyed_batch`` from the restatement."""
    device_name = "no device (numpy restatement, tests only)"
    device_id = 0

    def __init__(self):
        self.calls = []

    def glue_keyed_batch(self, key, pred, xprt, vals, sigma, max_dist=None):
        self.calls.append(dict(key=np.array(key), sigma=sigma, max_dist=max_dist, R=len(key)))
        return glue_keyed_fast(key, pred, xprt, vals, sigma, max_dist)
