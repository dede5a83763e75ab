"""GPU: deferred predictions (fp32 4-wave build, time-sliced launches) return the same bits as inline ones.

A tile that finishes its fit while other tiles wait leaves a snapshot of what its prediction reads, and a workgroup that idles
at the end of the launch predicts it (gpsat_ring.h).  The same code runs on the same values, so every
output must be bit for bit that of the inline prediction (GPSAT_DEBUG_DEFER=0), also when the snapshot pool is too small for
every tile and some tiles predict inline, and a tile whose factorisation fails still reports NaN predictions."""
import re

import numpy as np
import pytest

from gpsat_amd import synthetic as syn

pytestmark = pytest.mark.gpu

T, N, P, D = 4096, 500, 500, 3


def _batch(fail_tiles=()):
    b = syn.make_batch(64, N, P, D, 0, base_seed=5)
    rep = T // 64
    X = np.tile(b["X"], (rep, 1)).astype(np.float32)
    y = np.tile(b["y"], rep).astype(np.float32)
    y = (y.reshape(T, N) * (1.0 + 0.02 * np.arange(T)[:, None] / T)).reshape(-1).astype(np.float32)    # distinct tiles
    Xs = np.tile(b["Xs"], (rep, 1)).astype(np.float32)
    th = np.ones((T, D + 2))
    for t in fail_tiles:                       # duplicate points and (fixed) near-zero noise: the fp32 Cholesky fails
        X[t * N:(t + 1) * N] = 0.0
        th[t, D + 1] = 1e-12
    lo, hi = syn.default_bounds(T, D)
    return dict(D=D, obs_off=np.arange(T + 1) * N, X=X, y=y, pred_off=np.arange(T + 1) * P, Xs=Xs, theta0=th, lo=lo, hi=hi,
                kernel="RBF", optimiser="lbfgs", max_iter=20, want_grad=True)


def _run(monkeypatch, kw, defer, **extra):
    from gpsat_amd.engine import Engine
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_DEFER_STATS", "1")
    if defer is None:
        monkeypatch.delenv("GPSAT_DEBUG_DEFER", raising=False)
    else:
        monkeypatch.setenv("GPSAT_DEBUG_DEFER", str(defer))
    eng = Engine(0)
    try:
        return eng.fit_predict_batch(**kw, **extra)
    finally:
        eng.close()


def _deferred(capfd):
    """deferred predictions and snapshot slots of the last launch (GPSAT_DEBUG_DEFER_STATS)"""
    m = re.findall(r"gpsat defer: T \d+: deferred predictions (\d+) of (\d+) snapshot slots", capfd.readouterr().err)
    assert m, "no deferral statistics printed"
    return int(m[-1][0]), int(m[-1][1])


def _same_bits(a, b):
    for f in ("status", "n_eval", "nll", "theta", "grad", "f_mean", "f_var", "y_var"):
        va, vb = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert va.tobytes() == vb.tobytes(), f"{f} differs"


def test_deferred_predictions_are_bit_identical_to_inline(monkeypatch, capfd):
    kw = _batch()
    inline = _run(monkeypatch, kw, 0)
    assert _deferred(capfd)[0] == 0
    assert (inline.status >= 0).all() and np.isfinite(inline.f_mean).all()
    _same_bits(_run(monkeypatch, kw, None), inline)
    n, slots = _deferred(capfd)
    assert slots == T and n > 0, (n, slots)
    # a pool of 64 slots: the first 64 deferred, every later tile inline
    _same_bits(_run(monkeypatch, kw, 64), inline)
    assert _deferred(capfd) == (64, 64)


def test_failed_tile_still_reports_nan_predictions(monkeypatch, capfd):
    fail = [7, 2049]
    kw = _batch(fail)
    trainable = [True] * D + [True, False]          # the noise stays at its near-zero start
    r = _run(monkeypatch, kw, None, trainable=trainable)
    assert _deferred(capfd)[0] > 0
    inline = _run(monkeypatch, kw, 0, trainable=trainable)
    _same_bits(r, inline)
    for t in fail:
        assert r.status[t] in (2, 3) and np.isnan(r.f_mean[t * P:(t + 1) * P]).all()
        assert np.isnan(r.f_var[t * P:(t + 1) * P]).all() and np.isnan(r.y_var[t * P:(t + 1) * P]).all()
    ok = np.setdiff1d(np.arange(T), fail)
    assert np.isfinite(r.f_mean.reshape(T, P)[ok]).all()
