"""HipSklearnGPRModel and gpsat_fit_predict_batch_ms on the GPU against sklearn's GaussianProcessRegressor and SciPy."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import minimize
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern

from gpsat_amd import _lib as L
from gpsat_amd.engine import Engine, GpsatError
from gpsat_amd.models import HipSklearnGPRModel

pytestmark = pytest.mark.gpu

NU = {"Matern12": 0.5, "Matern32": 1.5, "Matern52": 2.5}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _sk_kernel(kernel, ls, c=1.0, ls_bounds=(1e-5, 1e5)):
    base = RBF(ls, ls_bounds) if kernel == "RBF" else Matern(ls, ls_bounds, nu=NU[kernel])
    return base * ConstantKernel(c)


def _sin_tile(seed, N=60):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, 1))
    return X, np.sin(30 * X[:, 0]) * 0.3 + np.sin(2 * X[:, 0])


def test_tutorial_tile_matches_sklearn(eng):
    # 1d_local_expert_model_part_2.ipynb: 100 points of sin(1/x) + N(0, 0.05^2), RBF, likelihood_variance 0.0025;
    # the expert at 0.25 with radius 0.15
    np.random.seed(0)
    x = np.random.uniform(0.1, 1.0, 100)
    y = np.sin(1 / x) + np.random.normal(0, 0.05, 100)
    sel = np.abs(x - 0.25) <= 0.15
    X, yv = x[sel, None], y[sel]
    m = HipSklearnGPRModel(coords=X, obs=yv, kernel="RBF", likelihood_variance=0.0025, random_state=0, engine=eng)
    assert m.optimise_parameters()
    gp = GaussianProcessRegressor(_sk_kernel("RBF", [1.0], 1.0), alpha=0.0025, n_restarts_optimizer=2,
                                  random_state=0).fit(X, yv[:, None])
    assert m.get_objective_function_value() == pytest.approx(gp.log_marginal_likelihood_value_, rel=1e-8)
    np.testing.assert_allclose(m.get_lengthscales(), gp.kernel_.k1.length_scale, rtol=1e-3)
    Xs = np.linspace(0.1, 0.4, 25)[:, None]
    p = m.predict(Xs)
    mu, sd = gp.predict(Xs, return_std=True)
    np.testing.assert_allclose(p["f*"], mu.ravel(), atol=1e-6)
    np.testing.assert_allclose(p["f*_var"], sd.ravel() ** 2, atol=1e-6)
    assert set(p) == {"f*", "f*_var"}


def test_restarts_find_the_better_optimum(eng):
    # this tile has two optima: from (l, c) = (1, 1) L-BFGS-B ends at LML -51.3 (l = 0.59), the best of three at +44.0
    X, y = _sin_tile(7)
    rs = 0
    kw = dict(coords=X, obs=y, kernel="RBF", likelihood_variance=0.01, random_state=rs, engine=eng)
    one = HipSklearnGPRModel(n_restarts_optimizer=0, **kw)
    three = HipSklearnGPRModel(n_restarts_optimizer=2, **kw)
    assert one.optimise_parameters() and three.optimise_parameters()
    gp1 = GaussianProcessRegressor(_sk_kernel("RBF", [1.0]), alpha=0.01, n_restarts_optimizer=0, random_state=rs).fit(X, y)
    gp3 = GaussianProcessRegressor(_sk_kernel("RBF", [1.0]), alpha=0.01, n_restarts_optimizer=2, random_state=rs).fit(X, y)
    assert one.get_objective_function_value() == pytest.approx(gp1.log_marginal_likelihood_value_, rel=1e-8)
    assert three.get_objective_function_value() == pytest.approx(gp3.log_marginal_likelihood_value_, rel=1e-8)
    assert three.get_objective_function_value() > one.get_objective_function_value() + 1.0
    # the per-start objectives show which start won, and the first start alone is the single-start run
    assert three.f_start.shape == (3,)
    assert three.f_start[0] == pytest.approx(-one.get_objective_function_value(), rel=1e-8)
    assert -three.get_objective_function_value() == pytest.approx(three.f_start.min(), rel=1e-12)
    assert int(np.argmin(three.f_start)) != 0


# Starts whose final objective differs from SciPy's run from the same start by more than 1e-6 relative (measured,
# DESIGN.md section 10), each a divergence of the line search from MINPACK's dcsrch: ("Matern12", 3, 0, 2) stops on
# SciPy's ftol test after an accepted step of near-zero decrease, with a projected gradient of 5.5 (GPU 118.96, SciPy
# 76.33); ("Matern12", 4, 0, 2) ends 0.009 above SciPy; ("Matern32", 3, 0, 1) ends in a BETTER optimum (77.12 against
# 80.01).  The set may shrink, never grow.
KNOWN_DIVERGENT = {("Matern12", 3, 0, 2), ("Matern12", 4, 0, 2), ("Matern32", 3, 0, 1)}


@pytest.mark.parametrize("kernel", ["RBF", "Matern12", "Matern32", "Matern52"])
def test_batch_against_sklearn_and_scipy(eng, kernel):
    rng = np.random.default_rng(5)
    tiles, S = [], 3
    for t, (D, N) in enumerate([(1, 40), (2, 120), (3, 77), (4, 200), (2, 500)]):
        X = rng.uniform(0, 1, size=(N, D))
        y = np.sin(4 * X.sum(1)) + 0.1 * rng.normal(size=N)
        tiles.append((X, y))
    divergent = set()
    for D in (1, 2, 3, 4):
        sub = [(X, y) for X, y in tiles if X.shape[1] == D]
        obs_off = np.concatenate([[0], np.cumsum([len(y) for _, y in sub])])
        T, H = len(sub), D + 2
        theta0 = np.tile(np.r_[np.ones(D), 1.0, 0.05], (T, 1))
        lo = np.tile(np.r_[np.full(D + 1, 1e-5), np.nan], (T, 1))
        hi = np.tile(np.r_[np.full(D + 1, 1e5), np.nan], (T, 1))
        tr = np.r_[np.ones(D + 1, bool), False]
        # sklearn's draws for random_state = t: check_random_state(t).uniform(log lo, log hi), one start at a time
        starts = np.empty((T, S - 1, H))
        for t in range(T):
            rs = np.random.RandomState(t)
            for k in range(S - 1):
                starts[t, k] = np.r_[np.exp(rs.uniform(np.log(1e-5), np.log(1e5), D + 1)), 0.05]
        Xs = np.concatenate([X[:7] for X, _ in sub])
        pred_off = np.arange(T + 1) * 7
        r = eng.fit_predict_batch(D=D, obs_off=obs_off, X=np.concatenate([X for X, _ in sub]),
                                  y=np.concatenate([y for _, y in sub]), pred_off=pred_off, Xs=Xs, theta0=theta0,
                                  lo=lo, hi=hi, trainable=tr, kernel=kernel, optimiser="lbfgs", max_iter=15000,
                                  dtype="f64", n_starts=S, starts=starts)
        for t, (X, y) in enumerate(sub):
            k0 = _sk_kernel(kernel, np.ones(D))
            gp = GaussianProcessRegressor(k0, alpha=0.05, optimizer=None).fit(X, y)

            def obj(u):
                lml, g = gp.log_marginal_likelihood(u, eval_gradient=True, clone_kernel=False)
                return -lml, -g
            agree = True
            for k in range(S):
                th = theta0[t] if k == 0 else starts[t, k - 1]
                res = minimize(obj, np.log(th[:D + 1]), jac=True, method="L-BFGS-B", bounds=k0.bounds)
                if k == 0:     # from theta0: SciPy's end point to 1e-8
                    assert r.f_start[t, 0] == pytest.approx(res.fun, rel=1e-8, abs=1e-8), (D, t)
                # runs that stop on ftol (relative decrease <= 2.2e-9 per iteration) end up to ~1e-7 apart
                if r.f_start[t, k] != pytest.approx(res.fun, rel=1e-6):
                    divergent.add((kernel, D, t, k))
                    agree = False
            best = int(np.argmin(r.f_start[t]))
            assert r.nll[t] == pytest.approx(r.f_start[t, best], rel=1e-10)
            if agree:
                # every start ended where SciPy's did: the tile is sklearn's fit with random_state = t
                sk = GaussianProcessRegressor(_sk_kernel(kernel, np.ones(D)), alpha=0.05, n_restarts_optimizer=S - 1,
                                              random_state=t).fit(X, y)
                assert -r.nll[t] == pytest.approx(sk.log_marginal_likelihood_value_, rel=1e-6)
            gpb = GaussianProcessRegressor(_sk_kernel(kernel, r.theta[t, :D], r.theta[t, D]), alpha=0.05,
                                           optimizer=None).fit(X, y)
            assert -gpb.log_marginal_likelihood_value_ == pytest.approx(r.nll[t], rel=1e-10)
            mu, sd = gpb.predict(Xs[7 * t:7 * t + 7], return_std=True)
            np.testing.assert_allclose(r.f_mean[7 * t:7 * t + 7], mu, atol=1e-6)
            np.testing.assert_allclose(r.f_var[7 * t:7 * t + 7], sd ** 2, atol=1e-6)
    assert divergent <= KNOWN_DIVERGENT, divergent - KNOWN_DIVERGENT


def test_active_upper_bound(eng):
    X, y = _sin_tile(3)
    hi = 0.02
    m = HipSklearnGPRModel(coords=X, obs=y, kernel="RBF", likelihood_variance=0.01, n_restarts_optimizer=0, engine=eng)
    m.set_lengthscales_constraints([1e-5], [hi])
    m.set_lengthscales([0.01])
    assert m.optimise_parameters()
    gp = GaussianProcessRegressor(_sk_kernel("RBF", [0.01], 1.0, (1e-5, hi)), alpha=0.01, n_restarts_optimizer=0).fit(X, y)
    assert gp.kernel_.k1.length_scale == pytest.approx(hi, rel=1e-12)
    assert m.get_lengthscales()[0] == pytest.approx(np.exp(np.log(hi)), rel=1e-12)
    assert m.get_objective_function_value() == pytest.approx(gp.log_marginal_likelihood_value_, rel=1e-8)


def _ragged_batch(T, D, seed=1):
    rng = np.random.default_rng(seed)
    Ns = rng.integers(20, 120, T)
    obs_off = np.concatenate([[0], np.cumsum(Ns)])
    X = rng.uniform(0, 1, size=(obs_off[-1], D))
    y = np.sin(5 * X[:, 0]) + 0.1 * rng.normal(size=len(X))
    H = D + 2
    starts = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), size=(T, 2, H)))
    starts[..., -1] = 0.01
    return dict(D=D, obs_off=obs_off, X=X, y=y, pred_off=np.arange(T + 1) * 3, Xs=rng.uniform(0, 1, size=(3 * T, D)),
                theta0=np.tile(np.r_[np.ones(D), 1.0, 0.01], (T, 1)),
                lo=np.tile(np.r_[np.full(D + 1, 1e-5), np.nan], (T, 1)), hi=np.tile(np.r_[np.full(D + 1, 1e5), np.nan], (T, 1)),
                trainable=np.r_[np.ones(D + 1, bool), False], starts=starts, kernel="Matern32", optimiser="lbfgs",
                max_iter=15000, n_starts=3)


def _same_bytes(a, b, sl=slice(None), psl=slice(None)):
    for k in ("theta", "nll", "status", "n_eval", "n_iter", "f_start"):
        assert getattr(a, k)[sl].tobytes() == getattr(b, k)[sl].tobytes(), k
    for k in ("f_mean", "f_var"):
        assert np.asarray(getattr(a, k))[psl].tobytes() == np.asarray(getattr(b, k))[psl].tobytes(), k


def test_a_tile_alone_and_inside_a_batch(eng):
    T = 300
    kw = _ragged_batch(T, 2)
    full = eng.fit_predict_batch(dtype="f64", **kw)
    for t in (0, 17, T - 1):
        a, b = kw["obs_off"][t], kw["obs_off"][t + 1]
        one = eng.fit_predict_batch(dtype="f64", **{**kw, "obs_off": [0, b - a], "X": kw["X"][a:b], "y": kw["y"][a:b],
                                                    "pred_off": [0, 3], "Xs": kw["Xs"][3 * t:3 * t + 3],
                                                    "theta0": kw["theta0"][t:t + 1], "starts": kw["starts"][t:t + 1],
                                                    "lo": kw["lo"][t:t + 1], "hi": kw["hi"][t:t + 1]})
        for k in ("theta", "nll", "f_start"):
            assert getattr(one, k)[0].tobytes() == getattr(full, k)[t].tobytes(), k
        assert one.f_mean.tobytes() == full.f_mean[3 * t:3 * t + 3].tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_time_sliced_queue_does_not_change_a_bit(eng, monkeypatch, capfd, dtype):
    # 1,000 ragged tiles, S = 3.  Sliced: every evaluation is a slice (GPSAT_DEBUG_SEG=1) and 64 resident workgroups, so
    # tiles are suspended inside a start and between starts and resume on other workgroups, which read the restart state
    # back from device memory; fp32 also runs its deferred predictions.  Unsliced: every tile runs to completion.
    kw = _ragged_batch(1000, 3, seed=2)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "0")
    plain = eng.fit_predict_batch(dtype=dtype, **kw)
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "1")
    monkeypatch.setenv("GPSAT_DEBUG_GRID", "64")
    monkeypatch.setenv("GPSAT_DEBUG_DEFER_STATS", "1")
    capfd.readouterr()
    sliced = eng.fit_predict_batch(dtype=dtype, **kw)
    err = capfd.readouterr().err
    assert "re-running" not in err
    if dtype == "f32":
        import re
        m = re.search(r"deferred predictions (\d+)", err)
        assert m and int(m.group(1)) > 0, err
    _same_bytes(plain, sliced)


def test_fp32_what_it_achieves(eng):
    # fp32 does NOT meet the exact path's stated fp32 tolerance (tests/test_gpu_sklearn_pins.py: 2e-3 on the objective,
    # 2 % on the parameters) on the tutorial tile at 0.45 (alpha = 0.0025, cond(K) ~ 1e4).  The fp32 objective carries
    # rounding noise ~ cond(K) eps N, and the log-space optimiser stops on the flat ridge of length scale against
    # amplitude: measured l 0.244 against 0.202, c^2 2.99 against 0.79, LML 0.108 below the fp64 optimum of 30.39.
    # Pinned here: what it achieves -- the LML at the fp32 parameters, evaluated in fp64, within 0.15 of the fp64
    # optimum, and the length scale within 25 %
    np.random.seed(0)
    x = np.random.uniform(0.1, 1.0, 100)
    y = np.sin(1 / x) + np.random.normal(0, 0.05, 100)
    sel = np.abs(x - 0.45) <= 0.15
    X, yv = x[sel, None], y[sel]
    fit = {}
    for dt in ("f64", "f32"):
        m = HipSklearnGPRModel(coords=X, obs=yv, kernel="RBF", likelihood_variance=0.0025, random_state=0,
                               engine=eng, dtype=dt)
        assert m.optimise_parameters()
        fit[dt] = (m.get_lengthscales()[0], m.get_kernel_variance(), m.get_objective_function_value())
    l32, v32, _ = fit["f32"]
    gp = GaussianProcessRegressor(_sk_kernel("RBF", [l32], np.sqrt(v32)), alpha=0.0025, optimizer=None).fit(X, yv)
    assert -1e-8 <= fit["f64"][2] - gp.log_marginal_likelihood_value_ < 0.15
    assert abs(fit["f32"][0] / fit["f64"][0] - 1.0) < 0.25


def test_refusals_leave_the_handle_usable(eng):
    lib = eng._lib
    X, y = _sin_tile(0, N=20)
    base = dict(D=1, obs_off=[0, 20], X=X, y=y, pred_off=[0, 0], Xs=np.zeros((0, 1)), theta0=[[1.0, 1.0, 0.01]],
                lo=[[1e-5, 1e-5, np.nan]], hi=[[1e5, 1e5, np.nan]], trainable=[1, 1, 0], kernel="RBF",
                optimiser="lbfgs", max_iter=100, dtype="f64")
    bad = [dict(n_starts=2, starts=None),                                           # NULL starts with S > 1
           dict(n_starts=1, lo=[[0.0, 1e-5, np.nan]]),                              # bound <= 0 on a trainable one
           dict(n_starts=2, starts=np.ones((1, 1, 3)), hi=[[np.inf, 1e5, np.nan]]),  # non-finite bounds with S > 1
           dict(n_starts=1, optimiser="adam")]
    for extra in bad:
        with pytest.raises(GpsatError) as e:
            eng.fit_predict_batch(**{**base, **extra})
        assert "multistart" in str(e.value)
        r = eng.fit_predict_batch(**base, n_starts=1)
        assert r.status[0] == 0
    # S < 1 with a valid batch
    for S in (0, -1):
        with pytest.raises(GpsatError) as e:
            eng.fit_predict_batch(**base, n_starts=S)
        assert "n_starts" in str(e.value)
        assert eng.fit_predict_batch(**base, n_starts=1).status[0] == 0
    # a NULL multistart struct
    b = L.GpsatBatch()
    assert lib.gpsat_fit_predict_batch_ms(eng._h, C.byref(b), None) != 0
    assert "multistart" in lib.gpsat_last_error().decode()
    assert eng.fit_predict_batch(**base, n_starts=1).status[0] == 0


def _tutorial_run(eng, xprt_locs, radius):
    """docs/notebooks/1d_local_expert_model_part_2.ipynb replayed expert by expert, as LocalExpertOI runs it: the
    notebook's data (np.random.seed(0)), sklearnGPRModel(kernel='RBF', likelihood_variance=0.05**2) on the points within
    the training radius, predictions on the grid points within radius + 1e-8 (strict), glued with
    glue_local_predictions_1d.  random_state=None: the restarts draw from numpy's global state, in expert order."""
    import pandas as pd
    import scipy.stats
    from gpsat_amd.postprocessing import glue_local_predictions_1d
    np.random.seed(0)
    X_grid = np.linspace(0.1, 0.6, 100)
    X = np.random.uniform(0.1, 0.6, (100,))
    y = np.sin(1 / X) + 0.05 * np.random.randn(100)
    rows = []
    for xe in xprt_locs:
        sel = np.abs(X - xe) <= radius
        m = HipSklearnGPRModel(coords=X[sel, None], obs=y[sel], kernel="RBF", likelihood_variance=0.05 ** 2,
                               verbose=False, engine=eng)
        assert m.optimise_parameters()
        pl = X_grid[np.abs(X_grid - xe) < radius + 1e-8]
        p = m.predict(pl[:, None])
        rows.append(pd.DataFrame({"x": xe, "f*": p["f*"], "f*_var": p["f*_var"], "pred_loc_x": pl}))
    preds = pd.concat(rows, ignore_index=True)
    glued = glue_local_predictions_1d(preds_df=preds, pred_loc_col="pred_loc_x", xprt_loc_col="x",
                                      vars_to_glue=["f*", "f*_var"], inference_radius=radius + 1e-8, engine=eng)
    f_mean, f_std = glued["f*"].to_numpy(), np.sqrt(glued["f*_var"].to_numpy())
    truth = np.sin(1 / glued["pred_loc_x"].to_numpy())
    return preds, np.mean((truth - f_mean) ** 2), scipy.stats.norm.logpdf(truth, f_mean, f_std).mean()


def test_tutorial_part2_known_answers(eng):
    # run (a): experts {0.25, 0.45}, radius 0.15 -- the notebook's printed preds rows and glued scores
    preds, mse, mll = _tutorial_run(eng, [0.25, 0.45], 0.15)
    first = preds[preds["x"] == 0.25].head(5)
    np.testing.assert_allclose(first["f*"], [-0.501423, -0.080115, 0.310646, 0.635114, 0.866515], atol=5e-7)
    np.testing.assert_allclose(first["f*_var"], [0.003268, 0.000920, 0.000572, 0.000698, 0.000760], atol=5e-7)
    assert f"{mse:.4f}" == "0.0005" and f"{mll:.4f}" == "2.5734"
    # run (b): experts {0.2, 0.3, 0.4, 0.5}, radius 0.1
    _, mse, mll = _tutorial_run(eng, [0.2, 0.3, 0.4, 0.5], 0.1)
    assert f"{mse:.4f}" == "0.0003" and f"{mll:.4f}" == "2.7179"


def test_reference_test_scikit_to_1e6(eng):
    # tests/test_localexperts.py::test_scikit of the reference (kernel_variance=None, likelihood_variance=eps^2,
    # length scales in [1e-10, 5]) on its recorded answers, held to 1e-6 rather than its 1e-1
    import os
    import pandas as pd
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "kat_sklearn_matern32.npz"))
    df = pd.DataFrame({"x": d["x_train"], "y": d["y_train"]})
    np.random.seed(0)
    m = HipSklearnGPRModel(data=df, obs_col="y", coords_col="x", obs_mean=None, kernel_variance=None,
                           likelihood_variance=float(d["eps"]) ** 2, engine=eng)
    m.set_parameter_constraints({"lengthscales": {"low": 1e-10, "high": 5.}})
    assert m.optimise_parameters()
    out = m.predict(coords=np.array([float(d["x_test"])]))
    assert abs(m.get_lengthscales()[0] - float(d["ls"])) < 1e-6
    assert abs(m.get_objective_function_value() - float(d["ml"])) < 1e-6
    assert abs(out["f*"][0] - float(d["pred_mean"])) < 1e-6
    assert abs(out["f*_var"][0] - float(d["pred_std"]) ** 2) < 1e-6


def test_destroyed_engines_release_the_multistart_state():
    # gpsat_destroy frees every device buffer of the handle, the multi-start state included.  20 000 tiles of 3 observations,
    # S = 3, H = 3: that state is T (16 + (S - 1) H + S) doubles = 4 MB per engine, far above what the runtime rounds to.
    # The first create / run / close cycle absorbs what the runtime itself keeps; after it, free device memory stays put.
    import torch
    T, N, S = 20_000, 3, 3
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, size=(T * N, 1))
    kw = dict(D=1, obs_off=np.arange(T + 1) * N, X=X, y=np.sin(5 * X[:, 0]), pred_off=np.zeros(T + 1, dtype=np.int64),
              Xs=np.zeros((0, 1)), theta0=[[1.0, 1.0, 0.01]], lo=[[1e-5, 1e-5, np.nan]], hi=[[1e5, 1e5, np.nan]],
              trainable=[1, 1, 0], kernel="RBF", optimiser="lbfgs", max_iter=1, dtype="f64", n_starts=S,
              starts=np.tile([0.5, 2.0, 0.01], (T, S - 1, 1)))
    free = []
    for _ in range(4):
        e = Engine(0)
        r = e.fit_predict_batch(**kw)
        assert r.f_start.shape == (T, S) and np.isfinite(r.f_start).all()
        e.close()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free bytes after each close:", free)
    assert free[-1] == free[0], free
