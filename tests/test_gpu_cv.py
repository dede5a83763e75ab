"""GPU: held-out (leave-one-out / leave-group-out) predictions from every tile's own factor (gpsat_fit_predict_batch_cv),
against deletion: the rows of a fold are deleted and the fp64 oracle predicts them from the rest, at the same theta.

Bounds: the ones tests/test_gpu_parity.py::test_fp64_objective_gradient_predict holds the fp64 predictions to on the same
generator -- mean atol 1e-9 max(|y|max, 1), variances atol 1e-10 -- and y_var - f*_var = sigma^2 to 1e-12.
"""
import numpy as np
import pytest

import cv_numpy as cvn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NAMES = ["RBF", "Matern12", "Matern32", "Matern52"]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _pack(tiles, P=0):
    """tiles: list of (X, y, Xs, theta) -> the packed arrays of Engine.fit_predict_batch."""
    D = tiles[0][0].shape[1]
    obs_off = np.concatenate([[0], np.cumsum([len(t[1]) for t in tiles])]).astype(np.int64)
    pred_off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int64)
    return dict(D=D, obs_off=obs_off, pred_off=pred_off, X=np.concatenate([t[0] for t in tiles]).reshape(-1, D),
                y=np.concatenate([t[1] for t in tiles]), Xs=np.concatenate([t[2] for t in tiles]).reshape(-1, D),
                theta0=np.array([t[3] for t in tiles]), dtype="f64")


def _check(r, a, e, X, y, theta, kid, labels, tag=""):
    """Held-out outputs of rows a:e of the batch result against deletion."""
    mean, fvar, yvar = (np.asarray(v)[a:e] for v in (r.cv_mean, r.cv_f_var, r.cv_y_var))
    m0, f0, y0 = cvn.deletion(kid, X, y, theta, labels)
    D = X.shape[1]
    never = np.isnan(m0)
    assert (np.isnan(mean) == never).all() and (np.isnan(fvar) == never).all() and (np.isnan(yvar) == never).all(), tag
    ok = ~never
    ymax = max(float(np.abs(y).max()) if len(y) else 0.0, 1.0)
    errs = (np.abs(mean - m0)[ok].max(initial=0.0), np.abs(fvar - f0)[ok].max(initial=0.0), np.abs(yvar - y0)[ok].max(initial=0.0),
            np.abs(yvar - fvar - theta[D + 1])[ok].max(initial=0.0))
    print(f"cv {tag}: N={len(y)} max|mean err|={errs[0]:.3e} max|f_var err|={errs[1]:.3e} max|y_var err|={errs[2]:.3e} "
          f"max|y_var-f_var-sn2|={errs[3]:.3e}")
    assert errs[0] <= 1e-9 * ymax, tag
    assert errs[1] <= 1e-10 and errs[2] <= 1e-10, tag
    assert errs[3] <= 1e-12, tag


def _cv_one(eng, X, y, theta, kid, labels, **kw):
    b = _pack([(X, y, np.zeros((0, X.shape[1])), theta)])
    return eng.fit_predict_batch(kernel=NAMES[kid], optimiser="none", cv_fold="loo" if labels is None else labels, **b, **kw)


# ---- 1. leave-one-out against deletion
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_loo_against_deletion(eng, kid, D):
    N = 200
    X, y, _, th = syn.make_tile(900 + 10 * kid + D, N, 0, D, kid)
    r = _cv_one(eng, X, y, th, kid, None)
    assert r.status[0] == 5
    _check(r, 0, N, X, y, th, kid, None, f"loo kid={kid} D={D}")


@pytest.mark.parametrize("kid", [0, 2])
@pytest.mark.parametrize("N", [1, 2, 17, 500, 1000])
def test_loo_tile_sizes(eng, kid, N):
    X, y, _, th = syn.make_tile(40 + N + kid, N, 0, 3, kid)
    r = _cv_one(eng, X, y, th, kid, None)
    _check(r, 0, N, X, y, th, kid, None, f"loo kid={kid} N={N}")


# ---- 2. folds against deletion
@pytest.mark.parametrize("kid", [0, 2])
def test_folds_against_deletion(eng, kid):
    N, D = 500, 3
    rng = np.random.default_rng(17 + kid)
    X, y, _, th = syn.make_tile(70 + kid, N, 0, D, kid)
    runs = cvn.run_labels(N, rng, 1, 64)
    shuffled = rng.permutation(runs)
    sparse = (shuffled.astype(np.int64) * 1000 + 7).astype(np.int32)
    sparse[rng.random(N) < 0.1] = -5
    sparse[3] = -1
    gmax = L.max_cv_fold("f64", D)
    assert gmax >= 256
    big = np.arange(N, dtype=np.int32) + 10
    big[rng.permutation(N)[:gmax]] = 2                   # one fold at exactly the limit, scattered over the tile
    for tag, lab in (("runs", runs), ("shuffled", shuffled), ("sparse", sparse), ("limit", big)):
        r = _cv_one(eng, X, y, th, kid, lab)
        _check(r, 0, N, X, y, th, kid, lab, f"{tag} kid={kid}")
    assert np.isnan(np.asarray(r.cv_mean)).sum() == 0
    # a fold that is the whole tile: the prior
    Nw = 200
    Xw, yw, _, thw = syn.make_tile(71 + kid, Nw, 0, D, kid)
    r = _cv_one(eng, Xw, yw, thw, kid, np.zeros(Nw, dtype=np.int32))
    _check(r, 0, Nw, Xw, yw, thw, kid, np.zeros(Nw, dtype=np.int32), f"whole tile kid={kid}")
    np.testing.assert_allclose(r.cv_f_var, thw[D], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.cv_mean, 0.0, rtol=0, atol=1e-9)


def test_folds_on_the_eight_wave_build(eng):
    """A tile whose LDS does not fit twice into a CU runs on the 8-wave build (gpsat_plan.h): the same phase there, next to a
    small tile in the same batch."""
    D, kid = 3, 2
    rng = np.random.default_rng(23)
    tiles = [syn.make_tile(80, 1200, 0, D, kid), syn.make_tile(81, 90, 0, D, kid)]
    labels = [rng.permutation(cvn.run_labels(1200, rng, 1, 64)), cvn.run_labels(90, rng, 1, 64)]
    b = _pack(tiles)
    r = eng.fit_predict_batch(kernel=NAMES[kid], optimiser="none", cv_fold=np.concatenate(labels).astype(np.int32), **b)
    for t, (X, y, _, th) in enumerate(tiles):
        _check(r, int(b["obs_off"][t]), int(b["obs_off"][t + 1]), X, y, th, kid, labels[t], f"8-wave build, tile {t}")


# ---- 3. every other output keeps its bits
def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("optimiser,max_iter", [("lbfgs", 12), ("none", 0)])
def test_other_outputs_bit_identical(eng, optimiser, max_iter, want_grad):
    """want_grad=False: the final evaluation of the plain call runs without L^-1, that of the held-out call with it."""
    Ns, D, kid = [300, 64, 500, 17, 1, 128, 0, 250], 3, 2
    rng = np.random.default_rng(5)
    tiles = [syn.make_tile(200 + t, n, 9, D, kid) for t, n in enumerate(Ns)]
    b = _pack(tiles)
    if optimiser == "lbfgs":
        b["theta0"] = np.ones_like(b["theta0"])
    lo, hi = syn.default_bounds(len(Ns), D)
    kw = dict(kernel=NAMES[kid], optimiser=optimiser, max_iter=max_iter, lo=lo, hi=hi, want_grad=want_grad, **b)
    labels = np.concatenate([cvn.run_labels(n, rng, 1, 40) for n in Ns]).astype(np.int32)
    r0 = eng.fit_predict_batch(**kw)
    assert r0.cv_mean is None and r0.cv_f_var is None and r0.cv_y_var is None
    for cv_fold in ("loo", labels):
        r1 = eng.fit_predict_batch(cv_fold=cv_fold, **kw)
        for name in ("theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var") + (("grad",) if want_grad else ()):
            assert _same_bits(getattr(r0, name), getattr(r1, name)), name
        assert want_grad or (r0.grad is None and r1.grad is None)
        assert np.isfinite(np.asarray(r1.cv_mean)).all()


# ---- 4. determinism: alone, in the middle of a ragged batch, on a second launch
def test_held_out_bits_do_not_depend_on_the_batch(eng):
    D, kid, T = 3, 0, 300
    rng = np.random.default_rng(11)
    Ns = rng.integers(20, 300, T)
    Ns[150] = 412
    tiles = [syn.make_tile(3000 + t, int(n), 0, D, kid) for t, n in enumerate(Ns)]
    labels = [rng.permutation(cvn.run_labels(int(n), rng, 1, 30)).astype(np.int32) for n in Ns]
    b = _pack(tiles)
    kw = dict(kernel=NAMES[kid], optimiser="none")
    rb = eng.fit_predict_batch(cv_fold=np.concatenate(labels), **b, **kw)
    rb2 = eng.fit_predict_batch(cv_fold=np.concatenate(labels), **b, **kw)
    a, e = int(b["obs_off"][150]), int(b["obs_off"][151])
    X, y, _, th = tiles[150]
    r1 = _cv_one(eng, X, y, th, kid, labels[150])
    for name in ("cv_mean", "cv_f_var", "cv_y_var"):
        assert _same_bits(getattr(rb, name), getattr(rb2, name)), name
        assert _same_bits(np.asarray(getattr(rb, name))[a:e], getattr(r1, name)), name
    _check(rb, a, e, X, y, th, kid, labels[150], "tile 150 of 300")


# ---- 5. after a fit: deletion at the returned theta
def test_held_out_after_a_fit(eng):
    Ns, D, kid = [300, 150, 420], 3, 2
    rng = np.random.default_rng(3)
    tiles = [syn.make_tile(500 + t, n, 4, D, kid) for t, n in enumerate(Ns)]
    b = _pack(tiles)
    b["theta0"] = np.ones_like(b["theta0"])
    lo, hi = syn.default_bounds(len(Ns), D)
    labels = [cvn.run_labels(n, rng, 1, 25) for n in Ns]
    r = eng.fit_predict_batch(kernel=NAMES[kid], optimiser="lbfgs", max_iter=20, lo=lo, hi=hi, cv_fold=np.concatenate(labels), **b)
    assert (r.status <= 1).all() and (r.n_eval > 1).all()
    for t, (X, y, _, _) in enumerate(tiles):
        a, e = int(b["obs_off"][t]), int(b["obs_off"][t + 1])
        _check(r, a, e, X, y, r.theta[t], kid, labels[t], f"fitted tile {t}")


# ---- 6. errors
def test_errors(eng):
    from gpsat_amd.engine import GpsatError
    D, kid, N = 3, 0, 300
    X, y, Xs, th = syn.make_tile(1, N, 5, D, kid)
    b = _pack([(X, y, Xs, th)])
    with pytest.raises(GpsatError, match=r"\(-1\).*GPSAT_F64 only"):
        eng.fit_predict_batch(kernel="RBF", optimiser="none", cv_fold="loo", **{**b, "dtype": "f32"})
    lab = np.arange(N, dtype=np.int32)
    lab[:L.max_cv_fold("f64", D) + 1] = 123456
    with pytest.raises(GpsatError, match=r"\(-1\).*tile 0: fold 123456 holds 257 rows"):
        eng.fit_predict_batch(kernel="RBF", optimiser="none", cv_fold=lab, **b)
    with pytest.raises(GpsatError, match=r"\(-1\).*f_cov"):
        eng.fit_predict_batch(kernel="RBF", optimiser="none", cv_fold="loo", full_cov=True, **b)
    assert L.max_cv_fold("f32", D) == 0 and L.max_cv_fold("f64", 5) == 0


# ---- 7. HipGPRModel.cross_validate
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_model_cross_validate(eng, dtype):
    from gpsat_amd.models import HipGPRModel, HipSGPRModel
    from oracle.gp_oracle import OracleGPR
    N, D, kid = 240, 2, 2
    rng = np.random.default_rng(8)
    X, y, _, th = syn.make_tile(33, N, 0, D, kid)
    cs, osc = np.array([2.0, 0.5]), 3.0
    coords, obs = X * cs, y * osc + 12.5
    track = np.array(["t%d" % (i // 23) for i in range(N)], dtype=object)
    kw = dict(coords=coords, obs=obs, coords_scale=cs, obs_scale=osc, obs_mean="local", kernel=NAMES[kid])
    m = HipGPRModel(engine=eng, dtype=dtype, **kw)
    m.set_parameters(lengthscales=th[:D], kernel_variance=th[D], likelihood_variance=th[D + 1])
    for fold in (None, track, np.column_stack([np.arange(N) // 50, np.arange(N) % 2])):
        out = m.cross_validate(fold=fold)
        lab = np.arange(N) if fold is None else (np.unique(fold, return_inverse=True)[1] if np.ndim(fold) == 1
                                                else np.unique(fold, axis=0, return_inverse=True)[1].reshape(-1))
        ymax = max(float(np.abs(m.obs).max()), 1.0)
        for g in np.unique(lab):
            G = lab == g
            o = OracleGPR(coords[~G], obs[~G] - m.obs_mean[0, 0], coords_scale=cs, obs_scale=osc, obs_mean=None, kernel=NAMES[kid])
            o.set_parameters(lengthscales=th[:D], kernel_variance=th[D], likelihood_variance=th[D + 1])
            ref = o.predict(coords[G])
            np.testing.assert_allclose(out["f*"][G], ref["f*"], rtol=0, atol=1e-9 * ymax)
            np.testing.assert_allclose(out["f*_var"][G], ref["f*_var"], rtol=0, atol=1e-10)
            np.testing.assert_allclose(out["y_var"][G], ref["y_var"], rtol=0, atol=1e-10)
        assert (out["f_bar"] == m.obs_mean[0, 0]).all()
    with pytest.raises(ValueError, match="at most 256"):
        HipGPRModel(engine=eng, coords=rng.normal(size=(300, 2)), obs=rng.normal(size=300)).cross_validate(fold=np.zeros(300, dtype=int))
    with pytest.raises(NotImplementedError):
        HipSGPRModel(engine=eng, coords=coords, obs=obs, num_inducing_points=20).cross_validate()


# ---- 8. orchestrator: table cv_preds
def test_orchestrator_cv_preds(eng, tmp_path):
    import pandas as pd
    from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
    from gpsat_amd.models import HipGPRModel
    rng = np.random.default_rng(4)
    n = 6000
    df = pd.DataFrame({"x": rng.uniform(0, 20, n), "y": rng.uniform(0, 20, n), "t": rng.integers(0, 3, n).astype(float),
                       "track": rng.integers(0, 12, n)})
    df["z"] = np.sin(df["x"] / 3) * np.cos(df["y"] / 4) + 0.1 * rng.standard_normal(n)
    xl = pd.DataFrame([(x, y, t) for t in (0.0, 1.0, 2.0) for x in (3.0, 6.5, 10.0, 13.5, 17.0) for y in (5.0, 10.0, 15.0)][:42],
                      columns=["x", "y", "t"])
    data = {"data_source": df, "obs_col": "z", "coords_col": ["x", "y", "t"],
            "local_select": [{"col": "t", "comp": "<=", "val": 1}, {"col": "t", "comp": ">=", "val": -1},
                             {"col": ["x", "y"], "comp": "<", "val": 3.5}]}
    cs = [2.0, 2.0, 1.0]
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "coords_scale": cs},
             "constraints": {"lengthscales": {"low": [0.1, 0.1, 0.1], "high": [30, 30, 30]}}, "optim_kwargs": {"max_iter": 6}}
    args = ({"source": xl}, data, model, {"method": "expert_loc"})
    base = BatchedLocalExpertOI(*args, engine=eng, dtype="f64").run(None)
    store = str(tmp_path / "cv")
    out = BatchedLocalExpertOI(*args, engine=eng, dtype="f64", cv={"by": ["track"]}).run(store, store_every=16)
    assert len(xl) >= 40 and set(base) | {"cv_preds"} == set(out)
    for name, tab in base.items():               # the other tables: bit for bit those of the run without cv
        got = out[name].drop(columns=["cv_rows_skipped", "run_time"], errors="ignore")
        ref = tab.drop(columns=["run_time"], errors="ignore")
        assert list(got.columns) == list(ref.columns) and got.index.equals(ref.index), name
        for c in ref.columns:
            a, b = got[c].values, ref[c].values
            assert a.dtype == b.dtype and (a.tobytes() == b.tobytes() if a.dtype != object else (a == b).all()), (name, c)
    cvp, rd = out["cv_preds"], out["run_details"]
    assert (rd["cv_rows_skipped"] == 0).all() and len(cvp) == int(rd["num_obs"].sum())
    ls, kv, lv = out["lengthscales"], out["kernel_variance"], out["likelihood_variance"]
    for key in xl.itertuples(index=False):
        key = tuple(float(v) for v in key)
        rows = cvp.loc[[key]]
        d = df.iloc[rows["obs_index"].values]
        m = HipGPRModel(data=d, obs_col="z", coords_col=["x", "y", "t"], coords_scale=cs, kernel="Matern32", engine=eng, dtype="f64")
        m.set_parameters(lengthscales=ls.loc[[key]].sort_values("_dim_0")["lengthscales"].values,
                         kernel_variance=float(kv.loc[[key]]["kernel_variance"].values[0]),
                         likelihood_variance=float(lv.loc[[key]]["likelihood_variance"].values[0]))
        ref = m.cross_validate(fold=d["track"].values)
        for c in ("f*", "f*_var", "y_var"):
            assert rows[c].values.tobytes() == ref[c].tobytes(), (key, c)
    # a second run on the same store adds nothing
    n_disk = len(get_results(store)["cv_preds"])
    assert n_disk == len(cvp)
    out2 = BatchedLocalExpertOI(*args, engine=eng, dtype="f64", cv={"by": ["track"]}).run(store, store_every=16)
    assert len(out2["run_details"]) == 0 and len(get_results(store)["cv_preds"]) == n_disk
