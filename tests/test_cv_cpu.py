"""CPU: held-out (cross-validation) predictions -- the closed form against deletion in NumPy, the host-side label
factorisation, what the orchestrator refuses, the ``cv_preds`` table layout (with the fp64 oracle as the engine) and the new
symbols of the C ABI."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import cv_numpy as cvn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult, factorise_folds
from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
from oracle import gp_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kid", [0, 2])
@pytest.mark.parametrize("N", [200, 500, 1000])
def test_closed_form_equals_deletion(kid, N):
    """A_GG = (L^-1[:, G])^T (L^-1[:, G]); mean = y_G - A_GG^-1 alpha_G; cov = A_GG^-1 -- against deleting the rows."""
    rng = np.random.default_rng(N + kid)
    X, y, _, th = syn.make_tile(5 + N + kid, N, 0, 3, kid)
    runs = cvn.run_labels(N, rng, 1, 64)
    cases = [runs, rng.permutation(runs)] + ([None] if N == 200 else [])
    for lab in cases:
        a, b = cvn.closed_form(kid, X, y, th, lab), cvn.deletion(kid, X, y, th, lab)
        for u, v in zip(a, b):
            assert np.abs(u - v).max() <= 1e-12


def test_label_factorisation():
    # sparse and negative integer labels: negative = never held out; codes dense, by first appearance
    np.testing.assert_array_equal(factorise_folds(np.array([70000, -3, 70000, 5, -1, 2 ** 31 - 1])), [0, -1, 0, 1, -1, 2])
    # labels of any hashable kind; None is never held out
    np.testing.assert_array_equal(factorise_folds(np.array(["b", "a", "b", None], dtype=object)), [0, 1, 0, -1])
    # 2-D: equal rows form a fold
    np.testing.assert_array_equal(factorise_folds(np.array([[1, 2.5], [1, 2.5], [0, 2.5], [1, 2.0]])), [0, 0, 1, 2])
    # one-row folds, and a fold that is the whole tile
    np.testing.assert_array_equal(factorise_folds(np.arange(5)[::-1]), [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(factorise_folds(np.full(4, 9)), [0, 0, 0, 0])
    assert factorise_folds(np.zeros(0, dtype=int)).shape == (0,)
    with pytest.raises(ValueError):
        factorise_folds(np.arange(4), N=5)


def test_new_symbols_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpsat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpsat_[a-z_]+)\s*\(", src))
    assert {"gpsat_fit_predict_batch_cv", "gpsat_max_cv_fold"} <= declared
    assert declared == set(L.EXPORTS)
    lib = L.load()
    assert hasattr(lib, "gpsat_fit_predict_batch_cv") and hasattr(lib, "gpsat_max_cv_fold")
    assert all(lib.gpsat_max_cv_fold(L.F64, D) >= 256 for D in range(1, 5))
    assert lib.gpsat_max_cv_fold(L.F32, 3) == 0 and lib.gpsat_max_cv_fold(L.F64, 0) == 0 and lib.gpsat_max_cv_fold(L.F64, 5) == 0
    assert lib.gpsat_version() == 4
    # the ctypes mirror of gpsat_cv: four pointers and eight reserved words
    import ctypes as C
    assert C.sizeof(L.GpsatCv) == 4 * C.sizeof(C.c_void_p) + 32


# ------------------------------------------------------------------------------------------------------------------
# orchestrator
# ------------------------------------------------------------------------------------------------------------------
class OracleCvEngine:
    """Engine stand-in (tests only): the fp64 oracle, and cv_numpy.closed_form for ``cv_fold``."""
    device_name = "cpu-oracle (tests only)"
    device_id = 0

    def __init__(self):
        self.cv_calls = 0

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", cv_fold=None, **kw):
        kid = go.KERNEL_IDS[kernel]
        o = go.fit_predict_batch(kid, D, obs_off, X.astype(np.float64), y.astype(np.float64), pred_off, Xs.astype(np.float64),
                                 theta0, lo, hi, np.asarray(trainable, bool), max_iter=max_iter, optimise=optimiser != "none")
        cv = {}
        if cv_fold is not None:
            self.cv_calls += 1
            out = np.full((3, int(obs_off[-1])), np.nan)
            for t in range(len(obs_off) - 1):
                a, b = int(obs_off[t]), int(obs_off[t + 1])
                lab = None if isinstance(cv_fold, str) else np.asarray(cv_fold)[a:b]
                out[:, a:b] = cvn.closed_form(kid, X[a:b].astype(np.float64), y[a:b].astype(np.float64), o["theta"][t], lab)
            cv = dict(cv_mean=out[0], cv_f_var=out[1], cv_y_var=out[2])
        return BatchResult(theta=o["theta"], nll=o["nll"], status=np.where(o["success"], 0, 1).astype(np.int32),
                           n_eval=o["n_eval"].astype(np.int32), f_mean=o["f_mean"], f_var=o["f_var"], y_var=o["y_var"], **cv)


def _configs(n_track=7):
    rng = np.random.default_rng(0)
    n = 420
    df = pd.DataFrame({"x": rng.uniform(0, 10, n), "y": rng.uniform(0, 10, n), "t": rng.integers(0, 3, n).astype(float),
                       "track": rng.integers(0, n_track, n)})
    df["z"] = np.sin(df["x"]) + 0.1 * rng.standard_normal(n)
    xl = pd.DataFrame([(x, y, t) for t in (0.0, 1.0, 2.0) for x in (2.5, 5.0, 7.5) for y in (3.0, 7.0)], columns=["x", "y", "t"])
    data = {"data_source": df, "obs_col": "z", "coords_col": ["x", "y", "t"],
            "local_select": [{"col": "t", "comp": "<=", "val": 1}, {"col": "t", "comp": ">=", "val": -1},
                             {"col": ["x", "y"], "comp": "<", "val": 4.0}]}
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "obs_mean": "local", "coords_scale": [2.0, 2.0, 1.0]},
             "constraints": {"lengthscales": {"low": [0.1, 0.1, 0.1], "high": [20, 20, 20]}},
             "optim_kwargs": {"max_iter": 5}}
    return {"source": xl}, data, model, {"method": "expert_loc"}, df


def test_orchestrator_refuses_what_is_not_built():
    loc, data, model, pred, _ = _configs()
    eng = OracleCvEngine()
    with pytest.raises(NotImplementedError, match="fp64 only.*'f32'"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f32", cv="loo")
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, cv={"by": ["track"]})       # dtype None = fp32
    sg = dict(model, oi_model="HipSGPRModel", init_params=dict(model["init_params"], num_inducing_points=20))
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(loc, data, sg, pred, engine=eng, dtype="f64", cv="loo")
    with pytest.raises(ValueError, match="cv must be"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv="kfold")
    fc = dict(model, pred_kwargs={"full_cov": True})
    with pytest.raises(NotImplementedError, match="full_cov"):
        BatchedLocalExpertOI(loc, data, fc, pred, engine=eng, dtype="f64", cv="loo")
    with pytest.raises(KeyError, match="nope"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["nope"]})
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv="loo")
    with pytest.raises(NotImplementedError, match="sharded"):
        oi.run(None, world_size=2)


@pytest.mark.parametrize("cv", ["loo", {"by": ["track"]}])
def test_cv_preds_table(tmp_path, cv):
    loc, data, model, pred, df = _configs()
    eng = OracleCvEngine()
    base = BatchedLocalExpertOI(loc, data, model, pred, engine=OracleCvEngine(), dtype="f64").run(None)
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv=cv)
    store = str(tmp_path / "s")
    out = oi.run(store, store_every=7)                 # several waves
    assert "cv_preds" not in base and "cv_rows_skipped" not in base["run_details"].columns
    for name, tab in base.items():                     # every other table as without cv
        got = out[name].drop(columns=["cv_rows_skipped", "run_time"], errors="ignore")
        pd.testing.assert_frame_equal(got, tab.drop(columns=["run_time"], errors="ignore"))
    cvp, rd = out["cv_preds"], out["run_details"]
    by = [] if cv == "loo" else ["track"]
    assert list(cvp.columns) == ["_dim_0", "obs_index"] + by + ["pred_loc_x", "pred_loc_y", "pred_loc_t", "z", "f*", "f*_var", "y_var", "f_bar"]
    assert list(cvp.index.names) == ["x", "y", "t"] and len(cvp) == int(rd["num_obs"].sum()) and (rd["cv_rows_skipped"] == 0).all()
    # the rows are the tile's own, in the tile's order
    np.testing.assert_array_equal(cvp["z"].values, df["z"].values[cvp["obs_index"].values])
    np.testing.assert_array_equal(cvp["pred_loc_x"].values, df["x"].values[cvp["obs_index"].values])
    if by:
        np.testing.assert_array_equal(cvp["track"].values, df["track"].values[cvp["obs_index"].values])
    first = cvp.loc[(2.5, 3.0, 0.0)]
    np.testing.assert_array_equal(first["_dim_0"].values, np.arange(len(first)))
    assert np.isfinite(cvp[["f*", "f*_var", "y_var"]].values).all()
    # committed with the waves: the store holds the same table, and a second run adds nothing
    on_disk = get_results(store, expert_order=True)
    assert len(on_disk["cv_preds"]) == len(cvp)
    calls = eng.cv_calls
    out2 = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv=cv).run(store, store_every=7)
    assert eng.cv_calls == calls and len(out2.get("cv_preds", [])) == 0
    assert len(get_results(store)["cv_preds"]) == len(cvp)


def test_cv_fold_above_the_limit_is_not_held_out():
    loc, data, model, pred, df = _configs(n_track=1)            # one track: every tile is one fold
    data = dict(data, local_select=[{"col": "t", "comp": "<=", "val": 3}, {"col": "t", "comp": ">=", "val": -3}])
    assert len(df) > L.max_cv_fold("f64", 3)
    out = BatchedLocalExpertOI(loc, data, model, pred, engine=OracleCvEngine(), dtype="f64", cv={"by": ["track"]}).run(None, optimise=False)
    assert (out["run_details"]["cv_rows_skipped"] == len(df)).all()
    assert np.isnan(out["cv_preds"]["f*"].values).all()


def test_cv_preds_units_with_local_mean_and_obs_scale():
    """``cv_preds`` holds f* in the units of ``preds`` with the tile's ``f_bar``: ``f_bar + obs_scale f*`` predicts the raw
    observation.  Checked per expert against deletion with the de-meaning constant held fixed."""
    loc, data, model, pred, df = _configs()
    osc = 2.5
    df = df.copy()
    df["z"] = 40.0 + 3.0 * df["z"]
    data = dict(data, data_source=df)
    model = dict(model, init_params=dict(model["init_params"], obs_scale=osc))
    out = BatchedLocalExpertOI(loc, data, model, pred, engine=OracleCvEngine(), dtype="f64", cv={"by": ["track"]}).run(None, optimise=False)
    cvp = out["cv_preds"]
    cs = np.array(model["init_params"]["coords_scale"], dtype=np.float64)
    key = (5.0, 7.0, 1.0)
    rows = cvp.loc[[key]]
    d = df.iloc[rows["obs_index"].values]
    fbar = float(d["z"].mean())
    np.testing.assert_allclose(rows["f_bar"].values, fbar, rtol=1e-14)
    th = np.array([float(v) for v in out["lengthscales"].loc[[key]].sort_values("_dim_0")["lengthscales"].values] +
                  [float(out["kernel_variance"].loc[[key]]["kernel_variance"].values[0]),
                   float(out["likelihood_variance"].loc[[key]]["likelihood_variance"].values[0])])
    X, y = d[["x", "y", "t"]].values / cs, (d["z"].values - fbar) / osc
    m0, f0, y0 = cvn.deletion(2, X, y, th, d["track"].values)
    np.testing.assert_allclose(rows["f*"].values, m0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(rows["y_var"].values, y0, rtol=0, atol=1e-12)
    # in raw units: the held-out residuals are of the size of the predictive standard deviation, not of the offset 40
    resid = rows["z"].values - (rows["f_bar"].values + osc * rows["f*"].values)
    assert np.abs(resid).max() < 8 * osc * np.sqrt(rows["y_var"].values.max())


def test_missing_by_value_is_never_held_out():
    loc, data, model, pred, df = _configs()
    df = df.copy()
    df["track"] = df["track"].astype(float)
    df.loc[df.index[::9], "track"] = np.nan
    data = dict(data, data_source=df)
    out = BatchedLocalExpertOI(loc, data, model, pred, engine=OracleCvEngine(), dtype="f64", cv={"by": ["track"]}).run(None, optimise=False)
    cvp, rd = out["cv_preds"], out["run_details"]
    na = np.isnan(cvp["track"].values)
    assert na.any() and np.isnan(cvp["f*"].values[na]).all() and np.isfinite(cvp["f*"].values[~na]).all()
    assert int(rd["cv_rows_skipped"].sum()) == int(na.sum())


def test_engine_refuses_labels_outside_int32():
    from gpsat_amd.engine import Engine, GpsatError
    e = Engine.__new__(Engine)           # no device: the check comes before any library call
    e._lib = L.load()
    e._h = None
    kw = dict(D=1, obs_off=[0, 2], X=np.zeros((2, 1)), y=np.zeros(2), pred_off=[0, 0], Xs=np.zeros((0, 1)), theta0=np.ones((1, 3)),
              optimiser="none", dtype="f64")
    with pytest.raises(GpsatError, match="int32"):
        e.fit_predict_batch(cv_fold=np.array([2 ** 31, 0], dtype=np.int64), **kw)
    with pytest.raises(GpsatError, match="integer labels"):
        e.fit_predict_batch(cv_fold=np.array([0.5, 1.0]), **kw)
