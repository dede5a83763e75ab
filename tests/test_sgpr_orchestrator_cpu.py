"""CPU: the batched orchestrator's SGPR wiring (oi_model GPflowSGPRModel / HipSGPRModel) with a NumPy stand-in engine:
routing of the main profile, no error rows for tiles above gpsat_max_tile_obs, the inducing_points table, the ELBO as
objective_value, the dtype rule, the exact-GP replacement for small tiles and the refusals."""
import numpy as np
import pandas as pd
import pytest

import sgpr_numpy as sn
from gpsat_amd import _lib as L
from gpsat_amd.engine import BatchResult
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import select_inducing_points
from oracle import gp_oracle as go


class SparseOracleEngine:
    """Engine stand-in: the NumPy SGPR restatement (sparse calls) and the fp64 oracle (exact calls) behind the packed-batch
    interface, with the engine's host-side centring (test-only)."""
    device_name = "cpu-oracle (tests only)"
    device_id = 0

    def __init__(self):
        self.calls = []

    def sgpr_fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, z_off, Z, theta0, lo, hi, trainable, kernel,
                               optimiser, max_iter, dtype="f64", **kw):
        assert dtype == "f64"
        self.calls.append(dict(kind="sgpr", T=len(obs_off) - 1, obs_off=np.array(obs_off), z_off=np.array(z_off),
                               Z=np.array(Z), X=np.array(X)))
        kid = go.KERNEL_IDS[kernel]
        T, H = len(obs_off) - 1, D + 2
        theta, nll = np.zeros((T, H)), np.zeros(T)
        fm, fv, yv = (np.zeros(pred_off[-1]) for _ in range(3))
        for t in range(T):
            a, b, pa, pb, za, zb = obs_off[t], obs_off[t + 1], pred_off[t], pred_off[t + 1], z_off[t], z_off[t + 1]
            c = X[a:b].mean(0)
            Xt, Zt, Pt = X[a:b] - c, Z[za:zb] - c, Xs[pa:pb] - c
            th = np.array(theta0[t], dtype=np.float64)
            if optimiser != "none":
                th, _, _ = sn.fit_scipy(kid, Xt, y[a:b], Zt, th, lo[t], hi[t], trainable, maxiter=max_iter)
            theta[t], nll[t] = th, -sn.elbo(kid, Xt, y[a:b], Zt, th)
            if pb > pa:
                fm[pa:pb], fv[pa:pb], yv[pa:pb] = sn.predict(kid, Xt, y[a:b], Zt, Pt, th)
        return BatchResult(theta=theta, nll=nll, status=np.zeros(T, np.int32), n_eval=np.ones(T, np.int32),
                           f_mean=fm, f_var=fv, y_var=yv)

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser,
                          max_iter, **kw):
        self.calls.append(dict(kind="exact", T=len(obs_off) - 1, obs_off=np.array(obs_off)))
        o = go.fit_predict_batch(go.KERNEL_IDS[kernel], D, obs_off, np.asarray(X, np.float64), np.asarray(y, np.float64),
                                 pred_off, np.asarray(Xs, np.float64), theta0, lo, hi, np.asarray(trainable, bool),
                                 max_iter=max_iter, optimise=optimiser != "none")
        return BatchResult(theta=o["theta"], nll=o["nll"], status=np.where(o["success"], 0, 1).astype(np.int32),
                           n_eval=o["n_eval"].astype(np.int32), f_mean=o["f_mean"], f_var=o["f_var"], y_var=o["y_var"])


def _data(n=9000, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 10, n)
    x[:300] = rng.uniform(9.0, 10.0, 300)            # a sparse corner: few observations near x = 9.9 ... 10
    x[300:] = rng.uniform(0, 8.0, n - 300)           # dense elsewhere
    return pd.DataFrame({"x": x, "y": np.sin(x) + 0.1 * rng.normal(size=n)})


def _cfg(df, locs, radius, model="GPflowSGPRModel", **extra):
    return dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
                data_config={"data_source": df, "obs_col": "y", "coords_col": ["x"],
                             "local_select": [{"col": "x", "comp": "<=", "val": radius},
                                              {"col": "x", "comp": ">=", "val": -radius}]},
                model_config={"oi_model": model,
                              "init_params": {"kernel": "Matern32", "noise_variance": 0.01, "num_inducing_points": 20,
                                              "inducing_seed": 3, "coords_scale": 2.0},
                              "optim_kwargs": {"max_iter": 30}, **extra},
                pred_loc_config={"method": "expert_loc"})


def test_sgpr_profile_runs_tiles_above_the_exact_limit(tmp_path):
    df = _data()
    locs = [2.0, 4.0, 9.9]
    eng = SparseOracleEngine()
    oi = BatchedLocalExpertOI(engine=eng, **_cfg(df, locs, 2.0))
    assert oi.dtype == "f64"
    tabs = oi.run(store_path=str(tmp_path / "s"))
    rd = tabs["run_details"]
    n_obs = rd["num_obs"].values
    assert n_obs.max() > L.max_tile_obs("f64", 1)                         # tiles the exact path would refuse
    assert rd["objective_value"].notna().all() and rd["optimise_success"].all()   # every expert has a result row
    assert (rd["model"] == "gpsat_amd.models.HipSGPRModel").all()
    assert [c["kind"] for c in eng.calls] == ["sgpr"]
    # inducing_points: the reference's layout, the points HipSGPRModel picks for the same rows (expert index = position)
    ip = tabs["inducing_points"]
    assert list(ip.columns) == ["_dim_0", "_dim_1", "inducing_points"]
    X = df["x"].values
    for e, loc in enumerate(locs):
        rows = np.nonzero((X <= loc + 2.0) & (X >= loc - 2.0))[0]
        Z = select_inducing_points(X[rows][:, None] / 2.0, 20, 3, e)
        got = ip.loc[loc]
        assert got["_dim_0"].tolist() == list(range(len(Z))) and (got["_dim_1"] == 0).all()
        np.testing.assert_array_equal(got["inducing_points"].values, Z[:, 0])
    # the engine saw those same points, and objective_value is the ELBO (not its negative)
    call = eng.calls[0]
    np.testing.assert_array_equal(call["Z"][:, 0], ip["inducing_points"].values)
    th = np.stack([tabs["lengthscales"]["lengthscales"].values, tabs["kernel_variance"]["kernel_variance"].values,
                   tabs["likelihood_variance"]["likelihood_variance"].values], axis=1)
    for t in range(3):
        a, b, za, zb = call["obs_off"][t], call["obs_off"][t + 1], call["z_off"][t], call["z_off"][t + 1]
        yv = df["y"].values[np.nonzero((X <= locs[t] + 2.0) & (X >= locs[t] - 2.0))[0]]
        c = call["X"][a:b].mean(0)
        el = sn.elbo(2, call["X"][a:b] - c, yv, call["Z"][za:zb] - c, th[t])
        assert rd["objective_value"].iloc[t] == pytest.approx(el, rel=1e-12) != -el     # +ELBO, not -ELBO


def test_exact_replacement_for_small_tiles(tmp_path):
    df = _data()
    locs = [4.0, 9.9]                                  # 9.9: only the sparse corner's points within 0.3
    cfg = _cfg(df, locs, 0.3, replacement_threshold=200,
               replacement_init_params={"kernel": "Matern32", "noise_variance": 0.01})
    eng = SparseOracleEngine()
    tabs = BatchedLocalExpertOI(engine=eng, **cfg).run(store_path=str(tmp_path / "s"))
    rd = tabs["run_details"]
    assert rd.loc[9.9, "num_obs"] < 200 <= rd.loc[4.0, "num_obs"]
    assert sorted(c["kind"] for c in eng.calls) == ["exact", "sgpr"]
    assert rd.loc[4.0, "model"].endswith("HipSGPRModel") and rd.loc[9.9, "model"].endswith("HipGPRModel")
    assert tabs["inducing_points"].index.unique().tolist() == [4.0]      # the exact expert has no inducing points
    assert rd["objective_value"].notna().all()


def test_dtype_rule_and_refusals():
    df = _data(2000)
    assert BatchedLocalExpertOI(engine=SparseOracleEngine(), **_cfg(df, [2.0], 1.0, model="HipGPRModel")).dtype == "f32"
    assert BatchedLocalExpertOI(engine=SparseOracleEngine(), **_cfg(df, [2.0], 1.0)).dtype == "f64"
    assert BatchedLocalExpertOI(engine=SparseOracleEngine(), dtype="f64", **_cfg(df, [2.0], 1.0)).dtype == "f64"
    with pytest.raises(NotImplementedError):
        BatchedLocalExpertOI(engine=SparseOracleEngine(), dtype="f32", **_cfg(df, [2.0], 1.0))
    for lp in ({"previous": True}, {"file": "somewhere", "param_names": ["lengthscales", "inducing_points"]},
               {"inducing_points": [[0.0]]}):
        with pytest.raises(NotImplementedError):
            BatchedLocalExpertOI(engine=SparseOracleEngine(), **_cfg(df, [2.0], 1.0, load_params=lp))
    with pytest.raises(NotImplementedError):
        BatchedLocalExpertOI(engine=SparseOracleEngine(), **_cfg(df, [2.0], 1.0, pred_kwargs={"full_cov": True}))
    with pytest.raises(NotImplementedError):                 # inducing points of an exact-GP run
        BatchedLocalExpertOI(engine=SparseOracleEngine(), **_cfg(df, [2.0], 1.0, model="HipGPRModel",
                                                                params_to_store=["inducing_points"]))


def test_hyper_parameters_load_for_sgpr(tmp_path):
    """load_params of the three hyper-parameters works: a predict-only run from the stored optima reproduces them."""
    df = _data(3000)
    cfg = _cfg(df, [2.0, 5.0], 1.0)
    store = str(tmp_path / "s")
    tabs = BatchedLocalExpertOI(engine=SparseOracleEngine(), **cfg).run(store_path=store)
    cfg2 = _cfg(df, [2.0, 5.0], 1.0, load_params={"file": store, "table_suffix": ""})
    tabs2 = BatchedLocalExpertOI(engine=SparseOracleEngine(), **cfg2).run(store_path=str(tmp_path / "s2"), optimise=False)
    np.testing.assert_allclose(tabs2["lengthscales"]["lengthscales"].values, tabs["lengthscales"]["lengthscales"].values)
    np.testing.assert_allclose(tabs2["preds"]["f*"].values, tabs["preds"]["f*"].values, rtol=1e-12, atol=1e-12)
