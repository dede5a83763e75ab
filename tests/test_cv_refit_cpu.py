"""No GPU: refitted cross-validation (gpsat_fit_predict_batch_cv_refit) -- the fold count of the C ABI, the host tables under
the host sanitizers, the refusals of the Python layers, and the orchestrator's ``cv_preds`` / ``cv_params`` with a stub
engine that refits with the oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

from gpsat_amd import _lib as L
from gpsat_amd.engine import BatchResult, Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
from oracle import gp_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# labels with gaps, a -1 row, a one-row fold, a fold that is the whole tile, an empty tile, equal labels in two tiles
CASES = {
    "gaps, -1, one row": ([0, 9], [40, 7, 40, -1, 1000, 40, 7, 2 ** 31 - 1, 40]),
    "whole tile": ([0, 4], [5, 5, 5, 5]),
    "empty tile between": ([0, 3, 3, 6], [1, 0, 1, 0, 0, 0]),
    "equal labels in two tiles": ([0, 4, 9], [3, 8, 3, 8, 8, 3, -7, 3, 11]),
    "nothing held out": ([0, 2], [-1, -2]),
    "no tiles": ([0], []),
}


def numpy_count(obs_off, lab):
    """gpsat_cv_refit_count restated: folds per tile, sum over folds of N - g, and per fold (label, rows left)."""
    lab = np.asarray(lab, dtype=np.int64)
    fold_off, rows, folds = [0], 0, []
    for a, b in zip(obs_off[:-1], obs_off[1:]):
        vals, cnt = np.unique(lab[a:b][lab[a:b] >= 0], return_counts=True)
        fold_off.append(fold_off[-1] + len(vals))
        rows += int(((b - a) - cnt).sum())
        folds += [(int(v), int(b - a - c)) for v, c in zip(vals, cnt)]
    return np.array(fold_off, dtype=np.int64), rows, folds


@pytest.mark.parametrize("case", list(CASES))
def test_cv_refit_count_matches_numpy(case):
    obs_off, lab = CASES[case]
    lib = L.load()
    off = np.array(obs_off, dtype=np.int64)
    labels = np.array(lab, dtype=np.int32)
    T = len(off) - 1
    fold_off = np.full(T + 1, -1, dtype=np.int64)
    rows = C.c_int64(-1)
    assert lib.gpsat_cv_refit_count(T, _ptr(off), _ptr(labels), _ptr(fold_off), C.byref(rows)) == 0
    want_off, want_rows, _ = numpy_count(obs_off, lab)
    np.testing.assert_array_equal(fold_off, want_off)
    assert rows.value == want_rows


def test_cv_refit_count_refuses_bad_arguments():
    lib = L.load()
    off, lab, fo, rows = np.array([0, 2], dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64), C.c_int64(0)
    assert lib.gpsat_cv_refit_count(1, _ptr(off), None, _ptr(fo), C.byref(rows)) == -1 and b"fold is NULL" in lib.gpsat_last_error()
    assert lib.gpsat_cv_refit_count(1, None, _ptr(lab), _ptr(fo), C.byref(rows)) == -1 and b"obs_off" in lib.gpsat_last_error()
    assert lib.gpsat_cv_refit_count(1, _ptr(off), _ptr(lab), None, C.byref(rows)) == -1 and b"fold_off" in lib.gpsat_last_error()
    bad = np.array([0, 3, 2], dtype=np.int64)
    assert lib.gpsat_cv_refit_count(2, _ptr(bad), _ptr(lab), _ptr(np.zeros(3, dtype=np.int64)), C.byref(rows)) == -1
    assert b"non-decreasing" in lib.gpsat_last_error()


def test_symbols_and_struct_layout():
    lib = L.load()
    assert hasattr(lib, "gpsat_cv_refit_count") and hasattr(lib, "gpsat_fit_predict_batch_cv_refit")
    assert lib.gpsat_version() == 4
    # gpsat_cv_refit: pointer, three int32 (+ padding), twelve pointers, eight reserved words
    assert C.sizeof(L.GpsatCvRefit) == 8 + 16 + 12 * 8 + 32
    assert L.GpsatCvRefit.fold_off.offset == 24 and L.GpsatCvRefit.fold_label.offset == 112


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/cvfold_host_check.cpp with the host table builder, built with the address and undefined-behaviour sanitizers."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("cvfold") / "cvfold_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gpsat_amd", "csrc"),
           os.path.join(ROOT, "tests", "cvfold_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip(f"{cxx} has no sanitizer runtime: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("min_obs", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_host_tables_under_sanitizers(host_check, case, min_obs):
    obs_off, lab = CASES[case]
    r = subprocess.run([host_check, str(min_obs), str(len(obs_off) - 1)] + [str(v) for v in obs_off] + [str(v) for v in lab],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr            # a sanitizer report or a failed internal check ends it non-zero
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines()}
    want_off, want_rows, folds = numpy_count(obs_off, lab)
    assert out["fold_off"] == want_off.tolist() and out["expanded_rows"] == [want_rows]
    assert out["fold_label"] == [f[0] for f in folds] and out["fold_n_obs"] == [f[1] for f in folds]
    fitted = [f[1] >= max(min_obs, 1) for f in folds]
    assert [d >= 0 for d in out["derived"]] == fitted
    assert out["d_obs_off"] == np.concatenate([[0], np.cumsum([f[1] for f, ok in zip(folds, fitted) if ok])]).astype(int).tolist()


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_engine_refusals():
    e = Engine.__new__(Engine)           # no device: the checks come before any library call
    e._lib = L.load()
    e._h = None
    kw = dict(D=1, obs_off=[0, 2], X=np.zeros((2, 1)), y=np.zeros(2), pred_off=[0, 0], Xs=np.zeros((0, 1)), theta0=np.ones((1, 3)),
              optimiser="none", dtype="f64")
    lab = np.array([0, 1], dtype=np.int32)
    with pytest.raises(GpsatError, match="cv_refit is not built for cv_fold='loo'"):
        e.fit_predict_batch(cv_fold="loo", cv_refit=True, **kw)
    with pytest.raises(GpsatError, match="cv_refit and n_starts"):
        e.fit_predict_batch(cv_fold=lab, cv_refit=True, n_starts=2, **kw)
    with pytest.raises(GpsatError, match="cv_refit and full_cov"):
        e.fit_predict_batch(cv_fold=lab, cv_refit=True, full_cov=True, **kw)
    with pytest.raises(GpsatError, match="cv_fold is None"):
        e.fit_predict_batch(cv_refit=True, **kw)
    with pytest.raises(GpsatError, match="start must be 'theta0' or 'full'"):
        e.fit_predict_batch(cv_fold=lab, cv_refit={"start": "best"}, **kw)
    with pytest.raises(GpsatError, match="unknown keys \\['restarts'\\]"):
        e.fit_predict_batch(cv_fold=lab, cv_refit={"restarts": 2}, **kw)
    with pytest.raises(GpsatError, match="integer labels"):
        e.fit_predict_batch(cv_fold=np.array([0.5, 1.0]), cv_refit=True, **kw)


# ------------------------------------------------------------------------------------------------------------------
# orchestrator, with an engine stand-in that refits with the oracle
# ------------------------------------------------------------------------------------------------------------------
class OracleRefitEngine:
    """Engine stand-in (tests only): the fp64 oracle for the batch and, for ``cv_refit``, for every fold again without its
    rows, as gpsat_fit_predict_batch_cv_refit defines it."""
    device_name = "cpu-oracle (tests only)"
    device_id = 0

    def __init__(self):
        self.refit_calls, self.seen = 0, []

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, trainable, kernel, optimiser, max_iter,
                          dtype="f64", cv_fold=None, cv_refit=None, **kw):
        kid = go.KERNEL_IDS[kernel]
        X, y, Xs = X.astype(np.float64), y.astype(np.float64), Xs.astype(np.float64)
        tr = np.asarray(trainable, bool)
        o = go.fit_predict_batch(kid, D, obs_off, X, y, pred_off, Xs, theta0, lo, hi, tr, max_iter=max_iter, optimise=optimiser != "none")
        res = dict(theta=o["theta"], nll=o["nll"], status=np.where(o["success"], 0, 1).astype(np.int32), n_eval=o["n_eval"].astype(np.int32),
                   f_mean=o["f_mean"], f_var=o["f_var"], y_var=o["y_var"])
        if cv_refit is None:
            assert cv_fold is None
            return BatchResult(**res)
        self.refit_calls += 1
        self.seen.append(dict(cv_refit))
        lab = np.asarray(cv_fold)
        T, H = len(obs_off) - 1, D + 2
        cv = np.full((3, int(obs_off[-1])), np.nan)
        fold_off, per = [0], []
        for t in range(T):
            a, b = int(obs_off[t]), int(obs_off[t + 1])
            for v in np.unique(lab[a:b][lab[a:b] >= 0]):
                G = lab[a:b] == v
                n_left = int((~G).sum())
                if n_left < max(int(cv_refit["min_obs"]), 1):
                    per.append([np.nan] * H + [np.nan, 4, n_left, np.nan, v])
                    continue
                shift = float(y[a:b][~G].mean()) if cv_refit["recentre"] else 0.0
                th0 = o["theta"][t] if cv_refit["start"] == "full" else np.asarray(theta0)[t]
                f = go.fit_predict_batch(kid, D, np.array([0, n_left]), X[a:b][~G], y[a:b][~G] - shift, np.array([0, int(G.sum())]),
                                         X[a:b][G], th0[None], np.asarray(lo)[t][None], np.asarray(hi)[t][None], tr,
                                         max_iter=max_iter, optimise=optimiser != "none")
                cv[:, a:b][:, G] = np.stack([f["f_mean"] + shift, f["f_var"], f["y_var"]])
                per.append(list(f["theta"][0]) + [float(f["nll"][0]), 0 if f["success"][0] else 1, n_left, shift, v])
            fold_off.append(len(per))
        per = np.array(per, dtype=np.float64).reshape(-1, H + 5)
        return BatchResult(**res, cv_mean=cv[0], cv_f_var=cv[1], cv_y_var=cv[2], cv_fold_off=np.array(fold_off, dtype=np.int64),
                           cv_theta=per[:, :H], cv_nll=per[:, H], cv_status=per[:, H + 1].astype(np.int32),
                           cv_n_eval=np.zeros(len(per), np.int32), cv_n_iter=np.zeros(len(per), np.int32),
                           cv_n_obs=per[:, H + 2].astype(np.int32), cv_shift=per[:, H + 3], cv_label=per[:, H + 4].astype(np.int32))


def _configs(n_track=5, obs_scale=None, offset=0.0):
    rng = np.random.default_rng(0)
    n = 260
    df = pd.DataFrame({"x": rng.uniform(0, 10, n), "y": rng.uniform(0, 10, n), "t": rng.integers(0, 3, n).astype(float),
                       "track": rng.integers(0, n_track, n)})
    df["z"] = offset + np.sin(df["x"]) + 0.1 * rng.standard_normal(n)
    xl = pd.DataFrame([(x, y, t) for t in (0.0, 1.0) for x in (2.5, 7.5) for y in (3.0, 7.0)], columns=["x", "y", "t"])
    data = {"data_source": df, "obs_col": "z", "coords_col": ["x", "y", "t"],
            "local_select": [{"col": "t", "comp": "<=", "val": 1}, {"col": "t", "comp": ">=", "val": -1},
                             {"col": ["x", "y"], "comp": "<", "val": 4.0}]}
    init = {"kernel": "Matern32", "obs_mean": "local", "coords_scale": [2.0, 2.0, 1.0]}
    if obs_scale is not None:
        init["obs_scale"] = obs_scale
    model = {"oi_model": "HipGPRModel", "init_params": init,
             "constraints": {"lengthscales": {"low": [0.1, 0.1, 0.1], "high": [20, 20, 20]}}, "optim_kwargs": {"max_iter": 4}}
    return {"source": xl}, data, model, {"method": "expert_loc"}, df


def test_orchestrator_refusals():
    loc, data, model, pred, _ = _configs()
    eng = OracleRefitEngine()
    with pytest.raises(NotImplementedError, match="fp64 only.*'f32'"):            # without "refit": as ever
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f32", cv={"by": ["track"]})
    with pytest.raises(NotImplementedError, match="fp64 only.*'f32'"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f32", cv={"by": ["track"], "refit": False})
    for dt in ("f32", "f64"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype=dt, cv={"by": ["track"], "refit": True, "start": "full"})
    with pytest.raises(NotImplementedError, match="refit is not built for leave-one-out"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": "loo", "refit": True})
    with pytest.raises(NotImplementedError, match="refit is not built for leave-one-out"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"refit": True})
    with pytest.raises(ValueError, match="start must be"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True, "start": "warm"})
    with pytest.raises(ValueError, match="cv must be"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True, "folds": 3})
    with pytest.raises(ValueError, match="cv must be"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"], "start": "full"})
    sg = dict(model, oi_model="HipSGPRModel", init_params=dict(model["init_params"], num_inducing_points=20))
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(loc, data, sg, pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True})
    with pytest.raises(NotImplementedError, match="oi_model 'sklearnGPRModel'"):
        BatchedLocalExpertOI(loc, data, dict(model, oi_model="sklearnGPRModel"), pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True})
    fc = dict(model, pred_kwargs={"full_cov": True})
    with pytest.raises(NotImplementedError, match="full_cov"):
        BatchedLocalExpertOI(loc, data, fc, pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True})
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"], "refit": True})
    with pytest.raises(NotImplementedError, match="sharded"):
        oi.run(None, world_size=2)


def test_cv_preds_and_cv_params_tables(tmp_path):
    """Units with obs_mean="local" and obs_scale: the observation is f_bar + obs_scale f*, with cv_preds' f_bar the tile's
    and cv_params' f_bar the fold's own.  Checked per fold against an oracle refit made here from the raw frame."""
    osc, start = 2.5, "full"
    loc, data, model, pred, df = _configs(n_track=3, obs_scale=osc, offset=40.0)
    eng = OracleRefitEngine()
    cv = {"by": ["track"], "refit": True, "start": start}
    store = str(tmp_path / "s")
    min_obs = 45             # tiles hold 66 .. 117 rows; three folds leave fewer than 45
    out = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv=cv).run(store, store_every=3, min_obs=min_obs)
    assert all(s == {"start": start, "recentre": True, "min_obs": min_obs} for s in eng.seen) and eng.refit_calls >= 3
    cvp, par, rd = out["cv_preds"], out["cv_params"], out["run_details"]
    assert list(cvp.columns) == ["_dim_0", "obs_index", "track", "pred_loc_x", "pred_loc_y", "pred_loc_t", "z", "f*", "f*_var", "y_var", "f_bar"]
    assert list(par.columns) == ["track", "num_obs", "lengthscales_0", "lengthscales_1", "lengthscales_2", "kernel_variance",
                                 "likelihood_variance", "objective_value", "optimise_success", "f_bar"]
    assert list(par.index.names) == ["x", "y", "t"] and len(cvp) == int(rd["num_obs"].sum())
    cs = np.array(model["init_params"]["coords_scale"], dtype=np.float64)
    n_skipped_folds = 0
    for key in rd.index[rd["num_obs"] >= min_obs]:
        rows, prm = cvp.loc[[key]], par.loc[[key]]
        d = df.iloc[rows["obs_index"].values]
        tile_mean = float(d["z"].mean())
        np.testing.assert_allclose(rows["f_bar"].values, tile_mean, rtol=1e-14)
        assert sorted(prm["track"]) == sorted(d["track"].unique())        # one row per fold (in the order of the fold codes)
        th_tile = np.concatenate([out["lengthscales"].loc[[key]].sort_values("_dim_0")["lengthscales"].values,
                                  out["kernel_variance"].loc[[key]]["kernel_variance"].values,
                                  out["likelihood_variance"].loc[[key]]["likelihood_variance"].values]).astype(np.float64)
        skipped = 0
        for _, pr in prm.iterrows():
            G = d["track"].values == pr["track"]
            assert pr["num_obs"] == (~G).sum()
            if (~G).sum() < min_obs:
                n_skipped_folds += 1
                skipped += int(G.sum())
                assert np.isnan(rows["f*"].values[G]).all() and np.isnan(pr["kernel_variance"]) and not pr["optimise_success"]
                continue
            fold_mean = float(d["z"].values[~G].mean())
            np.testing.assert_allclose(pr["f_bar"], fold_mean, rtol=1e-13)
            X, y = d[["x", "y", "t"]].values / cs, (d["z"].values - fold_mean) / osc
            lo = np.array([0.05, 0.05, 0.1, np.nan, np.nan])
            hi = np.array([10.0, 10.0, 20.0, np.nan, np.nan])
            f = go.fit_predict_batch(2, 3, np.array([0, (~G).sum()]), X[~G], y[~G], np.array([0, G.sum()]), X[G], th_tile[None],
                                     lo[None], hi[None], np.ones(5, bool), max_iter=4)
            np.testing.assert_allclose([pr["lengthscales_0"], pr["lengthscales_1"], pr["lengthscales_2"], pr["kernel_variance"],
                                        pr["likelihood_variance"]], f["theta"][0], rtol=1e-6)
            np.testing.assert_allclose(pr["objective_value"], f["nll"][0], rtol=1e-8)
            # raw units both ways: tile f_bar + obs_scale f* (cv_preds) = fold f_bar + obs_scale (the fold's own f*)
            np.testing.assert_allclose(rows["f_bar"].values[G] + osc * rows["f*"].values[G], fold_mean + osc * f["f_mean"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(rows["y_var"].values[G], f["y_var"], rtol=0, atol=1e-8)
        assert rd.loc[key, "cv_rows_skipped"] == skipped
    assert n_skipped_folds > 0, "min_obs is meant to skip some folds here"
    # committed with the waves, and a resumed run adds nothing
    on_disk = get_results(store, expert_order=True)
    assert len(on_disk["cv_preds"]) == len(cvp) and len(on_disk["cv_params"]) == len(par)
    calls = eng.refit_calls
    out2 = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv=cv).run(store, store_every=3, min_obs=min_obs)
    assert eng.refit_calls == calls and len(out2.get("cv_params", [])) == 0
    again = get_results(store, expert_order=True)
    pd.testing.assert_frame_equal(again["cv_params"], on_disk["cv_params"])
    pd.testing.assert_frame_equal(again["cv_preds"], on_disk["cv_preds"])
