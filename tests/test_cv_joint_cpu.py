"""The joint log predictive density per held-out fold (cv_joint) without a GPU: the two routes of the NumPy restatement
against each other, the host logic of the three layers with recording stand-ins, and the units of table cv_folds."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import cv_joint_numpy as cjn
import cv_numpy as cvn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd import variants as V
from gpsat_amd.engine import BatchResult, Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel
from test_cv_cpu import OracleCvEngine, _configs
from test_variant_matrix_cpu import _Reached, _RecordingEngine, _RecordingLib, _tile

KID = 2


def _cases():
    rng = np.random.default_rng(3)
    one256 = np.full(300, -1, dtype=np.int32)
    one256[20:276] = 0
    return {"17/1 leave-one-out": (17, 1, None), "33/3 runs of 1-7": (33, 3, cvn.run_labels(33, rng, 1, 7)),
            "150/3 folds of 30": (150, 3, (np.arange(150) // 30).astype(np.int32)),
            "150/3 folds of 30 shuffled": (150, 3, rng.permutation(np.arange(150) // 30).astype(np.int32)),
            "64/4 whole tile": (64, 4, np.zeros(64, dtype=np.int32)), "500/3 runs of 1-64": (500, 3, cvn.run_labels(500, rng, 1, 64)),
            "300/2 one fold of 256": (300, 2, one256)}


@pytest.mark.parametrize("name", list(_cases()))
def test_the_two_routes_agree(name):
    N, D, lab = _cases()[name]
    X, y, _, th = syn.make_tile(700 + N, N, 4, D, KID)
    a, b = cjn.closed_form(KID, X, y, th, lab), cjn.deletion(KID, X, y, th, lab)
    err = cjn.rel_err(a, b)
    print(f"{name}: {len(a)} folds, max |lpd| {np.abs(b).max():.4g}, closed form against deletion {err:.3e}")
    assert np.isfinite(a).all() and np.isfinite(b).all() and len(a) == len(cjn.folds(lab, N))
    assert err <= 1e-12


def test_one_row_folds_are_the_univariate_terms():
    N, D = 60, 3
    X, y, _, th = syn.make_tile(760, N, 0, D, KID)
    mean, _, yvar = cvn.closed_form(KID, X, y, th, None)
    assert cjn.rel_err(cjn.closed_form(KID, X, y, th, None), cjn.univariate(y, mean, yvar)) <= 1e-12


# ---- host logic
def _recording_engine():
    eng = object.__new__(Engine)
    eng._lib, eng._h = _RecordingLib(), None
    return eng


def _engine_kw(dtype="f64", D=2):
    X, y, _ = _tile(D)
    return dict(D=D, obs_off=[0, len(y)], X=X, y=y, pred_off=[0, 3], Xs=X[:3], optimiser="none", dtype=dtype, theta0=np.ones(D + 2))


def test_engine_refusals_and_entry_points():
    eng, lab = _recording_engine(), np.arange(10, dtype=np.int32) % 3
    with pytest.raises(GpsatError, match="cv_joint.*needs cv_fold"):
        eng.fit_predict_batch(cv_joint=True, **_engine_kw())
    with pytest.raises(GpsatError, match="cv_joint with cv_refit is built in fp64 only"):
        eng.fit_predict_batch(cv_joint=True, cv_fold=lab, cv_refit=True, **_engine_kw("f32"))
    with pytest.raises(_Reached, match="gpsat_fit_predict_batch_cv_joint"):
        eng.fit_predict_batch(cv_joint=True, cv_fold="loo", **_engine_kw())
    with pytest.raises(_Reached, match="gpsat_fit_predict_batch_cv$"):
        eng.fit_predict_batch(cv_fold="loo", **_engine_kw())
    assert V.JOINT_ENTRY == {"cv": "gpsat_fit_predict_batch_cv_joint", "cv_refit": "gpsat_fit_predict_batch_cv_refit_joint"}
    assert set(V.JOINT_ENTRY.values()) <= set(L.OPTIONAL_EXPORTS)
    assert C.sizeof(L.GpsatCvJoint) == 2 * C.sizeof(C.c_void_p) + 32


def test_fold_offsets_of_leave_one_out_are_obs_off():
    eng = object.__new__(Engine)
    eng._lib, eng._h = L.get_lib(), None
    obs_off = np.array([0, 5, 5, 12], dtype=np.int64)
    off, rows = eng._cv_fold_off(3, obs_off, None)
    assert (off == obs_off).all() and off is not obs_off and rows is None
    # ... which is what gpsat_cv_refit_count counts for one label per row
    lab = np.concatenate([np.arange(5), np.arange(7)[::-1]]).astype(np.int32)
    off2, rows2 = eng._cv_fold_off(3, obs_off, lab)
    assert (off2 == obs_off).all() and rows2 == 5 * 4 + 7 * 6


def test_the_refit_budget_counts_the_covariances():
    obs_off = np.array([0, 10, 10, 40], dtype=np.int64)
    lab = np.concatenate([np.arange(10) % 2, [-1] * 3, np.arange(27) // 9]).astype(np.int32)
    # tile 0: two folds of 5 -> 50 elements; tile 2: three folds of 9 -> 243
    for D in (1, 3):
        assert list(Engine._joint_cov_rows(D, 3, obs_off, lab)) == [-(-50 // (D + 1)), 0, -(-243 // (D + 1))]


def test_model_refusals_and_keys():
    X, y, _ = _tile(2)
    with pytest.raises(_Reached):
        HipGPRModel(coords=X, obs=y, engine=_RecordingEngine(), dtype="f64").cross_validate(joint=True)

    class Eng(_RecordingEngine):
        def fit_predict_batch(self, **kw):
            assert "cv_joint" not in kw
            N = len(kw["y"])
            return BatchResult(theta=kw["theta0"], nll=np.zeros(1), status=np.array([5]), n_eval=np.ones(1), f_mean=np.zeros(0),
                               f_var=np.zeros(0), y_var=np.zeros(0), cv_mean=np.zeros(N), cv_f_var=np.ones(N), cv_y_var=np.ones(N))

    out = HipGPRModel(coords=X, obs=y, engine=Eng(), dtype="f64").cross_validate(np.arange(len(y)) % 3)
    assert set(out) == {"f*", "f*_var", "y_var", "f_bar"}


def test_orchestrator_refusals():
    loc, data, model, pred, _ = _configs()
    eng = OracleCvEngine()
    with pytest.raises(ValueError, match="cv_joint.*cv"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv_joint=True)
    with pytest.raises(ValueError, match="leave-one-out.*marginal.*cv_scores"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv="loo", cv_joint=True)
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f32", cv={"by": ["track"], "refit": True}, cv_joint=True)
    with pytest.raises(ValueError, match="cv must be"):                       # cv keeps refusing keys it does not know
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"], "joint": True})
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"]}, cv_joint=True)
    assert oi.config["cv_joint"] is True
    assert "cv_joint" not in BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"]}).config


# ---- the covariance offsets of the refit flavour's derived batch, under the host sanitizers
@pytest.fixture(scope="module")
def cov_host_check(tmp_path_factory):
    """tests/cvfold_cov_host_check.cpp, built with the address and undefined-behaviour sanitizers (a program of its own)."""
    import os
    import subprocess
    import test_cv_refit_cpu as tcr
    cxx = tcr._compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("cvfold_cov") / "cvfold_cov_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(tcr.ROOT, "gpsat_amd", "csrc"),
           os.path.join(tcr.ROOT, "tests", "cvfold_cov_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip(f"{cxx} has no sanitizer runtime: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("min_obs", [1, 4])
def test_covariance_offsets_under_sanitizers(cov_host_check, min_obs):
    import subprocess
    import test_cv_refit_cpu as tcr
    for case, (obs_off, lab) in tcr.CASES.items():
        r = subprocess.run([cov_host_check, str(min_obs), str(len(obs_off) - 1)] + [str(v) for v in obs_off] + [str(v) for v in lab],
                           capture_output=True, text=True)
        assert r.returncode == 0, (case, r.stdout + r.stderr)    # a sanitizer report or a failed internal check ends it non-zero
        if r.stdout.startswith("error"):
            continue
        _, _, folds = tcr.numpy_count(obs_off, lab)
        sizes = []
        for t in range(len(obs_off) - 1):
            lt = np.asarray(lab[obs_off[t]:obs_off[t + 1]], dtype=np.int64)
            sizes += list(np.unique(lt[lt >= 0], return_counts=True)[1])
        g = [s for s, f in zip(sizes, folds) if f[1] >= max(min_obs, 1)]
        assert [int(v) for v in r.stdout.split()[1:]] == np.concatenate([[0], np.cumsum(np.square(g))]).astype(int).tolist(), case


# ---- table cv_folds
class JointEngine(OracleCvEngine):
    """... and cv_joint_numpy.closed_form for ``cv_joint``; the calls are recorded."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def fit_predict_batch(self, *, cv_joint=False, **kw):
        r = super().fit_predict_batch(**kw)
        if cv_joint:
            kid, off = cvn.go.KERNEL_IDS[kw["kernel"]], kw["obs_off"]
            parts = [cjn.closed_form(kid, kw["X"][a:b].astype(np.float64), kw["y"][a:b].astype(np.float64), r.theta[t],
                                     np.asarray(kw["cv_fold"])[a:b]) for t, (a, b) in enumerate(zip(off[:-1], off[1:]))]
            r.cv_lpd = np.concatenate(parts)
            r.cv_fold_off = np.concatenate([[0], np.cumsum([len(p_) for p_ in parts])]).astype(np.int64)
            self.seen.append((kw["y"].copy(), np.asarray(kw["cv_fold"]).copy(), off.copy(), r))
        return r


def test_cv_folds_table_and_its_units(tmp_path):
    loc, data, model, pred, df = _configs()
    osc = 0.5
    model = dict(model, init_params=dict(model["init_params"], obs_scale=osc))
    eng = JointEngine()
    base = BatchedLocalExpertOI(loc, data, model, pred, engine=OracleCvEngine(), dtype="f64", cv={"by": ["track"]}).run(None)
    out = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv={"by": ["track"]}, cv_joint=True) \
        .run(str(tmp_path / "s"), store_every=7)
    for name, tab in base.items():                     # every other table as without cv_joint
        pd.testing.assert_frame_equal(out[name].drop(columns=["run_time"], errors="ignore"), tab.drop(columns=["run_time"], errors="ignore"))
    cvf, cvp = out["cv_folds"], out["cv_preds"]
    assert list(cvf.columns) == ["track", "n", "lpd", "lpd_marginal"] and list(cvf.index.names) == ["x", "y", "t"]
    assert int(cvf["n"].sum()) == len(cvp) and np.isfinite(cvf[["lpd", "lpd_marginal"]].values).all()
    # one row per expert and fold, folds in ascending code; n and the by values are those of the expert's cv_preds rows
    for key in cvf.index.unique():
        f, p_ = cvf.loc[[key]], cvp.loc[[key]]
        order = pd.unique(p_["track"])                 # codes ascend with the first appearance in the SELECTED frame, not here
        assert sorted(f["track"]) == sorted(order) and len(f) == len(order)
        for tr, n, lpd_m in zip(f["track"], f["n"], f["lpd_marginal"]):
            g = p_[p_["track"] == tr]
            mean, var = g["f_bar"].values + osc * g["f*"].values, osc * osc * g["y_var"].values
            ref = float(np.sum(-0.5 * (g["z"].values - mean) ** 2 / var - 0.5 * np.log(2.0 * np.pi * var)))
            assert n == len(g) and abs(lpd_m - ref) <= 1e-12 * max(1.0, abs(ref))
    # lpd in raw units = the engine's value - n log(obs_scale): every fold of every call, matched as (n, value) pairs (the
    # calls are not in the order of the table)
    assert len(eng.seen) > 1                           # several calls
    want = []
    for _, lab, off, r in eng.seen:
        for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
            n = np.unique(lab[a:b][lab[a:b] >= 0], return_counts=True)[1]
            dev = r.cv_lpd[r.cv_fold_off[t]:r.cv_fold_off[t + 1]]
            assert len(n) == len(dev)
            want += list(zip(n, dev - n * np.log(osc)))
    assert len(want) == len(cvf)
    want, got = np.array(sorted(want)), np.array(sorted(zip(cvf["n"], cvf["lpd"])))
    assert (want[:, 0] == got[:, 0]).all() and cjn.rel_err(got[:, 1], want[:, 1]) <= 1e-14
    # the joint density and the sum of the marginals are different numbers for correlated rows, equal for one-row folds
    one = cvf["n"] == 1
    assert cjn.rel_err(cvf["lpd"][one], cvf["lpd_marginal"][one]) <= 1e-10
    assert (np.abs(cvf["lpd"][~one] - cvf["lpd_marginal"][~one]) > 1e-6).any()
    # committed with the waves
    from gpsat_amd.local_experts import get_results
    assert len(get_results(str(tmp_path / "s"))["cv_folds"]) == len(cvf)
