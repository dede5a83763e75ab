"""GPU: RationalQuadratic experts in fp64 (GPSAT_KERNEL_RQ, H = D + 3 with alpha last): fixed parameters and the full covariance
on the bodies this variant shares with the others (tests/variant_cases.py, which states the bounds), scikit-learn's fixture, the
converged fit, the refusals and the orchestrator.  The large tile, the ragged batch and bit identity are in
tests/test_gpu_variants.py.

The converged fit is held to the bounds of tests/test_gpu_parity.py::test_fp64_learned_hyperparameters_match_scipy.
"""
import ctypes as C
import functools
import os

import numpy as np
import pandas as pd
import pytest

import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import GpsatError
from variant_cases import check_fixed_parameters, check_full_cov, eng, eng8, RQ as CASE, run, same as _same  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

KERNEL = vn.RQ_KERNEL
_run = functools.partial(run, CASE)


# ---- 1. fixed theta against variant_numpy, and the full covariance: the shared bodies of tests/variant_cases.py
@pytest.mark.parametrize("alpha", CASE.ALPHAS)
@pytest.mark.parametrize("N,P,D", CASE.SHAPES)
def test_objective_gradient_predict_at_fixed_parameters(eng, N, P, D, alpha):
    check_fixed_parameters(CASE, eng, KERNEL, N, P, D, N + int(10 * alpha), alpha, f"4-wave alpha {alpha}")


@pytest.mark.parametrize("N,P,D", CASE.SHAPES)
def test_fixed_parameters_on_the_eight_wave_build(eng8, N, P, D):
    check_fixed_parameters(CASE, eng8, KERNEL, N, P, D, N + 10, 1.0, "8-wave, one workgroup per CU", eight_wave=True)


@pytest.mark.parametrize("D", CASE.cov_D)
def test_full_cov_at_fixed_parameters(eng, D):
    check_full_cov(CASE, eng, D)


# ---- 2. scikit-learn's fixture through HipGPRModel
def _fixture_model(eng, golden_dir, **kernel_kwargs):
    from gpsat_amd.models import HipGPRModel
    g = np.load(os.path.join(golden_dir, "kat_sklearn_rq.npz"))
    df = pd.DataFrame(data={"x": g["x_train"], "y": g["y_train"]})
    m = HipGPRModel(data=df, obs_col="y", coords_col="x", obs_mean=None, engine=eng, dtype="f64", kernel=KERNEL,
                    kernel_kwargs=kernel_kwargs)
    m.set_parameters(likelihood_variance=float(g["eps"]) ** 2)
    return g, m


def test_sklearn_fixture_at_the_stored_parameters(eng, golden_dir):
    """The reference's tolerance for its own sklearn test: 1e-6."""
    g, m = _fixture_model(eng, golden_dir)
    m.set_parameters(lengthscales=float(g["ls"]), kernel_alpha=float(g["alpha"]))
    out = m.predict(coords=np.array([[float(g["x_test"])]]))
    lml = -m.get_objective_function_value()
    print("LML", lml, float(g["ml"]), "f*", out["f*"][0], float(g["pred_mean"]), "f*_var", out["f*_var"][0], float(g["pred_std"]) ** 2)
    assert abs(lml - float(g["ml"])) < 1e-6
    assert abs(out["f*"][0] - float(g["pred_mean"])) < 1e-6
    assert abs(out["f*_var"][0] - float(g["pred_std"]) ** 2) < 1e-6


def test_sklearn_fixture_optimised_on_the_device(eng, golden_dir):
    g, m = _fixture_model(eng, golden_dir)
    ok = m.optimise_parameters(fixed_params=["kernel_variance", "likelihood_variance"])
    p = m.get_parameters()
    lml = -m.get_objective_function_value()
    print("fitted", p, "LML", lml, "stored", float(g["ls"]), float(g["alpha"]), float(g["ml"]))
    assert ok
    assert p["kernel_variance"] == 1.0 and p["likelihood_variance"] == pytest.approx(1e-4)
    assert abs(lml - float(g["ml"])) < 1e-6


# ---- 3. a converged fit
FIT_SEEDS = (900, 902, 911)          # SciPy reports success on each, at an alpha inside its box (checked on the CPU)


def _fit_tile(seed, N=150, D=3, P=16):
    """Coordinates, prediction points and generating parameters of synthetic.make_tile; y drawn from the RQ prior, alpha = 1."""
    X, _, Xs, tr = syn.make_tile(seed, N, P, D, 0)
    y = vn.rq_prior_draw(np.random.default_rng(1000 + seed), X, tr[:D], tr[D], tr[D + 1], 1.0)
    return X, y - y.mean(), Xs


def test_learned_hyperparameters_match_scipy(eng):
    T, D = len(FIT_SEEDS), 3
    tiles = [_fit_tile(s) for s in FIT_SEEDS]
    b = dict(D=D, kernel=KERNEL, obs_off=np.arange(T + 1) * 150, pred_off=np.arange(T + 1) * 16, X=np.concatenate([t[0] for t in tiles]),
             y=np.concatenate([t[1] for t in tiles]), Xs=np.concatenate([t[2] for t in tiles]))
    lo, hi = CASE.bounds(T, D)                             # alpha in [0.1, 20]
    th0 = np.ones((T, D + 3))
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="lbfgs", max_iter=1000, want_grad=False)
    ref = [vn.fit(vn.RQ, KERNEL, X, y, th0[t], lo[t], hi[t], max_iter=1000) for t, (X, y, _) in enumerate(tiles)]
    assert all(res.success for _, _, res in ref)
    o_theta, o_nll = np.array([th for th, _, _ in ref]), np.array([f for _, f, _ in ref])
    print("device theta", r.theta, "nll", r.nll, "status", r.status, "n_eval", r.n_eval)
    print("scipy  theta", o_theta, "nll", o_nll)
    assert (r.status == 0).all(), r.status
    np.testing.assert_allclose(r.nll, o_nll, rtol=0, atol=5e-5)
    # alpha may lie along a flat direction: it is judged through the objective alone
    np.testing.assert_allclose(r.theta[:, :D + 2], o_theta[:, :D + 2], rtol=2e-3, atol=1e-5)
    assert ((r.theta[:, D + 2] >= 0.1) & (r.theta[:, D + 2] <= 20.0)).all()
    for t, (X, y, _) in enumerate(tiles):                  # the returned objective is the objective at the returned theta
        assert abs(vn.nll_and_grad(vn.RQ, KERNEL, X, y, r.theta[t], want_grad=False)[0] - r.nll[t]) <= 1e-9 * max(1.0, abs(r.nll[t])) * 150


# ---- 4. what the C ABI refuses for this kernel, and that the handle works afterwards
def test_refusals_leave_the_handle_usable(eng):
    b = CASE.batch(2, 40, 5, 3, KERNEL, 1)
    th = CASE.theta(np.random.default_rng(0), 2, 3, 1.0)
    good = _run(eng, b, th)

    def refused(match, e=eng, bb=b, tt=th, **kw):
        with pytest.raises(GpsatError, match=match) as ei:
            kw = {"dtype": "f64", "optimiser": "none", **kw}
            e.fit_predict_batch(D=bb["D"], obs_off=bb["obs_off"], X=bb["X"].astype(np.float32 if kw["dtype"] == "f32" else np.float64),
                                y=bb["y"], pred_off=bb["pred_off"], Xs=bb["Xs"], theta0=tt, kernel=KERNEL, **kw)
        assert "(-1)" in str(ei.value)                     # GPSAT_EINVAL
        _same(_run(eng, b, th), good, f"after the refusal {match!r}")

    refused("GPSAT_F64 only", dtype="f32")
    refused("gpsat_fit_predict_batch_ms", n_starts=1)
    refused("gpsat_fit_predict_batch_cv", cv_fold="loo")
    refused("gpsat_fit_predict_batch_cv_refit", cv_fold=np.arange(80, dtype=np.int32) % 4, cv_refit=True)
    # D = 4 and the sparse entry point have no shape the Python wrapper would lay out: straight through the C ABI
    lib = eng._lib
    T, D, H = 1, 4, 7
    obs_off, pred_off = np.array([0, 8], dtype=np.int64), np.array([0, 0], dtype=np.int64)
    X, y = np.random.default_rng(1).uniform(size=(8, D)), np.zeros(8)
    par, nan, tr = np.ones(H), np.full(H, np.nan), np.ones(H, dtype=np.uint8)
    out = dict(theta=np.zeros(H), nll=np.zeros(1), status=np.zeros(1, np.int32), n_eval=np.zeros(1, np.int32))
    fm = np.zeros(1)
    bt = L.GpsatBatch()
    bt.T, bt.D, bt.dtype, bt.kernel, bt.memory, bt.optimiser = T, D, L.F64, L.KERNEL_RQ, L.MEM_HOST, L.OPT_NONE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bt.obs_off, bt.pred_off, bt.theta0, bt.lo, bt.hi, bt.trainable = p(obs_off), p(pred_off), p(par), p(nan), p(nan), p(tr)
    bt.X, bt.y, bt.Xs = p(X), p(y), p(X)
    bt.theta, bt.nll, bt.status, bt.n_eval = p(out["theta"]), p(out["nll"]), p(out["status"]), p(out["n_eval"])
    bt.f_mean, bt.f_var, bt.y_var = p(fm), p(fm), p(fm)
    assert lib.gpsat_fit_predict_batch(eng._h, C.byref(bt)) == -1
    assert "D <= 3" in lib.gpsat_last_error().decode()
    _same(_run(eng, b, th), good, "after D = 4")
    bt.D = 3
    z_off, Z = np.array([0, 4], dtype=np.int64), np.ascontiguousarray(X[:4, :3])
    sp = L.GpsatSparse()
    sp.z_off, sp.Z, sp.jitter = p(z_off), p(Z), 0.0
    X3 = np.ascontiguousarray(X[:, :3])
    bt.X, bt.Xs = p(X3), p(X3)
    assert lib.gpsat_sgpr_fit_predict_batch(eng._h, C.byref(bt), C.byref(sp)) == -1
    assert "gpsat_sgpr_fit_predict_batch" in lib.gpsat_last_error().decode()
    _same(_run(eng, b, th), good, "after the sparse entry point")
    assert lib.gpsat_n_hyper(L.KERNEL_RQ, 3) == 6 and lib.gpsat_n_hyper(L.KERNEL_RQ, 4) == 0


# ---- 5. the orchestrator end to end
def test_orchestrator_tables_equal_the_per_tile_model(eng, tmp_path):
    """12 experts in waves of 5, the run killed after the first wave and resumed: the tables are those of HipGPRModel run
    tile by tile, kernel_alpha among them."""
    from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
    from gpsat_amd.models import HipGPRModel
    rng = np.random.default_rng(3)
    x = np.sort(rng.uniform(0.0, 14.0, 420))
    df = pd.DataFrame({"x": x, "y": vn.rq_prior_draw(rng, x[:, None], np.array([0.6]), 1.0, 0.05 ** 2, 0.4)})
    locs, radius = np.linspace(1.0, 13.0, 12), 1.5
    cons = {"kernel_alpha": {"low": 0.1, "high": 20.0}, "lengthscales": {"low": 1e-3, "high": 10.0}}
    optim = {"fixed_params": ["likelihood_variance"], "max_iter": 60}
    pred = pd.DataFrame({"x": np.linspace(0.5, 13.5, 53)})
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": {"kernel": KERNEL, "noise_variance": 0.05 ** 2},
                             "constraints": cons, "optim_kwargs": optim},
               pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.0})
    store = str(tmp_path / "store")

    class Stop(Exception):
        pass

    class OneWave:
        """The engine for the first wave only."""
        device_name, device_id = eng.device_name, eng.device_id

        def __init__(self):
            self.n = 0

        def fit_predict_batch(self, **kw):
            self.n += 1
            if self.n > 1:
                raise Stop()
            return eng.fit_predict_batch(**kw)

    oi = BatchedLocalExpertOI(engine=OneWave(), **cfg)
    oi.engine_workers = 1
    with pytest.raises(Stop):
        oi.run(store_path=store, store_every=5)
    assert len(get_results(store)["run_details"]) == 5
    oi2 = BatchedLocalExpertOI(engine=eng, **cfg)
    oi2.engine_workers = 1                                   # two small waves: no second engine (stream, workspace) for them
    assert oi2.dtype == "f64"
    oi2.run(store_path=store, store_every=5)                 # resumes behind the committed wave
    tabs = get_results(store, expert_order=True)
    assert len(tabs["run_details"]) == 12 and len(tabs["kernel_alpha"]) == 12
    for k, loc in enumerate(locs):
        d = df[(df["x"] <= loc + radius) & (df["x"] >= loc - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x"], engine=eng, dtype="f64", kernel=KERNEL, noise_variance=0.05 ** 2)
        m.set_parameter_constraints(cons, move_within_tol=True, tol=1e-2)
        ok = m.optimise_parameters(**optim)
        p = m.get_parameters()
        assert tabs["kernel_alpha"]["kernel_alpha"].values[k] == p["kernel_alpha"]
        assert tabs["lengthscales"]["lengthscales"].values[k] == p["lengthscales"][0]
        assert tabs["kernel_variance"]["kernel_variance"].values[k] == p["kernel_variance"]
        assert tabs["likelihood_variance"]["likelihood_variance"].values[k] == p["likelihood_variance"]
        rd = tabs["run_details"].iloc[k]
        assert rd["optimise_success"] == ok and rd["objective_value"] == m.get_objective_function_value()
        pc = pred["x"].values[(pred["x"].values - loc) ** 2 < 1.0]
        out = m.predict(pc[:, None])
        mine = tabs["preds"][np.isclose(tabs["preds"].index.values, loc)]
        np.testing.assert_array_equal(mine["f*"].values, out["f*"])
        np.testing.assert_array_equal(mine["f*_var"].values, out["f*_var"])
