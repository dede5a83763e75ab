"""GPU: known noise variances per observation in fp64 (gpsat_fit_predict_batch_noise: K_y = K + sn2 I + diag(v)): fixed
parameters and the full covariance on the bodies this variant shares with the others (tests/variant_cases.py, which states the
bounds), zero and NULL obs_var, a constant and a huge variance, the converged fit, Adam, scikit-learn's fixture, the refusals,
device tensors and the orchestrator.  The large tile, the ragged batch and bit identity are in tests/test_gpu_variants.py.

The converged fit is held to nll 5e-5 and theta rtol 2e-3 (tests/test_noise_cpu.py shows SciPy reproducing itself to a
tenth of that on the same inputs); the scikit-learn fixture to the reference's 1e-6.
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
from variant_cases import check_fixed_parameters, check_full_cov, eng, eng8, FIELDS, KERNELS, NOISE as CASE, ragged_inputs, run, same as _same  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

_run, _batch, _theta = functools.partial(run, CASE), CASE.batch, CASE.theta


# ---- 1. fixed theta against variant_numpy, and the full covariance: the shared bodies of tests/variant_cases.py
@pytest.mark.parametrize("i,N,P,D", [(i, *s) for i, s in enumerate(CASE.SHAPES)])
def test_objective_gradient_predict_at_fixed_parameters(eng, i, N, P, D):
    """Three tiles; the kernels take turns over the shapes (each at least once)."""
    check_fixed_parameters(CASE, eng, KERNELS[i % 4], N, P, D, N, None, f"4-wave {KERNELS[i % 4]}")


@pytest.mark.parametrize("i,N,P,D", [(i, *s) for i, s in enumerate(CASE.SHAPES)])
def test_fixed_parameters_on_the_eight_wave_build(eng8, i, N, P, D):
    check_fixed_parameters(CASE, eng8, KERNELS[(i + 2) % 4], N, P, D, N, None, f"8-wave, one workgroup per CU, {KERNELS[(i + 2) % 4]}",
                           eight_wave=True)


@pytest.mark.parametrize("D", CASE.cov_D)
def test_full_cov_at_fixed_parameters(eng, D):
    check_full_cov(CASE, eng, D)


# ---- 2. v = 0 and a NULL obs_var are gpsat_fit_predict_batch
@pytest.mark.parametrize("optimiser,max_iter", [("lbfgs", 5), ("none", 0)])
def test_zero_variances_and_null_return_the_bytes_of_the_plain_call(eng, monkeypatch, optimiser, max_iter):
    b, th = ragged_inputs(CASE)
    kw = dict(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th,
              kernel=b["kernel"], dtype="f64", optimiser=optimiser, max_iter=max_iter, want_grad=True)
    plain = eng.fit_predict_batch(**kw)
    zeros = eng.fit_predict_batch(obs_var=np.zeros(int(b["obs_off"][-1])), **kw)
    _same(zeros, plain, "v = 0")
    covp = eng.fit_predict_batch(full_cov=True, **kw)
    covz = eng.fit_predict_batch(full_cov=True, obs_var=np.zeros(int(b["obs_off"][-1])), **kw)
    _same(covz, covp, "v = 0, full covariance", FIELDS + ("f_cov",))
    calls = []

    def through_noise(h, bp):
        nz = L.GpsatNoise()                                  # obs_var NULL
        calls.append(1)
        return eng._lib.gpsat_fit_predict_batch_noise(h, bp, C.byref(nz))

    class Lib:
        """The engine's library with gpsat_fit_predict_batch routed through the new entry point."""
        def __getattr__(self, name):
            return through_noise if name == "gpsat_fit_predict_batch" else getattr(lib0, name)

    lib0 = eng._lib
    monkeypatch.setattr(eng, "_lib", Lib())
    routed = eng.fit_predict_batch(**kw)
    monkeypatch.undo()
    assert calls == [1]
    _same(routed, plain, "NULL obs_var")


# ---- 3. a constant v is a larger likelihood variance
def test_constant_variance_is_the_plain_call_at_a_larger_likelihood_variance(eng):
    """v = 0.2 everywhere at a given sn2: objective, gradient and predictions of the plain call at sn2 + 0.2, at the bounds
    (not bitwise: (k + sn2) + 0.2 and k + (sn2 + 0.2) round differently)."""
    T, N, P, D = 3, 150, 16, 3
    b = _batch(T, N, P, D, "Matern52", 4100)
    b["obs_var"] = np.full(T * N, 0.2)
    th = _theta(np.random.default_rng(41), T, D)
    th2 = th.copy()
    th2[:, D + 1] += 0.2
    r, r0 = _run(eng, b, th), _run(eng, b, th2, obs_var=None)
    for t in range(T):
        assert abs(r.nll[t] - r0.nll[t]) <= 1e-9 * max(1.0, abs(r0.nll[t])) * N
        np.testing.assert_allclose(r.grad[t], r0.grad[t], rtol=1e-7, atol=1e-8 * (np.abs(r0.grad[t]).max() + 1))
    ymax = np.abs(b["y"]).max()
    np.testing.assert_allclose(r.f_mean, r0.f_mean, rtol=0, atol=1e-9 * max(ymax, 1.0))
    np.testing.assert_allclose(r.f_var, r0.f_var, rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.y_var, r0.y_var - 0.2, rtol=0, atol=1e-10)       # a new point carries sn2 only


# ---- 4. each row meets its own variance
@pytest.mark.parametrize("N,D", [(17, 1), (100, 3), (500, 4)])
def test_a_huge_variance_deletes_the_row(eng, N, D):
    """v = 1e12 on every fifth row: f* and f*_var of the tile with these rows deleted, to 1e-9 and 1e-10 (on the CPU the two
    differ by at most 1.3e-13, tests/test_noise_cpu.py)."""
    X, y, Xs, theta = syn.make_tile(40 + N, N, 9, D, kid=2)
    v = np.zeros(N)
    v[::5] = 1e12
    keep = v == 0.0
    b = dict(D=D, kernel="Matern32", obs_off=np.array([0, N]), pred_off=np.array([0, 9]), X=X, y=y, Xs=Xs, obs_var=v)
    b0 = dict(D=D, kernel="Matern32", obs_off=np.array([0, int(keep.sum())]), pred_off=np.array([0, 9]), X=X[keep], y=y[keep], Xs=Xs)
    r, r0 = _run(eng, b, theta[None, :]), _run(eng, b0, theta[None, :])
    print("N", N, "D", D, "mean", np.abs(r.f_mean - r0.f_mean).max(), "var", np.abs(r.f_var - r0.f_var).max())
    assert r.status[0] == 5 and r0.status[0] == 5
    np.testing.assert_allclose(r.f_mean, r0.f_mean, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r.f_var, r0.f_var, rtol=0, atol=1e-10)
    # and against the restatement of the reduced tile
    f, fv, _ = vn.predict(vn.NOISE, "Matern32", X[keep], y[keep], Xs, theta, np.zeros(int(keep.sum())))
    np.testing.assert_allclose(r.f_mean, f, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r.f_var, fv, rtol=0, atol=1e-10)


# ---- 5. a converged fit
@pytest.fixture(scope="module")
def fit_case():
    b, th0, lo, hi = vn.fit_case()
    ref = [vn.fit(vn.NOISE, "Matern32", b["X"][150 * t:150 * (t + 1)], b["y"][150 * t:150 * (t + 1)], th0[t], lo[t], hi[t], max_iter=1000,
                  obs_var=b["obs_var"][150 * t:150 * (t + 1)]) for t in range(3)]
    return b, th0, lo, hi, ref


def test_learned_hyperparameters_match_scipy(eng, fit_case):
    b, th0, lo, hi, ref = fit_case
    T, D = 3, b["D"]
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="lbfgs", max_iter=1000, want_grad=True)
    assert all(res.success for _, _, res in ref)
    o_theta, o_nll = np.array([th for th, _, _ in ref]), np.array([f for _, f, _ in ref])
    print("device theta", r.theta, "nll", r.nll, "status", r.status, "n_eval", r.n_eval, "grad", r.grad)
    print("scipy  theta", o_theta, "nll", o_nll)
    assert (r.status == 0).all(), r.status
    np.testing.assert_allclose(r.nll, o_nll, rtol=0, atol=5e-5)
    np.testing.assert_allclose(r.theta, o_theta, rtol=2e-3)
    for t in range(T):
        sl = slice(150 * t, 150 * (t + 1))
        # the returned objective is the objective at the returned parameters
        assert abs(vn.nll_and_grad(vn.NOISE, "Matern32", b["X"][sl], b["y"][sl], r.theta[t], b["obs_var"][sl], want_grad=False)[0] - r.nll[t]) \
            <= 1e-9 * max(1.0, abs(r.nll[t])) * 150
    # v is part of the fit: without it the likelihood variance comes out larger
    rp = _run(eng, b, th0, lo=lo, hi=hi, optimiser="lbfgs", max_iter=1000, obs_var=None)
    assert (rp.theta[:, D + 1] > r.theta[:, D + 1]).all()


def test_adam(eng, fit_case):
    """GPSAT_OPT_ADAM is not refused: 30 steps, the objective falls, and the result is the noise model's."""
    b, th0, lo, hi, _ = fit_case
    r0 = _run(eng, b, th0, lo=lo, hi=hi)
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="adam", max_iter=30, adam_lr=0.05)
    assert (r.status == 1).all() and (r.nll < r0.nll).all()
    for t in range(3):
        sl = slice(150 * t, 150 * (t + 1))
        assert abs(vn.nll_and_grad(vn.NOISE, "Matern32", b["X"][sl], b["y"][sl], r.theta[t], b["obs_var"][sl], want_grad=False)[0] - r.nll[t]) \
            <= 1e-9 * max(1.0, abs(r.nll[t])) * 150


# ---- 6. the scikit-learn fixture through the model
def _fixture_model(eng, golden_dir):
    from gpsat_amd.models import HipGPRModel
    g = np.load(os.path.join(golden_dir, "kat_sklearn_noise.npz"))
    m = HipGPRModel(coords=g["x_train"][:, None], obs=g["y_train"], obs_var=g["obs_var"], engine=eng, dtype="f64", kernel="Matern32",
                    noise_variance=float(g["eps"]) ** 2)
    return g, m


def test_sklearn_fixture_at_the_stored_parameters(eng, golden_dir):
    """The reference's tolerance for its own sklearn test: 1e-6."""
    g, m = _fixture_model(eng, golden_dir)
    m.set_parameters(lengthscales=float(g["ls"]))
    out = m.predict(coords=np.array([[float(g["x_test"])]]))
    lml = -m.get_objective_function_value()
    print("LML", lml, float(g["ml"]), "f*", out["f*"][0], float(g["pred_mean"]), "f*_var", out["f*_var"][0], float(g["pred_std"]) ** 2)
    assert abs(lml - float(g["ml"])) < 1e-6
    assert abs(out["f*"][0] - float(g["pred_mean"])) < 1e-6
    assert abs(out["f*_var"][0] - float(g["pred_std"]) ** 2) < 1e-6
    assert out["y_var"][0] == out["f*_var"][0] + float(g["eps"]) ** 2


def test_sklearn_fixture_optimised_on_the_device(eng, golden_dir):
    g, m = _fixture_model(eng, golden_dir)
    ok = m.optimise_parameters(fixed_params=["kernel_variance", "likelihood_variance"])
    p = m.get_parameters()
    lml = -m.get_objective_function_value()
    print("fitted", p, "LML", lml, "stored", float(g["ls"]), float(g["ml"]))
    assert ok
    assert p["kernel_variance"] == 1.0 and p["likelihood_variance"] == pytest.approx(1e-4)
    assert abs(lml - float(g["ml"])) < 1e-6


# ---- 7. what the C ABI refuses, and that the handle works afterwards
def test_refusals_leave_the_handle_usable(eng):
    b = _batch(2, 40, 5, 3, "Matern32", 1)
    th = _theta(np.random.default_rng(0), 2, 3)
    good = _run(eng, b, th)
    lib = eng._lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(D=3, kernel=2, dtype=L.F64, reserved=None, v=None, null=False):
        T, H = 2, D + (3 if kernel == L.KERNEL_RQ else 2)
        obs_off, pred_off = np.array([0, 8, 13], dtype=np.int64), np.array([0, 0, 0], dtype=np.int64)
        X = np.ascontiguousarray(np.random.default_rng(1).uniform(size=(13, D)), dtype=np.float32 if dtype == L.F32 else np.float64)
        y = np.zeros(13, dtype=X.dtype)
        par, nan, tr = np.ones((T, H)), np.full((T, H), np.nan), np.ones(H, dtype=np.uint8)
        out = dict(theta=np.zeros((T, H)), nll=np.zeros(T), status=np.zeros(T, np.int32), n_eval=np.zeros(T, np.int32))
        fm = np.zeros(1, dtype=X.dtype)
        bt = L.GpsatBatch()
        bt.T, bt.D, bt.dtype, bt.kernel, bt.memory, bt.optimiser = T, D, dtype, kernel, L.MEM_HOST, L.OPT_NONE
        bt.obs_off, bt.pred_off, bt.theta0, bt.lo, bt.hi, bt.trainable = p(obs_off), p(pred_off), p(par), p(nan), p(nan), p(tr)
        bt.X, bt.y, bt.Xs = p(X), p(y), p(X)
        bt.theta, bt.nll, bt.status, bt.n_eval = p(out["theta"]), p(out["nll"]), p(out["status"]), p(out["n_eval"])
        bt.f_mean, bt.f_var, bt.y_var = p(fm), p(fm), p(fm)
        v = np.full(13, 0.1) if v is None else v
        nz = L.GpsatNoise()
        nz.obs_var = p(v)
        if reserved is not None:
            nz.reserved[reserved] = 1
        rc = lib.gpsat_fit_predict_batch_noise(eng._h, C.byref(bt), None if null else C.byref(nz))
        return rc, lib.gpsat_last_error().decode(), out

    rc, _, out = call()                                    # the straight call works
    assert rc == 0 and (out["status"] == 5).all()
    bad_v = np.full(13, 0.1)
    bad_v[10] = -1.0
    nan_v = np.full(13, 0.1)
    nan_v[3] = np.nan
    for kw, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(kernel=L.KERNEL_RQ), "GPSAT_KERNEL_RQ"), (dict(null=True), "noise is NULL"),
                      (dict(reserved=0), "reserved"), (dict(reserved=7), "reserved"), (dict(v=bad_v), "tile 1, row 2"),
                      (dict(v=nan_v), "tile 0, row 3")):
        rc, why, _ = call(**kw)
        assert rc == -1 and match in why, (kw, rc, why)
        _same(_run(eng, b, th), good, f"after the refusal {match!r}")
    # through the Python wrapper: refused before the library for fp32, and a wrong length
    with pytest.raises(GpsatError, match="f32"):
        eng.fit_predict_batch(D=3, obs_off=b["obs_off"], X=b["X"].astype(np.float32), y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"],
                              theta0=th, kernel="Matern32", dtype="f32", optimiser="none", obs_var=b["obs_var"])
    with pytest.raises(GpsatError, match="tile 1, row 0") as ei:
        w = b["obs_var"].copy()
        w[40] = -0.5
        _run(eng, b, th, obs_var=w)
    assert "(-1)" in str(ei.value)
    _same(_run(eng, b, th), good, "after the wrapper's refusals")


def test_device_tensors(eng):
    """obs_var as a device tensor beside device X, y, Xs: the bits of the host call."""
    import torch
    b = _batch(3, [40, 0, 77], [5, 3, 9], 3, "Matern32", 11)
    th = _theta(np.random.default_rng(3), 3, 3)
    host = _run(eng, b, th, want_grad=False)
    dev = torch.device("cuda", eng.device_id)
    X, y, Xs, v = (torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("X", "y", "Xs", "obs_var"))
    r = eng.fit_predict_batch(D=3, obs_off=b["obs_off"], X=X, y=y, pred_off=b["pred_off"], Xs=Xs, theta0=th, kernel="Matern32",
                              dtype="f64", optimiser="none", obs_var=v)
    assert r.nll.tobytes() == host.nll.tobytes()
    assert r.f_mean.cpu().numpy().tobytes() == host.f_mean.tobytes() and r.f_var.cpu().numpy().tobytes() == host.f_var.tobytes()


# ---- 8. the model and the orchestrator end to end
def test_orchestrator_tables_equal_the_per_tile_model(eng):
    """Six experts in waves of four, sharing rows: the tables are those of HipGPRModel(obs_var_col=...) run tile by tile."""
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    from gpsat_amd.models import HipGPRModel
    rng = np.random.default_rng(3)
    x = np.sort(np.concatenate([rng.uniform(0.0, 8.0, 160), rng.normal(3.0, 0.3, 60), rng.normal(6.0, 0.2, 50)]))
    var = rng.uniform(0.0, 0.02, len(x))
    var[::7] = 0.0
    df = pd.DataFrame({"x": x, "y": 0.2 * np.sin(1.3 * x) + np.sqrt(var + 0.03 ** 2) * rng.standard_normal(len(x)), "var": var})
    locs, radius = np.linspace(1.0, 7.0, 6), 1.5
    cons = {"lengthscales": {"low": 1e-3, "high": 10.0}}
    optim = {"max_iter": 60}
    pred = pd.DataFrame({"x": np.linspace(0.5, 7.5, 29)})
    ip = {"kernel": "Matern52", "noise_variance": 0.03 ** 2, "obs_scale": 0.5}
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"], "obs_var_col": "var",
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": ip, "constraints": cons, "optim_kwargs": optim},
               pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.0})
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    oi.engine_workers = 1                                    # two small waves: no second engine (stream, workspace) for them
    assert oi.dtype == "f64"
    tabs = oi.run(store_path=None, store_every=4)
    assert len(tabs["run_details"]) == 6
    plain = BatchedLocalExpertOI(engine=eng, dtype="f64", **{**cfg, "data_config": {k: v for k, v in cfg["data_config"].items() if k != "obs_var_col"}})
    plain.engine_workers = 1
    tabs0 = plain.run(store_path=None, store_every=4)
    assert (tabs0["likelihood_variance"]["likelihood_variance"].values != tabs["likelihood_variance"]["likelihood_variance"].values).any()
    for k, loc in enumerate(locs):
        d = df[(df["x"] <= loc + radius) & (df["x"] >= loc - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x"], obs_var_col="var", engine=eng, dtype="f64", **ip)
        m.set_parameter_constraints(cons, move_within_tol=True, tol=1e-2)
        ok = m.optimise_parameters(**optim)
        p = m.get_parameters()
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
