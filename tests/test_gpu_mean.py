"""GPU: experts with a trainable constant mean in fp64 (gpsat_fit_predict_batch_mean, GPSAT_MEAN_CONSTANT: H = D + 3 with c
last): fixed parameters and the full covariance on the bodies this variant shares with the others (tests/variant_cases.py,
which states the bounds), GPSAT_MEAN_ZERO, the converged fit and c through the generalised-least-squares identity
(variant_numpy.gls_sides, to rtol 1e-6), Adam, c fixed or boxed, the refusals, the model and the orchestrator.  The large tile,
the ragged batch and bit identity are in tests/test_gpu_variants.py.

The converged fit is held to the bounds of tests/test_gpu_parity.py::test_fp64_learned_hyperparameters_match_scipy.
"""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import GpsatError
from variant_cases import check_fixed_parameters, check_full_cov, eng, eng8, FIELDS, KERNELS, MEAN as CASE, ragged_inputs, run, same as _same  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

SHIFT = CASE.SHIFT                                 # the level added to synthetic's de-meaned y
_run, _batch, _theta = functools.partial(run, CASE), CASE.batch, CASE.theta


# ---- 1. fixed theta against variant_numpy, and the full covariance: the shared bodies of tests/variant_cases.py
@pytest.mark.parametrize("i,N,P,D", [(i, *s) for i, s in enumerate(CASE.SHAPES)])
def test_objective_gradient_predict_at_fixed_parameters(eng, i, N, P, D):
    """Three tiles, one per value of c; the kernels take turns over the shapes (each at least once)."""
    check_fixed_parameters(CASE, eng, KERNELS[i % 4], N, P, D, N, CASE.CS, f"4-wave {KERNELS[i % 4]} c {CASE.CS}")


@pytest.mark.parametrize("i,N,P,D", [(i, *s) for i, s in enumerate(CASE.SHAPES)])
def test_fixed_parameters_on_the_eight_wave_build(eng8, i, N, P, D):
    check_fixed_parameters(CASE, eng8, KERNELS[(i + 2) % 4], N, P, D, N, CASE.CS, f"8-wave, one workgroup per CU, {KERNELS[(i + 2) % 4]}",
                           eight_wave=True)


@pytest.mark.parametrize("D", CASE.cov_D)
def test_full_cov_at_fixed_parameters(eng, D):
    check_full_cov(CASE, eng, D)


# ---- 2. GPSAT_MEAN_ZERO is gpsat_fit_predict_batch
def test_kind_zero_returns_the_bytes_of_the_plain_call(eng, monkeypatch):
    b, th = ragged_inputs(CASE)
    th2 = th[:, :b["D"] + 2].copy()
    kw = dict(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th2,
              kernel=b["kernel"], dtype="f64", optimiser="lbfgs", max_iter=5, want_grad=True)
    plain = eng.fit_predict_batch(**kw)
    calls = []

    def through_mean(h, bp):
        m = L.GpsatMean()
        m.kind = L.MEAN_ZERO
        calls.append(1)
        return eng._lib.gpsat_fit_predict_batch_mean(h, bp, C.byref(m))

    class Lib:
        """The engine's library with gpsat_fit_predict_batch routed through the new entry point."""
        def __getattr__(self, name):
            return through_mean if name == "gpsat_fit_predict_batch" else getattr(lib0, name)

    lib0 = eng._lib
    monkeypatch.setattr(eng, "_lib", Lib())
    routed = eng.fit_predict_batch(**kw)
    monkeypatch.undo()
    assert calls == [1]
    for name in FIELDS:
        assert np.asarray(getattr(routed, name)).tobytes() == np.asarray(getattr(plain, name)).tobytes(), name


# ---- 3. a converged fit
FIT_SEEDS = (900, 902, 905)          # SciPy reports success on each (checked on the CPU)


@pytest.fixture(scope="module")
def fit_case(eng):
    T, D, kernel = len(FIT_SEEDS), 3, "Matern32"
    tiles = [syn.make_tile(s, 150, 16, D, kid=2)[:3] for s in FIT_SEEDS]
    b = dict(D=D, kernel=kernel, obs_off=np.arange(T + 1) * 150, pred_off=np.arange(T + 1) * 16,
             X=np.concatenate([t[0] for t in tiles]), y=np.concatenate([t[1] for t in tiles]) + SHIFT,
             Xs=np.concatenate([t[2] for t in tiles]))
    lo2, hi2 = syn.default_bounds(T, D)
    lo, hi = np.column_stack([lo2, np.full(T, np.nan)]), np.column_stack([hi2, np.full(T, np.nan)])
    th0 = np.ones((T, D + 3))
    th0[:, D + 2] = 0.0
    ref = [vn.fit(vn.MEAN, kernel, b["X"][150 * t:150 * (t + 1)], b["y"][150 * t:150 * (t + 1)], th0[t], lo[t], hi[t], max_iter=1000)
           for t in range(T)]
    return b, th0, lo, hi, ref


def test_learned_hyperparameters_match_scipy(eng, fit_case):
    b, th0, lo, hi, ref = fit_case
    T, D, kernel = len(FIT_SEEDS), b["D"], b["kernel"]
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="lbfgs", max_iter=1000, want_grad=True)
    assert all(res.success for _, _, res in ref)
    o_theta, o_nll = np.array([th for th, _, _ in ref]), np.array([f for _, f, _ in ref])
    print("device theta", r.theta, "nll", r.nll, "status", r.status, "n_eval", r.n_eval, "grad", r.grad)
    print("scipy  theta", o_theta, "nll", o_nll)
    assert (r.status == 0).all(), r.status
    np.testing.assert_allclose(r.nll, o_nll, rtol=0, atol=5e-5)
    np.testing.assert_allclose(r.theta[:, :D + 2], o_theta[:, :D + 2], rtol=2e-3)
    for t in range(T):
        X, y = b["X"][150 * t:150 * (t + 1)], b["y"][150 * t:150 * (t + 1)]
        # c: the returned c, the returned dnll/dc and a numpy K_y at the returned theta satisfy the GLS identity
        left, right = vn.gls_sides(kernel, X, y, r.theta[t], r.grad[t, D + 2])
        print("tile", t, "c", r.theta[t, D + 2], "scipy c", o_theta[t, D + 2], "GLS sides", left, right)
        np.testing.assert_allclose(left, right, rtol=1e-6)
        # the returned objective is the objective at the returned parameters
        assert abs(vn.nll_and_grad(vn.MEAN, kernel, X, y, r.theta[t], want_grad=False)[0] - r.nll[t]) <= 1e-9 * max(1.0, abs(r.nll[t])) * 150
        # c is really trained: away from its start, and not the sample mean
        assert abs(r.theta[t, D + 2] - SHIFT) > 1e-3 and abs(r.theta[t, D + 2] - y.mean()) > 1e-3


def test_adam_trains_the_constant_through_the_identity_transform(eng, fit_case):
    """GPSAT_OPT_ADAM is not refused: the objective falls and c leaves its start, in u = theta steps of adam_lr."""
    b, th0, lo, hi, _ = fit_case
    D = b["D"]
    r0 = _run(eng, b, th0, lo=lo, hi=hi)
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="adam", max_iter=30, adam_lr=0.05)
    assert (r.status == 1).all() and (r.nll < r0.nll).all()
    assert (r.theta[:, D + 2] > 0.05).all() and (r.theta[:, D + 2] < 1.6).all()           # at most 30 steps of 0.05 from 0


# ---- 4. c fixed, and c in a box
def test_constant_fixed_and_constant_in_a_box(eng, fit_case):
    b, th0, lo, hi, ref = fit_case
    D, T = b["D"], len(FIT_SEEDS)
    th1 = th0.copy()
    th1[:, D + 2] = [-0.2, 0.0, 0.45]
    tr = np.ones(D + 3, dtype=bool)
    tr[D + 2] = False
    r = _run(eng, b, th1, lo=lo, hi=hi, trainable=tr, optimiser="lbfgs", max_iter=1000)
    np.testing.assert_array_equal(r.theta[:, D + 2], th1[:, D + 2])
    assert (r.status == 0).all() and (r.theta[:, :D + 2] != 1.0).all()
    for t in range(T):                                     # the others are fitted: the zero-mean fit of y - c
        X, y = b["X"][150 * t:150 * (t + 1)], b["y"][150 * t:150 * (t + 1)]
        th, f, res = vn.fit(vn.MEAN, b["kernel"], X, y, th1[t], lo[t], hi[t], trainable=tr, max_iter=1000)
        print("fixed c", th1[t, D + 2], "device", r.theta[t], r.nll[t], "scipy", th, f)
        assert res.success and abs(r.nll[t] - f) <= 5e-5
    # a box that excludes the unconstrained optimum (about 0.3): c stays inside and goes to its upper end
    lob, hib = lo.copy(), hi.copy()
    lob[:, D + 2], hib[:, D + 2] = -0.5, 0.1
    th2 = th0.copy()
    th2[:, D + 2] = -0.1
    rb = _run(eng, b, th2, lo=lob, hi=hib, optimiser="lbfgs", max_iter=200)
    c = rb.theta[:, D + 2]
    print("boxed c", c, "status", rb.status)
    assert ((c > -0.5) & (c < 0.1)).all() and (c > -0.1).all(), c
    assert np.isin(rb.status, (0, 1, 6)).all() and (rb.theta[:, :D + 2] != 1.0).all()
    # and a box around it: the same optimum as without one
    lob[:, D + 2], hib[:, D + 2] = -2.0, 2.0
    rc = _run(eng, b, th2, lo=lob, hi=hib, optimiser="lbfgs", max_iter=1000)
    np.testing.assert_allclose(rc.nll, [f for _, f, _ in ref], rtol=0, atol=5e-5)


# ---- 5. what the C ABI refuses, and that the handle works afterwards
def test_refusals_leave_the_handle_usable(eng):
    b = _batch(2, 40, 5, 3, "Matern32", 1)
    th = _theta(np.random.default_rng(0), 2, 3, (0.3, -0.7))
    good = _run(eng, b, th)
    lib = eng._lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(D=3, kernel=2, dtype=L.F64, kind=L.MEAN_CONSTANT, reserved=None, c0=0.3):
        T, H = 1, D + 3
        obs_off, pred_off = np.array([0, 8], dtype=np.int64), np.array([0, 0], dtype=np.int64)
        X = np.ascontiguousarray(np.random.default_rng(1).uniform(size=(8, D)), dtype=np.float32 if dtype == L.F32 else np.float64)
        y = np.zeros(8, dtype=X.dtype)
        par, nan, tr = np.ones(H), np.full(H, np.nan), np.ones(H, dtype=np.uint8)
        par[H - 1] = c0
        out = dict(theta=np.zeros(H), nll=np.zeros(1), status=np.zeros(1, np.int32), n_eval=np.zeros(1, np.int32))
        fm = np.zeros(1, dtype=X.dtype)
        bt = L.GpsatBatch()
        bt.T, bt.D, bt.dtype, bt.kernel, bt.memory, bt.optimiser = T, D, dtype, kernel, L.MEM_HOST, L.OPT_NONE
        bt.obs_off, bt.pred_off, bt.theta0, bt.lo, bt.hi, bt.trainable = p(obs_off), p(pred_off), p(par), p(nan), p(nan), p(tr)
        bt.X, bt.y, bt.Xs = p(X), p(y), p(X)
        bt.theta, bt.nll, bt.status, bt.n_eval = p(out["theta"]), p(out["nll"]), p(out["status"]), p(out["n_eval"])
        bt.f_mean, bt.f_var, bt.y_var = p(fm), p(fm), p(fm)
        m = L.GpsatMean()
        m.kind = kind
        if reserved is not None:
            m.reserved[reserved] = 1
        rc = lib.gpsat_fit_predict_batch_mean(eng._h, C.byref(bt), C.byref(m))
        return rc, lib.gpsat_last_error().decode(), out

    rc, _, out = call()                                    # the straight call works: c = 0.3, y = 0
    assert rc == 0 and out["status"][0] == 5 and out["theta"][5] == 0.3
    for kw, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(D=4), "D <= 3"), (dict(kernel=L.KERNEL_RQ), "GPSAT_KERNEL_RQ"),
                      (dict(kind=2), "unknown kind"), (dict(kind=-1), "unknown kind"), (dict(reserved=3), "reserved"),
                      (dict(kind=L.MEAN_ZERO, reserved=0), "reserved"), (dict(c0=np.nan), "finite"), (dict(c0=-np.inf), "finite")):
        rc, why, _ = call(**kw)
        assert rc == -1 and match in why, (kw, rc, why)
        _same(_run(eng, b, th), good, f"after the refusal {match!r}")
    # through the Python wrapper: the library's own message for fp32
    with pytest.raises(GpsatError, match="GPSAT_F64 only") as ei:
        eng.fit_predict_batch(D=3, obs_off=b["obs_off"], X=b["X"].astype(np.float32), y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"],
                              theta0=th, kernel="Matern32", dtype="f32", optimiser="none", mean="constant")
    assert "(-1)" in str(ei.value)
    _same(_run(eng, b, th), good, "after fp32")
    # Adam is not refused
    r = _run(eng, b, th, optimiser="adam", max_iter=3)
    assert (r.status == 1).all()
    assert lib.gpsat_n_hyper_mean(2, 3, L.MEAN_CONSTANT) == 6 and lib.gpsat_n_hyper_mean(L.KERNEL_RQ, 3, L.MEAN_CONSTANT) == 0


# ---- 6. the model and the orchestrator end to end
def test_model_agrees_with_the_engine_call(eng):
    from gpsat_amd.models import HipGPRModel
    X, y, Xs, _ = syn.make_tile(900, 150, 16, 3, kid=2)
    y = y + SHIFT
    m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", kernel="Matern32", mean_function="Constant")
    lo2, hi2 = syn.default_bounds(1, 3)
    m.set_lengthscales_constraints(low=lo2[0, :3], high=hi2[0, :3], move_within_tol=False)
    b = dict(D=3, kernel="Matern32", obs_off=np.array([0, 150]), pred_off=np.array([0, 16]), X=X, y=y, Xs=Xs)
    th0 = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 0.0]])
    lo, hi = np.column_stack([lo2, [np.nan]]), np.column_stack([hi2, [np.nan]])
    assert m.get_objective_function_value() == _run(eng, b, th0, lo=lo, hi=hi).nll[0]
    ok = m.optimise_parameters()
    r = _run(eng, b, th0, lo=lo, hi=hi, optimiser="lbfgs", max_iter=10_000, full_cov=True)
    p = m.get_parameters()
    assert ok and r.status[0] == 0
    np.testing.assert_array_equal(np.concatenate([p["lengthscales"], [p["kernel_variance"], p["likelihood_variance"], p["mean_constant"]]]),
                                  r.theta[0])
    assert abs(p["mean_constant"] - SHIFT) > 1e-3
    assert m.get_objective_function_value() == r.nll[0]
    out = m.predict(Xs, full_cov=True, apply_scale=False)
    np.testing.assert_array_equal(out["f*"], r.f_mean)
    np.testing.assert_array_equal(out["f*_var"], np.diag(np.asarray(r.f_cov).reshape(16, 16)))
    np.testing.assert_array_equal(out["f*_cov"], np.asarray(r.f_cov).reshape(16, 16))
    np.testing.assert_array_equal(out["f_bar"], 0.0)
    with pytest.raises(NotImplementedError, match="held-out"):
        m.cross_validate()


def test_orchestrator_tables_equal_the_per_tile_model(eng):
    """Six experts in waves of four: the tables are those of HipGPRModel run tile by tile, mean_constant among them."""
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    from gpsat_amd.models import HipGPRModel
    rng = np.random.default_rng(3)
    x = np.sort(np.concatenate([rng.uniform(0.0, 8.0, 160), rng.normal(3.0, 0.3, 60), rng.normal(6.0, 0.2, 50)]))
    df = pd.DataFrame({"x": x, "y": 0.3 + 0.2 * np.sin(1.3 * x) + 0.05 * rng.standard_normal(len(x))})
    locs, radius = np.linspace(1.0, 7.0, 6), 1.5
    cons = {"lengthscales": {"low": 1e-3, "high": 10.0}}
    optim = {"fixed_params": ["likelihood_variance"], "max_iter": 60}
    pred = pd.DataFrame({"x": np.linspace(0.5, 7.5, 29)})
    ip = {"kernel": "Matern52", "mean_function": "Constant", "mean_func_kwargs": {"c": 0.1}, "noise_variance": 0.05 ** 2}
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": ip, "constraints": cons, "optim_kwargs": optim},
               pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.0})
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    oi.engine_workers = 1                                    # two small waves: no second engine (stream, workspace) for them
    assert oi.dtype == "f64"
    tabs = oi.run(store_path=None, store_every=4)            # the tables in expert order (the store itself: test_mean_cpu.py)
    assert len(tabs["run_details"]) == 6 and len(tabs["mean_constant"]) == 6
    for k, loc in enumerate(locs):
        d = df[(df["x"] <= loc + radius) & (df["x"] >= loc - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x"], engine=eng, dtype="f64", **ip)
        m.set_parameter_constraints(cons, move_within_tol=True, tol=1e-2)
        ok = m.optimise_parameters(**optim)
        p = m.get_parameters()
        assert tabs["mean_constant"]["mean_constant"].values[k] == p["mean_constant"] != 0.1
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
