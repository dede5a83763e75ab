"""GPU: sparse GP experts (gpsat_sgpr_fit_predict_batch, HipSGPRModel) against the numpy restatement in sgpr_numpy.py and
the reference's own SGPR test.

Accuracy bounds.  The kernel and numpy factor Kuu = k(Z, Z) + 1e-6 I in a different order of operations, so their results
differ by rounding amplified by the conditioning of Kuu: about eps * cond(Kuu) relative.  The ELBO and the predictions
are held to the stated starting bound (1e-9 relative) plus 64 eps cond(Kuu), with cond(Kuu) computed by numpy for the
tile.  Measured: at most 9 eps cond(Kuu) for the ELBO (RBF, cond up to 1.1e8) and 22 eps cond(Kuu) for f* (Matern-5/2,
D = 4, N = 20000, M = 500); 64 is about three times the largest ratio seen.
The gradient is a difference of large terms: R = Kuu^-1 / sn2 - S^-1, contracted with Kuf and dKuf over N rows.  This
holds in numpy's dense form as in the kernel's.  Component i is held to 1e-7 max|g| + 64 eps cond(Kuu) ||Kuu^-1||_2 / sn2
||Kuf||_F ||dKuf/dtheta_i||_F, the first-order size of the rounding of R carried through that contraction
(sgpr_numpy.grad_rounding_scale).  With the plain max-norm bound, RBF and Matern-5/2 tiles of N = 20000 missed by up to
1e-3 relative on the length scales; 6e-3 was observed where this estimate gives 4e-3 at cond(Kuu) = 3e4.  sn2 agreed to
4e-9.  At cond(Kuu) ~ 5e7 (RBF, M = 250) the estimate is loose by orders of magnitude, so there the gradient check only
rules out gross errors."""
import ctypes as C
import os

import numpy as np
import pytest

import sgpr_numpy as sn
from sgpr_edge_cases import check_fixed as _check_fixed, cond_kuu as _cond, pack as _pack

pytestmark = pytest.mark.gpu

M_MAX = 1024


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _make_tile(rng, N, M, D, P=5):
    side = 0.5 * M ** (1.0 / D)          # inducing points about half a length scale apart
    X = rng.uniform(0, side, (N, D))
    y = np.sin(X.sum(1)) + 0.3 * rng.normal(size=N)
    Z = X[:M].copy() if N >= M else rng.uniform(0, side, (M, D))
    return X, y, Z, rng.uniform(0, side, (P, D))


def test_reference_sgpr_known_answer(eng, golden_dir):
    """The reference's test_gpflow_sgpr (tests/test_localexperts.py:229-251): 50 inducing points = all 50 points, likelihood
    variance eps^2 and kernel variance fixed, lengthscale in [1e-10, 5]; lengthscale, f* and f*_var to 1e-4."""
    import pandas as pd
    from gpsat_amd.models import get_model
    g = np.load(os.path.join(golden_dir, "kat_sklearn_matern32.npz"))
    df = pd.DataFrame(data={"x": g["x_train"], "y": g["y_train"]})
    model = get_model("GPflowSGPRModel")(data=df, obs_col="y", coords_col="x", obs_mean=None, num_inducing_points=50,
                                         engine=eng)
    np.testing.assert_array_equal(model.get_inducing_points(), model.coords)
    model.set_parameters(likelihood_variance=float(g["eps"]) ** 2)
    model.set_parameter_constraints({"lengthscales": {"low": 1e-10, "high": 5.0}})
    assert model.optimise_parameters(fixed_params=["likelihood_variance", "kernel_variance"])
    out = model.predict(coords=np.array([[float(g["x_test"])]]))
    params = model.get_parameters()
    assert abs(params["lengthscales"][0] - float(g["ls"])) < 1e-4
    assert abs(out["f*"][0] - float(g["pred_mean"])) < 1e-4
    assert abs(out["f*_var"][0] - float(g["pred_std"]) ** 2) < 1e-4
    assert model.get_objective_function_value() < 0        # the ELBO, not its negative


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_fixed_theta_matches_numpy(eng, kid, D):
    """One ragged batch per (kernel, D); across the 16 batches every N in {1, M-1, M, 3000, 20000} meets every M in
    {1, 16, 250, 500, M_max} (a Latin-square rotation), except that N = 20000 with M = M_max runs as N = 3000 to keep the
    dense numpy restatement to seconds."""
    rng = np.random.default_rng(100 * kid + D)
    Ns = lambda M: [1, max(M - 1, 1), M, 3000, 20000]
    Ms = [1, 16, 250, 500, M_MAX]
    sh = (4 * kid + D) % 5
    tiles = []
    for i, M in enumerate(Ms):
        N = Ns(M)[(i + sh) % 5]
        if N * M > 20000 * 500:
            N = 3000
        tiles.append(_make_tile(rng, N, M, D))
    th = np.concatenate([rng.uniform(0.8, 1.5, D), [1.3], [0.2]])
    _check_fixed(eng, kid, D, tiles, th)


def test_tile_larger_than_any_exact_tile(eng):
    """N = 100 000 observations, more than gpsat_max_tile_obs allows any exact tile; M = 500: it finishes and matches numpy
    at fixed theta."""
    from gpsat_amd import _lib as L
    N = 100_000
    assert all(N > L.max_tile_obs(dt, D) for dt in ("f32", "f64") for D in range(1, 5))
    rng = np.random.default_rng(7)
    X = rng.uniform(0, 20, (N, 2))
    y = np.sin(X[:, 0]) * np.cos(X[:, 1]) + 0.1 * rng.normal(size=N)
    Z = X[rng.permutation(N)[:500]]
    _check_fixed(eng, 2, 2, [(X, y, Z, rng.uniform(0, 20, (9, 2)))], np.array([1.5, 1.2, 0.8, 0.05]))


def test_bits_do_not_depend_on_the_batch(eng):
    """A tile returns the same bits alone and inside a batch of 1 000 other tiles (fit included)."""
    rng = np.random.default_rng(11)
    D = 3
    target = _make_tile(rng, 700, 60, D)
    others = [_make_tile(rng, int(rng.integers(1, 400)), int(rng.integers(1, 80)), D) for _ in range(1000)]
    kw = dict(D=D, kernel="Matern32", theta0=np.ones(D + 2), optimiser="lbfgs", max_iter=15, want_grad=True)
    r1 = eng.sgpr_fit_predict_batch(**_pack([target]), **kw)
    r2 = eng.sgpr_fit_predict_batch(**_pack(others[:500] + [target] + others[500:]), **kw)
    a, b = 500, 501
    pk = _pack(others[:500] + [target])
    pa, pb = pk["pred_off"][-2], pk["pred_off"][-1]
    assert r1.theta[0].tobytes() == r2.theta[a:b][0].tobytes()
    assert r1.nll[0].tobytes() == r2.nll[a:b][0].tobytes()
    assert r1.grad[0].tobytes() == r2.grad[a:b][0].tobytes()
    for k in ("f_mean", "f_var", "y_var"):
        assert getattr(r1, k).tobytes() == getattr(r2, k)[pa:pb].tobytes(), k
    assert r1.n_eval[0] == r2.n_eval[a]


def test_refusals_return_einval_and_the_handle_recovers(eng):
    """M above gpsat_max_inducing, fp32, a NULL Z, full covariance: each GPSAT_EINVAL with a message; the next call works."""
    from gpsat_amd import _lib as L
    lib = eng._lib
    D, H = 2, 4
    rng = np.random.default_rng(5)
    X, y = rng.normal(size=(40, D)), rng.normal(size=40)
    Zbig = rng.normal(size=(M_MAX + 1, D))
    keep = []

    def p(a):
        a = np.ascontiguousarray(a)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def call(M, dtype=L.F64, null_z=False, cov=False):
        b = L.GpsatBatch()
        b.T, b.D, b.dtype, b.kernel, b.memory, b.optimiser = 1, D, dtype, 2, L.MEM_HOST, 0
        b.obs_off, b.pred_off = p(np.array([0, 40], dtype=np.int64)), p(np.array([0, 0], dtype=np.int64))
        b.theta0, b.lo, b.hi = p(np.ones(H)), p(np.full(H, np.nan)), p(np.full(H, np.nan))
        b.trainable = p(np.ones(H, dtype=np.uint8))
        b.X, b.y = p(X if dtype == L.F64 else X.astype(np.float32)), p(y if dtype == L.F64 else y.astype(np.float32))
        b.theta, b.nll = p(np.zeros(H)), p(np.zeros(1))
        b.status, b.n_eval = p(np.zeros(1, dtype=np.int32)), p(np.zeros(1, dtype=np.int32))
        if cov:
            b.cov_off, b.f_cov = p(np.array([0, 0], dtype=np.int64)), p(np.zeros(1))
        s = L.GpsatSparse()
        s.z_off = p(np.array([0, M], dtype=np.int64))
        s.Z = None if null_z else p(Zbig[:M])
        return lib.gpsat_sgpr_fit_predict_batch(eng._h, C.byref(b), C.byref(s))

    for kw in (dict(M=M_MAX + 1), dict(M=8, dtype=L.F32), dict(M=8, null_z=True), dict(M=8, cov=True)):
        assert call(**kw) == -1, kw
        assert lib.gpsat_last_error(), kw
        r = eng.sgpr_fit_predict_batch(D=D, obs_off=[0, 40], X=X, y=y, pred_off=[0, 0], Xs=np.zeros((0, D)), z_off=[0, 8],
                                       Z=Zbig[:8], theta0=np.ones(H), kernel="Matern32", optimiser="none")
        assert r.status[0] == 5 and np.isfinite(r.nll[0])
    assert call(M=M_MAX) == 0


@pytest.mark.parametrize("kid,D,side", [(0, 3, 4), (1, 1, 8), (2, 2, 6), (2, 3, 4), (3, 2, 5), (3, 3, 4)])
def test_converged_fits_match_scipy(eng, kid, D, side):
    """Full L-BFGS fits (all D + 2 parameters trainable) on well-conditioned tiles (cond(Kuu) 1e3 .. 8e4 at the optimum)
    land where SciPy L-BFGS-B lands on the NumPy ELBO with the same transforms: theta to 1e-5 relative, ELBO to 1e-8
    relative.  Both optimisers run with tolerances below the resolution of the arithmetic and may end on a failed line
    search at the optimum.  SciPy's u-space gradient must be <= 1e-5 there.  The device may stop earlier, by its fp64
    noise-floor rule (measured: u-space gradient 1.4e-4 on Matern-3/2, D = 2, where the Hessian puts theta within 1e-6 and
    the ELBO within 4e-13 of the optimum), so its result is held to the comparison, not to a gradient bound."""
    rng = np.random.default_rng(40 + 10 * kid + D)
    N, M = 400, 30
    X = rng.uniform(0, side, (N, D))
    y = np.sin(1.3 * X.sum(1)) + 0.2 * rng.normal(size=N)
    Z = X[rng.permutation(N)[:M]]
    th0 = np.concatenate([np.full(D, 0.7), [1.0], [0.3]])
    r = eng.sgpr_fit_predict_batch(D=D, obs_off=[0, N], X=X, y=y, pred_off=[0, 0], Xs=np.zeros((0, D)), z_off=[0, M], Z=Z,
                                   theta0=th0, kernel=kid, optimiser="lbfgs", max_iter=2000, ftol=1e-15, gtol=1e-9,
                                   want_grad=True)
    # with tolerances below the arithmetic's resolution the search ends like SciPy's: converged (0) -- which includes the
    # fp64 noise-floor rule of gpsat_opt.h, a step whose decrease was already <= 1e-12 |f| -- or a line search that failed
    # at the optimum (6, ABNORMAL_TERMINATION_IN_LNSRCH).  Whether that is the optimum is what the comparison below checks.
    assert r.status[0] in (0, 6), r.status
    c = X.mean(0)
    th_s, el_s, res = sn.fit_scipy(kid, X - c, y, Z - c, th0)
    assert np.max(np.abs(res.jac)) <= 1e-5, res.message
    assert _cond(kid, Z - c, th_s) < 1e5
    np.testing.assert_allclose(r.theta[0], th_s, rtol=1e-5)
    assert abs(-r.nll[0] - el_s) <= 1e-8 * abs(el_s)


def test_orchestrator_end_to_end(eng, tmp_path):
    """BatchedLocalExpertOI with oi_model GPflowSGPRModel on data where most experts select more observations than
    gpsat_max_tile_obs: every expert gets a result row and no error rows; the tables equal per-tile HipSGPRModel runs
    (same inducing points, theta, ELBO, predictions); inducing_points is stored; small tiles run the exact-GP replacement."""
    import pandas as pd
    from gpsat_amd import _lib as L
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    from gpsat_amd.models import HipGPRModel, HipSGPRModel
    rng = np.random.default_rng(21)
    x = np.concatenate([rng.uniform(0, 8, 40000), rng.uniform(9.5, 10, 60)])
    df = pd.DataFrame({"x": x, "y": np.sin(x) + 0.1 * rng.normal(size=len(x))})
    locs = [1.0, 3.0, 5.0, 7.0, 9.8]
    radius, ip = 1.0, {"kernel": "Matern32", "noise_variance": 0.01, "num_inducing_points": 100, "inducing_seed": 5,
                       "coords_scale": 2.0}
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": "y", "coords_col": ["x"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius},
                                             {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "GPflowSGPRModel", "init_params": ip, "optim_kwargs": {"max_iter": 50},
                             "replacement_threshold": 500,
                             "replacement_init_params": {"kernel": "Matern32", "noise_variance": 0.01, "coords_scale": 2.0}},
               pred_loc_config={"method": "expert_loc"})
    with _no_error_rows_warning():
        tabs = BatchedLocalExpertOI(engine=eng, **cfg).run(store_path=str(tmp_path / "s"))
    rd = tabs["run_details"]
    assert rd.index.tolist() == locs and rd["objective_value"].notna().all()
    assert (rd["num_obs"].values[:4] > L.max_tile_obs("f64", 1)).all() and rd["num_obs"].values[4] < 500
    assert rd["model"].iloc[4].endswith("HipGPRModel") and all(m.endswith("HipSGPRModel") for m in rd["model"].iloc[:4])
    X = df["x"].values
    for e, loc in enumerate(locs):
        sel = df[(X <= loc + radius) & (X >= loc - radius)]
        if e < 4:
            m = HipSGPRModel(data=sel, obs_col="y", coords_col=["x"], engine=eng, expert_index=e, **ip)
            np.testing.assert_array_equal(tabs["inducing_points"].loc[loc]["inducing_points"].values,
                                          m.get_inducing_points()[:, 0])
        else:
            m = HipGPRModel(data=sel, obs_col="y", coords_col=["x"], engine=eng, dtype="f64", kernel="Matern32",
                            noise_variance=0.01, coords_scale=2.0)
        assert m.optimise_parameters(max_iter=50) == bool(rd["optimise_success"].iloc[e])
        p = m.get_parameters()
        np.testing.assert_allclose(tabs["lengthscales"].loc[loc]["lengthscales"], p["lengthscales"][0], rtol=1e-12)
        np.testing.assert_allclose(tabs["kernel_variance"].loc[loc]["kernel_variance"], p["kernel_variance"], rtol=1e-12)
        np.testing.assert_allclose(rd["objective_value"].iloc[e], m.get_objective_function_value(), rtol=1e-10)
        out = m.predict(coords=np.array([[loc]]))
        np.testing.assert_allclose(tabs["preds"].loc[loc]["f*"], out["f*"][0], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(tabs["preds"].loc[loc]["f*_var"], out["f*_var"][0], rtol=1e-10, atol=1e-12)
    assert tabs["inducing_points"].index.unique().tolist() == locs[:4]


class _no_error_rows_warning:
    """No 'not run (error row in run_details)' warning may be raised by the run."""
    def __enter__(self):
        import warnings
        self._cm = warnings.catch_warnings(record=True)
        self._w = self._cm.__enter__()
        warnings.simplefilter("always")
        return self

    def __exit__(self, *a):
        self._cm.__exit__(*a)
        assert not [w for w in self._w if "error row" in str(w.message)]
        return False
