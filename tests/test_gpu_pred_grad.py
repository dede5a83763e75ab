"""GPU: the gradient of the posterior mean at the prediction points and its variance per component (gpsat_fit_predict_batch_grad,
Engine.fit_predict_batch(pred_grad=True)) against the fp64 restatement tests/pred_grad_numpy.py, on the
4-wave and the 8-wave build.

Bounds.  l_a f_grad_a is a sum of the kind f_mean is (V^T z with V = L^-1 of a right-hand side of the kernel's size), and
l_a^2 f_grad_var_a one of the kind f_var is (a prior term minus V^T V), so they are held to check_tile's bounds for those:
l_a |error of f_grad_a| <= 1e-9 max(|y|max, 1), and l_a^2 |error of f_grad_var_a| <= 3e-10 -- three times f_var's 1e-10, because
the prior term is up to 3 kernel_variance (gg(0) = 3 for Matern32) where f_var's is kernel_variance.
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import pred_grad_numpy as pg
import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd.engine import Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel
from variant_cases import FIELDS, Case, check_tile, eng, eng8, one, ragged_inputs, run, same  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

GRAD_FIELDS = FIELDS + ("f_grad", "f_grad_var")


class GradCase(Case):
    """The plain model (variant_numpy's NOISE with v = 0, which changes no bit of K_y) with pred_grad=True."""
    variant, name = vn.NOISE, "grad"

    def call_kw(self, b):
        return {"pred_grad": True}

    def batch(self, T, N, P, D, kernel, base_seed):
        b = super().batch(T, N, P, D, kernel, base_seed)
        b["obs_var"] = np.zeros(int(b["obs_off"][-1]))
        for t in range(T):                                 # the tile's first prediction point lies on one of its observations
            a, e, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
            if e > a and pe > pa:
                b["Xs"][pa] = b["X"][a + min(5, e - a - 1)]
        return b


GRAD = GradCase()
WORST = {"grad": 0.0, "var": 0.0}                          # largest scaled errors seen in this module (printed per test)


def check_grad_tile(r, b, t, theta, what=""):
    """Tile t's two outputs against the restatement at ``theta``, to the bounds of the module docstring; the prior, exactly, for
    a tile without observations."""
    D, kernel = b["D"], b["kernel"]
    a, e, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
    fg, fgv = np.asarray(r.f_grad)[pa:pe], np.asarray(r.f_grad_var)[pa:pe]
    assert fg.shape == fgv.shape == (pe - pa, D)
    if pe == pa:
        return
    ref_g, ref_v = pg.predict_grad(kernel, b["X"][a:e], b["y"][a:e], b["Xs"][pa:pe], theta)
    if e == a:
        np.testing.assert_array_equal(fg, 0.0)
        np.testing.assert_array_equal(fgv, ref_v)
        return
    ell, ymax = theta[:D], np.abs(b["y"][a:e]).max()
    eg, ev = np.abs(fg - ref_g) * ell, np.abs(fgv - ref_v) * ell ** 2
    WORST["grad"], WORST["var"] = max(WORST["grad"], eg.max() / max(ymax, 1.0)), max(WORST["var"], ev.max())
    assert eg.max() <= 1e-9 * max(ymax, 1.0), (what, t, int(e - a), eg.max())
    assert ev.max() <= 3e-10, (what, t, int(e - a), ev.max())


# ---- 1. fixed parameters against the restatement
#       smallest   below a block   one block   a row past   5 block rows: the     a wave's second pair      middle-sized
#                                              a block      second 4-row panel    of chunks on both builds
SHAPES = [(1, 2, 1), (15, 5, 2), (16, 16, 3), (17, 33, 4), (65, 17, 3),          (40, 261, 3),             (100, 33, 3)]


@pytest.mark.parametrize("N,P,D", SHAPES)
def test_fixed_parameters_match_the_restatement(eng, eng8, N, P, D):
    for kernel in pg.KERNELS:
        b = GRAD.batch(2, N, P, D, kernel, 7000 + N)
        th = GRAD.theta(np.random.default_rng(N + D), 2, D)
        for e_, what in ((eng, "4-wave"), (eng8, "8-wave")):
            r = run(GRAD, e_, b, th)
            assert r.f_grad.shape == r.f_grad_var.shape == (2 * P, D) and r.f_grad.dtype == np.float64
            assert (r.status == 5).all()
            for t in range(2):
                check_tile(GRAD, r, b, t, th[t], what)
                check_grad_tile(r, b, t, th[t], f"{what} {kernel}")
            # (one de-meaned observation is y = 0: the posterior mean is flat)
            assert (N == 1 or np.abs(r.f_grad).max() > 0) and (r.f_grad_var > 0).all()
    print("largest scaled errors so far: gradient", WORST["grad"], "variance", WORST["var"])


# ---- 2. the other outputs are the plain call's bytes
@pytest.mark.parametrize("opt", [dict(optimiser="none"), dict(optimiser="lbfgs", max_iter=12)], ids=["none", "lbfgs"])
def test_other_outputs_are_the_bytes_of_the_plain_call(eng, eng8, opt):
    b, th = ragged_inputs(GRAD)
    th0 = th if opt["optimiser"] == "none" else np.ones(th.shape)
    lo, hi = GRAD.bounds(len(th), b["D"])
    for e_ in (eng, eng8):
        r = run(GRAD, e_, b, th0, lo=lo, hi=hi, **opt)
        r0 = run(GRAD, e_, b, th0, lo=lo, hi=hi, pred_grad=False, **opt)
        assert r0.f_grad is None and r0.f_grad_var is None and r.f_grad is not None
        same(r, r0, f"pred_grad against the plain call, {opt['optimiser']}")
        if opt["optimiser"] != "none":
            assert r.n_eval.max() > 6 and (r.theta != th0).any()


# ---- 3. a ragged, unsorted batch: every tile has the bits it has alone, on a second call and time-sliced
@pytest.fixture(scope="module")
def ragged(eng):
    b, th = ragged_inputs(GRAD)
    return b, th, run(GRAD, eng, b, th)


def test_ragged_batch(ragged):
    b, th, r = ragged
    Ns, Ps = np.diff(b["obs_off"]), np.diff(b["pred_off"])
    assert len(Ns) == 60 and Ns.max() <= 200 and Ns[3] == 0 and Ps[3] > 0 and Ps[5] == 0 and Ns[5] > 0 and r.status[3] == 4
    assert r.f_grad.shape == (int(Ps.sum()), 3)
    for t in range(60):
        check_tile(GRAD, r, b, t, th[t], "ragged")
        check_grad_tile(r, b, t, th[t], "ragged")
    pa, pe = b["pred_off"][3], b["pred_off"][4]                         # the empty tile: the prior at theta0
    np.testing.assert_array_equal(r.f_grad[pa:pe], 0.0)
    np.testing.assert_array_equal(r.f_grad_var[pa:pe], np.tile(th[3, 3] * 3.0 / th[3, :3] ** 2, (pe - pa, 1)))
    print("largest scaled errors so far: gradient", WORST["grad"], "variance", WORST["var"])


def _part(r, b, t, name):
    whole = getattr(r, name)
    return whole[b["pred_off"][t]:b["pred_off"][t + 1]] if name in ("f_mean", "f_var", "y_var", "f_grad", "f_grad_var") else whole[[t]]


def test_same_bits_alone_in_the_batch_and_again(eng, ragged):
    b, th, r = ragged
    same(run(GRAD, eng, b, th), r, "second call", GRAD_FIELDS)
    for t in (3, 5, 17, 40):                                             # the empty tile, the tile with P = 0, the largest, any
        r1 = run(GRAD, eng, one(b, t), th[[t]])
        for name in GRAD_FIELDS:
            assert np.asarray(getattr(r1, name)).tobytes() == np.asarray(_part(r, b, t, name)).tobytes(), (t, name)


def test_time_sliced_optimisation_is_bit_identical(eng, ragged, monkeypatch):
    """The queue forced as tests/test_gpu_variants.py forces it: suspended after every evaluation, after every third of a
    200-point tile, or never."""
    b, th, _ = ragged
    lo, hi = GRAD.bounds(60, 3)
    th0 = np.ones(th.shape)
    kw = dict(lo=lo, hi=hi, optimiser="lbfgs", max_iter=12)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "0")
    r0 = run(GRAD, eng, b, th0, **kw)
    assert r0.n_eval.max() > 6 and (r0.status <= 1).sum() > 40
    for seg in ("1", str(3 * 14 ** 3)):
        monkeypatch.setenv("GPSAT_DEBUG_SEG", seg)
        same(run(GRAD, eng, b, th0, **kw), r0, f"slice {seg}", GRAD_FIELDS)
    monkeypatch.delenv("GPSAT_DEBUG_SEG")
    t = 17
    r1 = run(GRAD, eng, one(b, t), th0[[t]], lo=lo[[t]], hi=hi[[t]], optimiser="lbfgs", max_iter=12)
    for name in GRAD_FIELDS:
        assert np.asarray(getattr(r1, name)).tobytes() == np.asarray(_part(r0, b, t, name)).tobytes(), (t, name)
    # at the fitted parameters the outputs are the restatement's
    for t in (17, 40):
        if r0.status[t] <= 1:
            check_grad_tile(r0, b, t, r0.theta[t], "fitted")


# ---- 4. device tensors
def test_device_tensors_return_the_bits_of_host_mode(eng, ragged):
    import torch
    b, th, r = ragged
    dev = torch.device("cuda", eng.device_id)
    X, y, Xs = (torch.tensor(b[k], device=dev) for k in ("X", "y", "Xs"))
    rd = eng.fit_predict_batch(D=3, obs_off=b["obs_off"], X=X, y=y, pred_off=b["pred_off"], Xs=Xs, theta0=th, kernel=b["kernel"],
                               dtype="f64", optimiser="none", want_grad=True, pred_grad=True)
    assert isinstance(rd.f_grad, torch.Tensor) and rd.f_grad.is_cuda and rd.f_grad.shape == r.f_grad.shape
    for name in GRAD_FIELDS:
        v = getattr(rd, name)
        v = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        assert v.tobytes() == np.asarray(getattr(r, name)).tobytes(), name
    np.testing.assert_array_equal(X.cpu().numpy(), b["X"])               # the inputs are read only
    np.testing.assert_array_equal(Xs.cpu().numpy(), b["Xs"])
    # a batch without prediction points, in either mode
    e0 = dict(D=3, obs_off=[0, 20], pred_off=[0, 0], theta0=np.ones((1, 5)), kernel="RBF", dtype="f64", optimiser="none", pred_grad=True)
    rh = eng.fit_predict_batch(X=b["X"][:20], y=b["y"][:20], Xs=np.zeros((0, 3)), **e0)
    rz = eng.fit_predict_batch(X=X[:20].contiguous(), y=y[:20].contiguous(), Xs=torch.zeros((0, 3), dtype=torch.float64, device=dev), **e0)
    assert rh.f_grad.shape == (0, 3) and tuple(rz.f_grad_var.shape) == (0, 3) and rh.nll.tobytes() == rz.nll.tobytes()


# ---- 5. refusals leave the handle usable
def test_every_refusal_is_followed_by_a_good_call_with_the_same_bits(eng, ragged):
    b, th, r = ragged
    t = 40
    b1, th1 = one(b, t), th[[t]]
    good = run(GRAD, eng, b1, th1)
    lib, sumP = eng._lib, int(b1["pred_off"][-1])

    def raw_call(kernel="Matern32", dtype="f64", reserved=None, null_out=None, cov=False):
        """The entry point itself: the Python wrapper refuses most of these before the library sees them."""
        np_dt = np.float32 if dtype == "f32" else np.float64
        meta = ((np.asarray(b1["obs_off"], dtype=np.int64), np.asarray(b1["pred_off"], dtype=np.int64)),
                np.ascontiguousarray(th1[:, :L.n_hyper(kernel, 3)] if kernel != "RationalQuadratic" else np.ones((1, 6))),
                np.full((1, 6 if kernel == "RationalQuadratic" else 5), np.nan), np.full((1, 6 if kernel == "RationalQuadratic" else 5), np.nan),
                np.ones(6 if kernel == "RationalQuadratic" else 5, dtype=np.uint8))
        data = tuple(np.ascontiguousarray(b1[k], dtype=np_dt) for k in ("X", "y", "Xs"))
        preds = tuple(np.empty(sumP, dtype=np_dt) for _ in range(3))
        bb, res = Engine._fill_batch(3, dtype, False, meta, data, preds, kernel, "none", 0, 0, 0.0, 0.0, 0.0, False)
        outs = [np.empty(sumP * 3), np.empty(sumP * 3)]
        s = L.GpsatPredGrad()
        s.f_grad, s.f_grad_var = (None if null_out == i else o.ctypes.data for i, o in enumerate(outs))
        if reserved is not None:
            s.reserved[reserved] = 1
        cov_off, fc = np.array([0, sumP * sumP], dtype=np.int64), np.empty(sumP * sumP, dtype=np_dt)
        if cov:
            bb.cov_off, bb.f_cov = cov_off.ctypes.data, fc.ctypes.data
        rc = lib.gpsat_fit_predict_batch_grad(eng._h, C.byref(bb), C.byref(s))
        return rc, lib.gpsat_last_error().decode()

    assert raw_call()[0] == 0
    for kw, match in ((dict(dtype="f32"), "GPSAT_F64 only"), (dict(kernel="Matern12"), "not mean-square differentiable"),
                      (dict(kernel="RationalQuadratic"), "GPSAT_KERNEL_RQ"), (dict(reserved=3), "reserved"),
                      (dict(null_out=0), "f_grad is NULL"), (dict(null_out=1), "f_grad_var is NULL"), (dict(cov=True), "full covariance")):
        rc, why = raw_call(**kw)
        assert rc == -1 and match in why, (kw, rc, why)
        same(run(GRAD, eng, b1, th1), good, f"after the refusal of {kw}", GRAD_FIELDS)
    rc = lib.gpsat_fit_predict_batch_grad(eng._h, None, None)
    assert rc == -1
    for more in (dict(full_cov=True), dict(cv_fold="loo"), dict(n_starts=2), dict(obs_var=np.zeros(int(b1["obs_off"][-1]))), dict(dtype="f32")):
        with pytest.raises(GpsatError, match="pred_grad"):
            eng.fit_predict_batch(**{**dict(D=3, obs_off=b1["obs_off"], X=b1["X"], y=b1["y"], pred_off=b1["pred_off"], Xs=b1["Xs"],
                                            theta0=th1, kernel="Matern32", dtype="f64", optimiser="none", pred_grad=True), **more})
        same(run(GRAD, eng, b1, th1), good, f"after the wrapper's refusal of {sorted(more)}", GRAD_FIELDS)
    for name in GRAD_FIELDS:                                              # ... and they are the tile's bits inside the batch
        assert np.asarray(getattr(good, name)).tobytes() == np.asarray(_part(r, b, t, name)).tobytes(), name


# ---- 6. the model and the orchestrator
def test_model_predict_gradient_in_raw_units(eng):
    rng = np.random.default_rng(11)
    N, D = 120, 3
    X = rng.uniform(0.0, 4.0, (N, D)) * np.array([10.0, 1.0, 100.0])
    y = 5.0 + 2.0 * np.sin(X[:, 0] / 10.0 + X[:, 1]) * np.cos(X[:, 2] / 100.0) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 4.0, (17, D)) * np.array([10.0, 1.0, 100.0])
    Xs[0] = X[7]
    cs, osc = np.array([10.0, 1.0, 100.0]), 2.0
    for kernel in pg.KERNELS:
        m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", coords_scale=cs, obs_scale=osc, obs_mean="local", kernel=kernel,
                        kernel_kwargs={"lengthscales": [1.1, 0.9, 1.6], "variance": 0.8}, noise_variance=0.02)
        theta = np.array([1.1, 0.9, 1.6, 0.8, 0.02])
        out, plain = m.predict(Xs, gradient=True), m.predict(Xs)
        ys = (y - y.mean()) / osc
        fg, fgv = pg.predict_grad(kernel, X / cs, ys, Xs / cs, theta)
        for k in range(D):
            # the device's bounds in scaled units, carried to raw units by the factors of the conversion
            np.testing.assert_allclose(out[f"f*_grad_{k}"], osc * fg[:, k] / cs[k], rtol=0,
                                       atol=1e-9 * max(np.abs(ys).max(), 1.0) / theta[k] * osc / cs[k])
            np.testing.assert_allclose(out[f"f*_grad_var_{k}"], osc ** 2 * fgv[:, k] / cs[k] ** 2, rtol=0,
                                       atol=3e-10 / theta[k] ** 2 * osc ** 2 / cs[k] ** 2)
        for k in plain:
            np.testing.assert_array_equal(plain[k], out[k])
    with pytest.raises(NotImplementedError, match="full_cov"):
        m.predict(Xs, full_cov=True, gradient=True)


def test_orchestrator_columns_are_the_per_tile_models(eng):
    rng = np.random.default_rng(3)
    n, radius = 400, 2.0
    df = pd.DataFrame({"x": rng.uniform(0.0, 10.0, n), "t": rng.uniform(0.0, 4.0, n)})
    df["y"] = 0.4 * np.sin(1.3 * df["x"]) * np.cos(0.7 * df["t"]) + 0.03 * rng.standard_normal(n)
    locs = pd.DataFrame({"x": np.linspace(2.0, 8.0, 5), "t": np.full(5, 2.0)})
    pred = pd.DataFrame({"x": np.linspace(0.5, 9.5, 30), "t": np.linspace(1.0, 3.0, 30)})
    ip = {"coords_scale": [2.0, 0.5], "obs_scale": 0.5, "kernel": "Matern52"}
    cons = {"lengthscales": {"low": [1e-3, 1e-3], "high": [10.0, 10.0]}}
    oi = BatchedLocalExpertOI(
        engine=eng, expert_loc_config={"source": locs},
        data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x", "t"],
                     "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
        model_config={"oi_model": "HipGPRModel", "init_params": ip, "constraints": cons, "optim_kwargs": {"max_iter": 30},
                      "pred_kwargs": {"gradient": True}},
        pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.2})
    assert oi.dtype == "f64"
    preds = oi.run(store_path=None)["preds"]
    at = 0
    for k, loc in locs.iterrows():
        d = df[(df["x"] <= loc["x"] + radius) & (df["x"] >= loc["x"] - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x", "t"], engine=eng, dtype="f64", **ip)
        m.set_parameter_constraints({"lengthscales": {**cons["lengthscales"], "scale": True}}, move_within_tol=True, tol=1e-2)
        m.optimise_parameters(max_iter=30)
        rows = preds.iloc[at:at + int((np.hypot(pred["x"] - loc["x"], pred["t"] - loc["t"]) <= 1.2).sum())]
        at += len(rows)
        assert len(rows) > 0 and (rows.index.get_level_values("x") == loc["x"]).all()
        out = m.predict(rows[["pred_loc_x", "pred_loc_t"]].values, gradient=True)
        np.testing.assert_array_equal(rows["f*"].values, out["f*"])
        for ci, c in enumerate(["x", "t"]):
            # the same tile at the same parameters; the table's unit is f*'s, the model's raw: one rounding apart
            np.testing.assert_allclose(rows[f"f*_grad_{c}"].values, out[f"f*_grad_{ci}"] / 0.5, rtol=1e-13, atol=0)
            np.testing.assert_allclose(rows[f"f*_grad_var_{c}"].values, out[f"f*_grad_var_{ci}"] / 0.25, rtol=1e-13, atol=0)
    assert at == len(preds)
