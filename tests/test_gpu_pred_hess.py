"""GPU: the second derivatives of the posterior mean at the prediction points, their variances and the weighted Laplacian
(gpsat_fit_predict_batch_hess, Engine.fit_predict_batch(pred_hess=...)) against the fp64 restatement
tests/pred_hess_numpy.py, on the 4-wave and the 8-wave build.

Bounds, after check_tile and tests/test_gpu_pred_grad.py.  l_a l_b f_hess_ab is a sum of the kind f_mean is (V^T z with V = L^-1
of a right-hand side of the kernel's size) and l_a^2 l_b^2 f_hess_var_ab one of the kind f_var is (a prior term minus V^T V):
    l_a l_b |error of f_hess_ab| <= 1e-9 max(|y|max, 1),      l_a^2 l_b^2 |error of f_hess_var_ab| <= 2.5e-9
-- f_var's 1e-10 per unit of prior factor, which is up to 3 hh(0) = 25 here.  The Laplacian's right-hand side is of size
S = sum_a c_a / l_a^2 and its prior factor is hh(0) (2 sum_a c_a^2 / l_a^4 + S^2), with hh(0) taken as 25/3 for both kernels:
    |error of f_lap| <= 1e-9 max(|y|max, 1) S,      |error of f_lap_var| <= 1e-10 (25/3) (2 sum_a c_a^2 / l_a^4 + S^2)
(in one dimension with c = 1 these are the pair's bounds).
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import pred_grad_numpy as pg
import pred_hess_numpy as ph
import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd.engine import Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel
from variant_cases import FIELDS, Case, check_tile, eng, eng8, one, ragged_inputs, run, same  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

HESS_FIELDS = FIELDS + ("f_hess", "f_hess_var", "f_lap", "f_lap_var")
PER_POINT = ("f_mean", "f_var", "y_var", "f_hess", "f_hess_var", "f_lap", "f_lap_var", "f_grad", "f_grad_var")
RAGGED_SPEC = {"dims": [0, 2], "lap_weight": [0.7, 0.0, 2.0]}                    # of the ragged batch (D = 3)


class HessCase(Case):
    """The plain model (variant_numpy's NOISE with v = 0, which changes no bit of K_y) with pred_hess; the ragged batch, which
    variant_cases draws for Matern32, is Matern52 here."""
    variant, name = vn.NOISE, "hess"

    def call_kw(self, b):
        return {"pred_hess": b.get("pred_hess", True)}

    def batch(self, T, N, P, D, kernel, base_seed):
        b = super().batch(T, N, P, D, "Matern52" if kernel == "Matern32" else kernel, base_seed)
        b["obs_var"] = np.zeros(int(b["obs_off"][-1]))
        for t in range(T):                                 # the tile's first prediction point lies on one of its observations
            a, e, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
            if e > a and pe > pa:
                b["Xs"][pa] = b["X"][a + min(5, e - a - 1)]
        if isinstance(N, list):
            b["pred_hess"] = RAGGED_SPEC
        return b


HESS = HessCase()
WORST = {"hess": 0.0, "var": 0.0, "lap": 0.0, "lap_var": 0.0}   # largest errors seen in this module, in units of their bounds' scales


def check_hess_tile(r, b, t, theta, spec, what=""):
    """Tile t's outputs against the restatement at ``theta``, to the bounds of the module docstring; the prior, exactly, for a
    tile without observations.  ``spec``: the call's pred_hess as a dict with dims and lap_weight (None: no Laplacian)."""
    D, kernel = b["D"], b["kernel"]
    a, e, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
    pairs = ph.pairs(spec["dims"])
    assert r.hess_pairs == pairs
    fh, fhv = np.asarray(r.f_hess)[pa:pe], np.asarray(r.f_hess_var)[pa:pe]
    assert fh.shape == fhv.shape == (pe - pa, len(pairs))
    w = spec["lap_weight"]
    assert (r.f_lap is None) == (w is None) and (r.f_lap_var is None) == (w is None)
    if pe == pa:
        return
    ref = ph.predict_hess(kernel, b["X"][a:e], b["y"][a:e], b["Xs"][pa:pe], theta, spec["dims"], np.zeros(D) if w is None else w)
    if e == a:
        np.testing.assert_array_equal(fh, 0.0)
        # the same products in another order, a dozen roundings (two dozen for the Laplacian's sums) of 1.1e-16 each
        np.testing.assert_allclose(fhv, ref[1], rtol=2e-15, atol=0)
        if w is not None:
            np.testing.assert_array_equal(np.asarray(r.f_lap)[pa:pe], 0.0)
            np.testing.assert_allclose(np.asarray(r.f_lap_var)[pa:pe], ref[3], rtol=4e-15, atol=0)
        return
    ell, ymax = theta[:D], max(np.abs(b["y"][a:e]).max(), 1.0)
    sc = np.array([ell[i] * ell[j] for i, j in pairs])
    eh, ev = np.abs(fh - ref[0]) * sc, np.abs(fhv - ref[1]) * sc ** 2
    WORST["hess"], WORST["var"] = max(WORST["hess"], eh.max() / ymax), max(WORST["var"], ev.max())
    assert eh.max() <= 1e-9 * ymax, (what, t, int(e - a), eh.max())
    assert ev.max() <= 2.5e-9, (what, t, int(e - a), ev.max())
    if w is not None:
        wl = np.asarray(w) / ell ** 2
        S, F = wl.sum(), (25.0 / 3.0) * (2.0 * np.sum(wl ** 2) + wl.sum() ** 2)
        el, elv = np.abs(np.asarray(r.f_lap)[pa:pe] - ref[2]).max() / S, np.abs(np.asarray(r.f_lap_var)[pa:pe] - ref[3]).max() / F
        WORST["lap"], WORST["lap_var"] = max(WORST["lap"], el / ymax), max(WORST["lap_var"], elv)
        assert el <= 1e-9 * ymax, (what, t, int(e - a), el)
        assert elv <= 1e-10, (what, t, int(e - a), elv)


# ---- 1. fixed parameters against the restatement
#       smallest   below a block   one block   a row past   5 block rows: the     a wave's second pair      middle-sized
#                                              a block      second 4-row panel    of chunks on both builds
SHAPES = [(1, 2, 1), (15, 5, 2), (16, 16, 3), (17, 33, 4), (65, 17, 3),          (40, 261, 3),             (100, 33, 3)]
W4 = [1.3, 0.2, 3.0, 0.6]


def _specs(D):
    """dims = all with unequal weights; a single coordinate (the last), without a Laplacian at D = 3; {1, 3} at D = 4."""
    out = [{"dims": list(range(D)), "lap_weight": W4[:D]},
           {"dims": [D - 1], "lap_weight": None if D == 3 else [0.0] * (D - 1) + [1.0]}]
    if D == 4:
        out.append({"dims": [1, 3], "lap_weight": [0.0, 0.5, 0.0, 2.0]})
    return out


@pytest.mark.parametrize("N,P,D", SHAPES)
def test_fixed_parameters_match_the_restatement(eng, eng8, N, P, D):
    for kernel in ph.KERNELS:
        b = HESS.batch(2, N, P, D, kernel, 7000 + N)
        th = HESS.theta(np.random.default_rng(N + D), 2, D)
        for spec in _specs(D):
            for e_, what in ((eng, "4-wave"), (eng8, "8-wave")):
                r = run(HESS, e_, b, th, pred_hess=spec)
                npair = len(ph.pairs(spec["dims"]))
                assert r.f_hess.shape == r.f_hess_var.shape == (2 * P, npair) and r.f_hess.dtype == np.float64
                assert (r.status == 5).all() and r.f_grad is None
                for t in range(2):
                    check_tile(HESS, r, b, t, th[t], what)
                    check_hess_tile(r, b, t, th[t], spec, f"{what} {kernel} {spec}")
                # (one de-meaned observation is y = 0: the posterior mean is flat)
                assert (N == 1 or np.abs(r.f_hess).max() > 0) and (r.f_hess_var > 0).all()
    print("largest scaled errors so far:", WORST)


def test_true_means_every_coordinate_and_unit_weights(eng):
    b = HESS.batch(1, 30, 9, 3, "RBF", 7100)
    th = HESS.theta(np.random.default_rng(1), 1, 3)
    r = run(HESS, eng, b, th, pred_hess=True)
    r1 = run(HESS, eng, b, th, pred_hess={"dims": [2, 0, 1], "lap_weight": [1.0, 1.0, 1.0]})
    same(r, r1, "True against the spelled-out call", HESS_FIELDS)
    check_hess_tile(r, b, 0, th[0], {"dims": [0, 1, 2], "lap_weight": [1.0, 1.0, 1.0]}, "True")
    # unit weights: the Laplacian is the sum of the diagonal second derivatives, from a solve of its own
    diag = [k for k, (i, j) in enumerate(r.hess_pairs) if i == j]
    np.testing.assert_allclose(r.f_lap, r.f_hess[:, diag].sum(axis=1), rtol=0, atol=1e-9 * np.sum(1.0 / th[0, :3] ** 2))


# ---- 2. the other outputs are the plain call's bytes; the gradient through this entry point is the gradient call's
@pytest.mark.parametrize("opt", [dict(optimiser="none"), dict(optimiser="lbfgs", max_iter=12)], ids=["none", "lbfgs"])
def test_other_outputs_are_the_bytes_of_the_plain_call_and_of_the_gradient_call(eng, eng8, opt):
    b, th = ragged_inputs(HESS)
    th0 = th if opt["optimiser"] == "none" else np.ones(th.shape)
    lo, hi = HESS.bounds(len(th), b["D"])
    for e_ in (eng, eng8):
        r = run(HESS, e_, b, th0, lo=lo, hi=hi, **opt)
        r0 = run(HESS, e_, b, th0, lo=lo, hi=hi, pred_hess=False, **opt)
        assert r0.f_hess is None and r0.f_lap is None and r.f_hess is not None and r.f_grad is None
        same(r, r0, f"pred_hess against the plain call, {opt['optimiser']}")
        rg = run(HESS, e_, b, th0, lo=lo, hi=hi, pred_hess=False, pred_grad=True, **opt)
        rb = run(HESS, e_, b, th0, lo=lo, hi=hi, pred_grad=True, **opt)
        assert rg.f_hess is None and rg.f_grad is not None
        same(rb, rg, f"the gradient through the new entry point, {opt['optimiser']}", FIELDS + ("f_grad", "f_grad_var"))
        same(rb, r, f"the second derivatives beside the gradient, {opt['optimiser']}", HESS_FIELDS)
        if opt["optimiser"] != "none":
            assert r.n_eval.max() > 6 and (r.theta != th0).any()


# ---- 3. a ragged, unsorted batch: every tile has the bits it has alone, on a second call and time-sliced
@pytest.fixture(scope="module")
def ragged(eng):
    b, th = ragged_inputs(HESS)
    return b, th, run(HESS, eng, b, th)


def test_ragged_batch(ragged):
    b, th, r = ragged
    Ns, Ps = np.diff(b["obs_off"]), np.diff(b["pred_off"])
    assert len(Ns) == 60 and Ns.max() <= 200 and Ns[3] == 0 and Ps[3] > 0 and Ps[5] == 0 and Ns[5] > 0 and r.status[3] == 4
    assert b["kernel"] == "Matern52" and r.f_hess.shape == (int(Ps.sum()), 3) and r.f_lap.shape == (int(Ps.sum()),)
    for t in range(60):
        check_tile(HESS, r, b, t, th[t], "ragged")
        check_hess_tile(r, b, t, th[t], RAGGED_SPEC, "ragged")
    pa, pe = b["pred_off"][3], b["pred_off"][4]                         # the empty tile: the prior at theta0
    np.testing.assert_array_equal(r.f_hess[pa:pe], 0.0)
    np.testing.assert_array_equal(r.f_lap[pa:pe], 0.0)
    l0, l2, sf2 = th[3, 0], th[3, 2], th[3, 3]
    np.testing.assert_allclose(r.f_hess_var[pa:pe], np.tile(sf2 * (25.0 / 3.0) * np.array([3 / l0 ** 4, 1 / (l0 * l2) ** 2, 3 / l2 ** 4]),
                                                            (pe - pa, 1)), rtol=2e-15)
    wl = np.array([0.7 / l0 ** 2, 2.0 / l2 ** 2])
    np.testing.assert_allclose(r.f_lap_var[pa:pe], sf2 * (25.0 / 3.0) * (2 * np.sum(wl ** 2) + wl.sum() ** 2), rtol=4e-15)
    print("largest scaled errors so far:", WORST)


def _part(r, b, t, name):
    whole = getattr(r, name)
    return whole[b["pred_off"][t]:b["pred_off"][t + 1]] if name in PER_POINT else whole[[t]]


def test_same_bits_alone_in_the_batch_and_again(eng, ragged):
    b, th, r = ragged
    same(run(HESS, eng, b, th), r, "second call", HESS_FIELDS)
    for t in (3, 5, 17, 40):                                             # the empty tile, the tile with P = 0, the largest, any
        r1 = run(HESS, eng, one(b, t), th[[t]], pred_hess=RAGGED_SPEC)
        for name in HESS_FIELDS:
            assert np.asarray(getattr(r1, name)).tobytes() == np.asarray(_part(r, b, t, name)).tobytes(), (t, name)


def test_time_sliced_optimisation_is_bit_identical(eng, ragged, monkeypatch):
    """The queue forced as tests/test_gpu_variants.py forces it: suspended after every evaluation, after every third of a
    200-point tile, or never."""
    b, th, _ = ragged
    lo, hi = HESS.bounds(60, 3)
    th0 = np.ones(th.shape)
    kw = dict(lo=lo, hi=hi, optimiser="lbfgs", max_iter=12)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "0")
    r0 = run(HESS, eng, b, th0, **kw)
    assert r0.n_eval.max() > 6 and (r0.status <= 1).sum() > 40
    for seg in ("1", str(3 * 14 ** 3)):
        monkeypatch.setenv("GPSAT_DEBUG_SEG", seg)
        same(run(HESS, eng, b, th0, **kw), r0, f"slice {seg}", HESS_FIELDS)
    monkeypatch.delenv("GPSAT_DEBUG_SEG")
    t = 17
    r1 = run(HESS, eng, one(b, t), th0[[t]], lo=lo[[t]], hi=hi[[t]], optimiser="lbfgs", max_iter=12, pred_hess=RAGGED_SPEC)
    for name in HESS_FIELDS:
        assert np.asarray(getattr(r1, name)).tobytes() == np.asarray(_part(r0, b, t, name)).tobytes(), (t, name)
    # at the fitted parameters the outputs are the restatement's
    for t in (17, 40):
        if r0.status[t] <= 1:
            check_hess_tile(r0, b, t, r0.theta[t], RAGGED_SPEC, "fitted")


# ---- 4. device tensors
def test_device_tensors_return_the_bits_of_host_mode(eng, ragged):
    import torch
    b, th, _ = ragged
    r = run(HESS, eng, b, th, pred_grad=True)
    dev = torch.device("cuda", eng.device_id)
    X, y, Xs = (torch.tensor(b[k], device=dev) for k in ("X", "y", "Xs"))
    rd = eng.fit_predict_batch(D=3, obs_off=b["obs_off"], X=X, y=y, pred_off=b["pred_off"], Xs=Xs, theta0=th, kernel=b["kernel"],
                               dtype="f64", optimiser="none", want_grad=True, pred_hess=RAGGED_SPEC, pred_grad=True)
    assert isinstance(rd.f_hess, torch.Tensor) and rd.f_hess.is_cuda and rd.f_hess.shape == r.f_hess.shape
    assert isinstance(rd.f_lap_var, torch.Tensor) and isinstance(rd.f_grad, torch.Tensor)
    for name in HESS_FIELDS + ("f_grad", "f_grad_var"):
        v = getattr(rd, name)
        v = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        assert v.tobytes() == np.asarray(getattr(r, name)).tobytes(), name
    np.testing.assert_array_equal(X.cpu().numpy(), b["X"])               # the inputs are read only
    np.testing.assert_array_equal(Xs.cpu().numpy(), b["Xs"])
    # a batch without prediction points, in either mode
    e0 = dict(D=3, obs_off=[0, 20], pred_off=[0, 0], theta0=np.ones((1, 5)), kernel="RBF", dtype="f64", optimiser="none", pred_hess=True)
    rh = eng.fit_predict_batch(X=b["X"][:20], y=b["y"][:20], Xs=np.zeros((0, 3)), **e0)
    rz = eng.fit_predict_batch(X=X[:20].contiguous(), y=y[:20].contiguous(), Xs=torch.zeros((0, 3), dtype=torch.float64, device=dev), **e0)
    assert rh.f_hess.shape == (0, 6) and tuple(rz.f_hess_var.shape) == (0, 6) and tuple(rz.f_lap.shape) == (0,)
    assert rh.nll.tobytes() == rz.nll.tobytes()


# ---- 5. refusals leave the handle usable
def test_every_refusal_is_followed_by_a_good_call_with_the_same_bits(eng, ragged):
    b, th, r = ragged
    t = 40
    b1, th1 = one(b, t), th[[t]]
    good = run(HESS, eng, b1, th1, pred_hess=RAGGED_SPEC)
    lib, sumP = eng._lib, int(b1["pred_off"][-1])
    OUT = ("f_hess", "f_hess_var", "f_lap", "f_lap_var", "f_grad", "f_grad_var")

    def raw_call(kernel="Matern52", dtype="f64", reserved=None, missing=(), cov=False, dims=0b101, weights=(0.7, 0.0, 2.0, 0.0)):
        """The entry point itself: the Python wrapper refuses most of these before the library sees them."""
        np_dt = np.float32 if dtype == "f32" else np.float64
        H = 6 if kernel == "RationalQuadratic" else 5
        meta = ((np.asarray(b1["obs_off"], dtype=np.int64), np.asarray(b1["pred_off"], dtype=np.int64)),
                np.ascontiguousarray(th1[:, :5] if H == 5 else np.ones((1, 6))), np.full((1, H), np.nan), np.full((1, H), np.nan),
                np.ones(H, dtype=np.uint8))
        data = tuple(np.ascontiguousarray(b1[k], dtype=np_dt) for k in ("X", "y", "Xs"))
        preds = tuple(np.empty(sumP, dtype=np_dt) for _ in range(3))
        bb, res = Engine._fill_batch(3, dtype, False, meta, data, preds, kernel, "none", 0, 0, 0.0, 0.0, 0.0, False)
        outs = {f: np.empty(sumP * 6) for f in OUT}
        s = L.GpsatPredHess()
        for f in OUT:
            setattr(s, f, None if f in missing else outs[f].ctypes.data)
        s.dims = dims
        for a, c in enumerate(weights):
            s.lap_weight[a] = c
        if reserved is not None:
            s.reserved[reserved] = 1
        cov_off, fc = np.array([0, sumP * sumP], dtype=np.int64), np.empty(sumP * sumP, dtype=np_dt)
        if cov:
            bb.cov_off, bb.f_cov = cov_off.ctypes.data, fc.ctypes.data
        rc = lib.gpsat_fit_predict_batch_hess(eng._h, C.byref(bb), C.byref(s))
        return rc, lib.gpsat_last_error().decode(), outs

    rc, _, outs = raw_call()
    assert rc == 0
    assert outs["f_hess"][:sumP * 3].tobytes() == good.f_hess.tobytes() and outs["f_lap_var"][:sumP].tobytes() == good.f_lap_var.tobytes()
    for kw, match in ((dict(dtype="f32"), "GPSAT_F64 only"), (dict(kernel="Matern12"), "not mean-square differentiable"),
                      (dict(kernel="Matern32"), "not mean-square differentiable"), (dict(kernel="RationalQuadratic"), "not built for kernel 4"),
                      (dict(reserved=3), "reserved"), (dict(dims=0), "dims is empty"), (dict(dims=0b1001), ">= D"),
                      (dict(missing=("f_hess",)), "f_hess is NULL"), (dict(missing=("f_hess_var",)), "f_hess_var is NULL"),
                      (dict(missing=("f_lap",)), "f_lap is NULL"), (dict(missing=("f_lap_var",)), "f_lap_var is NULL"),
                      (dict(missing=("f_grad",)), "together"), (dict(weights=(0.7, 0.0, -2.0, 0.0)), "negative or not finite"),
                      (dict(weights=(0.7, 0.0, float("nan"), 0.0)), "negative or not finite"),
                      (dict(weights=(0.7, 1.0, 2.0, 0.0)), "outside dims"), (dict(cov=True), "full covariance")):
        rc, why, _ = raw_call(**kw)
        assert rc == -1 and match in why, (kw, rc, why)
        same(run(HESS, eng, b1, th1, pred_hess=RAGGED_SPEC), good, f"after the refusal of {kw}", HESS_FIELDS)
    rc = lib.gpsat_fit_predict_batch_hess(eng._h, None, None)
    assert rc == -1
    for more in (dict(full_cov=True), dict(cv_fold="loo"), dict(n_starts=2), dict(obs_var=np.zeros(int(b1["obs_off"][-1]))), dict(dtype="f32"),
                 dict(kernel="Matern32")):
        with pytest.raises(GpsatError, match="pred_hess"):
            eng.fit_predict_batch(**{**dict(D=3, obs_off=b1["obs_off"], X=b1["X"], y=b1["y"], pred_off=b1["pred_off"], Xs=b1["Xs"],
                                            theta0=th1, kernel="Matern52", dtype="f64", optimiser="none", pred_hess=RAGGED_SPEC), **more})
        same(run(HESS, eng, b1, th1, pred_hess=RAGGED_SPEC), good, f"after the wrapper's refusal of {sorted(more)}", HESS_FIELDS)
    for name in HESS_FIELDS:                                              # ... and they are the tile's bits inside the batch
        assert np.asarray(getattr(good, name)).tobytes() == np.asarray(_part(r, b, t, name)).tobytes(), name


# ---- 6. the model and the orchestrator
def test_model_predict_hessian_in_raw_units(eng):
    rng = np.random.default_rng(11)
    N, D = 120, 3
    X = rng.uniform(0.0, 4.0, (N, D)) * np.array([10.0, 1.0, 100.0])
    y = 5.0 + 2.0 * np.sin(X[:, 0] / 10.0 + X[:, 1]) * np.cos(X[:, 2] / 100.0) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(0.0, 4.0, (17, D)) * np.array([10.0, 1.0, 100.0])
    Xs[0] = X[7]
    cs, osc = np.array([10.0, 1.0, 100.0]), 2.0
    for kernel in ph.KERNELS:
        m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", coords_scale=cs, obs_scale=osc, obs_mean="local", kernel=kernel,
                        kernel_kwargs={"lengthscales": [1.1, 0.9, 1.6], "variance": 0.8}, noise_variance=0.02)
        theta = np.array([1.1, 0.9, 1.6, 0.8, 0.02])
        out, plain = m.predict(Xs, hessian=True, gradient=True), m.predict(Xs)
        ys = (y - y.mean()) / osc
        ymax = max(np.abs(ys).max(), 1.0)
        w = 1.0 / cs ** 2
        fh, fhv, fl, flv = ph.predict_hess(kernel, X / cs, ys, Xs / cs, theta, lap_weight=w)
        for k, (a, b) in enumerate(ph.pairs(range(D))):
            # the device's bounds in scaled units, carried to raw units by the factors of the conversion
            f = osc / (cs[a] * cs[b])
            np.testing.assert_allclose(out[f"f*_hess_{a}_{b}"], f * fh[:, k], rtol=0, atol=1e-9 * ymax / (theta[a] * theta[b]) * f)
            np.testing.assert_allclose(out[f"f*_hess_var_{a}_{b}"], f ** 2 * fhv[:, k], rtol=0, atol=2.5e-9 / (theta[a] * theta[b]) ** 2 * f ** 2)
        wl = w / theta[:D] ** 2
        np.testing.assert_allclose(out["f*_lap"], osc * fl, rtol=0, atol=1e-9 * ymax * wl.sum() * osc)
        np.testing.assert_allclose(out["f*_lap_var"], osc ** 2 * flv, rtol=0,
                                   atol=1e-10 * (25.0 / 3.0) * (2 * np.sum(wl ** 2) + wl.sum() ** 2) * osc ** 2)
        only_grad = m.predict(Xs, gradient=True)
        for k in range(D):
            np.testing.assert_array_equal(out[f"f*_grad_{k}"], only_grad[f"f*_grad_{k}"])
            np.testing.assert_array_equal(out[f"f*_grad_var_{k}"], only_grad[f"f*_grad_var_{k}"])
        for k in plain:
            np.testing.assert_array_equal(plain[k], out[k])
    with pytest.raises(NotImplementedError, match="full_cov"):
        m.predict(Xs, full_cov=True, hessian=True)


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
                      "pred_kwargs": {"hessian": True, "gradient": True}},
        pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.2})
    assert oi.dtype == "f64"
    preds = oi.run(store_path=None)["preds"]
    at = 0
    cc = ["x", "t"]
    for k, loc in locs.iterrows():
        d = df[(df["x"] <= loc["x"] + radius) & (df["x"] >= loc["x"] - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=cc, engine=eng, dtype="f64", **ip)
        m.set_parameter_constraints({"lengthscales": {**cons["lengthscales"], "scale": True}}, move_within_tol=True, tol=1e-2)
        m.optimise_parameters(max_iter=30)
        rows = preds.iloc[at:at + int((np.hypot(pred["x"] - loc["x"], pred["t"] - loc["t"]) <= 1.2).sum())]
        at += len(rows)
        assert len(rows) > 0 and (rows.index.get_level_values("x") == loc["x"]).all()
        out = m.predict(rows[["pred_loc_x", "pred_loc_t"]].values, hessian=True, gradient=True)
        np.testing.assert_array_equal(rows["f*"].values, out["f*"])
        # the same tile at the same parameters; the table's unit is f*'s, the model's raw: a rounding or two apart
        for a, b in ((0, 0), (0, 1), (1, 1)):
            np.testing.assert_allclose(rows[f"f*_hess_{cc[a]}_{cc[b]}"].values, out[f"f*_hess_{a}_{b}"] / 0.5, rtol=1e-13, atol=0)
            np.testing.assert_allclose(rows[f"f*_hess_var_{cc[a]}_{cc[b]}"].values, out[f"f*_hess_var_{a}_{b}"] / 0.25, rtol=1e-13, atol=0)
        np.testing.assert_allclose(rows["f*_lap"].values, out["f*_lap"] / 0.5, rtol=1e-13, atol=0)
        np.testing.assert_allclose(rows["f*_lap_var"].values, out["f*_lap_var"] / 0.25, rtol=1e-13, atol=0)
        for ci, c in enumerate(cc):
            np.testing.assert_allclose(rows[f"f*_grad_{c}"].values, out[f"f*_grad_{ci}"] / 0.5, rtol=1e-13, atol=0)
    assert at == len(preds)
