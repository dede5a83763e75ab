"""GPU: the joint log predictive density of every held-out fold (cv_joint), both flavours -- from the tile's own factor
(gpsat_fit_predict_batch_cv_joint) and from refitted folds (gpsat_fit_predict_batch_cv_refit_joint) -- against the NumPy
restatement of tests/cv_joint_numpy.py.

Bound of every comparison with the restatement: 1e-9 max(1, |lpd|), the scale the held-out mean is held to
(tests/test_gpu_cv.py); the restatement's two routes differ by 6.7e-15 relative, |lpd| up to 329 (tests/test_cv_joint_cpu.py).  No NaN is
masked: exactly the folds a test names are NaN.
"""
import ctypes as C

import numpy as np
import pytest

import cv_joint_numpy as cjn
import cv_numpy as cvn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from variant_cases import eng, eng8  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KID, KERNEL = 2, "Matern32"
PLAIN = ("theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var")
CV = ("cv_mean", "cv_f_var", "cv_y_var")


def _pack(tiles):
    """tiles: list of (X, y, Xs, theta) -> the packed arrays of Engine.fit_predict_batch."""
    D = tiles[0][0].shape[1]
    obs_off = np.concatenate([[0], np.cumsum([len(t[1]) for t in tiles])]).astype(np.int64)
    pred_off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int64)
    return dict(D=D, obs_off=obs_off, pred_off=pred_off, X=np.concatenate([t[0] for t in tiles]).reshape(-1, D),
                y=np.concatenate([t[1] for t in tiles]), Xs=np.concatenate([t[2] for t in tiles]).reshape(-1, D),
                theta0=np.array([t[3] for t in tiles]), dtype="f64", kernel=KERNEL)


def _tile(N, D, P=0):
    return syn.make_tile(700 + N, N, P, D, KID)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold(got, ref, what):
    """Every fold finite and within 1e-9 max(1, |lpd|) of the restatement; the largest error is printed."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(ref).all() and np.isfinite(got).all(), (what, got)
    err = cjn.rel_err(got, ref)
    print(f"cv_joint {what}: {len(ref)} folds, max |lpd| {np.abs(ref).max(initial=0.0):.4g}, max rel err {err:.3e}")
    assert err <= 1e-9, what


def _ragged():
    """Three tiles N = 17 / 0 / 150, D = 3: leave-one-out by label on the first, runs of 1..30 with every 11th row never held
    out on the third."""
    rng = np.random.default_rng(11)
    tiles = [_tile(17, 3, 2), _tile(0, 3, 1), _tile(150, 3, 3)]
    l150 = cvn.run_labels(150, rng, 1, 30)
    l150[::11] = -1
    labels = [np.arange(17, dtype=np.int32)[::-1].copy(), np.zeros(0, dtype=np.int32), l150]
    return tiles, labels


# ---- factor flavour
@pytest.mark.parametrize("build", ["eng", "eng8"])
def test_factor_ragged_batch_against_both_routes(build, request):
    e = request.getfixturevalue(build)
    tiles, labels = _ragged()
    r = e.fit_predict_batch(optimiser="none", cv_fold=np.concatenate(labels), cv_joint=True, **_pack(tiles))
    assert r.status[0] == 5 and r.status[2] == 5
    nf = [len(cjn.folds(lab, len(lab))) for lab in labels]
    assert (r.cv_fold_off == np.concatenate([[0], np.cumsum(nf)])).all() and len(r.cv_lpd) == sum(nf)
    for t in (0, 2):
        X, y, _, th = tiles[t]
        got = r.cv_lpd[r.cv_fold_off[t]:r.cv_fold_off[t + 1]]
        _hold(got, cjn.deletion(KID, X, y, th, labels[t]), f"factor ragged {build} tile {t} (deletion)")
        _hold(got, cjn.closed_form(KID, X, y, th, labels[t]), f"factor ragged {build} tile {t} (closed form)")


def test_factor_folds_across_block_boundaries_and_shuffled(eng):  # noqa: F811
    N, D = 33, 1
    X, y, _, th = _tile(N, D)
    straddle = np.zeros(N, dtype=np.int32)
    straddle[10:21] = 1                                  # rows 10..20: one fold over the 16-row block boundary
    straddle[21:] = 2
    shuffled = np.random.default_rng(4).permutation(np.arange(N) % 5).astype(np.int32)
    for name, lab in (("straddle", straddle), ("shuffled", shuffled)):
        r = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_joint=True, **_pack([(X, y, np.zeros((0, D)), th)]))
        _hold(r.cv_lpd, cjn.deletion(KID, X, y, th, lab), f"factor N=33 D=1 {name}")


def test_factor_fold_at_the_limit(eng):  # noqa: F811
    N, D = 300, 2
    X, y, _, th = _tile(N, D)
    lab = np.full(N, -1, dtype=np.int32)
    lab[20:276] = 7
    assert (lab == 7).sum() == L.max_cv_fold("f64", D) == 256
    r = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_joint=True, **_pack([(X, y, np.zeros((0, D)), th)]))
    assert (r.cv_fold_off == [0, 1]).all()
    _hold(r.cv_lpd, cjn.deletion(KID, X, y, th, lab), "factor one fold of 256 in N=300")


def test_factor_whole_tile_is_the_prior(eng):  # noqa: F811
    N, D = 64, 3
    X, y, _, th = _tile(N, D)
    r = eng.fit_predict_batch(optimiser="none", cv_fold=np.zeros(N, dtype=np.int32), cv_joint=True,
                              **_pack([(X, y, np.zeros((0, D)), th)]))
    _hold(r.cv_lpd, cjn.deletion(KID, X, y, th, np.zeros(N, dtype=np.int32)), "factor whole tile N=64 (the prior)")


def test_factor_bitwise_identity(eng):  # noqa: F811
    tiles, labels = _ragged()
    b, lab = _pack(tiles), np.concatenate(labels)
    for kw in (dict(optimiser="none"), dict(optimiser="lbfgs", max_iter=6, lo=syn.default_bounds(3, 3)[0], hi=syn.default_bounds(3, 3)[1])):
        r0 = eng.fit_predict_batch(cv_fold=lab, **b, **kw)
        r1 = eng.fit_predict_batch(cv_fold=lab, cv_joint=True, **b, **kw)
        r2 = eng.fit_predict_batch(cv_fold=lab, cv_joint=True, **b, **kw)
        assert r0.cv_lpd is None and r0.cv_fold_off is None
        for name in PLAIN + CV:
            assert _bits(getattr(r0, name), getattr(r1, name)), name
        assert _bits(r1.cv_lpd, r2.cv_lpd) and np.isfinite(r1.cv_lpd).all()
    # the 150-row tile alone: the bytes it has inside the ragged batch
    alone = eng.fit_predict_batch(optimiser="none", cv_fold=labels[2], cv_joint=True, **_pack(tiles[2:]))
    inside = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_joint=True, **b)
    assert _bits(alone.cv_lpd, inside.cv_lpd[inside.cv_fold_off[2]:])


def test_factor_loo_equals_the_univariate_terms(eng):  # noqa: F811
    tiles = [_tile(17, 3), _tile(130, 3)]
    b = _pack(tiles)
    r = eng.fit_predict_batch(optimiser="none", cv_fold="loo", cv_joint=True, **b)
    assert (r.cv_fold_off == b["obs_off"]).all()
    _hold(r.cv_lpd, cjn.univariate(b["y"], r.cv_mean, r.cv_y_var), "factor loo against the call's own cv_mean / cv_y_var")
    for t, (X, y, _, th) in enumerate(tiles):
        _hold(r.cv_lpd[b["obs_off"][t]:b["obs_off"][t + 1]], cjn.closed_form(KID, X, y, th), f"factor loo tile {t} (closed form)")


def test_factor_failed_tile_is_nan_and_alone(eng):  # noqa: F811
    """Identical rows, kernel variance 1 and a likelihood variance below fp64's resolution of it: the second pivot of K_y is
    exactly 0 (the recipe of tests/test_gpu_parity.py::test_not_positive_definite_is_reported, in fp64)."""
    D = 3
    good = [_tile(17, D), _tile(40, D)]
    bad = (np.zeros((20, D)), np.ones(20), np.zeros((0, D)), np.array([1.0] * D + [1.0, 1e-300]))
    tiles = [good[0], bad, good[1]]
    labels = [np.arange(17, dtype=np.int32) // 3, np.arange(20, dtype=np.int32) // 4, np.arange(40, dtype=np.int32) // 7]
    r = eng.fit_predict_batch(optimiser="none", cv_fold=np.concatenate(labels), cv_joint=True, **_pack(tiles))
    assert r.status[1] == 2 and r.status[0] == 5 and r.status[2] == 5
    off = r.cv_fold_off
    assert np.isnan(r.cv_lpd[off[1]:off[2]]).all() and off[2] - off[1] == 5
    for t in (0, 2):
        X, y, _, th = tiles[t]
        _hold(r.cv_lpd[off[t]:off[t + 1]], cjn.deletion(KID, X, y, th, labels[t]), f"factor beside a failed tile, tile {t}")


def _ctypes_batch(e, D, b):
    from gpsat_amd.engine import _host_meta
    meta = _host_meta(D, (b["obs_off"], b["pred_off"]), b["theta0"], None, None, None)
    P = int(b["pred_off"][-1])
    preds = tuple(np.empty(max(P, 1)) for _ in range(3))
    bt, res = e._fill_batch(D, "f64", False, meta, (b["X"], b["y"], b["Xs"]), preds, KERNEL, "none", 0, 0, 0.0, 0.0, 0.0, False)
    return bt, (meta, preds, res)


def test_factor_refusals_leave_the_handle_usable(eng):  # noqa: F811
    N, D = 24, 2
    X, y, _, th = _tile(N, D)
    b = _pack([(X, y, np.zeros((0, D)), th)])
    labels = (np.arange(N) // 5).astype(np.int32)
    bt, keep = _ctypes_batch(eng, D, b)
    lib, ptr = eng._lib, lambda a: a.ctypes.data_as(C.c_void_p)
    cvo = [np.empty(N) for _ in range(3)]
    cv = L.GpsatCv()
    cv.fold, cv.cv_mean, cv.cv_f_var, cv.cv_y_var = ptr(labels), ptr(cvo[0]), ptr(cvo[1]), ptr(cvo[2])
    fold_off, lpd = np.array([0, 5], dtype=np.int64), np.full(5, 7.0)

    def call(null=False, **over):
        jt = L.GpsatCvJoint()
        jt.fold_off, jt.fold_lpd = ptr(fold_off), ptr(lpd)
        for k, v in over.items():
            if k == "reserved3":
                jt.reserved[3] = v
            else:
                setattr(jt, k, v)
        rc = lib.gpsat_fit_predict_batch_cv_joint(eng._h, C.byref(bt), C.byref(cv), None if null else C.byref(jt))
        return rc, lib.gpsat_last_error().decode()

    assert call()[0] == 0
    good = lpd.copy()
    _hold(good, cjn.deletion(KID, X, y, th, labels), "factor through ctypes")
    for over, text in ((dict(null=True), "NULL gpsat_cv_joint"), (dict(fold_lpd=None), "fold_lpd is NULL"),
                       (dict(fold_off=None), "fold_off is NULL"), (dict(reserved3=1), "reserved[3] must be 0"),
                       (dict(fold_off=ptr(np.array([0, 6], dtype=np.int64))), "fold_off[1] = 6 differs from gpsat_cv_refit_count's 5")):
        rc, msg = call(**over)
        assert rc == -1 and text in msg, (over, rc, msg)
        lpd[:] = 7.0
        assert call()[0] == 0 and _bits(lpd, good), over


# ---- refit flavour (fp64)
REFIT_NS = (33, 64, 150)


def test_refit_refusals_leave_the_handle_usable(eng):  # noqa: F811
    """The refit entry point's own refusals through ctypes -- the struct's, a differing fold_off and GPSAT_F32, which the
    Python wrapper refuses before the library is called -- each followed by a good call with unchanged bytes."""
    from gpsat_amd.engine import _host_meta
    N, D, F = 24, 2, 5
    X, y, _, th = _tile(N, D)
    b = _pack([(X, y, np.zeros((0, D)), th)])
    labels = (np.arange(N) // 5).astype(np.int32)
    bt, keep = _ctypes_batch(eng, D, b)
    meta = _host_meta(D, (b["obs_off"], b["pred_off"]), b["theta0"], None, None, None)
    p32 = tuple(np.empty(1, dtype=np.float32) for _ in range(3))
    d32 = (b["X"].astype(np.float32), b["y"].astype(np.float32), b["Xs"].astype(np.float32))
    bt32, keep32 = eng._fill_batch(D, "f32", False, meta, d32, p32, KERNEL, "none", 0, 0, 0.0, 0.0, 0.0, False)
    lib, ptr = eng._lib, lambda a: a.ctypes.data_as(C.c_void_p)
    fold_off, lpd = np.array([0, F], dtype=np.int64), np.full(F, 7.0)
    cvo = [np.empty(N) for _ in range(3)]
    per = dict(fold_theta=np.empty((F, D + 2)), fold_nll=np.empty(F), fold_shift=np.empty(F), fold_status=np.empty(F, np.int32),
               fold_n_eval=np.empty(F, np.int32), fold_n_iter=np.empty(F, np.int32), fold_n_obs=np.empty(F, np.int32),
               fold_label=np.empty(F, np.int32))
    cv = L.GpsatCvRefit()
    for k, v in dict(fold=ptr(labels), fold_off=ptr(fold_off), start=0, recentre=0, min_obs=1, cv_mean=ptr(cvo[0]), cv_f_var=ptr(cvo[1]),
                     cv_y_var=ptr(cvo[2]), **{k: ptr(v) for k, v in per.items()}).items():
        setattr(cv, k, v)

    def call(null=False, batch=bt, **over):
        jt = L.GpsatCvJoint()
        jt.fold_off, jt.fold_lpd = ptr(fold_off), ptr(lpd)
        for k, v in over.items():
            if k == "reserved3":
                jt.reserved[3] = v
            else:
                setattr(jt, k, v)
        rc = lib.gpsat_fit_predict_batch_cv_refit_joint(eng._h, C.byref(batch), C.byref(cv), None if null else C.byref(jt))
        return rc, lib.gpsat_last_error().decode()

    assert call()[0] == 0
    good = lpd.copy()
    _hold(good, cjn.deletion(KID, X, y, th, labels), "refit through ctypes")
    for over, text in ((dict(null=True), "NULL gpsat_cv_joint"), (dict(fold_lpd=None), "fold_lpd is NULL"),
                       (dict(fold_off=None), "fold_off is NULL"), (dict(reserved3=1), "reserved[3] must be 0"),
                       (dict(fold_off=ptr(np.array([0, 6], dtype=np.int64))), "fold_off[1] = 6 differs from gpsat_cv_refit_count's 5"),
                       (dict(batch=bt32), "GPSAT_F64 only")):
        rc, msg = call(**over)
        assert rc == -1 and text in msg, (over, rc, msg)
        lpd[:] = 7.0
        assert call()[0] == 0 and _bits(lpd, good), over


def _refit_inputs(D):
    rng = np.random.default_rng(20 + D)
    tiles = [(X, y + 2.5, Xs, th) for X, y, Xs, th in (_tile(N, D, 2) for N in REFIT_NS)]     # a mean worth removing
    labels = [rng.permutation(np.arange(33) % 4).astype(np.int32), cvn.run_labels(64, rng, 1, 20), (np.arange(150) // 30).astype(np.int32)]
    labels[2][::13] = -1
    return tiles, labels


@pytest.mark.parametrize("recentre", [False, True])
@pytest.mark.parametrize("D", [1, 3])
def test_refit_at_theta0_against_deletion_and_the_factor_flavour(eng, D, recentre):  # noqa: F811
    tiles, labels = _refit_inputs(D)
    b, lab = _pack(tiles), np.concatenate(labels)
    r = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit={"recentre": recentre}, cv_joint=True, **b)
    assert (r.cv_status == 5).all()
    for t, (X, y, _, th) in enumerate(tiles):
        got = r.cv_lpd[r.cv_fold_off[t]:r.cv_fold_off[t + 1]]
        _hold(got, cjn.deletion(KID, X, y, th, labels[t], recentre=recentre), f"refit theta0 D={D} recentre={recentre} tile {t}")
    if not recentre:
        f = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_joint=True, **b)
        assert (f.cv_fold_off == r.cv_fold_off).all()
        _hold(r.cv_lpd, f.cv_lpd, f"refit at theta0 against the factor flavour D={D}")


def _fitted_case():
    b = syn.make_batch(2, 150, 4, 3, 0, base_seed=900, dtype=np.float64)
    lab = np.tile((np.arange(150) // 30).astype(np.int32), 2)
    lo, hi = syn.default_bounds(2, 3)
    kw = dict(D=3, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=np.ones((2, 5)), lo=lo, hi=hi,
              kernel="RBF", optimiser="lbfgs", max_iter=40, dtype="f64", cv_fold=lab)
    return b, lab, kw


def test_refit_fitted_folds_against_the_restatement_at_their_theta(eng):  # noqa: F811
    b, lab, kw = _fitted_case()
    r = eng.fit_predict_batch(cv_refit=True, cv_joint=True, **kw)
    assert (r.cv_status <= 1).all() and (r.cv_n_eval > 1).all()
    for t in range(2):
        a, e = int(b["obs_off"][t]), int(b["obs_off"][t + 1])
        f0, f1 = int(r.cv_fold_off[t]), int(r.cv_fold_off[t + 1])
        ref = cjn.deletion(0, b["X"][a:e].reshape(-1, 3), b["y"][a:e], None, lab[a:e], recentre=True, thetas=r.cv_theta[f0:f1])
        _hold(r.cv_lpd[f0:f1], ref, f"refit fitted tile {t}")
    r2 = eng.fit_predict_batch(cv_refit=True, cv_joint=True, **kw)
    assert _bits(r.cv_lpd, r2.cv_lpd) and _bits(r.cv_theta, r2.cv_theta)


def test_refit_skipped_fold_is_the_only_nan(eng):  # noqa: F811
    N, D = 40, 2
    X, y, _, th = _tile(N, D)
    lab = np.where(np.arange(N) < 30, 0, 1 + (np.arange(N) - 30) // 5).astype(np.int32)      # fold 0 leaves 10 rows
    r = eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit={"min_obs": 11, "recentre": False}, cv_joint=True,
                              **_pack([(X, y, np.zeros((0, D)), th)]))
    assert (r.cv_status == [4, 5, 5]).all()
    assert np.isnan(r.cv_lpd[0]) and np.isfinite(r.cv_lpd[1:]).all()
    _hold(r.cv_lpd[1:], cjn.deletion(KID, X, y, th, lab)[1:], "refit beside a skipped fold")


def test_refit_f32_is_refused_and_budget_counts_the_covariances(eng):  # noqa: F811
    from gpsat_amd.engine import GpsatError
    N, D = 40, 2
    X, y, _, th = _tile(N, D)
    lab = (np.arange(N) // 20).astype(np.int32)
    b = _pack([(X, y, np.zeros((0, D)), th)])
    with pytest.raises(GpsatError, match="fp64 only"):
        eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit=True, cv_joint=True, **dict(b, dtype="f32"))
    # 2 folds of 20: 40 expanded rows, and 2 * 400 covariance elements = 267 rows of D + 1 = 3 elements
    eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit={"max_expanded_rows": 40}, **b)
    eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit={"max_expanded_rows": 307}, cv_joint=True, **b)
    with pytest.raises(GpsatError, match="tile 0 alone expands to 307 rows"):
        eng.fit_predict_batch(optimiser="none", cv_fold=lab, cv_refit={"max_expanded_rows": 306}, cv_joint=True, **b)


@pytest.mark.parametrize("refit", [False, True])
def test_device_tensors_return_the_host_bytes(eng, refit):  # noqa: F811
    import torch
    tiles, labels = _refit_inputs(3)
    b, lab = _pack(tiles), np.concatenate(labels)
    kw = dict(optimiser="none", cv_fold=lab, cv_joint=True, **({"cv_refit": True} if refit else {}))
    h = eng.fit_predict_batch(**kw, **b)
    dev = torch.device("cuda", eng.device_id)
    d = eng.fit_predict_batch(**kw, **dict(b, **{k: torch.from_numpy(np.ascontiguousarray(b[k])).to(dev) for k in ("X", "y", "Xs")}))
    assert _bits(h.cv_lpd, d.cv_lpd) and (h.cv_fold_off == d.cv_fold_off).all() and np.isfinite(h.cv_lpd).all()
    for name in CV:
        assert _bits(np.asarray(getattr(h, name)), getattr(d, name).cpu().numpy()), name


# ---- the layers above the engine
def test_model_cross_validate_joint_equals_the_engine(eng):  # noqa: F811
    from gpsat_amd.engine import factorise_folds
    from gpsat_amd.models import HipGPRModel
    N, D = 90, 2
    X, y, _, th = _tile(N, D)
    track = np.array(["t%d" % v for v in np.random.default_rng(2).integers(0, 4, N)], dtype=object)
    m = HipGPRModel(coords=X, obs=y + 3.0, kernel=KERNEL, engine=eng, dtype="f64", verbose=False, obs_mean="local")
    m.set_parameters(lengthscales=th[:D], kernel_variance=th[D], likelihood_variance=th[D + 1])
    assert set(m.cross_validate(track)) == {"f*", "f*_var", "y_var", "f_bar"}
    codes = factorise_folds(track, N)
    for refit in (False, True):
        out = m.cross_validate(track, joint=True, **({"refit": True, "optimiser": "none", "recentre": False} if refit else {}))
        assert (out["fold"] == np.arange(4)).all() and (out["fold_size"] == np.bincount(codes)).all()
        _hold(out["lpd"], cjn.deletion(KID, m.coords, m.obs[:, 0], th, codes), f"model cross_validate joint refit={refit}")
    loo = m.cross_validate(joint=True)
    assert (loo["fold"] == np.arange(N)).all() and (loo["fold_size"] == 1).all()
    _hold(loo["lpd"], cjn.univariate(m.obs[:, 0], loo["f*"], loo["y_var"]), "model cross_validate joint leave-one-out")


@pytest.mark.parametrize("refit", [False, True])
def test_orchestrator_cv_folds_equal_the_model_tile_by_tile(eng, refit):  # noqa: F811
    """refit=False: a fitted run, cv_folds at every expert's fitted parameters.  refit=True: the run and the model both with
    the optimiser off, so every fold sits at theta0 -- this holds the table's bookkeeping and units for the refit flavour, not
    folds that moved; fitted folds are held at engine level (test_refit_fitted_folds_against_the_restatement_at_their_theta)."""
    import pandas as pd
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    from gpsat_amd.models import HipGPRModel
    rng = np.random.default_rng(8)
    n, osc = 400, 0.5
    df = pd.DataFrame({"x": np.sort(rng.uniform(0, 12, n))})
    df["track"] = (np.arange(n) // 16) % 5
    df["z"] = 4.0 + np.sin(df["x"]) + 0.1 * rng.standard_normal(n)
    xl = pd.DataFrame({"x": [2.0, 4.0, 6.0, 8.0, 10.0]})
    data = {"data_source": df, "obs_col": "z", "coords_col": ["x"], "local_select": [{"col": ["x"], "comp": "<", "val": 2.0}]}
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": KERNEL, "obs_mean": "local", "coords_scale": [2.0], "obs_scale": osc},
             "constraints": {"lengthscales": {"low": [0.05], "high": [20]}}, "optim_kwargs": {"max_iter": 6}}
    cv = {"by": ["track"], **({"refit": True} if refit else {})}
    args = ({"source": xl}, data, model, {"method": "expert_loc"})
    base = BatchedLocalExpertOI(*args, engine=eng, dtype="f64", cv=cv).run(None, optimise=not refit)
    out = BatchedLocalExpertOI(*args, engine=eng, dtype="f64", cv=cv, cv_joint=True).run(None, optimise=not refit)
    for name, tab in base.items():                      # the other tables are those of the run without cv_joint
        a, b = out[name].drop(columns=["run_time"], errors="ignore"), tab.drop(columns=["run_time"], errors="ignore")
        if refit:                                       # the refit flavour's folds are planned as a batch with f_cov: no bits claimed
            pd.testing.assert_frame_equal(a, b, check_exact=False, rtol=1e-9, atol=1e-9)
        else:
            pd.testing.assert_frame_equal(a, b)
    cvf, cvp = out["cv_folds"], out["cv_preds"]
    assert list(cvf.columns) == ["track", "n", "lpd", "lpd_marginal"] and len(cvf.index.unique()) == 5
    ls, kv, lv = out["lengthscales"], out["kernel_variance"], out["likelihood_variance"]
    for key in cvf.index.unique():
        f, rows = cvf.loc[[key]], cvp.loc[[key]]
        d = df.iloc[rows["obs_index"].values]
        m = HipGPRModel(data=d, obs_col="z", coords_col=["x"], coords_scale=[2.0], obs_scale=osc, obs_mean="local", kernel=KERNEL,
                        engine=eng, dtype="f64", verbose=False)
        m.set_parameters(lengthscales=ls.loc[[key]]["lengthscales"].values, kernel_variance=float(kv.loc[[key]]["kernel_variance"].values[0]),
                         likelihood_variance=float(lv.loc[[key]]["likelihood_variance"].values[0]))
        ref = m.cross_validate(d["track"].values, joint=True, **({"refit": True, "optimiser": "none"} if refit else {}))
        # the model numbers the folds by first appearance, the table by the code in the selected frame: match on the size-ordered label
        first = d["track"].values[np.unique(factorise(d["track"].values), return_index=True)[1]]
        got = f.set_index("track").loc[first]
        assert (got["n"].values == ref["fold_size"]).all()
        _hold(got["lpd"].values, ref["lpd"] - ref["fold_size"] * np.log(osc), f"orchestrator cv_folds refit={refit} expert {key}")
        for tr, lm in zip(got.index, got["lpd_marginal"].values):
            g = rows[rows["track"] == tr]
            mean, var = g["f_bar"].values + osc * g["f*"].values, osc * osc * g["y_var"].values
            want = float(np.sum(-0.5 * (g["z"].values - mean) ** 2 / var - 0.5 * np.log(2.0 * np.pi * var)))
            assert abs(lm - want) <= 1e-12 * max(1.0, abs(want))


def factorise(labels):
    from gpsat_amd.engine import factorise_folds
    return factorise_folds(labels, len(labels))
