"""GPU: cross-validation that fits every held-out fold again (gpsat_fit_predict_batch_cv_refit).

The main checks compare no optimiser trajectories.  The folds run as one ordinary batch through the existing launch path,
so (1) the call is compared BYTE FOR BYTE with the same derived batch built here on the host and handed to plain
fit_predict_batch, (2) with the independent held-out phase of gpsat_fit_predict_batch_cv at fixed parameters, and (3) with
the fp64 oracle at the parameters the call returned.

"cv_mean - delta equal byte for byte": cv_mean is dtype(double(f*) + delta) by definition, and (f* + delta) - delta need not
round back to f*, so the test applies the same definition to the reference's f* -- dtype(double(f*_ref) + delta) -- and
compares bytes.  That pins every bit of cv_mean, and without recentre (delta = 0 exactly) it is f*_ref itself.
"""
import ctypes as C

import numpy as np
import pytest

from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from oracle import gp_oracle as go

pytestmark = pytest.mark.gpu

NAMES = ["RBF", "Matern12", "Matern32", "Matern52"]
FOLD_FIELDS = ["cv_theta", "cv_nll", "cv_status", "cv_n_eval", "cv_n_iter", "cv_n_obs", "cv_shift", "cv_label", "cv_fold_off"]
PLAIN_FIELDS = ["theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var"]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ"


def folds_of(obs_off, labels):
    """(tile, label, rows held out (bool over the tile)) of every fold, in the call's fold order."""
    out = []
    for t in range(len(obs_off) - 1):
        lab = labels[obs_off[t]:obs_off[t + 1]]
        out += [(t, int(v), lab == v) for v in np.unique(lab[lab >= 0])]
    return out


def derived_batch(b, labels, r, theta0, lo, hi, start):
    """The derived batch of the call ``r`` built on the host from the call's own fold_shift: the fitted folds in fold order."""
    dt = b["X"].dtype
    tiles, which = [], []
    for f, (t, v, G) in enumerate(folds_of(b["obs_off"], labels)):
        assert r.cv_label[f] == v and r.cv_n_obs[f] == (~G).sum()
        if r.cv_status[f] == 4:
            continue
        a, e = b["obs_off"][t], b["obs_off"][t + 1]
        X, y = b["X"][a:e], b["y"][a:e]
        tiles.append((X[~G], (y[~G].astype(np.float64) - r.cv_shift[f]).astype(dt), X[G],
                      r.theta[t] if start == "full" else theta0[t], lo[t], hi[t]))
        which.append((f, a + np.flatnonzero(G)))
    D = b["X"].shape[1]
    off = lambda k: np.concatenate([[0], np.cumsum([len(t_[k]) for t_ in tiles])]).astype(np.int64)
    kw = dict(D=D, obs_off=off(0), pred_off=off(2), X=np.concatenate([t_[0] for t_ in tiles]).reshape(-1, D),
              y=np.concatenate([t_[1] for t_ in tiles]), Xs=np.concatenate([t_[2] for t_ in tiles]).reshape(-1, D),
              theta0=np.array([t_[3] for t_ in tiles]), lo=np.array([t_[4] for t_ in tiles]), hi=np.array([t_[5] for t_ in tiles]))
    return kw, which


def ragged_labels(Ns, rng):
    """Shuffled labels with gaps; one -1 row, a one-row fold and a fold of 27 rows in the first tile (N = 33): with
    min_obs = 8 that fold leaves 6 rows and is not fitted."""
    labs = []
    for k, N in enumerate(Ns):
        if k == 0:
            lab = np.array([40] * 27 + [7] + [1000] * (N - 29) + [-1], dtype=np.int32)
        else:
            lab = (rng.integers(0, 5, N) * 37 + 3).astype(np.int32)
            lab[N // 2] = -1
        labs.append(rng.permutation(lab))
    return np.concatenate(labs)


def make_ragged(D, dtype, seed):
    Ns = [33, 64, 150]
    b = syn.make_batch(3, Ns, [5, 0, 3], D, 2, base_seed=seed, dtype=np.float32 if dtype == "f32" else np.float64)
    return b, ragged_labels(Ns, np.random.default_rng(seed)), np.ones((3, D + 2)), *syn.default_bounds(3, D)


# ---- 1. same bytes as the existing entry point
@pytest.mark.parametrize("recentre", [True, False])
@pytest.mark.parametrize("start", ["theta0", "full"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("D", [1, 3])
def test_same_bytes_as_the_plain_entry_point(eng, D, dtype, start, recentre):
    b, labels, th0, lo, hi = make_ragged(D, dtype, 300 + D)
    run = dict(kernel="Matern32", optimiser="lbfgs", max_iter=6, dtype=dtype)
    base = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th0, lo=lo, hi=hi)
    r = eng.fit_predict_batch(**base, **run, cv_fold=labels, cv_refit={"start": start, "recentre": recentre, "min_obs": 8})
    plain = eng.fit_predict_batch(**base, **run)
    for k in PLAIN_FIELDS:
        same_bytes(getattr(r, k), getattr(plain, k), f"plain output {k}")
    folds = folds_of(b["obs_off"], labels)
    assert len(folds) == r.cv_fold_off[-1] == len(r.cv_status) and (np.diff(r.cv_fold_off) == [3, 5, 5]).all()
    assert (r.cv_status == 4).sum() == 1
    skipped = int(np.flatnonzero(r.cv_status == 4)[0])
    assert r.cv_label[skipped] == 40 and r.cv_n_obs[skipped] == 6 and np.isnan(r.cv_theta[skipped]).all() and r.cv_n_eval[skipped] == 0
    kw, which = derived_batch(b, labels, r, th0, lo, hi, start)
    ref = eng.fit_predict_batch(**kw, **run)
    np_dt = b["X"].dtype.type
    fitted = np.array([f for f, _ in which])
    same_bytes(r.cv_theta[fitted], ref.theta, "cv_theta")
    same_bytes(r.cv_nll[fitted], ref.nll, "cv_nll")
    same_bytes(r.cv_status[fitted], ref.status, "cv_status")
    same_bytes(r.cv_n_eval[fitted], ref.n_eval, "cv_n_eval")
    same_bytes(r.cv_n_iter[fitted], ref.n_iter, "cv_n_iter")
    want = np.full((3, len(labels)), np.nan, dtype=np_dt)
    ymax = max(float(np.abs(b["y"]).max()), 1.0)
    for j, (f, rows) in enumerate(which):
        pa, pe = kw["pred_off"][j], kw["pred_off"][j + 1]
        if ref.status[j] in (2, 3):
            continue
        want[0, rows] = (ref.f_mean[pa:pe].astype(np.float64) + r.cv_shift[f]).astype(np_dt)
        want[1, rows], want[2, rows] = ref.f_var[pa:pe], ref.y_var[pa:pe]
        t, _, G = folds[f]
        a, e = b["obs_off"][t], b["obs_off"][t + 1]
        mean = float(np.mean(b["y"][a:e][~G].astype(np.float64)))
        if recentre:
            print(f"fold {f}: |shift - numpy mean| = {abs(r.cv_shift[f] - mean):.3e}")
            assert abs(r.cv_shift[f] - mean) <= 1e-15 * ymax
        else:
            assert r.cv_shift[f] == 0.0 and not np.signbit(r.cv_shift[f])
    same_bytes(r.cv_mean, want[0], "cv_mean")
    same_bytes(r.cv_f_var, want[1], "cv_f_var")
    same_bytes(r.cv_y_var, want[2], "cv_y_var")
    # NaN exactly at the rows never held out and the rows of the fold that was not fitted
    nan_rows = (labels < 0) | ((labels == 40) & (np.arange(len(labels)) < 33))
    assert (np.isnan(r.cv_mean) == nan_rows).all() and nan_rows.sum() == 27 + 3


# ---- 2. against the independent held-out phase, at fixed parameters
def test_against_the_held_out_phase(eng):
    N, D, kid = 150, 3, 2
    X, y, _, th = syn.make_tile(77, N, 0, D, kid)
    rng = np.random.default_rng(5)
    labels = rng.permutation(np.concatenate([np.repeat([0, 1, 2], 30), np.repeat(np.arange(7) + 10, 7), np.arange(11) + 100])).astype(np.int32)
    assert len(labels) == N and sorted(np.unique(np.bincount(labels)[np.bincount(labels) > 0])) == [1, 7, 30]
    kw = dict(D=D, obs_off=np.array([0, N]), X=X, y=y, pred_off=np.array([0, 0]), Xs=np.zeros((0, D)), theta0=th[None],
              kernel=NAMES[kid], optimiser="none", dtype="f64", cv_fold=labels)
    r = eng.fit_predict_batch(**kw, cv_refit={"recentre": False})
    c = eng.fit_predict_batch(**kw)
    assert (r.cv_status == 5).all() and (r.cv_shift == 0).all() and (r.cv_theta == th).all()
    ymax = max(float(np.abs(y).max()), 1.0)
    errs = [float(np.abs(np.asarray(a) - np.asarray(b_)).max()) for a, b_ in ((r.cv_mean, c.cv_mean), (r.cv_f_var, c.cv_f_var), (r.cv_y_var, c.cv_y_var))]
    print("refit at fixed theta against the held-out phase: max|mean|, |f_var|, |y_var| =", errs)
    assert errs[0] <= 1e-9 * ymax and errs[1] <= 1e-10 and errs[2] <= 1e-10


# ---- 3. against the oracle
@pytest.fixture(scope="module")
def oracle_case(eng):
    """The inputs of DESIGN.md section 13's CPU check, the oracle's refits from theta0 = 1 (computed once) and the fixed-theta
    held-out means of gpsat_fit_predict_batch_cv."""
    T, N, D, kid = 2, 150, 3, 0
    b = syn.make_batch(T, N, 4, D, kid, base_seed=900, dtype=np.float64)
    labels = np.tile(np.repeat(np.arange(5), 30), T).astype(np.int32)
    th0 = np.ones((T, D + 2))
    lo, hi = syn.default_bounds(T, D)
    tiles = []
    for t, v, G in folds_of(b["obs_off"], labels):
        a, e = b["obs_off"][t], b["obs_off"][t + 1]
        X, y = b["X"][a:e], b["y"][a:e]
        tiles.append((X[~G], y[~G] - y[~G].mean(), X[G], float(y[~G].mean()), a + np.flatnonzero(G)))
    off = lambda k: np.concatenate([[0], np.cumsum([len(t_[k]) for t_ in tiles])]).astype(np.int64)
    o = go.fit_predict_batch(kid, D, off(0), np.concatenate([t_[0] for t_ in tiles]), np.concatenate([t_[1] for t_ in tiles]), off(2),
                             np.concatenate([t_[2] for t_ in tiles]), np.ones((len(tiles), D + 2)), np.repeat(lo, 5, axis=0),
                             np.repeat(hi, 5, axis=0), np.ones(D + 2, bool), max_iter=1000)
    assert o["success"].all()
    base = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th0, lo=lo, hi=hi,
                kernel="RBF", optimiser="lbfgs", max_iter=1000, dtype="f64", cv_fold=labels)
    fixed = eng.fit_predict_batch(**base)
    return b, labels, tiles, off(2), o, base, fixed


@pytest.mark.parametrize("start", ["theta0", "full"])
def test_against_the_oracle(eng, oracle_case, start):
    b, labels, tiles, p_off, o, base, fixed = oracle_case
    D, kid = 3, 0
    r = eng.fit_predict_batch(**base, cv_refit={"start": start, "recentre": True})
    assert (r.cv_status == 0).all(), r.cv_status
    print(f"start={start}: evaluations per fold {r.cv_n_eval.tolist()}")
    ymax = max(float(np.abs(b["y"]).max()), 1.0)
    far = np.zeros(2)
    for f, (Xo, yo, Xp, shift, rows) in enumerate(tiles):
        # (a) at the returned parameters
        fm, fv, yv = go.predict(kid, Xo, yo, Xp, r.cv_theta[f])
        ea = (np.abs(r.cv_mean[rows] - (fm + shift)).max(), np.abs(r.cv_f_var[rows] - fv).max(), np.abs(r.cv_y_var[rows] - yv).max())
        # (b) against the oracle's own refit
        pa, pe = p_off[f], p_off[f + 1]
        eb = np.abs(r.cv_mean[rows] - (o["f_mean"][pa:pe] + shift)).max()
        print(f"fold {f}: at cv_theta mean {ea[0]:.2e} f_var {ea[1]:.2e} y_var {ea[2]:.2e}; refit: mean {eb:.2e} "
              f"nll {abs(r.cv_nll[f] - o['nll'][f]):.2e} theta rel {np.abs(r.cv_theta[f] / o['theta'][f] - 1).max():.2e}")
        assert abs(r.cv_shift[f] - shift) <= 1e-15 * ymax
        assert ea[0] <= 1e-9 * ymax and ea[1] <= 1e-10 and ea[2] <= 1e-10
        np.testing.assert_allclose(r.cv_theta[f], o["theta"][f], rtol=2e-3, atol=1e-5)
        np.testing.assert_allclose(r.cv_nll[f], o["nll"][f], rtol=0, atol=5e-5)
        assert eb <= 1e-4
        far[f // 5] = max(far[f // 5], np.abs(r.cv_mean[rows] - np.asarray(fixed.cv_mean)[rows]).max())
    # (c) the refit is told from none: per tile the refitted means leave the fixed-theta held-out means by more than 1e-2
    print("largest distance of the refitted from the fixed-theta held-out means, per tile:", far)
    assert (far > 1e-2).all()


# ---- 4. splitting (fp32: a tile's result does not depend on the batch it arrives in)
def test_split_calls_return_the_unsplit_bytes(eng):
    T, N, D = 6, 64, 3
    b = syn.make_batch(T, N, 2, D, 2, base_seed=410, dtype=np.float32)
    labels = np.tile(np.repeat(np.arange(4), 16), T).astype(np.int32)          # 4 folds: 192 expanded rows per tile
    lo, hi = syn.default_bounds(T, D)
    kw = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=np.ones((T, D + 2)), lo=lo,
              hi=hi, kernel="Matern32", optimiser="lbfgs", max_iter=5, dtype="f32", cv_fold=labels)
    whole = eng.fit_predict_batch(**kw, cv_refit=True)
    split = eng.fit_predict_batch(**kw, cv_refit={"max_expanded_rows": 400})   # two tiles per call: three calls
    for k in PLAIN_FIELDS + FOLD_FIELDS + ["cv_mean", "cv_f_var", "cv_y_var"]:
        same_bytes(getattr(split, k), getattr(whole, k), k)
    assert np.isfinite(whole.cv_mean).all()
    from gpsat_amd.engine import GpsatError
    with pytest.raises(GpsatError, match="tile 0 alone expands to 192 rows"):
        eng.fit_predict_batch(**kw, cv_refit={"max_expanded_rows": 100})


# ---- 5. determinism
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_second_call_same_bytes(eng, dtype):
    b, labels, th0, lo, hi = make_ragged(3, dtype, 520)
    kw = dict(D=3, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th0, lo=lo, hi=hi,
              kernel="Matern32", optimiser="lbfgs", max_iter=6, dtype=dtype, cv_fold=labels, cv_refit={"start": "full"})
    r1 = eng.fit_predict_batch(**kw)
    r2 = eng.fit_predict_batch(**kw)
    for k in PLAIN_FIELDS + FOLD_FIELDS + ["cv_mean", "cv_f_var", "cv_y_var"]:
        same_bytes(getattr(r1, k), getattr(r2, k), k)


def test_device_mode_equals_host_mode(eng):
    import torch
    b, labels, th0, lo, hi = make_ragged(3, "f32", 521)
    kw = dict(D=3, obs_off=b["obs_off"], pred_off=b["pred_off"], theta0=th0, lo=lo, hi=hi, kernel="Matern32", optimiser="lbfgs",
              max_iter=6, dtype="f32", cv_fold=labels, cv_refit=True)
    h = eng.fit_predict_batch(X=b["X"], y=b["y"], Xs=b["Xs"], **kw)
    d = eng.fit_predict_batch(X=torch.from_numpy(b["X"]).cuda(), y=torch.from_numpy(b["y"]).cuda(), Xs=torch.from_numpy(b["Xs"]).cuda(), **kw)
    for k in ["cv_mean", "cv_f_var", "cv_y_var", "f_mean"]:
        same_bytes(getattr(d, k).cpu().numpy(), getattr(h, k), k)
    for k in FOLD_FIELDS:
        same_bytes(getattr(d, k), getattr(h, k), k)


# ---- 6. errors
def test_every_refusal_names_its_argument(eng):
    D, N = 2, 12
    b = syn.make_batch(1, N, 2, D, 2, base_seed=7, dtype=np.float64)
    labels = np.repeat(np.arange(3), 4).astype(np.int32)
    from gpsat_amd.engine import _host_meta
    meta = _host_meta(D, (b["obs_off"], b["pred_off"]), np.ones((1, D + 2)), None, None, None)
    preds = tuple(np.empty(2) for _ in range(3))
    bt, res = eng._fill_batch(D, "f64", False, meta, (b["X"], b["y"], b["Xs"]), preds, "Matern32", "none", 0, 0, 0.0, 0.0, 0.0, False)
    lib, ptr = eng._lib, lambda a: a.ctypes.data_as(C.c_void_p)
    fold_off = np.array([0, 3], dtype=np.int64)
    cvo = [np.empty(N) for _ in range(3)]
    per = dict(fold_theta=np.empty((3, D + 2)), fold_nll=np.empty(3), fold_shift=np.empty(3), fold_status=np.empty(3, np.int32),
               fold_n_eval=np.empty(3, np.int32), fold_n_iter=np.empty(3, np.int32), fold_n_obs=np.empty(3, np.int32),
               fold_label=np.empty(3, np.int32))

    def call(batch=bt, **over):
        cv = L.GpsatCvRefit()
        f = dict(fold=ptr(labels), fold_off=ptr(fold_off), start=0, recentre=1, min_obs=1, cv_mean=ptr(cvo[0]), cv_f_var=ptr(cvo[1]),
                 cv_y_var=ptr(cvo[2]), **{k: ptr(v) for k, v in per.items()})
        f.update(over)
        for k, v in f.items():
            setattr(cv, k, v)
        rc = lib.gpsat_fit_predict_batch_cv_refit(eng._h, C.byref(batch), C.byref(cv))
        return rc, lib.gpsat_last_error().decode()

    assert call()[0] == 0 and call(fold_n_iter=None, cv_y_var=None)[0] == 0          # the two optional outputs
    assert lib.gpsat_fit_predict_batch_cv_refit(eng._h, C.byref(bt), None) == -1 and "NULL gpsat_cv_refit" in lib.gpsat_last_error().decode()
    for name in ["fold", "fold_off", "cv_mean", "cv_f_var", "fold_theta", "fold_nll", "fold_shift", "fold_status", "fold_n_eval",
                 "fold_n_obs", "fold_label"]:
        rc, msg = call(**{name: None})
        assert rc == -1 and f"{name} is NULL" in msg, (name, rc, msg)
    rc, msg = call(fold_off=ptr(np.array([0, 4], dtype=np.int64)))
    assert rc == -1 and "fold_off[1] = 4 differs from gpsat_cv_refit_count's 3" in msg
    for name in ("start", "recentre"):
        for bad in (-1, 2):
            rc, msg = call(**{name: bad})
            assert rc == -1 and f"{name} must be" in msg, (name, bad, msg)
    cov_off, f_cov = np.array([0, 4], dtype=np.int64), np.empty(4)
    bt.cov_off, bt.f_cov = ptr(cov_off), ptr(f_cov)
    rc, msg = call()
    assert rc == -1 and "cov_off / f_cov must be NULL" in msg
    bt.cov_off, bt.f_cov = None, None
    assert call()[0] == 0


# ---- 7. the layers above the engine
def test_model_cross_validate_refit_equals_the_engine(eng):
    from gpsat_amd.models import HipGPRModel
    N, D = 90, 2
    X, y, _, th = syn.make_tile(31, N, 0, D, 2)
    y = y + 3.0
    track = np.random.default_rng(2).integers(0, 4, N)
    m = HipGPRModel(coords=X, obs=y, kernel="Matern32", engine=eng, dtype="f64", verbose=False, obs_mean="local")
    out = m.cross_validate(track, refit=True, start="full", recentre=True, max_iter=8)
    from gpsat_amd.engine import factorise_folds
    r = eng.fit_predict_batch(dtype="f64", D=D, obs_off=np.array([0, N]), X=m.coords, y=m.obs[:, 0], pred_off=np.array([0, 0]),
                              Xs=np.zeros((0, D)), theta0=m._theta[None, :], lo=m._lo[None, :], hi=m._hi[None, :],
                              trainable=m._trainable, kernel="Matern32", optimiser="lbfgs", max_iter=8,
                              cv_fold=factorise_folds(track, N), cv_refit={"start": "full", "recentre": True})
    same_bytes(out["f*"], np.asarray(r.cv_mean), "f*")
    same_bytes(out["y_var"], np.asarray(r.cv_y_var), "y_var")
    same_bytes(out["theta"], r.cv_theta, "theta")
    same_bytes(out["shift"], r.cv_shift, "shift")
    assert len(out["theta"]) == 4 and np.isfinite(out["f*"]).all() and (out["f_bar"] == m.obs_mean[0, 0]).all()
    # the held-out residuals in raw units are of the size of the predictive standard deviation, not of the offset 3
    assert np.abs(y - (out["f_bar"] + out["f*"])).max() < 8 * np.sqrt(out["y_var"].max())


def test_orchestrator_refit_equals_the_engine_by_hand(eng, tmp_path):
    import pandas as pd
    from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
    rng = np.random.default_rng(1)
    n = 700
    df = pd.DataFrame({"x": rng.uniform(0, 10, n), "y": rng.uniform(0, 10, n), "track": rng.integers(0, 6, n)})
    df["z"] = 5.0 + np.sin(df["x"]) * np.cos(0.5 * df["y"]) + 0.1 * rng.standard_normal(n)
    xl = pd.DataFrame([(x, y) for x in (2.0, 4.0, 6.0, 8.0) for y in (2.0, 4.0, 6.0, 8.0)], columns=["x", "y"])
    data = {"data_source": df, "obs_col": "z", "coords_col": ["x", "y"], "local_select": [{"col": ["x", "y"], "comp": "<", "val": 2.5}]}
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "obs_mean": "local", "coords_scale": [2.0, 2.0]},
             "constraints": {"lengthscales": {"low": [0.1, 0.1], "high": [20, 20]}}, "optim_kwargs": {"max_iter": 6}}
    cv = {"by": ["track"], "refit": True, "start": "theta0"}
    store = str(tmp_path / "s")
    oi = BatchedLocalExpertOI({"source": xl}, data, model, {"method": "expert_loc"}, engine=eng, dtype="f32", cv=cv)
    out = oi.run(store, store_every=8, min_obs=20)
    cvp, par, rd = out["cv_preds"], out["cv_params"], out["run_details"]
    assert len(rd) == 16 and len(cvp) == int(rd["num_obs"].sum()) and len(par) == 16 * 6
    # the engine by hand, on the arrays the orchestrator packs for the same experts (fp32: a tile's result does not depend
    # on the batch it arrives in, so one call over all 16 tiles gives the bytes of the two waves)
    plan = oi._plan(np.arange(16), None, True, True, 20, "", 1)
    pk = oi._pack_job(plan, plan.profiles[0], np.arange(16))
    pf = plan.profiles[0]
    r = eng.fit_predict_batch(D=2, obs_off=pk["o_off"], X=pk["X"], y=pk["y"], pred_off=pk["p_off"], Xs=pk["Xs"], theta0=plan.theta0,
                              lo=plan.lo, hi=plan.hi, trainable=pf.trainable, kernel=pf.kernel, optimiser=pf.optimiser,
                              max_iter=pf.max_iter, dtype="f32", cv_fold=pk["cv_fold"],
                              cv_refit={"start": "theta0", "recentre": True, "min_obs": 20}, **pf.eng_kw)
    same_bytes(cvp["f*"].values, np.asarray(r.cv_mean, dtype=np.float64), "cv_preds f*")
    same_bytes(cvp["y_var"].values, np.asarray(r.cv_y_var, dtype=np.float64), "cv_preds y_var")
    same_bytes(par["kernel_variance"].values, r.cv_theta[:, 2], "cv_params kernel_variance")
    same_bytes(par["lengthscales_1"].values, r.cv_theta[:, 1], "cv_params lengthscales_1")
    same_bytes(par["objective_value"].values, r.cv_nll, "cv_params objective_value")
    same_bytes(par["num_obs"].values, r.cv_n_obs.astype(np.int64), "cv_params num_obs")
    np.testing.assert_array_equal(par["optimise_success"].values, r.cv_status == 0)
    np.testing.assert_allclose(par["f_bar"].values, np.repeat(pk["mean"], 6) + r.cv_shift, rtol=1e-15)
    assert np.isfinite(cvp["f*"].values).all() and (rd["cv_rows_skipped"] == 0).all()
    # a resumed run leaves the store's tables unchanged
    before = get_results(store, expert_order=True)
    out2 = BatchedLocalExpertOI({"source": xl}, data, model, {"method": "expert_loc"}, engine=eng, dtype="f32", cv=cv).run(store, store_every=8, min_obs=20)
    assert len(out2.get("cv_params", [])) == 0
    after = get_results(store, expert_order=True)
    for name in ("cv_preds", "cv_params", "run_details"):
        pd.testing.assert_frame_equal(after[name], before[name])
