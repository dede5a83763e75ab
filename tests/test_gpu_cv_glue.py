"""GPU: gpsat_glue_keyed_batch against its NumPy restatement (tests/glue_keyed_numpy.py) at the glue bound of
tests/test_gpu_post.py, its determinism, the capacity protocol, and held-out predictions glued and scored end to end by
BatchedLocalExpertOI(cv_glue=...)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import glue_keyed_numpy as gk

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-14
# every edge of a team of 8 lanes (and of 16 and of a wave, whichever is chosen), one row, and a group of many rounds
SIZES = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import default_engine
    return default_engine()


def rows(sizes, ndim=2, nvars=3, seed=0, keys=None, sigma_rows=False, shuffle=True):
    """Shuffled rows of groups of the given sizes: key, pred, xprt, vals, sigma.  Values around 3 (predictions, not
    residuals: no cancellation in the weighted sums), experts within a few sigma of the prediction location."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    keys = np.arange(len(sizes), dtype=np.int64) * 3 + 1 if keys is None else np.asarray(keys, dtype=np.int64)
    key = np.repeat(keys, sizes)
    R = len(key)
    pred = np.repeat(rng.uniform(0, 100, (ndim, len(sizes))), sizes, axis=1)
    xprt = pred + rng.uniform(-4, 4, (ndim, R))
    vals = rng.normal(3.0, 1.0, (nvars, R))
    sigma = rng.uniform(1.0, 3.0, R) if sigma_rows else 1.75
    if shuffle:
        p = rng.permutation(R)
        key, pred, xprt, vals = key[p], pred[:, p], xprt[:, p], vals[:, p]
        sigma = sigma[p] if sigma_rows else sigma
    return key, pred, xprt, vals, sigma


def agree(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].shape == want[2].shape
    np.testing.assert_array_equal(np.isnan(got[2]), np.isnan(want[2]))
    np.testing.assert_allclose(got[2], want[2], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("sigma_rows", [False, True])
@pytest.mark.parametrize("nvars", [1, 4])
@pytest.mark.parametrize("ndim", [1, 2])
def test_group_sizes_against_the_restatement(eng, ndim, nvars, sigma_rows):
    a = rows(SIZES, ndim, nvars, seed=10 * ndim + nvars, sigma_rows=sigma_rows)
    got = eng.glue_keyed_batch(*a)
    agree(got, gk.glue_keyed(*a))
    np.testing.assert_array_equal(got[1], SIZES)
    # negative keys among them are ignored altogether
    key = a[0].copy()
    key[::5] = -1 - key[::5]
    agree(eng.glue_keyed_batch(key, *a[1:]), gk.glue_keyed(key, *a[1:]))


def test_degenerate_calls(eng):
    a = rows([1], seed=1)
    agree(eng.glue_keyed_batch(*a), gk.glue_keyed(*a))                       # R = 1
    np.testing.assert_allclose(eng.glue_keyed_batch(*a)[2][:, 0], a[3][:, 0], rtol=1e-15)     # one row: w v / w
    a = rows([1000], seed=2)                                                  # all keys equal
    got = eng.glue_keyed_batch(*a)
    agree(got, gk.glue_keyed(*a))
    assert got[1].tolist() == [1000]
    a = rows(np.ones(1000, dtype=int), seed=3)                                # all keys distinct
    got = eng.glue_keyed_batch(*a)
    agree(got, gk.glue_keyed_fast(*a))
    srt = np.argsort(a[0])
    np.testing.assert_allclose(got[2], a[3][:, srt], rtol=1e-15)
    key = -1 - a[0]                                                           # all keys negative
    got = eng.glue_keyed_batch(key, *a[1:])
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].shape == (3, 0)
    e = np.zeros((2, 0))                                                      # no rows
    got = eng.glue_keyed_batch(np.zeros(0, dtype=np.int64), e, e, np.zeros((3, 0)), 1.0)
    assert got[0].shape == (0,) and got[2].shape == (3, 0)


def test_keys_up_to_2_62(eng):
    keys = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 53 + 1, 2 ** 62 - 1, 2 ** 62]
    a = rows([3, 1, 9, 2, 17, 4, 8, 5], keys=keys, seed=4)
    got = eng.glue_keyed_batch(*a)
    agree(got, gk.glue_keyed(*a))
    np.testing.assert_array_equal(got[0], keys)


def test_nan_values_follow_glue_batch(eng):
    """A NaN value is left out of the numerator, its weight stays in the denominator; a group of NaN values alone gives 0."""
    key, pred, xprt, vals, sigma = rows([5, 9, 3, 1], nvars=2, seed=5)
    vals[0, key == key.min()] = np.nan                    # a whole group of variable 0
    vals[1, ::4] = np.nan
    got = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)
    agree(got, gk.glue_keyed(key, pred, xprt, vals, sigma))
    assert got[2][0, 0] == 0.0 and np.isfinite(got[2]).all()


def test_max_dist(eng):
    key, pred, xprt, vals, sigma = rows(SIZES, seed=6)
    md = 3.0
    d2 = ((pred - xprt) ** 2).sum(axis=0)
    assert (np.abs(d2 - md * md) > 1e-9 * md * md).all()  # no row at the boundary: the kernel's d2 may differ in its last bit
    assert 0.2 < (d2 < md * md).mean() < 0.8
    far = key == key.max()                                # one key with all its rows outside
    xprt[:, far] = pred[:, far] + 2.5
    got = eng.glue_keyed_batch(key, pred, xprt, vals, sigma, max_dist=md)
    want = gk.glue_keyed(key, pred, xprt, vals, sigma, max_dist=md)
    agree(got, want)
    assert got[1][-1] == 0 and np.isnan(got[2][:, -1]).all() and (got[1][:-1] <= SIZES[:-1]).all() and got[1].sum() < len(key)
    for off in (None, np.inf, 0.0, -2.0):                 # no limit
        np.testing.assert_array_equal(eng.glue_keyed_batch(key, pred, xprt, vals, sigma, max_dist=off)[1], SIZES)
    # exactly on the boundary, exact under any contraction: (dx, dy, max_dist) = (3, 4, 5) is outside (strict)
    key = np.array([7, 7, 7, 8])
    pred = np.array([[10.0, 10.0, 10.0, 20.0], [10.0, 10.0, 10.0, 20.0]])
    xprt = pred + np.array([[3.0, -3.0, 1.0, 4.0], [4.0, 4.0, 1.0, -3.0]])
    vals = np.array([[100.0, 200.0, 5.0, 9.0]])
    k, c, o = eng.glue_keyed_batch(key, pred, xprt, vals, 2.0, max_dist=5.0)
    assert k.tolist() == [7, 8] and c.tolist() == [1, 0] and abs(o[0, 0] - 5.0) < 1e-14 and np.isnan(o[0, 1])
    k, c, o = eng.glue_keyed_batch(key, pred, xprt, vals, 2.0, max_dist=np.nextafter(5.0, 6.0))
    assert c.tolist() == [3, 1] and abs(o[0, 1] - 9.0) < 1e-14
    # one dimension
    k, c, o = eng.glue_keyed_batch(key, pred[:1], xprt[:1], vals, 2.0, max_dist=3.0)
    assert c.tolist() == [1, 0]


def test_against_glue_batch_on_rows_sorted_on_the_host(eng):
    for sigma_rows in (False, True):
        key, pred, xprt, vals, sigma = rows(SIZES + [3] * 50, seed=7, sigma_rows=sigma_rows)
        order = np.argsort(key, kind="stable")
        uniq, cnt = np.unique(key, return_counts=True)
        seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        want = eng.glue_batch(seg, pred[:, order], xprt[:, order], vals[:, order], sigma[order] if sigma_rows else sigma)
        keys, counts, out = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)
        np.testing.assert_array_equal(keys, uniq)
        np.testing.assert_array_equal(counts, cnt)
        np.testing.assert_allclose(out, want, rtol=RTOL, atol=ATOL)


def test_a_group_depends_on_its_own_rows_only(eng):
    key, pred, xprt, vals, sigma = rows(SIZES, seed=8, sigma_rows=True)
    cols = lambda sel: (key[sel], pred[:, sel], xprt[:, sel], vals[:, sel], sigma[sel])
    base = eng.glue_keyed_batch(key, pred, xprt, vals, sigma, max_dist=4.5)
    again = eng.glue_keyed_batch(key, pred, xprt, vals, sigma, max_dist=4.5)
    for u, v in zip(base, again):
        assert u.tobytes() == v.tobytes()                 # a second call: the same bytes
    rng = np.random.default_rng(0)
    R = len(key)
    for j, k in enumerate(base[0]):
        mine = np.nonzero(key == k)[0]
        others = np.nonzero(key != k)[0]
        # the rows of the other keys permuted among their places (this key's rows stay where they are)
        perm = np.arange(R)
        perm[others] = rng.permutation(others)
        got = eng.glue_keyed_batch(*cols(perm), max_dist=4.5)
        np.testing.assert_array_equal(got[0], base[0])
        assert got[2][:, j].tobytes() == base[2][:, j].tobytes() and got[1][j] == base[1][j], ("permuted", k)
        if j % 3:
            continue
        # rows of other keys removed (every second one), the order of the rest kept
        keep = np.sort(np.concatenate([mine, others[::2]]))
        got = eng.glue_keyed_batch(*cols(keep), max_dist=4.5)
        i = int(np.searchsorted(got[0], k))
        assert got[0][i] == k and got[2][:, i].tobytes() == base[2][:, j].tobytes() and got[1][i] == base[1][j], ("removed", k)
        # rows added: new keys below, between and above, and ignored rows, interleaved
        extra = rows([4, 70, 1, 9], seed=100 + j, keys=[0, int(k) + 1, 2 ** 40, 2 ** 62], sigma_rows=True)
        ek = extra[0].copy()
        ek[::6] = -1
        ins = np.sort(rng.integers(0, R + 1, len(ek)))
        more = (np.insert(key, ins, ek), np.insert(pred, ins, extra[1], axis=1), np.insert(xprt, ins, extra[2], axis=1),
                np.insert(vals, ins, extra[3], axis=1), np.insert(sigma, ins, extra[4]))
        got = eng.glue_keyed_batch(*more, max_dist=4.5)
        i = int(np.searchsorted(got[0], k))
        assert got[0][i] == k and got[2][:, i].tobytes() == base[2][:, j].tobytes() and got[1][i] == base[1][j], ("added", k)
    # alone in the call
    k = base[0][5]
    got = eng.glue_keyed_batch(*cols(np.nonzero(key == k)[0]), max_dist=4.5)
    assert got[2][:, 0].tobytes() == base[2][:, 5].tobytes()


def test_capacity_too_small_reports_G_and_the_handle_stays_usable(eng):
    key, pred, xprt, vals, sigma = rows(SIZES, seed=9)
    pred, xprt, vals = (np.ascontiguousarray(a) for a in (pred, xprt, vals))      # handed to the library as they are
    base = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)
    lib, h = eng._lib, eng._h
    R, G = len(key), len(SIZES)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(cap):
        ok, oc, out, n = np.full(max(cap, 1), -5, dtype=np.int64), np.full(max(cap, 1), -5, dtype=np.int32), np.full((3, max(cap, 1)), -5.0), C.c_int64(-1)
        rc = lib.gpsat_glue_keyed_batch(h, R, 2, 3, ptr(key), ptr(pred), ptr(xprt), ptr(vals), float(sigma), None, float("inf"), cap,
                                        C.byref(n), ptr(ok), ptr(oc), ptr(out))
        return rc, int(n.value), ok, oc, out

    for cap in (G - 1, 1):
        rc, n, ok, oc, out = call(cap)
        assert rc == -1 and n == G and f"capacity {cap} < G {G}" in lib.gpsat_last_error().decode()
        assert (ok == -5).all() and (oc == -5).all() and (out == -5.0).all()          # nothing written
    rc, n, ok, oc, out = call(0)
    assert rc == -1 and n == G
    rc, n, ok, oc, out = call(G)                          # sized by the G of the refused call
    assert rc == 0 and n == G
    assert ok.tobytes() == base[0].tobytes() and oc.tobytes() == base[1].tobytes() and out.tobytes() == base[2].tobytes()
    rc, n, ok, oc, out = call(G + 7)                      # variable v at out + v * capacity
    assert rc == 0 and out[:, :G].tobytes() == base[2].tobytes() and (out[:, G:] == -5.0).all() and (ok[G:] == -5).all()
    # refusals of the checks leave the handle usable as well
    n = C.c_int64(-1)
    assert lib.gpsat_glue_keyed_batch(h, R, 3, 3, ptr(key), ptr(pred), ptr(xprt), ptr(vals), 1.0, None, 0.0, R, C.byref(n), ptr(ok), ptr(oc), ptr(out)) == -1
    assert "ndim" in lib.gpsat_last_error().decode()
    for u, v in zip(eng.glue_keyed_batch(key, pred, xprt, vals, sigma), base):
        assert u.tobytes() == v.tobytes()
    assert all(t >= 0.0 for t in eng.glue_keyed_timing())


@pytest.mark.parametrize("refit", [False, True])
def test_orchestrator_glues_and_scores_end_to_end(eng, refit):
    from gpsat_amd import postprocessing as post
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    rng = np.random.default_rng(11)
    n, osc = 200, 2.0
    df = pd.DataFrame({"x": rng.uniform(0, 10, n), "y": rng.uniform(0, 10, n), "track": rng.integers(0, 6, n)})
    df["elev"] = 20.0 + 2.0 * np.sin(df["x"]) * np.cos(0.5 * df["y"]) + 0.2 * rng.standard_normal(n)
    xl = pd.DataFrame([(x, y) for x in (2.5, 5.0, 7.5) for y in (2.5, 5.0, 7.5)], columns=["x", "y"])
    data = {"data_source": df, "obs_col": "elev", "coords_col": ["x", "y"], "local_select": [{"col": ["x", "y"], "comp": "<", "val": 4.0}]}
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "obs_mean": "local", "coords_scale": [2.0, 2.0], "obs_scale": osc},
             "constraints": {"lengthscales": {"low": [0.1, 0.1], "high": [20, 20]}}, "optim_kwargs": {"max_iter": 20}}
    cv = {"by": ["track"], "refit": True} if refit else {"by": ["track"]}
    opt = {"inference_radius": 4.0, "R": 3, "max_dist": 3.5}
    out = BatchedLocalExpertOI({"source": xl}, data, model, {"method": "expert_loc"}, engine=eng, dtype="f64", cv=cv,
                               cv_glue=opt).run(None, min_obs=20)
    cvp, glued, scores = out["cv_preds"], out["cv_glued"], out["cv_scores"]
    assert len(out["run_details"]) == 9 and np.isfinite(cvp["f*"].values).mean() > 0.9
    assert list(glued.columns) == ["obs_index", "track", "pred_loc_x", "pred_loc_y", "elev", "f*", "f*_var", "y_var", "n_experts", "z"]
    # the public function on the run's own cv_preds: the same table exactly (the frame's labels are its positions)
    again = post.glue_cv_predictions(out, None, 4.0, R=3, max_dist=3.5, obs_scale=osc, engine=eng)
    pd.testing.assert_frame_equal(again, glued, check_exact=True)
    for c in ("f*", "f*_var", "y_var", "z"):
        assert again[c].values.tobytes() == glued[c].values.tobytes()
    # the restatement on the rows in raw units
    key = np.where(np.isnan(cvp["f*"].values), -1, cvp["obs_index"].values)
    vals = np.stack([cvp["f_bar"].values + osc * cvp["f*"].values, osc ** 2 * cvp["f*_var"].values, osc ** 2 * cvp["y_var"].values])
    p = np.stack([cvp["pred_loc_x"].values, cvp["pred_loc_y"].values])
    x = np.stack([cvp.index.get_level_values("x").values, cvp.index.get_level_values("y").values])
    d2 = ((p - x) ** 2).sum(axis=0)
    assert (np.abs(d2 - 3.5 ** 2) > 1e-9 * 3.5 ** 2).all()
    keys, counts, want = gk.glue_keyed(key, p, x, vals, 4.0 / 3, 3.5)
    np.testing.assert_array_equal(glued["obs_index"].values, keys)
    np.testing.assert_array_equal(glued["n_experts"].values, counts)
    np.testing.assert_array_equal(glued["elev"].values, df["elev"].values[keys])
    np.testing.assert_array_equal(glued["track"].values, df["track"].values[keys])
    for i, c in enumerate(("f*", "f*_var", "y_var")):
        np.testing.assert_allclose(glued[c].values, want[i], rtol=RTOL, atol=ATOL)
    assert counts.max() >= 3 and len(keys) > 150
    # the scores: numpy on cv_glued
    ok = (glued["n_experts"].values > 0) & np.isfinite(glued[["elev", "f*", "y_var"]].values).all(axis=1)
    assert len(scores) == 1 + df["track"].nunique() and list(scores.columns) == ["track", "n", "n_missing", "bias", "rmse", "nll", "mean_z2"]
    for i, sel in enumerate([np.ones(len(glued), dtype=bool)] + [glued["track"].values == t for t in sorted(df["track"].unique())]):
        s, row = glued[sel & ok], scores.iloc[i]
        y, mu, sig = s["elev"].values, s["f*"].values, np.sqrt(s["y_var"].values)
        assert row["n"] == len(s) and row["n_missing"] == int(sel.sum()) - len(s)
        np.testing.assert_allclose([row["bias"], row["rmse"], row["nll"], row["mean_z2"]],
                                   [np.mean(mu - y), np.sqrt(np.mean((y - mu) ** 2)),
                                    np.mean(np.log(sig * np.sqrt(2 * np.pi)) + (y - mu) ** 2 / (2 * sig ** 2)), np.mean(((y - mu) / sig) ** 2)],
                                   rtol=1e-13)
    # glued held-out predictions of the raw observations are useful ones: errors well below the field's spread
    assert scores["rmse"].iloc[0] < 0.75 * df["elev"].std()
