"""CPU: the slope of the glued map -- the restatement of gpsat_glue_keyed_grad_batch (tests/glue_grad_numpy.py) against the
keyed glue's restatement and against central differences of the glue itself, the plain average of the gradients pinned as
the wrong answer, the new symbol, every refusal of its exported host check, and postprocessing.glue_local_gradient with a
device-free engine that answers from the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import glue_grad_numpy as gg
import glue_keyed_numpy as gk
from gpsat_amd import _lib as L
from gpsat_amd import postprocessing as post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 1.0e5                        # metres: inference_radius 300 km / R 3
CASES = [(ndim, rows, nan, off) for ndim in (1, 2) for rows in (False, True) for nan in (False, True) for off in (0.0, 3.0e6)]


def fields(ndim, sigma_rows, nan_row, offset, seed, G=6):
    """G prediction locations, each predicted by 2..6 experts 0.5..2 sigma away; every expert carries a quadratic field of
    its own, f_i(p) = a_i + b_i.(p - c_i) + (p - c_i)' Q_i (p - c_i) / 2, of size 1 with a slope of size 1 / sigma: experts
    that disagree by as much as they vary, which is what makes the weights' term as large as the glued slope."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, G)
    key = rng.permutation(np.repeat(np.arange(G), sizes))
    n = len(key)
    p = offset + rng.uniform(-5, 5, (ndim, G)) * SIGMA
    pred = p[:, key]
    xprt = pred + rng.uniform(0.5, 2.0, (ndim, n)) * rng.choice([-1.0, 1.0], (ndim, n)) * SIGMA
    sg = rng.uniform(0.7, 1.4, n) * SIGMA if sigma_rows else SIGMA
    a = rng.normal(0, 1, n)
    b = rng.normal(0, 1, (ndim, n)) / SIGMA
    Q = rng.normal(0, 1, (ndim, ndim, n)) / SIGMA ** 2
    Q = (Q + Q.transpose(1, 0, 2)) / 2
    dead = np.zeros(n, dtype=bool)
    if nan_row:
        dead[np.nonzero(key == 1)[0][0]] = True            # one row of a group of several

    def at(q):
        """value [n] and gradient [ndim, n] of every row's field at prediction locations q [ndim, n]"""
        d = q - xprt
        f = a + (b * d).sum(0) + 0.5 * np.einsum("in,ijn,jn->n", d, Q, d)
        g = b + np.einsum("ijn,jn->in", Q, d)
        f[dead] = np.nan
        g[:, dead] = np.nan
        return f, g

    return key, pred, xprt, sg, at


@pytest.mark.parametrize("ndim,sigma_rows,nan_row,offset", CASES)
def test_restated_value_is_the_keyed_glue(ndim, sigma_rows, nan_row, offset):
    key, pred, xprt, sg, at = fields(ndim, sigma_rows, nan_row, offset, seed=1)
    f, g = at(pred)
    key = key.copy()
    key[3] = -4                                             # an ignored row
    for md in (None, 1.5 * SIGMA):
        want = gk.glue_keyed(key, pred, xprt, f[None], sg, md)
        for fn in (gg.glue_grad, gg.glue_grad_fast, gg.glue_grad_mp):
            got = fn(key, pred, xprt, f, g, sg, md)
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
            np.testing.assert_allclose(got[2], want[2][0], rtol=1e-13, atol=0, equal_nan=True)
        assert md is None or 0 < want[1].sum() < (key >= 0).sum()
    # the three restatements of the slope agree far inside what the device is held to
    a, b, c = (fn(key, pred, xprt, f, g, sg)[3] for fn in (gg.glue_grad, gg.glue_grad_fast, gg.glue_grad_mp))
    kappa = gg.glue_grad_mp(key, pred, xprt, f, g, sg)[4]
    assert np.abs(a - c).max() < 1e-13 * kappa.max() and np.abs(b - c).max() < 1e-13 * kappa.max()
    np.testing.assert_allclose(gg.glue_grad_fast(key, pred, xprt, f, g, sg)[4], kappa, rtol=1e-12)


@pytest.mark.parametrize("ndim,sigma_rows,nan_row,offset", CASES)
def test_slope_against_central_differences_of_the_glue(ndim, sigma_rows, nan_row, offset):
    """G_a is the derivative of the glue formula: the glue of the fields evaluated at p + h e_a minus that at p - h e_a,
    over 2h.  h = 10 m; the step's own error is ~ h^2 F''' ~ 1e-8 relative.  The bound: 1e-6 of max|g| + max|f| / sigma_min.
    The plain weighted average of the gradients -- what gluing the gradient columns returns -- misses by more than 1e-3."""
    key, pred, xprt, sg, at = fields(ndim, sigma_rows, nan_row, offset, seed=2 + ndim)
    f, g = at(pred)
    keys, counts, F, G = gg.glue_grad(key, pred, xprt, f, g, sg)
    scale = np.nanmax(np.abs(g)) + np.nanmax(np.abs(f)) / np.min(sg)
    plain = gk.glue_keyed(key, pred, xprt, g, sg)[2]
    h = 10.0
    for a in range(ndim):
        step = np.zeros((ndim, 1))
        step[a] = h
        up = gk.glue_keyed(key, pred + step, xprt, at(pred + step)[0][None], sg)[2][0]
        dn = gk.glue_keyed(key, pred - step, xprt, at(pred - step)[0][None], sg)[2][0]
        cd = (up - dn) / (2 * h)
        err = np.abs(G[a] - cd).max() / scale
        miss = np.abs(plain[a] - cd).max() / scale
        print(f"ndim {ndim} axis {a} sigma_rows {sigma_rows} nan {nan_row} offset {offset:g}: exact {err:.2e}, plain average {miss:.2e}")
        assert err < 1e-6
        assert miss > 1e-3


def test_rules_count_zero_negative_keys_and_nan_gradient():
    key = np.array([4, 4, -1, 9, 4, 7])
    pred = np.zeros((1, 6))
    xprt = np.array([[1.0, -2.0, 0.0, 5.0, 0.5, 1.0]])
    f = np.array([1.0, 2.0, 100.0, 3.0, np.nan, 4.0])
    g = np.array([[0.1, np.nan, 100.0, 0.3, 0.2, 0.4]])
    sg = 2.0
    w = np.exp(-xprt[0] ** 2 / 8) / (2.0 * np.sqrt(2 * np.pi))
    u = xprt[0] / 4
    for fn in (gg.glue_grad, gg.glue_grad_fast, gg.glue_grad_mp):
        keys, counts, F, G = fn(key, pred, xprt, f, g, sg, 3.0)[:4]
        assert keys.tolist() == [4, 7, 9] and counts.tolist() == [3, 1, 0]
        W = w[0] + w[1] + w[4]                              # the NaN value's weight stays in the denominator
        Fw = (w[0] * f[0] + w[1] * f[1]) / W
        np.testing.assert_allclose(F[:2], [Fw, 4.0], rtol=1e-14)
        # row 1 has a value and no gradient: out of S alone; row 4 has no value: out of N and S, in W and U
        S = w[0] * (g[0, 0] + u[0] * f[0])
        U = w[0] * u[0] + w[1] * u[1] + w[4] * u[4]
        np.testing.assert_allclose(G[0, :2], [(S - Fw * U) / W, 0.4], rtol=1e-13)      # one row: G = g, whatever u is
        assert np.isnan(F[2]) and np.isnan(G[0, 2])


# ------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpsat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpsat_[a-z_]+)\s*\(", src))
    assert "gpsat_glue_keyed_grad_batch" in declared and declared == set(L.EXPORTS)
    assert "gpsat_glue_keyed_grad_batch" in L.OPTIONAL_EXPORTS
    lib = L.load()
    assert hasattr(lib, "gpsat_glue_keyed_grad_batch")
    assert lib.gpsat_version() == 4 == L.ABI_VERSION
    flat = re.sub(r"\s+", " ", src)
    assert ("int gpsat_glue_keyed_grad_batch(gpsat_handle *h, int64_t R, int32_t ndim, const int64_t *key, const double *pred, "
            "const double *xprt, const double *val, const double *grad, double sigma, const double *sigma_rows, double max_dist, "
            "int64_t capacity, int64_t *G, int64_t *out_key, int32_t *out_count, double *out_val, double *out_grad);") in flat
    assert len(L.SIGNATURES["gpsat_glue_keyed_grad_batch"][1]) == 17


def test_host_checks_of_the_keyed_gradient_glue():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat21check_glue_keyed_gradEliPKlPKdS3_S3_S3_dS3_dlS1_S1_PKiS3_S3_Pcm")
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                   C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    R = 6
    buf = {k: np.zeros(2 * R) for k in ("pred", "xprt", "val", "grad", "sig", "oval", "ograd")}
    buf.update(key=np.zeros(R, dtype=np.int64), G=np.zeros(1, dtype=np.int64), okey=np.zeros(R, dtype=np.int64),
               ocnt=np.zeros(R, dtype=np.int32))
    p = {k: v.ctypes.data for k, v in buf.items()}

    def check(**kw):
        a = dict(R=R, ndim=2, key=p["key"], pred=p["pred"], xprt=p["xprt"], val=p["val"], grad=p["grad"], sigma=1.5, sig=None,
                 max_dist=np.inf, cap=R, G=p["G"], okey=p["okey"], ocnt=p["ocnt"], oval=p["oval"], ograd=p["ograd"])
        a.update(kw)
        why = C.create_string_buffer(200)
        rc = fn(a["R"], a["ndim"], a["key"], a["pred"], a["xprt"], a["val"], a["grad"], a["sigma"], a["sig"], a["max_dist"],
                a["cap"], a["G"], a["okey"], a["ocnt"], a["oval"], a["ograd"], why, 200)
        return rc, why.value.decode()

    good = [{}, dict(ndim=1), dict(sigma=0.0, sig=p["sig"]), dict(sigma=np.nan, sig=p["sig"]), dict(max_dist=5.0),
            dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=-np.inf), dict(R=2 ** 31 - 1),
            dict(R=0, key=None, pred=None, xprt=None, val=None, grad=None), dict(cap=0, okey=None, ocnt=None, oval=None, ograd=None)]
    for kw in good:
        assert check(**kw) == (0, ""), kw
    bad = [(dict(G=None), "G is NULL"), (dict(key=None), "NULL"), (dict(pred=None), "NULL"), (dict(xprt=None), "NULL"),
           (dict(val=None), "NULL"), (dict(grad=None), "NULL"), (dict(okey=None), "NULL"), (dict(ocnt=None), "NULL"),
           (dict(oval=None), "NULL"), (dict(ograd=None), "NULL"), (dict(ndim=0), "ndim"), (dict(ndim=3), "ndim"),
           (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=np.inf), "sigma"), (dict(sigma=np.nan), "sigma"),
           (dict(max_dist=np.nan), "max_dist"), (dict(R=2 ** 31), "2^31-1"), (dict(R=-1), "negative"), (dict(cap=-1), "negative")]
    for kw, match in bad:
        rc, why = check(**kw)
        assert rc == -1 and match in why and why.startswith("gpsat_glue_keyed_grad_batch: "), (kw, rc, why)
    # the entry point itself, before any device is touched: a NULL handle
    assert lib.gpsat_glue_keyed_grad_batch(None, 0, 2, None, None, None, None, None, 1.0, None, 0.0, 0, C.byref(C.c_int64(0)),
                                           None, None, None, None) == -1
    assert "gpsat_glue_keyed_grad_batch: handle is NULL" in lib.gpsat_last_error().decode()


def test_engine_without_the_symbol_raises():
    from gpsat_amd.engine import Engine, GpsatError

    class Old:
        pass

    eng = Engine.__new__(Engine)
    eng._lib = Old()
    with pytest.raises(GpsatError, match="gpsat_glue_keyed_grad_batch.*no host fallback"):
        eng.glue_keyed_grad_batch(np.zeros(1, dtype=np.int64), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(1), np.zeros((1, 1)), 1.0)
    eng._lib = None


# ------------------------------------------------------------------------------------------------------------------
# glue_local_gradient
# ------------------------------------------------------------------------------------------------------------------
def _preds(seed=0, nx=5, ny=4):
    """A prediction grid predicted by the experts within 2.6 of it and its nearest two, rows in expert order (locations interleaved), with a
    per-expert f_bar, in the column layout of a run with pred_grad."""
    rng = np.random.default_rng(seed)
    px, py = (a.reshape(-1) for a in np.meshgrid(np.linspace(0, 8, nx)[::-1], np.linspace(0, 6, ny), indexing="ij"))
    ex, ey = rng.uniform(0, 8, 7), rng.uniform(0, 6, 7)
    dist = np.hypot(ex[:, None] - px[None], ey[:, None] - py[None])
    e, j = np.nonzero((dist < 2.6) | (dist <= np.sort(dist, axis=0)[1]))      # and the nearest two, wherever they are
    n = len(e)
    return pd.DataFrame({"x": ex[e], "y": ey[e], "pred_loc_x": px[j], "pred_loc_y": py[j], "pred_loc_t": 3.0,
                         "f*": rng.normal(0, 1, n), "f*_var": rng.uniform(0.1, 0.2, n), "f_bar": 20.0 + rng.normal(0, 1, 7)[e],
                         "f*_grad_x": rng.normal(0, 1, n), "f*_grad_y": rng.normal(0, 1, n), "f*_grad_t": rng.normal(0, 1, n),
                         "f*_grad_var_x": rng.uniform(0.1, 0.2, n), "f*_grad_var_y": rng.uniform(0.1, 0.2, n)})


def test_glue_local_gradient_units_order_and_columns():
    df = _preds()
    osc, rad = 2.5, 6.0
    eng = gg.GlueGradNumpyEngine()
    pl, xl = ["pred_loc_x", "pred_loc_y"], ["x", "y"]
    extra = ["f*_var", "f*_grad_var_x", "f*_grad_var_y", "f*_grad_t", "f_bar"]          # five: two plain calls
    got = post.glue_local_gradient(df, pl, xl, rad, R=3, obs_scale=osc, also_glue=extra, engine=eng)
    assert list(got.columns) == pl + ["f*", "f*_grad_x", "f*_grad_y", "n_experts"] + extra      # the default grad_cols
    assert [c.get("grad", False) for c in eng.calls] == [True, False, False] and all(c["sigma"] == 2.0 for c in eng.calls)
    # the rows and their order: those of glue_local_predictions_2d (sorted unique locations), the frame not sorted
    ref = post.glue_local_predictions_2d(df, pl, xl, ["f*_var"], rad, R=3, engine=_SegEngine())
    np.testing.assert_array_equal(got[pl].values, ref[pl].values)
    np.testing.assert_allclose(got["f*_var"].values, ref["f*_var"].values, rtol=1e-13)
    key = eng.calls[0]["key"]
    assert key.min() == 0 and key.max() == len(got) - 1 and not (np.diff(key) >= 0).all()
    np.testing.assert_array_equal(got[pl].values[key], df[pl].values)                   # the key is the rank of the location
    np.testing.assert_array_equal(got["n_experts"].values, np.bincount(key))
    assert got["n_experts"].dtype == np.int64 and got["n_experts"].max() > 1
    # raw units, by the per-group loop on the converted rows
    pred, xprt = df[pl].values.T, df[xl].values.T
    val = df["f_bar"].values + osc * df["f*"].values
    grad = osc * df[["f*_grad_x", "f*_grad_y"]].values.T
    _, _, F, G = gg.glue_grad(key, pred, xprt, val, grad, rad / 3)
    np.testing.assert_allclose(got["f*"].values, F, rtol=1e-13)
    np.testing.assert_allclose(got[["f*_grad_x", "f*_grad_y"]].values.T, G, rtol=1e-10, atol=1e-13)
    assert np.abs(F - 20.0).max() < 10                      # the mean is inside
    # the per-expert mean tilts the glued map: without it in the value the slope is another one
    no_mean = post.glue_local_gradient(df, pl, xl, rad, obs_scale=osc, mean_col=None, engine=eng)
    np.testing.assert_allclose(no_mean["f*"].values, gg.glue_grad(key, pred, xprt, osc * df["f*"].values, grad, rad / 3)[2], rtol=1e-13)
    assert np.abs(no_mean["f*_grad_x"].values - got["f*_grad_x"].values).max() > 1e-3
    # also_glue columns are unscaled plain averages
    plain = gk.glue_keyed(key, pred, xprt, df[extra].values.T, rad / 3)[2]
    np.testing.assert_allclose(got[extra].values.T, plain, rtol=1e-13)
    # one glue axis, named gradient column, a string for the column lists
    one = post.glue_local_gradient(df, "pred_loc_x", "x", rad, grad_cols="f*_grad_x", mean_col=None, engine=eng)
    assert list(one.columns) == ["pred_loc_x", "f*", "f*_grad_x", "n_experts"] and len(one) == df["pred_loc_x"].nunique()
    assert (np.diff(one["pred_loc_x"].values) > 0).all()
    k1 = eng.calls[-1]["key"]
    _, _, F1, G1 = gg.glue_grad(k1, df[["pred_loc_x"]].values.T, df[["x"]].values.T, df["f*"].values, df[["f*_grad_x"]].values.T, rad / 3)
    np.testing.assert_allclose(one["f*_grad_x"].values, G1[0], rtol=1e-10, atol=1e-13)
    # columns that are not called pred_loc_<c> keep their whole name in the default
    ren = df.rename(columns={"pred_loc_x": "px", "f*_grad_x": "f*_grad_px"})
    assert list(post.glue_local_gradient(ren, ["px"], ["x"], rad, engine=eng).columns) == ["px", "f*", "f*_grad_px", "n_experts"]


def test_glue_local_gradient_max_dist_leaves_nan_rows():
    df = _preds(seed=3)
    eng = gg.GlueGradNumpyEngine()
    pl, xl = ["pred_loc_x", "pred_loc_y"], ["x", "y"]
    got = post.glue_local_gradient(df, pl, xl, 6.0, max_dist=1.0, also_glue=["f*_var"], engine=eng)
    full = post.glue_local_gradient(df, pl, xl, 6.0, engine=eng)
    assert eng.calls[0]["max_dist"] == 1.0 and eng.calls[1]["max_dist"] == 1.0
    np.testing.assert_array_equal(got[pl].values, full[pl].values)        # a location that lost every expert keeps its row
    near = np.hypot(df["x"] - df["pred_loc_x"], df["y"] - df["pred_loc_y"]).values < 1.0
    np.testing.assert_array_equal(got["n_experts"].values, np.bincount(eng.calls[0]["key"], weights=near).astype(int))
    none = got["n_experts"].values == 0
    assert none.any() and not none.all()
    for c in ("f*", "f*_grad_x", "f*_grad_y", "f*_var"):
        assert np.isnan(got[c].values[none]).all() and np.isfinite(got[c].values[~none]).all()
    # a row without a location belongs to no group, on either axis and with one axis alone
    for c, cols in (("pred_loc_x", pl), ("pred_loc_y", pl), ("pred_loc_x", pl[:1])):
        lost = df.copy()
        lost.loc[[0, 5], c] = np.nan
        part = post.glue_local_gradient(lost, cols, xl[:len(cols)], 6.0, grad_cols=["f*_grad_x", "f*_grad_y"][:len(cols)], engine=eng)
        key = eng.calls[-1]["key"]
        assert (key[[0, 5]] == -1).all() and (np.delete(key, [0, 5]) >= 0).all() and key.max() == len(part) - 1
        assert np.isfinite(part[cols].values).all()
        np.testing.assert_array_equal(part[cols].values[np.delete(key, [0, 5])], np.delete(lost[cols].values, [0, 5], axis=0))


def test_glue_local_gradient_refusals():
    df = _preds()
    eng = gg.GlueGradNumpyEngine()
    pl, xl = ["pred_loc_x", "pred_loc_y"], ["x", "y"]
    with pytest.raises(TypeError, match="one number"):
        post.glue_local_gradient(df, pl, xl, {1.0: 3.0}, engine=eng)
    with pytest.raises(ValueError, match="1 or 2 glue axes"):
        post.glue_local_gradient(df, [], [], 6.0, engine=eng)
    with pytest.raises(ValueError, match="1 or 2 glue axes"):
        post.glue_local_gradient(df, pl + ["pred_loc_t"], xl + ["x"], 6.0, engine=eng)
    with pytest.raises(ValueError, match="same number of glue axes"):
        post.glue_local_gradient(df, pl, ["x"], 6.0, engine=eng)
    with pytest.raises(ValueError, match="one gradient column per glue axis"):
        post.glue_local_gradient(df, pl, xl, 6.0, grad_cols=["f*_grad_x"], engine=eng)
    for kw, name in ((dict(value_col="g*"), "g\\*"), (dict(mean_col="mu"), "mu"), (dict(also_glue=["nope"]), "nope"),
                     (dict(grad_cols=["f*_grad_x", "f*_grad_z"]), "f\\*_grad_z")):
        with pytest.raises(ValueError, match=f"no column.*{name}"):
            post.glue_local_gradient(df, pl, xl, 6.0, engine=eng, **dict(dict(grad_cols=["f*_grad_x", "f*_grad_y"]), **kw))
    with pytest.raises(ValueError, match="no column.*f\\*_grad_x"):        # a run without pred_grad
        post.glue_local_gradient(df.drop(columns=["f*_grad_x"]), pl, xl, 6.0, engine=eng)
    with pytest.raises(ValueError, match="no column.*ex"):
        post.glue_local_gradient(df, pl, ["ex", "y"], 6.0, engine=eng)
    assert not eng.calls


class _SegEngine:
    """glue_batch (rows in segments) from the keyed restatement: the engine glue_local_predictions_2d asks."""

    def glue_batch(self, seg, pred, xprt, vals, sigma):
        key = np.repeat(np.arange(len(seg) - 1), np.diff(seg))
        return gk.glue_keyed(key, pred, xprt, vals, sigma)[2]
