"""CPU: the second derivatives of the glued map -- the restatement of gpsat_glue_keyed_hess_batch (tests/glue_hess_numpy.py)
against central differences of the restated slope, rows that all carry one field, the plain average of the second
derivatives pinned as the wrong answer, the new symbol, every refusal of its exported host check, and
postprocessing.glue_local_hessian with a device-free engine that answers from the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import glue_grad_numpy as gg
import glue_hess_numpy as gh
import glue_keyed_numpy as gk
from gpsat_amd import _lib as L
from gpsat_amd import postprocessing as post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SIGMA = 1.0e5                        # metres: inference_radius 300 km / R 3
CASES = [(ndim, rows, nan, off) for ndim in (1, 2) for rows in (False, True) for nan in (False, True) for off in (0.0, 3.0e6)]


def fields(ndim, sigma_rows, nan_row, offset, seed, G=6, same=False):
    """G prediction locations, each predicted by 2..6 experts 0.5..3 sigma away per axis (within 4.5 sigma of them); every
    expert carries a quadratic field of its own, f_i(p) = a_i + b_i.(p - c_i) + (p - c_i)' Q_i (p - c_i) / 2, of size 1 with
    a slope of size 1 / sigma and a curvature of size 1 / sigma^2: experts that disagree by as much as they vary.  same:
    every row of a group carries one field, centred on the group's first expert."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, G)
    key = rng.permutation(np.repeat(np.arange(G), sizes))
    n = len(key)
    p = offset + rng.uniform(-5, 5, (ndim, G)) * SIGMA
    pred = p[:, key]
    sg = rng.uniform(0.7, 1.4, n) * SIGMA if sigma_rows else SIGMA
    xprt = pred + rng.uniform(0.5, 3.0, (ndim, n)) * rng.choice([-1.0, 1.0], (ndim, n)) * np.minimum(sg, SIGMA)
    a = rng.normal(0, 1, n)
    b = rng.normal(0, 1, (ndim, n)) / SIGMA
    Q = rng.normal(0, 1, (ndim, ndim, n)) / SIGMA ** 2
    Q = (Q + Q.transpose(1, 0, 2)) / 2
    centre = xprt
    if same:
        first = np.array([np.nonzero(key == k)[0][0] for k in range(G)])[key]
        a, b, Q, centre = a[first], b[:, first], Q[:, :, first], xprt[:, first]
    dead = np.zeros(n, dtype=bool)
    if nan_row:
        dead[np.nonzero(key == 1)[0][0]] = True            # one row of a group of several
    pr = gh.pairs(ndim)

    def at(q):
        """value [n], gradient [ndim, n] and second derivatives [npair, n] of every row's field at locations q [ndim, n]"""
        d = q - centre
        f = a + (b * d).sum(0) + 0.5 * np.einsum("in,ijn,jn->n", d, Q, d)
        g = b + np.einsum("ijn,jn->in", Q, d)
        h = np.stack([Q[i, j] for i, j in pr])
        f[dead] = np.nan
        g[:, dead] = np.nan
        h[:, dead] = np.nan
        return f, g, h

    return key, pred, xprt, sg, at


def differenced(key, pred, xprt, sg, at, h=10.0):
    """Central differences of the 50-digit slope: D[a][b] = (G_a(p + h e_b) - G_a(p - h e_b)) / (the step as it was taken)."""
    ndim = pred.shape[0]
    D = [[None] * ndim for _ in range(ndim)]
    for b in range(ndim):
        step = np.zeros((ndim, 1))
        step[b] = h
        up, dn = pred + step, pred - step
        f, g, _ = at(up)
        Gu = gg.glue_grad_mp(key, up, xprt, f, g, sg)
        f, g, _ = at(dn)
        Gd = gg.glue_grad_mp(key, dn, xprt, f, g, sg)
        taken = np.array([(up[b] - dn[b])[key == k][0] for k in Gu[0]])
        for a in range(ndim):
            D[a][b] = (Gu[3][a] - Gd[3][a]) / taken
    return D


@pytest.mark.parametrize("ndim,sigma_rows,nan_row,offset", CASES)
def test_hessian_against_central_differences_of_the_slope(ndim, sigma_rows, nan_row, offset):
    """H_ab is the derivative of G_a along b (and of G_b along a): central differences of the 50-digit restatement of the
    slope with h = 10 m at sigma ~ 1e5.  The step's truncation is (h / sigma)^2 = 1e-8 times a polynomial in z; the bound is
    1e-7 kappa_ab.  The vectorised fp64 restatement agrees with the 50-digit one far inside that."""
    key, pred, xprt, sg, at = fields(ndim, sigma_rows, nan_row, offset, seed=10 + ndim)
    key = key.copy()
    key[3] = -4                                             # an ignored row
    f, g, h = at(pred)
    keys, counts, F, G, H, kappa = gh.glue_hess_mp(key, pred, xprt, f, g, h, sg)
    want = gg.glue_grad_mp(key, pred, xprt, f, g, sg)
    np.testing.assert_array_equal(keys, want[0])
    np.testing.assert_array_equal(counts, want[1])
    np.testing.assert_array_equal(F, want[2])
    np.testing.assert_array_equal(G, want[3])
    D = differenced(key, pred, xprt, sg, at)
    worst = 0.0
    for p, (a, b) in enumerate(gh.pairs(ndim)):
        for d in {(a, b), (b, a)}:
            worst = max(worst, float((np.abs(H[p] - D[d[0]][d[1]]) / kappa[p]).max()))
    print(f"ndim {ndim} sigma_rows {sigma_rows} nan {nan_row} offset {offset:g}: |H - differences| / kappa <= {worst:.2e}")
    assert worst < 1e-7
    fast = gh.glue_hess_fast(key, pred, xprt, f, g, h, sg)
    np.testing.assert_array_equal(fast[0], keys)
    np.testing.assert_array_equal(fast[1], counts)
    assert (np.abs(fast[4] - H) <= 1e-12 * kappa).all()
    np.testing.assert_allclose(fast[5], kappa, rtol=1e-12)


@pytest.mark.parametrize("ndim,sigma_rows,nan_row,offset", CASES)
def test_rows_that_carry_one_field_return_it(ndim, sigma_rows, nan_row, offset):
    """Independent of the formula's derivation: rows with identical f, g and h give F = f, G = g and H = h whatever the
    experts' positions -- every term from the weights cancels.  The 50-digit values, rounded to fp64, at 2 eps kappa."""
    key, pred, xprt, sg, at = fields(ndim, sigma_rows, nan_row, offset, seed=20 + ndim, same=True)
    f, g, h = at(pred)
    if nan_row:                                             # a row without a Hessian entry alone would tilt T: leave the dead row out
        key = np.where(np.isnan(f), -1, key)
    keys, counts, F, G, H, kappa = gh.glue_hess_mp(key, pred, xprt, f, g, h, sg)
    first = np.array([np.nonzero(key == k)[0][0] for k in keys])
    for k in keys:                                          # the premise: one field per group
        r = np.nonzero(key == k)[0]
        assert np.ptp(f[r]) <= 1e-12 * np.abs(f[r]).max() and (np.ptp(h[:, r], axis=1) == 0).all()
    kg = gg.glue_grad_mp(key, pred, xprt, f, g, sg)[4]
    # f and g of a group's rows agree to the rounding of their evaluation only: that, carried through, is inside these
    assert (np.abs(F - f[first]) <= 1e-12 * np.abs(f[first])).all()
    assert (np.abs(G - g[:, first]) <= 1e-11 * kg).all()
    assert (np.abs(H - h[:, first]) <= 1e-10 * kappa).all()
    # with exactly identical rows the statement is exact
    fx, gx, hx = f[first][np.searchsorted(keys, np.maximum(key, 0))], g[:, first][:, np.searchsorted(keys, np.maximum(key, 0))], h
    keys, counts, F, G, H, kappa = gh.glue_hess_mp(key, pred, xprt, fx, gx, hx, sg)
    assert (np.abs(F - f[first]) <= 2 * EPS * np.abs(f[first])).all()
    assert (np.abs(G - g[:, first]) <= 2 * EPS * kg).all()
    assert (np.abs(H - h[:, first]) <= 2 * EPS * kappa).all()


@pytest.mark.parametrize("ndim", [1, 2])
def test_the_plain_average_of_the_second_derivatives_is_wrong(ndim):
    """Experts that disagree by as much as they vary: the plain weighted average of h_ab -- what gluing the f*_hess columns
    returns -- misses the differenced glue by a share of max|h| + max|g| / sigma + max|f| / sigma^2 that is printed (DESIGN.md
    section 29 records it), more than 100 times what the formula misses it by."""
    key, pred, xprt, sg, at = fields(ndim, False, False, 3.0e6, seed=30 + ndim)
    f, g, h = at(pred)
    H = gh.glue_hess_mp(key, pred, xprt, f, g, h, sg)[4]
    plain = gk.glue_keyed(key, pred, xprt, h, sg)[2]
    D = differenced(key, pred, xprt, sg, at)
    scale = np.abs(h).max() + np.abs(g).max() / SIGMA + np.abs(f).max() / SIGMA ** 2
    for p, (a, b) in enumerate(gh.pairs(ndim)):
        err = np.abs(H[p] - D[a][b]).max() / scale
        miss = np.abs(plain[p] - D[a][b]).max() / scale
        print(f"ndim {ndim} pair ({a},{b}): the formula misses the differences by {err:.2e}, the plain average by {miss:.2e} of the scale")
        assert miss > 100 * err


def test_rules_count_zero_negative_keys_and_nan_entries():
    key = np.array([4, 4, -1, 9, 4, 7, 4])
    pred = np.zeros((1, 7))
    xprt = np.array([[1.0, -2.0, 0.0, 5.0, 0.5, 1.0, -0.5]])
    f = np.array([1.0, 2.0, 100.0, 3.0, np.nan, 4.0, 0.5])
    g = np.array([[0.1, np.nan, 100.0, 0.3, 0.2, 0.4, 0.7]])
    h = np.array([[0.01, 0.02, 100.0, 0.03, 0.04, 0.05, np.nan]])
    sg = 2.0
    w = np.exp(-xprt[0] ** 2 / 8) / (2.0 * np.sqrt(2 * np.pi))
    u = xprt[0] / 4
    c = u * u - 0.25
    for fn in (gh.glue_hess_fast, gh.glue_hess_mp):
        keys, counts, F, G, H = fn(key, pred, xprt, f, g, h, sg, 3.0)[:5]
        assert keys.tolist() == [4, 7, 9] and counts.tolist() == [4, 1, 0]
        r = [0, 1, 4, 6]
        W, U, V = w[r].sum(), (w[r] * u[r]).sum(), (w[r] * c[r]).sum()      # every row's weight stays in W, U and V
        Fw = (w[0] * f[0] + w[1] * f[1] + w[6] * f[6]) / W
        S = w[0] * (g[0, 0] + u[0] * f[0]) + w[6] * (g[0, 6] + u[6] * f[6])
        Gw = (S - Fw * U) / W
        T = w[0] * (h[0, 0] + 2 * u[0] * g[0, 0] + c[0] * f[0])          # row 1: no gradient; 4: no value; 6: no Hessian entry
        np.testing.assert_allclose(F[:2], [Fw, 4.0], rtol=1e-14)
        np.testing.assert_allclose(G[0, :2], [Gw, 0.4], rtol=1e-13)
        np.testing.assert_allclose(H[0, :2], [(T - 2 * Gw * U - Fw * V) / W, 0.05], rtol=1e-12)      # one row: H = h
        assert np.isnan(F[2]) and np.isnan(G[0, 2]) and np.isnan(H[0, 2])


# ------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    raw = open(os.path.join(ROOT, "include", "gpsat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gpsat_[a-z_]+)\s*\(", src))
    assert "gpsat_glue_keyed_hess_batch" in declared and declared == set(L.EXPORTS)
    assert "gpsat_glue_keyed_hess_batch" in L.OPTIONAL_EXPORTS
    lib = L.load()
    assert hasattr(lib, "gpsat_glue_keyed_hess_batch")
    assert lib.gpsat_version() == 4 == L.ABI_VERSION
    flat = re.sub(r"\s+", " ", src)
    assert ("int gpsat_glue_keyed_hess_batch(gpsat_handle *h, int64_t R, int32_t ndim, const int64_t *key, const double *pred, "
            "const double *xprt, const double *val, const double *grad, const double *hess, double sigma, const double *sigma_rows, "
            "double max_dist, int64_t capacity, int64_t *G, int64_t *out_key, int32_t *out_count, double *out_val, double *out_grad, "
            "double *out_hess);") in flat
    assert len(L.SIGNATURES["gpsat_glue_keyed_hess_batch"][1]) == 19
    # the comment in front of it states the quantity, the NaN rule, the pair order and the workspace
    doc = re.sub(r"\s*\n \*\s*", " ", raw[:raw.index("int gpsat_glue_keyed_hess_batch(")].rsplit("/*", 1)[1])
    for text in ("H_ab = (T_ab - G_a U_b - G_b U_a - F V_ab) / W", "V_ab = sum w_i (u_ia u_ib - delta_ab q_i)",
                 "(0,0), (0,1), (1,1)", "stays out of the numerators", "its weight stays in W, U and V",
                 "1 + ndim + npair value columns", "out_hess[k * capacity + j]", "A key with count 0 has NaN in F, every G_a and every H_ab"):
        assert text in doc, text


def test_host_checks_of_the_keyed_hessian_glue():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat21check_glue_keyed_hessEliPKlPKdS3_S3_S3_S3_dS3_dlS1_S1_PKiS3_S3_S3_Pcm")
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                   C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    R = 6
    buf = {k: np.zeros(3 * R) for k in ("pred", "xprt", "val", "grad", "hess", "sig", "oval", "ograd", "ohess")}
    buf.update(key=np.zeros(R, dtype=np.int64), G=np.zeros(1, dtype=np.int64), okey=np.zeros(R, dtype=np.int64),
               ocnt=np.zeros(R, dtype=np.int32))
    p = {k: v.ctypes.data for k, v in buf.items()}

    def check(**kw):
        a = dict(R=R, ndim=2, key=p["key"], pred=p["pred"], xprt=p["xprt"], val=p["val"], grad=p["grad"], hess=p["hess"], sigma=1.5,
                 sig=None, max_dist=np.inf, cap=R, G=p["G"], okey=p["okey"], ocnt=p["ocnt"], oval=p["oval"], ograd=p["ograd"],
                 ohess=p["ohess"])
        a.update(kw)
        why = C.create_string_buffer(200)
        rc = fn(a["R"], a["ndim"], a["key"], a["pred"], a["xprt"], a["val"], a["grad"], a["hess"], a["sigma"], a["sig"], a["max_dist"],
                a["cap"], a["G"], a["okey"], a["ocnt"], a["oval"], a["ograd"], a["ohess"], why, 200)
        return rc, why.value.decode()

    good = [{}, dict(ndim=1), dict(sigma=0.0, sig=p["sig"]), dict(sigma=np.nan, sig=p["sig"]), dict(max_dist=5.0),
            dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=-np.inf), dict(R=2 ** 31 - 1),
            dict(R=0, key=None, pred=None, xprt=None, val=None, grad=None, hess=None),
            dict(cap=0, okey=None, ocnt=None, oval=None, ograd=None, ohess=None)]
    for kw in good:
        assert check(**kw) == (0, ""), kw
    bad = [(dict(G=None), "G is NULL"), (dict(key=None), "NULL"), (dict(pred=None), "NULL"), (dict(xprt=None), "NULL"),
           (dict(val=None), "NULL"), (dict(grad=None), "NULL"), (dict(hess=None), "NULL"), (dict(okey=None), "NULL"),
           (dict(ocnt=None), "NULL"), (dict(oval=None), "NULL"), (dict(ograd=None), "NULL"), (dict(ohess=None), "NULL"),
           (dict(ndim=0), "ndim"), (dict(ndim=3), "ndim"),
           (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=np.inf), "sigma"), (dict(sigma=np.nan), "sigma"),
           (dict(max_dist=np.nan), "max_dist"), (dict(R=2 ** 31), "2^31-1"), (dict(R=-1), "negative"), (dict(cap=-1), "negative")]
    for kw, match in bad:
        rc, why = check(**kw)
        assert rc == -1 and match in why and why.startswith("gpsat_glue_keyed_hess_batch: "), (kw, rc, why)
    # the entry point itself, before any device is touched: a NULL handle
    assert lib.gpsat_glue_keyed_hess_batch(None, 0, 2, None, None, None, None, None, None, 1.0, None, 0.0, 0, C.byref(C.c_int64(0)),
                                           None, None, None, None, None) == -1
    assert "gpsat_glue_keyed_hess_batch: handle is NULL" in lib.gpsat_last_error().decode()


def test_engine_without_the_symbol_raises():
    from gpsat_amd.engine import Engine, GpsatError

    class Old:
        pass

    eng = Engine.__new__(Engine)
    eng._lib = Old()
    with pytest.raises(GpsatError, match="gpsat_glue_keyed_hess_batch.*no host fallback"):
        eng.glue_keyed_hess_batch(np.zeros(1, dtype=np.int64), np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(1), np.zeros((1, 1)),
                                  np.zeros((1, 1)), 1.0)
    eng._lib = None
    assert "glue_keyed_hess_batch" in Engine.glue_keyed_timing.__doc__


# ------------------------------------------------------------------------------------------------------------------
# glue_local_hessian
# ------------------------------------------------------------------------------------------------------------------
PL, XL = ["pred_loc_x", "pred_loc_y"], ["x", "y"]
GRADS = ["f*_grad_x", "f*_grad_y"]
HESS = ["f*_hess_x_x", "f*_hess_x_y", "f*_hess_y_y"]
TCOLS = ["f*_grad_t", "f*_hess_t_t", "f*_hess_x_t", "f*_hess_y_t"]


def _preds(seed=0, nx=5, ny=4):
    """A prediction grid predicted by the experts within 2.6 of it and its nearest two, rows in expert order (locations
    interleaved), with a per-expert f_bar, in the column layout of a run with pred_grad and pred_hess over x, y and t."""
    rng = np.random.default_rng(seed)
    px, py = (a.reshape(-1) for a in np.meshgrid(np.linspace(0, 8, nx)[::-1], np.linspace(0, 6, ny), indexing="ij"))
    ex, ey = rng.uniform(0, 8, 7), rng.uniform(0, 6, 7)
    dist = np.hypot(ex[:, None] - px[None], ey[:, None] - py[None])
    e, j = np.nonzero((dist < 2.6) | (dist <= np.sort(dist, axis=0)[1]))      # and the nearest two, wherever they are
    n = len(e)
    fr = {"x": ex[e], "y": ey[e], "pred_loc_x": px[j], "pred_loc_y": py[j], "pred_loc_t": 3.0,
          "f*": rng.normal(0, 1, n), "f*_var": rng.uniform(0.1, 0.2, n), "f_bar": 20.0 + rng.normal(0, 1, 7)[e]}
    fr.update({c: rng.normal(0, 1, n) for c in GRADS + HESS + TCOLS})
    fr.update({"f*_hess_var_x_x": rng.uniform(0.1, 0.2, n)})
    return pd.DataFrame(fr)


def test_glue_local_hessian_units_order_and_columns():
    df = _preds()
    osc, rad = 2.5, 6.0
    eng = gh.GlueHessNumpyEngine()
    extra = ["f*_var", "f*_hess_var_x_x", "f_bar", "x", "y"]                             # five: two plain calls
    got = post.glue_local_hessian(df, PL, XL, rad, R=3, obs_scale=osc, also_glue=extra, engine=eng)
    assert list(got.columns) == PL + ["f*"] + GRADS + HESS + ["f*_lap", "n_experts"] + extra      # the default grad_cols, hess_cols
    assert [("hess" in c, "grad" in c) for c in eng.calls] == [(True, False), (False, False), (False, False)]
    assert all(c["sigma"] == 2.0 for c in eng.calls)
    # the rows and their order: those of glue_local_gradient (and so of glue_local_predictions_2d), the frame not sorted
    ref = post.glue_local_gradient(df, PL, XL, rad, R=3, obs_scale=osc, also_glue=extra, engine=gg.GlueGradNumpyEngine())
    for c in PL + ["f*"] + GRADS + ["n_experts"] + extra:
        np.testing.assert_array_equal(got[c].values, ref[c].values)
    key = eng.calls[0]["key"]
    assert key.min() == 0 and key.max() == len(got) - 1 and not (np.diff(key) >= 0).all()
    np.testing.assert_array_equal(got[PL].values[key], df[PL].values)                   # the key is the rank of the location
    assert got["n_experts"].dtype == np.int64 and got["n_experts"].max() > 1
    # raw units, by the 50-digit loop on the converted rows
    pred, xprt = df[PL].values.T, df[XL].values.T
    val = df["f_bar"].values + osc * df["f*"].values
    grad, hess = osc * df[GRADS].values.T, osc * df[HESS].values.T
    _, _, F, G, H, kappa = gh.glue_hess_mp(key, pred, xprt, val, grad, hess, rad / 3)
    np.testing.assert_allclose(got["f*"].values, F, rtol=1e-13)
    assert (np.abs(got[HESS].values.T - H) <= 1e-12 * kappa).all()
    np.testing.assert_array_equal(got["f*_lap"].values, got["f*_hess_x_x"].values + got["f*_hess_y_y"].values)
    # the per-expert mean bends the glued map: without it in the value the Hessian is another one
    no_mean = post.glue_local_hessian(df, PL, XL, rad, obs_scale=osc, mean_col=None, engine=eng)
    assert np.abs(no_mean["f*_hess_x_y"].values - got["f*_hess_x_y"].values).max() > 1e-3
    np.testing.assert_allclose(no_mean[HESS].values.T, gh.glue_hess_fast(key, pred, xprt, osc * df["f*"].values, grad, hess, rad / 3)[4], rtol=1e-10, atol=1e-12)
    # one glue axis, named columns, strings for the column lists: the Laplacian is the one second derivative
    one = post.glue_local_hessian(df, "pred_loc_x", "x", rad, grad_cols="f*_grad_x", hess_cols="f*_hess_x_x", mean_col=None, engine=eng)
    assert list(one.columns) == ["pred_loc_x", "f*", "f*_grad_x", "f*_hess_x_x", "f*_lap", "n_experts"] and len(one) == df["pred_loc_x"].nunique()
    assert (np.diff(one["pred_loc_x"].values) > 0).all()
    np.testing.assert_array_equal(one["f*_lap"].values, one["f*_hess_x_x"].values)
    k1 = eng.calls[-1]["key"]
    H1 = gh.glue_hess_fast(k1, df[["pred_loc_x"]].values.T, df[["x"]].values.T, df["f*"].values, df[["f*_grad_x"]].values.T,
                           df[["f*_hess_x_x"]].values.T, rad / 3)[4]
    np.testing.assert_array_equal(one["f*_hess_x_x"].values, H1[0])
    # columns that are not called pred_loc_<c> keep their whole name in the defaults
    ren = df.rename(columns={"pred_loc_x": "px", "f*_grad_x": "f*_grad_px", "f*_hess_x_x": "f*_hess_px_px"})
    assert list(post.glue_local_hessian(ren, ["px"], ["x"], rad, engine=eng).columns) == ["px", "f*", "f*_grad_px", "f*_hess_px_px", "f*_lap", "n_experts"]


def test_glue_local_hessian_other_coords_against_the_closed_forms():
    """t is no glue axis: dF/dt = sum w~ f_t, d2F/dt2 = sum w~ f_tt, d2F/dp_c dt = (sum w (h_ct + u_c f_t) - F_t U_c) / W."""
    df = _preds(seed=1)
    osc, rad = 0.5, 6.0
    eng = gh.GlueHessNumpyEngine()
    got = post.glue_local_hessian(df, PL, XL, rad, obs_scale=osc, other_coords=["t"], also_glue=["f*_var"], engine=eng)
    assert list(got.columns) == PL + ["f*"] + GRADS + HESS + ["f*_lap", "n_experts"] + TCOLS + ["f*_var"]
    assert [("hess" in c, "grad" in c) for c in eng.calls] == [(True, False), (False, False), (False, True), (False, False)]
    key = eng.calls[0]["key"]
    sg = rad / 3
    d = df[XL].values.T - df[PL].values.T
    w = np.exp(-(d ** 2).sum(0) / (2 * sg * sg))            # the normalisation cancels with one sigma
    u = d / (sg * sg)
    su = lambda x: np.bincount(key, weights=x)
    W = su(w)
    ft, ftt = osc * df["f*_grad_t"].values, osc * df["f*_hess_t_t"].values
    Ft = su(w * ft) / W
    np.testing.assert_allclose(got["f*_grad_t"].values, Ft, rtol=1e-12)
    np.testing.assert_allclose(got["f*_hess_t_t"].values, su(w * ftt) / W, rtol=1e-12)
    for a, c in enumerate("xy"):
        hct = osc * df[f"f*_hess_{c}_t"].values
        want = (su(w * (hct + u[a] * ft)) - Ft * su(w * u[a])) / W
        np.testing.assert_allclose(got[f"f*_hess_{c}_t"].values, want, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match="must not name a glue axis"):
        post.glue_local_hessian(df, PL, XL, rad, other_coords=["x"], engine=eng)
    with pytest.raises(ValueError, match="no column.*f\\*_hess_x_z"):
        post.glue_local_hessian(df, PL, XL, rad, other_coords=["z"], engine=eng)


def test_glue_local_hessian_max_dist_leaves_nan_rows():
    df = _preds(seed=3)
    eng = gh.GlueHessNumpyEngine()
    got = post.glue_local_hessian(df, PL, XL, 6.0, max_dist=1.0, other_coords="t", also_glue=["f*_var"], engine=eng)
    full = post.glue_local_hessian(df, PL, XL, 6.0, engine=eng)
    assert [c["max_dist"] for c in eng.calls] == [1.0, 1.0, 1.0, 1.0, None]
    np.testing.assert_array_equal(got[PL].values, full[PL].values)        # a location that lost every expert keeps its row
    near = np.hypot(df["x"] - df["pred_loc_x"], df["y"] - df["pred_loc_y"]).values < 1.0
    np.testing.assert_array_equal(got["n_experts"].values, np.bincount(eng.calls[0]["key"], weights=near).astype(int))
    none = got["n_experts"].values == 0
    assert none.any() and not none.all()
    for c in ["f*"] + GRADS + HESS + ["f*_lap"] + TCOLS + ["f*_var"]:
        assert np.isnan(got[c].values[none]).all() and np.isfinite(got[c].values[~none]).all(), c
    # a row without a location belongs to no group
    lost = df.copy()
    lost.loc[[0, 5], "pred_loc_y"] = np.nan
    part = post.glue_local_hessian(lost, PL, XL, 6.0, engine=eng)
    key = eng.calls[-1]["key"]
    assert (key[[0, 5]] == -1).all() and (np.delete(key, [0, 5]) >= 0).all() and key.max() == len(part) - 1


def test_glue_local_hessian_refusals():
    df = _preds()
    eng = gh.GlueHessNumpyEngine()
    with pytest.raises(TypeError, match="one number"):
        post.glue_local_hessian(df, PL, XL, {1.0: 3.0}, engine=eng)
    with pytest.raises(ValueError, match="1 or 2 glue axes"):
        post.glue_local_hessian(df, [], [], 6.0, engine=eng)
    with pytest.raises(ValueError, match="1 or 2 glue axes"):
        post.glue_local_hessian(df, PL + ["pred_loc_t"], XL + ["x"], 6.0, engine=eng)
    with pytest.raises(ValueError, match="same number of glue axes"):
        post.glue_local_hessian(df, PL, ["x"], 6.0, engine=eng)
    with pytest.raises(ValueError, match="one gradient column per glue axis"):
        post.glue_local_hessian(df, PL, XL, 6.0, grad_cols=["f*_grad_x"], engine=eng)
    for cols in (["f*_hess_x_x"], HESS[:2], HESS + ["f*_hess_t_t"]):
        with pytest.raises(ValueError, match="one column per pair"):
            post.glue_local_hessian(df, PL, XL, 6.0, hess_cols=cols, engine=eng)
    with pytest.raises(ValueError, match="one column per pair"):
        post.glue_local_hessian(df, PL[:1], XL[:1], 6.0, hess_cols=HESS, engine=eng)
    for kw, name in ((dict(value_col="g*"), "g\\*"), (dict(mean_col="mu"), "mu"), (dict(also_glue=["nope"]), "nope"),
                     (dict(grad_cols=["f*_grad_x", "f*_grad_z"]), "f\\*_grad_z"), (dict(hess_cols=HESS[:2] + ["f*_hess_z_z"]), "f\\*_hess_z_z")):
        with pytest.raises(ValueError, match=f"no column.*{name}"):
            post.glue_local_hessian(df, PL, XL, 6.0, engine=eng, **dict(dict(grad_cols=GRADS, hess_cols=HESS), **kw))
    with pytest.raises(ValueError, match="no column.*f\\*_hess_x_y"):      # a run without pred_hess
        post.glue_local_hessian(df.drop(columns=["f*_hess_x_y"]), PL, XL, 6.0, engine=eng)
    with pytest.raises(ValueError, match="no column.*ex"):
        post.glue_local_hessian(df, PL, ["ex", "y"], 6.0, engine=eng)
    assert not eng.calls
