"""GPU: gpsat_glue_keyed_hess_batch against its restatements (tests/glue_hess_numpy.py) -- the glued value and the slope as
the bytes of gpsat_glue_keyed_grad_batch and at its bounds, the second derivatives of the glued map at C eps kappa from the
mpmath restatement -- its determinism, the edge cases and the capacity protocol, a property run and
postprocessing.glue_local_hessian on the device."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

import glue_grad_numpy as gg
import glue_hess_numpy as gh

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-14            # the glue's bound (tests/test_gpu_cv_glue.py), for the glued value
EPS = np.finfo(np.float64).eps
C_GRAD = 16.0                        # the slope's bound in eps kappa_a (tests/test_gpu_glue_grad.py)
# H_ab is held to C_HESS * EPS * kappa_ab of the mpmath restatement (kappa_ab: tests/glue_hess_numpy.py).  On exactly the
# inputs of `case` below (8 cases) the vectorised fp64 NumPy restatement lies within NUMPY_RATIO = 2.31 of these units of
# the 50-digit values, measured on the CPU (its slope within 1.34 of the slope's units).  The device -- another exp, an 8-lane summation order -- gets 4 times that and not
# less than 16.  test_numpy_restatement_in_units_of_the_bound repeats the measurement and holds it to C_HESS / 4, what the
# constant relies on.
NUMPY_RATIO = 2.31
C_HESS = max(16.0, 4 * NUMPY_RATIO)
# a lane's first, second and ninth row on a team of 8 lanes
SIZES = [1, 2, 7, 8, 9, 16, 17, 64, 65]
SIGMA = 1.0e5
CASES = [(1, False), (1, True), (2, False), (2, True)]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import default_engine
    return default_engine()


def max_dist_of(ndim):
    return 3.0e5 if ndim == 1 else 4.0e5


def rows(sizes, ndim, seed, sigma_rows, keys=None):
    """Interleaved rows of groups of the given sizes in EASE2-sized coordinates (around 3e6 m): key (negative on a sixth of
    the rows, which belong to no group), pred, xprt (every row within 4.5 sigma of its expert per axis), val around 3, grad
    of size 1 / sigma and hess of size 1 / sigma^2 with NaN rows among them, sigma.  With max_dist_of(ndim) some rows of
    most groups are cut and group 4 altogether."""
    rng = np.random.default_rng(seed)
    keys = np.arange(len(sizes), dtype=np.int64) * 3 + 1 if keys is None else np.asarray(keys, dtype=np.int64)
    ignored = keys.max() + 1                                # a fifth more rows, made like the others, whose keys turn negative
    sizes, keys = np.append(sizes, sum(sizes) // 5 + 1), np.append(keys, ignored)
    key = np.repeat(keys, sizes)
    R = len(key)
    npair = ndim * (ndim + 1) // 2
    pred = np.repeat(3.0e6 + rng.uniform(-1.0e6, 1.0e6, (ndim, len(sizes))), sizes, axis=1)
    sigma = rng.uniform(0.7, 1.4, R) * SIGMA if sigma_rows else SIGMA
    xprt = pred + rng.uniform(-4.5, 4.5, (ndim, R)) * sigma
    if len(sizes) > 4:
        far = key == keys[4]
        xprt[:, far] = pred[:, far] + 3.1e5                 # beyond max_dist_of, within 4.5 sigma (sigma >= 0.7e5)
    val = rng.normal(3.0, 1.0, R)
    grad = rng.normal(0.0, 1.0, (ndim, R)) / SIGMA
    hess = rng.normal(0.0, 1.0, (npair, R)) / SIGMA ** 2
    val[rng.random(R) < 0.06] = np.nan                      # a failed tile: no value (nothing else of the row is read)
    grad[:, rng.random(R) < 0.04] = np.nan                  # a value without a gradient
    grad[0, rng.random(R) < 0.03] = np.nan                  # one gradient component
    hess[:, rng.random(R) < 0.04] = np.nan                  # a value and a gradient without second derivatives
    hess[npair - 1, rng.random(R) < 0.03] = np.nan          # one Hessian entry
    p = rng.permutation(R)
    key, pred, xprt, val, grad, hess = key[p], pred[:, p], xprt[:, p], val[p], grad[:, p], hess[:, p]
    sigma = sigma[p] if sigma_rows else sigma
    key = np.where(key == ignored, -1 - np.arange(R) % 7, key)
    d2 = ((pred - xprt) ** 2).sum(axis=0)
    md = max_dist_of(ndim)
    assert (np.abs(d2 - md * md) > 1e-9 * md * md).all()    # no row at the boundary: the kernel's d2 may differ in its last bit
    return key, pred, xprt, val, grad, hess, sigma


def no_hess(a):
    return a[:5] + a[6:]


@functools.lru_cache(maxsize=None)
def case(ndim, sigma_rows, limited):
    """The inputs of one case, their 50-digit answer with kappa and the 50-digit slope with its kappa: computed once,
    shared, left unchanged."""
    a = rows(SIZES, ndim, seed=40 + 2 * ndim + sigma_rows, sigma_rows=sigma_rows)
    md = max_dist_of(ndim) if limited else None
    want = gh.glue_hess_mp(*a, md)
    kg = gg.glue_grad_mp(*no_hess(a), md)[4]
    for x in a + want + (kg,):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a, md, want, kg


def agree(got, want, kg=None, c=C_HESS):
    keys, counts, F, G, H, kappa = want
    np.testing.assert_array_equal(got[0], keys)
    np.testing.assert_array_equal(got[1], counts)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert got[2].shape == F.shape and got[3].shape == G.shape and got[4].shape == H.shape
    ok = counts > 0
    for x in got[2:5]:
        np.testing.assert_array_equal(np.isnan(x), np.broadcast_to(~ok, x.shape))
    np.testing.assert_allclose(got[2], F, rtol=RTOL, atol=ATOL)
    if kg is not None:
        assert (np.abs(got[3] - G)[:, ok] <= C_GRAD * EPS * kg[:, ok]).all()
    err, unit = np.abs(got[4] - H)[:, ok], EPS * kappa[:, ok]
    ratio = float((err[unit > 0] / unit[unit > 0]).max())  # kappa is 0 where a lone row has no value: F = G = H = 0 exactly
    print(f"second derivatives: largest |H - H_ref| / (eps kappa) = {ratio:.2f} (bound {c:g})")
    assert (err <= c * unit).all()
    return ratio


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("ndim,sigma_rows", CASES)
def test_numpy_restatement_in_units_of_the_bound(ndim, sigma_rows, limited):
    """The measurement behind C_HESS, on the CPU (no device is asked): the fp64 restatement against mpmath."""
    a, md, want, kg = case(ndim, sigma_rows, limited)
    assert agree(gh.glue_hess_fast(*a, md), want, kg, c=C_HESS / 4) <= NUMPY_RATIO


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("ndim,sigma_rows", CASES)
def test_group_sizes_against_the_restatement(eng, ndim, sigma_rows, limited):
    a, md, want, kg = case(ndim, sigma_rows, limited)
    key, pred, xprt, val, grad, hess, sigma = a
    got = eng.glue_keyed_hess_batch(*a, max_dist=md)
    agree(got, want, kg)
    assert (key < 0).any() and np.isnan(val).any() and np.isnan(grad).any() and np.isnan(hess).any()
    assert (np.isnan(grad[0]) & ~np.isnan(grad[-1]) & ~np.isnan(val)).any() or ndim == 1
    assert (np.isnan(hess[-1]) & ~np.isnan(hess[0]) & ~np.isnan(val)).any() or ndim == 1
    if limited:
        assert got[1][4] == 0 and 0 < got[1].sum() < (key >= 0).sum() and (got[1] > 0).sum() == len(SIZES) - 1
    else:
        np.testing.assert_array_equal(got[1], SIZES)
    # the keys, the counts, the glued value and the slope: the bytes of the keyed gradient glue on the same rows
    same = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md)
    for u, v in zip(got[:4], same):
        assert u.tobytes() == v.tobytes()


def test_a_group_depends_on_its_own_rows_only(eng):
    (key, pred, xprt, val, grad, hess, sigma), md, _, _ = case(2, True, True)
    cols = lambda sel: (key[sel], pred[:, sel], xprt[:, sel], val[sel], grad[:, sel], hess[:, sel], sigma[sel])
    base = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist=md)
    again = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist=md)
    for u, v in zip(base, again):
        assert u.tobytes() == v.tobytes()                   # a second call: the same bytes
    rng = np.random.default_rng(0)
    R = len(key)
    for j, k in enumerate(base[0]):
        others = np.nonzero(key != k)[0]
        perm = np.arange(R)
        perm[others] = rng.permutation(others)              # the other keys' rows permuted among their places
        got = eng.glue_keyed_hess_batch(*cols(perm), max_dist=md)
        np.testing.assert_array_equal(got[0], base[0])
        assert got[1][j] == base[1][j] and got[2][j:j + 1].tobytes() == base[2][j:j + 1].tobytes(), ("permuted", k)
        assert got[3][:, j].tobytes() == base[3][:, j].tobytes() and got[4][:, j].tobytes() == base[4][:, j].tobytes(), ("permuted", k)
        alone = eng.glue_keyed_hess_batch(*cols(np.nonzero(key == k)[0]), max_dist=md)
        assert alone[0].tolist() == [k] and alone[1][0] == base[1][j], ("alone", k)
        assert alone[2].tobytes() == base[2][j:j + 1].tobytes() and alone[3][:, 0].tobytes() == base[3][:, j].tobytes(), ("alone", k)
        assert alone[4][:, 0].tobytes() == base[4][:, j].tobytes(), ("alone", k)


def test_degenerate_calls(eng):
    e = np.zeros((2, 0))
    got = eng.glue_keyed_hess_batch(np.zeros(0, dtype=np.int64), e, e, np.zeros(0), e, np.zeros((3, 0)), 1.0)      # R = 0
    assert [x.shape for x in got] == [(0,), (0,), (0,), (2, 0), (3, 0)]
    key, pred, xprt, val, grad, hess, sigma = case(1, False, False)[0]
    got = eng.glue_keyed_hess_batch(-1 - np.abs(key), pred, xprt, val, grad, hess, sigma)             # no key >= 0
    assert got[0].shape == (0,) and got[3].shape == (1, 0) and got[4].shape == (1, 0)
    # a group wholly beyond max_dist among others: count 0, NaN
    key, pred, xprt, val, grad, hess, sigma = case(2, False, True)[0]
    got = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist=max_dist_of(2))
    assert got[1][4] == 0 and np.isnan(got[2][4]) and np.isnan(got[3][:, 4]).all() and np.isnan(got[4][:, 4]).all()
    assert np.isfinite(np.delete(got[4], 4, axis=1)).all()
    # one row alone: F = f, G = g and H = h, whatever the weight's own derivatives are
    h = np.array([[2.0e-10], [-1.0e-10], [3.0e-10]])
    got = eng.glue_keyed_hess_batch(np.array([7]), np.array([[3.0e6], [2.0e6]]), np.array([[3.2e6], [1.9e6]]), np.array([2.5]),
                                    np.array([[4.0e-6], [-2.0e-6]]), h, SIGMA)
    assert got[0].tolist() == [7] and got[1].tolist() == [1] and got[2][0] == 2.5
    assert np.abs(got[3][:, 0] - [4.0e-6, -2.0e-6]).max() < C_GRAD * EPS * 1e-4
    # kappa: |h| + 2 |u g| + |c| 2 |f| + 2 |G U| / W with |u| <= 2e-5, |c| <= 4e-10: below 4e-9
    assert np.abs(got[4][:, 0] - h[:, 0]).max() < C_HESS * EPS * 4e-9


def test_capacity_too_small_reports_G_and_the_handle_stays_usable(eng):
    (key, pred, xprt, val, grad, hess, sigma), md, _, _ = case(2, False, True)
    pred, xprt, grad, hess = (np.ascontiguousarray(a) for a in (pred, xprt, grad, hess))      # handed to the library as they are
    base = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist=md)
    lib, h = eng._lib, eng._h
    R, G = len(key), len(SIZES)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(cap, ndim=2):
        m = max(cap, 1)
        ok, oc, ov, n = np.full(m, -5, dtype=np.int64), np.full(m, -5, dtype=np.int32), np.full(m, -5.0), C.c_int64(-1)
        og, oh = np.full((2, m), -5.0), np.full((3, m), -5.0)
        rc = lib.gpsat_glue_keyed_hess_batch(h, R, ndim, ptr(key), ptr(pred), ptr(xprt), ptr(val), ptr(grad), ptr(hess), float(sigma),
                                             None, float(md), cap, C.byref(n), ptr(ok), ptr(oc), ptr(ov), ptr(og), ptr(oh))
        return rc, int(n.value), ok, oc, ov, og, oh

    def same_as_base():
        for u, v in zip(eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist=md), base):
            assert u.tobytes() == v.tobytes()

    for cap in (G - 1, 1, 0):
        rc, n, ok, oc, ov, og, oh = call(cap)
        assert rc == -1 and n == G and f"capacity {cap} < G {G}" in lib.gpsat_last_error().decode()
        assert (ok == -5).all() and (oc == -5).all() and (ov == -5.0).all() and (og == -5.0).all() and (oh == -5.0).all()      # nothing written
        same_as_base()
    rc, n, ok, oc, ov, og, oh = call(G)                     # sized by the G of the refused call
    assert rc == 0 and n == G
    assert ok.tobytes() == base[0].tobytes() and oc.tobytes() == base[1].tobytes()
    assert ov.tobytes() == base[2].tobytes() and og.tobytes() == base[3].tobytes() and oh.tobytes() == base[4].tobytes()
    rc, n, ok, oc, ov, og, oh = call(G + 7)                 # a larger capacity: pair k at out_hess + k * capacity
    assert rc == 0 and ov[:G].tobytes() == base[2].tobytes() and np.ascontiguousarray(og[:, :G]).tobytes() == base[3].tobytes()
    assert np.ascontiguousarray(oh[:, :G]).tobytes() == base[4].tobytes()
    assert (oh[:, G:] == -5.0).all() and (og[:, G:] == -5.0).all() and (ov[G:] == -5.0).all() and (ok[G:] == -5).all()
    # a refusal of the checks leaves the handle usable as well
    rc, n, *_ = call(G, ndim=3)
    assert rc == -1 and "gpsat_glue_keyed_hess_batch: ndim" in lib.gpsat_last_error().decode()
    same_as_base()
    assert all(t >= 0.0 for t in eng.glue_keyed_timing())


# The property run's inputs are made like the cases' and are a thousand times as many: the weights' rounding grows with z^2
# (rows out to 4.5 sigma on two axes: an exponent of up to 20, known to ~20 eps), and among 20 000 groups the tail of that
# shows.  On exactly these inputs the vectorised restatement lies within 19.45 units of the 50-digit values (measured on the
# CPU, 30 s of mpmath: not repeated here).  By the rule above the device gets 4 times that from the exact value, so the two
# fp64 results may lie 5 times that apart.
NUMPY_RATIO_PROPERTY = 19.45
C_PROPERTY = 5 * NUMPY_RATIO_PROPERTY


def property_rows():
    rng = np.random.default_rng(177)
    sizes = rng.integers(1, 20, 20000)
    sizes = np.append(sizes, 200000 - sizes.sum())
    return rows(sizes, 2, seed=178, sigma_rows=True), max_dist_of(2)


def test_property_run_against_the_vectorised_restatement(eng):
    """200 000 rows in about 20 000 groups, fp64 on both sides: C_PROPERTY above."""
    a, md = property_rows()
    want = gh.glue_hess_fast(*a, md)
    got = eng.glue_keyed_hess_batch(*a, max_dist=md)
    assert (a[0] >= 0).sum() == 200000 and len(got[0]) == 20001 and (want[1] == 0).any()
    agree(got, want, c=C_PROPERTY)
    same = eng.glue_keyed_grad_batch(*no_hess(a), max_dist=md)
    assert got[2].tobytes() == same[2].tobytes() and got[3].tobytes() == same[3].tobytes()


def test_glue_local_hessian_on_the_device(eng):
    from gpsat_amd import postprocessing as post
    rng = np.random.default_rng(6)
    gx, gy = (a.reshape(-1) for a in np.meshgrid(np.linspace(-4, 4, 9)[::-1] * SIGMA, np.linspace(-3, 3, 7) * SIGMA, indexing="ij"))
    ex, ey = rng.uniform(-4, 4, 12) * SIGMA, rng.uniform(-3, 3, 12) * SIGMA
    dist = np.hypot(ex[:, None] - gx[None], ey[:, None] - gy[None])
    e, j = np.nonzero((dist < 3.0 * SIGMA) | (dist <= np.sort(dist, axis=0)[1]))
    n = len(e)
    grads, hcols = ["f*_grad_x", "f*_grad_y"], ["f*_hess_x_x", "f*_hess_x_y", "f*_hess_y_y"]
    fr = {"x": 3.0e6 + ex[e], "y": -2.0e6 + ey[e], "pred_loc_x": 3.0e6 + gx[j], "pred_loc_y": -2.0e6 + gy[j],
          "f*": rng.normal(0, 1, n), "f*_var": rng.uniform(0.1, 0.2, n), "f_bar": 20.0 + rng.normal(0, 1, 12)[e]}
    fr.update({c: rng.normal(0, 1, n) / SIGMA for c in grads + ["f*_hess_x_t", "f*_hess_y_t"]})
    fr.update({c: rng.normal(0, 1, n) / SIGMA ** 2 for c in hcols})
    fr.update({"f*_grad_t": rng.normal(0, 1, n), "f*_hess_t_t": rng.normal(0, 1, n)})
    df = pd.DataFrame(fr)
    pl, xl = ["pred_loc_x", "pred_loc_y"], ["x", "y"]
    kw = dict(R=3, obs_scale=0.5, other_coords=["t"], also_glue=["f*_var"], max_dist=2.9 * SIGMA)
    ref_eng = gh.GlueHessNumpyEngine()
    want = post.glue_local_hessian(df, pl, xl, 3.0 * SIGMA, engine=ref_eng, **kw)
    got = post.glue_local_hessian(df, pl, xl, 3.0 * SIGMA, engine=eng, **kw)
    assert list(got.columns) == list(want.columns) and len(got) == 63
    for c in ("pred_loc_x", "pred_loc_y", "n_experts"):
        np.testing.assert_array_equal(got[c].values, want[c].values)
    for c in ("f*", "f*_var", "f*_grad_t", "f*_hess_t_t"):
        np.testing.assert_allclose(got[c].values, want[c].values, rtol=RTOL, atol=ATOL, equal_nan=True)
    assert got["n_experts"].max() > 2
    some = want["n_experts"].values > 0
    assert some.sum() > 50 and not some.all() and np.isnan(got.loc[~some, ["f*", "f*_lap"] + grads + hcols].values).all()
    np.testing.assert_array_equal(got["f*_lap"].values[some], (got["f*_hess_x_x"] + got["f*_hess_y_y"]).values[some])
    # the second derivatives: both answers against mpmath on the rows the function handed to the engine, the device at
    # C_HESS and the device-free engine at the quarter of it that C_HESS allows the restatement
    exact = gh.glue_hess_mp(*ref_eng.last_hess)
    kg = gg.glue_grad_mp(*no_hess(ref_eng.last_hess))[4]
    agree((exact[0], exact[1], got["f*"].values, got[grads].values.T, got[hcols].values.T), exact, kg)
    agree((exact[0], exact[1], want["f*"].values, want[grads].values.T, want[hcols].values.T), exact, kg, c=C_HESS / 4)
    # the mixed derivatives: the slope of the glued df/dt, on the rows of the last gradient call
    mixed = gg.glue_grad_mp(*ref_eng.last)
    ok = mixed[1] > 0
    err = np.abs(got[["f*_hess_x_t", "f*_hess_y_t"]].values.T - mixed[3])[:, ok]
    assert (err <= C_GRAD * EPS * mixed[4][:, ok]).all()
