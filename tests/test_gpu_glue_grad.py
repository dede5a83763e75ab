"""GPU: gpsat_glue_keyed_grad_batch against its restatements (tests/glue_grad_numpy.py) -- the glued value at the glue's
bound and as the bytes of gpsat_glue_keyed_batch, the slope of the glued map at C eps kappa from the mpmath restatement --
its determinism, the capacity protocol, a property run and postprocessing.glue_local_gradient on the device."""
import ctypes as C
import functools

import numpy as np
import pandas as pd
import pytest

import glue_grad_numpy as gg

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-14            # the glue's bound (tests/test_gpu_cv_glue.py), for the glued value
EPS = np.finfo(np.float64).eps
# The slope is held to C_GRAD * EPS * kappa_a of the mpmath restatement, kappa_a = sum w~ (|g_a| + |u_a| (|f| + |F|)).
# On exactly the inputs of `case` below (4 cases, with and without max_dist) the fp64 NumPy restatement lies within
# NUMPY_RATIO = 1.03 of these units of the 50-digit values, measured on the CPU.  The device -- another exp, an 8-lane
# summation order -- gets 4 times that and not less than 16: C_GRAD = 16.  test_numpy_restatement_in_units_of_the_bound
# repeats the measurement and holds it to C_GRAD / 4, what the constant and the fp64-to-fp64 bound below rely on.
NUMPY_RATIO = 1.03
C_GRAD = max(16.0, 4 * NUMPY_RATIO)
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
    the rows, which belong to no group), pred, xprt (every row within 4.5 sigma of its expert per axis), val around 3 and
    grad of size 1 / sigma with NaN rows among them, sigma.  With max_dist_of(ndim) some rows of most groups are cut and group 4 altogether."""
    rng = np.random.default_rng(seed)
    keys = np.arange(len(sizes), dtype=np.int64) * 3 + 1 if keys is None else np.asarray(keys, dtype=np.int64)
    ignored = keys.max() + 1                                # a fifth more rows, made like the others, whose keys turn negative
    sizes, keys = np.append(sizes, sum(sizes) // 5 + 1), np.append(keys, ignored)
    key = np.repeat(keys, sizes)
    R = len(key)
    pred = np.repeat(3.0e6 + rng.uniform(-1.0e6, 1.0e6, (ndim, len(sizes))), sizes, axis=1)
    sigma = rng.uniform(0.7, 1.4, R) * SIGMA if sigma_rows else SIGMA
    xprt = pred + rng.uniform(-4.5, 4.5, (ndim, R)) * sigma
    if len(sizes) > 4:
        far = key == keys[4]
        xprt[:, far] = pred[:, far] + 3.1e5                 # beyond max_dist_of, within 4.5 sigma (sigma >= 0.7e5)
    val = rng.normal(3.0, 1.0, R)
    grad = rng.normal(0.0, 1.0, (ndim, R)) / SIGMA
    val[rng.random(R) < 0.06] = np.nan                      # a failed tile: no value (its gradient is not read)
    grad[:, rng.random(R) < 0.06] = np.nan                  # a value without a gradient
    grad[0, rng.random(R) < 0.03] = np.nan
    p = rng.permutation(R)
    key, pred, xprt, val, grad = key[p], pred[:, p], xprt[:, p], val[p], grad[:, p]
    sigma = sigma[p] if sigma_rows else sigma
    key = np.where(key == ignored, -1 - np.arange(R) % 7, key)
    d2 = ((pred - xprt) ** 2).sum(axis=0)
    md = max_dist_of(ndim)
    assert (np.abs(d2 - md * md) > 1e-9 * md * md).all()    # no row at the boundary: the kernel's d2 may differ in its last bit
    return key, pred, xprt, val, grad, sigma


@functools.lru_cache(maxsize=None)
def case(ndim, sigma_rows, limited):
    """The inputs of one case, and their 50-digit answer with kappa: computed once, shared, left unchanged."""
    a = rows(SIZES, ndim, seed=20 + 2 * ndim + sigma_rows, sigma_rows=sigma_rows)
    md = max_dist_of(ndim) if limited else None
    want = gg.glue_grad_mp(*a, md)
    for x in a + want:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a, md, want


def agree(got, want, c=C_GRAD):
    keys, counts, F, G, kappa = want
    np.testing.assert_array_equal(got[0], keys)
    np.testing.assert_array_equal(got[1], counts)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].shape == F.shape and got[3].shape == G.shape
    np.testing.assert_array_equal(np.isnan(got[2]), counts == 0)
    np.testing.assert_array_equal(np.isnan(got[3]), np.broadcast_to(counts == 0, G.shape))
    np.testing.assert_allclose(got[2], F, rtol=RTOL, atol=ATOL)
    ok = counts > 0
    err, unit = np.abs(got[3] - G)[:, ok], EPS * kappa[:, ok]
    ratio = float((err[unit > 0] / unit[unit > 0]).max())  # kappa is 0 where a lone row has no value: F = G = 0 exactly
    print(f"slope: largest |G - G_ref| / (eps kappa) = {ratio:.2f} (bound {c:g})")
    assert (err <= c * unit).all()
    return ratio


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("ndim,sigma_rows", CASES)
def test_numpy_restatement_in_units_of_the_bound(ndim, sigma_rows, limited):
    """The measurement behind C_GRAD, on the CPU (no device is asked): the fp64 restatements against mpmath."""
    a, md, want = case(ndim, sigma_rows, limited)
    agree(gg.glue_grad(*a, md), want, c=C_GRAD / 4)
    agree(gg.glue_grad_fast(*a, md)[:4], want, c=C_GRAD / 4)


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("ndim,sigma_rows", CASES)
def test_group_sizes_against_the_restatement(eng, ndim, sigma_rows, limited):
    a, md, want = case(ndim, sigma_rows, limited)
    got = eng.glue_keyed_grad_batch(*a, max_dist=md)
    agree(got, want)
    key = a[0]
    assert (key < 0).any() and np.isnan(a[3]).any() and np.isnan(a[4]).any()
    if limited:
        assert got[1][4] == 0 and 0 < got[1].sum() < (key >= 0).sum() and (got[1] > 0).sum() == len(SIZES) - 1
    else:
        np.testing.assert_array_equal(got[1], SIZES)
    # the glued value, the keys and the counts: the bytes of the keyed glue on the value column alone
    keys, counts, out = eng.glue_keyed_batch(key, a[1], a[2], a[3][None], a[5], max_dist=md)
    assert got[0].tobytes() == keys.tobytes() and got[1].tobytes() == counts.tobytes() and got[2].tobytes() == out[0].tobytes()


def test_a_group_depends_on_its_own_rows_only(eng):
    (key, pred, xprt, val, grad, sigma), md, _ = case(2, True, True)
    cols = lambda sel: (key[sel], pred[:, sel], xprt[:, sel], val[sel], grad[:, sel], sigma[sel])
    base = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md)
    again = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md)
    for u, v in zip(base, again):
        assert u.tobytes() == v.tobytes()                   # a second call: the same bytes
    rng = np.random.default_rng(0)
    R = len(key)
    for j, k in enumerate(base[0]):
        others = np.nonzero(key != k)[0]
        perm = np.arange(R)
        perm[others] = rng.permutation(others)              # the other keys' rows permuted among their places
        got = eng.glue_keyed_grad_batch(*cols(perm), max_dist=md)
        np.testing.assert_array_equal(got[0], base[0])
        assert got[1][j] == base[1][j] and got[2][j:j + 1].tobytes() == base[2][j:j + 1].tobytes(), ("permuted", k)
        assert got[3][:, j].tobytes() == base[3][:, j].tobytes(), ("permuted", k)
        alone = eng.glue_keyed_grad_batch(*cols(np.nonzero(key == k)[0]), max_dist=md)
        assert alone[0].tolist() == [k] and alone[1][0] == base[1][j], ("alone", k)
        assert alone[2].tobytes() == base[2][j:j + 1].tobytes() and alone[3][:, 0].tobytes() == base[3][:, j].tobytes(), ("alone", k)


def test_degenerate_calls(eng):
    e = np.zeros((2, 0))
    got = eng.glue_keyed_grad_batch(np.zeros(0, dtype=np.int64), e, e, np.zeros(0), e, 1.0)          # R = 0
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].shape == (0,) and got[3].shape == (2, 0)
    key, pred, xprt, val, grad, sigma = case(1, False, False)[0]
    got = eng.glue_keyed_grad_batch(-1 - np.abs(key), pred, xprt, val, grad, sigma)                   # no key >= 0
    assert got[0].shape == (0,) and got[3].shape == (1, 0)
    # one row: F = f and G = g, whatever the weight's own slope is
    got = eng.glue_keyed_grad_batch(np.array([7]), np.array([[3.0e6]]), np.array([[3.2e6]]), np.array([2.5]), np.array([[4.0e-6]]), SIGMA)
    assert got[0].tolist() == [7] and got[1].tolist() == [1] and got[2][0] == 2.5 and abs(got[3][0, 0] - 4.0e-6) < 16 * EPS * 5e-5


def test_capacity_too_small_reports_G_and_the_handle_stays_usable(eng):
    (key, pred, xprt, val, grad, sigma), md, _ = case(2, False, True)
    pred, xprt, grad = (np.ascontiguousarray(a) for a in (pred, xprt, grad))      # handed to the library as they are
    base = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md)
    lib, h = eng._lib, eng._h
    R, G = len(key), len(SIZES)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(cap, ndim=2):
        m = max(cap, 1)
        ok, oc, ov, og, n = np.full(m, -5, dtype=np.int64), np.full(m, -5, dtype=np.int32), np.full(m, -5.0), np.full((2, m), -5.0), C.c_int64(-1)
        rc = lib.gpsat_glue_keyed_grad_batch(h, R, ndim, ptr(key), ptr(pred), ptr(xprt), ptr(val), ptr(grad), float(sigma), None,
                                             float(md), cap, C.byref(n), ptr(ok), ptr(oc), ptr(ov), ptr(og))
        return rc, int(n.value), ok, oc, ov, og

    def same_as_base():
        for u, v in zip(eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md), base):
            assert u.tobytes() == v.tobytes()

    for cap in (G - 1, 1, 0):
        rc, n, ok, oc, ov, og = call(cap)
        assert rc == -1 and n == G and f"capacity {cap} < G {G}" in lib.gpsat_last_error().decode()
        assert (ok == -5).all() and (oc == -5).all() and (ov == -5.0).all() and (og == -5.0).all()      # nothing written
        same_as_base()
    rc, n, ok, oc, ov, og = call(G)                         # sized by the G of the refused call
    assert rc == 0 and n == G
    assert ok.tobytes() == base[0].tobytes() and oc.tobytes() == base[1].tobytes()
    assert ov.tobytes() == base[2].tobytes() and og.tobytes() == base[3].tobytes()
    rc, n, ok, oc, ov, og = call(G + 7)                     # a larger capacity: component a at out_grad + a * capacity
    assert rc == 0 and ov[:G].tobytes() == base[2].tobytes() and np.ascontiguousarray(og[:, :G]).tobytes() == base[3].tobytes()
    assert (og[:, G:] == -5.0).all() and (ov[G:] == -5.0).all() and (ok[G:] == -5).all()
    # a refusal of the checks leaves the handle usable as well
    rc, n, *_ = call(G, ndim=3)
    assert rc == -1 and "gpsat_glue_keyed_grad_batch: ndim" in lib.gpsat_last_error().decode()
    same_as_base()
    assert all(t >= 0.0 for t in eng.glue_keyed_timing())


# The property run's inputs are made like the cases' and are a thousand times as many: the weights' rounding grows with z^2
# (rows out to 4.5 sigma on two axes: an exponent of up to 20, known to ~20 eps), and among 20 000 groups the tail of that
# shows.  On exactly these inputs the vectorised restatement lies within 10.62 units of the 50-digit values (measured on the
# CPU, 20 s of mpmath: not repeated here).  By the rule above the device gets 4 times that from the exact value, so the two
# fp64 results may lie 5 times that apart.
NUMPY_RATIO_PROPERTY = 10.62
C_PROPERTY = 5 * NUMPY_RATIO_PROPERTY


def test_property_run_against_the_vectorised_restatement(eng):
    """200 000 rows in about 20 000 groups, fp64 on both sides: C_PROPERTY above."""
    rng = np.random.default_rng(77)
    sizes = rng.integers(1, 20, 20000)
    sizes = np.append(sizes, 200000 - sizes.sum())
    key, pred, xprt, val, grad, sigma = rows(sizes, 2, seed=78, sigma_rows=True)
    md = max_dist_of(2)
    want = gg.glue_grad_fast(key, pred, xprt, val, grad, sigma, md)
    got = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist=md)
    assert (key >= 0).sum() == 200000 and len(got[0]) == 20001 and (want[1] == 0).any()
    agree(got, want, c=C_PROPERTY)
    out = eng.glue_keyed_batch(key, pred, xprt, val[None], sigma, max_dist=md)[2]
    assert got[2].tobytes() == out[0].tobytes()


def test_glue_local_gradient_on_the_device(eng):
    from gpsat_amd import postprocessing as post
    rng = np.random.default_rng(5)
    gx, gy = (a.reshape(-1) for a in np.meshgrid(np.linspace(-4, 4, 9)[::-1] * SIGMA, np.linspace(-3, 3, 7) * SIGMA, indexing="ij"))
    ex, ey = rng.uniform(-4, 4, 12) * SIGMA, rng.uniform(-3, 3, 12) * SIGMA
    dist = np.hypot(ex[:, None] - gx[None], ey[:, None] - gy[None])
    e, j = np.nonzero((dist < 3.0 * SIGMA) | (dist <= np.sort(dist, axis=0)[1]))
    n = len(e)
    df = pd.DataFrame({"x": 3.0e6 + ex[e], "y": -2.0e6 + ey[e], "pred_loc_x": 3.0e6 + gx[j], "pred_loc_y": -2.0e6 + gy[j],
                       "f*": rng.normal(0, 1, n), "f*_var": rng.uniform(0.1, 0.2, n), "f_bar": 20.0 + rng.normal(0, 1, 12)[e],
                       "f*_grad_x": rng.normal(0, 1, n) / SIGMA, "f*_grad_y": rng.normal(0, 1, n) / SIGMA})
    kw = dict(R=3, obs_scale=0.5, also_glue=["f*_var"], max_dist=2.9 * SIGMA)
    ref_eng = gg.GlueGradNumpyEngine()
    want = post.glue_local_gradient(df, ["pred_loc_x", "pred_loc_y"], ["x", "y"], 3.0 * SIGMA, engine=ref_eng, **kw)
    got = post.glue_local_gradient(df, ["pred_loc_x", "pred_loc_y"], ["x", "y"], 3.0 * SIGMA, engine=eng, **kw)
    assert list(got.columns) == list(want.columns) and len(got) == 63
    for c in ("pred_loc_x", "pred_loc_y", "n_experts"):
        np.testing.assert_array_equal(got[c].values, want[c].values)
    for c in ("f*", "f*_var"):
        np.testing.assert_allclose(got[c].values, want[c].values, rtol=RTOL, atol=ATOL, equal_nan=True)
    assert got["n_experts"].max() > 2
    some = want["n_experts"].values > 0
    assert some.sum() > 50 and not some.all() and np.isnan(got.loc[~some, ["f*", "f*_grad_x", "f*_grad_y"]].values).all()
    # the slope: both answers against mpmath on the rows the function handed to the engine, the device at C_GRAD and the
    # device-free engine at the quarter of it that C_GRAD allows the restatement
    exact = gg.glue_grad_mp(*ref_eng.last)
    cols = ["f*_grad_x", "f*_grad_y"]
    agree((exact[0], exact[1], got["f*"].values, got[cols].values.T), exact)
    agree((exact[0], exact[1], want["f*"].values, want[cols].values.T), exact, c=C_GRAD / 4)
