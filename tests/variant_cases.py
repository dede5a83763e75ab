"""What differs between the variants of the exact fp64 expert, as data, and the helpers every variant's GPU tests share.

To add a fourth variant: one Case here (its fit_predict_batch keywords, how a batch and theta are drawn, its shapes), one
Variant in variant_numpy.py (its K_y and whatever arithmetic cannot merge bit for bit), and a tests/test_gpu_<name>.py for
what only it has, with the fixed-parameter, full-covariance and restatement tests as one-line calls of the bodies below.
tests/test_gpu_variants.py then holds it to the rest of the shared contract.
"""
import functools
import os

import numpy as np
import pytest

import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import sharding, synthetic as syn

KERNELS = ["RBF", "Matern12", "Matern32", "Matern52"]
FIELDS = ("theta", "nll", "grad", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var")


class Case:
    """A variant that reads obs_var=None, H = D + 2; the subclasses state what they change."""
    variant, name = None, ""
    SHAPES = [(1, 2, 1), (15, 5, 2), (16, 16, 3), (17, 3, 3), (100, 33, 3), (500, 40, 3)]
    T_fixed = 3                                            # tiles of a fixed-parameter batch
    x_large = None                                         # the extra parameter of the large-tile batch
    x_cov = []                                             # ... and of the full-covariance batch
    x_box = None                                           # ... and its box in a fit
    cov_D = [1, 2, 3]
    ragged_T, ragged_P0, alone = 60, 1, (17, 40)           # tiles, least P, and the tiles run alone
    empty_tile_returns_theta0 = True

    def call_kw(self, b):
        """The variant's keywords of fit_predict_batch."""
        return {}

    def kid(self, kernel):
        """The kernel synthetic.make_batch draws y from."""
        return L.KERNEL_IDS[kernel]

    def batch(self, T, N, P, D, kernel, base_seed):
        b = syn.make_batch(T, N, P, D, self.kid(kernel), base_seed=base_seed, dtype=np.float64)
        b["kernel"] = kernel
        return b

    def theta(self, rng, T, D, x=None):
        cols = [rng.uniform(1.5, 6.0, (T, D)), rng.uniform(0.05, 1.0, T), rng.uniform(0.01, 0.5, T)]
        return np.column_stack(cols + ([np.broadcast_to(x, (T,))] if self.variant.extra else []))

    def ragged_theta(self, rng, b, Ns, D):
        return self.theta(rng, len(Ns), D)

    def bounds(self, T, D):
        lo, hi = syn.default_bounds(T, D)
        if self.x_box is None:
            return lo, hi
        return np.column_stack([lo, np.full(T, self.x_box[0])]), np.column_stack([hi, np.full(T, self.x_box[1])])

    def start(self, th):
        """theta0 of the time-sliced fit, given the ragged batch's theta."""
        return np.ones(th.shape)

    def prior_mean(self, theta, D):
        return 0.0

    def prior_cov(self, kernel, Xs, theta):
        return vn.kernel_matrix(self.variant, kernel, Xs, Xs, theta)

    # what one variant asserts beyond the shared body of a test
    def after_fixed(self, eng, b, th, r):
        pass

    def check_ragged(self, b, r):
        assert r.status[3] == 4 and b["pred_off"][4] > b["pred_off"][3]

    def check_sliced(self, r0, th0, D):
        assert (r0.status <= 1).sum() > 40

    def after_sliced(self, eng, b, th0, kw, r0):
        pass

    def __repr__(self):
        return self.name


class RqCase(Case):
    """kernel="RationalQuadratic": H = D + 3 with alpha last; y is synthetic's RBF draw."""
    variant, name = vn.RQ, "rq"
    ALPHAS = [0.3, 1.0, 30.0]
    T_fixed, x_large, x_cov, x_box = 2, 2.0, [1.5], (0.1, 20.0)
    cov_D = [3, 1]
    ragged_T, ragged_P0, alone = 300, 0, (17, 100)
    empty_tile_returns_theta0 = False                      # not asserted for this variant

    def kid(self, kernel):
        return 0

    def batch(self, T, N, P, D, kernel, base_seed):
        return super().batch(T, N, P, D, vn.RQ_KERNEL, base_seed)

    def ragged_theta(self, rng, b, Ns, D):
        th = self.theta(rng, len(Ns), D, 1.0)
        th[:, D + 2] = rng.choice([0.3, 1.0, 4.0, 30.0], size=len(Ns))
        return th

    def check_ragged(self, b, r):
        pass

    def check_sliced(self, r0, th0, D):
        assert (r0.theta[r0.status <= 1, D + 2] != 1.0).all()                 # alpha moved


class MeanCase(Case):
    """mean="constant": H = D + 3 with c last; synthetic's de-meaned y on a level of SHIFT."""
    variant, name = vn.MEAN, "mean"
    SHIFT = 0.3
    CS = (-0.7, 0.0, 2.5)
    x_large, x_cov, x_box = (2.5, -0.7), [-0.7], (np.nan, np.nan)

    def call_kw(self, b):
        return {"mean": "constant"}

    def batch(self, T, N, P, D, kernel, base_seed):
        b = super().batch(T, N, P, D, kernel, base_seed)
        b["y"] = b["y"] + self.SHIFT
        return b

    def ragged_theta(self, rng, b, Ns, D):
        th = self.theta(rng, len(Ns), D, rng.choice([-0.7, 0.0, 0.3, 2.5], size=len(Ns)))
        th[3, D + 2] = 2.5
        return th

    def start(self, th):
        th0 = np.ones(th.shape)
        th0[:, -1] = th[:, -1]                               # a different start of c in every tile
        return th0

    def prior_mean(self, theta, D):
        return theta[D + 2]

    def check_ragged(self, b, r):
        super().check_ragged(b, r)
        assert (r.f_mean[b["pred_off"][3]:b["pred_off"][4]] == 2.5).all()     # the empty tile predicts its c

    def check_sliced(self, r0, th0, D):
        moved = r0.status <= 1
        assert moved.sum() > 40 and (r0.theta[moved, D + 2] != th0[moved, D + 2]).all()      # c moved


class NoiseCase(Case):
    """obs_var=: H = D + 2, D up to 4; v ~ U(0, vmax) per row, about one row in five exactly 0."""
    variant, name = vn.NOISE, "noise"
    SHAPES = [(1, 2, 1), (15, 5, 2), (16, 16, 3), (17, 3, 4), (100, 33, 3), (500, 40, 4)]

    def call_kw(self, b):
        return {"obs_var": b.get("obs_var")}

    def batch(self, T, N, P, D, kernel, base_seed, vmax=0.3):
        b = super().batch(T, N, P, D, kernel, base_seed)
        rng = np.random.default_rng(base_seed + 1)
        v = rng.uniform(0.0, vmax, int(b["obs_off"][-1]))
        v[rng.uniform(size=len(v)) < 0.2] = 0.0
        b["obs_var"] = v
        return b

    def ragged_theta(self, rng, b, Ns, D):
        b["obs_var"] = b["obs_var"] * np.repeat(rng.uniform(0.01, 3.0, len(Ns)), Ns)      # a scale of its own per tile
        return self.theta(rng, len(Ns), D)

    def after_fixed(self, eng, b, th, r):
        """v is really read: the plain call answers something else."""
        r0 = run(self, eng, b, th, obs_var=None)
        has_v = np.array([b["obs_var"][b["obs_off"][t]:b["obs_off"][t + 1]].any() for t in range(len(th))])
        assert has_v.any() and (r0.nll[has_v] != r.nll[has_v]).all() and (r0.nll[~has_v] == r.nll[~has_v]).all()

    def after_sliced(self, eng, b, th0, kw, r0):
        """The fit is the noise model's: not the plain call's."""
        rp = run(self, eng, b, th0, obs_var=None, **kw)
        big = (r0.status <= 1) & (np.diff(b["obs_off"]) >= 20)
        assert big.sum() > 30 and (rp.theta[big] != r0.theta[big]).any(axis=1).all()


RQ, MEAN, NOISE = RqCase(), MeanCase(), NoiseCase()
CASES = [RQ, MEAN, NOISE]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    """One workgroup per CU: the 8-wave build whatever the batch."""
    from gpsat_amd.engine import Engine
    e = Engine(0, workgroups_per_cu=1)
    yield e
    e.close()


def run(case, e, b, theta0, **kw):
    kw = {"optimiser": "none", "want_grad": True, **case.call_kw(b), **kw}
    return e.fit_predict_batch(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"],
                               theta0=theta0, kernel=b["kernel"], dtype="f64", **kw)


@functools.lru_cache(maxsize=None)
def ragged_inputs(case):
    """One ragged batch, N <= 200, in no order of size (an empty tile, tiles without prediction points), and its theta0: drawn
    once per variant, for every test that reads it."""
    T, D = case.ragged_T, 3
    rng = np.random.default_rng(5)
    Ns = rng.integers(1, 201, size=T)
    Ps = rng.integers(case.ragged_P0, 40, size=T)
    Ns[3], Ns[17], Ps[5] = 0, 200, 0
    b = case.batch(T, Ns.tolist(), Ps.tolist(), D, "Matern32", 8000)
    return b, case.ragged_theta(rng, b, Ns, D)


def check_tile(case, r, b, t, theta, what=""):
    """One tile of a result against variant_numpy at the same theta.  The four bounds, stated here once for every variant, are
    those of tests/test_gpu_parity.py::test_fp64_objective_gradient_predict: objective 1e-9 max(1, |nll|) N, gradient rtol 1e-7
    with atol 1e-8 (max|g| + 1), mean 1e-9 max(|y|max, 1), variances 1e-10.  A tile without observations returns the prior at
    theta0, exactly."""
    D, kernel = b["D"], b["kernel"]
    a, e, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
    N = int(e - a)
    X, y, Xs = b["X"][a:e], b["y"][a:e], b["Xs"][pa:pe]
    v = b["obs_var"][a:e] if case.variant is vn.NOISE else None
    if N == 0:
        assert r.status[t] == 4 and r.nll[t] == 0.0, what
        np.testing.assert_array_equal(r.f_mean[pa:pe], case.prior_mean(theta, D))
        np.testing.assert_array_equal(r.f_var[pa:pe], theta[D])
        np.testing.assert_array_equal(r.y_var[pa:pe], theta[D] + theta[D + 1])
        if case.empty_tile_returns_theta0:
            np.testing.assert_array_equal(r.theta[t], theta)
        return
    nll, g = vn.nll_and_grad(case.variant, kernel, X, y, theta, v)
    ymax = np.abs(y).max()
    assert abs(r.nll[t] - nll) <= 1e-9 * max(1.0, abs(nll)) * max(N, 1), (what, t, N, r.nll[t], nll)
    np.testing.assert_allclose(r.grad[t], g, rtol=1e-7, atol=1e-8 * (np.abs(g).max() + 1), err_msg=f"{what} tile {t} N {N}")
    if pe > pa:
        f, fv, yv = vn.predict(case.variant, kernel, X, y, Xs, theta, v)
        np.testing.assert_allclose(r.f_mean[pa:pe], f, rtol=0, atol=1e-9 * max(ymax, 1.0), err_msg=f"{what} tile {t}")
        np.testing.assert_allclose(r.f_var[pa:pe], fv, rtol=0, atol=1e-10, err_msg=f"{what} tile {t}")
        np.testing.assert_allclose(r.y_var[pa:pe], yv, rtol=0, atol=1e-10, err_msg=f"{what} tile {t}")


def check_fixed_parameters(case, e, kernel, N, P, D, seed, x, what, eight_wave=False):
    """A batch of the case's tiles at fixed parameters (theta drawn from ``seed``, the extra parameter ``x``) against
    variant_numpy, on the 4-wave or the 8-wave build; the 4-wave test also holds the call's shapes and statuses."""
    T, H = case.T_fixed, D + 2 + case.variant.extra
    b = case.batch(T, N, P, D, kernel, 7000 + N)
    th = case.theta(np.random.default_rng(seed), T, D, x)
    r = run(case, e, b, th)
    if not eight_wave:
        assert r.theta.shape == (T, H) and r.grad.shape == (T, H) and r.f_mean.dtype == np.float64
        assert (r.status == 5).all() and (r.n_eval == 0).all()
        np.testing.assert_array_equal(r.theta, th)
    for t in range(T):
        check_tile(case, r, b, t, th[t], what)
    if not eight_wave:
        case.after_fixed(e, b, th, r)


def check_full_cov(case, e, D):
    """The full covariance of a ragged batch at fixed parameters, to 1e-9: the fp64 bound of
    tests/test_gpu_parity.py::test_full_cov_ragged_batch_matches_oracle."""
    Ns, Ps = [40, 0, 100, 33, 257, 64], [5, 3, 0, 32, 70, 1]
    T = len(Ns)
    b = case.batch(T, Ns, Ps, D, KERNELS[D], 321)
    kernel = b["kernel"]                                   # RationalQuadratic has one
    th0 = np.tile(np.concatenate([np.full(D, 2.0), [0.8, 0.05], case.x_cov]), (T, 1))
    r = run(case, e, b, th0, full_cov=True, want_grad=False)
    r0 = run(case, e, b, th0, want_grad=False)
    np.testing.assert_array_equal(r.f_mean, r0.f_mean)
    np.testing.assert_array_equal(r.f_var, r0.f_var)
    assert r0.f_cov is None and len(r.f_cov) == sum(p * p for p in Ps)
    tol = 1e-9
    for t in range(T):
        a, o, pa, pe = b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]
        P = pe - pa
        if P == 0:
            continue
        Cv = np.asarray(r.f_cov[r.cov_off[t]:r.cov_off[t + 1]]).reshape(P, P)
        Xs = b["Xs"][pa:pe]
        v = b["obs_var"][a:o] if case.variant is vn.NOISE else None
        ref = case.prior_cov(kernel, Xs, th0[t]) if Ns[t] == 0 else \
            vn.predict_cov(case.variant, kernel, b["X"][a:o], b["y"][a:o], Xs, th0[t], v)
        np.testing.assert_allclose(Cv, ref, rtol=0, atol=tol)
        np.testing.assert_array_equal(Cv, Cv.T)
        np.testing.assert_allclose(np.diag(Cv), r.f_var[pa:pe], rtol=0, atol=tol)
        if Ns[t] == 0 and case.variant is vn.MEAN:           # the empty tile's mean is its c
            np.testing.assert_array_equal(r.f_mean[pa:pe], -0.7)


def cpu_tile(variant, seed, N, D, P=7):
    """A small tile for the CPU tests: X, y (on a level of 0.3 for the constant mean), v (every seventh entry exactly 0; None
    unless the variant reads one), Xs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 4.0, (N, D))
    signal = np.sin(X.sum(axis=1))
    y = (0.3 + signal if variant is vn.MEAN else signal) + 0.1 * rng.standard_normal(N)
    v = None
    if variant is vn.NOISE:
        v = rng.uniform(0.0, 0.3, N)
        v[::7] = 0.0
    return X, y, v, rng.uniform(0.0, 4.0, (P, D))


def same(a, e, what, fields=FIELDS):
    for name in fields:
        assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(e, name)).tobytes(), (what, name)


def one(b, t):
    """Tile t of a batch, packed alone, with its obs_var where the batch has one."""
    s = sharding.pack_subset(b, np.array([t]))
    out = dict(D=b["D"], kernel=b["kernel"], obs_off=s["obs_off"], pred_off=s["pred_off"], X=s["X"], y=s["y"], Xs=s["Xs"])
    if "obs_var" in b:
        out["obs_var"] = b["obs_var"][b["obs_off"][t]:b["obs_off"][t + 1]].copy()
    return out


# ---- the checks of the restatement that more than one variant has (CPU)
def check_gradient(variant, D):
    """The analytic gradient against central differences, to rtol 1e-7."""
    X, y, v, _ = cpu_tile(variant, 10 + D, 30, D)
    rng = np.random.default_rng(D)
    kernel = vn.RQ_KERNEL if variant is vn.RQ else KERNELS[D % 4]
    for x in {vn.RQ: ([1.7],), vn.MEAN: ([-0.7], [0.0], [2.5]), vn.NOISE: ([],)}[variant]:
        theta = np.concatenate([rng.uniform(0.8, 2.0, D), [0.9, 0.07], x])
        _, g = vn.nll_and_grad(variant, kernel, X, y, theta, v)
        fd = np.empty_like(g)
        for i in range(len(theta)):
            h = 1e-5 * (max(abs(theta[i]), 1.0) if variant is vn.MEAN else theta[i])         # c may be 0
            tp, tm = theta.copy(), theta.copy()
            tp[i] += h
            tm[i] -= h
            fd[i] = (vn.nll_and_grad(variant, kernel, X, y, tp, v, want_grad=False)[0]
                     - vn.nll_and_grad(variant, kernel, X, y, tm, v, want_grad=False)[0]) / (2 * h)
        np.testing.assert_allclose(g, fd, rtol=1e-7, atol=1e-7 * np.abs(g).max())
    if variant is vn.RQ:       # on the diagonal the covariance does not depend on alpha or the length scales
        K = vn.kernel_matrix(vn.RQ, kernel, X, X, theta)
        np.testing.assert_array_equal(np.diag(K), np.full(len(X), theta[D]))


def check_matches_sklearn(variant, kernel, D, seed, N, ell, s, sn2, alpha=None):
    """LML, predictive mean and variance of GaussianProcessRegressor(ConstantKernel(s) * k, alpha=sn2 [+ v], optimizer=None) --
    sklearn adds alpha to the diagonal of K -- to 1e-10; k is RationalQuadratic(l, alpha), RBF or Matern nu."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern, RationalQuadratic
    X, y, v, Xs = cpu_tile(variant, seed, N, D)
    if variant is vn.RQ:
        k, theta = RationalQuadratic(length_scale=ell, alpha=alpha), np.array([ell] * D + [s, sn2, alpha])
    else:
        k = RBF(length_scale=ell) if kernel == "RBF" else Matern(length_scale=ell, nu={"Matern12": 0.5, "Matern32": 1.5, "Matern52": 2.5}[kernel])
        theta = np.concatenate([ell, [s, sn2]])
    gp = GaussianProcessRegressor(ConstantKernel(s) * k, alpha=sn2 if v is None else sn2 + v, optimizer=None).fit(X, y)
    nll, _ = vn.nll_and_grad(variant, kernel, X, y, theta, v)
    f, fv, yv = vn.predict(variant, kernel, X, y, Xs, theta, v)
    mu, sd = gp.predict(Xs, return_std=True)
    print("lml", abs(-nll - gp.log_marginal_likelihood_value_), "mean", np.abs(f - mu).max(), "var", np.abs(fv - sd ** 2).max())
    assert abs(-nll - gp.log_marginal_likelihood_value_) < 1e-10
    np.testing.assert_allclose(f, mu, rtol=0, atol=1e-10)
    np.testing.assert_allclose(fv, sd ** 2, rtol=0, atol=1e-10)
    np.testing.assert_array_equal(yv, fv + sn2)           # a new point carries the homogeneous part only
    np.testing.assert_allclose(np.diag(vn.predict_cov(variant, kernel, X, y, Xs, theta, v)), fv, rtol=0, atol=1e-12)


def check_sklearn_fixture(golden_dir, variant):
    """tests/golden/kat_sklearn_rq.npz and kat_sklearn_noise.npz (tests/golden/make_rq_golden.py, make_noise_golden.py,
    scikit-learn only): the restatement at the stored optimum."""
    g = np.load(os.path.join(golden_dir, f"kat_sklearn_{variant.name}.npz"))
    m = np.load(os.path.join(golden_dir, "kat_sklearn_matern32.npz"))
    np.testing.assert_array_equal(g["x_train"], m["x_train"])
    np.testing.assert_array_equal(g["y_train"], m["y_train"])
    assert float(g["x_test"]) == float(m["x_test"]) and float(g["eps"]) ** 2 == pytest.approx(1e-4)
    X, y = g["x_train"][:, None], g["y_train"]
    if variant is vn.RQ:
        kernel, v, theta, free = vn.RQ_KERNEL, None, np.array([float(g["ls"]), 1.0, float(g["eps"]) ** 2, float(g["alpha"])]), [0, 3]
    else:
        kernel, v, theta, free = "Matern32", g["obs_var"], np.array([float(g["ls"]), 1.0, float(g["eps"]) ** 2]), [0]
        assert v.shape == (50,) and (v[::7] == 0.0).all() and (v >= 0).all() and v.max() > 0.04
    nll, grad = vn.nll_and_grad(variant, kernel, X, y, theta, v)
    f, fv, _ = vn.predict(variant, kernel, X, y, np.array([[float(g["x_test"])]]), theta, v)
    assert abs(-nll - float(g["ml"])) < 1e-8
    assert abs(f[0] - float(g["pred_mean"])) < 1e-8 and abs(fv[0] - float(g["pred_std"]) ** 2) < 1e-8
    # a stationary point of the objective in sklearn's log space: dNLL/dlog(theta) = theta dNLL/dtheta
    assert np.abs(grad[free] * theta[free]).max() < 1e-3
    if variant is vn.NOISE:
        assert abs(float(g["ls"]) - float(m["ls"])) > 1e-2    # and v matters: not the optimum of the fixture without it
