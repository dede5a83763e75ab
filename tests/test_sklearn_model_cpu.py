"""HipSklearnGPRModel host logic against real sklearn (no GPU): parameter mapping, bounds, the no-op constraints, the
objective sign rule, the restart draws, the registry and the C layout of gpsat_multistart."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, Matern
from sklearn.utils import check_random_state

from gpsat_amd import _lib as L
from gpsat_amd.models import HipSklearnGPRModel, get_model, sklearn_restart_starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _SklearnEngine:
    """CPU stand-in for the engine: evaluates -LML at theta0 with sklearn (optimiser 'none' only)."""
    device_name = "cpu"

    def __init__(self):
        self.calls = []

    def fit_predict_batch(self, *, D, X, y, theta0, kernel, optimiser, n_starts=0, **kw):
        self.calls.append(dict(optimiser=optimiser, n_starts=n_starts, theta0=np.array(theta0), **kw))
        assert optimiser == "none"
        th = np.asarray(theta0)[0]
        base = RBF(th[:D]) if kernel == "RBF" else Matern(th[:D], nu={"Matern12": 0.5, "Matern32": 1.5, "Matern52": 2.5}[kernel])
        gp = GaussianProcessRegressor(base * ConstantKernel(th[D]), alpha=th[D + 1], optimizer=None).fit(X, y)

        class R:
            nll = np.array([-gp.log_marginal_likelihood_value_])
            status = np.array([5])
        return R()


def _data(N=30, D=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(N, D))
    return X, np.sin(6 * X[:, 0]) + 0.1 * rng.normal(size=N)


def _ref_gpr(D, kernel_variance=1.0, alpha=1.0, nu=1.5):
    k = Matern(length_scale=np.ones(D), nu=nu)
    if kernel_variance is not None:
        k *= ConstantKernel(np.sqrt(kernel_variance))
    return GaussianProcessRegressor(kernel=k, alpha=alpha, n_restarts_optimizer=2)


def test_registry_resolves_the_sklearn_names():
    assert get_model("sklearnGPRModel") is HipSklearnGPRModel
    assert get_model("HipSklearnGPRModel") is HipSklearnGPRModel


def test_parameter_mapping_matches_sklearn():
    X, y = _data()
    m = HipSklearnGPRModel(coords=X, obs=y, engine=_SklearnEngine(), kernel_variance=2.5, likelihood_variance=0.3)
    gp = _ref_gpr(2, kernel_variance=2.5, alpha=0.3)
    # sklearn's theta (log space) is [log l_1 .. log l_D, log c]: the trainable entries of the device vector
    np.testing.assert_allclose(np.log(m._theta[m._trainable]), gp.kernel.theta, rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.log(np.c_[m._lo, m._hi][m._trainable]), gp.kernel.bounds, rtol=0, atol=1e-15)
    assert m.kernel == "Matern32" and m.dtype == "f64"
    assert m.get_kernel_variance() == pytest.approx(2.5)          # c^2, the device sees sf2 = c
    assert m._theta[2] == pytest.approx(np.sqrt(2.5))
    assert m.get_likelihood_variance() == 0.3 and not m._trainable[3]
    m.set_kernel_variance(4.0)
    assert m._theta[2] == pytest.approx(2.0) and m.get_kernel_variance() == pytest.approx(4.0)
    # no constant term: sf2 = 1, not trained, reported as 1
    m0 = HipSklearnGPRModel(coords=X, obs=y, engine=_SklearnEngine(), kernel_variance=None)
    assert m0.get_kernel_variance() == 1.0 and not m0._trainable[2] and m0._theta[2] == 1.0
    m0.set_kernel_variance(7.0)
    assert m0.get_kernel_variance() == 1.0
    assert m0.get_likelihood_variance() == 1.0                    # alpha defaults to 1
    np.testing.assert_allclose(np.log(m0._theta[m0._trainable]), _ref_gpr(2, None).kernel.theta)


def test_kernels_and_refusals():
    X, y = _data(D=3)
    e = _SklearnEngine()
    for nu, name in ((0.5, "Matern12"), (1.5, "Matern32"), (2.5, "Matern52"), (np.inf, "RBF")):
        assert HipSklearnGPRModel(coords=X, obs=y, engine=e, kernel_kwargs={"nu": nu}).kernel == name
    assert HipSklearnGPRModel(coords=X, obs=y, engine=e, kernel="RBF").kernel == "RBF"
    with pytest.raises(NotImplementedError):
        HipSklearnGPRModel(coords=X, obs=y, engine=e, kernel_kwargs={"nu": 1.0})
    with pytest.raises(NotImplementedError):
        HipSklearnGPRModel(coords=X, obs=y, engine=e, kernel="RationalQuadratic")
    with pytest.raises(NotImplementedError):
        HipSklearnGPRModel(coords=X, obs=y, engine=e, kernel_kwargs={"length_scale": 1.0})
    with pytest.raises(NotImplementedError):
        HipSklearnGPRModel(coords=X, obs=y, engine=e, mean_value=1.0)
    with pytest.raises(AttributeError):
        HipSklearnGPRModel(coords=X, obs=y, engine=e, param_bounds={"k1__length_scale": (1e-3, 1e3)})
    with pytest.raises(NotImplementedError):
        get_model("SVGP")


def test_constraints_lengthscale_bounds_and_no_ops():
    X, y = _data()
    m = HipSklearnGPRModel(coords=X, obs=y, engine=_SklearnEngine(), coords_scale=[2.0, 4.0])
    m.set_lengthscales_constraints([0.1, 0.2], [1.0, 2.0], scale=True)
    np.testing.assert_allclose(m._lo[:2], [0.05, 0.05])
    np.testing.assert_allclose(m._hi[:2], [0.5, 0.5])
    # move_within_tol edits a copy in the reference: the length scales (1, 1) stay outside the new box
    np.testing.assert_allclose(m.get_lengthscales(), [1.0, 1.0])
    before = (m._theta.copy(), m._lo.copy(), m._hi.copy())
    m.set_kernel_variance_constraints(0.5, 0.6)
    m.set_likelihood_variance_constraints(0.5, 0.6)
    for a, b in zip(before, (m._theta, m._lo, m._hi)):
        np.testing.assert_array_equal(a, b)
    # sklearn itself: the kernel_variance constraint of the reference does not reach kernel.bounds
    gp = _ref_gpr(2)
    b0 = gp.kernel.bounds.copy()
    gp.kernel.constant_value_bounds = (0.5, 0.6)
    np.testing.assert_array_equal(gp.kernel.bounds, b0)


def test_objective_sign_rule_without_fit():
    X, y = _data()
    e = _SklearnEngine()
    m = HipSklearnGPRModel(coords=X, obs=y, engine=e, likelihood_variance=0.1)
    gp = GaussianProcessRegressor(_ref_gpr(2).kernel, alpha=0.1, optimizer=None).fit(X, y[:, None])
    # without a fit: -LML at the current parameters (the reference's _fake_fit branch)
    assert m.get_objective_function_value() == pytest.approx(-gp.log_marginal_likelihood_value_, rel=1e-12)
    assert e.calls[-1]["n_starts"] == 1
    # after a fit: +LML of the fit
    m._lml = 12.5
    assert m.get_objective_function_value() == 12.5


@pytest.mark.parametrize("random_state", [0, 7, "rs", None])
def test_restart_starts_equal_sklearn_draws(random_state):
    X, y = _data(D=2)
    e = _SklearnEngine()
    if random_state == "rs":
        mine, theirs = np.random.RandomState(3), np.random.RandomState(3)
    elif random_state is None:
        mine = theirs = None
    else:
        mine = theirs = random_state
    m = HipSklearnGPRModel(coords=X, obs=y, engine=e, random_state=mine, n_restarts_optimizer=3)
    if random_state is None:
        np.random.seed(11)
    got = m.restart_starts()
    # what GaussianProcessRegressor.fit draws: check_random_state(random_state).uniform(bounds[:, 0], bounds[:, 1])
    if random_state is None:
        np.random.seed(11)
    rng = check_random_state(theirs)
    bounds = _ref_gpr(2).kernel.bounds
    want = np.array([rng.uniform(bounds[:, 0], bounds[:, 1]) for _ in range(3)])
    np.testing.assert_array_equal(np.log(got[:, m._trainable]), np.log(np.exp(want)))
    np.testing.assert_array_equal(got[:, 3], m.get_likelihood_variance())
    assert sklearn_restart_starts(np.random.RandomState(0), [0.0], [1.0], 2).shape == (2, 1)


def test_multistart_struct_layout_matches_c(tmp_path):
    fields = [f[0] for f in L.GpsatMultistart._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gpsat_hip.h"', 'int main(){',
            'printf("%zu\\n", sizeof(gpsat_multistart));']
    prog += [f'printf("%zu\\n", offsetof(gpsat_multistart, {f}));' for f in fields]
    prog.append('printf("%d %d\\n", GPSAT_TRANSFORM_LOG, GPSAT_ABI_VERSION); return 0;}')
    cfile = tmp_path / "ms.c"
    cfile.write_text("\n".join(prog))
    exe = tmp_path / "ms"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.GpsatMultistart)
    for f, off in zip(fields, vals[1:-2]):
        assert getattr(L.GpsatMultistart, f).offset == off, f
    assert vals[-2] == L.TRANSFORM_LOG and vals[-1] == L.ABI_VERSION == 4


def test_new_symbol_is_exported():
    lib = L.load()
    assert hasattr(lib, "gpsat_fit_predict_batch_ms")
    assert "gpsat_fit_predict_batch_ms" in L.OPTIONAL_EXPORTS
