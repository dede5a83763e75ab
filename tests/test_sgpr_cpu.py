"""CPU: sparse GP experts (GPflowSGPRModel / HipSGPRModel) -- the numpy restatement's algebra, the model class, the C ABI
additions.  Nothing here needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sgpr_numpy as sn
from gpsat_amd import _lib as L
from gpsat_amd import models
from oracle import gp_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile(rng, N, M, D):
    X = rng.normal(size=(N, D))
    y = rng.normal(size=N)
    Z = X[rng.permutation(N)[:M]] + 0.05 * rng.normal(size=(M, D))
    return X, y, Z


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("D", [1, 2, 4])
def test_numpy_elbo_gradient_matches_central_differences(kid, D):
    rng = np.random.default_rng(10 * kid + D)
    X, y, Z = _tile(rng, 40, 12, D)
    th = np.concatenate([rng.uniform(0.6, 2.0, D), [1.3], [0.4]])
    g = sn.elbo_grad(kid, X, y, Z, th)
    fd = np.zeros_like(g)
    for i in range(len(th)):
        h = 1e-5 * th[i]
        tp, tm = th.copy(), th.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (sn.elbo(kid, X, y, Z, tp) - sn.elbo(kid, X, y, Z, tm)) / (2 * h)
    # central differences: truncation ~ h^2 |f'''|, rounding ~ eps |f| / h  (|f| ~ 1e2, h ~ 1e-5)
    assert np.max(np.abs(g - fd)) <= 1e-6 * max(1.0, np.max(np.abs(g)))


@pytest.mark.parametrize("kid", [0, 2, 3])
def test_inducing_points_at_the_data_give_the_exact_marginal_likelihood(kid):
    """Z = X: the bound is tight up to the jitter.  With Kuu = K + eps I, Qff = K (K + eps I)^-1 K = K - eps I + O(eps^2 /
    lambda_min), so the Gaussian term moves by about eps * tr(Sigma^-1) / 2 and the trace term by N eps / (2 sn2)."""
    rng = np.random.default_rng(kid)
    D, N = 2, 30
    X, y = rng.uniform(0, 4, (N, D)), rng.normal(size=N)
    th = np.array([0.9, 1.2, 1.5, 0.3])
    nll, _ = go.nll_and_grad(kid, X, y, th)
    el = sn.elbo(kid, X, y, X, th)
    K = go.kernel_matrix(kid, X, X, th[:D], th[D])
    lam_min = np.linalg.eigvalsh(K)[0]
    eps, sn2 = sn.JITTER, th[-1]
    bound = eps * N / sn2 + eps * N / (2 * sn2) + eps ** 2 / max(lam_min, eps) * N / sn2 ** 2 + 1e-10 * abs(nll)
    assert abs(el - (-nll)) <= bound, (el, -nll, bound)
    assert el <= -nll + 1e-12 * abs(nll)        # the ELBO is a lower bound


def test_registry_resolves_the_sparse_names():
    assert models.get_model("GPflowSGPRModel") is models.HipSGPRModel
    assert models.get_model("HipSGPRModel") is models.HipSGPRModel
    assert models.get_model("GPflowGPRModel") is models.HipGPRModel
    with pytest.raises(NotImplementedError):
        models.get_model("GPflowSVGPModel")


def test_inducing_point_selection():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(50, 2))
    # N <= M: every coordinate, in order
    np.testing.assert_array_equal(models.select_inducing_points(X, 50), X)
    np.testing.assert_array_equal(models.select_inducing_points(X, 500), X)
    # N > M: a seeded subset of rows, the same every time, different across experts / seeds
    a = models.select_inducing_points(X, 10, seed=0, expert_index=7)
    b = models.select_inducing_points(X, 10, seed=0, expert_index=7)
    np.testing.assert_array_equal(a, b)
    rows = np.random.default_rng([0, 7]).permutation(50)[:10]
    np.testing.assert_array_equal(a, X[rows])
    assert not np.array_equal(a, models.select_inducing_points(X, 10, seed=0, expert_index=8))
    assert not np.array_equal(a, models.select_inducing_points(X, 10, seed=1, expert_index=7))
    assert len({tuple(r) for r in a}) == 10          # rows without replacement


class _StubEngine:
    device_name = "stub"


def _model(**kw):
    rng = np.random.default_rng(0)
    return models.HipSGPRModel(coords=rng.normal(size=(30, 2)), obs=rng.normal(size=30), engine=_StubEngine(),
                               num_inducing_points=10, **kw)


def test_model_interface_without_device():
    m = _model()
    assert m.param_names == ["lengthscales", "kernel_variance", "likelihood_variance", "inducing_points"]
    Z = m.get_inducing_points()
    assert Z.shape == (10, 2)
    np.testing.assert_array_equal(Z, models.select_inducing_points(m.coords, 10, 0, 0))
    m.set_inducing_points(Z[:4] * 2)
    np.testing.assert_array_equal(m.get_inducing_points(), Z[:4] * 2)
    assert m.dtype == "f64"
    # scaled coordinates: inducing points live in the model's frame
    m2 = models.HipSGPRModel(coords=m.coords * 10, obs=m.obs[:, 0], coords_scale=10, engine=_StubEngine(),
                             num_inducing_points=10)
    np.testing.assert_allclose(m2.get_inducing_points(), Z)


def test_not_implemented_cases():
    with pytest.raises(NotImplementedError):
        _model(dtype="f32")
    m = _model()
    with pytest.raises(NotImplementedError):
        m.optimise_parameters(train_inducing_points=True)
    with pytest.raises(NotImplementedError):
        m.predict(np.zeros((2, 2)), full_cov=True)


def test_sparse_struct_layout_matches_c(tmp_path):
    fields = [f[0] for f in L.GpsatSparse._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gpsat_hip.h"', 'int main(){',
            'printf("%zu\\n", sizeof(gpsat_sparse));']
    prog += [f'printf("%zu\\n", offsetof(gpsat_sparse, {f}));' for f in fields]
    prog.append('printf("%d\\n", GPSAT_ABI_VERSION); return 0;}')
    cfile = tmp_path / "sparse.c"
    cfile.write_text("\n".join(prog))
    exe = tmp_path / "sparse"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.GpsatSparse)
    for f, off in zip(fields, vals[1:-1]):
        assert getattr(L.GpsatSparse, f).offset == off, f
    assert vals[-1] == L.ABI_VERSION == 4


def test_max_inducing_table_is_pinned():
    lib = L.load()
    assert tuple(lib.gpsat_max_inducing(1, D) for D in range(1, 5)) == (1024, 1024, 1024, 1024)
    assert tuple(lib.gpsat_max_inducing(0, D) for D in range(1, 5)) == (0, 0, 0, 0)
    for D in (0, 5):
        assert lib.gpsat_max_inducing(1, D) == 0
    assert L.max_inducing("f64", 3) == 1024 and L.max_inducing("f32", 3) == 0

