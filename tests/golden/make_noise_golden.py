"""Writes tests/golden/kat_sklearn_noise.npz with scikit-learn alone: the twin of the reference's sklearn known-answer fixture
(kat_sklearn_matern32.npz, tests/test_localexperts.py:22-49 of the reference) with a known noise variance per observation.

The 50 training points and the test point of that fixture; v ~ U(0, 0.05) per point with every seventh entry exactly 0
(seed 17, stored); GaussianProcessRegressor(ConstantKernel(1, fixed) * Matern(nu=1.5), alpha=eps^2 + v) fitted from
length_scale = 1 by sklearn's own L-BFGS-B.  sklearn adds alpha to the diagonal of K: alpha_i = sn2 + v_i is the model
y ~ N(0, K + sn2 I + diag(v)).  Stored: v, the fitted length scale, the log marginal likelihood there, and the predictive mean
and standard deviation (of f*) at x_test.

    python tests/golden/make_noise_golden.py
"""
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, Matern

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    m = np.load(os.path.join(HERE, "kat_sklearn_matern32.npz"))
    x, y, eps, x_test = m["x_train"], m["y_train"], float(m["eps"]), float(m["x_test"])
    v = np.random.default_rng(17).uniform(0.0, 0.05, len(x))
    v[::7] = 0.0
    kernel = ConstantKernel(1.0, constant_value_bounds="fixed") * Matern(length_scale=1.0, nu=1.5)
    gp = GaussianProcessRegressor(kernel=kernel, alpha=eps ** 2 + v).fit(x[:, None], y)
    mean, std = gp.predict(np.array([[x_test]]), return_std=True)
    np.savez(os.path.join(HERE, "kat_sklearn_noise.npz"), x_train=x, y_train=y, eps=eps, x_test=x_test, obs_var=v,
             ls=gp.kernel_.k2.length_scale, ml=gp.log_marginal_likelihood_value_, pred_mean=mean[0], pred_std=std[0])
    print("length_scale", gp.kernel_.k2.length_scale, "lml", gp.log_marginal_likelihood_value_, "mean", mean[0], "std", std[0])


if __name__ == "__main__":
    main()
