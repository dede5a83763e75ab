"""Writes tests/golden/kat_sklearn_rq.npz with scikit-learn alone: the RationalQuadratic twin of the reference's sklearn
known-answer fixture (kat_sklearn_matern32.npz, tests/test_localexperts.py:22-49 of the reference).

The 50 training points, the noise level and the test point of that fixture; GaussianProcessRegressor(ConstantKernel(1,
fixed) * RationalQuadratic, alpha=eps^2 = 1e-4) fitted from length_scale = alpha = 1 by sklearn's own L-BFGS-B.  Stored: the
fitted length scale and alpha, the log marginal likelihood there, and the predictive mean and standard deviation at x_test.

    python tests/golden/make_rq_golden.py
"""
import os

import numpy as np
from sklearn.gaussian_process import GaussianProcessRegressor
from sklearn.gaussian_process.kernels import ConstantKernel, RationalQuadratic

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    m = np.load(os.path.join(HERE, "kat_sklearn_matern32.npz"))
    x, y, eps, x_test = m["x_train"], m["y_train"], float(m["eps"]), float(m["x_test"])
    kernel = ConstantKernel(1.0, constant_value_bounds="fixed") * RationalQuadratic(length_scale=1.0, alpha=1.0)
    gp = GaussianProcessRegressor(kernel=kernel, alpha=eps ** 2).fit(x[:, None], y)
    mean, std = gp.predict(np.array([[x_test]]), return_std=True)
    np.savez(os.path.join(HERE, "kat_sklearn_rq.npz"), x_train=x, y_train=y, eps=eps, x_test=x_test,
             ls=gp.kernel_.k2.length_scale, alpha=gp.kernel_.k2.alpha, ml=gp.log_marginal_likelihood_value_,
             pred_mean=mean[0], pred_std=std[0])
    print("length_scale", gp.kernel_.k2.length_scale, "alpha", gp.kernel_.k2.alpha, "lml", gp.log_marginal_likelihood_value_,
          "mean", mean[0], "std", std[0])


if __name__ == "__main__":
    main()
