"""Throughput of the sparse GP experts (gpsat_sgpr_fit_predict_batch): tiles/s and the fraction of the fp64 MFMA peak.

Flop model, counted from the algorithm (not from the instructions issued), per evaluation of a tile with N rows, M
inducing points and input dimension D; G = D + 1 with the gradient (L-BFGS), G = 1 without (objective + predict only):
  pass over the rows   2 G N M^2             Phi = Kuf Kuf^T and, with the gradient, Psi_d = dKuf_d Kuf^T (MFMA)
                       + 2 G N M             b, e_d
  M x M algebra        objective: (1/3 + 1/3 + 2 + 1/3 + 1/3) M^3 = 3.33 M^3
                       chol Kuu, L^-1, P = L^-1 Phi L^-T, chol B, Q = LB^-1 L^-1
                       gradient adds (1 + 1 + 2 + 2) M^3 = 6 M^3: Kuu^-1, S^-1, Phi Kuu^-1, R Phi Kuu^-1
The kernel evaluations (exp, sqrt) are not counted.  flop / s over the kernel time is compared with the fp64 matrix peak of
the MI355X (78.6 TFLOP/s, datasheet).  Without --full, only shape 1 is run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from gpsat_amd.engine import Engine

PEAK_F64 = 78.6e12


def flops_per_eval(N, M, D, grad):
    G = D + 1 if grad else 1
    return 2 * G * N * M * M + 2 * G * N * M + (9.33 if grad else 3.33) * M ** 3


def run(eng, T, N, M, D, kernel, max_iter, seed=0):
    rng = np.random.default_rng(seed)
    side = 10.0
    X = rng.uniform(0, side, (T * N, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=T * N)
    Z = np.concatenate([X[t * N + rng.permutation(N)[:M]] for t in range(T)])
    P = 16
    Xs = rng.uniform(0, side, (T * P, D))
    off = lambda n: np.arange(T + 1, dtype=np.int64) * n
    t0 = time.perf_counter()
    r = eng.sgpr_fit_predict_batch(D=D, obs_off=off(N), X=X, y=y, pred_off=off(P), Xs=Xs, z_off=off(M), Z=Z,
                                   theta0=np.ones(D + 2), kernel=kernel, optimiser="lbfgs" if max_iter else "none",
                                   max_iter=max_iter)
    wall = time.perf_counter() - t0
    n_eval = int(np.sum(np.maximum(r.n_eval, 1)))
    fl = n_eval * flops_per_eval(N, M, D, grad=max_iter > 0)
    k_s = r.kernel_ms / 1e3
    return dict(T=T, N=N, M=M, D=D, kernel=kernel, max_iter=max_iter, kernel_s=round(k_s, 3), wall_s=round(wall, 3),
                tiles_per_s=round(T / k_s, 2), evals=n_eval, evals_per_tile=round(n_eval / T, 2),
                tflops=round(fl / k_s / 1e12, 3), frac_fp64_peak=round(fl / k_s / PEAK_F64, 4),
                status=np.bincount(r.status, minlength=7).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="also run shape 2 (256 tiles x N 100 000 x M 500)")
    ap.add_argument("--max-iter2", type=int, default=2, help="L-BFGS iterations of shape 2 (0 = objective + predict only)")
    a = ap.parse_args()
    eng = Engine(0)
    print(json.dumps(dict(shape=1, **run(eng, 1024, 8192, 256, 3, "Matern32", 20))), flush=True)
    if a.full:
        print(json.dumps(dict(shape=2, **run(eng, 256, 100_000, 500, 3, "Matern32", a.max_iter2, seed=1))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
