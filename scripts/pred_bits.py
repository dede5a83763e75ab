"""The bits of the prediction phase of the fp64 tile kernel: one SHA-256 per output array of a fixed, seeded set of small
batches, to compare two builds of the library (run it on each and diff the listings; GPSAT_LIB picks the library).

What predict_tile, predict_grad_tile and predict_hess_tile share is one panelled triangular solve over pairs of 16-column
chunks of prediction points; the batches are the smallest at which it takes each of its paths, not a workload's:
  N in {0, 1, 16, 64, 65, 80, 130}: the prior without a solve; one panel of up to 4 block rows; a second panel with the
      pipelined k loop; a tail panel of one and of two block rows;
  P in {1, 17, 272}: an empty second chunk; a ragged second chunk; a second round of chunk pairs for a wave of either build;
every (N, P) is a tile of one batch, for D in {1, 3, 4}, RBF, Matern32 (no second derivatives) and Matern52, on the 4-wave
and the 8-wave build (Engine(0) and Engine(0, workgroups_per_cu=1), as the tests choose them), for the calls plain, full_cov,
pred_grad, pred_hess with the Laplacian, and both together -- optimiser "none" at a drawn theta0, and once a short L-BFGS
run.  One batch each at N = 80, P = 17 for the mean, noise, cv and RQ variants, which compile the plain prediction too, and
one tile of 1601 observations run by a team of two workgroups with the full covariance (tests/test_gpu_team.py's size).

    python scripts/pred_bits.py > listing.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["GPSAT_DEVELOPER"] = "1"             # GPSAT_DEBUG_TEAM below is read in developer mode only

from gpsat_amd import synthetic as syn          # noqa: E402
from gpsat_amd.engine import Engine             # noqa: E402

FIELDS = ("theta", "nll", "grad", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var", "f_cov", "f_grad", "f_grad_var",
          "f_hess", "f_hess_var", "f_lap", "f_lap_var", "cv_mean", "cv_f_var", "cv_y_var")
KID = {"RBF": 0, "Matern32": 2, "Matern52": 3}
NS, PS = (0, 1, 16, 64, 65, 80, 130), (1, 17, 272)
CALLS = {"plain": {}, "full_cov": {"full_cov": True}, "grad": {"pred_grad": True}, "hess": {"pred_hess": True},
         "grad_hess": {"pred_grad": True, "pred_hess": True}}


def listing(name, r):
    for f in FIELDS:
        v = getattr(r, f)
        if v is not None:
            assert np.isfinite(np.asarray(v)).all(), f"{name}.{f}: not finite (NaN would compare equal across builds)"
            print(f"{name}.{f} {hashlib.sha256(np.ascontiguousarray(np.asarray(v)).tobytes()).hexdigest()}")


def theta0(rng, T, D, last=None):
    cols = [rng.uniform(1.5, 6.0, (T, D)), rng.uniform(0.05, 1.0, T), rng.uniform(0.01, 0.5, T)]
    return np.column_stack(cols + ([] if last is None else [np.full(T, last)]))


def batch(Ns, Ps, D, kid, seed):
    b = syn.make_batch(len(Ns), Ns, Ps, D, kid, base_seed=seed, dtype=np.float64)
    return dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], dtype="f64"), b


def main():
    engines = {"w4": Engine(0), "w8": Engine(0, workgroups_per_cu=1)}
    Ns, Ps = [n for n in NS for _ in PS], [p for _ in NS for p in PS]
    T = len(Ns)
    for D in (1, 3, 4):
        for kernel, kid in KID.items():
            kw, _ = batch(Ns, Ps, D, kid, 1000 * D + kid)
            th = theta0(np.random.default_rng(D + 10 * kid), T, D)
            for call, more in CALLS.items():
                if kernel == "Matern32" and "pred_hess" in more:
                    continue
                for en, eng in engines.items():
                    listing(f"{en}.D{D}.{kernel}.{call}", eng.fit_predict_batch(theta0=th, kernel=kernel, optimiser="none", **kw, **more))
    # a short optimised run: the prediction at a theta the kernel found
    kw, _ = batch(Ns, Ps, 3, 3, 77)
    lo, hi = syn.default_bounds(T, 3)
    for call in ("plain", "grad_hess"):
        for en, eng in engines.items():
            listing(f"{en}.lbfgs.{call}", eng.fit_predict_batch(theta0=np.ones((T, 5)), lo=lo, hi=hi, kernel="Matern52", optimiser="lbfgs",
                                                                 max_iter=5, **kw, **CALLS[call]))
    # the other variants of the table, which compile predict_tile too
    kw, b = batch([80, 80], [17, 17], 3, 0, 5)
    rng = np.random.default_rng(6)
    th = theta0(rng, 2, 3)
    variants = {"mean": dict(theta0=theta0(rng, 2, 3, 0.3), kernel="Matern52", mean="constant"),
                "noise": dict(theta0=th, kernel="Matern52", obs_var=rng.uniform(0.0, 0.3, 160)),
                "cv": dict(theta0=th, kernel="Matern52", cv_fold="loo"),
                "rq": dict(theta0=theta0(rng, 2, 3, 1.5), kernel="RationalQuadratic")}
    for vname, more in variants.items():
        for en, eng in engines.items():
            listing(f"{en}.{vname}", eng.fit_predict_batch(optimiser="none", **kw, **more))
    # a team of two workgroups on one large tile, with the full covariance
    kw, _ = batch([1601], [60], 3, 3, 11)
    os.environ["GPSAT_DEBUG_TEAM"] = "2"
    try:
        listing("team2", engines["w4"].fit_predict_batch(theta0=np.full((1, 5), 1.5), kernel="Matern52", optimiser="none",
                                                         full_cov=True, **kw))
    finally:
        os.environ.pop("GPSAT_DEBUG_TEAM", None)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
