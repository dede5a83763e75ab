"""Cost of the held-out phase (gpsat_fit_predict_batch_cv) on the fp64 tile kernel.

Batch: T tiles x N observations, D = 3, RBF, fp64, optimiser "none", no prediction points.  Kernel time (the C ABI's own
events around the launch, gpsat_last_timing) of: the plain call, leave-one-out, contiguous folds of G rows, the same labels
shuffled inside every tile -- and, for scale, one evaluation with the gradient.  Prints one JSON line.

    python scripts/cv_bench.py [--tiles 4096] [--obs 500] [--fold 25] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpsat_amd import synthetic as syn          # noqa: E402
from gpsat_amd.engine import Engine             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--obs", type=int, default=500)
    ap.add_argument("--fold", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    T, N, D = a.tiles, a.obs, 3
    # 64 distinct tiles, repeated: the kernel's time does not depend on the values
    base = [syn.make_tile(1000 + t, N, 0, D, 0) for t in range(min(T, 64))]
    tiles = [base[t % len(base)] for t in range(T)]
    X = np.concatenate([t[0] for t in tiles])
    y = np.concatenate([t[1] for t in tiles])
    theta = np.array([t[3] for t in tiles])
    off = np.arange(T + 1, dtype=np.int64) * N
    rng = np.random.default_rng(0)
    runs = np.tile(np.arange(N, dtype=np.int32) // a.fold, T)
    shuffled = np.concatenate([rng.permutation(runs[:N]) for _ in range(T)]).astype(np.int32)
    eng = Engine(0)
    kw = dict(D=D, obs_off=off, X=X, y=y, pred_off=np.zeros(T + 1, dtype=np.int64), Xs=np.zeros((0, D)), theta0=theta,
              kernel="RBF", optimiser="none", dtype="f64")
    cases = {"plain": {}, "loo": {"cv_fold": "loo"}, f"runs_of_{a.fold}": {"cv_fold": runs},
             f"shuffled_{a.fold}": {"cv_fold": shuffled}, "plain_with_gradient": {"want_grad": True}}
    out = {"tiles": T, "obs": N, "D": D, "kernel": "RBF", "dtype": "f64", "device": eng.device_name, "reps": a.reps, "kernel_ms": {}}
    for name, extra in cases.items():
        eng.fit_predict_batch(**kw, **extra)                       # warm-up: buffers, code objects
        ms = [eng.fit_predict_batch(**kw, **extra).kernel_ms for _ in range(a.reps)]
        out["kernel_ms"][name] = {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
