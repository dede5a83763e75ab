"""Cost of the RationalQuadratic covariance function on the fp64 tile kernel, beside Matern32 in the same process.

Batch: T tiles x N observations, D = 3, fp64, L-BFGS with max_iter 20 from theta0 = 1 with the default length-scale box
(RationalQuadratic: alpha in [0.1, 20]), no prediction points.  The same tiles for both kernels.  Kernel time (the C ABI's own
events around the launch, gpsat_last_timing): the median of ``--reps`` launches after one warm-up launch each.  Both kernels
run one workgroup per tile at these sizes, from the same build (4-wave) and the same time-sliced queue; RationalQuadratic has
one more hyper-parameter, so the two fits do not run the same number of evaluations: the time per evaluation is printed too.
Prints one JSON line.

    python scripts/rq_bench.py [--tiles 4096] [--obs 500] [--reps 5] [--max-iter 20]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    a = ap.parse_args()
    T, N, D = a.tiles, a.obs, 3
    b = syn.make_batch(T, N, 0, D, 2, base_seed=42, dtype=np.float64)
    lo, hi = syn.default_bounds(T, D)
    eng = Engine(0)
    out = {"tiles": T, "obs": N, "D": D, "dtype": "f64", "max_iter": a.max_iter, "reps": a.reps, "device": eng.device_name,
           "cases": {}}
    cases = {"Matern32": (np.ones((T, D + 2)), lo, hi),
             "RationalQuadratic": (np.ones((T, D + 3)), np.column_stack([lo, np.full(T, 0.1)]), np.column_stack([hi, np.full(T, 20.0)]))}
    for kernel, (th0, lo_k, hi_k) in cases.items():
        kw = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=th0, lo=lo_k, hi=hi_k,
                  kernel=kernel, optimiser="lbfgs", max_iter=a.max_iter, dtype="f64")
        eng.fit_predict_batch(**kw)                                   # warm-up
        ms, r = [], None
        for _ in range(a.reps):
            r = eng.fit_predict_batch(**kw)
            ms.append(r.kernel_ms)
        n_eval = int(r.n_eval.sum())
        out["cases"][kernel] = {"kernel_ms": round(float(np.median(ms)), 3), "kernel_ms_all": [round(m, 3) for m in ms],
                                "evaluations": n_eval, "us_per_evaluation": round(float(np.median(ms)) * 1e3 / max(n_eval, 1), 4),
                                "status_ok": float((r.status <= 1).mean())}
    m32, rq = out["cases"]["Matern32"], out["cases"]["RationalQuadratic"]
    out["ratio_kernel_ms"] = round(rq["kernel_ms"] / m32["kernel_ms"], 4)
    out["ratio_per_evaluation"] = round(rq["us_per_evaluation"] / m32["us_per_evaluation"], 4)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
