"""Cost of the trainable constant mean on the fp64 tile kernel, beside the zero-mean build in the same process.

Batch: T tiles x N observations, D = 3, Matern32, fp64, L-BFGS with max_iter 20 from theta0 = 1 (c0 = 0) with the default
length-scale box, no prediction points.  The same tiles for both: the zero-mean build (gpsat_fit_predict_batch) fits the
de-meaned y, the mean build (gpsat_fit_predict_batch_mean) fits y + 0.3 with c unconstrained.  Kernel time (the C ABI's own
events around the launch, gpsat_last_timing): the median of ``--reps`` launches per build after one warm-up launch each, the
two builds taking turns.  Both run one workgroup per tile at these sizes, from the build of the same wave count (4-wave) and
the same time-sliced queue; the mean has one more hyper-parameter, so the two fits do not run the same number of
evaluations: evaluations per tile and the time per evaluation are printed too.  Prints one JSON line.

    python scripts/mean_bench.py [--tiles 4096] [--obs 500] [--reps 5] [--max-iter 20]
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
    nan = np.full(T, np.nan)
    eng = Engine(0)
    out = {"tiles": T, "obs": N, "D": D, "kernel": "Matern32", "dtype": "f64", "max_iter": a.max_iter, "reps": a.reps,
           "device": eng.device_name, "cases": {}}
    th_mean = np.ones((T, D + 3))
    th_mean[:, D + 2] = 0.0
    cases = {"zero_mean": dict(y=b["y"], theta0=np.ones((T, D + 2)), lo=lo, hi=hi),
             "constant_mean": dict(y=b["y"] + 0.3, theta0=th_mean, lo=np.column_stack([lo, nan]), hi=np.column_stack([hi, nan]),
                                   mean="constant")}
    common = dict(D=D, obs_off=b["obs_off"], X=b["X"], pred_off=b["pred_off"], Xs=b["Xs"], kernel="Matern32", optimiser="lbfgs",
                  max_iter=a.max_iter, dtype="f64")
    ms, last = {k: [] for k in cases}, {}
    for k, kw in cases.items():
        eng.fit_predict_batch(**common, **kw)                         # warm-up
    for _ in range(a.reps):
        for k, kw in cases.items():
            last[k] = eng.fit_predict_batch(**common, **kw)
            ms[k].append(last[k].kernel_ms)
    for k, r in last.items():
        n_eval, med = int(r.n_eval.sum()), float(np.median(ms[k]))
        out["cases"][k] = {"kernel_ms": round(med, 3), "kernel_ms_all": [round(m, 3) for m in ms[k]], "evaluations": n_eval,
                           "evaluations_per_tile": round(n_eval / T, 3), "us_per_evaluation": round(med * 1e3 / max(n_eval, 1), 4),
                           "status_ok": float((r.status <= 1).mean())}
    z, c = out["cases"]["zero_mean"], out["cases"]["constant_mean"]
    out["ratio_kernel_ms"] = round(c["kernel_ms"] / z["kernel_ms"], 4)
    out["ratio_per_evaluation"] = round(c["us_per_evaluation"] / z["us_per_evaluation"], 4)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
