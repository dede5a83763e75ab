"""Cost of the noise variances per observation on the fp64 tile kernel, beside the plain build in the same process.

Batch: T tiles x N observations, D = 3, Matern32, fp64, L-BFGS with max_iter 20 from theta0 = 1 with the default
length-scale box, no prediction points.  The same tiles for both: the plain build (gpsat_fit_predict_batch) and the noise
build (gpsat_fit_predict_batch_noise) with obs_var = 0 everywhere, which returns the plain call's bits -- so both run the
same evaluations, and the ratio of the kernel times is the cost of the kernel's own change: one predicated load per diagonal
element of every K build.  Kernel time (the C ABI's own events around the launch, gpsat_last_timing): the median of
``--reps`` launches per build after one warm-up launch each, the two builds taking turns.  Both run one workgroup per tile
from the build of the same wave count (4-wave at these sizes) and the same time-sliced queue.  Prints one JSON line.

    python scripts/noise_bench.py [--tiles 4096] [--obs 500] [--reps 5] [--max-iter 20]
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
    out = {"tiles": T, "obs": N, "D": D, "kernel": "Matern32", "dtype": "f64", "max_iter": a.max_iter, "reps": a.reps,
           "device": eng.device_name, "cases": {}}
    cases = {"plain": {}, "noise_v0": {"obs_var": np.zeros(T * N)}}
    common = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=np.ones((T, D + 2)),
                  lo=lo, hi=hi, kernel="Matern32", optimiser="lbfgs", max_iter=a.max_iter, dtype="f64")
    ms, last = {k: [] for k in cases}, {}
    for k, kw in cases.items():
        eng.fit_predict_batch(**common, **kw)                         # warm-up
    for _ in range(a.reps):
        for k, kw in cases.items():
            last[k] = eng.fit_predict_batch(**common, **kw)
            ms[k].append(last[k].kernel_ms)
    for k, r in last.items():
        n_eval, med = int(r.n_eval.sum()), float(np.median(ms[k]))
        out["cases"][k] = {"kernel_ms": round(med, 3), "kernel_ms_min": round(min(ms[k]), 3), "kernel_ms_max": round(max(ms[k]), 3),
                           "kernel_ms_all": [round(m, 3) for m in ms[k]], "evaluations": n_eval,
                           "us_per_evaluation": round(med * 1e3 / max(n_eval, 1), 4), "status_ok": float((r.status <= 1).mean())}
    out["same_bits"] = bool(last["plain"].theta.tobytes() == last["noise_v0"].theta.tobytes()
                            and last["plain"].nll.tobytes() == last["noise_v0"].nll.tobytes()
                            and last["plain"].n_eval.tobytes() == last["noise_v0"].n_eval.tobytes())
    p, n = out["cases"]["plain"], out["cases"]["noise_v0"]
    out["ratio_kernel_ms"] = round(n["kernel_ms"] / p["kernel_ms"], 4)
    out["plain_spread_ms"] = round(p["kernel_ms_max"] - p["kernel_ms_min"], 3)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
