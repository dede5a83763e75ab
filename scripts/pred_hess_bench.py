"""Cost of the second derivatives of the posterior mean (pred_hess) on the fp64 tile kernel, beside the plain and the grad build
in the same process.

Batch: T tiles x N observations, P prediction points per tile, D = 3, Matern52, fp64, optimiser "none" (one evaluation at
theta0 = 1, then the prediction).  The cases take turns on one engine: the plain build without prediction points (the evaluation
alone), the plain build with them (gpsat_fit_predict_batch), the grad build (gpsat_fit_predict_batch_grad: D more passes of the
prediction's triangular solve) and the hess build (gpsat_fit_predict_batch_hess: m (m + 1) / 2 passes for the pairs of the m
chosen coordinates and one for the Laplacian) with the first two coordinates and with all three.  All builds are those of the
same wave count.  Kernel time (the C ABI's own events around the launch, gpsat_last_timing): the median of ``--reps`` launches
per case after one warm-up launch each, with min and max.  The prediction phase of a case is its kernel time minus the
evaluation's; the expectation for its ratio to the plain build's is 1 + m (m + 1) / 2 + 1.  Prints one JSON line.

    python scripts/pred_hess_bench.py [--tiles 4096] [--obs 500] [--pred 500] [--reps 5]
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
    ap.add_argument("--pred", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    T, N, P, D = a.tiles, a.obs, a.pred, 3
    b = syn.make_batch(T, N, P, D, 3, base_seed=42, dtype=np.float64)
    eng = Engine(0)
    out = {"tiles": T, "obs": N, "pred": P, "D": D, "kernel": "Matern52", "dtype": "f64", "optimiser": "none", "reps": a.reps,
           "device": eng.device_name, "cases": {}}
    common = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], theta0=np.ones((T, D + 2)), kernel="Matern52", optimiser="none",
                  dtype="f64")
    with_pred = dict(pred_off=b["pred_off"], Xs=b["Xs"])
    hess = {"hess_xy": [0, 1], "hess_all": [0, 1, 2]}
    cases = {"evaluation_only": dict(pred_off=np.zeros(T + 1, dtype=np.int64), Xs=np.zeros((0, D))),
             "plain": with_pred, "grad": dict(pred_grad=True, **with_pred),
             **{k: dict(pred_hess={"dims": dims}, **with_pred) for k, dims in hess.items()}}
    ms, last = {k: [] for k in cases}, {}
    for k, kw in cases.items():
        eng.fit_predict_batch(**common, **kw)                         # warm-up
    for _ in range(a.reps):
        for k, kw in cases.items():
            last[k] = eng.fit_predict_batch(**common, **kw)
            ms[k].append(last[k].kernel_ms)
    for k in cases:
        out["cases"][k] = {"kernel_ms": round(float(np.median(ms[k])), 3), "kernel_ms_min": round(min(ms[k]), 3),
                           "kernel_ms_max": round(max(ms[k]), 3), "kernel_ms_all": [round(m, 3) for m in ms[k]]}
    out["same_bits"] = bool(all(np.asarray(getattr(last["plain"], f)).tobytes() == np.asarray(getattr(last[k], f)).tobytes()
                                for k in ("grad", *hess) for f in ("theta", "nll", "status", "f_mean", "f_var", "y_var")))
    ev, pl = out["cases"]["evaluation_only"]["kernel_ms"], out["cases"]["plain"]["kernel_ms"]
    out["prediction_ms"] = {k: round(out["cases"][k]["kernel_ms"] - ev, 3) for k in cases if k != "evaluation_only"}
    out["ratio_prediction"] = {k: round((out["cases"][k]["kernel_ms"] - ev) / (pl - ev), 4) if pl > ev else None
                               for k in ("grad", *hess)}
    out["ratio_kernel_ms"] = {k: round(out["cases"][k]["kernel_ms"] / pl, 4) for k in ("grad", *hess)}
    out["expected_ratio_prediction"] = {"grad": 1 + D, **{k: 1 + len(d) * (len(d) + 1) // 2 + 1 for k, d in hess.items()}}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
