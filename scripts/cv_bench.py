"""Cost of the held-out phase (gpsat_fit_predict_batch_cv) on the fp64 tile kernel.

Batch: T tiles x N observations, D = 3, RBF, fp64, optimiser "none", no prediction points.  Kernel time (the C ABI's own
events around the launch, gpsat_last_timing) of: the plain call, leave-one-out, contiguous folds of G rows, the same labels
shuffled inside every tile -- and, for scale, one evaluation with the gradient.  Prints one JSON line.

    python scripts/cv_bench.py [--tiles 4096] [--obs 500] [--fold 25] [--reps 5]

``--refit``: the cost of fitting every fold again (gpsat_fit_predict_batch_cv_refit): the same tiles with contiguous folds of
``--fold`` rows, L-BFGS from theta0 = 1 with the default bounds, fp32 and fp64, both ``start`` values.  Beside the kernel time
of the call (both launches and the two streaming kernels around the second) it prints the BASELINE: the plain call plus the
same derived tiles built on the host and handed to gpsat_fit_predict_batch as one batch (existing code, same process), and
the time of the two streaming kernels alone with the bytes they move (read: every tile's X, y and two int32 per row once per
fold; written: the derived X', y', Xs').

    python scripts/cv_bench.py --refit [--tiles 4096] [--obs 500] [--fold 25] [--max-iter 10000]

``--joint``: the cost of the joint log predictive density per fold (cv_joint): the same tiles with
contiguous folds of ``--fold`` rows in fp64, the factor flavour (optimiser "none") and the refit flavour (L-BFGS from theta0 = 1,
``--max-iter``), each without and with ``cv_joint``.  With a library that lacks the entry points (an earlier commit's) the calls
without it are timed alone, so that the unchanged path can be set beside its parent's.

    python scripts/cv_bench.py --joint [--tiles 4096] [--obs 500] [--fold 25] [--max-iter 10000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpsat_amd import synthetic as syn          # noqa: E402
from gpsat_amd.engine import Engine             # noqa: E402


def refit_bench(a):
    import re
    import subprocess
    if os.environ.get("GPSAT_DEBUG_CVFOLD_STATS") is None:
        # the library's own figures for the two streaming kernels come on stderr (developer statistics): a child process
        # with them switched on, its stderr read here
        env = dict(os.environ, GPSAT_DEVELOPER="1", GPSAT_DEBUG_CVFOLD_STATS="1")
        p = subprocess.run([sys.executable] + sys.argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        sys.stderr.write("".join(ln + "\n" for ln in p.stderr.splitlines() if not ln.startswith("gpsat cvfold:")))
        if p.returncode != 0:
            sys.exit(p.returncode)
        out = json.loads(p.stdout.strip().splitlines()[-1])
        stats = re.findall(r"gpsat cvfold: (\d+) derived tiles, (\d+) expanded rows, (\d+) held-out rows: expand ([\d.]+) ms, scatter ([\d.]+) ms", p.stderr)
        nfold = -(-out["obs"] // out["fold"])
        stats = [st for st in stats if int(st[0]) == out["tiles"] * nfold]          # not the warm-up calls
        for (name, case), st in zip(out["cases"].items(), stats):
            F2, E, P2, ems, sms = int(st[0]), int(st[1]), int(st[2]), float(st[3]), float(st[4])
            esz = 4 if name.startswith("f32") else 8
            D = out["D"]
            rows_read = F2 * out["obs"]                          # every derived tile reads its whole source tile
            moved = rows_read * ((D + 1) * esz + 8) + (E * (D + 1) + P2 * D) * esz
            case.update(expand_ms=ems, scatter_ms=sms, expand_bytes=moved, expand_GBps=round(moved / ems * 1e-6, 1))
        print(json.dumps(out))
        return
    T, N, D, G = a.tiles, a.obs, 3, a.fold
    out = {"tiles": T, "obs": N, "D": D, "fold": G, "kernel": "RBF", "max_iter": a.max_iter, "cases": {}}
    eng = Engine(0)
    out["device"] = eng.device_name
    labels = np.tile(np.arange(N, dtype=np.int32) // G, T)
    lo, hi = syn.default_bounds(T, D)
    for dtype, np_dt in (("f32", np.float32), ("f64", np.float64)):
        b = syn.make_batch(T, N, 0, D, 0, base_seed=2000, dtype=np_dt)
        kw = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=np.ones((T, D + 2)), lo=lo,
                  hi=hi, kernel="RBF", optimiser="lbfgs", max_iter=a.max_iter, dtype=dtype)
        small = {k: (v[:2 * N] if k in ("X", "y") else v[:3] if k in ("obs_off", "pred_off") else v[:2] if k in ("theta0", "lo", "hi") else v)
                 for k, v in kw.items()}
        eng.fit_predict_batch(**small, cv_fold=labels[:2 * N], cv_refit=True)       # warm-up: code objects
        for start in ("theta0", "full"):
            r = eng.fit_predict_batch(**kw, cv_fold=labels, cv_refit={"start": start, "max_expanded_rows": 1 << 40})
            plain = eng.fit_predict_batch(**kw)
            # baseline: the derived tiles from the host, as one batch through the existing entry point
            Xo, yo, Xp, th, nfold = [], [], [], [], N // G + (N % G > 0)
            for t in range(T):
                Xt, yt = b["X"][t * N:(t + 1) * N], b["y"][t * N:(t + 1) * N]
                for k in range(nfold):
                    keep = labels[:N] != k
                    f = t * nfold + k
                    Xo.append(Xt[keep]); yo.append((yt[keep].astype(np.float64) - r.cv_shift[f]).astype(np_dt)); Xp.append(Xt[~keep])
                    th.append(r.theta[t] if start == "full" else np.ones(D + 2))
            off = lambda v: np.concatenate([[0], np.cumsum([len(x) for x in v])]).astype(np.int64)
            base = eng.fit_predict_batch(D=D, obs_off=off(Xo), X=np.concatenate(Xo), y=np.concatenate(yo), pred_off=off(Xp), Xs=np.concatenate(Xp),
                                         theta0=np.array(th), lo=np.repeat(lo, nfold, axis=0), hi=np.repeat(hi, nfold, axis=0), kernel="RBF",
                                         optimiser="lbfgs", max_iter=a.max_iter, dtype=dtype)
            same = bool((base.theta == r.cv_theta).all())
            out["cases"][f"{dtype}_{start}"] = {
                "call_kernel_ms": round(r.kernel_ms, 2), "call_total_ms": round(r.total_ms, 2),
                "baseline_kernel_ms": round(plain.kernel_ms + base.kernel_ms, 2), "baseline_total_ms": round(plain.total_ms + base.total_ms, 2),
                "plain_kernel_ms": round(plain.kernel_ms, 2), "folds": int(len(r.cv_nll)), "mean_evaluations_per_fold": round(float(r.cv_n_eval.mean()), 2),
                "folds_converged": int((r.cv_status == 0).sum()), "same_theta_as_baseline": same}
    eng.close()
    print(json.dumps(out))


def joint_bench(a):
    """The cost of the joint density per fold (cv_joint) beside the same call without it, both flavours, fp64."""
    T, N, D, G = a.tiles, a.obs, 3, a.fold
    b = syn.make_batch(T, N, 0, D, 0, base_seed=2000, dtype=np.float64)
    labels = np.tile(np.arange(N, dtype=np.int32) // G, T)
    lo, hi = syn.default_bounds(T, D)
    eng = Engine(0)
    out = {"tiles": T, "obs": N, "D": D, "fold": G, "kernel": "RBF", "dtype": "f64", "device": eng.device_name, "reps": a.reps,
           "refit_max_iter": a.max_iter, "has_joint": hasattr(eng._lib, "gpsat_fit_predict_batch_cv_joint"), "kernel_ms": {}}
    kw = dict(D=D, obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], kernel="RBF", dtype="f64", cv_fold=labels)
    factor = dict(kw, theta0=np.ones((T, D + 2)), optimiser="none")
    refit = dict(kw, theta0=np.ones((T, D + 2)), lo=lo, hi=hi, optimiser="lbfgs", max_iter=a.max_iter,
                 cv_refit={"max_expanded_rows": 1 << 40})
    cases = {"factor": factor, "refit": refit}
    if out["has_joint"]:                                  # a library without the entry points: the calls without it only
        cases.update(factor_joint=dict(factor, cv_joint=True), refit_joint=dict(refit, cv_joint=True))
    for name, c in cases.items():
        reps = a.reps if name.startswith("factor") else max(1, min(a.reps, 2))
        eng.fit_predict_batch(**c)                        # warm-up: buffers, code objects
        ms = [eng.fit_predict_batch(**c).kernel_ms for _ in range(reps)]
        out["kernel_ms"][name] = {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}
        print(name, out["kernel_ms"][name], file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refit", action="store_true")
    ap.add_argument("--joint", action="store_true")
    ap.add_argument("--max-iter", type=int, default=10_000)
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--obs", type=int, default=500)
    ap.add_argument("--fold", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.joint:
        return joint_bench(a)
    if a.refit:
        return refit_bench(a)
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
