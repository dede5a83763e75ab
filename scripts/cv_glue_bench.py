"""Developer: the keyed glue (Engine.glue_keyed_batch -> gpsat_glue_keyed_batch) at the sizes of cv_preds.

Synthetic held-out predictions (seeded): groups of 4..16 rows (the experts that overlap one observation), two weight
columns, three variables, the rows of a group scattered over the table as the tiles emit them (a random permutation: the
worst case for the gather).  Reported per size, medians of --reps after a warm-up at that size:
  * the keyed call: wall, events (copies + kernels, kernels) and the kernels split into sort, run detection and reduce, with
    the bytes each stage has to move;
  * the way without it: np.argsort(key, kind="stable"), the columns gathered on the host, Engine.glue_batch;
  * pandas: groupby(key).sum() of the weights and weighted values (the reference's glue_local_predictions on an integer key);
  * the reduce kernel at every team width (GPSAT_DEBUG_GLUE_TEAM; 64 is one wave per group), the widths taken in turn
    inside every repetition so that drift hits them alike: median, min and max.

    python scripts/cv_glue_bench.py [--rows 2000000 20000000] [--reps 5] [--no-pandas]
"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ["GPSAT_DEVELOPER"] = "1"            # the team width is a developer knob
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pandas as pd

from gpsat_amd.engine import default_engine

WIDTHS = (1, 4, 8, 16, 32, 64)
NDIM, NVARS = 2, 3


def make_rows(R, seed=0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(4, 17, R // 4 + 1)                         # at least R rows whatever is drawn
    sizes = sizes[:np.searchsorted(np.cumsum(sizes), R) + 1]
    key = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)[:R]
    G = int(key[-1]) + 1
    pred = np.repeat(rng.uniform(0, 4e6, (NDIM, G)), np.bincount(key), axis=1)
    xprt = pred + rng.uniform(-3e5, 3e5, (NDIM, R))
    vals = rng.normal(0.3, 0.1, (NVARS, R))
    p = rng.permutation(R)
    return key[p], np.ascontiguousarray(pred[:, p]), np.ascontiguousarray(xprt[:, p]), np.ascontiguousarray(vals[:, p]), 1e5, G


def last_timing(eng):
    km, tm = C.c_double(0.0), C.c_double(0.0)
    eng._lib.gpsat_last_timing(eng._h, C.byref(km), C.byref(tm))
    return km.value, tm.value


def stage_bytes(R, G, key_bits):
    """Bytes each stage has to move (every array read or written once per use; a gathered 8-byte value counted as 8 bytes,
    whatever the width of the line it sits in)."""
    passes = -(-key_bits // 8)                                      # rocPRIM's radix sort takes 8 bits per pass
    sort = R * (8 + 8 + 4) + R * 12 * 2 * passes + R * 8            # key kernel; every pass reads and writes (key, row); histogram
    runs = R * (8 + 1) + R * (1 + 4) + G * 4                        # flags from the sorted keys; select reads flags, writes starts
    reduce_ = R * (4 + 8 * (2 * NDIM + NVARS)) + G * (4 + 8 + 8 + 4 + 8 * NVARS)
    return sort, runs, reduce_


def med(a):
    return float(np.median(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2_000_000, 20_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pandas", action="store_true")
    args = ap.parse_args()
    eng = default_engine()
    print(f"device {eng.device_name}", flush=True)
    for R in args.rows:
        t0 = time.perf_counter()
        key, pred, xprt, vals, sigma, G = make_rows(R)
        print(f"\n{R} rows, {G} groups of 4..16 rows, ndim {NDIM}, nvars {NVARS} (made in {time.perf_counter() - t0:.1f} s)", flush=True)
        os.environ.pop("GPSAT_DEBUG_GLUE_TEAM", None)
        ref = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)                     # warm-up: workspace, rocPRIM kernels
        wall, kern, total, split = [], [], [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            got = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)
            wall.append(time.perf_counter() - t)
            k, tt = last_timing(eng)
            kern.append(k), total.append(tt), split.append(eng.glue_keyed_timing())
            assert all(u.tobytes() == v.tobytes() for u, v in zip(got, ref)), "a second call returned other bytes"
        split = np.array(split)
        sb = stage_bytes(R, G, int(G).bit_length())
        print(f"  keyed call: wall {med(wall) * 1e3:.1f} ms, events: copies + kernels {med(total):.1f} ms, kernels {med(kern):.2f} ms "
              f"({R / med(kern) / 1e3:.0f} M rows/s)")
        for name, j, b in (("sort", 0, sb[0]), ("run detection", 1, sb[1]), ("reduce", 2, sb[2])):
            m = med(split[:, j])
            print(f"    {name}: {m:.3f} ms (min {split[:, j].min():.3f}, max {split[:, j].max():.3f}); {b / 1e6:.0f} MB to move -> "
                  f"{b / m / 1e9:.2f} TB/s", flush=True)
        # ---- the way without the keyed call: host sort, gathered columns, glue_batch
        hs, hg, hk, hw = [], [], [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            order = np.argsort(key, kind="stable")
            t1 = time.perf_counter()
            cnt = np.bincount(key)
            seg = np.concatenate([[0], np.cumsum(cnt[cnt > 0])]).astype(np.int64)
            ps, xs, vs = pred[:, order], xprt[:, order], vals[:, order]
            t2 = time.perf_counter()
            base = eng.glue_batch(seg, ps, xs, vs, sigma)
            t3 = time.perf_counter()
            hs.append(t1 - t), hg.append(t2 - t1), hw.append(t3 - t), hk.append(last_timing(eng)[0])
        err = float(np.max(np.abs(base - ref[2]) / np.abs(base)))
        print(f"  host sort + glue_batch: wall {med(hw) * 1e3:.1f} ms = np.argsort(stable) {med(hs) * 1e3:.1f} + segments and gathered "
              f"columns {med(hg) * 1e3:.1f} + Engine.glue_batch {(med(hw) - med(hs) - med(hg)) * 1e3:.1f} (its kernel {med(hk):.2f} ms); "
              f"largest relative difference to the keyed call {err:.1e}", flush=True)
        print(f"  keyed call against it: wall {med(hw) / med(wall):.1f}x, reduce kernel against glue_kernel {med(hk) / med(split[:, 2]):.1f}x")
        if not args.no_pandas:
            reps = args.reps if R <= 5_000_000 else 1
            pw = []
            for _ in range(reps):
                t = time.perf_counter()
                d = pred - xprt
                w = np.prod(np.exp(-(d / sigma) ** 2 / 2) / (sigma * np.sqrt(2 * np.pi)), axis=0)
                df = pd.DataFrame({"key": key, "w": w, **{f"v{i}": w * vals[i] for i in range(NVARS)}})
                s = df.groupby("key").sum()
                out = np.stack([s[f"v{i}"].values / s["w"].values for i in range(NVARS)])
                pw.append(time.perf_counter() - t)
            err = float(np.max(np.abs(out - ref[2]) / np.abs(out)))
            print(f"  pandas on the host (weights, groupby(key).sum(), divide): {med(pw) * 1e3:.0f} ms of {reps}; largest relative "
                  f"difference {err:.1e}; keyed call {med(pw) / med(wall):.1f}x", flush=True)
        # ---- team widths, in turn inside every repetition
        ms = {w_: [] for w_ in WIDTHS}
        outs = {}
        for rep in range(args.reps + 1):                   # the first round warms every width's code object
            for w_ in WIDTHS:
                os.environ["GPSAT_DEBUG_GLUE_TEAM"] = str(w_)
                outs[w_] = eng.glue_keyed_batch(key, pred, xprt, vals, sigma)
                if rep:
                    ms[w_].append(eng.glue_keyed_timing()[2])
        os.environ.pop("GPSAT_DEBUG_GLUE_TEAM", None)
        for w_ in WIDTHS:
            a = np.array(ms[w_])
            err = float(np.max(np.abs(outs[w_][2] - ref[2]) / np.abs(ref[2])))
            print(f"  reduce, {w_:2d} lanes per group: median {med(a):.3f} ms (min {a.min():.3f}, max {a.max():.3f}), "
                  f"{sb[2] / med(a) / 1e9:.2f} TB/s; against the product's width {err:.1e}", flush=True)


if __name__ == "__main__":
    main()
