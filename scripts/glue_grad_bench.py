"""Developer: the glued value with the slope of the glued map (Engine.glue_keyed_grad_batch -> gpsat_glue_keyed_grad_batch)
beside the plain average it replaces, Engine.glue_keyed_batch with nvars = 3 (the value and the two gradient columns).

Synthetic predictions (seeded), as scripts/cv_glue_bench.py makes them: groups of 4..16 rows, two glue axes, the rows of a
group scattered over the table (a random permutation: the worst case for the gather).  Both calls read the same columns, so
about the same sort and about the same reduction are expected; no threshold is set.  Reported per size, medians of --reps
after a warm-up at that size, the two calls taken in turn inside every repetition so that drift hits them alike: wall,
events (copies + kernels, kernels) and the kernels split into sort, run detection and reduce (gpsat_glue_keyed_timing).

    python scripts/glue_grad_bench.py [--rows 20000000] [--reps 5] [--max-dist 2.39e5]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gpsat_amd.engine import default_engine

NDIM = 2


def make_rows(R, seed=0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(4, 17, R // 4 + 1)                         # at least R rows whatever is drawn
    sizes = sizes[:np.searchsorted(np.cumsum(sizes), R) + 1]
    key = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)[:R]
    G = int(key[-1]) + 1
    pred = np.repeat(rng.uniform(2e6, 4e6, (NDIM, G)), np.bincount(key), axis=1)
    xprt = pred + rng.uniform(-3e5, 3e5, (NDIM, R))
    val = rng.normal(0.3, 0.1, R)
    grad = rng.normal(0.0, 1e-6, (NDIM, R))
    p = rng.permutation(R)
    return key[p], np.ascontiguousarray(pred[:, p]), np.ascontiguousarray(xprt[:, p]), val[p], np.ascontiguousarray(grad[:, p]), 1e5, G


def last_timing(eng):
    km, tm = C.c_double(0.0), C.c_double(0.0)
    eng._lib.gpsat_last_timing(eng._h, C.byref(km), C.byref(tm))
    return km.value, tm.value


def med(a):
    return float(np.median(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[20_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-dist", type=float, default=None, help="rows at that distance from their expert or beyond stay out "
                    "(2.39e5 leaves out about half of these rows)")
    args = ap.parse_args()
    md = args.max_dist
    eng = default_engine()
    print(f"device {eng.device_name}", flush=True)
    for R in args.rows:
        t0 = time.perf_counter()
        key, pred, xprt, val, grad, sigma, G = make_rows(R)
        vals = np.ascontiguousarray(np.concatenate([val[None], grad]))
        print(f"\n{R} rows, {G} groups of 4..16 rows, ndim {NDIM} (made in {time.perf_counter() - t0:.1f} s)", flush=True)
        calls = {"glue_keyed_grad_batch (value, slope of the glued map)": lambda: eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, md),
                 "glue_keyed_batch, nvars 3 (value, plain average of the gradients)": lambda: eng.glue_keyed_batch(key, pred, xprt, vals, sigma, md)}
        ref = {name: fn() for name, fn in calls.items()}             # warm-up: workspace, rocPRIM kernels, both code objects
        rec = {name: dict(wall=[], kern=[], total=[], split=[]) for name in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                t = time.perf_counter()
                got = fn()
                r = rec[name]
                r["wall"].append(time.perf_counter() - t)
                k, tt = last_timing(eng)
                r["kern"].append(k), r["total"].append(tt), r["split"].append(eng.glue_keyed_timing())
                assert all(u.tobytes() == v.tobytes() for u, v in zip(got, ref[name])), "a second call returned other bytes"
        for name, r in rec.items():
            split = np.array(r["split"])
            print(f"  {name}:\n    wall {med(r['wall']) * 1e3:.1f} ms, events: copies + kernels {med(r['total']):.1f} ms, kernels "
                  f"{med(r['kern']):.2f} ms ({R / med(r['kern']) / 1e3:.0f} M rows/s)")
            for what, j in (("sort", 0), ("run detection", 1), ("reduce", 2)):
                print(f"    {what}: {med(split[:, j]):.3f} ms (min {split[:, j].min():.3f}, max {split[:, j].max():.3f})", flush=True)
        a, b = ref.values()
        assert a[2].tobytes() == b[2][0].tobytes(), "the glued value is not the keyed glue's"
        if md is not None:
            print(f"  max_dist {md:g}: {a[1].sum() / R:.2f} of the rows take part, {np.mean(a[1] == 0):.3f} of the groups have none (NaN)")
        miss = np.nanmax(np.abs(a[3] - b[2][1:]), axis=1) / np.nanmax(np.abs(a[3]), axis=1)
        print(f"  the glued value: the same bytes; the plain average of the gradients misses the slope of the glued map by up to "
              f"{miss[0]:.2f} and {miss[1]:.2f} of its largest value on these rows", flush=True)


if __name__ == "__main__":
    main()
