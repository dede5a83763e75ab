"""Developer: the glued value with the slope and the second derivatives of the glued map (Engine.glue_keyed_hess_batch ->
gpsat_glue_keyed_hess_batch) beside what the plain rule offers for the same six columns: two Engine.glue_keyed_batch calls,
nvars 4 (the value, the two gradient columns and the first second derivative) and nvars 2 (the other two).

Synthetic predictions (seeded), as scripts/glue_grad_bench.py makes them: groups of 4..16 rows, two glue axes, the rows of a
group scattered over the table (a random permutation: the worst case for the gather).  The new call sorts once where the
baseline sorts twice and gathers a row's ten columns once where the baseline reads the four location columns twice; no
threshold is set.  Reported per size, medians of --reps after a warm-up at that size, the three calls taken in turn inside
every repetition so that drift hits them alike: wall, events (copies + kernels, kernels) and the kernels split into sort,
run detection and reduce (gpsat_glue_keyed_timing); then the baseline's two calls summed.

    python scripts/glue_hess_bench.py [--rows 20000000] [--reps 5]
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
    hess = rng.normal(0.0, 1e-11, (3, R))
    p = rng.permutation(R)
    c = np.ascontiguousarray
    return key[p], c(pred[:, p]), c(xprt[:, p]), val[p], c(grad[:, p]), c(hess[:, p]), 1e5, G


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
    args = ap.parse_args()
    eng = default_engine()
    print(f"device {eng.device_name}", flush=True)
    for R in args.rows:
        t0 = time.perf_counter()
        key, pred, xprt, val, grad, hess, sigma, G = make_rows(R)
        four = np.ascontiguousarray(np.concatenate([val[None], grad, hess[:1]]))
        two = np.ascontiguousarray(hess[1:])
        print(f"\n{R} rows, {G} groups of 4..16 rows, ndim {NDIM} (made in {time.perf_counter() - t0:.1f} s)", flush=True)
        new, plain4, plain2 = "glue_keyed_hess_batch (value, slope and second derivatives of the glued map)", \
            "glue_keyed_batch, nvars 4 (value, plain average of the gradients and of h_00)", "glue_keyed_batch, nvars 2 (plain average of h_01 and h_11)"
        calls = {new: lambda: eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma),
                 plain4: lambda: eng.glue_keyed_batch(key, pred, xprt, four, sigma),
                 plain2: lambda: eng.glue_keyed_batch(key, pred, xprt, two, sigma)}
        ref = {name: fn() for name, fn in calls.items()}             # warm-up: workspace, rocPRIM kernels, the code objects
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
        both = lambda k: med(np.array(rec[plain4][k]) + np.array(rec[plain2][k]))
        red = med(np.array(rec[plain4]["split"])[:, 2] + np.array(rec[plain2]["split"])[:, 2])
        print(f"  the two plain calls together: wall {both('wall') * 1e3:.1f} ms, copies + kernels {both('total'):.1f} ms, kernels "
              f"{both('kern'):.2f} ms, reduce {red:.3f} ms; the new call's reduce: {med(np.array(rec[new]['split'])[:, 2]):.3f} ms")
        a, b, c = ref[new], ref[plain4], ref[plain2]
        assert a[2].tobytes() == b[2][0].tobytes(), "the glued value is not the keyed glue's"
        plain = np.concatenate([b[2][3:], c[2]])
        miss = np.abs(a[4] - plain).max(axis=1) / np.abs(a[4]).max(axis=1)
        print(f"  the glued value: the same bytes; the plain average of the second derivatives misses those of the glued map by up to "
              f"{miss[0]:.2f}, {miss[1]:.2f} and {miss[2]:.2f} of their largest value on these rows", flush=True)


if __name__ == "__main__":
    main()
