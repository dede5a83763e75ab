"""Developer: device binning (DataPrep.bin_data_by -> gpsat_bin_batch) against the reference's way on the host CPUs.

Synthetic along-track rows (seeded): straight tracks crossing a +-4 500 km square, 27 groups = 9 days x 3 sources, rows in
the order daily files are appended (by day, by source, along track).  Grids of 50 km (180 x 180 cells) and 5 km
(1 800 x 1 800), statistic `mean` and the set mean, std, count, median.  Reported per case: wall time of
bin_data_by(return_df=True) end to end with its split (host group coding, the device call with its copies, the kernels
alone, frame building), rows/s, the kernels against a traffic estimate of the three stages, and the reference's procedure
restated here: per group a mask over the whole frame, scipy.stats.binned_statistic_2d per statistic, drop the empty cells.
Last, the kernels on skewed tables (all rows in one cell, in 100 cells).

    python scripts/bin_bench.py [--rows 10000000] [--reps 3] [--no-scipy]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pandas as pd
from scipy import stats as scst

from gpsat_amd import dataprep as dp
from gpsat_amd.dataprep import DataPrep
from gpsat_amd.engine import default_engine

HALF = 4.5e6
BY = ["date", "source"]


def make_rows(R, seed=0, days=9, sources=("CS2", "S3A", "S3B"), tracks_per_group=120):
    rng = np.random.default_rng(seed)
    G = days * len(sources)
    per_track = R // (G * tracks_per_group) + 1
    n_tracks = G * tracks_per_group
    # a track: from a point on the left/bottom side to a point on the right/top side of a slightly larger square
    a = rng.uniform(-1.05 * HALF, 1.05 * HALF, (n_tracks, 2))
    b = rng.uniform(-1.05 * HALF, 1.05 * HALF, (n_tracks, 2))
    side = rng.random(n_tracks) < 0.5
    a[side, 0], b[side, 0] = -1.05 * HALF, 1.05 * HALF
    a[~side, 1], b[~side, 1] = -1.05 * HALF, 1.05 * HALF
    s = np.linspace(0.0, 1.0, per_track)[None, :]
    x = (a[:, :1] + (b[:, :1] - a[:, :1]) * s).ravel()[:R]
    y = (a[:, 1:] + (b[:, 1:] - a[:, 1:]) * s).ravel()[:R]
    g = np.repeat(np.arange(G), tracks_per_group * per_track)[:R]
    z = 0.3 * np.sin(x / 6e5) * np.cos(y / 4e5) + 0.1 * rng.standard_normal(R)
    date = np.datetime64("2020-03-01") + (g // len(sources)).astype("timedelta64[D]")
    return pd.DataFrame({"x": x, "y": y, "z": z, "date": date, "source": np.asarray(sources, dtype=object)[g % len(sources)]})


def scipy_loop(df, grid_res, stats):
    """The reference's bin_data_by(return_df=True) + dropna, restated."""
    n = int(2 * HALF / grid_res + 1)
    edge = np.linspace(-HALF, HALF, n)
    ctr = edge[:-1] + np.diff(edge) / 2
    parts = []
    for _, bcp in df[BY].drop_duplicates().iterrows():
        sel = np.ones(len(df), dtype=bool)
        for bc in BY:
            sel &= (df[bc] == bcp[bc]).values
        d = df.loc[sel, :]
        b = [scst.binned_statistic_2d(d["x"].values, d["y"].values, d["z"].values, statistic=s, bins=[edge, edge],
                                      range=[[-HALF, HALF], [-HALF, HALF]])[0].T for s in stats]
        iy, ix = np.nonzero(~np.any([np.isnan(a) for a in b], axis=0))
        cols = {bc: np.repeat(np.asarray([bcp[bc]]), len(iy)) for bc in BY}
        cols.update({"y": ctr[iy], "x": ctr[ix]})
        cols.update({f"z_{s}": a[iy, ix] for s, a in zip(stats, b)})
        parts.append(pd.DataFrame(cols))
    return pd.concat(parts, ignore_index=True)


def sort_passes(n_keys):
    bits = max(1, int(n_keys).bit_length())
    return -(-bits // 8)                      # rocPRIM's radix sort takes 8 bits per pass


def traffic_bytes(R, n_cells, n_keys, stats):
    """Bytes the three stages move per call (a lower bound: every array read or written once per use)."""
    keys = R * (8 + 8 + 4 + 8 + 4)                                # x, y, gid in; key, row out
    sort = R * 12 * 2 * sort_passes(n_keys) + R * 8               # every pass reads and writes (key, row); one histogram read
    gather = R * (4 + 8 + 8 + 8 + 1)                              # perm, v in; vs out; sorted keys in; flag out
    walks = (1 if {"sum", "mean", "std"} & set(stats) else 0) + ("std" in stats) + (1 if {"min", "max"} & set(stats) else 0)
    stat = R * (1 + 8 * walks) + n_cells * (4 + 8 + 8 * len(stats))
    if "median" in stats:
        stat += R * (8 + 8) + R * 8 * 2 * 8 + n_cells * 16        # canonical copy, 8 passes over the values, two reads
    return keys + sort + gather + stat


def skewed(eng, R):
    """Tables whose rows fall into one cell / into 100 cells: the sums are sequential by definition, a wave walks each cell."""
    rng = np.random.default_rng(1)
    e = np.linspace(-100, 100, 11)
    v = rng.uniform(-1e3, 1e3, R)
    for label, lo, hi in (("one cell", 20, 40), ("100 cells", -100, 100)):
        x, y = rng.uniform(lo, hi, R), rng.uniform(lo, hi, R)
        for stats in (["mean"], ["mean", "std", "min", "max"], ["median"]):
            eng.bin_batch(x, y, v, None, 1, e, e, stats)
            ms = min(eng.bin_batch(x, y, v, None, 1, e, e, stats).kernel_ms for _ in range(3))
            print(f"skewed, {R} rows in {label}, {'+'.join(stats)}: kernels {ms:.2f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    eng = default_engine()
    t0 = time.perf_counter()
    df = make_rows(args.rows)
    print(f"device {eng.device_name}; {len(df)} rows, {len(df[BY].drop_duplicates())} groups, made in {time.perf_counter() - t0:.1f} s", flush=True)
    DataPrep.bin_data_by(df.iloc[:100_000], by_cols=BY, val_col="z", grid_res=50_000, x_range=[-HALF, HALF], y_range=[-HALF, HALF],
                         bin_statistic=["mean", "median"], return_df=True)          # warm-up: library, workspace, rocPRIM kernels
    for grid_res in (50_000, 5_000):
        for stats in (["mean"], ["mean", "std", "count", "median"]):
            kw = dict(by_cols=BY, val_col="z", grid_res=grid_res, x_range=[-HALF, HALF], y_range=[-HALF, HALF],
                      bin_statistic=stats if len(stats) > 1 else stats[0], return_df=True)
            DataPrep.bin_data_by(df, **kw)                                            # warm-up at this size (workspace growth)
            wall, dev, kern = [], [], []
            real, real_code = eng.bin_batch, dp.code_groups
            code = []
            for _ in range(args.reps):
                seen = {}

                def timed_code(*a, **k):
                    t = time.perf_counter()
                    r = real_code(*a, **k)
                    seen["code"] = time.perf_counter() - t
                    return r
                dp.code_groups = timed_code

                def timed(*a, **k):
                    t = time.perf_counter()
                    r = real(*a, **k)
                    seen["call"], seen["res"] = time.perf_counter() - t, r
                    return r
                eng.bin_batch = timed
                t = time.perf_counter()
                out = DataPrep.bin_data_by(df, **kw)
                wall.append(time.perf_counter() - t)
                eng.bin_batch, dp.code_groups = real, real_code
                code.append(seen["code"])
                dev.append(seen["call"])
                kern.append(seen["res"].kernel_ms * 1e-3)
                total_ms = seen["res"].total_ms
            i = int(np.argmin(wall))
            coding = code[i]
            n_edges = int(2 * HALF / grid_res + 1)
            n_keys = 27 * (n_edges - 1) ** 2
            tb = traffic_bytes(len(df), len(out), n_keys, stats)
            print(f"grid {grid_res / 1e3:.0f} km, {'+'.join(stats)}: {len(out)} non-empty cells", flush=True)
            print(f"  bin_data_by end to end: min {min(wall):.3f} s, median {np.median(wall):.3f} s of {args.reps} "
                  f"({len(df) / min(wall) / 1e6:.1f} M rows/s)")
            print(f"  split of the fastest: host group coding {coding:.3f} s, Engine.bin_batch {dev[i]:.3f} s (events: copies + "
                  f"kernels {total_ms * 1e-3:.3f} s, kernels {kern[i]:.4f} s), columns + frame {wall[i] - coding - dev[i]:.3f} s")
            print(f"  kernels: {len(df) / kern[i] / 1e6:.0f} M rows/s, traffic estimate {tb / 1e9:.2f} GB -> {tb / kern[i] / 1e12:.2f} TB/s "
                  f"(streamed reads on this chip: 5.3-6.0 TB/s)", flush=True)
            if not args.no_scipy:
                t = time.perf_counter()
                ref = scipy_loop(df, grid_res, stats)
                ts = time.perf_counter() - t
                cols = ["z"] if len(stats) == 1 else [f"z_{s}" for s in stats]
                same = len(ref) == len(out) and all(
                    np.array_equal(np.sort(ref[f"z_{s}"].to_numpy()), np.sort(out[c].to_numpy())) for s, c in zip(stats, cols))
                print(f"  scipy loop on the host: {ts:.2f} s ({len(df) / ts / 1e6:.2f} M rows/s), {len(ref)} rows, same values: {same}; "
                      f"end to end {ts / min(wall):.1f}x, kernels alone {ts / kern[i]:.0f}x", flush=True)
    skewed(eng, args.rows)


if __name__ == "__main__":
    main()
