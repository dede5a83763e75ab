"""Times the first stage of the pipeline on the GPU: lon / lat -> EASE2 (gpsat_project_batch) and the track numbers
(gpsat_track_batch, DataPrep.assign_tracks) on --rows raw rows in --groups groups, with the NumPy restatement
(tests/prep_numpy.py) on the same host beside them.  Prints one JSON line.

  python scripts/prep_bench.py [--rows 10000000] [--groups 27] [--repeat 3]

Every time is the best of --repeat calls after one warm-up call.  kernel_ms / total_ms come from the library's device events
(gpsat_last_timing: total = with the copies of host mode), wall_ms from a host clock around the whole Python call.  The
restatement's projection is vectorised NumPy on all rows; its track loops are plain Python, so they run on the first
--loop-rows rows and are reported per row, scaled to --rows (marked "scaled").  There is no fallback: without a GPU this fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def best(fn, repeat):
    fn()
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), out


def make_rows(n, groups, seed=0):
    """Rows as a day of altimetry looks: every group (satellite / day) on its own orbit, one row a second, a gap and a jump every
    few thousand rows; interleaved in time."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, groups, n).astype(np.int32)
    gap = rng.random(n) < 1.0 / 3000
    secs = np.cumsum(np.where(gap, 900.0, 0.05))
    phase = np.cumsum(np.where(gap, 1.3, 1e-5)) + g
    lon = (phase * 57.0 * (1 + g % 5)) % 360.0 - 180.0
    lat = 75.0 + 12.0 * np.sin(phase)
    dt = np.datetime64("2020-03-01T00:00:00") + (secs * 1000).astype("timedelta64[ms]")
    return pd.DataFrame({"datetime": dt, "lon": lon, "lat": lat, "sat": g})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--groups", type=int, default=27)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--loop-rows", type=int, default=200_000)
    a = ap.parse_args()
    import torch
    import prep_numpy as pn
    from gpsat_amd.dataprep import DataPrep
    from gpsat_amd.engine import Engine
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    df = make_rows(a.rows, a.groups)
    lon, lat = df["lon"].to_numpy(), df["lat"].to_numpy()
    res = {"rows": a.rows, "groups": a.groups, "device": eng.device_name, "repeat": a.repeat}

    # ---- projection
    def timed(fn):
        wall, out = best(fn, a.repeat)
        return wall, eng.last_prep_ms, out          # the device's times of the last call

    wall, (k, t), (x, y) = timed(lambda: eng.project_batch(lon, lat, "forward"))
    res["project_forward_host"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall, "kernel_GBps": 32.0 * a.rows / k / 1e6}
    wall, (k, t), _ = timed(lambda: eng.project_batch(x, y, "inverse"))
    res["project_inverse_host"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall, "kernel_GBps": 32.0 * a.rows / k / 1e6}
    dlon, dlat = torch.from_numpy(lon).to(dev), torch.from_numpy(lat).to(dev)
    wall, (k, t), _ = timed(lambda: eng.project_batch(dlon, dlat, "forward"))
    res["project_forward_device"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall}
    wall, (rx, ry) = best(lambda: pn.laea_forward(lon, lat), 1)
    res["project_forward_numpy"] = {"wall_ms": wall, "max_abs_diff_m": float(max(np.abs(rx - x).max(), np.abs(ry - y).max()))}
    wall, _ = best(lambda: pn.laea_inverse(x, y), 1)
    res["project_inverse_numpy"] = {"wall_ms": wall}

    # ---- tracks
    codes = df["sat"].to_numpy()
    first = pd.factorize(codes)[0].astype(np.int32)
    wall, (k, t), (delta, track, order) = timed(lambda: eng.track_batch([x, y], group=first, cut_off=600_000.0))
    res["track_host"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall, "tracks": int(track.max()) + 1}
    dx, dy, dg = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(first).to(dev)
    wall, (k, t), _ = timed(lambda: eng.track_batch([dx, dy], group=dg, cut_off=600_000.0))
    res["track_device"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall}
    wall, (k, t), _ = timed(lambda: eng.track_batch([dx, dy], cut_off=600_000.0))
    res["track_device_one_group"] = {"kernel_ms": k, "total_ms": t, "wall_ms": wall, "kernel_GBps": 40.0 * a.rows / k / 1e6}
    m = min(a.loop_rows, a.rows)
    t0 = time.perf_counter()
    o2, d2, t2 = pn.tracks_by_group(np.stack([x[:m], y[:m]], axis=1), first[:m], 600_000.0)
    loop_ms = (time.perf_counter() - t0) * 1e3
    res["track_numpy_loops"] = {"rows": m, "wall_ms": loop_ms, "scaled_wall_ms": loop_ms * a.rows / m}
    d_m, t_m, o_m = eng.track_batch([x[:m], y[:m]], group=first[:m], cut_off=600_000.0)
    res["track_equal_to_loops"] = bool(np.array_equal(t_m, t2) and np.array_equal(o_m, o2))

    # ---- assign_tracks, end to end
    wall, out = best(lambda: DataPrep.assign_tracks(df, sort_by="datetime", get_track_by="sat", cut_off=600_000, engine=eng), max(1, a.repeat - 1))
    res["assign_tracks"] = {"wall_ms": wall, "rows_out": len(out), "tracks": int(out["track"].max()) + 1}
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
