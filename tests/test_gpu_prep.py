"""GPU: gpsat_prep.hip through gpsat_project_batch / gpsat_track_batch, Engine, gpsat_amd.prep and DataPrep.assign_tracks,
against tests/prep_numpy.py and the mpmath values of tests/golden/kat_ease2.npz.  The bounds are those of tests/test_prep_cpu.py
(its docstring derives them).  Tracks are integers: equal to the restatement's; dr / dt within 1 ulp (the device takes one
correctly rounded root where NumPy may take pow(s, 0.5))."""
import numpy as np
import pandas as pd
import pytest

import prep_numpy as pn
from test_prep_cpu import (EPS, forward_unit, golden, golden_cases, inverse_errors, lon_diff, reference_like,  # noqa: F401
                           satellite_frame, sorted_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def B():
    from gpsat_amd import _lib as L
    return int(L.load()._ZN5gpsat15prep_scan_blockEv())


@pytest.fixture(scope="module")
def device_project(eng):
    def project(direction, a, b, lon_0, lat_0):
        return eng.project_batch(a, b, direction, lon_0, lat_0)
    return project


# ---- projection
def test_forward_golden_on_the_device(golden, device_project):
    """Worst seen on the device (MI355X, 2026-10-20, ROCm 7.2.0): 3.0 units."""
    worst = 0.0
    for lat_0, lon_0, m, ok, (x, y), _ in golden_cases(golden, device_project):
        err = np.maximum(np.abs(x - golden["x"][m]), np.abs(y - golden["y"][m])) / forward_unit(golden["x"][m], golden["y"][m])
        worst = max(worst, err.max())
    print("device forward worst units:", worst)
    assert worst <= 16.0


def test_inverse_golden_own_hemisphere_on_the_device(golden, device_project):
    err, unit, _, _, own = inverse_errors(golden, device_project)
    units = (err / unit)[own > 0]
    print("device inverse, own hemisphere, worst units:", units.max())
    assert units.max() <= 16.0


def test_inverse_golden_opposite_hemisphere_on_the_device(golden, device_project):
    """The bound beyond the equator, where it tends to 8 EPS (test_prep_cpu.test_inverse_golden_opposite_hemisphere).  The
    kernel's statements, built for the host, give the restatement's 2.4 units; NOT yet run on a device."""
    err, unit, _, _, own = inverse_errors(golden, device_project)
    units = (err / unit)[own == 0]
    print("device inverse, opposite hemisphere, worst units:", units.max())
    assert units.max() <= 16.0


def test_inverse_golden_first_order_bound_on_the_device(golden, device_project):
    err, _, cosphi, dlon, _ = inverse_errors(golden, device_project)
    units = err / (EPS / np.maximum(cosphi, 1.0 / pn.A))
    print("device inverse, all points, worst units of EPS / cos(phi):", units.max(), "longitude:", dlon.max())
    assert units.max() <= 16.0
    assert dlon.max() <= 4 * EPS * 360.0


def test_documented_values_on_the_device():
    from gpsat_amd import prep
    x, y = prep.WGS84toEASE2(-105.01621, 39.57422)
    assert abs(x - -5254767.014984061) <= 1e-8 and abs(y - 1409604.1043472202) <= 1e-8
    lon, lat = prep.EASE2toWGS84(1000000, 2000000)
    print("device documented values:", repr(x), repr(y), repr(lon), repr(lat))
    assert abs(lon - 153.434948822922) <= 1e-12 and abs(lat - 69.86894542225777) <= 2e-9
    assert abs(lat - 69.86894542320586) <= 1e-12


def points(n, seed, lat_0):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-180.0, 180.0, n)
    lat = np.degrees(np.arcsin(rng.uniform(-np.sin(np.radians(60.0)), 1.0, n))) * np.sign(lat_0)
    return lon, lat


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000003])
def test_projection_sizes(eng, n):
    """Device against restatement: each lies within 16 units of the exact value, so the two within 32 of each other."""
    for lat_0 in (90.0, -90.0):
        lon, lat = points(n, n + 1, lat_0)
        x, y = eng.project_batch(lon, lat, "forward", 10.0, lat_0)
        rx, ry = pn.laea_forward(lon, lat, 10.0, lat_0)
        assert x.shape == (n,) and y.shape == (n,)
        lo, la = eng.project_batch(rx, ry, "inverse", 10.0, lat_0)
        rlo, rla = pn.laea_inverse(rx, ry, 10.0, lat_0)
        if n:
            assert (np.maximum(np.abs(x - rx), np.abs(y - ry)) / forward_unit(rx, ry)).max() <= 32.0
            assert (np.abs(np.radians(la - rla)) / (EPS / np.maximum(np.cos(np.radians(lat)), 1.0 / pn.A))).max() <= 32.0
            assert lon_diff(lo, rlo).max() <= 8 * EPS * 360.0


def test_nan_rows_stay_nan_and_disturb_no_neighbour(eng):
    lon, lat = points(1000, 5, 90.0)
    clean = eng.project_batch(lon, lat, "forward")
    lon2, lat2 = lon.copy(), lat.copy()
    lon2[[0, 63, 64, 500]] = np.nan
    lat2[[65, 500, 999]] = np.nan
    bad = np.isnan(lon2) | np.isnan(lat2)
    for direction, (a, b), ref in (("forward", (lon2, lat2), clean), ("inverse", (np.where(bad, np.nan, clean[0]), clean[1]), None)):
        o0, o1 = eng.project_batch(a, b, direction)
        assert np.isnan(o0[bad]).all() and np.isnan(o1[bad]).all()
        assert np.isfinite(o0[~bad]).all() and np.isfinite(o1[~bad]).all()
        if ref is None:
            ref = eng.project_batch(clean[0], clean[1], direction)
        assert o0[~bad].tobytes() == ref[0][~bad].tobytes() and o1[~bad].tobytes() == ref[1][~bad].tobytes()


def test_centre_and_outside_of_the_disc(eng):
    for lat_0 in (90.0, -90.0):
        x, y = eng.project_batch(np.array([33.0, -170.0]), np.array([lat_0, lat_0]), "forward", 12.0, lat_0)
        assert (x == 0.0).all() and (y == 0.0).all()
        edge = pn.A * np.sqrt(2.0 * pn.QP)
        lon, lat = eng.project_batch(np.array([0.0, edge * (1 + 1e-9), 0.0, 3e7, 1e6]), np.array([0.0, 0.0, -edge * 1.001, 3e7, 2e6]),
                                     "inverse", 12.0, lat_0)
        assert (lon[0], lat[0]) == (12.0, lat_0)
        assert np.isposinf(lon[1:4]).all() and np.isposinf(lat[1:4]).all()
        assert np.isfinite(lon[4]) and np.isfinite(lat[4])


def test_device_tensors_give_the_bytes_of_host_arrays(eng):
    import torch
    dev = torch.device("cuda", eng.device_id)
    lon, lat = points(70001, 9, 90.0)
    for direction, (a, b) in (("forward", (lon, lat)), ("inverse", pn.laea_forward(lon, lat, -45.0, 90.0))):
        h0, h1 = eng.project_batch(a, b, direction, -45.0, 90.0)
        d0, d1 = eng.project_batch(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), direction, -45.0, 90.0)
        assert isinstance(d0, torch.Tensor) and d0.is_cuda
        assert d0.cpu().numpy().tobytes() == h0.tobytes() and d1.cpu().numpy().tobytes() == h1.tobytes()
        again = eng.project_batch(a, b, direction, -45.0, 90.0)
        assert again[0].tobytes() == h0.tobytes() and again[1].tobytes() == h1.tobytes()
    cols, codes = sorted_rows(np.random.default_rng(2), 70001, 27, n_cols=3, null_every=11)
    codes = codes.astype(np.int32)
    host = eng.track_batch(list(cols.T.copy()), group=codes, cut_off=20.0, start_track=5)
    tens = eng.track_batch([torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols.T], group=torch.from_numpy(codes).to(dev),
                           cut_off=20.0, start_track=5)
    again = eng.track_batch(list(cols.T.copy()), group=codes, cut_off=20.0, start_track=5)
    for h, t, a in zip(host, tens, again):
        assert t.cpu().numpy().tobytes() == h.tobytes() == a.tobytes()


# ---- tracks
def ulp_close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return bool((np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok]))).all())


def check_tracks(eng, cols, codes, cut_off, start_track=0):
    """The device against the group loop; first, on the restatement: no distance within a relative 1e-9 of cut_off."""
    cols = np.asarray(cols, dtype=np.float64)
    cols = cols[:, None] if cols.ndim == 1 else cols
    order, delta, track = pn.tracks_by_group(cols, codes, cut_off, start_track)
    fin = delta[np.isfinite(delta)]
    assert not (np.abs(fin - cut_off) <= 1e-9 * abs(cut_off)).any()
    d, t, o = eng.track_batch([np.ascontiguousarray(cols[:, c]) for c in range(cols.shape[1])],
                              group=None if codes is None else np.asarray(codes, dtype=np.int32), cut_off=cut_off, start_track=start_track)
    assert d.dtype == np.float64 and t.dtype == np.int32 and o.dtype == np.int32
    assert np.array_equal(o, order)
    assert np.array_equal(t, track)
    assert ulp_close(d, delta)
    return t


def steps_column(steps):
    return np.cumsum(np.asarray(steps, dtype=np.float64))


@pytest.mark.parametrize("size", ["0", "1", "2", "B-1", "B", "B+1", "3*B+7", "B*B+1"])
def test_track_sizes(eng, B, size):
    n = eval(size, {"B": B})
    cols, _ = sorted_rows(np.random.default_rng(n + 3), max(n, 1), 1)
    t = check_tracks(eng, cols[:n], None, 20.0)
    if n > 50:
        assert t[-1] > n // 40


def test_flags_at_block_edges(eng, B):
    n = 3 * B + 7
    for flagged in ([B], [B - 1], [2 * B - 1, 2 * B], [0], [n - 1], list(range(n)), []):
        steps = np.ones(n)
        steps[flagged] = 100.0
        t = check_tracks(eng, steps_column(steps), None, 10.0)
        assert t[-1] == len([f for f in flagged if f > 0])


def test_groups(eng, B):
    n = 3 * B + 7
    rng = np.random.default_rng(8)
    cols, codes27 = sorted_rows(rng, n, 27)
    assert len(set(codes27)) == 27
    check_tracks(eng, cols, np.arange(n), 20.0)                           # groups of one row: every row starts a track
    check_tracks(eng, cols, np.zeros(n, dtype=np.int64), 20.0)            # one group
    check_tracks(eng, cols, codes27, 20.0)                                # 27 groups interleaved
    check_tracks(eng, cols, np.where(codes27 >= 3, codes27 + 1, codes27), 20.0)       # a code that no row has
    nulls = codes27.copy()
    nulls[::5] = -1
    t = check_tracks(eng, cols, nulls, 20.0)
    assert (t[-len(range(0, n, 5)):] == -1).all() and (t[:-len(range(0, n, 5))] >= 0).all()
    check_tracks(eng, cols, np.full(n, -1), 20.0)                         # no row in any group


def test_nan_coordinate_starts_no_track(eng):
    col = steps_column(np.ones(600))
    col[[0, 100, 255, 256, 599]] = np.nan
    t = check_tracks(eng, col, None, 0.5)                                 # every finite distance is above the cut
    assert t[100] == t[99] and t[101] == t[100] and t[102] == t[101] + 1
    xy = np.stack([col, steps_column(np.ones(600))], axis=1)
    check_tracks(eng, xy, None, 0.5)


@pytest.mark.parametrize("n_cols", [1, 2, 3])
def test_columns_and_start_track(eng, n_cols):
    cols, codes = sorted_rows(np.random.default_rng(n_cols), 5000, 4, n_cols=n_cols)
    t = check_tracks(eng, cols, codes, 20.0, start_track=5)
    assert t.min() == 5


def test_track_num_for_date_across_blocks(eng, B):
    from gpsat_amd import prep
    runs = [1, B - 1, 1, B, 2, B + 1, 3 * B + 7, 1, 1, 5]
    x = np.repeat(np.arange(len(runs)) % 3 + 18000, runs).astype(np.int64)
    got = prep.track_num_for_date(x, engine=eng)
    assert got.dtype == np.float64 and np.array_equal(got, pn.track_num_for_date(x))
    _, run, order = eng.track_batch([x.astype(np.float64)], group=(np.arange(len(x)) % 2).astype(np.int32), mode="runs")
    want = np.concatenate([pn.track_num_for_date(x[0::2]), pn.track_num_for_date(x[1::2])])
    assert np.array_equal(run, want) and np.array_equal(order, np.r_[np.arange(0, len(x), 2), np.arange(1, len(x), 2)])
    d = np.array([np.nan, 1.0, 7.0, 2.0, 7.0, 7.0] * 100)
    assert np.array_equal(prep.guess_track_num(d, 5.0, start_track=3, engine=eng), pn.guess_track_num(d, 5.0, 3))
    xy = np.random.default_rng(0).normal(size=(777, 2))
    assert ulp_close(prep.diff_distance(xy, engine=eng), pn.diff_distance(xy))


def test_refusals_leave_the_handle_usable(eng):
    from gpsat_amd.engine import GpsatError
    one = np.ones(4)
    with pytest.raises(GpsatError, match="lat_0"):
        eng.project_batch(one, one, "forward", 0.0, 45.0)
    with pytest.raises(GpsatError, match="lon_0"):
        eng.project_batch(one, one, "forward", float("nan"), 90.0)
    with pytest.raises(GpsatError, match="cut_off"):
        eng.track_batch([one], cut_off=float("inf"))
    with pytest.raises(GpsatError, match=r"group\[2\] = -7"):
        eng.track_batch([one], group=np.array([0, 0, -7, 1], dtype=np.int32), cut_off=1.0)
    d, t, o = eng.track_batch([one], cut_off=1.0)
    assert t.tolist() == [0, 0, 0, 0] and o.tolist() == [0, 1, 2, 3]


# ---- end to end
def test_assign_tracks_end_to_end(eng, tmp_path):
    from gpsat_amd.dataprep import DataPrep
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    df = satellite_frame(np.random.default_rng(21), n_per=6667).iloc[:20000]
    out = DataPrep.assign_tracks(df, sort_by="datetime", get_track_by="sat", delta_measure="dr", cut_off=600_000, engine=eng)
    want = reference_like(df, "sat", "dr", 600_000, 0)
    fin = want["dr"].to_numpy()[np.isfinite(want["dr"].to_numpy())]
    assert not (np.abs(fin - 600_000) <= 1e-9 * 600_000).any() and (np.abs(fin - 600_000) > 1.0).all()
    assert list(out.columns) == list(want.columns) and np.array_equal(out.index.to_numpy(), want.index.to_numpy())
    assert np.array_equal(out["track"].to_numpy(), want["track"].to_numpy()) and out["track"].nunique() > 100
    assert np.array_equal(out["t"].to_numpy(), want["t"].to_numpy())
    unit = forward_unit(want["x"].to_numpy(), want["y"].to_numpy())
    assert (np.maximum(np.abs(out["x"] - want["x"]), np.abs(out["y"] - want["y"])).to_numpy() / unit).max() <= 32.0
    # the distances of the device's own x, y: 1 ulp
    for sat, rows in out.groupby("sat", sort=False):
        assert ulp_close(rows["dr"].to_numpy(), pn.diff_distance(rows[["x", "y"]].to_numpy()))
        assert ulp_close(rows["dt"].to_numpy(), pn.diff_distance(rows["t"].to_numpy()))
    # the column is usable where it is needed: cross-validation by track on a handful of experts
    rng = np.random.default_rng(0)
    data = out.reset_index(drop=True)
    data["z"] = np.sin(data["x"] / 4e5) * np.cos(data["y"] / 4e5) + 0.1 * rng.standard_normal(len(data))
    centres = data.iloc[[100, 4000, 8000, 12000, 16000, 19000]]
    xl = pd.DataFrame({"x": centres["x"].to_numpy(), "y": centres["y"].to_numpy()})
    cfg = {"data_source": data, "obs_col": "z", "coords_col": ["x", "y"],
           "local_select": [{"col": ["x", "y"], "comp": "<", "val": 250_000.0}]}
    model = {"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "coords_scale": [1e5, 1e5]},
             "constraints": {"lengthscales": {"low": [0.1, 0.1], "high": [50, 50]}}, "optim_kwargs": {"max_iter": 6}}
    res = BatchedLocalExpertOI({"source": xl}, cfg, model, {"method": "expert_loc"}, engine=eng, dtype="f64",
                               cv={"by": ["track"]}).run(str(tmp_path / "cv"), store_every=16)
    cvp, rd = res["cv_preds"], res["run_details"]
    print("experts:", len(rd), "obs:", rd["num_obs"].tolist(), "skipped:", rd["cv_rows_skipped"].tolist())
    assert len(rd) == 6 and (rd["num_obs"] > 20).all()
    held = int(rd["num_obs"].sum() - rd["cv_rows_skipped"].sum())          # a track of more than 256 rows in a tile is skipped
    assert len(cvp) == int(rd["num_obs"].sum()) and held > 1000
    assert int(np.isfinite(cvp["f*"].to_numpy()).sum()) >= held
    tracks = data["track"].to_numpy()[cvp["obs_index"].to_numpy()]
    assert len(np.unique(tracks)) > 12                                       # the folds: many tracks per tile
