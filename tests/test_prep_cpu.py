"""CPU: the restatement the device is held to (tests/prep_numpy.py) against the reference's documented values and against
mpmath (tests/golden/kat_ease2.npz, written by tests/golden/make_ease2_golden.py); the one-pass track rule against the group
loop; the host logic of gpsat_amd.prep and DataPrep.assign_tracks on a device-free stand-in engine; the ABI structs and every
refusal of gpsat_amd/csrc/gpsat_prep_plan.h without a device.

Bounds (EPS = 2^-52, a = 6378137 m, rho = the point's distance from the centre of the projection):
  forward   16 EPS (a^2 / max(rho, 1 mm) + rho) metres: the first-order size of the cancellation in q_p - q;
  inverse   16 EPS a / max(rho, 1 m) radians of latitude, on every point.  Towards the projection's own pole that is the
            cancellation of q_p - q seen from the other side; beyond the equator rho tends to 2 a and the bound to 8 EPS while
            d(phi) / d(q) = 1 / (2 cos phi) grows again, so Newton's iteration on q itself cannot meet it (25 359 units at lat
            89.99 under lat_0 = -90 when it was tried).  The inverse therefore works in the angle from the NEARER pole, with
            (rho / a)^2 and q_p in two doubles on the far side: then it does (tests/prep_numpy.py pole_distance, pole_g).
            The first-order bound 16 EPS / cos(phi) is asserted beside it;
  longitude 4 EPS 360 degrees: atan2, the scaling to degrees, the addition of lon_0 and the wrap, one rounding each at a
            magnitude of at most 360."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import prep_numpy as pn
from gpsat_amd import _lib as L
from gpsat_amd import prep
from gpsat_amd.dataprep import DataPrep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
ASPECTS = [(lat_0, lon_0) for lat_0 in (90.0, -90.0) for lon_0 in (0.0, -45.0, 100.0)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "kat_ease2.npz")))
    assert len(g["lon"]) >= 290 and set(g["lat_0"]) == {90.0, -90.0}
    for lat_0 in (90.0, -90.0):                   # what the issue asks the set to hold
        lat = g["lat"][g["lat_0"] == lat_0]
        assert {90.0, -90.0, 89.9999999, 0.0} <= set(lat) and (lat * lat_0 < 0).sum() > 30
        assert {180.0, -180.0} <= set(g["lon"][g["lat_0"] == lat_0])
    return g


def forward_unit(x, y):
    rho = np.hypot(x, y)
    return EPS * (pn.A ** 2 / np.maximum(rho, 1e-3) + rho)


def inverse_unit(x, y):
    return EPS * pn.A / np.maximum(np.hypot(x, y), 1.0)


def lon_diff(a, b):
    return np.abs((a - b + 180.0) % 360.0 - 180.0)


def golden_cases(g, project):
    """Per aspect of the golden file: (mask, forward result, inverse result on the rows that have one)."""
    for lat_0, lon_0 in ASPECTS:
        m = (g["lat_0"] == lat_0) & (g["lon_0"] == lon_0)
        ok = m & g["inv_ok"]
        yield lat_0, lon_0, m, ok, project("forward", g["lon"][m], g["lat"][m], lon_0, lat_0), \
            project("inverse", g["x"][ok], g["y"][ok], lon_0, lat_0)


def numpy_project(direction, a, b, lon_0, lat_0):
    return (pn.laea_forward if direction == "forward" else pn.laea_inverse)(a, b, lon_0, lat_0)


# ---- the reference's documented values
def test_documented_forward_value():
    x, y = pn.laea_forward(-105.01621, 39.57422)
    print("forward:", repr(float(x)), repr(float(y)))
    assert abs(x - -5254767.014984061) <= 1e-8 and abs(y - 1409604.1043472202) <= 1e-8


def test_documented_inverse_value():
    """PROJ's documented latitude lies 9.5e-10 degrees from the exact one (69.86894542320586, mpmath): its authalic series is
    truncated.  The bound is twice that."""
    lon, lat = pn.laea_inverse(1000000.0, 2000000.0)
    print("inverse:", repr(float(lon)), repr(float(lat)))
    assert abs(lon - 153.434948822922) <= 1e-12
    assert abs(lat - 69.86894542225777) <= 2e-9
    assert abs(lat - 69.86894542320586) <= 1e-12


# ---- mpmath
def test_forward_golden(golden):
    """Worst seen on the restatement: 3.9 units of EPS (a^2 / rho + rho)."""
    worst = 0.0
    for lat_0, lon_0, m, ok, (x, y), _ in golden_cases(golden, numpy_project):
        err = np.maximum(np.abs(x - golden["x"][m]), np.abs(y - golden["y"][m])) / forward_unit(golden["x"][m], golden["y"][m])
        worst = max(worst, err.max())
    print("forward worst units:", worst)
    assert worst <= 16.0


def inverse_errors(golden, project):
    """Latitude error in radians, the issue's unit and cos(phi), longitude error in degrees, own-hemisphere flag: all rows."""
    rows = []
    for lat_0, lon_0, m, ok, _, (lon, lat) in golden_cases(golden, project):
        gx, gy, glat, glon = (golden[k][ok] for k in ("x", "y", "inv_lat", "inv_lon"))
        rows.append(np.stack([np.abs(np.radians(lat - glat)), inverse_unit(gx, gy), np.cos(np.radians(glat)),
                              np.where(np.hypot(gx, gy) > 0, lon_diff(lon, glon), np.abs(lon - lon_0)), (glat * lat_0 >= 0).astype(float)]))
    return np.concatenate(rows, axis=1)


def test_inverse_golden_own_hemisphere(golden):
    """The issue's bound where it was derived: the hemisphere of the projection's pole, the equator included.  Worst seen on
    the restatement: 1.6 units of EPS a / rho."""
    err, unit, _, _, own = inverse_errors(golden, numpy_project)
    units = (err / unit)[own > 0]
    print("inverse, own hemisphere, worst units:", units.max(), "of", len(units), "points")
    assert len(units) > 150 and units.max() <= 16.0


def test_inverse_golden_opposite_hemisphere(golden):
    """The same bound, 16 EPS a / rho, on the points beyond the equator, where it tends to 8 EPS: it needs 2 q_p - (rho / a)^2
    to twice the working precision.  Worst seen on the restatement: 2.4 units."""
    err, unit, _, _, own = inverse_errors(golden, numpy_project)
    units = (err / unit)[own == 0]
    print("inverse, opposite hemisphere, worst units:", units.max(), "of", len(units), "points")
    assert units.max() <= 16.0


def test_inverse_golden_first_order_bound(golden):
    """Every point of the golden file, both hemispheres: |d phi| <= 16 EPS / cos(phi), phi the golden latitude (cos floored at
    that of 1 m from a pole).  Towards the projection's own pole cos(phi) -> rho / a and this is the issue's bound.  Worst seen
    on the restatement: 1.3 units.  Longitude: 4 EPS 360 degrees, worst seen 2.9e-14."""
    err, _, cosphi, dlon, _ = inverse_errors(golden, numpy_project)
    units = err / (EPS / np.maximum(cosphi, 1.0 / pn.A))
    print("inverse, all points, worst units of EPS / cos(phi):", units.max(), "longitude:", dlon.max())
    assert units.max() <= 16.0
    assert dlon.max() <= 4 * EPS * 360.0


def test_special_values():
    nan, inf = np.nan, np.inf
    for lat_0 in (90.0, -90.0):
        x, y = pn.laea_forward([10.0, nan, 20.0, 30.0], [80.0, 70.0, nan, 60.0 * np.sign(lat_0)], 0.0, lat_0)
        assert np.isnan(x[1:3]).all() and np.isnan(y[1:3]).all() and np.isfinite(x[[0, 3]]).all()
        x, y = pn.laea_forward(33.0, lat_0, 12.0, lat_0)
        assert x == 0.0 and y == 0.0
        lon, lat = pn.laea_inverse([0.0, nan, 1e6, 2e7, 1.0], [0.0, 1.0, nan, 0.0, inf], 12.0, lat_0)
        assert (lon[0], lat[0]) == (12.0, lat_0)
        assert np.isnan(lon[1:3]).all() and np.isnan(lat[1:3]).all()
        assert np.isposinf(lon[3:]).all() and np.isposinf(lat[3:]).all()


@pytest.mark.parametrize("lat_0", [90.0, -90.0])
def test_round_trip(lat_0):
    """inverse(forward(lon, lat)): the forward's error in rho, k EPS (a^2 / rho + rho), moves phi by that over
    d(rho) / d(phi) = a^2 cos(phi) / rho (to first order in e^2), at most 3 k EPS / cos(phi) inside the disc; with the
    inverse's own 16: 64 EPS / cos(phi).  The far cap beyond 60 degrees of the other hemisphere is left to the golden points."""
    rng = np.random.default_rng(7)
    n = 20000
    lon = rng.uniform(-180.0, 180.0, n)
    lat = np.degrees(np.arcsin(rng.uniform(-np.sin(np.radians(60.0)), 1.0, n))) * np.sign(lat_0)
    lat[:4] = [lat_0, np.sign(lat_0) * 89.9999999, 0.0, -np.sign(lat_0) * 60.0]
    for lon_0 in (0.0, 100.0):
        x, y = pn.laea_forward(lon, lat, lon_0, lat_0)
        lo, la = pn.laea_inverse(x, y, lon_0, lat_0)
        units = np.abs(np.radians(la - lat)) / (EPS / np.maximum(np.cos(np.radians(lat)), 1.0 / pn.A))
        far = np.hypot(x, y) > 1.0
        print("round trip", lat_0, lon_0, "worst units:", units.max(), "longitude:", lon_diff(lo, lon)[far].max())
        assert units.max() <= 64.0
        assert lon_diff(lo, lon)[far].max() <= 8 * EPS * 360.0
        assert la[0] == lat_0 and lo[0] == lon_0


# ---- tracks
def one_pass_tracks(cols, codes, cut_off, start_track):
    """The rule the kernels implement, vectorised: a stable sort by code, distances inside groups, flags, one prefix sum."""
    cols = np.asarray(cols, dtype=np.float64).reshape(len(cols), -1)
    n = len(cols)
    codes = np.zeros(n, dtype=np.int64) if codes is None else np.asarray(codes, dtype=np.int64)
    key = np.where(codes < 0, codes.max(initial=-1) + 1, codes)
    order = np.argsort(key, kind="stable")
    k, c = key[order], cols[order]
    valid = codes[order] >= 0
    head = np.r_[True, k[1:] != k[:-1]]
    delta = np.full(n, np.nan)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((c[1:] - c[:-1]) ** 2).sum(axis=1))
    delta[1:] = d
    delta[head | ~valid] = np.nan
    with np.errstate(invalid="ignore"):
        flag = valid & ((delta > cut_off) | (head & (np.arange(n) > 0)))
    track = np.where(valid, start_track + np.cumsum(flag), -1)
    return order, delta, track


def sorted_rows(rng, n, n_groups, n_cols=2, null_every=0):
    """Rows as they look after sort_values: a slow drift with a jump every 20-odd rows; groups interleaved at random and
    numbered in order of first appearance, some rows in no group."""
    step = rng.uniform(0.5, 1.5, (n, n_cols))
    step[rng.random(n) < 0.05] += 50.0
    cols = np.cumsum(step, axis=0)
    raw = rng.integers(0, n_groups, n)
    _, first = np.unique(raw, return_index=True)
    rank = np.empty(n_groups, dtype=np.int64)
    rank[raw[np.sort(first)]] = np.arange(len(first))
    codes = rank[raw]
    if null_every:
        codes[::null_every] = -1
        codes = pd.factorize(np.where(codes < 0, np.nan, codes.astype(float)))[0]
    return cols, codes


@pytest.mark.parametrize("n_groups, null_every, start_track", [(1, 0, 0), (2, 0, 3), (27, 0, 0), (27, 7, 5), (2, 2, 1)])
def test_one_pass_rule_is_the_group_loop(n_groups, null_every, start_track):
    rng = np.random.default_rng(100 + n_groups + null_every)
    cols, codes = sorted_rows(rng, 3000, n_groups, null_every=null_every)
    cut = 20.0
    order, delta, track = pn.tracks_by_group(cols, codes if n_groups > 1 or null_every else None, cut, start_track)
    o2, d2, t2 = one_pass_tracks(cols, codes, cut, start_track)
    assert np.array_equal(order, o2) and np.array_equal(track, t2)
    assert np.array_equal(np.isnan(delta), np.isnan(d2)) and np.allclose(delta, d2, rtol=4 * EPS, atol=0, equal_nan=True)
    n_in = int((codes >= 0).sum())
    assert track[:n_in].min() == start_track and (np.diff(track[:n_in]) >= 0).all() and (track[n_in:] == -1).all()
    assert track[:n_in].max() > start_track + n_groups         # jumps were found, not only group starts


def test_prep_module_on_the_stand_in_engine():
    eng = pn.NumpyPrepEngine()
    x, y = prep.WGS84toEASE2(-105.01621, 39.57422, engine=eng)
    assert isinstance(x, float) and abs(x - -5254767.014984061) <= 1e-8 and abs(y - 1409604.1043472202) <= 1e-8
    assert prep.WGS84toEASE2(-105.01621, 39.57422, return_vals="y", engine=eng) == y
    lon = prep.EASE2toWGS84(np.array([[1e6, 0.0], [0.0, -1e6]]), np.array([[2e6, 1e6], [-1e6, 0.0]]), return_vals="lon", lon_0=10, engine=eng)
    assert lon.shape == (2, 2) and abs(lon[0, 0] - 163.434948822922) <= 1e-12
    with pytest.warns(DeprecationWarning):
        assert prep.WGS84toEASE2_New(0.0, -80.0, lat_0=-90, engine=eng) == prep.WGS84toEASE2(0.0, -80.0, lat_0=-90, engine=eng)
    with pytest.warns(DeprecationWarning):
        prep.EASE2toWGS84_New(0.0, 1.0, engine=eng)
    with pytest.raises(AssertionError):
        prep.WGS84toEASE2(0.0, 0.0, return_vals="lon", engine=eng)
    xy = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0], [np.nan, 1.0], [0.0, 1.0]])
    d = prep.diff_distance(xy, engine=eng)
    assert np.isnan(d[0]) and d[1] == 5.0 and d[2] == 0.0 and np.isnan(d[3:]).all()
    assert prep.diff_distance(xy[:, 0], default_val=-1.0, engine=eng)[0] == -1.0
    for kw in (dict(p=1), dict(k=2), dict(p=2.5)):
        with pytest.raises(NotImplementedError):
            prep.diff_distance(xy, engine=eng, **kw)
    with pytest.raises(NotImplementedError):
        prep.diff_distance(np.zeros((4, 4)), engine=eng)
    t = prep.guess_track_num(np.array([np.nan, 1.0, 7.0, 2.0, 7.0, 7.0]), 5.0, start_track=3, engine=eng)
    assert t.dtype == np.float64 and t.tolist() == [3, 3, 4, 4, 5, 6]
    r = prep.track_num_for_date(np.array([5, 5, 5, 6, 7, 7], dtype=np.int64), engine=eng)
    assert r.dtype == np.float64 and r.tolist() == [0, 1, 2, 0, 0, 1]
    with pytest.raises(NotImplementedError):
        prep.track_num_for_date(np.array([2 ** 53 + 1, 0], dtype=np.int64), engine=eng)


# ---- DataPrep.assign_tracks, host logic
def satellite_frame(rng, n_per=400, sats=("S3A", "CS2", "S3B"), null_every=0):
    """Three "satellites" on crossing orbits around the pole, a 10-minute gap (and a jump in position) every ~90 rows, rows of
    the satellites interleaved in time; returned shuffled."""
    frames = []
    for k, sat in enumerate(sats):
        gap = rng.random(n_per) < 1.0 / 90
        gap[:120] = False                                   # the first track runs from 23:59:00 past midnight
        secs = np.cumsum(np.where(gap, 600.0, 1.0)) + 0.25 * k
        phase = np.cumsum(np.where(gap, 1.3, 0.0009)) + k
        frames.append(pd.DataFrame({"datetime": np.datetime64("2020-03-01T23:59:00") + (secs * 1000).astype("timedelta64[ms]"),
                                    "lon": (phase * 57.0 * (k + 1)) % 360.0 - 180.0, "lat": 75.0 + 12.0 * np.sin(phase),
                                    "sat": sat, "z": rng.normal(size=n_per)}))
    df = pd.concat(frames, ignore_index=True)
    if null_every:
        df.loc[::null_every, "sat"] = None
    return df.sample(frac=1.0, random_state=3)


def reference_like(df, get_track_by, delta_measure, cut_off, start_track, lon_0=0, lat_0=90):
    """What TrackId computes, spelled with the restatement: xyt columns, the sort, per group the two distances and the
    tracks."""
    df = df.copy()
    df["t"] = df["datetime"].values.astype("datetime64[ms]").astype(float)
    df["x"], df["y"] = pn.laea_forward(df["lon"].to_numpy(), df["lat"].to_numpy(), lon_0, lat_0)
    df.sort_values("datetime", inplace=True)
    parts = []
    groups = [None] if get_track_by is None else [u for u in df[get_track_by].unique() if u is not None and u == u]
    for u in groups:
        part = df if u is None else df.loc[df[get_track_by] == u].copy()
        part = part.copy()
        part["dr"] = pn.diff_distance(part[["x", "y"]].to_numpy())
        part["dt"] = pn.diff_distance(part["t"].to_numpy())
        part["track"] = pn.guess_track_num(part[delta_measure].to_numpy(), cut_off, start_track).astype(int)
        start_track = part["track"].max() + 1
        parts.append(part)
    return pd.concat(parts)


@pytest.mark.parametrize("get_track_by, delta_measure, null_every", [("sat", "dr", 0), ("sat", "dt", 0), (None, "dr", 0), ("sat", "dr", 5)])
def test_assign_tracks_host_logic(get_track_by, delta_measure, null_every):
    df = satellite_frame(np.random.default_rng(11), null_every=null_every)
    before = df.copy()
    cut = 600_000 if delta_measure == "dr" else 60_000
    out = DataPrep.assign_tracks(df, sort_by="datetime", get_track_by=get_track_by, delta_measure=delta_measure, cut_off=cut,
                                 start_track=2, engine=pn.NumpyPrepEngine())
    pd.testing.assert_frame_equal(df, before)                               # the caller's frame is left alone
    want = reference_like(df, get_track_by, delta_measure, cut, 2)
    assert list(out.columns) == ["datetime", "lon", "lat", "sat", "z", "t", "x", "y", "dr", "dt", "track"]
    assert list(out.columns) == list(want.columns)
    assert np.array_equal(out.index.to_numpy(), want.index.to_numpy())      # the reference's row order, the source index kept
    pd.testing.assert_frame_equal(out, want)
    assert len(out) == len(df) - (df["sat"].isna().sum() if get_track_by else 0)
    if get_track_by:
        assert out["sat"].notna().all()
        assert list(out["sat"].drop_duplicates()) == list(df.sort_values("datetime")["sat"].dropna().drop_duplicates())
        per = out.groupby("sat", sort=False)["track"].agg(["min", "max"])
        assert per["min"].iloc[0] == 2 and (per["min"].to_numpy()[1:] == per["max"].to_numpy()[:-1] + 1).all()
    assert out["track"].nunique() > 6


def test_assign_tracks_by_track_date_spans_midnight():
    """A track that starts before midnight and ends after it belongs to the day it started on; the count of tracks per
    day restarts in every group."""
    df = satellite_frame(np.random.default_rng(5), n_per=1500)
    out = DataPrep.assign_tracks(df, sort_by=["datetime"], get_track_by="sat", delta_measure="dt", cut_off=60_000,
                                 add_by_track_date=True, engine=pn.NumpyPrepEngine())
    assert list(out.columns)[-3:] == ["track", "start_date", "track_start"] and len(out) == len(df)
    assert isinstance(out.index, pd.RangeIndex)
    days = out["datetime"].values.astype("datetime64[D]")
    spans = out.groupby("track")["datetime"].agg(["min", "max"])
    crossing = spans.index[spans["min"].values.astype("datetime64[D]") != spans["max"].values.astype("datetime64[D]")]
    assert len(crossing) >= 1                                               # every satellite's first track
    for tr, rows in out.groupby("track"):
        assert rows["start_date"].nunique() == 1 and rows["track_start"].nunique() == 1
        assert rows["start_date"].iloc[0] == rows["datetime"].min().floor("D")
    assert (out["start_date"].values.astype("datetime64[D]") != days).any()  # rows after midnight that belong to the day before
    for sat, rows in out.groupby("sat", sort=False):
        per_track = rows.drop_duplicates("track")
        want = pn.track_num_for_date(per_track["start_date"].values.astype("datetime64[D]").astype("int64"))
        assert per_track["track_start"].tolist() == want.astype(int).tolist()
        assert per_track["track_start"].iloc[0] == 0 and per_track["track_start"].max() >= 1


def test_assign_tracks_refusals():
    df = satellite_frame(np.random.default_rng(1), n_per=20)
    eng = pn.NumpyPrepEngine()
    with pytest.raises(AssertionError):
        DataPrep.assign_tracks(df, sort_by="datetime", delta_measure="dx", engine=eng)
    with pytest.raises(AssertionError):
        DataPrep.assign_tracks(df, sort_by=None, engine=eng)
    with pytest.raises(AssertionError):
        DataPrep.assign_tracks(df.drop(columns="lat"), sort_by="datetime", engine=eng)
    with pytest.raises(NotImplementedError):
        DataPrep.assign_tracks(df, sort_by="datetime", get_track_by=["sat", "z"], engine=eng)


# ---- ABI and refusals
def test_prep_struct_layout_matches_c(tmp_path):
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gpsat_hip.h"', 'int main(){']
    for st, cls in (("gpsat_project", L.GpsatProject), ("gpsat_track", L.GpsatTrack)):
        prog.append(f'printf("%zu\\n", sizeof({st}));')
        prog += [f'printf("%zu\\n", offsetof({st}, {f[0]}));' for f in cls._fields_]
    prog.append('printf("%d %d %d %d %d %d\\n", GPSAT_PROJECT_FORWARD, GPSAT_PROJECT_INVERSE, GPSAT_TRACK_CUT, GPSAT_TRACK_RUNS, '
                'GPSAT_TRACK_GIVEN, GPSAT_ABI_VERSION); return 0;}')
    cfile, exe = tmp_path / "layout.c", tmp_path / "layout"
    cfile.write_text("\n".join(prog))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    for cls in (L.GpsatProject, L.GpsatTrack):
        assert vals.pop(0) == C.sizeof(cls)
        for f in cls._fields_:
            assert vals.pop(0) == getattr(cls, f[0]).offset, (cls.__name__, f[0])
    assert vals == [L.PROJECT_IDS["forward"], L.PROJECT_IDS["inverse"], L.TRACK_MODES["cut"], L.TRACK_MODES["runs"],
                    L.TRACK_MODES["given"], L.ABI_VERSION]
    assert C.sizeof(L.GpsatProject) == 96 and C.sizeof(L.GpsatTrack) == 120
    assert {"gpsat_project_batch", "gpsat_track_batch"} <= set(L.OPTIONAL_EXPORTS)


def _checks():
    lib = L.load()
    cp = getattr(lib, "_ZN5gpsat13check_projectEPK13gpsat_projectPcm")
    cp.restype, cp.argtypes = C.c_int, [C.POINTER(L.GpsatProject), C.c_char_p, C.c_size_t]
    ct = getattr(lib, "_ZN5gpsat11check_trackEPK11gpsat_trackPyPcm")
    ct.restype, ct.argtypes = C.c_int, [C.POINTER(L.GpsatTrack), C.POINTER(C.c_ulonglong), C.c_char_p, C.c_size_t]
    return cp, ct


def test_refusals_of_the_exported_checks():
    """gpsat::check_project / gpsat::check_track are what the entry points call first: every refusal the header documents, with a
    message that names the reason, and nothing refused that it allows."""
    cp, ct = _checks()
    buf = C.create_string_buffer(160)
    a = np.ones(8)
    o = np.empty(8)
    grp = np.array([0, 0, 1, -1, 1, 2, 0, 5], dtype=np.int32)
    it, io = np.empty(8, dtype=np.int32), np.empty(8, dtype=np.int32)

    def project(**kw):
        p = L.GpsatProject(n=8, direction=0, memory=0, lon_0=0.0, lat_0=90.0, in0=a.ctypes.data, in1=a.ctypes.data,
                           out0=o.ctypes.data, out1=o.ctypes.data)
        for k, v in kw.items():
            setattr(p, k, v)
        return cp(C.byref(p), buf, 160), buf.value.decode()

    assert project() == (0, "")
    assert project(lat_0=-90.0, direction=1, memory=1) == (0, "")
    assert project(n=0, in0=None, in1=None, out0=None, out1=None) == (0, "")
    for kw, word in ((dict(lat_0=45.0), "lat_0"), (dict(lat_0=float("nan")), "lat_0"), (dict(lon_0=float("inf")), "lon_0"),
                     (dict(lon_0=float("nan")), "lon_0"), (dict(direction=2), "direction"), (dict(memory=3), "memory"),
                     (dict(n=-1), "negative"), (dict(n=2 ** 31), "2^31-1"), (dict(in0=None), "NULL"), (dict(out1=None), "NULL")):
        rc, msg = project(**kw)
        assert rc == -1 and msg.startswith("gpsat_project_batch: ") and word in msg, (kw, msg)
    p = L.GpsatProject(n=0, lat_0=90.0)
    p.reserved[7] = 1
    assert cp(C.byref(p), buf, 160) == -1 and b"reserved" in buf.value

    sentinel = C.c_ulonglong(7)

    def track(**kw):
        t = L.GpsatTrack(n=8, n_cols=2, memory=0, group=grp.ctypes.data, cut_off=6e5, start_track=0, mode=0,
                         out_delta=o.ctypes.data, out_track=it.ctypes.data, out_order=io.ctypes.data)
        t.cols[0] = t.cols[1] = a.ctypes.data
        for k, v in kw.items():
            setattr(t, k, v)
        return ct(C.byref(t), C.byref(sentinel), buf, 160), buf.value.decode()

    assert track() == (0, "") and sentinel.value == 6
    assert track(group=None) == (0, "") and sentinel.value == 2 ** 31
    assert track(memory=1) == (0, "") and sentinel.value == 2 ** 31
    assert track(mode=1, n_cols=1, cut_off=float("nan"), start_track=-1, out_delta=None) == (0, "")
    assert track(mode=2, n_cols=1) == (0, "")
    for kw, word in ((dict(n_cols=0), "n_cols"), (dict(n_cols=4), "n_cols"), (dict(mode=1), "one column"), (dict(mode=2), "one column"),
                     (dict(mode=3), "mode"), (dict(memory=2), "memory"), (dict(cut_off=float("nan")), "cut_off"),
                     (dict(cut_off=float("-inf")), "cut_off"), (dict(start_track=-1), "start_track"),
                     (dict(start_track=2 ** 31 - 8), "int32"), (dict(n=-1), "negative"), (dict(n=2 ** 31, memory=1), "2^31-1"),
                     (dict(out_delta=None), "out_delta"), (dict(out_track=None), "NULL"), (dict(out_order=None), "NULL")):
        rc, msg = track(**kw)
        assert rc == -1 and msg.startswith("gpsat_track_batch: ") and word in msg, (kw, msg)
    grp[6] = -2
    rc, msg = track()
    assert rc == -1 and "group[6] = -2" in msg
    assert track(memory=1)[0] == 0               # device mode does not read the codes
    grp[6] = 0
    t = L.GpsatTrack(n=0, n_cols=1)
    t.reserved[0] = 1
    assert ct(C.byref(t), None, buf, 160) == -1 and b"reserved" in buf.value


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_plan_header_under_the_host_sanitizers(tmp_path):
    """tests/prep_plan_host_check.cpp, its own main, built with the address and undefined-behaviour sanitizers and run directly:
    the launch geometry at n = 0, 1, B - 1, B, B + 1, B^2 + 1 and 2^31 - 1, the buffer layout, every refusal."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "prep_plan_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gpsat_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "prep_plan_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip(f"{cxx} has no sanitizer runtime: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    B = L.load()._ZN5gpsat15prep_scan_blockEv()
    assert B == 256
    r = subprocess.run([exe, str(B)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "done 0"
    blocks = {int(l.split()[1]): int(l.split()[2]) for l in lines if l.startswith("blocks ")}
    assert {0, 1, B - 1, B, B + 1, B * B + 1, 2 ** 31 - 1} <= set(blocks)
    assert all(v == -(-n // B) for n, v in blocks.items())
    scan = {int(l.split()[1]): tuple(map(int, l.split()[2:])) for l in lines if l.startswith("scan ")}
    assert scan[B * B] == (B, 1) and scan[B * B + 1] == (B + 1, 2) and scan[2 ** 31 - 1] == (2 ** 23, 2 ** 15)
    const = [float(v) for v in next(l for l in lines if l.startswith("const ")).split()[1:]]
    assert const == [pn.E2, pn.E, pn.INV_2E, pn.QP, pn.QP_LO]           # the host's constants are the restatement's, bit for bit
    assert sum(l.startswith("refuse project") for l in lines) >= 19 and sum(l.startswith("refuse track") for l in lines) >= 25
    key_runs = {int(l.split()[1]): tuple(map(int, l.split()[2:])) for l in lines if l.startswith("key_runs ")}
    assert sorted(key_runs) == [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024]
    assert key_runs[63] == (1008, 504, 256 + 256 + 63, 256, 272, 512) and key_runs[64] == (1024, 512, 512 + 256 + 64, 512, 528, 768)
