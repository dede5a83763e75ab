"""GPU: device binning (gpsat_bin.hip through gpsat_bin_batch, Engine.bin_batch, DataPrep) against
scipy.stats.binned_statistic(_2d) called here.  Equality is np.array_equal(..., equal_nan=True): bit for bit, no tolerance.
scipy's sums are sequential fp64 additions in source row order (np.bincount); the values span +-1e3 so that any other order
of additions changes bits (test_summation_order_is_visible confirms it for the seeds used)."""
import numpy as np
import pandas as pd
import pytest
from scipy import stats as scst

pytestmark = pytest.mark.gpu

STATS = ["count", "sum", "mean", "std", "min", "max", "median"]
EMPTY = {"count": 0.0, "sum": 0.0}


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import default_engine
    return default_engine()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def rows(R, seed, lo=-100.0, hi=100.0):
    """R rows, some of them outside [lo, hi] on either axis, values spanning +-1e3."""
    rng = np.random.default_rng(seed)
    w = hi - lo
    return rng.uniform(lo - 0.05 * w, hi + 0.05 * w, R), rng.uniform(lo - 0.05 * w, hi + 0.05 * w, R), rng.uniform(-1e3, 1e3, R)


def ref_dense(x, y, v, stat, ex, ey=None):
    """The reference's bin_data: scipy's statistic, transposed."""
    if ey is None:
        return scst.binned_statistic(x, v, statistic=stat, bins=ex, range=[ex[0], ex[-1]]).statistic.T
    return scst.binned_statistic_2d(x, y, v, statistic=stat, bins=[ex, ey],
                                    range=[[ex[0], ex[-1]], [ey[0], ey[-1]]]).statistic.T


def dense(res, stat, ex, ey=None):
    shape = (len(ey) - 1, len(ex) - 1) if ey is not None else (len(ex) - 1,)
    out = np.full(shape, EMPTY.get(stat, np.nan))
    out[(res.iy, res.ix) if ey is not None else (res.ix,)] = res.stats[stat]
    return out


def check_all(eng, x, y, v, ex, ey, stats=STATS):
    res = eng.bin_batch(x, y, v, None, 1, ex, ey, stats)
    assert np.all(np.diff(res.keys) > 0)
    for s in stats:
        ref = ref_dense(x, y, v, s, ex, ey)
        got = dense(res, s, ex, ey)
        assert same(got, ref), (s, int(np.sum(~((got == ref) | (np.isnan(got) & np.isnan(ref))))))
    if len(res.keys):
        n_ref = ref_dense(x, y, v, "count", ex, ey)
        assert len(res.keys) == np.count_nonzero(n_ref)
    return res


def test_summation_order_is_visible():
    """The test can fail: on these values a reversed or a pairwise sum differs from scipy's sequential one in some cell."""
    x, y, v = rows(200_000, 200_000)
    ex = np.linspace(-100, 100, 11)
    ref = scst.binned_statistic_2d(x, y, v, statistic="mean", bins=[ex, ex], expand_binnumbers=False)
    seq, rev, pair = np.zeros(144), np.zeros(144), np.zeros(144)
    for b in np.unique(ref.binnumber):
        vb = v[ref.binnumber == b]
        s = 0.0
        for t in vb:
            s += t
        r = 0.0
        for t in vb[::-1]:
            r += t
        seq[b], rev[b], pair[b] = s / len(vb), r / len(vb), np.sum(vb) / len(vb)      # np.sum: pairwise
    core = seq.reshape(12, 12)[1:-1, 1:-1]
    assert same(core, ref.statistic)                                                  # scipy IS the sequential sum
    assert not same(rev.reshape(12, 12)[1:-1, 1:-1], ref.statistic)
    assert not same(pair.reshape(12, 12)[1:-1, 1:-1], ref.statistic)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000, 200_000])
@pytest.mark.parametrize("nb", [10, 180])
def test_2d_every_statistic(eng, R, nb):
    x, y, v = rows(R, R + nb)
    check_all(eng, x, y, v, np.linspace(-100, 100, nb + 1), np.linspace(-100, 100, nb + 1))


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000, 200_000])
@pytest.mark.parametrize("nb", [10, 180])
def test_1d_every_statistic(eng, R, nb):
    x, _, v = rows(R, 7 * R + nb)
    check_all(eng, x, None, v, np.linspace(-100, 100, nb + 1), None)


def test_rectangular_grid_and_production_edges(eng):
    """x_range != y_range (the dense form is (ny - 1, nx - 1)), and the published 50 km grid."""
    rng = np.random.default_rng(3)
    R = 50_000
    x, y, v = rng.uniform(-120, 120, R), rng.uniform(-10, 70, R), rng.uniform(-1e3, 1e3, R)
    check_all(eng, x, y, v, np.linspace(-100, 100, 11), np.linspace(0, 60, 4))
    x, y = rng.uniform(-4.6e6, 4.6e6, R), rng.uniform(-4.6e6, 4.6e6, R)
    e = np.linspace(-4.5e6, 4.5e6, 181)
    check_all(eng, x, y, v, e, e, ["mean", "std", "count"])


@pytest.mark.parametrize("lo,hi,n", [(-100.0, 100.0, 11), (-4.5e6, 4.5e6, 181), (0.0, 1.0, 11), (-0.5, 0.25, 751)])
def test_rows_on_the_edges(eng, lo, hi, n):
    """Rows exactly on interior edges, on the first and the last edge, within and just beyond scipy's rounding interval above
    the last edge, below the range, NaN and infinite coordinates, many duplicates of one coordinate."""
    from gpsat_amd.dataprep import right_edge_limit
    e = np.linspace(lo, hi, n)
    x_hi = right_edge_limit(e)

    def up(t, k=1):
        for _ in range(k):
            t = np.nextafter(t, np.inf)
        return t

    def dn(t, k=1):
        for _ in range(k):
            t = np.nextafter(t, -np.inf)
        return t

    special = np.concatenate([
        e, [up(t) for t in e], [dn(t) for t in e],                      # every edge and its two neighbours
        [x_hi, up(x_hi), dn(x_hi), up(x_hi, 5), 0.5 * (e[-1] + x_hi), e[-1] + 2 * (x_hi - e[-1])],
        [lo - 1.0, dn(lo, 3), hi + (hi - lo), np.nan, np.inf, -np.inf],
        np.full(500, e[3]), np.full(500, e[-1]), np.full(300, x_hi),     # duplicates
    ])
    rng = np.random.default_rng(n)
    x = rng.permutation(np.tile(special, 3))
    y = rng.permutation(np.tile(special, 3))
    v = rng.uniform(-1e3, 1e3, len(x))
    check_all(eng, x, y, v, e, e)
    check_all(eng, x, None, v, e, None)
    # the guess of the bin from (x - e0) / step alone would misplace edges: the kernel's answer is np.digitize's
    res = eng.bin_batch(e[:-1], None, np.ones(n - 1), None, 1, e, None, ["count"])
    assert same(res.ix, np.arange(n - 1)) and same(res.stats["count"], np.ones(n - 1))


def test_nan_values_follow_scipy(eng):
    """A cell holding [nan, 1, 2, 9]: count 4; mean, sum, std, max NaN; min 1; median (2 + 9) / 2 -- and the same on bulk data
    with NaNs of either sign bit."""
    ex = np.linspace(0, 4, 5)
    x = np.array([0.5, 0.5, 0.5, 0.5, 2.5, 3.5, 3.5])
    v = np.array([np.nan, 1.0, 2.0, 9.0, 4.0, np.nan, -np.nan])
    res = check_all(eng, x, None, v, ex, None)
    got = {s: res.stats[s][0] for s in STATS}
    assert got["count"] == 4 and got["min"] == 1.0 and got["median"] == 5.5
    assert all(np.isnan(got[s]) for s in ("mean", "sum", "std", "max"))
    assert np.isnan(res.stats["min"][2]) and np.isnan(res.stats["median"][2])        # a cell of NaNs only
    x, y, v = rows(20_000, 11)
    rng = np.random.default_rng(12)
    v[rng.random(len(v)) < 0.05] = np.nan
    v[rng.random(len(v)) < 0.05] = -np.nan
    v[rng.random(len(v)) < 0.01] = np.inf
    v[rng.random(len(v)) < 0.01] = -np.inf
    e = np.linspace(-100, 100, 11)
    with np.errstate(invalid="ignore"):
        check_all(eng, x, y, v, e, e)


def test_one_cell_and_one_row_per_cell(eng):
    R = 200_000
    rng = np.random.default_rng(8)
    e = np.linspace(-100, 100, 11)
    x, y, v = rng.uniform(20, 40, R), rng.uniform(-60, -40, R), rng.uniform(-1e3, 1e3, R)
    res = check_all(eng, x, y, v, e, e)
    assert len(res.keys) == 1 and res.stats["count"][0] == R
    n = 180
    e = np.linspace(-100, 100, n + 1)
    c = e[:-1] + np.diff(e) / 2
    xx, yy = np.meshgrid(c, c)
    p = rng.permutation(n * n)
    x, y = xx.ravel()[p], yy.ravel()[p]
    v = rng.uniform(-1e3, 1e3, n * n)
    res = check_all(eng, x, y, v, e, e)
    assert len(res.keys) == n * n and np.all(res.stats["count"] == 1) and np.all(res.stats["std"] == 0)


def test_long_cells_are_walked_by_a_wave_with_the_same_bits(eng):
    """Cells of 1 024 rows or more take another code path (one wave per cell, 64 values per load): row counts either side of
    that limit and of the multiples of 64, NaN values in long cells."""
    counts = [1023, 1024, 1025, 1087, 1088, 1089, 5000, 6400, 1, 64]
    e = np.linspace(0.0, len(counts), len(counts) + 1)
    rng = np.random.default_rng(77)
    x = rng.permutation(np.repeat(np.arange(len(counts)) + 0.5, counts))
    v = rng.uniform(-1e3, 1e3, len(x))
    res = check_all(eng, x, None, v, e, None)
    assert same(res.stats["count"], np.array(counts, dtype=float))
    y = rng.uniform(0.0, 2.0, len(x))
    check_all(eng, x, y, v, e, np.linspace(0.0, 2.0, 3))
    v[rng.random(len(v)) < 0.001] = np.nan
    v[(x > 7) & (x < 8)] = -np.nan                                    # a long cell of NaNs only
    with np.errstate(invalid="ignore"):
        check_all(eng, x, None, v, e, None)


def synthetic_frame(R, seed, days=9, sats=("CS2", "S3A", "S3B")):
    rng = np.random.default_rng(seed)
    x, y, v = rows(R, seed)
    day = np.datetime64("2020-03-01") + rng.integers(0, days, R).astype("timedelta64[D]")
    return pd.DataFrame({"x": x, "y": y, "z": v, "date": day, "sat": rng.choice(list(sats), R)})


def reference_bin_data_by(df, by_cols, val_col, x_range, y_range, grid_res, stats, bin_2d=True):
    """The reference's procedure, restated: per observed combination a mask over the whole frame, scipy, transpose, bin
    centres, drop the cells in which a statistic is NaN.  Returns rows keyed by (by values..., y, x)."""
    nx = int((x_range[1] - x_range[0]) / grid_res + 1)
    ny = int((y_range[1] - y_range[0]) / grid_res + 1)
    ex, ey = np.linspace(x_range[0], x_range[1], nx), np.linspace(y_range[0], y_range[1], ny)
    xc, yc = ex[:-1] + np.diff(ex) / 2, ey[:-1] + np.diff(ey) / 2
    out = {}
    for _, bcp in df[by_cols].drop_duplicates().iterrows():
        sel = np.ones(len(df), dtype=bool)
        for bc in by_cols:
            sel &= (df[bc] == bcp[bc]).values
        d = df.loc[sel]
        b = [ref_dense(d["x"].values, d["y"].values if bin_2d else None, d[val_col].values, s, ex, ey if bin_2d else None)
             for s in stats]
        keep = ~np.any([np.isnan(a) for a in b], axis=0)
        for idx in zip(*np.nonzero(keep)):
            pos = (yc[idx[0]], xc[idx[1]]) if bin_2d else (xc[idx[0]],)
            out[tuple(bcp[bc] for bc in by_cols) + pos] = tuple(a[idx] for a in b)
    return out


def frame_rows(out, by_cols, coord_cols, stat_cols):
    keys = list(zip(*[out[c].tolist() for c in by_cols + coord_cols]))
    vals = list(zip(*[out[c].to_numpy() for c in stat_cols]))
    assert len(set(keys)) == len(keys)
    return dict(zip(keys, vals))


@pytest.mark.parametrize("stats", ["mean", ["mean", "std", "count", "median"]])
def test_bin_data_by_27_groups(eng, stats):
    from gpsat_amd.dataprep import DataPrep
    df = synthetic_frame(60_000, 21)
    by = ["date", "sat"]
    out = DataPrep.bin_data_by(df, by_cols=by, val_col="z", x_range=[-100, 100], y_range=[-100, 60], grid_res=10,
                               bin_statistic=stats, return_df=True)
    slist = stats if isinstance(stats, list) else [stats]
    cols = ["z"] if isinstance(stats, str) else [f"z_{s}" for s in slist]
    assert list(out.columns) == by + ["y", "x"] + cols
    assert len(out[by].drop_duplicates()) == 27
    ref = reference_bin_data_by(df, by, "z", [-100, 100], [-100, 60], 10, slist)
    got = frame_rows(out, by, ["y", "x"], cols)
    assert set(got) == set(ref)
    for k, val in ref.items():
        assert same(np.array(got[k]), np.array(val)), k
    # this project's row order: by_cols ascending, then y, then x
    assert out.equals(out.sort_values(by + ["y", "x"], kind="stable").reset_index(drop=True))


def test_bin_data_by_1d_strings_and_row_select(eng):
    from gpsat_amd.dataprep import DataPrep
    df = synthetic_frame(20_000, 22)
    out = DataPrep.bin_data_by(df, by_cols="sat", val_col="z", x_range=[-100, 100], grid_res=5, bin_statistic=["min", "max"],
                               bin_2d=False, return_df=True, row_select=[{"col": "y", "comp": ">=", "val": 0.0}])
    assert list(out.columns) == ["sat", "x", "z_min", "z_max"]
    ref = reference_bin_data_by(df[df["y"] >= 0.0], ["sat"], "z", [-100, 100], [-4.5e6, 4.5e6], 5, ["min", "max"], bin_2d=False)
    got = frame_rows(out, ["sat"], ["x"], ["z_min", "z_max"])
    assert set(got) == set(ref)
    assert all(same(np.array(got[k]), np.array(ref[k])) for k in ref)


def test_bin_data_matches_the_reference_form(eng):
    from gpsat_amd.dataprep import DataPrep
    df = synthetic_frame(30_000, 23)
    for stat in STATS:
        b, (xo, yo) = DataPrep.bin_data(df, x_range=[-100, 100], y_range=[-50, 100], grid_res=7, val_col="z", bin_statistic=stat)
        ex, ey = np.linspace(-100, 100, int(200 / 7 + 1)), np.linspace(-50, 100, int(150 / 7 + 1))
        assert b.shape == (len(ey) - 1, len(ex) - 1)
        assert same(b, ref_dense(df["x"].values, df["y"].values, df["z"].values, stat, ex, ey))
        assert same(xo, ex[:-1] + np.diff(ex) / 2) and same(yo, ey[:-1] + np.diff(ey) / 2)
    b, xo = DataPrep.bin_data(df, x_range=[-100, 100], grid_res=7, val_col="z", bin_2d=False, return_bin_center=False)
    assert same(xo, ex) and same(b, ref_dense(df["x"].values, None, df["z"].values, "mean", ex))


def test_bits_do_not_depend_on_other_cells_or_the_batch(eng):
    """Shuffling the rows of different cells relative to each other while every cell keeps its internal order leaves every
    output bit unchanged; two identical calls return identical bytes; a batch equals the per-group results."""
    R, G = 100_000, 27
    x, y, v = rows(R, 31)
    rng = np.random.default_rng(32)
    gid = rng.integers(0, G, R).astype(np.int32)
    e = np.linspace(-100, 100, 21)
    a = eng.bin_batch(x, y, v, gid, G, e, e, STATS)
    b = eng.bin_batch(x, y, v, gid, G, e, e, STATS)
    assert a.keys.tobytes() == b.keys.tobytes() and all(a.stats[s].tobytes() == b.stats[s].tobytes() for s in STATS)
    # a permutation that keeps the source order inside every (group, cell): a stable sort by a random label per cell
    ix, iy = np.digitize(x, e), np.digitize(y, e)
    cell = (gid.astype(np.int64) * 32 + iy) * 32 + ix
    label = rng.permutation(cell.max() + 1)[cell]
    p = np.argsort(label, kind="stable")
    c = eng.bin_batch(x[p], y[p], v[p], gid[p], G, e, e, STATS)
    assert a.keys.tobytes() == c.keys.tobytes() and all(a.stats[s].tobytes() == c.stats[s].tobytes() for s in STATS)
    # a subset of the statistics from the same call
    d = eng.bin_batch(x, y, v, gid, G, e, e, ["std", "median"])
    assert all(a.stats[s].tobytes() == d.stats[s].tobytes() for s in ("std", "median"))
    # per group
    cells = 20 * 20
    for g in range(G):
        m = gid == g
        r = eng.bin_batch(x[m], y[m], v[m], None, 1, e, e, STATS)
        sel = a.gid == g
        assert same(a.keys[sel] - g * cells, r.keys) and same(a.iy[sel], r.iy) and same(a.ix[sel], r.ix)
        for s in STATS:
            assert a.stats[s][sel].tobytes() == r.stats[s].tobytes()
            assert same(dense(r, s, e, e), ref_dense(x[m], y[m], v[m], s, e, e))


def test_empty_inputs_and_groups(eng):
    from gpsat_amd.engine import GpsatError
    e = np.linspace(-100, 100, 11)
    z = np.zeros(0)
    r = eng.bin_batch(z, z, z, None, 1, e, e, STATS)
    assert len(r.keys) == 0 and all(len(r.stats[s]) == 0 for s in STATS)
    r = eng.bin_batch(z, z, z, np.zeros(0, np.int32), 0, e, e, ["mean"])
    assert len(r.keys) == 0
    # every row outside the grid
    r = eng.bin_batch(np.array([500.0, np.nan]), np.array([0.0, 0.0]), np.ones(2), None, 1, e, e, ["mean", "median"])
    assert len(r.keys) == 0
    # a group with no row inside the range; G = 1 without gid
    x, y, v = rows(5000, 41)
    gid = (np.arange(5000) % 3).astype(np.int32)
    x[gid == 1] = 1e4
    r = eng.bin_batch(x, y, v, gid, 3, e, e, ["mean"])
    assert sorted(np.unique(r.gid).tolist()) == [0, 2]
    for g in (0, 2):
        assert same(dense(eng.bin_batch(x[gid == g], y[gid == g], v[gid == g], None, 1, e, e, ["mean"]), "mean", e, e),
                    ref_dense(x[gid == g], y[gid == g], v[gid == g], "mean", e, e))
    # refused arguments
    with pytest.raises(GpsatError, match="gid"):
        eng.bin_batch(x, y, v, gid, 2, e, e, ["mean"])
    with pytest.raises(GpsatError, match="increasing"):
        eng.bin_batch(x, y, v, None, 1, e[::-1].copy(), e, ["mean"], x_hi=100.0)
    with pytest.raises(GpsatError, match="at least 2 edges"):
        eng.bin_batch(x, y, v, None, 1, e[:1], e, ["mean"], x_hi=0.0)
    with pytest.raises(GpsatError, match="statistics"):
        eng.bin_batch(x, y, v, None, 1, e, e, ["mode"])


def test_raw_rows_to_local_experts(eng, tmp_path):
    """Raw synthetic rows -> bin_data_by -> BatchedLocalExpertOI on the binned frame: it is a valid data_source."""
    from gpsat_amd.dataprep import DataPrep
    from gpsat_amd.local_experts import BatchedLocalExpertOI
    rng = np.random.default_rng(51)
    R = 40_000
    raw = pd.DataFrame({"x": rng.uniform(0, 1, R), "y": rng.uniform(0, 1, R), "t": rng.integers(0, 6, R).astype(float)})
    raw["z"] = np.sin(6 * raw["x"]) * np.cos(5 * raw["y"]) + 0.3 * np.sin(raw["t"]) + 0.3 * rng.normal(size=R)
    binned = DataPrep.bin_data_by(raw, by_cols="t", val_col="z", x_range=[0, 1], y_range=[0, 1], grid_res=0.05, return_df=True)
    assert list(binned.columns) == ["t", "y", "x", "z"] and 0 < len(binned) <= 6 * 20 * 20
    xl = pd.DataFrame({"x": [0.3, 0.7, 0.5], "y": [0.4, 0.6, 0.5], "t": [3.0, 2.0, 4.0]})
    oi = BatchedLocalExpertOI(
        expert_loc_config={"source": xl},
        data_config={"data_source": binned, "obs_col": "z", "coords_col": ["x", "y", "t"],
                     "local_select": [{"col": ["x", "y"], "comp": "<=", "val": 0.25}, {"col": "t", "comp": "<=", "val": 2.0},
                                      {"col": "t", "comp": ">=", "val": -2.0}]},
        model_config={"oi_model": "HipGPRModel", "init_params": {"kernel": "Matern32", "obs_mean": "local"},
                      "constraints": {"lengthscales": {"low": [1e-3] * 3, "high": [5.0] * 3}}},
        pred_loc_config={"method": "expert_loc"}, engine=eng, dtype="f64")
    tabs = oi.run(store_path=str(tmp_path / "binned"))
    rd, pr = tabs["run_details"], tabs["preds"]
    assert len(rd) == 3 and (rd["num_obs"] > 50).all()
    assert len(pr) == 3 and np.isfinite(pr["f*"].values).all() and (pr["f*_var"].values > 0).all()
