"""Binning of raw observations into the table the expert tiles draw from, on the GPU.

``DataPrep.bin_data`` / ``DataPrep.bin_data_by`` are the counterparts of the reference's methods of the same names
(GPSat/dataprepper.py:21-401): same argument names, defaults and assertions, the statistics of
``scipy.stats.binned_statistic(_2d)`` bit for bit.  Where the reference loops over the distinct values of ``by_cols``
(a boolean mask over the whole frame and one scipy call per group and statistic), all groups and statistics here go
through ONE ``gpsat_bin_batch`` call (``Engine.bin_batch``, gpsat_amd/csrc/gpsat_bin.hip).  The host only makes the
edges (``np.linspace``, never restated on the device), finds the inclusive limit of the last bin (scipy's rounded
right-edge rule, ``right_edge_limit``) and rank-codes the groups.  There is no host fallback: every number comes from
the device.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _lib as L

DEFAULT_RANGE = [-4500000.0, 4500000.0]
# what an empty cell holds in the dense form (scipy: count and sum 0, everything else NaN)
_EMPTY = {"count": 0.0, "sum": 0.0}


# ---- scipy's right edge ---------------------------------------------------------------------------------------------
def _to_ord(x) -> int:
    """Doubles -> integers in the same order (neighbouring doubles are neighbouring integers)."""
    i = int(np.float64(x).view(np.int64))
    return i if i >= 0 else -(i + 2 ** 63)


def _from_ord(k: int) -> float:
    return float(np.int64(k if k >= 0 else -k - 2 ** 63).view(np.float64))


def edge_decimals(edges) -> int:
    """The rounding precision of scipy's right-edge test (scipy/stats/_binned_statistic.py::_bin_numbers)."""
    dmin = np.diff(np.asarray(edges, dtype=np.float64)).min()
    if dmin == 0:
        raise ValueError("The smallest edge difference is numerically 0.")
    return int(-np.log10(dmin)) + 6


def right_edge_limit(edges) -> float:
    """Largest x that scipy still puts into the LAST bin: x >= edges[-1] with np.around(x, d) == np.around(edges[-1], d),
    d = edge_decimals(edges).  np.around is monotone, so those x are the interval [edges[-1], x_hi]; x_hi is found by
    bisection over the doubles with np.around itself."""
    edges = np.asarray(edges, dtype=np.float64)
    dec = edge_decimals(edges)
    last = float(edges[-1])
    target = np.around(np.array([last]), dec)[0]

    def on_edge(x):
        return bool(np.around(np.array([x]), dec)[0] == target)

    if not on_edge(last):          # rounding overflowed (NaN != NaN): scipy shifts nothing
        return last
    step = 10.0 ** (-dec)
    hi = last + step
    while on_edge(hi):
        step *= 2.0
        hi = last + step
        if not np.isfinite(hi):
            return float(np.finfo(np.float64).max)
    lo_k, hi_k = _to_ord(last), _to_ord(hi)
    while hi_k - lo_k > 1:
        mid = (lo_k + hi_k) // 2
        if on_edge(_from_ord(mid)):
            lo_k = mid
        else:
            hi_k = mid
    return _from_ord(lo_k)


# ---- grid -----------------------------------------------------------------------------------------------------------
def grid_edges(x_range, y_range, grid_res, bin_2d=True):
    """(x_edge, y_edge) as the reference makes them: int((max - min) / grid_res + 1) edges, np.linspace(min, max, n);
    default ranges +-4 500 000 with the reference's notice."""
    if x_range is None:
        x_range = list(DEFAULT_RANGE)
        print(f"x_range, not provided, using default: {x_range}")
    assert x_range[0] < x_range[1], f"x_range should be (min, max), got: {x_range}"
    if y_range is None:
        y_range = list(DEFAULT_RANGE)
        if bin_2d:
            print(f"y_range, not provided, using default: {y_range}")
    assert y_range[0] < y_range[1], f"y_range should be (min, max), got: {y_range}"
    assert len(x_range) == 2, f"x_range expected to be len = 2, got: {len(x_range)}"
    assert len(y_range) == 2, f"y_range expected to be len = 2, got: {len(y_range)}"
    n_x = int((x_range[1] - x_range[0]) / grid_res + 1)
    n_y = int((y_range[1] - y_range[0]) / grid_res + 1)
    return np.linspace(x_range[0], x_range[1], n_x), np.linspace(y_range[0], y_range[1], n_y)


def bin_centres(edge):
    return edge[:-1] + np.diff(edge) / 2


def _check_statistics(bin_statistic):
    stats = bin_statistic if isinstance(bin_statistic, list) else [bin_statistic]
    for s in stats:
        if callable(s):
            raise NotImplementedError("callable bin_statistic is not built: the device computes " + ", ".join(L.BIN_STATS))
        if s not in L.BIN_STATS:
            raise ValueError(f"invalid statistic {s!r}: choose from {list(L.BIN_STATS)}")
    assert len(stats) > 0, "bin_statistic is empty"
    return stats


def _stat_columns(stats, val_col):
    """Column of every statistic: val_col for a single one, f"{val_col}_{stat}" for a list."""
    return {s: (val_col if len(stats) == 1 else f"{val_col}_{s}") for s in stats}


# ---- groups ---------------------------------------------------------------------------------------------------------
def code_groups(df, by_cols):
    """Rank-code the observed combinations of ``by_cols``.

    Returns (gid [len(df)] int32, -1 where a by-column is null: such rows equal nothing, the reference's mask never selects
    them), the list of per-column value arrays of the G observed combinations in ascending (lexicographic) order, and
    the number of distinct combinations as the reference counts them (``drop_duplicates``: null combinations included)."""
    n = len(df)
    null = np.zeros(n, dtype=bool)
    hashed = []
    for bc in by_cols:
        # np.unique(column, return_inverse=True) without sorting every row: hash the rows to their distinct values
        # (pd.factorize, O(rows); None / NaN / NaT get -1), then rank the few distinct values with np.unique
        first, distinct = pd.factorize(df[bc].to_numpy())
        hashed.append((first, np.asarray(distinct)))
        null |= first < 0
    any_null = bool(null.any())
    ok = ~null
    uniq, codes = [], []
    for first, distinct in hashed:
        u, rank = np.unique(distinct, return_inverse=True)
        uniq.append(u)
        codes.append(np.asarray(rank, dtype=np.int64).reshape(-1)[first[ok] if any_null else first])
    combined = np.zeros(int(ok.sum()) if any_null else n, dtype=np.int64)
    for u, c in zip(uniq, codes):
        assert float(len(u)) * float(combined.max(initial=0) + 1) < 2.0 ** 62, "too many distinct by_cols values to code"
        combined = combined * max(len(u), 1) + c
    span = int(np.prod([max(len(u), 1) for u in uniq], dtype=np.float64))
    if 0 < span <= 1 << 24:                      # few possible combinations: a table instead of a sort of every row
        present = np.bincount(combined, minlength=span) > 0
        observed = np.flatnonzero(present)
        inv = (np.cumsum(present) - 1)[combined]
    else:
        observed, inv = np.unique(combined, return_inverse=True)
    gid = np.full(n, -1, dtype=np.int32)
    gid[ok] = np.asarray(inv).reshape(-1)
    values, rem = [], observed.copy()
    for u in reversed(uniq):                      # decode the mixed-radix code, last column first
        rem, c = np.divmod(rem, max(len(u), 1))
        values.append(u[c] if len(u) else u)
    values.reverse()
    n_null = len(df.loc[null, list(by_cols)].drop_duplicates()) if any_null else 0
    return gid, values, len(observed) + n_null


def _engine():
    from .engine import default_engine
    return default_engine()


class DataPrep:
    """Class / static methods that prepare (bin) data, as GPSat.dataprepper.DataPrep."""

    def __init__(self):
        pass

    @classmethod
    def bin_data_by(cls, df, col_funcs=None, row_select=None, by_cols=None, val_col=None, x_col='x', y_col='y',
                    x_range=None, y_range=None, grid_res=None, bin_statistic="mean", bin_2d=True, limit=10000,
                    return_df=False, verbose=False):
        """Bin ``val_col`` on a regular grid for every observed combination of ``by_cols``: ALL groups and statistics in
        one device call.

        ``return_df=True`` returns what users take from the reference, ``to_dataframe().dropna().reset_index()``: one row
        per non-empty cell with the columns by_cols..., y_col, x_col (bin centres; 1-D: x_col only) and one column per
        statistic (``val_col`` for a single statistic, f"{val_col}_{stat}" for a list), without the rows in which a
        statistic is NaN.  Row ORDER is this project's: by_cols ascending, then y, then x.  (With only count / sum asked
        for, no cell is NaN and the reference's dropna would also keep the empty cells with their zeros; they are not
        returned here.)  ``return_df=False`` builds the reference's xarray.Dataset when xarray is installed.
        ``row_select``: static {col, comp, val} entries; ``col_funcs`` and callable statistics are not built."""
        if col_funcs is None:
            col_funcs = {}
        assert isinstance(col_funcs, dict), f"col_funcs must be a dictionary, got type: {type(col_funcs)}"
        if col_funcs:
            raise NotImplementedError("col_funcs are not built (DESIGN.md §8): add the columns to df before the call")
        if bin_2d is False:
            y_col = x_col
        assert by_cols is not None, "by_col needs to be provided"
        if isinstance(by_cols, str):
            by_cols = [by_cols]
        assert isinstance(by_cols, (list, tuple)), f"by_cols must be list or tuple, got type: {type(by_cols)}"
        by_cols = list(by_cols)
        for bc in by_cols:
            assert bc in df, f"by_cols value: {bc} is not in df.columns: {df.columns}"
        assert val_col in df, f"val_col: {val_col} is not in df.columns: {df.columns}"
        assert x_col in df, f"x_col: {x_col} is not in df.columns: {df.columns}"
        assert y_col in df, f"y_col: {y_col} is not in df.columns: {df.columns}"
        assert grid_res is not None, "grid_res is None, must be supplied - expressed in km"
        stats = _check_statistics(bin_statistic)
        if not return_df:
            try:
                import xarray  # noqa: F401
            except ImportError:
                raise NotImplementedError("return_df=False returns an xarray.Dataset and xarray is not installed: "
                                          "call with return_df=True") from None
        if row_select is not None:
            from .local_experts import data_select
            df = data_select(df, row_select if isinstance(row_select, (list, tuple)) else [row_select])

        gid, group_vals, n_combos = code_groups(df, by_cols)
        assert n_combos < limit, f"number unique values of by_cols found in data: {n_combos} > limit: {limit} " \
                                 f"are you sure you want this many? if so increase limit"
        x_edge, y_edge = grid_edges(x_range, y_range, grid_res, bin_2d)
        G = len(group_vals[0]) if group_vals else 0
        keep = gid >= 0
        x = df[x_col].to_numpy(dtype=np.float64)
        y = df[y_col].to_numpy(dtype=np.float64) if bin_2d else None
        v = df[val_col].to_numpy(dtype=np.float64)
        if not keep.all():
            x, v, gid = x[keep], v[keep], gid[keep]
            y = y[keep] if bin_2d else None
        if verbose:
            print(f"bin_data_by: {len(x)} rows, {G} groups, grid {len(x_edge) - 1} x {len(y_edge) - 1 if bin_2d else 1}, "
                  f"statistics {stats}")
        res = _engine().bin_batch(x, y, v, gid, G, x_edge, y_edge if bin_2d else None, stats)
        names = _stat_columns(stats, val_col)
        xc, yc = bin_centres(x_edge), bin_centres(y_edge)
        if return_df:
            cols = {bc: gv[res.gid] for bc, gv in zip(by_cols, group_vals)}
            if bin_2d:
                cols[y_col] = yc[res.iy]
            cols[x_col] = xc[res.ix]
            ok = np.ones(len(res.keys), dtype=bool)
            for s in stats:
                cols[names[s]] = res.stats[s]
                ok &= ~np.isnan(res.stats[s])
            out = pd.DataFrame(cols)
            return out if ok.all() else out.loc[ok].reset_index(drop=True)
        return cls._to_dataset(res, stats, names, by_cols, group_vals, x_col, y_col, xc, yc, bin_2d)

    @staticmethod
    def _to_dataset(res, stats, names, by_cols, group_vals, x_col, y_col, xc, yc, bin_2d):
        """The reference's Dataset: dims (y, x, by_cols...), one variable per statistic; combinations of by_cols values that
        were not observed are NaN (xarray.combine_by_coords), empty cells of observed ones hold scipy's empty value."""
        import xarray as xr
        axes = [np.unique(gv) for gv in group_vals]
        pos = tuple(np.searchsorted(a, gv) for a, gv in zip(axes, group_vals))
        grid_shape = (len(yc), len(xc)) if bin_2d else (len(xc),)
        data = {}
        for s in stats:
            arr = np.full(grid_shape + tuple(len(a) for a in axes), np.nan)
            arr[(Ellipsis,) + pos] = _EMPTY.get(s, np.nan)
            cell = (res.iy, res.ix) if bin_2d else (res.ix,)
            arr[cell + tuple(p[res.gid] for p in pos)] = res.stats[s]
            data[names[s]] = ((([y_col, x_col] if bin_2d else [x_col]) + list(by_cols)), arr)
        coords = {**({y_col: yc} if bin_2d else {}), x_col: xc, **dict(zip(by_cols, axes))}
        return xr.Dataset(data, coords=coords)

    @staticmethod
    def assign_tracks(df, sort_by, get_track_by=None, delta_measure="dr", cut_off=600_000, start_track=0,
                      add_by_track_date=False, lon_col="lon", lat_col="lat", lon_0=0, lat_0=90, datetime_col="datetime",
                      engine=None):
        """Raw ``lon``, ``lat``, ``datetime`` rows to ``t``, ``x``, ``y``, ``dr``, ``dt`` and a ``track`` number: the body of
        the reference's ``TrackId`` (examples/generate_track_id.py: ``add_xyt_columns`` + ``add_tracks``) without its files and
        plots.  ``t`` is the time in ms; ``x``, ``y`` the EASE2 projection (``Engine.project_batch``); the rows are sorted by
        ``sort_by``; within every value of ``get_track_by`` (one column; None: the whole frame) ``dr`` / ``dt`` are the
        distance in space / time to the row before and ``track`` goes up by one where ``delta_measure`` exceeds
        ``cut_off``, each group starting one above the last one's largest track (``Engine.track_batch``, one call for all
        groups).  ``add_by_track_date`` adds ``start_date`` (the day of a track's first row) and ``track_start`` (the
        track's number among its group's tracks of that day); the per-track minimum and the merge run on the host.

        The rows come back in the reference's order: groups in order of first appearance, the sorted order inside a group;
        rows whose group value is null are dropped (the reference's ``==`` selects them for no group).  A copy is returned,
        ``df`` is left as it was.  With ``add_by_track_date`` the index is a new RangeIndex (the reference's merge makes
        one per group)."""
        assert sort_by is not None
        assert isinstance(sort_by, (list, tuple, str)), f"sort_by should be str, list or tuple, got: {type(sort_by)}"
        assert isinstance(add_by_track_date, bool)
        assert isinstance(cut_off, (int, float))
        assert delta_measure in ['dt', 'dr'], f"delta_measure: '{delta_measure}', must in ['dt', 'dr']"
        assert datetime_col in df, f"'{datetime_col}' is not in data"
        for c in [lon_col, lat_col]:
            assert c in df, f"column: '{c}' is not in data"
        if isinstance(get_track_by, (list, tuple)):
            if len(get_track_by) != 1:
                raise NotImplementedError("get_track_by takes one column (the reference's df[get_track_by].unique() does too)")
            get_track_by = get_track_by[0]
        if get_track_by is not None:
            assert get_track_by in df, f"get_track_by: '{get_track_by}' is not in data"
        eng = engine if engine is not None else _engine()
        df = df.copy()
        df['t'] = df[datetime_col].values.astype("datetime64[ms]").astype(float)
        x, y = eng.project_batch(df[lon_col].to_numpy(dtype=np.float64), df[lat_col].to_numpy(dtype=np.float64), "forward",
                                 lon_0, lat_0)
        df['x'], df['y'] = np.asarray(x), np.asarray(y)
        df.sort_values(sort_by, inplace=True)
        codes = None
        if get_track_by is not None:
            # numbered in order of first appearance, null -> -1: df[get_track_by].unique() without its null entry
            codes = pd.factorize(df[get_track_by].to_numpy())[0].astype(np.int32)
        cols = {"dr": [df['x'].to_numpy(dtype=np.float64), df['y'].to_numpy(dtype=np.float64)],
                "dt": [df['t'].to_numpy(dtype=np.float64)]}
        other = "dt" if delta_measure == "dr" else "dr"
        delta, track, order = eng.track_batch(cols[delta_measure], group=codes, cut_off=cut_off, start_track=start_track)
        delta2, _, order2 = eng.track_batch(cols[other], group=codes, cut_off=cut_off, start_track=start_track)
        order = np.asarray(order)
        assert np.array_equal(order, np.asarray(order2))
        n_in = len(order) if codes is None else int((codes >= 0).sum())
        out = df.iloc[order[:n_in]].copy()
        out[delta_measure] = np.asarray(delta)[:n_in]
        out[other] = np.asarray(delta2)[:n_in]
        out = out[[c for c in out.columns if c not in ("dr", "dt")] + ["dr", "dt"]]
        out['track'] = np.asarray(track)[:n_in].astype(int)
        if add_by_track_date:
            # per track, not per row: the first row of every track on the host, the counter on the device
            first = np.flatnonzero(np.diff(out['track'].to_numpy(), prepend=start_track - 1) != 0)
            tsd = out.groupby('track', sort=True)[datetime_col].min().reset_index()
            tsd.rename(columns={datetime_col: "start_date"}, inplace=True)
            tsd['start_date'] = tsd['start_date'].values.astype("datetime64[D]")
            tgroup = None if codes is None else codes[order[:n_in]][first]
            _, run, _ = eng.track_batch([tsd['start_date'].values.astype('int64').astype(np.float64)], group=tgroup, mode="runs")
            tsd['track_start'] = np.asarray(run).astype(int)
            out = out.merge(tsd, on=['track'], how='left')
        return out

    @staticmethod
    def bin_data(df, x_range=None, y_range=None, grid_res=None, x_col="x", y_col="y", val_col=None,
                 bin_statistic="mean", bin_2d=True, return_bin_center=True):
        """Bin ``val_col`` of ``df`` on a regular grid: returns ``(binned, (x_out, y_out))``, or ``(binned, x_out)`` when
        ``bin_2d`` is False.  ``binned`` is dense, shape (ny - 1, nx - 1) (scipy's statistic transposed, as the
        reference returns it), empty cells NaN (count and sum: 0); x_out / y_out are the bin centres or the edges."""
        assert val_col is not None, "val_col - the column containing values to bin cannot be None"
        assert grid_res is not None, "grid_res is None, must be supplied - expressed in km"
        assert len(df) > 0, "dataframe (df) provide must have len > 0"
        if not bin_2d:
            y_col = x_col
        x_edge, y_edge = grid_edges(x_range, y_range, grid_res, bin_2d)
        assert x_col in df, f"x_col: {x_col} is not in df columns: {df.columns}"
        assert y_col in df, f"y_col: {y_col} is not in df columns: {df.columns}"
        assert val_col in df, f"val_col: {val_col} is not in df columns: {df.columns}"
        if isinstance(bin_statistic, list):
            raise ValueError("bin_data takes one statistic; bin_data_by takes a list")
        stat = _check_statistics(bin_statistic)[0]
        x = df[x_col].to_numpy(dtype=np.float64)
        v = df[val_col].to_numpy(dtype=np.float64)
        y = df[y_col].to_numpy(dtype=np.float64) if bin_2d else None
        res = _engine().bin_batch(x, y, v, None, 1, x_edge, y_edge if bin_2d else None, [stat])
        shape = (len(y_edge) - 1, len(x_edge) - 1) if bin_2d else (len(x_edge) - 1,)
        binned = np.full(shape, _EMPTY.get(stat, np.nan))
        binned[(res.iy, res.ix) if bin_2d else (res.ix,)] = res.stats[stat]
        xy_out = (bin_centres(x_edge), bin_centres(y_edge)) if return_bin_center else (x_edge, y_edge)
        return (binned, (xy_out[0], xy_out[1])) if bin_2d else (binned, xy_out[0])
