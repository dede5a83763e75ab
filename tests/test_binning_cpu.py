"""CPU: the host side of the device binning (gpsat_amd/dataprep.py): the reference's assertions raised before any device
call, edges and centres, scipy's right-edge rule as one inclusive limit per axis, group coding, and the new symbol."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

from gpsat_amd import _lib as L
from gpsat_amd import dataprep as dp
from gpsat_amd.dataprep import DataPrep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(n=50, seed=0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({"x": rng.uniform(-100, 100, n), "y": rng.uniform(-100, 100, n), "z": rng.normal(size=n),
                         "day": rng.integers(0, 3, n), "sat": rng.choice(["a", "b"], n)})


# ---- assertions and NotImplementedErrors, without a device -----------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom():
        raise RuntimeError("the device was called")
    monkeypatch.setattr(dp, "_engine", boom)


def test_bin_data_assertions(no_device):
    df = _frame()
    kw = dict(x_range=[-100, 100], y_range=[-100, 100], grid_res=20, val_col="z")
    with pytest.raises(AssertionError, match="val_col"):
        DataPrep.bin_data(df, **{**kw, "val_col": None})
    with pytest.raises(AssertionError, match="grid_res"):
        DataPrep.bin_data(df, **{**kw, "grid_res": None})
    with pytest.raises(AssertionError, match="len > 0"):
        DataPrep.bin_data(df.iloc[:0], **kw)
    with pytest.raises(AssertionError, match="x_range should be"):
        DataPrep.bin_data(df, **{**kw, "x_range": [100, -100]})
    with pytest.raises(AssertionError, match="y_range should be"):
        DataPrep.bin_data(df, **{**kw, "y_range": [100, -100]})
    with pytest.raises(AssertionError, match="x_col"):
        DataPrep.bin_data(df, x_col="nope", **kw)
    with pytest.raises(AssertionError, match="y_col"):
        DataPrep.bin_data(df, y_col="nope", **kw)
    with pytest.raises(AssertionError, match="val_col"):
        DataPrep.bin_data(df, **{**kw, "val_col": "nope"})
    with pytest.raises(NotImplementedError, match="callable"):
        DataPrep.bin_data(df, bin_statistic=np.mean, **kw)
    with pytest.raises(ValueError, match="invalid statistic"):
        DataPrep.bin_data(df, bin_statistic="mode", **kw)
    # 1-D: y_col is not looked at
    with pytest.raises(RuntimeError, match="the device was called"):
        DataPrep.bin_data(df, y_col="nope", bin_2d=False, **kw)


def test_bin_data_by_assertions(no_device):
    df = _frame()
    kw = dict(by_cols=["day", "sat"], val_col="z", x_range=[-100, 100], y_range=[-100, 100], grid_res=20, return_df=True)
    with pytest.raises(AssertionError, match="col_funcs must be a dictionary"):
        DataPrep.bin_data_by(df, col_funcs=[], **kw)
    with pytest.raises(NotImplementedError, match="col_funcs"):
        DataPrep.bin_data_by(df, col_funcs={"t": {"func": "lambda x: x", "col_args": "day"}}, **kw)
    with pytest.raises(AssertionError, match="by_col needs"):
        DataPrep.bin_data_by(df, **{**kw, "by_cols": None})
    with pytest.raises(AssertionError, match="must be list or tuple"):
        DataPrep.bin_data_by(df, **{**kw, "by_cols": {"day"}})
    with pytest.raises(AssertionError, match="by_cols value"):
        DataPrep.bin_data_by(df, **{**kw, "by_cols": "nope"})
    with pytest.raises(AssertionError, match="val_col"):
        DataPrep.bin_data_by(df, **{**kw, "val_col": None})
    with pytest.raises(AssertionError, match="x_col"):
        DataPrep.bin_data_by(df, x_col="nope", **kw)
    with pytest.raises(AssertionError, match="y_col"):
        DataPrep.bin_data_by(df, y_col="nope", **kw)
    with pytest.raises(AssertionError, match="grid_res"):
        DataPrep.bin_data_by(df, **{**kw, "grid_res": None})
    with pytest.raises(AssertionError, match="x_range should be"):
        DataPrep.bin_data_by(df, **{**kw, "x_range": [1, 0]})
    with pytest.raises(NotImplementedError, match="callable"):
        DataPrep.bin_data_by(df, bin_statistic=["mean", np.std], **kw)
    with pytest.raises(AssertionError, match="limit"):
        DataPrep.bin_data_by(df, limit=6, **kw)             # 3 days x 2 satellites = 6 combinations: not < 6
    with pytest.raises(NotImplementedError, match="col, comp, val"):
        DataPrep.bin_data_by(df, row_select=[{"loc_col": "day", "src_col": "day", "func": "lambda x, y: x == y"}], **kw)
    with pytest.raises(RuntimeError, match="the device was called"):
        DataPrep.bin_data_by(df, limit=7, **kw)


def test_dataset_needs_xarray(no_device, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "xarray", None)          # `import xarray` raises ImportError, installed or not
    with pytest.raises(NotImplementedError, match="return_df=True"):
        DataPrep.bin_data_by(_frame(), by_cols="day", val_col="z", grid_res=20, x_range=[-100, 100], y_range=[-100, 100])


def test_default_ranges_and_notice(capsys):
    xe, ye = dp.grid_edges(None, None, 50_000)
    out = capsys.readouterr().out
    assert "x_range, not provided, using default: [-4500000.0, 4500000.0]" in out
    assert "y_range, not provided, using default: [-4500000.0, 4500000.0]" in out
    assert len(xe) == len(ye) == 181 and xe[0] == -4.5e6 and xe[-1] == 4.5e6
    dp.grid_edges(None, None, 50_000, bin_2d=False)
    out = capsys.readouterr().out
    assert "x_range" in out and "y_range" not in out


# ---- edges and centres -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x_range,y_range,res", [
    ([-4.5e6, 4.5e6], [-4.5e6, 4.5e6], 50_000), ([-4.5e6, 4.5e6], [-4.5e6, 4.5e6], 5_000),
    ([-100, 100], [0, 60], 20), ([0.0, 1.0], [-2.0, 1.0], 0.1), ([-0.5, 0.25], [0.0, 0.01], 1e-3),
    ([0, 10], [0, 7], 3),              # a resolution that does not divide the range
    ([-1e6, 2.5e6], [-3e6, 1e5], 12_345.6),
])
def test_edges_and_centres(x_range, y_range, res):
    xe, ye = dp.grid_edges(x_range, y_range, res)
    for e, (lo, hi) in ((xe, x_range), (ye, y_range)):
        n = int((hi - lo) / res + 1)
        assert np.array_equal(e, np.linspace(lo, hi, n))
        assert np.array_equal(dp.bin_centres(e), e[:-1] + np.diff(e) / 2)
        assert len(dp.bin_centres(e)) == n - 1


# ---- scipy's right edge ----------------------------------------------------------------------------------------------
def _walk(x0, n):
    up, dn = [x0], [x0]
    for _ in range(n):
        up.append(np.nextafter(up[-1], np.inf))
        dn.append(np.nextafter(dn[-1], -np.inf))
    return np.array(dn[::-1] + up[1:])


@pytest.mark.parametrize("lo,hi,step", [(-4.5e6, 4.5e6, 50_000), (-100.0, 100.0, 20), (0.0, 1.0, 0.1), (-0.5, 0.25, 1e-3),
                                        (-300.0, -100.0, 20), (-1.0, 0.0, 0.1)])
def test_right_edge_limit_is_scipys_rule(lo, hi, step):
    edges = np.linspace(lo, hi, int((hi - lo) / step + 1))
    x_hi = dp.right_edge_limit(edges)
    decimal = int(-np.log10(np.diff(edges).min())) + 6            # scipy/stats/_binned_statistic.py::_bin_numbers
    assert decimal == dp.edge_decimals(edges)
    boundary = edges[-1] + 0.5 * 10.0 ** (-decimal)              # where the rounding changes, to a few ulps
    xs = np.concatenate([_walk(edges[-1], 400), _walk(boundary, 400), _walk(x_hi, 400),
                         edges[-1] + np.linspace(0, 2, 2001) * 10.0 ** (-decimal)])
    on_edge = (xs >= edges[-1]) & (np.around(xs, decimal) == np.around(edges[-1], decimal))
    inside = (xs >= edges[-1]) & (xs <= x_hi)
    assert np.array_equal(on_edge, inside)
    assert on_edge.any() and not on_edge.all()


def test_right_edge_limit_matches_binned_statistic():
    from scipy import stats as scst
    edges = np.linspace(-100, 100, 11)
    x_hi = dp.right_edge_limit(edges)
    xs = np.array([100.0, 100.0000004, 100.0000006, x_hi, np.nextafter(x_hi, np.inf), 100.1])
    ref = scst.binned_statistic(xs, np.ones_like(xs), statistic="count", bins=edges)
    assert ref.statistic[-1] == np.count_nonzero(xs <= x_hi) == 4


def test_ordered_integers_round_trip():
    for x in (0.0, 1.0, -1.0, 4.5e6, -4.5e6, 5e-324, -5e-324, 1.7e308):
        k = dp._to_ord(x)
        assert dp._from_ord(k) == x
        assert dp._from_ord(k + 1) == np.nextafter(x, np.inf)
        assert dp._from_ord(k - 1) == np.nextafter(x, -np.inf)


# ---- group coding ----------------------------------------------------------------------------------------------------
def test_group_coding_mixed_columns():
    df = pd.DataFrame({
        "sat": ["S3B", "CS2", "S3A", "CS2", "S3A", "CS2"],
        "date": pd.to_datetime(["2020-03-02", "2020-03-01", "2020-03-02", "2020-03-01", "2020-03-01", "2020-03-02"]),
        "lead": [0.5, 1.5, 0.5, 1.5, 0.5, 1.5],
    })
    gid, vals, n = dp.code_groups(df, ["sat", "date", "lead"])
    assert n == 5                                                    # observed combinations only (2 x 3 x 2 = 12 possible)
    combos = list(zip(*[v.tolist() for v in vals]))
    assert combos == sorted(combos) and len(set(combos)) == 5       # ascending, lexicographic by by_cols
    for i in range(len(df)):
        assert vals[0][gid[i]] == df["sat"][i] and vals[1][gid[i]] == df["date"].to_numpy()[i] and vals[2][gid[i]] == df["lead"][i]
    assert gid[1] == gid[3] and gid.dtype == np.int32 and gid.min() == 0 and gid.max() == 4


def test_group_coding_nulls_match_the_reference_mask():
    """A row whose by-value is null equals nothing: the reference's mask never selects it, but drop_duplicates counts it."""
    df = pd.DataFrame({"sat": ["a", None, "b", "a"], "day": [1.0, 1.0, np.nan, 2.0]})
    gid, vals, n = dp.code_groups(df, ["sat", "day"])
    assert gid.tolist() == [0, -1, -1, 1]
    assert n == len(df[["sat", "day"]].drop_duplicates()) == 4
    assert vals[0].tolist() == ["a", "a"] and vals[1].tolist() == [1.0, 2.0]


def test_group_coding_empty():
    gid, vals, n = dp.code_groups(pd.DataFrame({"d": np.array([], dtype=float)}), ["d"])
    assert len(gid) == 0 and n == 0 and len(vals[0]) == 0


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_bin_symbol_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpsat_hip.h")).read()
    assert re.search(r"\bint\s+gpsat_bin_batch\s*\(", hdr)
    for name, bit in L.BIN_STATS.items():
        assert int(re.search(rf"#define\s+GPSAT_BIN_{name.upper()}\s+(\d+)u", hdr).group(1)) == bit
    assert "gpsat_bin_batch" in L.EXPORTS and "gpsat_bin_batch" in L.OPTIONAL_EXPORTS
    lib = L.load()
    assert hasattr(lib, "gpsat_bin_batch")
    assert lib.gpsat_bin_batch.restype is C.c_int and len(lib.gpsat_bin_batch.argtypes) == 18
    from gpsat_amd.engine import Engine
    assert callable(Engine.bin_batch)
    import gpsat_amd
    assert gpsat_amd.DataPrep is DataPrep


def test_bin_batch_validates_before_the_device():
    """Argument errors come back as GPSAT_EINVAL with a message; no handle, no device needed for the first of them."""
    lib = L.load()
    n = C.c_int64(7)
    assert lib.gpsat_bin_batch(None, 0, None, None, None, None, 1, 2, None, 0.0, 0, None, 0.0, 4, 0, C.byref(n), None, None) == -1
    assert b"NULL handle" in lib.gpsat_last_error()
