"""CPU: dynamic global_select entries {loc_col, src_col, func} (GPSat/dataloader.py:2893-2978, local_experts.py:426-472,
971-985) on the host selector and through BatchedLocalExpertOI, against a plain per-expert pandas restatement of the rules."""
import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

from gpsat_amd.local_experts import BatchedLocalExpertOI, DynamicSelect, LocalSelector, split_global_select
from test_local_experts_cpu import OracleEngine


def _restate(df, xl, local_select, global_select):
    """Per expert: ref = rl.iloc[0, :].to_dict(); the where list (static as is, dynamic per matching local entry) ANDed with
    pandas' own comparisons; then local_data_select on what is left.  Returns the kept row POSITIONS of df per expert."""
    out = []
    for i in range(len(xl)):
        ref = xl.iloc[[i]].iloc[0, :].to_dict()
        keep = np.ones(len(df), dtype=bool)
        for gs in global_select:
            if all(c in gs for c in ["col", "comp", "val"]):
                x, y = df[gs["col"]], gs["val"]
                keep &= eval(f"x {gs['comp']} y").to_numpy(dtype=bool)
                continue
            func = eval(gs["func"]) if isinstance(gs["func"], str) else gs["func"]
            for ls in local_select:
                if gs["loc_col"] == ls["col"]:
                    x, y = df[gs["src_col"]], func(ref[gs["loc_col"]], ls["val"])
                    keep &= eval(f"x {ls['comp']} y").to_numpy(dtype=bool)
        pos = np.nonzero(keep)[0]
        sub = df.iloc[pos]
        m = np.ones(len(sub), dtype=bool)
        for ls in local_select:
            if isinstance(ls["col"], str):
                x, y = sub[ls["col"]].values, ref[ls["col"]] + ls["val"]
                m &= eval(f"x {ls['comp']} y")
            else:
                ids = cKDTree(sub.loc[:, ls["col"]].values).query_ball_point(x=[ref[c] for c in ls["col"]], r=ls["val"]) \
                    if len(sub) else []
                b = np.zeros(len(sub), dtype=bool)
                b[ids] = True
                m &= b
        out.append(pos[m])
    return out


def _host(df, xl, local_select, global_select):
    static, dynamic = split_global_select(global_select)
    assert not static
    dyn = DynamicSelect(dynamic, local_select, df, xl.columns)
    if not dyn.items:
        return LocalSelector(df, local_select).select(xl)
    codes, _ = dyn.codes()
    return LocalSelector(df, local_select, interval_codes=codes).select(xl, bounds=dyn.bounds(xl))


def _check(df, xl, local_select, global_select):
    off, idx = _host(df, xl, local_select, global_select)
    want = _restate(df, xl, local_select, global_select)
    for i, w in enumerate(want):
        np.testing.assert_array_equal(idx[off[i]:off[i + 1]], w)
    return off


def _frame(rng, M=3000):
    t = rng.integers(0, 12, M) + np.round(rng.uniform(0, 1, M), 2)
    df = pd.DataFrame({"t": t, "x": rng.uniform(-5, 5, M), "y": rng.uniform(-5, 5, M)})
    df["day"] = np.floor(t)
    df["date"] = pd.to_datetime(np.floor(t), unit="D").astype("datetime64[ns]")
    return df


@pytest.mark.parametrize("comp", [">=", ">", "==", "<", "<="])
def test_every_comparison(comp):
    rng = np.random.default_rng(1)
    df = _frame(rng)
    xl = pd.DataFrame({"t": [3.0, 4.5, 6.25, 11.0, 0.0], "x": 0.0, "y": 0.0})
    ls = [{"col": "t", "comp": comp, "val": 2}]
    gs = [{"loc_col": "t", "src_col": "day", "func": lambda x, y: np.floor(x + y)}]       # thresholds equal to column values
    off = _check(df, xl, ls, gs)
    assert off[-1] > 0


def test_several_entries_on_one_and_two_src_cols_string_and_callable_func():
    rng = np.random.default_rng(2)
    df = _frame(rng)
    df["u"] = rng.integers(0, 20, len(df)).astype(float)
    xl = pd.DataFrame({"t": [2.5, 5.0, 7.75, 9.1], "x": [0.0, 1.0, -1.0, 2.0], "y": 0.0, "u": [3.0, 10.0, 10.0, 15.0]})
    ls = [{"col": "t", "comp": "<=", "val": 3}, {"col": "t", "comp": ">=", "val": -3}, {"col": ["x", "y"], "comp": "<", "val": 3.0},
          {"col": "u", "comp": "<", "val": 4}]
    gs = [{"loc_col": "t", "src_col": "date", "func": "lambda x,y: np.datetime64(pd.to_datetime(x+y, unit='D'))"},
          {"loc_col": "u", "src_col": "day", "func": lambda x, y: x - y}]
    dyn = DynamicSelect(split_global_select(gs)[1], ls, df, xl.columns)
    assert dyn.src_cols == ["date", "day"] and len(dyn.items) == 3           # t<= and t>= intersect into one date interval
    off = _check(df, xl, ls, gs)
    assert off[-1] > 0


def test_nan_rows_and_nat_threshold():
    rng = np.random.default_rng(3)
    df = _frame(rng, 2000)
    df.loc[rng.choice(len(df), 100, replace=False), "date"] = pd.NaT
    df.loc[rng.choice(len(df), 100, replace=False), "day"] = np.nan
    xl = pd.DataFrame({"t": [2.0, 5.5, 8.0], "x": 0.0, "y": 0.0})
    ls = [{"col": "t", "comp": "<=", "val": 2}, {"col": "t", "comp": ">=", "val": -2}]
    nat = lambda x, y: pd.NaT if x > 5 else np.datetime64(pd.to_datetime(x + y, unit="D"))     # noqa: E731
    off = _check(df, xl, ls, [{"loc_col": "t", "src_col": "date", "func": nat}])
    assert off[2] - off[1] == 0 and off[1] > 0                  # any comparison with NaT is False
    _check(df, xl, ls, [{"loc_col": "t", "src_col": "day", "func": lambda x, y: x + y}])


def test_int64_beyond_2_53_and_datetime_1ns_apart():
    base = 2 ** 60
    n = 400
    df = pd.DataFrame({"t": np.tile(np.arange(8.0), n // 8), "k": base + np.arange(n, dtype=np.int64)})
    df["ns"] = pd.Timestamp("2020-03-05").as_unit("ns") + pd.to_timedelta(np.arange(n), unit="ns")
    xl = pd.DataFrame({"t": [2.0, 5.0]})
    ls = [{"col": "t", "comp": "<=", "val": 1}, {"col": "t", "comp": ">=", "val": -1}]
    # int thresholds that differ by 1 at 2^60 (not representable in fp64) -- the rank codes keep them apart
    off = _check(df, xl, ls, [{"loc_col": "t", "src_col": "k", "func": lambda x, y: base + 100 + int(x) * 10 + int(y)}])
    assert off[-1] > 0
    off = _check(df, xl, ls, [{"loc_col": "t", "src_col": "ns",
                               "func": lambda x, y: pd.Timestamp("2020-03-05") + pd.Timedelta(int(x * 20 + y), unit="ns")}])
    assert off[-1] > 0


def test_string_column():
    rng = np.random.default_rng(4)
    df = _frame(rng, 1500)
    df["label"] = ["d%02d" % int(v) for v in df["day"]]
    xl = pd.DataFrame({"t": [3.0, 6.5], "x": 0.0, "y": 0.0})
    ls = [{"col": "t", "comp": "<", "val": 3}, {"col": "t", "comp": ">", "val": -1}]
    off = _check(df, xl, ls, [{"loc_col": "t", "src_col": "label", "func": lambda x, y: "d%02d" % int(x + y)}])
    assert off[-1] > 0


def test_unmatched_loc_col_adds_nothing():
    rng = np.random.default_rng(5)
    df = _frame(rng, 1000)
    xl = pd.DataFrame({"t": [3.0, 6.5], "x": 0.0, "y": 0.0})
    ls = [{"col": "t", "comp": "<=", "val": 2}, {"col": ["x", "y"], "comp": "<", "val": 2.0}]
    gs = [{"loc_col": "x", "src_col": "day", "func": lambda x, y: 1 / 0}]           # never called
    off, idx = _host(df, xl, ls, gs)
    off0, idx0 = LocalSelector(df, ls).select(xl)
    np.testing.assert_array_equal(off, off0)
    np.testing.assert_array_equal(idx, idx0)
    _check(df, xl, ls, gs)


def test_func_called_once_per_distinct_value():
    rng = np.random.default_rng(6)
    df = _frame(rng, 1000)
    xl = pd.DataFrame({"t": np.repeat([2.0, 4.0, 6.0], 50), "x": rng.uniform(-1, 1, 150), "y": 0.0})
    calls = []

    def f(x, y):
        calls.append((x, y))
        return np.datetime64(pd.to_datetime(x + y, unit="D"))
    ls = [{"col": "t", "comp": "<=", "val": 2}, {"col": "t", "comp": ">=", "val": -2}]
    dyn = DynamicSelect([{"loc_col": "t", "src_col": "date", "func": f}], ls, df, xl.columns)
    dyn.bounds(xl)
    assert len(calls) == 6 and all(type(x) is float for x, _ in calls)       # the boxing of rl.iloc[0, :].to_dict()


def _config(rng, n_days=9):
    """A synthetic stand-in for the reference's configs[0] shape: t in days since the epoch, date = that day."""
    day0 = 18326                                        # 2020-03-05
    M = 2500
    day = day0 - 4 + rng.integers(0, n_days, M)
    t = day + rng.uniform(0, 1, M)
    obs = pd.DataFrame({"x": rng.uniform(-6e5, 6e5, M), "y": rng.uniform(-6e5, 6e5, M), "t": t,
                        "date": pd.to_datetime(day, unit="D").astype("datetime64[ns]"), "lat": rng.uniform(55, 90, M)})
    obs["obs"] = np.sin(obs["x"] / 2e5) + 0.1 * rng.standard_normal(M)
    xl = pd.DataFrame({"x": rng.uniform(-4e5, 4e5, 12), "y": rng.uniform(-4e5, 4e5, 12),
                       "t": day0 + np.array([0, 0.25, 0.5, 1, 1.5, 0.75, -1, -0.5, 0, 1, 0.3, -0.9])})
    xl["date"] = pd.to_datetime(np.floor(xl["t"]), unit="D")
    func = "lambda x,y: np.datetime64(pd.to_datetime(x+y, unit='D'))"
    data = {"data_source": obs, "obs_col": "obs", "coords_col": ["x", "y", "t"],
            "local_select": [{"col": "t", "comp": "<=", "val": 4}, {"col": "t", "comp": ">=", "val": -4},
                             {"col": ["x", "y"], "comp": "<", "val": 300000}],
            "global_select": [{"col": "lat", "comp": ">=", "val": 60}, {"loc_col": "t", "src_col": "date", "func": func}]}
    model = {"oi_model": "GPflowGPRModel", "init_params": {"coords_scale": [50000, 50000, 1]},
             "constraints": {"lengthscales": {"low": [1e-8, 1e-8, 1e-8], "high": [600000, 600000, 9]}},
             "optim_kwargs": {"max_iter": 5}}
    return obs, xl, data, model, func


def test_orchestrator_num_obs_and_oi_config():
    rng = np.random.default_rng(7)
    obs, xl, data, model, func = _config(rng)
    oi = BatchedLocalExpertOI(expert_loc_config={"source": xl}, data_config=data, model_config=model,
                              pred_loc_config={"method": "expert_loc"}, engine=OracleEngine(), dtype="f64")
    out = oi.run(store_every=10)
    want = _restate(obs, xl, data["local_select"], data["global_select"])
    assert out["run_details"]["num_obs"].tolist() == [len(w) for w in want]
    assert oi.config["data"]["global_select"][1]["func"] == func
    assert oi.timings["dynamic_select_s"] > 0
    # without the dynamic entry the tiles are larger: the date criterion removes the rows of days the fractional t excludes
    data0 = {**data, "global_select": data["global_select"][:1]}
    oi0 = BatchedLocalExpertOI(expert_loc_config={"source": xl}, data_config=data0, model_config=model,
                               pred_loc_config={"method": "expert_loc"}, engine=OracleEngine(), dtype="f64")
    n0 = oi0.run(optimise=False)["run_details"]["num_obs"].to_numpy()
    assert (n0 >= out["run_details"]["num_obs"].to_numpy()).all() and (n0 != out["run_details"]["num_obs"].to_numpy()).any()


def test_refusals():
    rng = np.random.default_rng(8)
    obs, xl, data, model, _ = _config(rng)
    base = dict(expert_loc_config={"source": xl}, model_config=model, pred_loc_config={"method": "expert_loc"},
                engine=OracleEngine())
    with pytest.raises(AssertionError):                 # missing keys
        BatchedLocalExpertOI(data_config={**data, "global_select": [{"loc_col": "t", "src_col": "date"}]}, **base)
    with pytest.raises(AssertionError):                 # loc_col not among the expert locations' columns
        BatchedLocalExpertOI(data_config={**data, "global_select": [{"loc_col": "lat", "src_col": "date",
                                                                     "func": "lambda x, y: x"}]}, **base)

    class Odd:                                          # compares True on every other value: no contiguous rank run
        __hash__ = object.__hash__
        __le__ = __ge__ = __lt__ = __gt__ = __eq__ = lambda self, o: o % 2 < 1

    obj = pd.DataFrame({"t": [1.0, 2.0, 3.0, 4.0], "s": pd.Series([0.0, 1.0, 2.0, 3.0], dtype=object)})
    dyn = DynamicSelect([{"loc_col": "t", "src_col": "s", "func": lambda x, y: Odd()}], [{"col": "t", "comp": "<=", "val": 1}],
                        obj, ["t"])
    with pytest.raises(NotImplementedError):
        dyn.bounds(pd.DataFrame({"t": [1.0]}))
    # the example config needs exactly 4 device criteria; one more local entry is refused, naming the limit
    BatchedLocalExpertOI(data_config=data, device_select=True, **base)
    more = {**data, "local_select": data["local_select"] + [{"col": "x", "comp": ">=", "val": -1e6}]}
    with pytest.raises(NotImplementedError, match="at most 4"):
        BatchedLocalExpertOI(data_config=more, device_select=True, **base)
    BatchedLocalExpertOI(data_config=more, device_select=False, **base)           # the host path has no such limit
