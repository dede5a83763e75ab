"""GPU: dynamic global_select entries as device interval criteria (kind 2 of gpsat_select_batch_ex): device CSR equal to the
host selector's bit for bit, the two-call cache, and a synthetic stand-in for the reference's configs[0] end to end."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from gpsat_amd.local_experts import BatchedLocalExpertOI, DynamicSelect, LocalSelector
from oracle import gp_oracle as go
import select_numpy
from test_dynamic_select_cpu import _restate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


LOCAL = [{"col": "t", "comp": "<=", "val": 4}, {"col": "t", "comp": ">=", "val": -4},
         {"col": ["x", "y"], "comp": "<", "val": 3e5}]
DYN = [{"loc_col": "t", "src_col": "date", "func": "lambda x,y: np.datetime64(pd.to_datetime(x+y, unit='D'))"}]


def _table(rng, M, n_days=60, ordered=False):
    day = rng.integers(0, n_days, M)
    if ordered:
        day = np.sort(day)
    df = pd.DataFrame({"x": rng.uniform(-2e6, 2e6, M), "y": rng.uniform(-2e6, 2e6, M), "t": day + rng.uniform(0, 1, M)})
    df["date"] = pd.to_datetime(day, unit="D").astype("datetime64[ns]")
    return df


def _experts(rng, T, n_days=60):
    return pd.DataFrame({"x": rng.uniform(-1.8e6, 1.8e6, T), "y": rng.uniform(-1.8e6, 1.8e6, T),
                         "t": rng.integers(4, n_days - 4, T) + rng.choice([0.0, 0.25, 0.5, 0.9], T)})


def _device_and_host(eng, df, xl, check):
    dyn = DynamicSelect(DYN, LOCAL, df, xl.columns)
    codes, _ = dyn.codes()
    b = dyn.bounds(xl)
    from gpsat_amd.local_experts import DeviceSelector
    off, idx = DeviceSelector(df, LOCAL, eng, interval_codes=codes).select(xl, bounds=b)
    assert len(DeviceSelector(df, LOCAL, eng, interval_codes=codes).criteria) == 4
    ho, hi = LocalSelector(df, LOCAL, interval_codes=codes).select(xl.iloc[check], bounds=b[check])
    for j, e in enumerate(check):
        np.testing.assert_array_equal(idx[off[e]:off[e + 1]], hi[ho[j]:ho[j + 1]])
    # EVERY expert against the NumPy restatement (the host selector above, a KD-tree query per expert, answers the sample)
    w_off, w_idx = select_numpy.select_frames(df, LOCAL, xl, interval_codes=codes, bounds=b)
    np.testing.assert_array_equal(off, w_off)
    np.testing.assert_array_equal(idx, w_idx)
    return off, idx


@pytest.mark.parametrize("ordered", [False, True])
def test_two_million_rows_four_criteria(eng, ordered):
    """Shuffled rows go through the spatial binning; day-ordered rows, with binning off, through the box skip."""
    rng = np.random.default_rng(31)
    df = _table(rng, 2_000_003, ordered=ordered)
    xl = _experts(rng, 400)
    if ordered:
        os.environ["GPSAT_DEVELOPER"] = "1"
        os.environ["GPSAT_DEBUG_NO_BINNING"] = "1"
    try:
        off, _ = _device_and_host(eng, df, xl, list(range(0, 400, 13)))
    finally:
        os.environ.pop("GPSAT_DEBUG_NO_BINNING", None)
    # the date interval removes rows: without it the tiles are larger
    from gpsat_amd.local_experts import DeviceSelector
    off0, _ = DeviceSelector(df, LOCAL, eng).select(xl)
    assert (np.diff(off0) >= np.diff(off)).all() and (np.diff(off0) > np.diff(off)).any()


@pytest.mark.parametrize("T", [1, 50_000])
def test_expert_counts(eng, T):
    rng = np.random.default_rng(32)
    df = _table(rng, 300_007)
    xl = _experts(rng, T)
    _device_and_host(eng, df, xl, sorted(set([0, T - 1] + list(range(0, T, max(1, T // 25))))))


def test_interval_ends_on_values_empty_intervals_and_nan(eng):
    rng = np.random.default_rng(33)
    M, T = 150_001, 64
    code = rng.integers(0, 50, M).astype(np.float64)
    code[rng.choice(M, 5000, replace=False)] = np.nan
    x = rng.uniform(-1, 1, M)
    pts = np.stack([x, code], axis=1)
    refs = np.zeros((T, 2))
    refs[:, 0] = rng.uniform(-0.5, 0.5, T)
    lo = rng.integers(0, 50, T).astype(np.float64)
    hi = lo + rng.integers(0, 6, T)                           # ends on the codes themselves; hi == lo: empty
    hi[:4] = lo[:4] - 1                                       # lo > hi: empty
    lo[4], hi[4] = -np.inf, np.inf                            # everything but the NaN codes
    bounds = np.stack([lo, hi], axis=1)[:, None, :]
    crit = [("cmp", 0, "<=", 0.5), ("cmp", 0, ">=", -0.5), ("interval", 1, 0)]
    for env in (False, True):
        if env:
            os.environ["GPSAT_DEVELOPER"] = "1"
            os.environ["GPSAT_DEBUG_NO_BINNING"] = "1"
        try:
            off, idx = eng.select_batch(pts, refs, crit, bounds=bounds)
        finally:
            os.environ.pop("GPSAT_DEBUG_NO_BINNING", None)
        for e in range(T):
            want = np.nonzero((x <= refs[e, 0] + 0.5) & (x >= refs[e, 0] - 0.5) & (lo[e] <= code) & (code < hi[e]))[0]
            np.testing.assert_array_equal(idx[off[e]:off[e + 1]], want)
        assert (np.diff(off)[:4] == 0).all()
        assert np.diff(off)[4] == np.sum((np.abs(x - refs[4, 0]) <= 0.5) & ~np.isnan(code))
    # without bounds, kind 2 is refused (gpsat_select_batch keeps rejecting it)
    from gpsat_amd import _lib as L
    sp = L.GpsatSelectSpec()
    sp.n_crit, sp.kind[0], sp.ncols[0] = 1, 2, 1
    o = np.zeros(T + 1, np.int64)
    pc = np.ascontiguousarray(pts.T)
    rc = eng._lib.gpsat_select_batch(eng._h, C.byref(sp), M, 2, pc.ctypes.data_as(C.c_void_p), T,
                                     refs.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), None, 0)
    assert rc != 0


def test_two_call_cache_sees_new_bounds(eng):
    rng = np.random.default_rng(34)
    M, T = 100_000, 40
    pts = np.stack([rng.uniform(-1, 1, M), rng.integers(0, 30, M).astype(np.float64)], axis=1)
    refs = np.zeros((T, 2))
    crit = [("cmp", 0, "<=", 0.5), ("interval", 1, 0)]
    lo = rng.integers(0, 25, T).astype(np.float64)
    A = np.stack([lo, lo + 5], axis=1)[:, None, :].copy()
    B = np.stack([lo + 2, lo + 4], axis=1)[:, None, :].copy()
    offB, idxB = eng.select_batch(pts, refs, crit, bounds=B)
    offA, idxA = eng.select_batch(pts, refs, crit, bounds=A)
    assert offA[-1] > offB[-1]
    from gpsat_amd import _lib as L
    sp = L.GpsatSelectSpec()
    sp.n_crit = 2
    sp.kind[0], sp.comp[0], sp.ncols[0], sp.val[0] = 0, L.COMP_IDS["<="], 1, 0.5
    sp.kind[1], sp.ncols[1] = 2, 1
    sp.cols[1][0], sp.cols[1][1] = 1, 0
    pc = np.ascontiguousarray(pts.T)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                      # noqa: E731
    cap = int(offA[-1])
    for same_buffer in (False, True):
        buf = A.copy()
        off = np.zeros(T + 1, np.int64)
        assert eng._lib.gpsat_select_batch_ex(eng._h, C.byref(sp), M, 2, p(pc), T, p(refs), 1, p(buf), p(off), None, 0) == 0
        np.testing.assert_array_equal(off, offA)
        fill = B.copy()
        if same_buffer:
            buf[...] = B                                 # the same host buffer refilled between the two calls
            fill = buf
        idx = np.empty(cap, np.int32)
        assert eng._lib.gpsat_select_batch_ex(eng._h, C.byref(sp), M, 2, p(pc), T, p(refs), 1, p(fill), p(off), p(idx), cap) == 0
        np.testing.assert_array_equal(off, offB)
        np.testing.assert_array_equal(idx[:off[-1]], idxB)


def _configs0_standin(rng):
    day0 = 18326                                                  # 2020-03-05, days since the epoch
    M = 6000
    day = day0 - 4 + rng.integers(0, 9, M)                       # 9 days of observations
    obs = pd.DataFrame({"x": rng.uniform(-5e5, 5e5, M), "y": rng.uniform(-5e5, 5e5, M), "t": day + rng.uniform(0, 1, M),
                        "date": pd.to_datetime(day, unit="D").astype("datetime64[ns]"), "lat": rng.uniform(50, 90, M)})
    obs["obs"] = np.sin(obs["x"] / 2e5) * np.cos(obs["y"] / 3e5) + 0.1 * np.sin(obs["t"]) + 0.05 * rng.standard_normal(M)
    T = 42
    xl = pd.DataFrame({"x": rng.uniform(-3e5, 3e5, T), "y": rng.uniform(-3e5, 3e5, T),
                       "t": (day0 - 1 + np.arange(T) % 3) + np.where(np.arange(T) % 4 == 0, 0.0, rng.uniform(0.05, 0.95, T))})
    xl["date"] = pd.to_datetime(np.floor(xl["t"]), unit="D")
    grid = pd.DataFrame({"x": np.repeat(np.arange(-5, 6) * 1e5, 11), "y": np.tile(np.arange(-5, 6) * 1e5, 11)})
    data = {"data_source": obs, "obs_col": "obs", "coords_col": ["x", "y", "t"], "local_select": LOCAL,
            "global_select": [{"col": "lat", "comp": ">=", "val": 60}] + DYN}
    model = {"oi_model": "GPflowGPRModel", "init_params": {"coords_scale": [50000, 50000, 1]},
             "constraints": {"lengthscales": {"low": [1e-08, 1e-08, 1e-08], "high": [600000, 600000, 9]}}}
    pred = {"method": "from_dataframe", "df": grid, "max_dist": 200000}
    return obs, xl, data, model, pred


def test_configs0_standin_device_and_host_agree_with_oracle(eng):
    rng = np.random.default_rng(35)
    obs, xl, data, model, pred = _configs0_standin(rng)
    run = lambda d, dev: BatchedLocalExpertOI(expert_loc_config={"source": xl}, data_config=d, model_config=model,   # noqa: E731
                                              pred_loc_config=pred, engine=eng, device_select=dev, dtype="f64").run(store_every=10)
    dev = run(data, True)
    host = run(data, False)
    assert set(dev) == set(host)
    for k in dev:
        if isinstance(dev[k], pd.DataFrame) and k != "run_details":
            pd.testing.assert_frame_equal(dev[k], host[k])
    rd = dev["run_details"]
    num_cols = [c for c in rd.columns if c != "run_time"]                 # per-tile wall time
    pd.testing.assert_frame_equal(rd[num_cols], host["run_details"][num_cols])
    want = _restate(obs, xl, data["local_select"], data["global_select"])
    assert rd["num_obs"].tolist() == [len(w) for w in want]
    n0 = run({**data, "global_select": data["global_select"][:1]}, True)["run_details"]["num_obs"].to_numpy()
    assert (n0 != rd["num_obs"].to_numpy()).any() and (n0 >= rd["num_obs"].to_numpy()).all()
    # objective and predictions at the returned parameters: the fp64 oracle on the tile's rows
    cc, scale = ["x", "y", "t"], np.array([50000.0, 50000.0, 1.0])
    static = obs[obs["lat"] >= 60]
    ls, kv, lv, pr = dev["lengthscales"], dev["kernel_variance"], dev["likelihood_variance"], dev["preds"]
    for i in (0, 1, 2, 17, 41):
        loc = xl.iloc[i]
        key = tuple(loc[cc])
        d = obs.iloc[want[i]]
        assert len(d) >= 3 and set(d.index) <= set(static.index)
        th = np.concatenate([ls.loc[[key]].sort_values("_dim_0")["lengthscales"].values, kv.loc[[key]]["kernel_variance"].values,
                             lv.loc[[key]]["likelihood_variance"].values])
        Xo, yo = d[cc].values / scale, d["obs"].values.astype(np.float64)
        nll, _ = go.nll_and_grad(go.KERNEL_IDS["Matern32"], Xo, yo, th, want_grad=False)
        assert rd.loc[[key]]["objective_value"].values[0] == pytest.approx(nll, rel=1e-9, abs=1e-7)
        p = pr.loc[[key]]
        f, fv, _ = go.predict(go.KERNEL_IDS["Matern32"], Xo, yo, p[[f"pred_loc_{c}" for c in cc]].values / scale, th)
        np.testing.assert_allclose(p["f*"].values, f, rtol=0, atol=1e-7)
        np.testing.assert_allclose(p["f*_var"].values, fv, rtol=0, atol=1e-8)
