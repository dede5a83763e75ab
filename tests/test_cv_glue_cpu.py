"""CPU: held-out predictions glued and scored per observation -- the NumPy restatement of gpsat_glue_keyed_batch against the
glue oracle, every refusal of the entry point's exported host checks, the new symbols, and glue_cv_predictions /
score_cv_predictions / BatchedLocalExpertOI(cv_glue=...) with a device-free engine that answers from the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import glue_keyed_numpy as gk
from gpsat_amd import _lib as L
from gpsat_amd import postprocessing as post
from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
from oracle import post_oracle as po
from test_cv_cpu import OracleCvEngine, _configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-12, 1e-14          # the bound tests/test_gpu_post.py uses for glue


class CvGlueEngine(OracleCvEngine, gk.GlueKeyedNumpyEngine):
    """The fp64 oracle for the tiles, the restatement for the keyed glue."""

    def __init__(self):
        OracleCvEngine.__init__(self)
        gk.GlueKeyedNumpyEngine.__init__(self)


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [1, 2])
def test_restatement_equals_the_glue_oracle(ndim):
    """Every key has its own prediction location, so the oracle's grouping by location is grouping by key."""
    rng = np.random.default_rng(3 + ndim)
    G = 40
    sizes = rng.integers(1, 9, G)
    key = rng.permutation(np.repeat(np.arange(G), sizes))
    loc = rng.uniform(0, 10, (2, G))
    loc[0] = np.sort(loc[0])                              # ascending key = ascending location, the order groupby returns
    R = len(key)
    pred = loc[:ndim, key]
    xprt = pred + rng.normal(0, 1.0, (ndim, R))
    vals = rng.normal(0, 1, (3, R))
    cols_p, cols_x = ["px", "py"][:ndim], ["ex", "ey"][:ndim]
    df = pd.DataFrame({**{c: pred[i] for i, c in enumerate(cols_p)}, **{c: xprt[i] for i, c in enumerate(cols_x)},
                       "a": vals[0], "b": vals[1], "c": vals[2]})
    want = po.glue_local_predictions(df, cols_p, cols_x, ["a", "b", "c"], inference_radius=4.5, R=3)
    for fn in (gk.glue_keyed, gk.glue_keyed_fast):
        keys, counts, out = fn(key, pred, xprt, vals, 4.5 / 3)
        np.testing.assert_array_equal(keys, np.arange(G))
        np.testing.assert_array_equal(counts, sizes)
        np.testing.assert_allclose(want[cols_p[0]].values, loc[0])
        for i, v in enumerate("abc"):
            np.testing.assert_allclose(out[i], want[v].values, rtol=RTOL, atol=ATOL)


def test_restatement_rules():
    key = np.array([5, -1, 5, 2, 2, 9, 2 ** 62, -7])
    pred = np.zeros((2, 8))
    xprt = np.array([[1.0, 0, 2.0, 3.0, 0.5, 3.0, 0.1, 0], [0.0, 0, 0.0, 4.0, 0.5, 4.1, 0.1, 0]])
    vals = np.array([[1.0, 100.0, np.nan, 7.0, 3.0, 2.0, 6.0, 100.0]])
    w = np.exp(-(xprt ** 2).sum(0) / 2 / 4.0) / (2 * np.pi * 4.0)
    for fn in (gk.glue_keyed, gk.glue_keyed_fast):
        keys, counts, out = fn(key, pred, xprt, vals, 2.0)
        np.testing.assert_array_equal(keys, [2, 5, 9, 2 ** 62])
        np.testing.assert_array_equal(counts, [2, 2, 1, 1])
        # NaN: out of the numerator, its weight stays in the denominator
        np.testing.assert_allclose(out[0], [(w[3] * 7 + w[4] * 3) / (w[3] + w[4]), w[0] * 1.0 / (w[0] + w[2]), 2.0, 6.0], rtol=1e-14)
        # max_dist 5: (3, 4) lies exactly on the limit and is out; key 9 has no row left
        keys, counts, out = fn(key, pred, xprt, vals, 2.0, max_dist=5.0)
        np.testing.assert_array_equal(counts, [1, 2, 0, 1])
        assert out[0, 0] == 3.0 and np.isnan(out[0, 2])
        for off in (np.inf, 0.0, -1.0, None):
            np.testing.assert_array_equal(fn(key, pred, xprt, vals, 2.0, max_dist=off)[1], [2, 2, 1, 1])
        assert fn(np.array([-1, -2]), pred[:, :2], xprt[:, :2], vals[:, :2], 1.0)[0].shape == (0,)


# ------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpsat_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpsat_[a-z_]+)\s*\(", src))
    assert {"gpsat_glue_keyed_batch", "gpsat_glue_keyed_timing"} <= declared and declared == set(L.EXPORTS)
    assert {"gpsat_glue_keyed_batch", "gpsat_glue_keyed_timing"} <= set(L.OPTIONAL_EXPORTS)
    lib = L.load()
    assert hasattr(lib, "gpsat_glue_keyed_batch") and hasattr(lib, "gpsat_glue_keyed_timing")
    assert lib.gpsat_version() == 4 == L.ABI_VERSION
    assert re.search(r"int gpsat_glue_keyed_batch\(gpsat_handle \*h, int64_t R, int32_t ndim, int32_t nvars, const int64_t \*key,", src)


def test_host_checks_of_the_keyed_glue():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat16check_glue_keyedEliiPKlPKdS3_S3_dS3_dlS1_S1_PKiS3_Pcm")
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                   C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    R = 6
    buf = {k: np.zeros(4 * R) for k in ("pred", "xprt", "vals", "sig", "out")}
    buf.update(key=np.zeros(R, dtype=np.int64), G=np.zeros(1, dtype=np.int64), okey=np.zeros(R, dtype=np.int64),
               ocnt=np.zeros(R, dtype=np.int32))
    p = {k: v.ctypes.data for k, v in buf.items()}

    def check(**kw):
        a = dict(R=R, ndim=2, nvars=3, key=p["key"], pred=p["pred"], xprt=p["xprt"], vals=p["vals"], sigma=1.5, sig=None,
                 max_dist=np.inf, cap=R, G=p["G"], okey=p["okey"], ocnt=p["ocnt"], out=p["out"])
        a.update(kw)
        why = C.create_string_buffer(200)
        rc = fn(a["R"], a["ndim"], a["nvars"], a["key"], a["pred"], a["xprt"], a["vals"], a["sigma"], a["sig"], a["max_dist"],
                a["cap"], a["G"], a["okey"], a["ocnt"], a["out"], why, 200)
        return rc, why.value.decode()

    good = [{}, dict(ndim=1), dict(nvars=1), dict(nvars=4), dict(sigma=0.0, sig=p["sig"]), dict(sigma=np.nan, sig=p["sig"]),
            dict(max_dist=5.0), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=-np.inf), dict(R=2 ** 31 - 1),
            dict(R=0, key=None, pred=None, xprt=None, vals=None), dict(cap=0, okey=None, ocnt=None, out=None)]
    for kw in good:
        assert check(**kw) == (0, ""), kw
    bad = [(dict(G=None), "G is NULL"), (dict(key=None), "NULL"), (dict(pred=None), "NULL"), (dict(xprt=None), "NULL"),
           (dict(vals=None), "NULL"), (dict(okey=None), "NULL"), (dict(ocnt=None), "NULL"), (dict(out=None), "NULL"),
           (dict(ndim=0), "ndim"), (dict(ndim=3), "ndim"), (dict(nvars=0), "nvars"), (dict(nvars=5), "nvars"),
           (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=np.inf), "sigma"), (dict(sigma=np.nan), "sigma"),
           (dict(max_dist=np.nan), "max_dist"), (dict(R=2 ** 31), "2^31-1"), (dict(R=-1), "negative"), (dict(cap=-1), "negative")]
    for kw, match in bad:
        rc, why = check(**kw)
        assert rc == -1 and match in why and why.startswith("gpsat_glue_keyed_batch: "), (kw, rc, why)
    cap = getattr(lib, "_ZN5gpsat19check_glue_capacityEllPcm")
    cap.restype, cap.argtypes = C.c_int, [C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]
    why = C.create_string_buffer(200)
    assert cap(7, 7, why, 200) == 0 and cap(0, 0, why, 200) == 0 and why.value == b""
    assert cap(6, 7, why, 200) == -1 and b"capacity 6 < G 7" in why.value
    # the entry point itself, before any device is touched: a NULL handle, and nothing to do
    assert lib.gpsat_glue_keyed_batch(None, 0, 2, 3, None, None, None, None, 1.0, None, 0.0, 0, C.byref(C.c_int64(0)), None, None, None) == -1
    assert "handle is NULL" in lib.gpsat_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------
# glue_cv_predictions, score_cv_predictions
# ------------------------------------------------------------------------------------------------------------------
def _cv_preds(obs_index, seed=0, n_obs=30, n_xprt=5):
    """A hand-made cv_preds: experts on a line in x, every observation predicted by the experts within 2.5 of it."""
    rng = np.random.default_rng(seed)
    ox, oy = rng.uniform(0, 10, n_obs), rng.uniform(0, 1, n_obs)
    z = 50.0 + rng.normal(0, 1, n_obs)
    track = rng.integers(0, 3, n_obs)
    ex = np.linspace(1, 9, n_xprt)
    rows = [(e, o) for e in range(n_xprt) for o in range(n_obs) if abs(ex[e] - ox[o]) < 2.5]
    e, o = np.array(rows).T
    n = len(rows)
    cvp = pd.DataFrame({"_dim_0": np.arange(n), "obs_index": np.asarray(obs_index)[o], "track": track[o], "pred_loc_x": ox[o],
                        "pred_loc_y": oy[o], "z": z[o], "f*": rng.normal(0, 1, n), "f*_var": rng.uniform(0.1, 0.2, n),
                        "y_var": rng.uniform(0.3, 0.4, n), "f_bar": 50.0 + rng.normal(0, 0.1, n_xprt)[e]},
                       index=pd.MultiIndex.from_arrays([ex[e], np.full(n, 0.5)], names=["x", "y"]))
    return cvp, o, e


def test_glue_cv_predictions_units_nan_rows_and_max_dist():
    cvp, o, e = _cv_preds(np.arange(100, 130))
    cvp.iloc[::7, cvp.columns.get_loc("f*")] = np.nan     # not held out / skipped fold / failed tile
    assert 0 < int(np.isnan(cvp["f*"].values).sum()) < len(cvp) // 4
    osc = 2.5
    eng = gk.GlueKeyedNumpyEngine()
    got = post.glue_cv_predictions({"cv_preds": cvp}, ["x"], inference_radius=3.0, R=3, obs_scale=osc, engine=eng)
    assert list(got.columns) == ["obs_index", "track", "pred_loc_x", "pred_loc_y", "z", "f*", "f*_var", "y_var", "n_experts", "z_score"]
    # (the observation column of these tables is called z, so the standardised residual is z_score)
    call = eng.calls[-1]
    np.testing.assert_array_equal(call["key"], np.where(np.isnan(cvp["f*"].values), -1, cvp["obs_index"].values))
    assert call["sigma"] == 1.0 and call["max_dist"] is None
    # by hand: per observation, over its non-NaN rows, in raw units
    ok = ~np.isnan(cvp["f*"].values)
    ex, px = cvp.index.get_level_values("x").values, cvp["pred_loc_x"].values
    w = np.exp(-((px - ex) / 1.0) ** 2 / 2)
    raw = cvp["f_bar"].values + osc * cvp["f*"].values
    ids = np.unique(cvp["obs_index"].values[ok])
    np.testing.assert_array_equal(got["obs_index"].values, ids)
    for j, k in enumerate(ids):
        r = np.nonzero(ok & (cvp["obs_index"].values == k))[0]
        assert got["n_experts"].values[j] == len(r)
        np.testing.assert_allclose(got["f*"].values[j], (w[r] * raw[r]).sum() / w[r].sum(), rtol=1e-13)
        np.testing.assert_allclose(got["f*_var"].values[j], osc ** 2 * (w[r] * cvp["f*_var"].values[r]).sum() / w[r].sum(), rtol=1e-13)
        np.testing.assert_allclose(got["y_var"].values[j], osc ** 2 * (w[r] * cvp["y_var"].values[r]).sum() / w[r].sum(), rtol=1e-13)
        for c in ("track", "pred_loc_x", "pred_loc_y", "z"):          # carried: the first row's value
            assert got[c].values[j] == cvp[c].values[r[0]]
    np.testing.assert_allclose(got["z_score"].values,(got["z"].values - got["f*"].values) / np.sqrt(got["y_var"].values), rtol=1e-15)
    # max_dist in the xprt_loc_cols: fewer experts per observation, and observations that lose all of theirs keep a NaN row
    lim = post.glue_cv_predictions({"cv_preds": cvp}, ["x"], 3.0, max_dist=0.5, obs_scale=osc, engine=eng)
    assert eng.calls[-1]["max_dist"] == 0.5
    near = np.array([int((ok & (cvp["obs_index"].values == k) & (np.abs(px - ex) < 0.5)).sum()) for k in ids])
    np.testing.assert_array_equal(lim["n_experts"].values, near)
    assert (near == 0).any() and np.isnan(lim["f*"].values[near == 0]).all() and np.isfinite(lim["f*"].values[near > 0]).all()
    # two weight columns, the default: the first two coordinate columns
    two = post.glue_cv_predictions({"cv_preds": cvp}, None, 3.0, obs_scale=osc, engine=eng)
    w2 = w * np.exp(-((cvp["pred_loc_y"].values - 0.5) / 1.0) ** 2 / 2)
    r = np.nonzero(ok & (cvp["obs_index"].values == ids[3]))[0]
    np.testing.assert_allclose(two["f*"].values[3], (w2[r] * raw[r]).sum() / w2[r].sum(), rtol=1e-13)
    # what is refused
    with pytest.raises(TypeError, match="one number"):
        post.glue_cv_predictions({"cv_preds": cvp}, ["x"], {1.0: 3.0}, engine=eng)
    with pytest.raises(ValueError, match="xprt_loc_cols"):
        post.glue_cv_predictions({"cv_preds": cvp}, ["t"], 3.0, engine=eng)
    with pytest.raises(KeyError, match="cv_preds_B"):
        post.glue_cv_predictions({"cv_preds": cvp}, ["x"], 3.0, table_suffix="_B", engine=eng)


def test_glue_cv_predictions_non_integer_obs_index():
    labels = np.array([f"obs{j:02d}" for j in range(30)], dtype=object)[::-1]
    cvp_s, o, e = _cv_preds(labels)
    cvp_i, _, _ = _cv_preds(np.arange(30))
    eng = gk.GlueKeyedNumpyEngine()
    a = post.glue_cv_predictions({"cv_preds": cvp_s}, ["x"], 3.0, engine=eng)
    key = eng.calls[-1]["key"]
    assert key.dtype == np.int64 and key.min() == 0 and len(np.unique(key)) == len(np.unique(o))
    b = post.glue_cv_predictions({"cv_preds": cvp_i}, ["x"], 3.0, engine=eng)
    # the same groups under other names: the factorised keys run in order of first appearance
    a = a.assign(pos=[int(s[3:]) for s in a["obs_index"]]).sort_values("pos")
    b = b.assign(pos=29 - b["obs_index"].values).sort_values("pos")
    for c in ("f*", "f*_var", "y_var", "n_experts", "z", "z_score"):
        np.testing.assert_array_equal(a[c].values, b[c].values)
    # an observation column of another name leaves "z" to the standardised residual
    c = post.glue_cv_predictions({"cv_preds": cvp_i.rename(columns={"z": "elev"})}, ["x"], 3.0, engine=eng)
    assert list(c.columns)[-6:] == ["elev", "f*", "f*_var", "y_var", "n_experts", "z"]
    np.testing.assert_array_equal(c["z"].values, b.sort_values("obs_index")["z_score"].values)
    # a float index, and a signed integer one with a negative label, are factorised too
    for idx in (np.arange(30) + 0.5, np.arange(30) - 3):
        cvp_f, _, _ = _cv_preds(idx)
        c = post.glue_cv_predictions({"cv_preds": cvp_f}, ["x"], 3.0, engine=eng)
        assert eng.calls[-1]["key"].min() == 0 and len(c) == len(b)
        np.testing.assert_array_equal(np.sort(c["f*"].values), np.sort(b["f*"].values))


def test_scores_against_numpy():
    rng = np.random.default_rng(5)
    n = 40
    g = pd.DataFrame({"obs_index": np.arange(n), "track": rng.integers(0, 3, n), "sat": rng.integers(0, 2, n),
                      "pred_loc_x": rng.uniform(0, 1, n), "z": rng.normal(10, 1, n), "f*": rng.normal(10, 1, n),
                      "f*_var": rng.uniform(0.1, 0.2, n), "y_var": rng.uniform(0.5, 1.5, n),
                      "n_experts": rng.integers(1, 5, n)})
    g.loc[3, "n_experts"] = 0
    g.loc[3, ["f*", "f*_var", "y_var"]] = np.nan
    g.loc[8, "y_var"] = np.nan
    g.loc[11, "z"] = np.nan
    s = post.score_cv_predictions(g, by=["track", "sat"])
    assert list(s.columns) == ["track", "sat", "n", "n_missing", "bias", "rmse", "nll", "mean_z2"]
    assert len(s) == 1 + len(g.groupby(["track", "sat"]))

    def direct(sub):
        sub = sub[(sub["n_experts"] > 0) & sub[["z", "f*", "y_var"]].notna().all(axis=1)]
        y, mu, sig = sub["z"].values, sub["f*"].values, np.sqrt(sub["y_var"].values)
        return [len(sub), np.mean(mu - y), np.sqrt(np.mean((y - mu) ** 2)),
                np.mean(np.log(sig * np.sqrt(2 * np.pi)) + (y - mu) ** 2 / (2 * sig ** 2)), np.mean(((y - mu) / sig) ** 2)]

    cols = ["n", "bias", "rmse", "nll", "mean_z2"]
    np.testing.assert_allclose(s.iloc[0][cols].values.astype(float), direct(g), rtol=1e-14)
    assert s.iloc[0]["n_missing"] == 3 and pd.isna(s.iloc[0]["track"]) and pd.isna(s.iloc[0]["sat"])
    for _, row in s.iloc[1:].iterrows():
        sub = g[(g["track"] == row["track"]) & (g["sat"] == row["sat"])]
        np.testing.assert_allclose(row[cols].values.astype(float), direct(sub), rtol=1e-14)
        assert row["n"] + row["n_missing"] == len(sub)
    assert int(s["n_missing"].iloc[1:].sum()) == 3
    one = post.score_cv_predictions(g)
    assert len(one) == 1 and list(one.columns) == cols[:1] + ["n_missing"] + cols[1:]
    np.testing.assert_array_equal(one.iloc[0][cols].values.astype(float), s.iloc[0][cols].values.astype(float))
    # nothing to score: NaN, not an error
    none = post.score_cv_predictions(g.iloc[[3]])
    assert none.iloc[0]["n"] == 0 and none.iloc[0]["n_missing"] == 1 and np.isnan(none.iloc[0]["rmse"])


# ------------------------------------------------------------------------------------------------------------------
# the orchestrator keyword
# ------------------------------------------------------------------------------------------------------------------
def test_cv_glue_needs_cv_and_a_well_formed_option():
    loc, data, model, pred, _ = _configs()
    eng = CvGlueEngine()
    with pytest.raises(ValueError, match="cv_glue.*with cv"):
        BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv_glue={"inference_radius": 4.0})
    for bad in ({"R": 3}, {"inference_radius": 4.0, "sigma": 1}, "yes", {"inference_radius": -1.0}, {"inference_radius": {1: 2}},
                {"inference_radius": 4.0, "xprt_loc_cols": ["x", "y", "t"]}, {"inference_radius": 4.0, "xprt_loc_cols": ["nope"]},
                {"inference_radius": 4.0, "max_dist": float("nan")}):
        with pytest.raises(ValueError, match="cv_glue"):
            BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv="loo", cv_glue=bad)
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv="loo", cv_glue={"inference_radius": 4.0})
    assert oi.cv_glue == {"inference_radius": 4.0, "R": 3.0, "max_dist": None, "xprt_loc_cols": ["x", "y"]}
    assert oi.config["cv_glue"] == oi.cv_glue
    with pytest.raises(NotImplementedError, match="sharded"):             # refused where cv is
        oi.run(None, world_size=2)


def test_a_run_without_the_keyword_is_unchanged(tmp_path):
    loc, data, model, pred, _ = _configs()
    cv = {"by": ["track"]}
    base_oi = BatchedLocalExpertOI(loc, data, model, pred, engine=CvGlueEngine(), dtype="f64", cv=cv)
    none_oi = BatchedLocalExpertOI(loc, data, model, pred, engine=CvGlueEngine(), dtype="f64", cv=cv, cv_glue=None)
    assert "cv_glue" not in none_oi.config and none_oi.config == base_oi.config
    base, none = base_oi.run(str(tmp_path / "a"), store_every=7), none_oi.run(str(tmp_path / "b"), store_every=7)
    assert list(base) == list(none) and "cv_glued" not in none and "cv_scores" not in none
    assert not none_oi.engine.calls
    for name in base:
        a, b = (t.drop(columns=["run_time"], errors="ignore") for t in (base[name], none[name]))
        pd.testing.assert_frame_equal(a, b, check_exact=True)
        for c in a.columns:
            if a[c].dtype.kind == "f":
                assert a[c].values.tobytes() == b[c].values.tobytes(), (name, c)
    assert sorted(get_results(str(tmp_path / "a"))) == sorted(get_results(str(tmp_path / "b")))
    assert [e["config"] for e in __import__("json").load(open(tmp_path / "a" / "oi_config.json"))] == \
           [e["config"] for e in __import__("json").load(open(tmp_path / "b" / "oi_config.json"))]


@pytest.mark.parametrize("cv", ["loo", {"by": ["track"]}])
def test_orchestrator_glues_and_scores(tmp_path, cv):
    loc, data, model, pred, df = _configs()
    osc = 2.5
    df = df.copy()
    df["z"] = 40.0 + 3.0 * df["z"]
    df.index = np.arange(len(df))[::-1] * 10 + 7          # labels are not positions: the run keys on the position
    data = dict(data, data_source=df)
    model = dict(model, init_params=dict(model["init_params"], obs_scale=osc))
    opt = {"inference_radius": 4.0, "R": 2, "max_dist": 3.5, "xprt_loc_cols": ["x", "y"]}
    plain = BatchedLocalExpertOI(loc, data, model, pred, engine=CvGlueEngine(), dtype="f64", cv=cv).run(None, optimise=False)
    eng = CvGlueEngine()
    oi = BatchedLocalExpertOI(loc, data, model, pred, engine=eng, dtype="f64", cv=cv, cv_glue=opt)
    store = str(tmp_path / "s")
    out = oi.run(store, optimise=False, store_every=7, table_suffix="_A")          # several waves
    assert set(out) == {f"{k}_A" for k in plain} | {"cv_glued_A", "cv_scores_A"}
    for name, tab in plain.items():                       # every other table as without the keyword
        pd.testing.assert_frame_equal(out[f"{name}_A"].drop(columns=["run_time"], errors="ignore"),
                                      tab.drop(columns=["run_time"], errors="ignore"))
    cvp, glued, scores = out["cv_preds_A"], out["cv_glued_A"], out["cv_scores_A"]
    by = [] if cv == "loo" else ["track"]
    assert list(glued.columns) == ["obs_index"] + by + ["pred_loc_x", "pred_loc_y", "pred_loc_t", "z", "f*", "f*_var", "y_var", "n_experts", "z_score"]
    # one call, keyed on the positional row, with the option's sigma and limit
    assert len(eng.calls) == 1
    call = eng.calls[0]
    pos = pd.Index(df.index).get_indexer(cvp["obs_index"].values)
    np.testing.assert_array_equal(call["key"], np.where(np.isnan(cvp["f*"].values), -1, pos))
    assert call["sigma"] == 2.0 and call["max_dist"] == 3.5
    # one row per held-out observation, ascending position; the labels are the frame's
    held = np.unique(pos[~np.isnan(cvp["f*"].values)])
    np.testing.assert_array_equal(glued["obs_index"].values, df.index.values[held])
    np.testing.assert_array_equal(glued["z"].values, df["z"].values[held])
    np.testing.assert_array_equal(glued["pred_loc_x"].values, df["x"].values[held])
    # raw units: against the restatement on the converted rows
    vals = np.stack([cvp["f_bar"].values + osc * cvp["f*"].values, osc ** 2 * cvp["f*_var"].values, osc ** 2 * cvp["y_var"].values])
    p = np.stack([cvp["pred_loc_x"].values, cvp["pred_loc_y"].values])
    x = np.stack([cvp.index.get_level_values("x").values, cvp.index.get_level_values("y").values])
    keys, counts, want = gk.glue_keyed(call["key"], p, x, vals, 2.0, 3.5)
    np.testing.assert_array_equal(keys, held)
    np.testing.assert_array_equal(glued["n_experts"].values, counts)
    for i, c in enumerate(("f*", "f*_var", "y_var")):
        np.testing.assert_allclose(glued[c].values, want[i], rtol=RTOL, atol=ATOL)
    assert counts.max() > 1 and (counts == 0).any()       # overlapping experts, and observations beyond max_dist of all of theirs
    assert np.isnan(glued["f*"].values[counts == 0]).all() and np.isfinite(glued["f*"].values[counts > 0]).all()
    # the glued prediction is of the raw observation: residuals of the size of the predictive deviation, not of the offset 40
    resid = df["z"].values[held] - glued["f*"].values
    assert np.nanmax(np.abs(resid)) < 8 * np.sqrt(np.nanmax(glued["y_var"].values))
    # the same table from the public function on the run's own cv_preds (labels are unique here), and its scores
    again = post.glue_cv_predictions(out, ["x", "y"], 4.0, R=2, max_dist=3.5, obs_scale=osc, table_suffix="_A", engine=eng)
    pd.testing.assert_frame_equal(again.sort_values("obs_index", ascending=False).reset_index(drop=True), glued, check_exact=True)
    pd.testing.assert_frame_equal(scores, post.score_cv_predictions(glued, by=by or None), check_exact=True)
    assert len(scores) == 1 + (df["track"].nunique() if by else 0) and scores["n"].iloc[0] == int((counts > 0).sum())
    assert scores["n_missing"].iloc[0] == int((counts == 0).sum())
    # both tables are in the store, and the option in its configuration
    from gpsat_amd.local_experts import ResultStore
    on_disk = ResultStore(store).tables()
    pd.testing.assert_frame_equal(on_disk["cv_glued_A"], glued)
    assert len(on_disk["cv_scores_A"]) == len(scores)
    cfg = __import__("json").load(open(os.path.join(store, "oi_config_A.json")))
    assert cfg[-1]["config"]["cv_glue"] == {"inference_radius": 4.0, "R": 2.0, "max_dist": 3.5, "xprt_loc_cols": ["x", "y"]}
