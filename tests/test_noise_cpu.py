"""CPU: known noise variances per observation (obs_var) without a GPU -- the ABI's struct through a compiled C program, the
host checks of gpsat_fit_predict_batch_noise (gpsat::check_noise), and the host logic of HipGPRModel / Engine /
BatchedLocalExpertOI with a device-free engine (variant_numpy's stand-in), and the restatement itself on the checks of tests/variant_cases.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel, HipSGPRModel, HipSklearnGPRModel
from oracle import gp_oracle as go
from variant_cases import KERNELS, check_gradient, check_matches_sklearn, check_sklearn_fixture, cpu_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tile, NoiseNumpyEngine = functools.partial(cpu_tile, vn.NOISE), functools.partial(vn.NumpyEngine, vn.NOISE)


# ---- the restatement
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", KERNELS)
def test_noise_numpy_matches_sklearn(kernel, D):
    """GaussianProcessRegressor(ConstantKernel(s) * {RBF, Matern nu}, alpha=sn2 + v, optimizer=None)."""
    check_matches_sklearn(vn.NOISE, kernel, D, D, 60, np.random.default_rng(D).uniform(0.7, 2.5, D), 1.3, 0.05)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_noise_numpy_gradient_matches_central_differences(D):
    check_gradient(vn.NOISE, D)


@pytest.mark.parametrize("kernel", KERNELS)
def test_constant_variance_is_the_oracle_at_a_larger_likelihood_variance(kernel):
    """v = 0.2 everywhere: the objective of the oracle at sn2 + 0.2, to 1e-12 relative; v = 0: the oracle itself."""
    X, y, _, Xs = _tile(4, 60, 3)
    theta = np.array([1.1, 2.0, 0.7, 0.9, 0.05])
    th2 = theta.copy()
    th2[4] += 0.2
    nll, g = vn.nll_and_grad(vn.NOISE, kernel, X, y, theta, np.full(60, 0.2))
    nll0, g0 = go.nll_and_grad(go.KERNEL_IDS[kernel], X, y, th2)
    print("relative difference", abs(nll - nll0) / abs(nll0))
    assert abs(nll - nll0) <= 1e-12 * abs(nll0)
    np.testing.assert_allclose(g, g0, rtol=1e-10, atol=1e-12)
    f, fv, yv = vn.predict(vn.NOISE, kernel, X, y, Xs, theta, np.full(60, 0.2))
    f0, fv0, yv0 = go.predict(go.KERNEL_IDS[kernel], X, y, Xs, th2)
    np.testing.assert_allclose(f, f0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fv, fv0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(yv, yv0 - 0.2, rtol=0, atol=1e-12)          # y_var leaves v out
    assert vn.nll_and_grad(vn.NOISE, kernel, X, y, theta, np.zeros(60))[0] == go.nll_and_grad(go.KERNEL_IDS[kernel], X, y, theta)[0]


@pytest.mark.parametrize("N,D", [(17, 1), (100, 3), (500, 4)])
def test_a_huge_variance_deletes_the_row(N, D):
    """v = 1e12 on every fifth row: f* and f*_var of the tile without these rows (each row meets its own variance).  The GPU
    test asks 1e-9 and 1e-10; here the two differ by far less."""
    X, y, Xs, theta = syn.make_tile(40 + N, N, 9, D, kid=2)
    v = np.zeros(N)
    v[::5] = 1e12
    keep = v == 0.0
    f, fv, _ = vn.predict(vn.NOISE, "Matern32", X, y, Xs, theta, v)
    f0, fv0, _ = go.predict(2, X[keep], y[keep], Xs, theta)
    print("N", N, "D", D, "mean", np.abs(f - f0).max(), "var", np.abs(fv - fv0).max())
    np.testing.assert_allclose(f, f0, rtol=0, atol=1e-11)
    np.testing.assert_allclose(fv, fv0, rtol=0, atol=1e-11)


def test_sklearn_fixture(golden_dir):
    check_sklearn_fixture(golden_dir, vn.NOISE)


def test_scipy_agrees_with_itself_from_two_starts_on_the_fit_case():
    """The GPU test holds the device's fit to SciPy's at nll 5e-5 and theta rtol 2e-3 (tests/test_gpu_noise.py); on these
    inputs SciPy from two starts agrees with itself to a tenth of that."""
    b, th0, lo, hi = vn.fit_case()
    for t in range(3):
        sl = slice(150 * t, 150 * (t + 1))
        a = vn.fit(vn.NOISE, "Matern32", b["X"][sl], b["y"][sl], th0[t], lo[t], hi[t], max_iter=1000, obs_var=b["obs_var"][sl])
        c = vn.fit(vn.NOISE, "Matern32", b["X"][sl], b["y"][sl], np.array([2.5, 0.6, 1.7, 0.3, 0.05]), lo[t], hi[t], max_iter=1000,
                   obs_var=b["obs_var"][sl])
        print("tile", t, "theta", a[0], c[0], "nll", a[1], c[1])
        assert a[2].success and c[2].success
        assert abs(a[1] - c[1]) <= 5e-6
        np.testing.assert_allclose(a[0], c[0], rtol=2e-4)
        assert 0.001 < a[0][4] < 0.02                     # sn2 is identified: near the draw's 0.004, not at its lower bound


# ---- ABI
def test_abi_struct_through_c_and_exports(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include <dlfcn.h>
#include "gpsat_hip.h"
int main(int argc, char** argv) {
    void* h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    int (*ver)(void) = (int (*)(void))dlsym(h, "gpsat_version");
    int (*fn)(gpsat_handle*, const gpsat_batch*, const gpsat_noise*) =
        (int (*)(gpsat_handle*, const gpsat_batch*, const gpsat_noise*))dlsym(h, "gpsat_fit_predict_batch_noise");
    if (!ver || !fn) return 2;
    printf("%d %d %d %d %d\n", (int)sizeof(gpsat_noise), (int)offsetof(gpsat_noise, obs_var), (int)offsetof(gpsat_noise, reserved),
           GPSAT_ABI_VERSION, ver());
    return 0;
}
'''
    cfile, exe = tmp_path / "noise_abi.c", tmp_path / "noise_abi"
    cfile.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe), "-ldl"], check=True)
    lib = L.load()
    out = subprocess.run([str(exe), L.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["40", "0", "8", "4", "4"]
    assert C.sizeof(L.GpsatNoise) == 40 and L.GpsatNoise.reserved.offset == 8 and L.ABI_VERSION == 4
    assert "gpsat_fit_predict_batch_noise" in L.EXPORTS and "gpsat_fit_predict_batch_noise" in L.OPTIONAL_EXPORTS
    assert hasattr(lib, "gpsat_fit_predict_batch_noise")
    header = open(os.path.join(ROOT, "include", "gpsat_hip.h")).read()
    assert "int gpsat_fit_predict_batch_noise(gpsat_handle *h, const gpsat_batch *b, const gpsat_noise *nz);" in header


def _batch(D=3, kernel=2, dtype=L.F64, memory=L.MEM_HOST):
    T, H = 3, D + 2
    keep = dict(obs_off=np.array([0, 4, 4, 9], dtype=np.int64), pred_off=np.zeros(T + 1, dtype=np.int64),
                theta0=np.ones((T, H)), nan=np.full((T, H), np.nan), tr=np.ones(H, dtype=np.uint8))
    b = L.GpsatBatch()
    b.T, b.D, b.dtype, b.kernel, b.memory, b.optimiser = T, D, dtype, kernel, memory, L.OPT_NONE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b.obs_off, b.pred_off, b.theta0, b.lo, b.hi, b.trainable = (p(keep[k]) for k in ("obs_off", "pred_off", "theta0", "nan", "nan", "tr"))
    return b, keep


def test_host_checks_of_the_noise_entry_point():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat11check_noiseEPK11gpsat_batchPK11gpsat_noisePcm")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.GpsatBatch), C.POINTER(L.GpsatNoise), C.c_char_p, C.c_size_t]

    def check(b, v, reserved=None, null=False):
        nz = L.GpsatNoise()
        nz.obs_var = None if v is None else v.ctypes.data_as(C.c_void_p)
        if reserved is not None:
            nz.reserved[reserved] = 1
        why = C.create_string_buffer(200)
        rc = fn(C.byref(b), None if null else C.byref(nz), why, 200)
        return rc, why.value.decode()

    v = np.array([0.0, 0.1, 0.0, 2.0, 0.3, 0.0, 1e12, 0.5, 0.25])
    for kern in range(4):
        for D in (1, 2, 3, 4):
            b, keep = _batch(D=D, kernel=kern)
            assert check(b, v) == (0, "") and check(b, None) == (0, "")
    b, keep = _batch()
    rc, why = check(b, v, null=True)
    assert rc == -1 and "noise is NULL" in why
    for i in (0, 7):
        for vv in (v, None):                                # reserved words are read whatever obs_var is
            rc, why = check(b, vv, reserved=i)
            assert rc == -1 and "reserved" in why
    for bad, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(kernel=L.KERNEL_RQ), "GPSAT_KERNEL_RQ")):
        b, keep = _batch(**bad)
        rc, why = check(b, v)
        assert rc == -1 and match in why, (bad, rc, why)
        assert check(b, None) == (0, "")                     # NULL obs_var asks nothing of the batch
    # a negative or non-finite entry: the message names the tile and the row inside it (tile 1 is empty)
    b, keep = _batch()
    for pos, val, tile, row in ((0, -1e-300, 0, 0), (3, np.nan, 0, 3), (4, np.inf, 2, 0), (8, -np.inf, 2, 4), (6, -0.5, 2, 2)):
        w = v.copy()
        w[pos] = val
        rc, why = check(b, w)
        assert rc == -1 and f"tile {tile}, row {row}" in why and "finite and not negative" in why, (pos, val, why)
    w = v.copy()
    w[2] = -0.0                                              # minus zero is zero
    assert check(b, w) == (0, "")
    # device mode: obs_var is not inspected (a pointer that must not be read)
    b, keep = _batch(memory=L.MEM_DEVICE)
    nz = L.GpsatNoise()
    nz.obs_var = 8
    why = C.create_string_buffer(200)
    assert fn(C.byref(b), C.byref(nz), why, 200) == 0
    # the entry point itself, before any device is touched
    assert lib.gpsat_fit_predict_batch_noise(None, C.byref(b), None) == -1
    assert "noise is NULL" in lib.gpsat_last_error().decode()


# ---- host logic with a device-free engine
class _NoDevice:
    device_name = "no device (host logic only)"
    device_id = 0


def test_model_scales_the_variances_and_hands_them_to_the_engine():
    X, y, v, Xs = _tile(4, 12, 2)
    eng = NoiseNumpyEngine()
    m = HipGPRModel(coords=X, obs=y, obs_var=v, engine=eng, dtype="f64", obs_scale=2.0, obs_mean="local",
                    kernel_kwargs={"lengthscales": 1.5}, noise_variance=0.05)
    assert m.param_names == ["lengthscales", "kernel_variance", "likelihood_variance"] and m._theta.shape == (4,)
    np.testing.assert_array_equal(m.obs_var, v / 4.0)                    # variances: divided by obs_scale squared
    theta = np.array([1.5, 1.5, 1.0, 0.05])
    ys = (y - y.mean()) / 2.0
    assert m.get_objective_function_value() == vn.nll_and_grad(vn.NOISE, "Matern32", X, ys, theta, v / 4.0, want_grad=False)[0]
    np.testing.assert_array_equal(eng.calls[-1]["obs_var"], v / 4.0)
    np.testing.assert_array_equal(m.predict(Xs)["f*"], vn.predict(vn.NOISE, "Matern32", X, ys, Xs, theta, v / 4.0)[0])
    assert m.optimise_parameters(fixed_params=["likelihood_variance"]) and m.get_likelihood_variance() == 0.05
    assert m.get_lengthscales()[0] != 1.5 and eng.calls[-1]["optimiser"] == "lbfgs"
    # the column form, beside data=
    df = pd.DataFrame({"a": X[:, 0], "b": X[:, 1], "obs": y, "var": v})
    m2 = HipGPRModel(data=df, coords_col=["a", "b"], obs_col="obs", obs_var_col="var", engine=eng, dtype="f64", obs_scale=2.0)
    np.testing.assert_array_equal(m2.obs_var, v / 4.0)
    # None is the model as it was: the engine is not handed an obs_var
    m3 = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), dtype="f64")
    assert m3.obs_var is None


def test_model_refusals():
    X, y, v, _ = _tile(4, 12, 2)
    kw = dict(coords=X, obs=y, engine=_NoDevice(), obs_var=v)
    for bad in (np.where(np.arange(12) == 3, np.nan, v), np.where(np.arange(12) == 3, -0.1, v), np.where(np.arange(12) == 5, np.inf, v),
                v[:11], np.concatenate([v, [0.1]])):
        with pytest.raises(AssertionError):
            HipGPRModel(**{**kw, "obs_var": bad}, dtype="f64")
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(dtype="f32", **kw)
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(**kw)                                                # the default dtype is fp32
    with pytest.raises(NotImplementedError, match="RationalQuadratic"):
        HipGPRModel(kernel="RationalQuadratic", dtype="f64", **kw)
    with pytest.raises(NotImplementedError, match="Constant"):
        HipGPRModel(mean_function="Constant", dtype="f64", **kw)
    with pytest.raises(NotImplementedError, match="likelihood"):
        HipGPRModel(dtype="f64", likelihood="Gaussian", **kw)            # stays refused as it is
    with pytest.raises(NotImplementedError, match="held-out"):
        HipGPRModel(dtype="f64", **kw).cross_validate()
    df = pd.DataFrame({"a": X[:, 0], "b": X[:, 1], "obs": y, "var": v})
    with pytest.raises(AssertionError, match="both"):
        HipGPRModel(data=df, coords_col=["a", "b"], obs_col="obs", obs_var_col="var", obs_var=v, engine=_NoDevice(), dtype="f64")
    with pytest.raises(AssertionError, match="data"):
        HipGPRModel(coords=X, obs=y, obs_var_col="var", engine=_NoDevice(), dtype="f64")
    for cls in (HipSGPRModel, HipSklearnGPRModel):
        with pytest.raises(NotImplementedError, match="obs_var"):
            cls(coords=X, obs=y, obs_var=v, engine=_NoDevice())
        with pytest.raises(NotImplementedError, match="obs_var"):
            cls(data=df, coords_col=["a", "b"], obs_col="obs", obs_var_col="var", engine=_NoDevice())


def test_engine_refuses_before_any_library_call():
    eng = object.__new__(Engine)                                         # no handle, no library: a call would fail otherwise
    X, y, v, Xs = _tile(5, 10, 2)
    kw = dict(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, optimiser="none", obs_var=v, theta0=np.ones(4))
    with pytest.raises(GpsatError, match="f32"):
        eng.fit_predict_batch(**kw)                                      # the default dtype is fp32
    with pytest.raises(GpsatError, match="f32"):
        eng.fit_predict_batch(dtype="f32", **kw)
    for more, match in ((dict(n_starts=2), "n_starts"), (dict(cv_fold="loo"), "cv_fold"),
                        (dict(cv_fold=np.zeros(10, np.int32), cv_refit=True), "cv_fold|cv_refit"),
                        (dict(mean="constant", theta0=np.ones(5)), "mean='constant'"), (dict(kernel="RationalQuadratic", theta0=np.ones(5)), "RationalQuadratic")):
        with pytest.raises(GpsatError, match=match):
            eng.fit_predict_batch(dtype="f64", **{**kw, **more})
    with pytest.raises(GpsatError, match="9 variances for 10 rows"):
        eng.fit_predict_batch(dtype="f64", **{**kw, "obs_var": v[:9]})
    with pytest.raises(NotImplementedError, match="obs_var"):
        eng.sgpr_fit_predict_batch(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, z_off=[0, 3], Z=X[:3], theta0=np.ones(4), obs_var=v)


def _noise_case(n_locs=6, seed=3):
    """One coordinate, binned-looking data: a smooth signal, every row with its own known error variance."""
    rng = np.random.default_rng(seed)
    x = np.sort(np.concatenate([rng.uniform(0.0, 10.0, 150), rng.normal(3.0, 0.3, 80), rng.normal(7.0, 0.2, 70)]))
    var = rng.uniform(0.0, 0.02, len(x))
    var[::7] = 0.0
    df = pd.DataFrame({"x": x, "y": 0.2 * np.sin(1.3 * x) + np.sqrt(var + 0.03 ** 2) * rng.standard_normal(len(x)), "var": var})
    locs = np.linspace(2.0, 8.0, n_locs)
    radius = 2.0
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"], "obs_var_col": "var",
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": {"noise_variance": 0.03 ** 2, "obs_scale": 0.5},
                             "constraints": {"lengthscales": {"low": 1e-3, "high": 10.0}},
                             "optim_kwargs": {"fixed_params": ["likelihood_variance"], "max_iter": 200}},
               pred_loc_config={"method": "from_dataframe", "df": pd.DataFrame({"x": np.linspace(0.5, 9.5, 40)}), "max_dist": 1.0})
    return cfg, locs, df, radius


def test_orchestrator_carries_the_column_to_the_right_rows(tmp_path):
    cfg, locs, df, radius = _noise_case()
    eng = NoiseNumpyEngine()
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    assert oi.dtype == "f64" and oi.H == 3 and oi.extra is None and oi.obs_var_col == "var"
    assert oi.config["data"]["obs_var_col"] == "var"                      # recorded in oi_config
    assert oi.param_names == ["lengthscales", "kernel_variance", "likelihood_variance"]
    tabs = oi.run(store_path=str(tmp_path / "store"), store_every=4)      # two waves: 4 + 2 experts
    assert [c["T"] for c in eng.calls] == [4, 2]
    assert {"lengthscales", "kernel_variance", "likelihood_variance", "preds", "run_details"} <= set(tabs)
    assert "obs_var" not in tabs and "var" not in tabs                    # tables are unchanged
    # every tile: the rows the selection gives it, y and obs_var in the same order, both in scaled units; neighbouring
    # experts share rows (radius 2.0, spacing 1.2)
    k = 0
    shared = 0
    for c in eng.calls:
        for t in range(c["T"]):
            a, e = c["obs_off"][t], c["obs_off"][t + 1]
            d = df[(df["x"] <= locs[k] + radius) & (df["x"] >= locs[k] - radius)]
            np.testing.assert_array_equal(c["X"][a:e, 0], d["x"].values)
            np.testing.assert_array_equal(c["y"][a:e], d["y"].values / 0.5)
            np.testing.assert_array_equal(c["obs_var"][a:e], d["var"].values / 0.25)
            if k + 1 < len(locs):
                shared += int((d["x"] >= locs[k + 1] - radius).sum())
            k += 1
    assert k == len(locs) and shared > 100
    # the tables are those of the per-tile model with obs_var_col
    for k, loc in enumerate(locs):
        d = df[(df["x"] <= loc + radius) & (df["x"] >= loc - radius)]
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x"], obs_var_col="var", engine=NoiseNumpyEngine(), dtype="f64",
                        **cfg["model_config"]["init_params"])
        m.set_parameter_constraints(cfg["model_config"]["constraints"], move_within_tol=True, tol=1e-2)
        m.optimise_parameters(**cfg["model_config"]["optim_kwargs"])
        assert tabs["lengthscales"]["lengthscales"].values[k] == m.get_lengthscales()[0] != 1.0
        assert tabs["likelihood_variance"]["likelihood_variance"].values[k] == 0.03 ** 2
    # one expert per engine call: the chunks carry their own rows
    eng2 = NoiseNumpyEngine()
    tabs2 = BatchedLocalExpertOI(engine=eng2, **cfg).run(store_path=None, engine_chunk=1)
    assert len(eng2.calls) == len(locs)
    np.testing.assert_array_equal(tabs2["preds"]["f*"].values, tabs["preds"]["f*"].values)
    np.testing.assert_array_equal(np.concatenate([c["obs_var"] for c in eng2.calls]), np.concatenate([c["obs_var"] for c in eng.calls]))


def test_orchestrator_refusals():
    cfg, _, df, _ = _noise_case()
    mc, dc = cfg["model_config"], cfg["data_config"]
    E = NoiseNumpyEngine
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(engine=E(), dtype="f32", **cfg)
    with pytest.raises(NotImplementedError, match="replacement"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10}})
    for cv in ("loo", {"by": ["x"]}, {"by": ["x"], "refit": True}):
        with pytest.raises(NotImplementedError, match="cv"):
            BatchedLocalExpertOI(engine=E(), cv=cv, **cfg)
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "oi_model": "GPflowSGPRModel"}})
    with pytest.raises(NotImplementedError, match="cannot be combined"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {"kernel": "RationalQuadratic"}}})
    with pytest.raises(NotImplementedError, match="cannot be combined"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {"mean_function": "Constant"}}})
    with pytest.raises(KeyError, match="obs_var_col"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "data_config": {**dc, "obs_var_col": "nope"}})
    with pytest.raises(ValueError, match="one column name"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "data_config": {**dc, "obs_var_col": ["var"]}})
    bad = df.copy()
    bad.loc[5, "var"] = -1.0
    with pytest.raises(AssertionError, match="obs_var"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "data_config": {**dc, "data_source": bad}}).run(store_path=None)
    # without the key: the run as it was, fp32 by default
    oi = BatchedLocalExpertOI(engine=E(), **{**cfg, "data_config": {k: v for k, v in dc.items() if k != "obs_var_col"}})
    assert oi.dtype == "f32" and oi.obs_var_col is None
