"""CPU: experts with a trainable constant mean (mean_function="Constant") without a GPU -- the ABI's struct, constants and
gpsat_n_hyper_mean through a compiled C program, the host checks of gpsat_fit_predict_batch_mean, and the host logic of
HipGPRModel / Engine / BatchedLocalExpertOI with a device-free engine (variant_numpy's stand-in), and the restatement itself on the checks of tests/variant_cases.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd.engine import Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI, get_results
from gpsat_amd.models import HipGPRModel, HipSGPRModel
from oracle import gp_oracle as go
from variant_cases import KERNELS, check_gradient, cpu_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tile, MeanNumpyEngine = functools.partial(cpu_tile, vn.MEAN), functools.partial(vn.NumpyEngine, vn.MEAN)


# ---- the restatement
@pytest.mark.parametrize("D", [1, 2, 3])
def test_mean_numpy_gradient_matches_central_differences(D):
    check_gradient(vn.MEAN, D)


@pytest.mark.parametrize("kernel", KERNELS)
def test_gls_identity(kernel):
    """c - 1^T K_y^-1 y / 1^T K_y^-1 1 = (dnll/dc) / (1^T K_y^-1 1) at any theta: the stationary c is the generalised
    least-squares level.  Independent of how the gradient was computed."""
    X, y, _, _ = _tile(3, 40, 2)
    for c in (-0.7, 0.0, 0.3, 2.5):
        theta = np.array([1.3, 0.9, 0.6, 0.05, c])
        _, g = vn.nll_and_grad(vn.MEAN, kernel, X, y, theta)
        left, right = vn.gls_sides(kernel, X, y, theta, g[-1])
        assert left == pytest.approx(right, rel=1e-9, abs=1e-12 * max(abs(c), 1.0)), (kernel, c)


def test_predictions_are_the_zero_mean_models_on_the_residual():
    X, y, _, Xs = _tile(5, 25, 2)
    theta = np.array([1.1, 2.0, 0.7, 0.03, 0.4])
    f, fv, yv = vn.predict(vn.MEAN, "Matern32", X, y, Xs, theta)
    f0, fv0, yv0 = go.predict(2, X, y - 0.4, Xs, theta[:4])
    np.testing.assert_array_equal(f, f0 + 0.4)
    np.testing.assert_array_equal(fv, fv0)
    np.testing.assert_allclose(np.diag(vn.predict_cov(vn.MEAN, "Matern32", X, y, Xs, theta)), fv, rtol=0, atol=1e-12)
    # the fit moves c off its start towards the GLS level, where dnll/dc vanishes
    th, nll, res = vn.fit(vn.MEAN, "Matern32", X, y, np.array([1.0, 1.0, 1.0, 1.0, 0.0]))
    assert res.success and th[-1] != 0.0
    left, right = vn.gls_sides("Matern32", X, y, th, vn.nll_and_grad(vn.MEAN, "Matern32", X, y, th)[1][-1])
    assert abs(left) < 1e-3 and left == pytest.approx(right, rel=1e-9, abs=1e-12)


# ---- ABI
def test_abi_struct_constants_and_n_hyper_mean_through_c(tmp_path):
    prog = r'''
#include <stdio.h>
#include <dlfcn.h>
#include "gpsat_hip.h"
int main(int argc, char** argv) {
    void* h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    int (*nh)(int, int, int) = (int (*)(int, int, int))dlsym(h, "gpsat_n_hyper_mean");
    int (*ver)(void) = (int (*)(void))dlsym(h, "gpsat_version");
    if (!nh || !ver || !dlsym(h, "gpsat_fit_predict_batch_mean")) return 2;
    printf("%d %d %d %d %d\n", (int)sizeof(gpsat_mean), GPSAT_MEAN_ZERO, GPSAT_MEAN_CONSTANT, GPSAT_ABI_VERSION, ver());
    for (int m = -1; m <= 2; ++m)
        for (int k = -1; k <= 5; ++k) { for (int D = 0; D <= 5; ++D) printf("%d ", nh(k, D, m)); printf("\n"); }
    return 0;
}
'''
    cfile, exe = tmp_path / "nhyper_mean.c", tmp_path / "nhyper_mean"
    cfile.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe), "-ldl"], check=True)
    L.load()
    out = subprocess.run([str(exe), L.LIB_PATH], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0].split() == ["32", "0", "1", "4", "4"]
    assert C.sizeof(L.GpsatMean) == 32 and (L.MEAN_ZERO, L.MEAN_CONSTANT) == (0, 1) and L.ABI_VERSION == 4
    rows = [[int(v) for v in line.split()] for line in out[1:1 + 4 * 7]]
    i = 0
    for m in range(-1, 3):
        for k in range(-1, 6):
            for D, v in enumerate(rows[i]):
                if m == 0:
                    want = (D + 3 if 1 <= D <= 3 else 0) if k == 4 else (D + 2 if (0 <= k <= 3 and 1 <= D <= 4) else 0)
                elif m == 1:
                    want = D + 3 if (0 <= k <= 3 and 1 <= D <= 3) else 0
                else:
                    want = 0
                assert v == want, (m, k, D, v)
                if want:
                    assert L.n_hyper(k, D, {0: None, 1: "constant"}[m]) == want
            i += 1
    assert L.n_hyper("Matern32", 3, "constant") == 6 and L.n_hyper("Matern32", 3) == 5 and L.n_hyper("Matern32", 3, None) == 5


# ---- the host checks of the entry point, without a device
def _batch(D=3, kernel=2, dtype=L.F64, T=2, c0=(0.3, -1.0)):
    H = D + 3
    keep = dict(obs_off=np.array([0, 4, 8][:T + 1], dtype=np.int64), pred_off=np.zeros(T + 1, dtype=np.int64),
                theta0=np.ones((T, H)), nan=np.full((T, H), np.nan), tr=np.ones(H, dtype=np.uint8))
    keep["theta0"][:, H - 1] = c0[:T]
    b = L.GpsatBatch()
    b.T, b.D, b.dtype, b.kernel, b.memory, b.optimiser = T, D, dtype, kernel, L.MEM_HOST, L.OPT_NONE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b.obs_off, b.pred_off, b.theta0, b.lo, b.hi, b.trainable = (p(keep[k]) for k in ("obs_off", "pred_off", "theta0", "nan", "nan", "tr"))
    return b, keep


def test_host_checks_of_the_mean_entry_point():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat10check_meanEPK11gpsat_batchPK10gpsat_meanPPKc")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.GpsatBatch), C.POINTER(L.GpsatMean), C.POINTER(C.c_char_p)]

    def check(b, kind=L.MEAN_CONSTANT, reserved=None):
        m = L.GpsatMean()
        m.kind = kind
        if reserved is not None:
            m.reserved[reserved] = 1
        why = C.c_char_p()
        rc = fn(C.byref(b), C.byref(m), C.byref(why))
        return rc, (why.value or b"").decode()

    for kern in range(4):
        for D in (1, 2, 3):
            b, keep = _batch(D=D, kernel=kern)
            assert check(b) == (0, "") and check(b, L.MEAN_ZERO) == (0, "")
    b, keep = _batch(c0=(0.0, -5.5))                          # zero and negatives are values of c like any other
    assert check(b) == (0, "")
    for bad, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(D=4), "D <= 3"), (dict(kernel=L.KERNEL_RQ), "GPSAT_KERNEL_RQ"),
                       (dict(c0=(0.3, np.nan)), "finite"), (dict(c0=(np.inf, 0.0)), "finite")):
        b, keep = _batch(**bad)
        rc, why = check(b)
        assert rc == -1 and match in why, (bad, rc, why)
        assert check(b, L.MEAN_ZERO) == (0, "")               # the zero mean asks nothing of the batch
    b, keep = _batch()
    for kind in (-1, 2, 7):
        rc, why = check(b, kind)
        assert rc == -1 and "unknown kind" in why
    for kind in (L.MEAN_ZERO, L.MEAN_CONSTANT):
        for i in (0, 6):
            rc, why = check(b, kind, reserved=i)
            assert rc == -1 and "reserved" in why
    # the entry point itself, before any device is touched
    assert lib.gpsat_fit_predict_batch_mean(None, C.byref(b), None) == -1
    assert "mean is NULL" in lib.gpsat_last_error().decode()


# ---- host logic with a device-free engine
class _NoDevice:
    device_name = "no device (host logic only)"
    device_id = 0


def test_model_param_names_accessors_and_fixed_params():
    X, y, _, _ = _tile(3, 12, 2)
    kw = dict(coords=X, obs=y, engine=_NoDevice(), dtype="f64", mean_function="Constant")
    m = HipGPRModel(kernel_kwargs={"lengthscales": [2.0, 3.0], "variance": 0.5}, **kw)
    assert m.param_names == ["lengthscales", "kernel_variance", "likelihood_variance", "mean_constant"]
    assert m.get_mean_constant() == 0.0                                  # GPflow's default
    np.testing.assert_array_equal(m._theta, [2.0, 3.0, 0.5, 1.0, 0.0])
    for c, want in ((0.25, 0.25), ([-1.5], -1.5), (np.array([2.0]), 2.0), (None, 0.0)):
        assert HipGPRModel(mean_func_kwargs={"c": c}, noise_variance=0.2, **kw)._theta.tolist() == [1.0, 1.0, 1.0, 0.2, want]
    with pytest.raises(AssertionError):
        HipGPRModel(mean_func_kwargs={"c": [1.0, 2.0]}, **kw)
    with pytest.raises(NotImplementedError, match="'c' only"):
        HipGPRModel(mean_func_kwargs={"A": 1.0}, **kw)
    m.set_parameters(mean_constant=-0.75, likelihood_variance=0.1)
    assert m.get_parameters()["mean_constant"] == -0.75 and m.get_likelihood_variance() == 0.1
    m.set_mean_constant(np.array([0.8]))
    assert m.get_mean_constant() == 0.8 and set(m.get_parameters()) == set(m.param_names)
    with pytest.raises(AssertionError):
        m.set_mean_constant(np.nan)
    assert np.isnan(m._lo).all() and m._lo.shape == (5,)                 # unconstrained until a box is set
    m.set_parameter_constraints({"mean_constant": {"low": -1.0, "high": 0.5}}, move_within_tol=True, tol=1e-2)
    assert m.get_mean_constant() == pytest.approx(0.49)
    np.testing.assert_array_equal(m._lo[-1:], [-1.0])
    np.testing.assert_array_equal(m._hi[-1:], [0.5])
    assert np.isnan(m._lo[:-1]).all()
    with pytest.raises(AssertionError):
        m.set_mean_constant_constraints(low=[1.0, 2.0], high=[3.0, 4.0])
    with pytest.raises(NotImplementedError, match="scale"):
        m.set_mean_constant_constraints(low=-1.0, high=1.0, scale=True)
    m._fix_hyperparameters(["mean_constant", "kernel_variance"])
    assert m._trainable.tolist() == [True, True, False, True, False]
    # None and "Zero" are the model as it was
    for mf in (None, "Zero"):
        m3 = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), mean_function=mf)
        assert m3.param_names == ["lengthscales", "kernel_variance", "likelihood_variance"] and m3._theta.shape == (4,)
        with pytest.raises(AssertionError):
            m3.set_parameters(mean_constant=1.0)
        with pytest.raises(AttributeError):
            m3.get_mean_constant()
        with pytest.raises(AttributeError):
            m3.set_mean_constant_constraints(low=0.0, high=1.0)


def test_model_hands_the_mean_to_the_engine():
    X, y, _, Xs = _tile(4, 12, 2)
    eng = MeanNumpyEngine()
    m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", mean_function="Constant", mean_func_kwargs={"c": 0.3},
                    kernel_kwargs={"lengthscales": 1.5}, noise_variance=0.05)
    theta = np.array([1.5, 1.5, 1.0, 0.05, 0.3])
    assert m.get_objective_function_value() == vn.nll_and_grad(vn.MEAN, "Matern32", X, y, theta, want_grad=False)[0]
    np.testing.assert_array_equal(m.predict(Xs)["f*"], vn.predict(vn.MEAN, "Matern32", X, y, Xs, theta)[0])
    assert m.optimise_parameters(fixed_params=["likelihood_variance"]) and m.get_mean_constant() != 0.3
    assert m.get_likelihood_variance() == 0.05


def test_model_refusals():
    X, y, _, _ = _tile(4, 12, 2)
    kw = dict(coords=X, obs=y, engine=_NoDevice(), mean_function="Constant")
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(dtype="f32", **kw)
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(**kw)                                                # the default dtype is fp32
    X4 = np.random.default_rng(0).uniform(size=(12, 4))
    with pytest.raises(NotImplementedError, match="1..3 input dimensions"):
        HipGPRModel(**{**kw, "coords": X4}, dtype="f64")
    with pytest.raises(NotImplementedError, match="RationalQuadratic"):
        HipGPRModel(kernel="RationalQuadratic", dtype="f64", **kw)
    for mf in ("Linear", "Polynomial", "constant", 1.0, object()):
        with pytest.raises(NotImplementedError, match="mean_function"):
            HipGPRModel(**{**kw, "mean_function": mf}, dtype="f64")
    with pytest.raises(NotImplementedError, match="likelihood"):
        HipGPRModel(dtype="f64", likelihood="Gaussian", **kw)
    for mf in ("Constant", "Zero"):
        with pytest.raises(NotImplementedError, match="mean_function"):
            HipSGPRModel(**{**kw, "mean_function": mf})
    with pytest.raises(NotImplementedError, match="held-out"):
        HipGPRModel(dtype="f64", **kw).cross_validate()


def test_engine_refuses_before_any_library_call():
    eng = object.__new__(Engine)                                         # no handle, no library: a call would fail otherwise
    X, y, _, Xs = _tile(5, 10, 2)
    kw = dict(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, dtype="f64", optimiser="none", mean="constant")
    with pytest.raises(GpsatError, match=r"H = D \+ 3 = 5"):
        eng.fit_predict_batch(theta0=np.ones((1, 4)), **kw)
    with pytest.raises(GpsatError, match="lo has shape"):
        eng.fit_predict_batch(theta0=np.ones(5), lo=np.zeros(4), hi=np.ones(5), **kw)
    with pytest.raises(GpsatError, match="trainable has shape"):
        eng.fit_predict_batch(theta0=np.ones(5), trainable=np.ones(4, bool), **kw)
    for more, match in ((dict(n_starts=2), "n_starts"), (dict(cv_fold="loo"), "cv_fold"),
                        (dict(cv_fold=np.zeros(10, np.int32), cv_refit=True), "cv_fold|cv_refit"),
                        (dict(kernel="RationalQuadratic"), "RationalQuadratic")):
        with pytest.raises(GpsatError, match=match):
            eng.fit_predict_batch(theta0=np.ones(5), **kw, **more)
    with pytest.raises(GpsatError, match="mean"):
        eng.fit_predict_batch(theta0=np.ones(5), **{**kw, "mean": "linear"})


def _mean_case(n_locs=6, seed=3):
    """One coordinate, a smooth signal on a level of 0.3 sampled in clusters."""
    rng = np.random.default_rng(seed)
    x = np.sort(np.concatenate([rng.uniform(0.0, 10.0, 150), rng.normal(3.0, 0.3, 80), rng.normal(7.0, 0.2, 70)]))
    df = pd.DataFrame({"x": x, "y": 0.3 + 0.2 * np.sin(1.3 * x) + 0.05 * rng.standard_normal(len(x))})
    locs = np.linspace(2.0, 8.0, n_locs)
    radius = 2.0
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel",
                             "init_params": {"mean_function": "Constant", "mean_func_kwargs": {"c": 0.1}, "noise_variance": 0.05 ** 2},
                             "constraints": {"mean_constant": {"low": -2.0, "high": 2.0}, "lengthscales": {"low": 1e-3, "high": 10.0}},
                             "optim_kwargs": {"fixed_params": ["likelihood_variance"], "max_iter": 200}},
               pred_loc_config={"method": "from_dataframe", "df": pd.DataFrame({"x": np.linspace(0.5, 9.5, 40)}), "max_dist": 1.0})
    return cfg, locs


def test_orchestrator_stores_mean_constant_and_reads_it_back(tmp_path):
    cfg, locs = _mean_case()
    eng = MeanNumpyEngine()
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    assert oi.dtype == "f64" and oi.H == 4 and oi.params_to_store[-1] == "mean_constant" and not oi.rq
    store = str(tmp_path / "store")
    tabs = oi.run(store_path=store, store_every=3)                        # two waves
    assert len(eng.calls) == 2 and [c["T"] for c in eng.calls] == [3, 3]
    mc = tabs["mean_constant"]
    assert list(mc.columns) == ["_dim_0", "mean_constant"] and mc.index.tolist() == pytest.approx(locs.tolist())
    assert ((mc["mean_constant"] > 0.0) & (mc["mean_constant"] < 0.6)).all() and mc["mean_constant"].nunique() == len(locs)
    on_disk = get_results(store)
    assert {"lengthscales", "kernel_variance", "likelihood_variance", "mean_constant", "preds", "run_details"} <= set(on_disk)
    # the start: the defaults and c of mean_func_kwargs; the box reached the engine
    np.testing.assert_array_equal(eng.calls[0]["theta0"], np.tile([1.0, 1.0, 0.05 ** 2, 0.1], (3, 1)))
    np.testing.assert_array_equal(eng.calls[0]["lo"][:, 3], -2.0)
    np.testing.assert_array_equal(eng.calls[0]["hi"][:, 3], 2.0)
    # second run: parameters from the store, no optimisation -> the same predictions
    eng2 = MeanNumpyEngine()
    cfg2 = {**cfg, "model_config": {**cfg["model_config"], "load_params": {"file": store, "table_suffix": ""}}}
    tabs2 = BatchedLocalExpertOI(engine=eng2, **cfg2).run(store_path=str(tmp_path / "store2"), optimise=False, table_suffix="_P")
    assert all(c["optimiser"] == "none" for c in eng2.calls)
    th_loaded = np.concatenate([c["theta0"] for c in eng2.calls])
    np.testing.assert_array_equal(th_loaded[:, 3], mc["mean_constant"].values)
    np.testing.assert_array_equal(th_loaded[:, 0], tabs["lengthscales"]["lengthscales"].values)
    np.testing.assert_array_equal(tabs2["preds_P"]["f*"].values, tabs["preds"]["f*"].values)
    np.testing.assert_array_equal(tabs2["mean_constant_P"]["mean_constant"].values, mc["mean_constant"].values)
    # direct values, a negative c among them; and without a box
    eng3 = MeanNumpyEngine()
    cfg3 = {**cfg, "model_config": {**cfg["model_config"], "constraints": None,
                                    "load_params": {"mean_constant": -0.4, "lengthscales": [0.8]}}}
    BatchedLocalExpertOI(engine=eng3, **cfg3).run(store_path=None, optimise=False)
    th3 = np.concatenate([c["theta0"] for c in eng3.calls])
    assert (th3[:, 3] == -0.4).all() and (th3[:, 0] == 0.8).all() and np.isnan(eng3.calls[0]["lo"][:, 3]).all()


def test_orchestrator_previous_running_mean_includes_the_constant():
    cfg, locs = _mean_case(n_locs=4)
    eng = MeanNumpyEngine()
    cfgp = {**cfg, "model_config": {**cfg["model_config"], "load_params": {"previous": True}}}
    tabs = BatchedLocalExpertOI(engine=eng, **cfgp).run(store_path=None, engine_chunk=1)
    th0 = np.concatenate([c["theta0"] for c in eng.calls])
    cs = tabs["mean_constant"]["mean_constant"].values
    ok = tabs["run_details"]["optimise_success"].values
    want = 0.1
    for k in range(len(locs)):
        assert th0[k, 3] == pytest.approx(want, rel=1e-14), k
        if ok[k]:
            want = 0.95 * want + 0.05 * cs[k]
    assert ok.any() and not np.allclose(th0[:, 3], 0.1)


def test_orchestrator_refusals():
    cfg, _ = _mean_case()
    mc = cfg["model_config"]
    E = MeanNumpyEngine
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(engine=E(), dtype="f32", **cfg)
    with pytest.raises(NotImplementedError, match="replacement"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10}})
    m32 = {**mc, "init_params": {"kernel": "Matern32"}, "constraints": None, "replacement_threshold": 10,
           "replacement_init_params": {"mean_function": "Constant"}}
    with pytest.raises(NotImplementedError, match="replacement"):
        BatchedLocalExpertOI(engine=E(), dtype="f64", **{**cfg, "model_config": m32})
    for cv in ("loo", {"by": ["x"]}, {"by": ["x"], "refit": True}):
        with pytest.raises(NotImplementedError, match="cv"):
            BatchedLocalExpertOI(engine=E(), cv=cv, **cfg)
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "oi_model": "GPflowSGPRModel"}})
    with pytest.raises(NotImplementedError, match="cannot be combined"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {**mc["init_params"], "kernel": "RationalQuadratic"}}})
    for mf in ("Linear", 3):
        with pytest.raises(NotImplementedError, match="mean_function"):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {"mean_function": mf}, "constraints": None}})
    df4 = pd.DataFrame(np.random.default_rng(0).uniform(size=(30, 5)), columns=["a", "b", "c", "d", "y"])
    cfg4 = {**cfg, "data_config": {"data_source": df4, "obs_col": ["y"], "coords_col": ["a", "b", "c", "d"], "local_select": []},
            "expert_loc_config": {"source": df4[["a", "b", "c", "d"]].iloc[:2]}, "pred_loc_config": {"method": "expert_loc"},
            "model_config": {**mc, "constraints": None}}
    with pytest.raises(NotImplementedError, match="1..3 coordinate columns"):
        BatchedLocalExpertOI(engine=E(), **cfg4)
    with pytest.raises(NotImplementedError, match="params_to_store"):
        BatchedLocalExpertOI(engine=E(), dtype="f64",
                             **{**cfg, "model_config": {**mc, "init_params": {"kernel": "Matern32"}, "constraints": None,
                                                        "params_to_store": ["mean_constant"]}})
    # "Zero" is the zero mean: the reference's three tables, fp32 by default
    oi = BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {"mean_function": "Zero"}, "constraints": None}})
    assert oi.dtype == "f32" and oi.H == 3 and oi.extra is None
