"""CPU: RationalQuadratic experts without a GPU -- the ABI's constant and gpsat_n_hyper through a compiled C program, and the host
logic of HipGPRModel / Engine / BatchedLocalExpertOI with a device-free engine (variant_numpy's stand-in), and the restatement itself on the checks of tests/variant_cases.py."""
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
from variant_cases import check_gradient, check_matches_sklearn, check_sklearn_fixture, cpu_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tile, RqNumpyEngine = functools.partial(cpu_tile, vn.RQ), functools.partial(vn.NumpyEngine, vn.RQ)


# ---- the restatement: the shared checks of tests/variant_cases.py
@pytest.mark.parametrize("ell,s,sn2,alpha", [(0.7, 1.3, 0.05, 0.3), (1.5, 0.4, 0.2, 1.0), (2.5, 2.0, 0.01, 30.0)])
def test_rq_numpy_matches_sklearn(ell, s, sn2, alpha):
    """GaussianProcessRegressor(ConstantKernel(s) * RationalQuadratic(l, alpha), alpha=sn2, optimizer=None) at three theta with
    equal length scales."""
    check_matches_sklearn(vn.RQ, vn.RQ_KERNEL, 2, 1, 40, ell, s, sn2, alpha)


@pytest.mark.parametrize("D", [1, 2, 3])
def test_rq_numpy_gradient_matches_central_differences(D):
    check_gradient(vn.RQ, D)


def test_sklearn_fixture(golden_dir):
    check_sklearn_fixture(golden_dir, vn.RQ)


# ---- ABI
def test_abi_constant_and_n_hyper_through_c(tmp_path):
    prog = r'''
#include <stdio.h>
#include <dlfcn.h>
#include "gpsat_hip.h"
int main(int argc, char** argv) {
    void* h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    int (*nh)(int, int) = (int (*)(int, int))dlsym(h, "gpsat_n_hyper");
    int (*ver)(void) = (int (*)(void))dlsym(h, "gpsat_version");
    if (!nh || !ver) return 2;
    printf("%d %d %d\n", GPSAT_KERNEL_RQ, GPSAT_ABI_VERSION, ver());
    for (int k = -1; k <= 5; ++k) { for (int D = 0; D <= 5; ++D) printf("%d ", nh(k, D)); printf("\n"); }
    return 0;
}
'''
    cfile, exe = tmp_path / "nhyper.c", tmp_path / "nhyper"
    cfile.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe), "-ldl"], check=True)
    L.load()                                   # the library's own loading rules (one HIP runtime) are not this test's subject
    out = subprocess.run([str(exe), L.LIB_PATH], check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0].split() == ["4", "4", "4"]
    assert L.KERNEL_IDS["RationalQuadratic"] == 4 == L.KERNEL_RQ and L.ABI_VERSION == 4
    table = [[int(v) for v in line.split()] for line in out[1:8]]
    for row, k in zip(table, range(-1, 6)):
        for D, v in enumerate(row):
            if k == 4:
                want = D + 3 if 1 <= D <= 3 else 0
            else:
                want = D + 2 if (0 <= k <= 3 and 1 <= D <= 4) else 0
            assert v == want, (k, D, v)
            if want:
                assert L.n_hyper(k, D) == want
    assert L.n_hyper("RationalQuadratic", 3) == 6 and L.n_hyper("Matern32", 3) == 5


# ---- host logic with a device-free engine
class _NoDevice:
    device_name = "no device (host logic only)"
    device_id = 0


def test_model_param_names_accessors_and_fixed_params():
    X, y, _, _ = _tile(3, 12, 2)
    m = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic", dtype="f64",
                    kernel_kwargs={"lengthscales": [2.0, 3.0], "variance": 0.5})
    assert m.param_names == ["lengthscales", "kernel_variance", "likelihood_variance", "kernel_alpha"]
    assert m.get_kernel_alpha() == 1.0                                   # GPflow's default
    np.testing.assert_array_equal(m._theta, [2.0, 3.0, 0.5, 1.0, 1.0])
    m = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic", dtype="f64", noise_variance=0.2,
                    kernel_kwargs={"alpha": 2.5})
    np.testing.assert_array_equal(m._theta, [1.0, 1.0, 1.0, 0.2, 2.5])
    m.set_parameters(kernel_alpha=0.75, likelihood_variance=0.1)
    m.set_kernel_alpha(np.array([0.8]))
    assert m.get_parameters()["kernel_alpha"] == 0.8 and m.get_likelihood_variance() == 0.1
    assert set(m.get_parameters()) == set(m.param_names)
    m.set_parameter_constraints({"kernel_alpha": {"low": 1.0, "high": 20.0}}, move_within_tol=True, tol=1e-2)
    assert m.get_kernel_alpha() == pytest.approx(1.01)
    np.testing.assert_array_equal(m._lo[-1:], [1.0])
    np.testing.assert_array_equal(m._hi[-1:], [20.0])
    assert np.isnan(m._lo[:-1]).all() and m._lo.shape == (5,)
    with pytest.raises(AssertionError):
        m.set_kernel_alpha_constraints(low=[1.0, 2.0], high=[3.0, 4.0])
    m._fix_hyperparameters(["kernel_alpha", "kernel_variance"])
    assert m._trainable.tolist() == [True, True, False, True, False]
    # the other kernels keep the reference's three names
    m3 = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="Matern32")
    assert m3.param_names == ["lengthscales", "kernel_variance", "likelihood_variance"] and m3._theta.shape == (4,)
    with pytest.raises(AssertionError):
        m3.set_parameters(kernel_alpha=1.0)
    with pytest.raises(AttributeError):
        m3.get_kernel_alpha()


def test_model_refusals():
    X, y, _, _ = _tile(4, 12, 2)
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic", dtype="f32")
    with pytest.raises(NotImplementedError, match="dtype='f64'"):
        HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic")           # the default dtype is fp32
    X4 = np.random.default_rng(0).uniform(size=(12, 4))
    with pytest.raises(NotImplementedError, match="1..3 input dimensions"):
        HipGPRModel(coords=X4, obs=y, engine=_NoDevice(), kernel="RationalQuadratic", dtype="f64")
    with pytest.raises(NotImplementedError, match="SGPR"):
        HipSGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic")
    m = HipGPRModel(coords=X, obs=y, engine=_NoDevice(), kernel="RationalQuadratic", dtype="f64")
    with pytest.raises(NotImplementedError, match="held-out"):
        m.cross_validate()


def test_engine_states_the_expected_width():
    """The check runs before anything reaches the library."""
    eng = object.__new__(Engine)
    X, y, _, Xs = _tile(5, 10, 2)
    kw = dict(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, kernel="RationalQuadratic", dtype="f64", optimiser="none")
    with pytest.raises(GpsatError, match=r"H = D \+ 3 = 5"):
        eng.fit_predict_batch(theta0=np.ones((1, 4)), **kw)
    with pytest.raises(GpsatError, match="lo has shape"):
        eng.fit_predict_batch(theta0=np.ones(5), lo=np.zeros(4), hi=np.ones(5), **kw)
    with pytest.raises(GpsatError, match="trainable has shape"):
        eng.fit_predict_batch(theta0=np.ones(5), trainable=np.ones(4, bool), **kw)


def _rq_case(n_locs=6, seed=3):
    """One coordinate, y drawn from an RQ prior (alpha = 0.4): with this seed every tile's fitted alpha lies inside its box,
    so the move-within-tol of a later run leaves loaded values alone."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 10.0, 300))
    df = pd.DataFrame({"x": x, "y": vn.rq_prior_draw(rng, x[:, None], np.array([0.6]), 1.0, 0.05 ** 2, 0.4)})
    locs = np.linspace(2.0, 8.0, n_locs)
    radius = 2.0
    cfg = dict(expert_loc_config={"source": pd.DataFrame({"x": locs})},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel",
                             "init_params": {"kernel": "RationalQuadratic", "noise_variance": 0.05 ** 2},
                             "constraints": {"kernel_alpha": {"low": 0.1, "high": 20.0}, "lengthscales": {"low": 1e-3, "high": 10.0}},
                             "optim_kwargs": {"fixed_params": ["likelihood_variance"], "max_iter": 200}},
               pred_loc_config={"method": "from_dataframe", "df": pd.DataFrame({"x": np.linspace(0.5, 9.5, 40)}), "max_dist": 1.0})
    return cfg, locs


def test_orchestrator_stores_kernel_alpha_and_reads_it_back(tmp_path):
    cfg, locs = _rq_case()
    eng = RqNumpyEngine()
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    assert oi.dtype == "f64" and oi.H == 4 and oi.params_to_store[-1] == "kernel_alpha"
    store = str(tmp_path / "store")
    tabs = oi.run(store_path=store, store_every=3)                        # two waves
    assert len(eng.calls) == 2 and [c["T"] for c in eng.calls] == [3, 3]
    ka = tabs["kernel_alpha"]
    assert list(ka.columns) == ["_dim_0", "kernel_alpha"] and ka.index.tolist() == pytest.approx(locs.tolist())
    assert ((ka["kernel_alpha"] > 0.12) & (ka["kernel_alpha"] < 19.0)).all() and ka["kernel_alpha"].nunique() == len(locs)
    on_disk = get_results(store)
    assert {"lengthscales", "kernel_variance", "likelihood_variance", "kernel_alpha", "preds", "run_details"} <= set(on_disk)
    # the start: the defaults, alpha = 1 inside its box; the constraints reached the engine
    np.testing.assert_array_equal(eng.calls[0]["theta0"], np.tile([1.0, 1.0, 0.05 ** 2, 1.0], (3, 1)))
    # second run: parameters from the store, no optimisation -> the same predictions
    eng2 = RqNumpyEngine()
    cfg2 = {**cfg, "model_config": {**cfg["model_config"], "load_params": {"file": store, "table_suffix": ""}}}
    tabs2 = BatchedLocalExpertOI(engine=eng2, **cfg2).run(store_path=str(tmp_path / "store2"), optimise=False, table_suffix="_P")
    assert all(c["optimiser"] == "none" for c in eng2.calls)
    th_loaded = np.concatenate([c["theta0"] for c in eng2.calls])
    np.testing.assert_array_equal(th_loaded[:, 3], ka["kernel_alpha"].values)
    np.testing.assert_array_equal(th_loaded[:, 0], tabs["lengthscales"]["lengthscales"].values)
    np.testing.assert_array_equal(tabs2["preds_P"]["f*"].values, tabs["preds"]["f*"].values)
    np.testing.assert_array_equal(tabs2["preds_P"]["f*_var"].values, tabs["preds"]["f*_var"].values)
    np.testing.assert_array_equal(tabs2["kernel_alpha_P"]["kernel_alpha"].values, ka["kernel_alpha"].values)
    # direct values
    eng3 = RqNumpyEngine()
    cfg3 = {**cfg, "model_config": {**cfg["model_config"], "load_params": {"kernel_alpha": 3.0, "lengthscales": [0.8]}}}
    BatchedLocalExpertOI(engine=eng3, **cfg3).run(store_path=None, optimise=False)
    th3 = np.concatenate([c["theta0"] for c in eng3.calls])
    assert (th3[:, 3] == 3.0).all() and (th3[:, 0] == 0.8).all()


def test_orchestrator_previous_running_mean_includes_alpha():
    cfg, locs = _rq_case(n_locs=4)
    eng = RqNumpyEngine()
    cfgp = {**cfg, "model_config": {**cfg["model_config"], "load_params": {"previous": True}}}
    tabs = BatchedLocalExpertOI(engine=eng, **cfgp).run(store_path=None, engine_chunk=1)
    th0 = np.concatenate([c["theta0"] for c in eng.calls])
    alpha = tabs["kernel_alpha"]["kernel_alpha"].values
    ok = tabs["run_details"]["optimise_success"].values
    want = 1.0
    for k in range(len(locs)):
        assert th0[k, 3] == pytest.approx(min(max(want, 0.1 + 1e-2), 20.0 - 1e-2), rel=1e-14), k
        if ok[k]:
            want = 0.95 * want + 0.05 * alpha[k]
    assert ok.any() and not np.allclose(th0[:, 3], 1.0)


def test_orchestrator_refusals():
    cfg, _ = _rq_case()
    mc = cfg["model_config"]
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), dtype="f32", **cfg)
    with pytest.raises(NotImplementedError, match="replacement"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10}})
    m32 = {**mc, "init_params": {"kernel": "Matern32"}, "constraints": None, "replacement_threshold": 10,
           "replacement_init_params": {"kernel": "RationalQuadratic"}}
    with pytest.raises(NotImplementedError, match="replacement"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), dtype="f64", **{**cfg, "model_config": m32})
    for cv in ("loo", {"by": ["x"]}, {"by": ["x"], "refit": True}):
        with pytest.raises(NotImplementedError, match="cv"):
            BatchedLocalExpertOI(engine=RqNumpyEngine(), cv=cv, **cfg)
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), **{**cfg, "model_config": {**mc, "oi_model": "GPflowSGPRModel"}})
    df4 = pd.DataFrame(np.random.default_rng(0).uniform(size=(30, 5)), columns=["a", "b", "c", "d", "y"])
    cfg4 = {**cfg, "data_config": {"data_source": df4, "obs_col": ["y"], "coords_col": ["a", "b", "c", "d"], "local_select": []},
            "expert_loc_config": {"source": df4[["a", "b", "c", "d"]].iloc[:2]}, "pred_loc_config": {"method": "expert_loc"},
            "model_config": {**mc, "constraints": None}}
    with pytest.raises(NotImplementedError, match="1..3 coordinate columns"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), **cfg4)
    with pytest.raises(NotImplementedError, match="params_to_store"):
        BatchedLocalExpertOI(engine=RqNumpyEngine(), dtype="f64",
                             **{**cfg, "model_config": {**mc, "init_params": {"kernel": "Matern32"}, "constraints": None,
                                                        "params_to_store": ["kernel_alpha"]}})
