"""CPU: the gradient of the posterior mean at the prediction points and its variance (pred_grad) without a GPU -- the restatement
of tests/pred_grad_numpy.py against differences of variant_numpy and against torch autograd, the ABI's struct through a compiled
C program, the host checks of gpsat_fit_predict_batch_grad (gpsat::check_pred_grad), and the host logic of Engine, the models and
BatchedLocalExpertOI with a device-free engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import pred_grad_numpy as pg
import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import variants as V
from gpsat_amd.engine import BatchResult, Engine, GpsatError
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel, HipSGPRModel, HipSklearnGPRModel
from variant_cases import cpu_tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile(D, N=60, P=9):
    """Inputs U(0, 4); prediction point 0 is observation 5."""
    X, y, _, Xs = cpu_tile(vn.NOISE, 20 + D, N, D, P=P)
    Xs[0] = X[5]
    theta = np.concatenate([np.random.default_rng(D).uniform(0.8, 2.0, D), [0.9, 0.07]])
    return X, y, Xs, theta


# ---- the restatement
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", pg.KERNELS)
def test_mean_gradient_matches_central_differences(kernel, D):
    """Central differences of variant_numpy.predict's mean, h = 1e-5: to 1e-7."""
    X, y, Xs, theta = _tile(D)
    fg, _ = pg.predict_grad(kernel, X, y, Xs, theta)
    h, fd = 1e-5, np.empty_like(fg)
    for a in range(D):
        e = np.zeros(D)
        e[a] = h
        fd[:, a] = (pg.plain_predict(kernel, X, y, Xs + e, theta)[0] - pg.plain_predict(kernel, X, y, Xs - e, theta)[0]) / (2 * h)
    print(kernel, D, "largest error", np.abs(fg - fd).max())
    assert np.abs(fg).max() > 1e-2
    np.testing.assert_allclose(fg, fd, rtol=0, atol=1e-7)


def _second_difference(cov_of, x, a, h):
    """d^2 C(x, x') / dx_a dx'_a at x' = x from the 2 x 2 covariance of x + h e_a and x - h e_a."""
    e = np.zeros(len(x))
    e[a] = h
    c = cov_of(np.stack([x + e, x - e]))
    return (c[0, 0] - c[0, 1] - c[1, 0] + c[1, 1]) / (4 * h * h)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", pg.KERNELS)
def test_variance_matches_the_second_difference_of_the_posterior_covariance(kernel, D):
    """The mixed second difference of variant_numpy.predict_cov, h = 1e-3: 1e-3 relative for RBF and Matern52.  Matern32: 2e-2,
    because its |r|^3 term makes the difference's error O(h), not O(h^2)."""
    X, y, Xs, theta = _tile(D)
    _, fgv = pg.predict_grad(kernel, X, y, Xs, theta)
    fd = np.array([[_second_difference(lambda q: pg.plain_predict_cov(kernel, X, y, q, theta), Xs[p], a, 1e-3) for a in range(D)]
                   for p in range(len(Xs))])
    rel = np.abs(fgv - fd) / np.abs(fd)
    print(kernel, D, "largest relative error", rel.max())
    assert (fgv > 0).all()
    assert rel.max() <= (2e-2 if kernel == "Matern32" else 1e-3)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", pg.KERNELS)
def test_mean_gradient_matches_torch_autograd(kernel, D):
    """A second route: autograd through a torch fp64 restatement of the posterior mean k(x*, X) K_y^-1 y, to 1e-10."""
    import torch
    X, y, Xs, theta = _tile(D)
    alpha = np.linalg.solve(vn.K_y(vn.NOISE, kernel, X, theta, np.zeros(len(X))), y)
    ell, sf2 = torch.tensor(theta[:D]), float(theta[D])
    xs = torch.tensor(Xs, requires_grad=True)
    d = (torch.tensor(X)[:, None, :] - xs[None, :, :]) / ell
    r2 = (d * d).sum(-1)
    if kernel == "RBF":
        k = torch.exp(-0.5 * r2)
    else:
        r = torch.sqrt(torch.clamp(r2, min=1e-36))                   # the floor's derivative is 0: no 0 / 0 at r = 0
        s = (3.0 if kernel == "Matern32" else 5.0) ** 0.5 * r
        k = (1.0 + s) * torch.exp(-s) if kernel == "Matern32" else (1.0 + s + s * s / 3.0) * torch.exp(-s)
    (sf2 * k * torch.tensor(alpha)[:, None]).sum().backward()
    fg, _ = pg.predict_grad(kernel, X, y, Xs, theta)
    print(kernel, D, "largest error", np.abs(fg - xs.grad.numpy()).max())
    np.testing.assert_allclose(fg, xs.grad.numpy(), rtol=0, atol=1e-10)


@pytest.mark.parametrize("kernel", pg.KERNELS)
def test_empty_tile_returns_the_prior(kernel):
    D, theta = 3, np.array([1.3, 0.7, 2.0, 0.9, 0.05])
    fg, fgv = pg.predict_grad(kernel, np.zeros((0, D)), np.zeros(0), np.ones((4, D)), theta)
    assert fg.shape == fgv.shape == (4, D) and (fg == 0.0).all()
    np.testing.assert_array_equal(fgv, np.tile(0.9 * pg.GG0[kernel] / theta[:D] ** 2, (4, 1)))
    # gg(0) itself: the mixed second difference of the prior covariance (O(h) for Matern32, as above)
    for a in range(D):
        fd = _second_difference(lambda q: vn.kernel_matrix(vn.NOISE, kernel, q, q, theta), np.ones(D), a, 1e-3)
        assert abs(fd - fgv[0, a]) <= (2e-2 if kernel == "Matern32" else 1e-3) * fgv[0, a]
    # and a point far from every observation tends to it
    X, y, _, theta4 = _tile(3)
    fg, fgv = pg.predict_grad(kernel, X, y, np.full((1, 3), 1e3), theta4)
    np.testing.assert_allclose(fg, 0.0, atol=1e-12)
    np.testing.assert_allclose(fgv, pg.prior_grad(kernel, theta4, 1, 3)[1], rtol=1e-12)


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
    int (*fn)(gpsat_handle*, const gpsat_batch*, const gpsat_pred_grad*) =
        (int (*)(gpsat_handle*, const gpsat_batch*, const gpsat_pred_grad*))dlsym(h, "gpsat_fit_predict_batch_grad");
    if (!ver || !fn) return 2;
    printf("%d %d %d %d %d %d\n", (int)sizeof(gpsat_pred_grad), (int)offsetof(gpsat_pred_grad, f_grad),
           (int)offsetof(gpsat_pred_grad, f_grad_var), (int)offsetof(gpsat_pred_grad, reserved), GPSAT_ABI_VERSION, ver());
    return 0;
}
'''
    cfile, exe = tmp_path / "pred_grad_abi.c", tmp_path / "pred_grad_abi"
    cfile.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe), "-ldl"], check=True)
    lib = L.load()
    out = subprocess.run([str(exe), L.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["48", "0", "8", "16", "4", "4"]
    assert C.sizeof(L.GpsatPredGrad) == 48 and L.GpsatPredGrad.f_grad_var.offset == 8 and L.GpsatPredGrad.reserved.offset == 16
    assert L.ABI_VERSION == 4
    assert V.PRED_GRAD_ENTRY == "gpsat_fit_predict_batch_grad" and V.PRED_GRAD_ENTRY in L.OPTIONAL_EXPORTS
    assert hasattr(lib, "gpsat_fit_predict_batch_grad")
    header = open(os.path.join(ROOT, "include", "gpsat_hip.h")).read()
    assert "int gpsat_fit_predict_batch_grad(gpsat_handle *h, const gpsat_batch *b, const gpsat_pred_grad *pg);" in header


def _batch(D=3, kernel=2, dtype=L.F64, memory=L.MEM_HOST, P=(2, 0, 3)):
    T, H = 3, D + 2
    keep = dict(obs_off=np.array([0, 4, 4, 9], dtype=np.int64), pred_off=np.concatenate([[0], np.cumsum(P)]).astype(np.int64),
                theta0=np.ones((T, H)), nan=np.full((T, H), np.nan), tr=np.ones(H, dtype=np.uint8))
    b = L.GpsatBatch()
    b.T, b.D, b.dtype, b.kernel, b.memory, b.optimiser = T, D, dtype, kernel, memory, L.OPT_NONE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b.obs_off, b.pred_off, b.theta0, b.lo, b.hi, b.trainable = (p(keep[k]) for k in ("obs_off", "pred_off", "theta0", "nan", "nan", "tr"))
    return b, keep


def test_host_checks_of_the_pred_grad_entry_point():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat15check_pred_gradEPK11gpsat_batchPK15gpsat_pred_gradPcm")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.GpsatBatch), C.POINTER(L.GpsatPredGrad), C.c_char_p, C.c_size_t]
    out = np.zeros(64)

    def check(b, f_grad=True, f_grad_var=True, reserved=None, null=False):
        s = L.GpsatPredGrad()
        s.f_grad = out.ctypes.data if f_grad else None
        s.f_grad_var = out.ctypes.data if f_grad_var else None
        if reserved is not None:
            s.reserved[reserved] = 1
        why = C.create_string_buffer(256)
        rc = fn(C.byref(b), None if null else C.byref(s), why, 256)
        return rc, why.value.decode()

    for kern in (0, 2, 3):
        for D in (1, 2, 3, 4):
            for memory in (L.MEM_HOST, L.MEM_DEVICE):
                b, keep = _batch(D=D, kernel=kern, memory=memory)
                assert check(b) == (0, "")
    b, keep = _batch()
    rc, why = check(b, null=True)
    assert rc == -1 and "pred_grad is NULL" in why
    for i in (0, 7):
        rc, why = check(b, reserved=i)
        assert rc == -1 and "reserved" in why
    for kw, match in ((dict(f_grad=False), "f_grad is NULL"), (dict(f_grad_var=False), "f_grad_var is NULL")):
        rc, why = check(b, **kw)
        assert rc == -1 and match in why
    b0, keep0 = _batch(P=(0, 0, 0))                                    # no prediction point: nothing is written
    assert check(b0, f_grad=False, f_grad_var=False) == (0, "")
    for bad, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(kernel=1), "not mean-square differentiable"),
                       (dict(kernel=L.KERNEL_RQ), "GPSAT_KERNEL_RQ")):
        b, keep = _batch(**bad)
        rc, why = check(b)
        assert rc == -1 and match in why, (bad, rc, why)
    # no full covariance in the same call: either of the two fields
    cov_off = np.array([0, 4, 4, 13], dtype=np.int64)
    for field, val in (("cov_off", cov_off.ctypes.data), ("f_cov", out.ctypes.data)):
        b, keep = _batch()
        setattr(b, field, val)
        rc, why = check(b)
        assert rc == -1 and "full covariance" in why and "cov_off / f_cov" in why
    # the entry point itself, before any device is touched
    b, keep = _batch()
    assert lib.gpsat_fit_predict_batch_grad(None, C.byref(b), None) == -1
    assert "pred_grad is NULL" in lib.gpsat_last_error().decode()


# ---- host logic with a device-free engine
class _NoDevice:
    device_name = "no device (host logic only)"
    device_id = 0


def test_why_refused_pred_grad_names_every_reason():
    assert V.why_refused_pred_grad([], "f64", "Matern32") is None and V.why_refused_pred_grad([], None, None) is None
    assert V.why_refused_pred_grad(["replacement"], "f64", "RBF") is None
    assert "fp64 only" in V.why_refused_pred_grad([], "f32", "Matern32")
    for k in ("Matern12", "Exponential"):
        assert "not mean-square differentiable" in V.why_refused_pred_grad([], "f64", k)
    assert "RationalQuadratic" in V.why_refused_pred_grad([], "f64", "RationalQuadratic")
    for row in V.PRED_GRAD_EXCLUDES:
        why = V.why_refused_pred_grad([row], "f64", "Matern32")
        assert "cannot be combined" in why and V.VARIANTS[row].arg in why and why.count(".") <= 2, why
    assert len(V.VARIANTS) == 9                                         # an option of the plain call, not a row


def test_engine_refuses_before_any_library_call():
    eng = object.__new__(Engine)                                         # no handle, no library: a call would fail otherwise
    X, y, _, Xs = cpu_tile(vn.NOISE, 5, 10, 2)
    kw = dict(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, optimiser="none", theta0=np.ones(4), pred_grad=True)
    with pytest.raises(GpsatError, match="fp64 only"):
        eng.fit_predict_batch(**kw)                                      # the default dtype is fp32
    with pytest.raises(GpsatError, match="fp64 only"):
        eng.fit_predict_batch(dtype="f32", **kw)
    for more, match in ((dict(kernel="Matern12"), "not mean-square differentiable"), (dict(kernel="Exponential"), "mean-square"),
                        (dict(kernel="RationalQuadratic", theta0=np.ones(5)), "RationalQuadratic"),
                        (dict(mean="constant", theta0=np.ones(5)), "mean='constant'"), (dict(obs_var=np.zeros(10)), "obs_var"),
                        (dict(cv_fold="loo"), "cv_fold"), (dict(cv_fold=np.zeros(10, np.int32), cv_refit=True), "cv_refit"),
                        (dict(n_starts=2), "n_starts"), (dict(full_cov=True), "full_cov")):
        with pytest.raises(GpsatError, match=match) as ei:
            eng.fit_predict_batch(dtype="f64", **{**kw, **more})
        assert "pred_grad" in str(ei.value)
    with pytest.raises(TypeError, match="pred_grad"):                   # the sparse call has no such argument
        eng.sgpr_fit_predict_batch(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, z_off=[0, 3], Z=X[:3], theta0=np.ones(4),
                                   pred_grad=True)
    assert BatchResult.__dataclass_fields__["f_grad"].default is None and BatchResult.__dataclass_fields__["f_grad_var"].default is None


def test_model_converts_the_units_and_names_the_columns():
    X, y, _, Xs = cpu_tile(vn.NOISE, 4, 30, 2)
    cs, osc = np.array([2.0, 0.5]), 4.0
    eng = pg.GradNumpyEngine()
    m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", coords_scale=cs, obs_scale=osc, obs_mean="local",
                    kernel="Matern52", kernel_kwargs={"lengthscales": [1.5, 0.8]}, noise_variance=0.05)
    theta = np.array([1.5, 0.8, 1.0, 0.05])
    out = m.predict(Xs, gradient=True)
    assert eng.calls[-1]["pred_grad"] is True
    assert sorted(k for k in out if "grad" in k) == ["f*_grad_0", "f*_grad_1", "f*_grad_var_0", "f*_grad_var_1"]
    fg, fgv = pg.predict_grad("Matern52", X / cs, (y - y.mean()) / osc, Xs / cs, theta)
    for k in range(2):
        assert out[f"f*_grad_{k}"].shape == (len(Xs),)
        np.testing.assert_array_equal(out[f"f*_grad_{k}"], osc * fg[:, k] / cs[k])
        np.testing.assert_array_equal(out[f"f*_grad_var_{k}"], osc ** 2 * fgv[:, k] / cs[k] ** 2)
    # raw units: the central difference of the raw prediction f_bar + obs_scale f* in raw coordinates
    h = 1e-5
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        up, dn = m.predict(Xs + e), m.predict(Xs - e)
        fd = osc * (up["f*"] - dn["f*"]) / (2 * h)
        np.testing.assert_allclose(out[f"f*_grad_{k}"], fd, rtol=0, atol=1e-6)
    # apply_scale=False: the scaled model's own numbers at scaled coordinates
    out2 = m.predict(Xs / cs, apply_scale=False, gradient=True)
    np.testing.assert_array_equal(out2["f*_grad_1"], fg[:, 1])
    np.testing.assert_array_equal(out2["f*_grad_var_0"], fgv[:, 0])
    # the other entries are those of the call without the option, which does not ask the engine for it
    plain = m.predict(Xs)
    assert eng.calls[-1]["pred_grad"] is False and not [k for k in plain if "grad" in k]
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k])


def test_model_refusals():
    X, y, _, Xs = cpu_tile(vn.NOISE, 4, 12, 2)
    kw = dict(coords=X, obs=y, engine=_NoDevice())
    for more, match in ((dict(dtype="f32"), "fp64 only"), (dict(), "fp64 only"), (dict(dtype="f64", kernel="Matern12"), "mean-square"),
                        (dict(dtype="f64", kernel="RationalQuadratic"), "RationalQuadratic"),
                        (dict(dtype="f64", mean_function="Constant"), "mean='constant'"),
                        (dict(dtype="f64", obs_var=np.full(12, 0.1)), "obs_var")):
        with pytest.raises(NotImplementedError, match=match):
            HipGPRModel(**kw, **more).predict(Xs, gradient=True)
    with pytest.raises(NotImplementedError, match="full_cov"):
        HipGPRModel(dtype="f64", **kw).predict(Xs, full_cov=True, gradient=True)
    with pytest.raises(NotImplementedError, match="SGPR"):
        HipSGPRModel(**kw).predict(Xs, gradient=True)
    with pytest.raises(NotImplementedError, match="n_starts"):
        HipSklearnGPRModel(**kw).predict(Xs, gradient=True)


def _oi_case(n_locs=5, seed=3):
    rng = np.random.default_rng(seed)
    n = 260
    df = pd.DataFrame({"x": rng.uniform(0.0, 10.0, n), "t": rng.uniform(0.0, 4.0, n)})
    df["y"] = 0.4 * np.sin(1.3 * df["x"]) * np.cos(0.7 * df["t"]) + 0.03 * rng.standard_normal(n)
    locs = pd.DataFrame({"x": np.linspace(2.0, 8.0, n_locs), "t": np.full(n_locs, 2.0)})
    radius = 2.0
    pred = pd.DataFrame({"x": np.linspace(0.5, 9.5, 30), "t": np.linspace(1.0, 3.0, 30)})
    cfg = dict(expert_loc_config={"source": locs},
               data_config={"data_source": df, "obs_col": ["y"], "coords_col": ["x", "t"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": {"coords_scale": [2.0, 0.5], "obs_scale": 0.5,
                                                                         "kernel": "Matern52"},
                             "constraints": {"lengthscales": {"low": [1e-3, 1e-3], "high": [10.0, 10.0]}},
                             "optim_kwargs": {"max_iter": 200}, "pred_kwargs": {"gradient": True}},
               pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.2})
    return cfg, locs, df, radius, pred


def test_orchestrator_names_the_columns_by_coordinate_and_fills_the_right_rows(tmp_path):
    cfg, locs, df, radius, pred = _oi_case()
    eng = pg.GradNumpyEngine()
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    assert oi.dtype == "f64" and oi.pred_grad is True                   # dtype None means fp64 here
    tabs = oi.run(store_path=str(tmp_path / "store"), store_every=3)     # two waves: 3 + 2 experts
    assert [c["T"] for c in eng.calls] == [3, 2] and all(c["pred_grad"] for c in eng.calls)
    preds = tabs["preds"]
    new = ["f*_grad_x", "f*_grad_var_x", "f*_grad_t", "f*_grad_var_t"]
    assert set(new) <= set(preds.columns) and {"f*", "f*_var", "y_var", "f_bar", "pred_loc_x", "pred_loc_t"} <= set(preds.columns)
    assert len(preds) > 20 and np.isfinite(preds[new].values).all() and (preds[["f*_grad_var_x", "f*_grad_var_t"]].values > 0).all()
    # every expert: the per-tile model on the rows the selection gives it, predicting at its own locations; neighbours share
    # rows (radius 2.0, spacing 1.5), and every expert's values land in its own rows of preds
    shared, at = 0, 0
    mc = cfg["model_config"]
    for k, loc in locs.iterrows():
        d = df[(df["x"] <= loc["x"] + radius) & (df["x"] >= loc["x"] - radius)]
        if k + 1 < len(locs):
            shared += int((d["x"] >= locs["x"][k + 1] - radius).sum())
        m = HipGPRModel(data=d, obs_col="y", coords_col=["x", "t"], engine=pg.GradNumpyEngine(), dtype="f64", **mc["init_params"])
        # (with a coords_scale the orchestrator scales the box of the length scales, as the reference's run does)
        m.set_parameter_constraints({"lengthscales": {**mc["constraints"]["lengthscales"], "scale": True}}, move_within_tol=True, tol=1e-2)
        m.optimise_parameters(**mc["optim_kwargs"])
        rows = preds.iloc[at:at + int((np.hypot(pred["x"] - loc["x"], pred["t"] - loc["t"]) <= 1.2).sum())]
        at += len(rows)
        assert len(rows) > 0 and (rows.index.get_level_values("x") == loc["x"]).all()
        out = m.predict(rows[["pred_loc_x", "pred_loc_t"]].values, gradient=True)
        np.testing.assert_array_equal(rows["f*"].values, out["f*"])
        osc = mc["init_params"]["obs_scale"]
        for ci, c in enumerate(["x", "t"]):
            # in the units f* is stored in (divided by obs_scale), per raw coordinate unit
            np.testing.assert_allclose(rows[f"f*_grad_{c}"].values, out[f"f*_grad_{ci}"] / osc, rtol=1e-13, atol=0)
            np.testing.assert_allclose(rows[f"f*_grad_var_{c}"].values, out[f"f*_grad_var_{ci}"] / osc ** 2, rtol=1e-13, atol=0)
    assert at == len(preds) and shared > 100
    # the store holds the same columns
    from gpsat_amd.local_experts import get_results
    np.testing.assert_array_equal(get_results(str(tmp_path / "store"))["preds"][new].values, preds[new].values)
    # one expert per engine call: the same table
    tabs1 = BatchedLocalExpertOI(engine=pg.GradNumpyEngine(), **cfg).run(store_path=None, engine_chunk=1)
    pd.testing.assert_frame_equal(tabs1["preds"], preds)


def test_orchestrator_without_the_option_is_unchanged():
    cfg, *_ = _oi_case()
    mc = cfg["model_config"]
    eng, eng0 = pg.GradNumpyEngine(), pg.GradNumpyEngine()
    tabs = BatchedLocalExpertOI(engine=eng, dtype="f64", **cfg).run(store_path=None)
    for pk in ({}, {"gradient": False}, None):
        oi0 = BatchedLocalExpertOI(engine=eng0, dtype="f64", **{**cfg, "model_config": {**mc, "pred_kwargs": pk}})
        assert oi0.pred_grad is False
        tabs0 = oi0.run(store_path=None)
        assert not any(c["pred_grad"] for c in eng0.calls)
        assert set(tabs0) == set(tabs) and not [c for c in tabs0["preds"].columns if "grad" in c]
        assert list(tabs0["preds"].columns) == ["_dim_0", "f*", "f*_var", "y_var", "f_bar", "pred_loc_x", "pred_loc_t"]
        for name in tabs0:
            if name != "run_details":
                cols = list(tabs0[name].columns)
                pd.testing.assert_frame_equal(tabs0[name], tabs[name][cols])
    # without the option dtype None stays fp32
    assert BatchedLocalExpertOI(engine=eng0, **{**cfg, "model_config": {**mc, "pred_kwargs": {}}}).dtype == "f32"


def test_orchestrator_refusals():
    cfg, *_ = _oi_case()
    mc, dc = cfg["model_config"], cfg["data_config"]
    E = pg.GradNumpyEngine
    ip = mc["init_params"]
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(engine=E(), dtype="f32", **cfg)
    for kernel, match in (("Matern12", "mean-square"), ("RationalQuadratic", "RationalQuadratic")):
        with pytest.raises(NotImplementedError, match=match):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {**ip, "kernel": kernel}}})
        # ... and as the kernel of a replacement profile
        with pytest.raises(NotImplementedError, match=match):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10,
                                                                         "replacement_init_params": {"kernel": kernel}}})
    with pytest.raises(NotImplementedError, match="mean='constant'"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {**ip, "mean_function": "Constant"}}})
    df = dc["data_source"].assign(var=0.01)
    with pytest.raises(NotImplementedError, match="obs_var"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "data_config": {**dc, "data_source": df, "obs_var_col": "var"}})
    for cv in ("loo", {"by": ["x"]}, {"by": ["x"], "refit": True}):
        with pytest.raises(NotImplementedError, match="cv"):
            BatchedLocalExpertOI(engine=E(), cv=cv, **cfg)
    with pytest.raises(NotImplementedError, match="SGPR"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "oi_model": "GPflowSGPRModel"}})
    with pytest.raises(NotImplementedError, match="full_cov"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "pred_kwargs": {"gradient": True, "full_cov": True}}})
    # a replacement profile with a kernel that has a gradient is accepted, and predicts the same columns
    oi = BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10,
                                                                      "replacement_init_params": {**ip, "kernel": "RBF"}}})
    assert oi.pred_grad and oi.dtype == "f64"
