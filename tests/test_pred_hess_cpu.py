"""CPU: the second derivatives of the posterior mean at the prediction points, their variances and the weighted Laplacian
(pred_hess) without a GPU -- the restatement of tests/pred_hess_numpy.py against torch autograd, against central differences of
pred_grad_numpy.predict_grad and against second-difference stencils applied on both sides of the posterior covariance; the
ABI's struct through a compiled C program, the host checks of gpsat_fit_predict_batch_hess (gpsat::check_pred_hess), and the
host logic of Engine, the models and BatchedLocalExpertOI with a device-free engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import pred_grad_numpy as pg
import pred_hess_numpy as ph
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


def _weights(D):
    return np.array([1.0, 0.3, 2.5, 0.7])[:D]


# ---- the restatement
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_mean_hessian_and_laplacian_match_torch_autograd(kernel, D):
    """torch.autograd.functional.hessian of a torch fp64 restatement of the posterior mean k(x*, X) K_y^-1 y: to 1e-10.  Matern52:
    without the point that sits on an observation, where autograd's sqrt has no derivative (the differences below cover it)."""
    import torch
    X, y, Xs, theta = _tile(D)
    alpha = torch.tensor(np.linalg.solve(vn.K_y(vn.NOISE, kernel, X, theta, np.zeros(len(X))), y))
    ell, sf2, Xt = torch.tensor(theta[:D]), float(theta[D]), torch.tensor(X)

    def mean(xs):
        d = (Xt - xs[None, :]) / ell
        r2 = (d * d).sum(-1)
        if kernel == "RBF":
            k = torch.exp(-0.5 * r2)
        else:
            s = 5.0 ** 0.5 * torch.sqrt(r2)
            k = (1.0 + s + s * s / 3.0) * torch.exp(-s)
        return (sf2 * k * alpha).sum()

    w = _weights(D)
    fh, _, fl, _ = ph.predict_hess(kernel, X, y, Xs, theta, lap_weight=w)
    pairs = ph.pairs(range(D))
    worst = 0.0
    for p in range(1 if kernel == "Matern52" else 0, len(Xs)):
        Ht = torch.autograd.functional.hessian(mean, torch.tensor(Xs[p])).numpy()
        assert np.isfinite(Ht).all()
        ref = np.array([Ht[a, b] for a, b in pairs])
        worst = max(worst, np.abs(fh[p] - ref).max(), abs(fl[p] - float(np.sum(w * np.diag(Ht)))))
    print(kernel, D, "largest error", worst)
    assert np.abs(fh).max() > 1e-2
    assert worst <= 1e-10


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_mean_hessian_and_laplacian_match_central_differences_of_the_gradient(kernel, D):
    """Central differences of pred_grad_numpy.predict_grad, h = 1e-5: to 1e-7, the point on an observation included."""
    X, y, Xs, theta = _tile(D)
    w = _weights(D)
    fh, _, fl, _ = ph.predict_hess(kernel, X, y, Xs, theta, lap_weight=w)
    h, fd = 1e-5, np.empty((len(Xs), D, D))
    for b in range(D):
        e = np.zeros(D)
        e[b] = h
        fd[:, :, b] = (pg.predict_grad(kernel, X, y, Xs + e, theta)[0] - pg.predict_grad(kernel, X, y, Xs - e, theta)[0]) / (2 * h)
    ref = np.stack([fd[:, a, b] for a, b in ph.pairs(range(D))], axis=1)
    lap = sum(w[a] * fd[:, a, a] for a in range(D))
    print(kernel, D, "largest error", np.abs(fh - ref).max(), np.abs(fl - lap).max())
    np.testing.assert_allclose(fh, ref, rtol=0, atol=1e-7)
    np.testing.assert_allclose(fl, lap, rtol=0, atol=1e-7)


def _stencil(x, h, terms):
    """Points and weights of sum_t c_t d2/dx_a dx_b at x by central second differences with steps h[a]: ``terms`` = [(c, a, b)].
    a == b: x + h e_a, x, x - h e_a with (1, -2, 1) / h_a^2; a != b: x +- h e_a +- h e_b with (+, -, -, +) / (4 h_a h_b)."""
    pts, wts = [], []
    for c, a, b in terms:
        ea, eb = np.zeros(len(x)), np.zeros(len(x))
        ea[a], eb[b] = h[a], h[b]
        if a == b:
            pts += [x + ea, x, x - ea]
            wts += [c / h[a] ** 2, -2.0 * c / h[a] ** 2, c / h[a] ** 2]
        else:
            pts += [x + ea + eb, x + ea - eb, x - ea + eb, x - ea - eb]
            wts += [c / (4 * h[a] * h[b]), -c / (4 * h[a] * h[b]), -c / (4 * h[a] * h[b]), c / (4 * h[a] * h[b])]
    return np.stack(pts), np.array(wts)


def _stencil_var(cov_of, x, h, terms):
    pts, wts = _stencil(x, h, terms)
    return float(wts @ cov_of(pts) @ wts)


# h in units of the length scale and the relative bound: RBF's truncation is O(h^2) (rounding about 1e-16 / h^4 = 1e-8);
# Matern52's |r|^5 term makes it O(h), about 6 h (rounding about 1e-4)
_FD = {"RBF": (1e-2, 1e-3), "Matern52": (1e-3, 2e-2)}


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_variances_match_the_stencil_on_both_sides_of_the_posterior_covariance(kernel, D):
    X, y, Xs, theta = _tile(D)
    w = _weights(D)
    _, fhv, _, flv = ph.predict_hess(kernel, X, y, Xs, theta, lap_weight=w)
    hrel, bound = _FD[kernel]
    h = hrel * theta[:D]
    cov_of = lambda q: pg.plain_predict_cov(kernel, X, y, q, theta)
    worst, worst_lap = 0.0, 0.0
    for p in range(len(Xs)):
        for k, (a, b) in enumerate(ph.pairs(range(D))):
            fd = _stencil_var(cov_of, Xs[p], h, [(1.0, a, b)])
            worst = max(worst, abs(fhv[p, k] - fd) / abs(fd))
        fd = _stencil_var(cov_of, Xs[p], h, [(w[a], a, a) for a in range(D)])
        worst_lap = max(worst_lap, abs(flv[p] - fd) / abs(fd))
    print(kernel, D, "largest relative error: pairs", worst, "Laplacian", worst_lap)
    assert (fhv > 0).all() and (flv > 0).all()
    assert worst <= bound and worst_lap <= bound


@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_prior_constants_match_the_stencil_on_the_prior_covariance(kernel):
    """hh(0), the factor 3 on the diagonal and the Laplacian's cross term; and an empty tile returns exactly these."""
    D, theta = 3, np.array([1.3, 0.7, 2.0, 0.9, 0.05])
    w = np.array([1.0, 0.4, 2.0])
    fh, fhv, fl, flv = ph.predict_hess(kernel, np.zeros((0, D)), np.zeros(0), np.ones((4, D)), theta, lap_weight=w)
    assert fh.shape == fhv.shape == (4, 6) and (fh == 0.0).all() and (fl == 0.0).all()
    hrel, bound = _FD[kernel]
    cov_of = lambda q: vn.kernel_matrix(vn.NOISE, kernel, q, q, theta)
    for k, (a, b) in enumerate(ph.pairs(range(D))):
        expect = 0.9 * ph.HH0[kernel] * (3.0 if a == b else 1.0) / (theta[a] ** 2 * theta[b] ** 2)
        np.testing.assert_array_equal(fhv[:, k], expect)
        fd = _stencil_var(cov_of, np.ones(D), hrel * theta[:D], [(1.0, a, b)])
        assert abs(fd - expect) <= bound * expect, (a, b, fd, expect)
    wl = w / theta[:D] ** 2
    expect = 0.9 * ph.HH0[kernel] * (2.0 * np.sum(wl ** 2) + np.sum(wl) ** 2)
    np.testing.assert_allclose(flv, expect, rtol=1e-15)
    fd = _stencil_var(cov_of, np.ones(D), hrel * theta[:D], [(w[a], a, a) for a in range(D)])
    assert abs(fd - expect) <= bound * expect, (fd, expect)
    # and a point far from every observation tends to the prior
    X, y, _, theta4 = _tile(3)
    fh, fhv, fl, flv = ph.predict_hess(kernel, X, y, np.full((1, 3), 1e3), theta4, lap_weight=w)
    np.testing.assert_allclose(fh, 0.0, atol=1e-12)
    np.testing.assert_allclose(fhv[0], [ph.prior_pair(kernel, theta4, 3, a, b) for a, b in ph.pairs(range(3))], rtol=1e-12)
    np.testing.assert_allclose(flv, ph.prior_lap(kernel, theta4, 3, w), rtol=1e-12)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_laplacian_variance_is_w_sigma_w_of_the_joint_covariance(kernel, D):
    X, y, Xs, theta = _tile(D)
    w = _weights(D)
    fh, fhv, fl, flv, cov = ph.predict_hess(kernel, X, y, Xs, theta, lap_weight=w, joint=True)
    diag = [k for k, (a, b) in enumerate(ph.pairs(range(D))) if a == b]
    np.testing.assert_allclose(np.einsum("pii->pi", cov), fhv[:, diag], rtol=1e-12)
    np.testing.assert_allclose(flv, np.einsum("a,pab,b->p", w, cov, w), rtol=1e-12, atol=0)
    np.testing.assert_allclose(fl, fh[:, diag] @ w, rtol=0, atol=1e-12 * np.abs(fh).max())
    # a subset of the coordinates, with weights on the subset only
    if D >= 3:
        dims, w2 = [0, 2], np.array([0.5, 0.0, 1.5, 0.0][:D])
        fh2, fhv2, fl2, flv2, cov2 = ph.predict_hess(kernel, X, y, Xs, theta, dims=dims, lap_weight=w2, joint=True)
        full = ph.pairs(range(D))
        np.testing.assert_array_equal(fh2, fh[:, [full.index(p) for p in ph.pairs(dims)]])
        np.testing.assert_allclose(flv2, np.einsum("a,pab,b->p", w2[dims], cov2, w2[dims]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("kernel", ph.KERNELS)
def test_in_one_dimension_with_weight_one_the_laplacian_is_the_hessian(kernel):
    X, y, Xs, theta = _tile(1)
    fh, fhv, fl, flv = ph.predict_hess(kernel, X, y, Xs, theta, lap_weight=[1.0])
    np.testing.assert_allclose(fl, fh[:, 0], rtol=1e-14, atol=0)
    np.testing.assert_allclose(flv, fhv[:, 0], rtol=1e-14, atol=0)


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
    int (*fn)(gpsat_handle*, const gpsat_batch*, const gpsat_pred_hess*) =
        (int (*)(gpsat_handle*, const gpsat_batch*, const gpsat_pred_hess*))dlsym(h, "gpsat_fit_predict_batch_hess");
    if (!ver || !fn) return 2;
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(gpsat_pred_hess), (int)offsetof(gpsat_pred_hess, f_hess),
           (int)offsetof(gpsat_pred_hess, f_hess_var), (int)offsetof(gpsat_pred_hess, f_lap), (int)offsetof(gpsat_pred_hess, f_lap_var),
           (int)offsetof(gpsat_pred_hess, f_grad), (int)offsetof(gpsat_pred_hess, f_grad_var), (int)offsetof(gpsat_pred_hess, lap_weight),
           (int)offsetof(gpsat_pred_hess, dims), (int)offsetof(gpsat_pred_hess, reserved), GPSAT_ABI_VERSION, ver());
    return 0;
}
'''
    cfile, exe = tmp_path / "pred_hess_abi.c", tmp_path / "pred_hess_abi"
    cfile.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe), "-ldl"], check=True)
    lib = L.load()
    out = subprocess.run([str(exe), L.LIB_PATH], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["112", "0", "8", "16", "24", "32", "40", "48", "80", "84", "4", "4"]
    S = L.GpsatPredHess
    assert C.sizeof(S) == 112
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 80, 84]
    assert L.ABI_VERSION == 4
    assert V.PRED_HESS_ENTRY == "gpsat_fit_predict_batch_hess" and V.PRED_HESS_ENTRY in L.OPTIONAL_EXPORTS
    assert hasattr(lib, "gpsat_fit_predict_batch_hess")
    header = open(os.path.join(ROOT, "include", "gpsat_hip.h")).read()
    assert "int gpsat_fit_predict_batch_hess(gpsat_handle *h, const gpsat_batch *b, const gpsat_pred_hess *ph);" in header


def _batch(D=3, kernel=3, dtype=L.F64, memory=L.MEM_HOST, P=(2, 0, 3)):
    T, H = 3, D + 2
    keep = dict(obs_off=np.array([0, 4, 4, 9], dtype=np.int64), pred_off=np.concatenate([[0], np.cumsum(P)]).astype(np.int64),
                theta0=np.ones((T, H)), nan=np.full((T, H), np.nan), tr=np.ones(H, dtype=np.uint8))
    b = L.GpsatBatch()
    b.T, b.D, b.dtype, b.kernel, b.memory, b.optimiser = T, D, dtype, kernel, memory, L.OPT_NONE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b.obs_off, b.pred_off, b.theta0, b.lo, b.hi, b.trainable = (p(keep[k]) for k in ("obs_off", "pred_off", "theta0", "nan", "nan", "tr"))
    return b, keep


def test_host_checks_of_the_pred_hess_entry_point():
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat15check_pred_hessEPK11gpsat_batchPK15gpsat_pred_hessPcm")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(L.GpsatBatch), C.POINTER(L.GpsatPredHess), C.c_char_p, C.c_size_t]
    out = np.zeros(64)
    OUT = ("f_hess", "f_hess_var", "f_lap", "f_lap_var", "f_grad", "f_grad_var")

    def check(b, dims=0b111, weights=(1.0, 1.0, 1.0, 0.0), missing=(), reserved=None, null=False):
        s = L.GpsatPredHess()
        for f in OUT:
            setattr(s, f, None if f in missing else out.ctypes.data)
        s.dims = dims
        for a, c in enumerate(weights):
            s.lap_weight[a] = c
        if reserved is not None:
            s.reserved[reserved] = 1
        why = C.create_string_buffer(256)
        rc = fn(C.byref(b), None if null else C.byref(s), why, 256)
        return rc, why.value.decode()

    for kern in (0, 3):
        for D in (1, 2, 3, 4):
            for memory in (L.MEM_HOST, L.MEM_DEVICE):
                b, keep = _batch(D=D, kernel=kern, memory=memory)
                for dims in range(1, 1 << D):
                    wts = [1.0 if (dims >> a) & 1 else 0.0 for a in range(4)]
                    assert check(b, dims=dims, weights=wts) == (0, "")
                # without a Laplacian, without the gradient: the pointers may be NULL
                assert check(b, dims=1, weights=(0.0,) * 4, missing=("f_lap", "f_lap_var", "f_grad", "f_grad_var")) == (0, "")
    b, keep = _batch()
    rc, why = check(b, null=True)
    assert rc == -1 and "pred_hess is NULL" in why
    for i in (0, 6):
        rc, why = check(b, reserved=i)
        assert rc == -1 and "reserved" in why
    for kw, match in ((dict(dims=0, weights=(0.0,) * 4), "dims is empty"), (dict(dims=0b1000, weights=(0.0,) * 4), ">= D"),
                      (dict(dims=0b10001, weights=(0.0,) * 4), ">= D"),
                      (dict(missing=("f_hess",)), "f_hess is NULL"), (dict(missing=("f_hess_var",)), "f_hess_var is NULL"),
                      (dict(missing=("f_lap",)), "f_lap is NULL"), (dict(missing=("f_lap_var",)), "f_lap_var is NULL"),
                      (dict(missing=("f_lap", "f_lap_var")), "f_lap is NULL"),                  # weights given, no output
                      (dict(missing=("f_grad",)), "together"), (dict(missing=("f_grad_var",)), "together"),
                      (dict(weights=(1.0, -0.5, 1.0, 0.0)), "negative or not finite"),
                      (dict(weights=(1.0, float("nan"), 1.0, 0.0)), "negative or not finite"),
                      (dict(weights=(1.0, float("inf"), 1.0, 0.0)), "negative or not finite"),
                      (dict(dims=0b101), "outside dims"), (dict(weights=(1.0, 1.0, 1.0, 1.0)), "outside dims")):
        rc, why = check(b, **kw)
        assert rc == -1 and match in why, (kw, rc, why)
    b0, keep0 = _batch(P=(0, 0, 0))                                    # no prediction point: nothing is written
    assert check(b0, missing=OUT) == (0, "")
    for bad, match in ((dict(dtype=L.F32), "GPSAT_F64 only"), (dict(kernel=1), "not mean-square differentiable"),
                       (dict(kernel=2), "not mean-square differentiable"), (dict(kernel=L.KERNEL_RQ), "not built for kernel 4")):
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
    assert lib.gpsat_fit_predict_batch_hess(None, C.byref(b), None) == -1
    assert "pred_hess is NULL" in lib.gpsat_last_error().decode()


# ---- host logic with a device-free engine
class _NoDevice:
    device_name = "no device (host logic only)"
    device_id = 0


def test_why_refused_pred_hess_names_every_reason():
    assert V.why_refused_pred_hess([], "f64", "Matern52") is None and V.why_refused_pred_hess([], None, None) is None
    assert V.why_refused_pred_hess(["replacement"], "f64", "RBF") is None
    assert "fp64 only" in V.why_refused_pred_hess([], "f32", "Matern52")
    for k in ("Matern12", "Exponential", "Matern32"):
        assert "not mean-square differentiable" in V.why_refused_pred_hess([], "f64", k)
    assert "not built for kernel 'RationalQuadratic'" in V.why_refused_pred_hess([], "f64", "RationalQuadratic")
    for row in V.PRED_HESS_EXCLUDES:
        why = V.why_refused_pred_hess([row], "f64", "Matern52")
        assert "cannot be combined" in why and V.VARIANTS[row].arg in why and why.count(".") <= 2, why
    assert len(V.VARIANTS) == 9                                         # an option of the plain call, not a row
    assert V.pred_hess_pairs([2, 0]) == [(0, 0), (0, 2), (2, 2)] and V.pred_hess_pairs([1]) == [(1, 1)]
    assert len(V.pred_hess_pairs(range(4))) == 10


def test_engine_refuses_before_any_library_call():
    eng = object.__new__(Engine)                                         # no handle, no library: a call would fail otherwise
    X, y, _, Xs = cpu_tile(vn.NOISE, 5, 10, 2)
    kw = dict(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, optimiser="none", theta0=np.ones(4), pred_hess=True,
              kernel="Matern52")
    with pytest.raises(GpsatError, match="fp64 only"):
        eng.fit_predict_batch(**kw)                                      # the default dtype is fp32
    with pytest.raises(GpsatError, match="fp64 only"):
        eng.fit_predict_batch(dtype="f32", **kw)
    for more, match in ((dict(kernel="Matern12"), "not mean-square differentiable"), (dict(kernel="Exponential"), "mean-square"),
                        (dict(kernel="Matern32"), "Matern-3/2"),
                        (dict(kernel="RationalQuadratic", theta0=np.ones(5)), "RationalQuadratic"),
                        (dict(mean="constant", theta0=np.ones(5)), "mean='constant'"), (dict(obs_var=np.zeros(10)), "obs_var"),
                        (dict(cv_fold="loo"), "cv_fold"), (dict(cv_fold=np.zeros(10, np.int32), cv_refit=True), "cv_refit"),
                        (dict(n_starts=2), "n_starts"), (dict(full_cov=True), "full_cov")):
        for grad in (False, True):                                       # beside pred_grad too: the wording is pred_hess's
            with pytest.raises(GpsatError, match=match) as ei:
                eng.fit_predict_batch(dtype="f64", pred_grad=grad, **{**kw, **more})
            assert "pred_hess" in str(ei.value)
    for spec, match in (({"dims": []}, "at least one coordinate"), ({"dims": [2]}, "at least one coordinate"),
                        ({"dims": [-1]}, "at least one coordinate"), ({"dims": [0], "lap_weight": [1.0]}, "one weight per coordinate"),
                        ({"lap_weight": [1.0, -1.0]}, "finite and >= 0"), ({"lap_weight": [1.0, np.nan]}, "finite and >= 0"),
                        ({"dims": [0], "lap_weight": [1.0, 1.0]}, "outside dims"), ({"what": 1}, "a dict with"), ("all", "a dict with")):
        with pytest.raises(GpsatError, match=match):
            eng.fit_predict_batch(dtype="f64", **{**kw, "pred_hess": spec})
    with pytest.raises(TypeError, match="pred_hess"):                   # the sparse call has no such argument
        eng.sgpr_fit_predict_batch(D=2, obs_off=[0, 10], X=X, y=y, pred_off=[0, 7], Xs=Xs, z_off=[0, 3], Z=X[:3], theta0=np.ones(4),
                                   pred_hess=True)
    for f in ("f_hess", "f_hess_var", "f_lap", "f_lap_var"):
        assert BatchResult.__dataclass_fields__[f].default is None
    import inspect
    assert inspect.signature(Engine.fit_predict_batch).parameters["pred_hess"].default is False


def test_model_converts_the_units_names_the_columns_and_passes_the_weights():
    X, y, _, Xs = cpu_tile(vn.NOISE, 4, 30, 3)
    cs, osc = np.array([2.0, 0.5, 1.25]), 4.0
    eng = ph.HessNumpyEngine()
    m = HipGPRModel(coords=X, obs=y, engine=eng, dtype="f64", coords_scale=cs, obs_scale=osc, obs_mean="local",
                    kernel="Matern52", kernel_kwargs={"lengthscales": [1.5, 0.8, 1.1]}, noise_variance=0.05)
    theta = np.array([1.5, 0.8, 1.1, 1.0, 0.05])
    out = m.predict(Xs, hessian=True)
    call = eng.calls[-1]
    assert call["pred_grad"] is False and call["pred_hess"]["dims"] == [0, 1, 2]
    np.testing.assert_array_equal(call["pred_hess"]["lap_weight"], 1.0 / cs ** 2)
    pairs = ph.pairs(range(3))
    names = [f"f*_hess_{a}_{b}" for a, b in pairs] + [f"f*_hess_var_{a}_{b}" for a, b in pairs] + ["f*_lap", "f*_lap_var"]
    assert sorted(k for k in out if "hess" in k or "lap" in k) == sorted(names) and not [k for k in out if "grad" in k]
    fh, fhv, fl, flv = ph.predict_hess("Matern52", X / cs, (y - y.mean()) / osc, Xs / cs, theta, lap_weight=1.0 / cs ** 2)
    for k, (a, b) in enumerate(pairs):
        assert out[f"f*_hess_{a}_{b}"].shape == (len(Xs),)
        np.testing.assert_array_equal(out[f"f*_hess_{a}_{b}"], osc * fh[:, k] / (cs[a] * cs[b]))
        np.testing.assert_array_equal(out[f"f*_hess_var_{a}_{b}"], osc ** 2 * fhv[:, k] / (cs[a] * cs[b]) ** 2)
    np.testing.assert_array_equal(out["f*_lap"], osc * fl)
    np.testing.assert_array_equal(out["f*_lap_var"], osc ** 2 * flv)
    # raw units: f*_lap is the Laplacian of the raw field in raw coordinates ...
    np.testing.assert_allclose(out["f*_lap"], sum(out[f"f*_hess_{a}_{a}"] for a in range(3)), rtol=1e-12, atol=1e-12)
    # ... and the second derivatives are central differences of the raw gradient in raw coordinates
    h = 1e-5
    for a, b in pairs:
        e = np.zeros(3)
        e[b] = h
        fd = (m.predict(Xs + e, gradient=True)[f"f*_grad_{a}"] - m.predict(Xs - e, gradient=True)[f"f*_grad_{a}"]) / (2 * h)
        np.testing.assert_allclose(out[f"f*_hess_{a}_{b}"], fd, rtol=0, atol=1e-6)
    # a subset, given out of order; and gradient beside it in one engine call
    n_calls = len(eng.calls)
    both = m.predict(Xs, hessian=[2, 0], gradient=True)
    assert len(eng.calls) == n_calls + 1
    call = eng.calls[-1]
    assert call["pred_grad"] is True and call["pred_hess"]["dims"] == [0, 2]
    np.testing.assert_array_equal(call["pred_hess"]["lap_weight"], [1.0 / cs[0] ** 2, 0.0, 1.0 / cs[2] ** 2])
    assert [k for k in both if "hess" in k and "var" not in k] == ["f*_hess_0_0", "f*_hess_0_2", "f*_hess_2_2"]
    for k in ("f*_hess_0_0", "f*_hess_0_2", "f*_hess_2_2", "f*_hess_var_0_2"):
        np.testing.assert_array_equal(both[k], out[k])
    np.testing.assert_allclose(both["f*_lap"], out["f*_hess_0_0"] + out["f*_hess_2_2"], rtol=1e-12, atol=1e-12)
    only_grad = m.predict(Xs, gradient=True)
    for k in range(3):
        np.testing.assert_array_equal(both[f"f*_grad_{k}"], only_grad[f"f*_grad_{k}"])
        np.testing.assert_array_equal(both[f"f*_grad_var_{k}"], only_grad[f"f*_grad_var_{k}"])
    # apply_scale=False: the scaled model's own numbers at scaled coordinates, unit weights
    out2 = m.predict(Xs / cs, apply_scale=False, hessian=True)
    np.testing.assert_array_equal(eng.calls[-1]["pred_hess"]["lap_weight"], np.ones(3))
    np.testing.assert_array_equal(out2["f*_hess_0_1"], fh[:, 1])
    np.testing.assert_array_equal(out2["f*_hess_var_2_2"], fhv[:, 5])
    # the other entries are those of the call without the option, which does not ask the engine for it
    plain = m.predict(Xs)
    assert eng.calls[-1]["pred_hess"] is None and not [k for k in plain if "hess" in k or "lap" in k]
    for k in plain:
        np.testing.assert_array_equal(plain[k], out[k])
    with pytest.raises(ValueError, match="coordinate indices"):
        m.predict(Xs, hessian=[3])


def test_model_refusals():
    X, y, _, Xs = cpu_tile(vn.NOISE, 4, 12, 2)
    kw = dict(coords=X, obs=y, engine=_NoDevice())
    for more, match in ((dict(dtype="f32", kernel="RBF"), "fp64 only"), (dict(kernel="RBF"), "fp64 only"),
                        (dict(dtype="f64", kernel="Matern12"), "mean-square"), (dict(dtype="f64"), "Matern-3/2"),
                        (dict(dtype="f64", kernel="RationalQuadratic"), "RationalQuadratic"),
                        (dict(dtype="f64", kernel="RBF", mean_function="Constant"), "mean='constant'"),
                        (dict(dtype="f64", kernel="RBF", obs_var=np.full(12, 0.1)), "obs_var")):
        for hs in (True, [0]):
            with pytest.raises(NotImplementedError, match=match) as ei:
                HipGPRModel(**kw, **more).predict(Xs, hessian=hs)
            assert "pred_hess" in str(ei.value)
    with pytest.raises(NotImplementedError, match="full_cov"):
        HipGPRModel(dtype="f64", kernel="RBF", **kw).predict(Xs, full_cov=True, hessian=True)
    with pytest.raises(NotImplementedError, match="Matern-3/2"):      # beside gradient, which Matern32 has: still refused
        HipGPRModel(dtype="f64", **kw).predict(Xs, gradient=True, hessian=True)
    with pytest.raises(NotImplementedError, match="SGPR"):
        HipSGPRModel(**kw).predict(Xs, hessian=True)
    with pytest.raises(NotImplementedError, match="n_starts"):
        HipSklearnGPRModel(**kw).predict(Xs, hessian=True)


def _oi_case(n_locs=4, seed=3, pred_kwargs=None):
    rng = np.random.default_rng(seed)
    n = 200
    df = pd.DataFrame({"x": rng.uniform(0.0, 8.0, n), "y": rng.uniform(0.0, 3.0, n), "t": rng.uniform(0.0, 4.0, n)})
    df["z"] = 0.4 * np.sin(1.3 * df["x"]) * np.cos(0.7 * df["t"]) * np.cos(0.9 * df["y"]) + 0.03 * rng.standard_normal(n)
    locs = pd.DataFrame({"x": np.linspace(2.0, 6.5, n_locs), "y": np.full(n_locs, 1.5), "t": np.full(n_locs, 2.0)})
    radius = 2.0
    pred = pd.DataFrame({"x": np.linspace(0.5, 7.5, 30), "y": np.linspace(1.0, 2.0, 30), "t": np.linspace(1.0, 3.0, 30)})
    cfg = dict(expert_loc_config={"source": locs},
               data_config={"data_source": df, "obs_col": ["z"], "coords_col": ["x", "y", "t"],
                            "local_select": [{"col": "x", "comp": "<=", "val": radius}, {"col": "x", "comp": ">=", "val": -radius}]},
               model_config={"oi_model": "HipGPRModel", "init_params": {"coords_scale": [2.0, 0.5, 4.0], "obs_scale": 0.5,
                                                                         "kernel": "Matern52"},
                             "constraints": {"lengthscales": {"low": [1e-3] * 3, "high": [10.0] * 3}},
                             "optim_kwargs": {"max_iter": 200},
                             "pred_kwargs": {"hessian": ["y", "x"]} if pred_kwargs is None else pred_kwargs},
               pred_loc_config={"method": "from_dataframe", "df": pred, "max_dist": 1.3})
    return cfg, locs, df, radius, pred


@pytest.mark.parametrize("gradient", [False, True])
def test_orchestrator_names_the_columns_by_coordinate_and_fills_the_right_rows(tmp_path, gradient):
    pk = {"hessian": ["y", "x"], **({"gradient": True} if gradient else {})}
    cfg, locs, df, radius, pred = _oi_case(pred_kwargs=pk)
    eng = ph.HessNumpyEngine()
    oi = BatchedLocalExpertOI(engine=eng, **cfg)
    assert oi.dtype == "f64" and oi.pred_hess == [0, 1] and oi.pred_grad is gradient       # dtype None means fp64 here
    tabs = oi.run(store_path=str(tmp_path / "store"), store_every=3, optimise=False)       # two waves: 3 + 1 experts
    assert [c["T"] for c in eng.calls] == [3, 1] and all(c["pred_grad"] is gradient for c in eng.calls)
    for c in eng.calls:                                                  # the coordinates by index, the weights 1 / coords_scale^2
        assert c["pred_hess"]["dims"] == [0, 1]
        np.testing.assert_array_equal(c["pred_hess"]["lap_weight"], [0.25, 4.0, 0.0])
    preds = tabs["preds"]
    new = ["f*_hess_x_x", "f*_hess_var_x_x", "f*_hess_x_y", "f*_hess_var_x_y", "f*_hess_y_y", "f*_hess_var_y_y", "f*_lap", "f*_lap_var"]
    grad_cols = [f"f*_grad{v}_{c}" for c in ("x", "y", "t") for v in ("", "_var")] if gradient else []
    assert list(preds.columns) == (["_dim_0", "f*", "f*_var", "y_var", "f_bar"] + grad_cols + new
                                   + ["pred_loc_x", "pred_loc_y", "pred_loc_t"])
    assert len(preds) > 20 and np.isfinite(preds[new].values).all() and (preds[[c for c in new if "var" in c]].values > 0).all()
    # every expert: the per-tile model on the rows the selection gives it, at the same (default) parameters, predicting at its
    # own locations; neighbours share rows (radius 2.0, spacing 1.5), and every expert's values land in its own rows of preds.
    # The stand-in's BLAS does not round a tile alike inside a batch and alone (the slices are aligned differently): with
    # cond(K_y) about 1e3 that is 1e-13 of the prior scale, held here to 1e-11 relative + 1e-13; a wrong row, unit or column is O(1).
    close = dict(rtol=1e-11, atol=1e-13)
    shared, at = 0, 0
    mc = cfg["model_config"]
    osc = mc["init_params"]["obs_scale"]
    cc = ["x", "y", "t"]
    for k, loc in locs.iterrows():
        d = df[(df["x"] <= loc["x"] + radius) & (df["x"] >= loc["x"] - radius)]
        if k + 1 < len(locs):
            shared += int((d["x"] >= locs["x"][k + 1] - radius).sum())
        m = HipGPRModel(data=d, obs_col="z", coords_col=cc, engine=ph.HessNumpyEngine(), dtype="f64", **mc["init_params"])
        dist = np.sqrt(sum((pred[c] - loc[c]) ** 2 for c in cc))
        rows = preds.iloc[at:at + int((dist <= 1.3).sum())]
        at += len(rows)
        assert len(rows) > 0 and (rows.index.get_level_values("x") == loc["x"]).all()
        out = m.predict(rows[["pred_loc_x", "pred_loc_y", "pred_loc_t"]].values, hessian=[1, 0], gradient=gradient)
        np.testing.assert_allclose(rows["f*"].values, out["f*"], **close)
        # in the units f* is stored in (divided by obs_scale), per raw coordinate unit
        for (a, b) in ((0, 0), (0, 1), (1, 1)):
            np.testing.assert_allclose(rows[f"f*_hess_{cc[a]}_{cc[b]}"].values, out[f"f*_hess_{a}_{b}"] / osc, **close)
            np.testing.assert_allclose(rows[f"f*_hess_var_{cc[a]}_{cc[b]}"].values, out[f"f*_hess_var_{a}_{b}"] / osc ** 2, **close)
        np.testing.assert_allclose(rows["f*_lap"].values, out["f*_lap"] / osc, **close)
        np.testing.assert_allclose(rows["f*_lap_var"].values, out["f*_lap_var"] / osc ** 2, **close)
        for ci, c in enumerate(cc if gradient else []):
            np.testing.assert_allclose(rows[f"f*_grad_{c}"].values, out[f"f*_grad_{ci}"] / osc, **close)
            np.testing.assert_allclose(rows[f"f*_grad_var_{c}"].values, out[f"f*_grad_var_{ci}"] / osc ** 2, **close)
    assert at == len(preds) and shared > 50
    # the store holds the same columns
    from gpsat_amd.local_experts import get_results
    np.testing.assert_array_equal(get_results(str(tmp_path / "store"))["preds"][new].values, preds[new].values)
    # one expert per engine call: the same table
    tabs1 = BatchedLocalExpertOI(engine=ph.HessNumpyEngine(), **cfg).run(store_path=None, engine_chunk=1, optimise=False)
    pd.testing.assert_frame_equal(tabs1["preds"], preds, check_exact=False, **close)


def test_orchestrator_without_the_option_is_unchanged():
    cfg, *_ = _oi_case()
    mc = cfg["model_config"]
    eng, eng0 = ph.HessNumpyEngine(), ph.HessNumpyEngine()
    tabs = BatchedLocalExpertOI(engine=eng, dtype="f64", **cfg).run(store_path=None, optimise=False)
    for pk in ({}, {"hessian": False}, {"hessian": None}, None):
        oi0 = BatchedLocalExpertOI(engine=eng0, dtype="f64", **{**cfg, "model_config": {**mc, "pred_kwargs": pk}})
        assert oi0.pred_hess is None and oi0.pred_grad is False
        tabs0 = oi0.run(store_path=None, optimise=False)
        assert not any(c["pred_hess"] for c in eng0.calls)
        assert set(tabs0) == set(tabs) and not [c for c in tabs0["preds"].columns if "hess" in c or "lap" in c]
        assert list(tabs0["preds"].columns) == ["_dim_0", "f*", "f*_var", "y_var", "f_bar", "pred_loc_x", "pred_loc_y", "pred_loc_t"]
        for name in tabs0:
            if name != "run_details":
                cols = list(tabs0[name].columns)
                pd.testing.assert_frame_equal(tabs0[name], tabs[name][cols])
    # without the option dtype None stays fp32; hessian=True names every coordinate
    assert BatchedLocalExpertOI(engine=eng0, **{**cfg, "model_config": {**mc, "pred_kwargs": {}}}).dtype == "f32"
    assert BatchedLocalExpertOI(engine=eng0, **{**cfg, "model_config": {**mc, "pred_kwargs": {"hessian": True}}}).pred_hess == [0, 1, 2]


def test_orchestrator_refusals():
    cfg, *_ = _oi_case()
    mc, dc = cfg["model_config"], cfg["data_config"]
    E = ph.HessNumpyEngine
    ip = mc["init_params"]
    with pytest.raises(NotImplementedError, match="fp64 only"):
        BatchedLocalExpertOI(engine=E(), dtype="f32", **cfg)
    for kernel, match in (("Matern12", "mean-square"), ("Matern32", "Matern-3/2"), ("RationalQuadratic", "RationalQuadratic")):
        with pytest.raises(NotImplementedError, match=match):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {**ip, "kernel": kernel}}})
        # ... and as the kernel of a replacement profile
        with pytest.raises(NotImplementedError, match=match):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10,
                                                                         "replacement_init_params": {"kernel": kernel}}})
    # beside gradient, which Matern32 has: the run is still refused
    with pytest.raises(NotImplementedError, match="Matern-3/2"):
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "init_params": {**ip, "kernel": "Matern32"},
                                                                     "pred_kwargs": {"hessian": True, "gradient": True}}})
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
        BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "pred_kwargs": {"hessian": True, "full_cov": True}}})
    for bad in (["x", "lon"], [], "lon"):
        with pytest.raises(ValueError, match="names from coords_col"):
            BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "pred_kwargs": {"hessian": bad}}})
    # a replacement profile with a kernel of the row is accepted, and predicts the same columns
    oi = BatchedLocalExpertOI(engine=E(), **{**cfg, "model_config": {**mc, "replacement_threshold": 10,
                                                                      "replacement_init_params": {**ip, "kernel": "RBF"}}})
    assert oi.pred_hess == [0, 1] and oi.dtype == "f64"
