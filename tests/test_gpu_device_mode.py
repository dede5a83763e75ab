"""GPU: device mode (contiguous torch tensors on the GPU, GPSAT_MEM_DEVICE) held to host mode's bits on every entry point of
Engine.fit_predict_batch and Engine.sgpr_fit_predict_batch, for every variant and every kernel build.

Every case runs the same inputs twice -- as numpy arrays and as views carved out of one device allocation at odd element
offsets between guard bands (tests/device_mode.py) -- and asserts that every field of the two BatchResults has the same
bytes, that guards and inputs kept theirs and that nothing beyond ``out[i][:sumP]`` was written.  Two equal runs can both be
wrong, so every case also holds its device result to the fp64 reference at the bounds the project states for the operation:
tests/variant_cases.check_tile (fp64 and its variants), tests/test_gpu_parity.py::_check_eval (fp64 -> fp32) and
test_full_cov_ragged_batch_matches_oracle, tests/test_gpu_cv.py::_check, tests/test_gpu_cv_refit.py, tests/sgpr_edge_cases.py.
"""
import dataclasses
import re

import numpy as np
import pytest

import device_mode as dm
import sgpr_edge_cases as ec
import variant_cases as vc
import variant_numpy as vn
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import GpsatError
from test_gpu_cv import _check as check_held_out
from test_gpu_parity import _check_eval as check_f32_tile
from variant_cases import eng  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

KERNELS = dm.KERNELS
PRED = ("f_mean", "f_var", "y_var")


class PlainCase(vc.Case):
    """The plain fp64 expert as a variant without a parameter or an argument of its own."""
    variant, name = vn.Variant("plain", 0, "none"), "plain"


PLAIN = PlainCase()


@pytest.fixture(scope="module", autouse=True)
def tally():
    yield
    for family, (runs, fields, nones) in dm.TALLY.items():
        print(f"\ndevice mode, {family}: {runs} device runs, {fields} fields byte-equal to host mode, {nones} fields None in both")


@pytest.fixture(scope="module")
def num_cu(eng):  # noqa: F811
    import torch
    return torch.cuda.get_device_properties(eng.device_id).multi_processor_count


def hold(case, dtype, r, b, thetas, what):
    """Every tile of the (downloaded) device result against the fp64 reference at ``thetas`` [T, H]."""
    T, kid = len(b["obs_off"]) - 1, (KERNELS.index(b["kernel"]) if b["kernel"] in KERNELS else None)
    for t in range(T):
        a, e = int(b["obs_off"][t]), int(b["obs_off"][t + 1])
        if dtype == "f32":
            if e > a:                                          # an empty tile has no fp64 -> fp32 bound: its bits are host mode's
                check_f32_tile(r, b, t, thetas[t], kid)
            continue
        rr = r
        if r.grad is None:                                     # check_tile reads a gradient: none was asked for, hand it the reference's own
            g = np.zeros_like(r.theta)
            if e > a:
                v = b["obs_var"][a:e] if case.variant is vn.NOISE else None
                g[t] = vn.nll_and_grad(case.variant, b["kernel"], b["X"][a:e], b["y"][a:e], thetas[t], v)[1]
            rr = dataclasses.replace(r, grad=g)
        vc.check_tile(case, rr, b, t, thetas[t], what)


def fit_kw(optimiser, T, D, case=PLAIN):
    if optimiser == "none":
        return {}
    lo, hi = case.bounds(T, D)
    return dict(lo=lo, hi=hi, max_iter=8, **({"adam_lr": 0.05} if optimiser == "adam" else {}))


# ---- 1. the plain call
PLAIN_RUNS = [(dt, opt, wg, "Matern32") for dt in ("f32", "f64") for opt in ("none", "lbfgs", "adam") for wg in (False, True)] + \
             [(dt, "none", True, k) for dt in ("f32", "f64") for k in ("RBF", "Matern12", "Matern52")]


@pytest.mark.parametrize("dtype,optimiser,want_grad,kernel", PLAIN_RUNS)
def test_plain_call(eng, dtype, optimiser, want_grad, kernel):  # noqa: F811
    b = dm.ragged(dtype, kid=KERNELS.index(kernel))
    T, D = 6, 3
    th0 = PLAIN.theta(np.random.default_rng(7), T, D) if optimiser == "none" else np.ones((T, D + 2))
    kw = dict(theta0=th0, kernel=kernel, optimiser=optimiser, want_grad=want_grad, dtype=dtype, **fit_kw(optimiser, T, D))
    host, r, _, _ = dm.run_pair(eng, b, dtype, kw, "plain", out={"none": "over", "lbfgs": "exact", "adam": None}[optimiser])
    assert (r.grad is not None) == want_grad and r.status[dm.EMPTY] == 4 and np.isin(np.delete(r.status, dm.EMPTY), (0, 1, 5, 6)).all(), r.status
    if optimiser != "none":
        assert (np.delete(r.n_eval, dm.EMPTY) > 1).all()
    hold(PLAIN, dtype, r, b, th0 if optimiser == "none" else r.theta, f"plain {dtype} {optimiser}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_dimension(eng, dtype):  # noqa: F811
    b = dm.ragged(dtype, D=1, kid=0, seed=4100)
    th0 = PLAIN.theta(np.random.default_rng(8), 6, 1)
    _, r, _, _ = dm.run_pair(eng, b, dtype, dict(theta0=th0, kernel="RBF", optimiser="none", want_grad=True, dtype=dtype), "plain", out="over")
    hold(PLAIN, dtype, r, b, th0, f"D = 1 {dtype}")


# ---- the two whole-batch edges
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_no_prediction_point_at_all(eng, dtype):  # noqa: F811
    """sumP == 0: Xs is a tensor without elements or storage, the outputs are one-element allocations that stay untouched."""
    b = dm.make_batch(dtype, dm.RAGGED_N[dtype], [0] * 6)
    th0 = PLAIN.theta(np.random.default_rng(9), 6, 3)
    _, r, dev, c = dm.run_pair(eng, b, dtype, dict(theta0=th0, kernel="Matern32", optimiser="none", want_grad=True, dtype=dtype), "edges")
    assert c.inputs["Xs"].numel() == 0 and c.inputs["Xs"].data_ptr() == 0 and all(o.numel() == 1 for o in c.outs.values())
    assert all(getattr(dev, k).numel() == 0 for k in PRED)
    hold(PLAIN, dtype, r, b, th0, f"sumP = 0 {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_no_observation_at_all(eng, dtype):  # noqa: F811
    """sumN == 0 with sumP > 0: every tile predicts the prior at theta0."""
    b = dm.make_batch(dtype, [0, 0, 0], [5, 0, 33])
    th0 = PLAIN.theta(np.random.default_rng(10), 3, 3)
    _, r, _, c = dm.run_pair(eng, b, dtype, dict(theta0=th0, kernel="Matern32", optimiser="none", want_grad=True, dtype=dtype), "edges", out="over")
    assert c.inputs["X"].data_ptr() == 0 and c.inputs["y"].data_ptr() == 0 and (r.status == 4).all()
    if dtype == "f64":
        hold(PLAIN, dtype, r, b, th0, "sumN = 0")
    else:                                                      # the prior, at the fp64 -> fp32 bounds of the predictions
        sf2, sn2 = np.repeat(th0[:, 3], [5, 0, 33]), np.repeat(th0[:, 4], [5, 0, 33])
        assert (r.f_mean == 0).all() and (np.abs(r.f_var - sf2) <= 2e-3 * sf2 + 1e-6).all()
        np.testing.assert_allclose(r.y_var - r.f_var, sn2, rtol=1e-3, atol=1e-6)


# ---- 2. the full covariance
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_full_covariance(eng, dtype):  # noqa: F811
    b = dm.ragged(dtype, kid=0)
    th0 = np.tile([2.0, 2.0, 2.0, 0.8, 0.05], (6, 1))
    _, r, _, _ = dm.run_pair(eng, b, dtype, dict(theta0=th0, kernel="RBF", optimiser="none", dtype=dtype, full_cov=True), "full_cov")
    np.testing.assert_array_equal(r.cov_off, np.concatenate([[0], np.cumsum(np.square(dm.RAGGED_P))]))
    assert r.cov_off.dtype == np.int64 and len(r.f_cov) == sum(p * p for p in dm.RAGGED_P)
    for t in range(6):
        dm.check_cov_tile(r, b, t, th0[t], dtype)


# ---- 3. held-out predictions from every tile's own factor (fp64)
def sparse_labels(Ns, rng):
    """Labels with gaps (1000 k + 7), shuffled, about one row in ten negative (-5) and one -1 per tile of more than two rows."""
    out = []
    for N in Ns:
        lab = (rng.integers(0, max(N // 8, 1) + 1, N).astype(np.int64) * 1000 + 7).astype(np.int32)
        lab[rng.random(N) < 0.1] = -5
        if N > 2:
            lab[N // 2] = -1
        out.append(lab)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


@pytest.mark.parametrize("fold,optimiser", [("loo", "none"), ("labels", "none"), ("labels", "lbfgs")])
def test_held_out_predictions(eng, fold, optimiser):  # noqa: F811
    b = dm.ragged("f64")
    Ns, T, D = dm.RAGGED_N["f64"], 6, 3
    labels = None if fold == "loo" else sparse_labels(Ns, np.random.default_rng(21))
    assert labels is None or ((labels < 0).sum() > 5 and labels.max() > 1000)
    th0 = PLAIN.theta(np.random.default_rng(11), T, D) if optimiser == "none" else np.ones((T, D + 2))
    kw = dict(theta0=th0, kernel="Matern32", optimiser=optimiser, dtype="f64", cv_fold="loo" if labels is None else labels,
              **fit_kw(optimiser, T, D))
    _, r, _, _ = dm.run_pair(eng, b, "f64", kw, "cv_fold", out="over")
    for t in range(T):
        a, e = int(b["obs_off"][t]), int(b["obs_off"][t + 1])
        if e > a:
            check_held_out(r, a, e, b["X"][a:e], b["y"][a:e], r.theta[t], 2, None if labels is None else labels[a:e], f"{fold} tile {t}")
    hold(PLAIN, "f64", r, b, r.theta, f"cv_fold {fold}")


# ---- 4. refitted folds, split over several library calls
REFIT_N = {"f32": [31, 100, 0, 1, 32, 100, 33], "f64": [15, 100, 0, 1, 16, 100, 17]}
REFIT_P = [1, 33, 7, 0, 0, 32, 1]


def refit_labels(Ns, rng):
    """Four folds (labels 3, 40, 77, 114), shuffled; one row of every tile of more than one row is never held out."""
    out = []
    for N in Ns:
        lab = (rng.integers(0, 4, N) * 37 + 3).astype(np.int32)
        if N > 1:
            lab[N // 2] = -1
        out.append(lab)
    return np.concatenate(out)


class CountingLib:
    """The engine's library, counting the calls of one entry point."""
    def __init__(self, lib, name):
        self.lib, self.name, self.calls = lib, name, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != self.name:
            return fn

        def counted(*args):
            self.calls += 1
            return fn(*args)
        return counted


@pytest.mark.parametrize("shape", ["2d", "flat", "no predictions"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_refitted_folds_split_over_library_calls(eng, monkeypatch, dtype, shape):  # noqa: F811
    """The device run is split by max_expanded_rows into at least three library calls and compared with the UNSPLIT host run.
    "flat": X and Xs as one-dimensional tensors of the same memory -- the ranges after the first must still be taken by rows.
    "no predictions": every P = 0, so every range hands the library one-element outputs."""
    Ns = REFIT_N[dtype]
    Ps = [0] * len(Ns) if shape == "no predictions" else REFIT_P
    b = dm.make_batch(dtype, Ns, Ps, seed=4200)
    T, D = len(Ns), 3
    labels = refit_labels(Ns, np.random.default_rng(31))
    folds = [len(np.unique(l_[l_ >= 0])) for l_ in np.split(labels, b["obs_off"][1:-1])]
    per_tile = np.array([f * n for f, n in zip(folds, Ns)]) - np.array([(l_ >= 0).sum() for l_ in np.split(labels, b["obs_off"][1:-1])])
    budget = int(per_tile.max())                                # the two largest tiles run alone
    lo, hi = syn.default_bounds(T, D)
    kw = dict(theta0=np.ones((T, D + 2)), lo=lo, hi=hi, kernel="Matern32", optimiser="lbfgs", max_iter=6, dtype=dtype, cv_fold=labels)
    lib = CountingLib(eng._lib, "gpsat_fit_predict_batch_cv_refit")
    monkeypatch.setattr(eng, "_lib", lib)
    names = ("X", "y", "Xs")
    host = eng.fit_predict_batch(**dm.meta_of(b), **{k: b[k] for k in names}, **kw, cv_refit=True)
    assert lib.calls == 1
    import torch
    sumP = int(b["pred_off"][-1])
    c = dm.Carved({k: (b[k].reshape(-1) if shape == "flat" else b[k]) for k in names}, {k: max(sumP, 1) for k in PRED}, dtype,
                  torch.device("cuda", eng.device_id))
    dev = eng.fit_predict_batch(**dm.meta_of(b), **c.inputs, out=tuple(c.outs.values()), **kw, cv_refit={"max_expanded_rows": budget})
    monkeypatch.undo()
    assert lib.calls >= 1 + 3, lib.calls
    c.verify(sumP)
    dm.same_result(host, dev, eng.device_id, "cv_refit", f"{dtype} {shape}")
    r = dm.to_numpy(dev)
    assert r.cv_status[r.cv_fold_off[3]] == 4 and (r.cv_fold_off[3] == r.cv_fold_off[2])    # the one-row tile's fold is not fitted; the empty tile has none
    assert dm.check_refit_fold(r, b, labels, 1, dtype) + dm.check_refit_fold(r, b, labels, 6, dtype) >= 6
    if dtype == "f64":
        hold(PLAIN, dtype, r, b, r.theta, f"cv_refit {shape}")


# ---- 5. multi-start
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_multi_start(eng, dtype):  # noqa: F811
    b = dm.ragged(dtype)
    T, D, H = 6, 3, 5
    lo, hi = np.tile([0.1, 0.1, 0.1, 1e-3, 1e-4], (T, 1)), np.tile([12.0, 12.0, 9.0, 10.0, 1.0], (T, 1))
    starts = np.exp(np.random.default_rng(41).uniform(np.log(lo), np.log(hi), (2, T, H))).transpose(1, 0, 2)
    kw = dict(theta0=np.tile([1.0, 1.0, 1.0, 0.1, 0.05], (T, 1)), lo=lo, hi=hi, kernel="Matern32", optimiser="lbfgs", max_iter=6, dtype=dtype,
              n_starts=3, starts=starts, want_grad=True)
    _, r, _, _ = dm.run_pair(eng, b, dtype, kw, "multistart", out="exact")
    assert r.f_start.shape == (T, 3) and np.isfinite(np.delete(r.f_start, dm.EMPTY, axis=0)).all()
    hold(PLAIN, dtype, r, b, r.theta, f"multi-start {dtype}")


# ---- 6. the variants of the fp64 expert
@pytest.mark.parametrize("optimiser", ["none", "lbfgs"])
@pytest.mark.parametrize("case,x", [(vc.MEAN, -0.7), (vc.RQ, 1.5), (vc.NOISE, None)], ids=["mean", "rq", "noise"])
def test_fp64_variants(eng, case, x, optimiser):  # noqa: F811
    Ns, T, D = dm.RAGGED_N["f64"], 6, 3
    b = case.batch(T, Ns, dm.RAGGED_P, D, "Matern32", 4300)
    th0 = case.theta(np.random.default_rng(51), T, D, x)
    kw = dict(theta0=th0, kernel=b["kernel"], optimiser=optimiser, want_grad=True, dtype="f64", **fit_kw(optimiser, T, D, case),
              **({"mean": "constant"} if case is vc.MEAN else {}))
    _, r, _, _ = dm.run_pair(eng, b, "f64", kw, f"variant {case.name}", out="over", more=("obs_var",) if case is vc.NOISE else ())
    assert r.theta.shape == (T, D + 2 + case.variant.extra)
    if optimiser == "lbfgs":
        assert (np.delete(r.n_eval, dm.EMPTY) > 1).all()
    thetas = r.theta.copy()
    thetas[dm.EMPTY] = th0[dm.EMPTY]                            # the empty tile: the prior at theta0
    hold(case, "f64", r, b, thetas, f"{case.name} {optimiser}")


# ---- 7. the sparse experts
@pytest.mark.parametrize("optimiser", ["none", "lbfgs"])
def test_sparse_experts_with_out(eng, optimiser):  # noqa: F811
    """The batch is centred on the host so that host mode's own centring subtracts exactly 0 (tests/sgpr_edge_cases.py)."""
    kid, D, pk, th0 = ec.centred_exact_batch()
    b = dict(pk, D=D)
    kw = dict(z_off=pk["z_off"], kernel=kid, theta0=th0, optimiser=optimiser, max_iter=8, want_grad=True)
    _, r, _, _ = dm.run_pair(eng, b, "f64", kw, "sgpr", out="over", more=("Z",), entry="sgpr_fit_predict_batch")
    for t in range(len(pk["obs_off"]) - 1):
        tile = tuple(pk[k][pk[o][t]:pk[o][t + 1]] for k, o in (("X", "obs_off"), ("y", "obs_off"), ("Z", "z_off"), ("Xs", "pred_off")))
        ec.check_tile(r, t, pk["pred_off"], kid, tile, r.theta[t], cond_max=ec.COND_MAX if optimiser == "none" else None)


# ---- 8. builds and launch modes: each at the smallest batch that reaches it, the mode asserted from gpsat::plan_tiles
def deferred_predictions(capfd):
    m = re.findall(r"gpsat defer: T \d+: deferred predictions (\d+) of (\d+) snapshot slots", capfd.readouterr().err)
    assert m, "no deferral statistics printed"
    return int(m[-1][0]), int(m[-1][1])


def test_fp32_four_wave_build_time_sliced_with_deferred_predictions(monkeypatch, capfd, num_cu):
    """What the benchmark runs: more tiles than CUs on the 4-wave fp32 build, every evaluation a time slice, predictions
    deferred to the end of the launch and written into the caller's ``out`` from there.  64 resident workgroups, so that
    tiles do wait when others finish: only then is a prediction deferred."""
    from gpsat_amd.engine import Engine
    T, D = num_cu + 44, 3
    rng = np.random.default_rng(61)
    b = dm.make_batch("f32", rng.integers(20, 91, T).tolist(), rng.integers(0, 10, T).tolist(), kid=0, seed=4400)
    knobs = {"seg": 1, "grid": 64}
    plan = dm.plan_of(b, "f32", num_cu, "lbfgs", 8, knobs=knobs)
    assert plan["build"] == dm.BUILD_F32_W4 and plan["seg_cost"] == 1 and plan["pq_slots"] == T and plan["grid"] == 64 and plan["coop"] == 0, plan
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "1")
    monkeypatch.setenv("GPSAT_DEBUG_GRID", "64")
    monkeypatch.setenv("GPSAT_DEBUG_DEFER_STATS", "1")
    monkeypatch.delenv("GPSAT_DEBUG_DEFER", raising=False)
    e = Engine(0)
    try:
        lo, hi = syn.default_bounds(T, D)
        kw = dict(theta0=np.ones((T, D + 2)), lo=lo, hi=hi, kernel="RBF", optimiser="lbfgs", max_iter=8, want_grad=True, dtype="f32")
        host, r, dev, c = dm.run_pair(e, b, "f32", kw, "fp32 4-wave sliced deferred", out="exact")
        n, slots = deferred_predictions(capfd)
        assert slots == T and n > 0, (n, slots)
        monkeypatch.setenv("GPSAT_DEBUG_DEFER", "0")
        inline = e.fit_predict_batch(**dm.meta_of(b), **c.inputs, out=tuple(c.outs.values()), **kw)
        assert deferred_predictions(capfd)[0] == 0
        c.verify(int(b["pred_off"][-1]))
        dm.same_result(host, inline, e.device_id, "fp32 4-wave sliced deferred", "inline")
    finally:
        e.close()
    assert np.isin(r.status, (0, 1, 6)).all() and np.isfinite(r.f_mean).all()
    for t in (0, T // 2, T - 1):
        check_f32_tile(r, b, t, r.theta[t], 0)


def test_fp32_eight_wave_build_with_cooperative_helpers(eng, num_cu):  # noqa: F811
    b = dm.make_batch("f32", [400, 64, 33], [9, 0, 33], kid=2, seed=4500)
    plan = dm.plan_of(b, "f32", num_cu, "lbfgs", 4)
    assert plan["build"] == dm.BUILD_F32_W8 and plan["coop"] == 1 and plan["grid"] > 3 and plan["NBmax"] >= 12, plan
    lo, hi = syn.default_bounds(3, 3)
    kw = dict(theta0=np.ones((3, 5)), lo=lo, hi=hi, kernel="Matern32", optimiser="lbfgs", max_iter=4, want_grad=True, dtype="f32")
    _, r, _, _ = dm.run_pair(eng, b, "f32", kw, "fp32 8-wave cooperative", out="over")
    hold(PLAIN, "f32", r, b, r.theta, "cooperative tiles")


@pytest.mark.parametrize("optimiser,max_iter", [("none", 0), ("lbfgs", 2)])
def test_fp64_eight_wave_build_with_a_team(eng, num_cu, optimiser, max_iter):  # noqa: F811
    b = dm.make_batch("f64", [1200, 90], [9, 33], kid=2, seed=4600)
    plan = dm.plan_of(b, "f64", num_cu, optimiser, max_iter)
    assert plan["build"] == dm.BUILD_F64_W8 and plan["team"] > 1 and plan["NBmax"] >= 64 and plan["grid"] == 2 * plan["team"], plan
    th0 = np.array([b["truth"][0], b["truth"][1]]) if optimiser == "none" else np.ones((2, 5))
    lo, hi = syn.default_bounds(2, 3)
    kw = dict(theta0=th0, lo=lo, hi=hi, kernel="Matern32", optimiser=optimiser, max_iter=max_iter, want_grad=True, dtype="f64")
    _, r, _, _ = dm.run_pair(eng, b, "f64", kw, "fp64 8-wave team", out="exact")
    hold(PLAIN, "f64", r, b, r.theta, f"team {optimiser}")


# ---- 9. the contract of out
def test_out_is_written_in_place_and_can_be_reused(eng):  # noqa: F811
    import torch
    b = dm.ragged("f32")
    sumP = int(b["pred_off"][-1])
    kw = dict(theta0=PLAIN.theta(np.random.default_rng(71), 6, 3), kernel="Matern32", optimiser="none", dtype="f32")
    host, r, dev, c = dm.run_pair(eng, b, "f32", kw, "out", out="exact")
    assert all(getattr(dev, k).data_ptr() == c.outs[k].data_ptr() and getattr(dev, k).numel() == c.outs[k].numel() == sumP for k in PRED)
    first = {k: c.outs[k].cpu().numpy().tobytes() for k in PRED}
    # the same out, filled with something else in between: the second call writes the same bits
    for o in c.outs.values():
        o.fill_(3.0)
    again = eng.fit_predict_batch(**dm.meta_of(b), **c.inputs, out=tuple(c.outs.values()), **kw)
    c.verify(sumP)
    dm.same_result(host, again, eng.device_id, "out", "reused")
    assert all(c.outs[k].cpu().numpy().tobytes() == first[k] == getattr(host, k).tobytes() for k in PRED)
    # oversized, and shaped (n, 1): accepted, the result is the flat [:sumP] view of the caller's storage, the tail untouched
    big = [torch.full((sumP + 5, 1), dm.SENTINEL, dtype=torch.float32, device=c.buf.device) for _ in range(3)]
    over = eng.fit_predict_batch(**dm.meta_of(b), **c.inputs, out=big, **kw)
    dm.same_result(host, over, eng.device_id, "out", "oversized")
    for o, k in zip(big, PRED):
        assert getattr(over, k).data_ptr() == o.data_ptr() and getattr(over, k).shape == (sumP,)
        assert (o.reshape(-1)[sumP:] == dm.SENTINEL).all() and o.reshape(-1)[:sumP].cpu().numpy().tobytes() == first[k]
    hold(PLAIN, "f32", r, b, kw["theta0"], "out")


# ---- 10. what the wrapper refuses, before any library call
def test_refusals_name_the_argument_and_reach_no_library_call(eng, monkeypatch):  # noqa: F811
    import torch
    b = dm.ragged("f32")
    sumN, sumP, D = int(b["obs_off"][-1]), int(b["pred_off"][-1]), 3
    dev = torch.device("cuda", eng.device_id)
    kw = dict(theta0=PLAIN.theta(np.random.default_rng(81), 6, D), kernel="Matern32", optimiser="none", dtype="f32", want_grad=True)
    good_host = eng.fit_predict_batch(**dm.meta_of(b), X=b["X"], y=b["y"], Xs=b["Xs"], **kw)
    X, y, Xs = (torch.from_numpy(b[k]).to(dev) for k in ("X", "y", "Xs"))
    outs = lambda n=sumP, dt=torch.float32, where=dev: tuple(torch.empty(n, dtype=dt, device=where) for _ in range(3))
    wide = torch.empty((sumP, 2), dtype=torch.float32, device=dev)
    Xt = torch.from_numpy(np.ascontiguousarray(b["X"].T)).to(dev).T            # [sumN, D] with strides (1, sumN)
    assert Xt.shape == X.shape and not Xt.is_contiguous()
    bad = [(dict(out=outs(sumP - 1)), r"out \(f_mean\).*at least"),
           (dict(out=outs()[:2] + (torch.empty(sumP - 1, dtype=torch.float32, device=dev),)), r"out \(y_var\).*at least"),
           (dict(out=outs(dt=torch.float64)), r"out \(f_mean\).*dtype"),
           (dict(out=outs(where="cpu")), r"out \(f_mean\).*cpu"),
           (dict(out=(wide[:, 0], wide[:, 1], wide[:, 0])), r"out \(f_mean\).*contiguous"),
           (dict(out=outs()[:2]), r"out: three tensors"),
           (dict(y=y[:-1]), rf"^y: has {sumN - 1} elements, {sumN} expected"),
           (dict(y=b["y"]), r"^y: .*torch tensors.*ndarray"),
           (dict(X=Xt), r"^X: .*contiguous"),
           (dict(Xs=Xs.double()), r"^Xs: .*dtype")]
    called = []

    class NoLib:
        def __getattr__(self, name):
            called.append(name)
            raise AssertionError(f"the library was reached ({name}) by a call that must be refused before")
    for change, match in bad:
        monkeypatch.setattr(eng, "_lib", NoLib())
        with pytest.raises(GpsatError, match=match):
            eng.fit_predict_batch(**dm.meta_of(b), **{**dict(X=X, y=y, Xs=Xs), **change}, **kw)
        monkeypatch.undo()
    # out with numpy inputs: host mode returns new arrays and says so
    monkeypatch.setattr(eng, "_lib", NoLib())
    with pytest.raises(GpsatError, match=r"^out: .*device mode"):
        eng.fit_predict_batch(**dm.meta_of(b), X=b["X"], y=b["y"], Xs=b["Xs"], out=outs(), **kw)
    with pytest.raises(GpsatError, match=r"^trainable has shape"):
        eng.fit_predict_batch(**dm.meta_of(b), X=X, y=y, Xs=Xs, trainable=[True] * 4, **kw)
    monkeypatch.undo()
    assert called == []
    # and the engine works as before
    o = outs()
    good = eng.fit_predict_batch(**dm.meta_of(b), X=X, y=y, Xs=Xs, out=o, **kw)
    dm.same_result(good_host, good, eng.device_id, "after the refusals")
    hold(PLAIN, "f32", dm.to_numpy(good), b, kw["theta0"], "after the refusals")


def test_tensors_on_another_device_are_refused(eng, monkeypatch):  # noqa: F811
    """Every bulk argument and every output is compared with the engine's device, not X alone."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device: no other device to put a tensor on")
    b = dm.ragged("f32")
    sumP = int(b["pred_off"][-1])
    dev, other = torch.device("cuda", eng.device_id), torch.device("cuda", (eng.device_id + 1) % torch.cuda.device_count())
    t = {k: torch.from_numpy(b[k]).to(dev) for k in ("X", "y", "Xs")}
    kw = dict(theta0=np.ones((6, 5)), kernel="Matern32", optimiser="none", dtype="f32")
    monkeypatch.setattr(eng, "_lib", None)                      # any library call would raise AttributeError
    for name in ("X", "y", "Xs"):
        with pytest.raises(GpsatError, match=rf"^{name}: lives on cuda:{other.index}"):
            eng.fit_predict_batch(**dm.meta_of(b), **{**t, name: t[name].to(other)}, **kw)
    for i, name in enumerate(PRED):
        out = [torch.empty(sumP, dtype=torch.float32, device=other if j == i else dev) for j in range(3)]
        with pytest.raises(GpsatError, match=rf"^out \({name}\): lives on cuda:{other.index}"):
            eng.fit_predict_batch(**dm.meta_of(b), **t, out=out, **kw)


# ---- 11. stream order
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_inputs_uploaded_on_a_side_stream_are_complete_when_read(eng, dtype):  # noqa: F811
    import torch
    rng = np.random.default_rng(91)
    T = 40
    b = dm.make_batch(dtype, rng.integers(60, 200, T).tolist(), [16] * T, kid=2, seed=4700)
    th0 = PLAIN.theta(rng, T, 3)
    kw = dict(theta0=th0, kernel="Matern32", optimiser="none", dtype=dtype, want_grad=True)
    host = eng.fit_predict_batch(**dm.meta_of(b), X=b["X"], y=b["y"], Xs=b["Xs"], **kw)
    dev = torch.device("cuda", eng.device_id)
    pinned = {k: torch.from_numpy(b[k]).pin_memory() for k in ("X", "y", "Xs")}
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        t = {k: v.to(dev, non_blocking=True) for k, v in pinned.items()}
        r = eng.fit_predict_batch(**dm.meta_of(b), **t, **kw)
    dm.same_result(host, r, eng.device_id, "stream order", dtype)
    hold(PLAIN, dtype, dm.to_numpy(r), b, th0, f"side stream {dtype}")
