"""CPU: what tests/test_gpu_variant_sizes.py leans on, checked without a GPU.

1. The size ladder (the last tile of the 4-wave build, the largest tile the ABI accepts) against gpsat_max_tile_obs and the LDS
   layouts: a change of the layout moves the ladder knowingly.
2. The references by themselves.  At the largest tiles of the GPU module (D = 1, N = 4096 and D = 4, N = 2416; its own inputs)
   every restatement is compared with a second fp64 route and has to stay within ONE TENTH of each bound it is used with, so that
   a failure of the GPU module is the kernel's:
     predictions, gradient and second derivatives   the quadratic forms k^T K_y^-1 y and prior - k^T K_y^-1 k through
                                                    scipy.linalg.solve(K_y, ., assume_a="sym") instead of V = L^-1 k
     held-out predictions                           the closed form against deletion, on the folds the GPU module deletes
     objective of rq, mean, noise                   through slogdet and solve
     gradient of rq, mean, noise                    central differences of that objective at a step of 1e-5 relative, held to the
                                                    gradient bound's own rtol 1e-7 (and atol): the tenth does not apply to a
                                                    difference quotient, whose own error is of the bound's size
3. The checks of the GPU module trip when what they are fed is subtly wrong: the restatement with one 16-row block row of
   V = L^-1 (right-hand side) zeroed, or with one fold's A_GG missing one pair of blocks, fails; the same restatement
   untouched passes.
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.linalg import solve, solve_triangular

import cv_numpy as cvn
import pred_grad_numpy as pg
import pred_hess_numpy as ph
import test_gpu_build_matrix as bm
import test_gpu_variant_sizes as vs
import variant_numpy as vn
from gpsat_amd import _lib as L

TENTH = 0.1
LOG_2PI = 1.8378770664093453


# ---- 1. the ladder
def test_size_ladder_is_the_abi_and_the_lds_layouts():
    assert [vs.ladder(D) for D in (1, 2, 3, 4)] == [(976, 4096), (784, 3392), (656, 2832), (560, 2416)]
    for D in (1, 2, 3, 4):
        nd4, Nmax = vs.ladder(D)
        # (D4_NB itself is held to the 4-wave LDS layout by tests/test_abi.py::test_four_wave_thresholds_of_the_build_matrix)
        assert Nmax == L.max_tile_obs("f64", D) and nd4 == 16 * bm.D4_NB[D] and nd4 + 1 < Nmax - 15
        assert L.max_cv_fold("f64", D) == 256
    assert Nmax - 15 == 16 * (Nmax // 16 - 1) + 1            # its last block holds one row
    assert sorted({D for row, D in vs.ROW_AND_D if row in ("rq", "mean")}) == [1, 2, 3]
    assert sorted({D for row, D in vs.ROW_AND_D if row not in ("rq", "mean")}) == [1, 2, 3, 4]
    # above 224 blocks the exchange area takes its second formula: only D = 1 gets there
    assert 4096 // 16 > 224 >= 3392 // 16


# ---- 2. the references' own margin
def _largest(row, D):
    b, theta = vs.inputs(row, D, "B")
    t = b["T"] - 1
    o, p = vs._tile(b, t)
    assert o.stop - o.start == vs.ladder(D)[1]
    return b, theta[t], o, p


def _second_route(variant, kernel, X, y, theta, v, W):
    """(K_y, K_y^-1 [y - c, W]) by a symmetric indefinite solve: no Cholesky factor, no triangular solve."""
    D = X.shape[1]
    Ky = vn.K_y(variant, kernel, X, theta, v)
    c = float(theta[D + 2]) if variant is vn.MEAN else 0.0
    return Ky, c, solve(Ky, np.column_stack([y - c, W]), assume_a="sym")


def _objective(variant, kernel, X, y, theta, v):
    D = X.shape[1]
    Ky = vn.K_y(variant, kernel, X, theta, v)
    r = y - (float(theta[D + 2]) if variant is vn.MEAN else 0.0)
    sign, logdet = np.linalg.slogdet(Ky)
    assert sign == 1.0
    return 0.5 * r @ solve(Ky, r, assume_a="sym") + 0.5 * logdet + 0.5 * len(y) * LOG_2PI


MARGINS = [(row, D) for row, D in vs.ROW_AND_D if D in (1, 4)]


@pytest.mark.parametrize("row,D", MARGINS, ids=[f"{row}-D{D}" for row, D in MARGINS])
def test_reference_stays_within_a_tenth_of_every_bound(row, D):
    b, theta, o, p = _largest(row, D)
    X, y, Xs, kernel = b["X"][o], b["y"][o], b["Xs"][p], b["kernel"]
    ymax = max(np.abs(y).max(), 1.0)
    t0 = time.perf_counter()
    if row == "cv":
        kid, lab = L.KERNEL_IDS[kernel], b["cv_fold"][o]
        folds = vs.deleted_folds(lab, len(lab))
        assert len(folds) == vs.N_DELETED and (lab == folds[0]).sum() == L.max_cv_fold("f64", D)
        keep = np.isin(lab, folds)
        m1, f1, y1 = cvn.closed_form(kid, X, y, theta, lab)
        m2, f2, y2 = cvn.deletion(kid, X, y, theta, np.where(keep, lab, -1))
        fig = {"cv_mean": np.abs(m1 - m2)[keep].max() / (1e-9 * ymax), "cv_f_var": np.abs(f1 - f2)[keep].max() / 1e-10,
               "cv_y_var": np.abs(y1 - y2)[keep].max() / 1e-10, "cv_sn2": np.abs(y1 - f1 - theta[D + 1]).max() / 1e-12}
    else:
        case = vs.CASE[row]
        variant = case.variant
        v = b["obs_var"][o] if variant is vn.NOISE else None
        ell = theta[:D]
        cols, Ks = [], vn.kernel_matrix(variant, kernel, X, Xs, theta)
        cols.append(Ks)
        if row == "grad":
            G = pg.cross_gradient(kernel, X, Xs, theta)
            cols += list(G)
        if row == "hess":
            spec = vs.hess_spec(D)
            pairs, w = ph.pairs(spec["dims"]), np.asarray(spec["lap_weight"])
            Hm = ph.cross_hessian(kernel, X, Xs, theta)
            cols += [Hm[a, c] for a, c in pairs] + [sum(w[a] * Hm[a, a] for a in range(D))]
        Ky, c, S = _second_route(variant, kernel, X, y, theta, v, np.column_stack(cols))
        alpha, P = S[:, 0], len(Xs)
        quad = [(W.T @ alpha, np.sum(W * S[:, 1 + k * P:1 + (k + 1) * P], axis=0)) for k, W in enumerate(cols)]
        f, fv, yv = vn.predict(variant, kernel, X, y, Xs, theta, v)
        fig = {"f_mean": np.abs(f - (quad[0][0] + c)).max() / (1e-9 * ymax), "f_var": np.abs(fv - (theta[D] - quad[0][1])).max() / 1e-10,
               "y_var": np.abs(yv - (theta[D] - quad[0][1] + theta[D + 1])).max() / 1e-10}
        if row == "grad":
            fg, fgv = pg.predict_grad(kernel, X, y, Xs, theta)
            prior = pg.prior_grad(kernel, theta, P, D)[1]
            fig["f_grad"] = max(np.abs(fg[:, a] - quad[1 + a][0]).max() * ell[a] for a in range(D)) / (1e-9 * ymax)
            fig["f_grad_var"] = max(np.abs(fgv[:, a] - (prior[:, a] - quad[1 + a][1])).max() * ell[a] ** 2 for a in range(D)) / 3e-10
        if row == "hess":
            fh, fhv, fl, flv = ph.predict_hess(kernel, X, y, Xs, theta, spec["dims"], spec["lap_weight"])
            sc = [ell[a] * ell[c_] for a, c_ in pairs]
            fig["f_hess"] = max(np.abs(fh[:, k] - quad[1 + k][0]).max() * sc[k] for k in range(len(pairs))) / (1e-9 * ymax)
            fig["f_hess_var"] = max(np.abs(fhv[:, k] - (ph.prior_pair(kernel, theta, D, *pairs[k]) - quad[1 + k][1])).max() * sc[k] ** 2
                                    for k in range(len(pairs))) / 2.5e-9
            wl = w / ell ** 2
            fig["f_lap"] = np.abs(fl - quad[-1][0]).max() / wl.sum() / (1e-9 * ymax)
            fig["f_lap_var"] = np.abs(flv - (ph.prior_lap(kernel, theta, D, w) - quad[-1][1])).max() / \
                ((25.0 / 3.0) * (2.0 * np.sum(wl ** 2) + wl.sum() ** 2)) / 1e-10
        if row in ("rq", "mean", "noise"):
            nll, g = vn.nll_and_grad(variant, kernel, X, y, theta, v)
            nll2 = _objective(variant, kernel, X, y, theta, v)
            fig["nll"] = abs(nll - nll2) / (1e-9 * max(1.0, abs(nll)) * len(y))
            fd = np.empty_like(g)
            for i in range(len(theta)):
                h = 1e-5 * (max(abs(theta[i]), 1.0) if variant is vn.MEAN and i == D + 2 else theta[i])
                tp, tm = theta.copy(), theta.copy()
                tp[i] += h
                tm[i] -= h
                fd[i] = (_objective(variant, kernel, X, y, tp, v) - _objective(variant, kernel, X, y, tm, v)) / (2 * h)
            gfig = (np.abs(g - fd) / (1e-7 * np.abs(g) + 1e-8 * (np.abs(g).max() + 1))).max()
            print(f"MARGIN {row} D={D} N={len(y)} grad against central differences, in units of the gradient bound: {gfig:.3g}")
            # a difference quotient: the bound itself, not its tenth
            np.testing.assert_allclose(g, fd, rtol=1e-7, atol=1e-8 * (np.abs(g).max() + 1))
    print(f"MARGIN {row} D={D} N={len(y)} {kernel}", " ".join(f"{k}={v_:.3g}" for k, v_ in fig.items()), f"({time.perf_counter() - t0:.1f} s)")
    assert max(fig.values()) <= TENTH, fig


# ---- 3. the GPU module's checks trip
def restate(row, b, theta, kw, spoil=None):
    """What the engine returns for a batch of the GPU module, from the restatements written out around V = L^-1 (right-hand
    side) and A_GG.  ``spoil`` = t: in tile t, block row 1 of V is zeroed (rq, mean, noise: the prediction's V; grad: the
    gradient's; hess: the second derivatives' and the Laplacian's), or (cv) the largest fold's A_GG misses the pair of its
    first and last block."""
    T, D, kernel, H = b["T"], b["D"], b["kernel"], theta.shape[1]
    variant = vn.NOISE if row == "cv" else vs.CASE[row].variant
    sumP, sumN = int(b["pred_off"][-1]), int(b["obs_off"][-1])
    grad_on, spec = row == "grad" or bool(kw.get("pred_grad")), kw.get("pred_hess")
    pairs = ph.pairs(spec["dims"]) if spec else []
    r = SimpleNamespace(theta=theta.copy(), nll=np.zeros(T), grad=np.zeros((T, H)), status=np.full(T, 5, dtype=np.int32),
                        n_eval=np.zeros(T, dtype=np.int32), n_iter=np.zeros(T, dtype=np.int32), kernel_ms=0.0,
                        f_mean=np.zeros(sumP), f_var=np.zeros(sumP), y_var=np.zeros(sumP),
                        f_grad=np.zeros((sumP, D)) if grad_on else None, f_grad_var=np.zeros((sumP, D)) if grad_on else None,
                        f_hess=np.zeros((sumP, len(pairs))) if spec else None, f_hess_var=np.zeros((sumP, len(pairs))) if spec else None,
                        f_lap=np.zeros(sumP) if spec else None, f_lap_var=np.zeros(sumP) if spec else None, hess_pairs=pairs or None,
                        cv_mean=np.full(sumN, np.nan), cv_f_var=np.full(sumN, np.nan), cv_y_var=np.full(sumN, np.nan))
    for t in range(T):
        o, p = vs._tile(b, t)
        X, y, Xs, th = b["X"][o], b["y"][o], b["Xs"][p], theta[t]
        N, P, hit = len(y), len(Xs), spoil == t
        v = b["obs_var"][o] if "obs_var" in b else (np.zeros(N) if variant is vn.NOISE else None)
        r.nll[t], r.grad[t] = vn.nll_and_grad(variant, kernel, X, y, th, v)
        Lf = np.linalg.cholesky(vn.K_y(variant, kernel, X, th, v))
        c = float(th[D + 2]) if variant is vn.MEAN else 0.0
        z = solve_triangular(Lf, y - c, lower=True)

        def quad(W, prior, zeroed):
            V = solve_triangular(Lf, W, lower=True)
            if zeroed:
                V[16:32] = 0.0
            return V.T @ z, prior - np.sum(V * V, axis=0)

        f, fv = quad(vn.kernel_matrix(variant, kernel, X, Xs, th), th[D], hit and row in ("rq", "mean", "noise"))
        r.f_mean[p], r.f_var[p], r.y_var[p] = f + c, fv, fv + th[D + 1]
        if grad_on:
            G, prior = pg.cross_gradient(kernel, X, Xs, th), pg.prior_grad(kernel, th, P, D)[1]
            for a in range(D):
                r.f_grad[p, a], r.f_grad_var[p, a] = quad(G[a], prior[:, a], hit and row == "grad")
        if spec:
            Hm, w = ph.cross_hessian(kernel, X, Xs, th), np.asarray(spec["lap_weight"])
            for k, (a, c_) in enumerate(pairs):
                r.f_hess[p, k], r.f_hess_var[p, k] = quad(Hm[a, c_], ph.prior_pair(kernel, th, D, a, c_), hit)
            r.f_lap[p], r.f_lap_var[p] = quad(sum(w[a] * Hm[a, a] for a in range(D)), ph.prior_lap(kernel, th, D, w), hit)
        if row == "cv":
            lab = b["cv_fold"][o]
            M = solve_triangular(Lf, np.eye(N), lower=True)
            alpha = M.T @ z
            big = vs.deleted_folds(lab, N)[0]
            for fold in np.unique(lab):
                G = np.flatnonzero(lab == fold)
                A = M[:, G].T @ M[:, G]
                if hit and fold == big:
                    first, last = G // 16 == G[0] // 16, G // 16 == G[-1] // 16
                    A[np.ix_(first, last)] = 0.0
                    A[np.ix_(last, first)] = 0.0
                Cf = np.linalg.inv(A)
                r.cv_mean[o][G], r.cv_y_var[o][G], r.cv_f_var[o][G] = y[G] - Cf @ alpha[G], np.diag(Cf), np.diag(Cf) - th[D + 1]
    return r


@pytest.fixture
def memo(monkeypatch):
    for (mod, name), fn in vs.MEMO.items():
        monkeypatch.setattr(mod, name, fn)


@pytest.mark.parametrize("row", vs.ROWS)
def test_the_gpu_checks_trip_on_a_spoiled_restatement(memo, row):
    """The last tile of the 4-wave build at the row's largest D (656 rows at D = 3, 560 at D = 4), beside the 17-row tile."""
    D = vs.ROW_D[row][-1]
    b, theta = vs.inputs(row, D, "A")
    kw = vs.row_kw(row, D, "A")
    good = restate(row, b, theta, kw)
    for t in range(b["T"]):
        vs.check_row_tile(row, good, b, t, theta[t], kw, f"{row} restated")
    bad = restate(row, b, theta, kw, spoil=0)
    vs.check_row_tile(row, bad, b, 1, theta[1], kw, f"{row} spoiled, the other tile")
    with pytest.raises(AssertionError):
        vs.check_row_tile(row, bad, b, 0, theta[0], kw, f"{row} spoiled")
    if row in ("grad", "hess"):                              # ... and it is the derivative's own check that trips
        vs.check_tile(vs.CASE[row], bad, b, 0, theta[0], "the shared outputs are untouched")
        if row == "hess":
            vs.tg.check_grad_tile(bad, b, 0, theta[0], "the gradient beside it is untouched")
