"""GPU: gpsat_sgpr.hip at the edges of its own code -- every boundary of M, N and P, prediction chunks, empty / failed / NaN
tiles and their neighbours, what a fit leaves behind, Adam, device-resident inputs -- against the numpy restatement
(sgpr_numpy.py) through Engine.sgpr_fit_predict_batch.

The inputs come from tests/sgpr_edge_cases.py: inducing points on a jittered lattice, where cond(Kuu) <= 1e3
(tests/test_sgpr_edges_cpu.py proves it without a GPU, and every comparison here asserts it again), so the bounds of
tests/test_gpu_sgpr.py, 1e-9 + 64 eps cond(Kuu) relative, are 1e-9 relative in effect: one dropped row or column of Kuf
moves the ELBO of the smallest tile here by far more."""
import numpy as np
import pytest

import sgpr_edge_cases as ec
import sgpr_numpy as sn

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "nll", "grad", "status", "n_eval")
PRED = ("f_mean", "f_var", "y_var")


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _refs(kid, tiles, th, jitter=sn.JITTER):
    return [ec.reference(kid, t, th, True, jitter) for t in tiles]


# ---------------------------------------------------------------------------------------------------------------------
# 1. fixed theta: every boundary of M, N and P
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_every_boundary_of_m_n_p_matches_numpy(eng, kid, D):
    """One ragged, unsorted batch of 11 tiles per (kernel, D) (sgpr_edge_cases.boundary_shapes): across the 16 batches every
    M in {2, 7, 8, 9, 15, 17, 31, 32, 33, 47, 49, 64, 65, 96, 97, 255, 257, 511, 512, 513, 600} meets every N in {1, 2, 3,
    5, M - 1, M, M + 1, ~2000} and every P in {0, 1, 7, 63, 64, 65}.  Run with the gradient (the G = true instantiation of
    the row pass) and again without (G = false): ELBO and predictions are held to the same bounds in both."""
    tiles, th = ec.boundary_batch(kid, D)
    refs = _refs(kid, tiles, th)
    ec.check_fixed(eng, kid, D, tiles, th, want_grad=True, refs=refs, cond_max=ec.COND_MAX)
    r = ec.check_fixed(eng, kid, D, tiles, th, want_grad=False, refs=refs, cond_max=ec.COND_MAX)
    assert r.grad is None


# ---------------------------------------------------------------------------------------------------------------------
# 2. prediction chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kid", [0, 1, 2, 3])
def test_prediction_chunks_match_numpy(eng, kid):
    """predict() serves 512 points per round: P in {0, 1, 511, 512, 513, 1100} at M = 97 and at M = 1, tiles without
    prediction points between the others; every f*, f*_var and y_var against sgpr_numpy.predict."""
    tiles, th = ec.chunk_batch(kid)
    r = ec.check_fixed(eng, kid, 2, tiles, th, want_grad=False, cond_max=ec.COND_MAX)
    assert len(r.f_mean) == sum(len(t[3]) for t in tiles) == 2 * sum(ec.CHUNK_PS)
    assert np.isfinite(r.f_mean).all() and np.isfinite(r.f_var).all() and np.isfinite(r.y_var).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. empty, failed and NaN tiles, and their neighbours
# ---------------------------------------------------------------------------------------------------------------------
def _same_bytes(r, t, pa, pb, r2, t2, qa, qb, what):
    for k in FIELDS:
        assert getattr(r, k)[t].tobytes() == getattr(r2, k)[t2].tobytes(), (what, k, t)
    for k in PRED:
        assert getattr(r, k)[pa:pb].tobytes() == getattr(r2, k)[qa:qb].tobytes(), (what, k, t)


def _check_special(r, pk, tiles, th, special):
    for t, kind in special.items():
        a, b = pk["pred_off"][t], pk["pred_off"][t + 1]
        assert b > a
        if kind == "empty":
            # gpsat_opt.h, tile_out_empty + tile_predict_prior: status 4, no evaluation, theta0 handed back, objective and
            # gradient 0, and the prior at theta0 as the prediction
            assert r.status[t] == 4 and r.n_eval[t] == 0
            assert r.theta[t].tobytes() == th.tobytes() and r.nll[t] == 0.0 and (r.grad[t] == 0.0).all()
            assert (r.f_mean[a:b] == 0.0).all() and (r.f_var[a:b] == th[-2]).all() and (r.y_var[a:b] == th[-2] + th[-1]).all()
        else:
            assert r.status[t] in (2, 3), (t, kind, r.status[t])
            assert np.isnan(r.nll[t]) and np.isnan(r.grad[t]).all(), (t, kind)
            for k in PRED:
                assert np.isnan(getattr(r, k)[a:b]).all(), (t, kind, k)


@pytest.fixture(scope="module")
def tiny():
    tiles, th, special = ec.tiny_batch()
    healthy = [t for t in range(len(tiles)) if t not in special]
    return tiles, th, special, healthy


@pytest.mark.parametrize("optimiser", ["none", "lbfgs"])
def test_failed_and_empty_tiles_leave_their_neighbours_alone(eng, tiny, optimiser):
    """600 tiny tiles, more than the GPU has CUs, so every workgroup serves several from the same workspace and the same
    LDS flags; 12 of them have no observations, a NaN observation or a NaN coordinate.  Those report what the header
    states; every healthy tile returns the bytes it returns in the same batch without the 12 (and, at fixed theta,
    matches numpy)."""
    tiles, th, special, healthy = tiny
    kw = dict(D=ec.TINY_D, kernel=ec.TINY_KID, theta0=th, want_grad=True, optimiser=optimiser)
    if optimiser == "lbfgs":
        kw["max_iter"] = 10
    pk = ec.pack(tiles)
    r = eng.sgpr_fit_predict_batch(**kw, **pk)
    _check_special(r, pk, tiles, th, special)
    pk2 = ec.pack([tiles[t] for t in healthy])
    r2 = eng.sgpr_fit_predict_batch(**kw, **pk2)
    assert np.isfinite(r2.nll).all() and np.isfinite(r2.f_mean).all()
    assert (r2.status == 5).all() if optimiser == "none" else np.isin(r2.status, (0, 1, 6)).all(), np.unique(r2.status)
    if optimiser == "lbfgs":
        assert (r2.n_eval > 1).all()
    for t2, t in enumerate(healthy):
        _same_bytes(r, t, pk["pred_off"][t], pk["pred_off"][t + 1], r2, t2, pk2["pred_off"][t2], pk2["pred_off"][t2 + 1],
                    optimiser)
    if optimiser == "none":
        for t in healthy:
            assert r.status[t] == 5
            ec.check_tile(r, t, pk["pred_off"], ec.TINY_KID, tiles[t], th, cond_max=ec.COND_MAX)


def test_exact_zero_pivot_reports_not_pd(eng):
    """RBF, kernel variance exactly 1, Z[1] == Z[0], jitter 1e-30: K00 = 1 + 1e-30 = 1, L10 = 1, the pivot is 1 - 1 = 0 and
    chol() must refuse it (!(0 > 0)): GPSAT_STATUS_NOT_PD with NaN objective, gradient and predictions.  The other tiles
    of the call match numpy at the same jitter."""
    tiles, th, bad = ec.zero_pivot_batch()
    rest = [t for t in range(len(tiles)) if t != bad]
    r = ec.check_fixed(eng, 0, 2, tiles, th, jitter=ec.ZERO_PIVOT_JITTER, only=rest, cond_max=ec.COND_MAX)
    pk = ec.pack(tiles)
    a, b = pk["pred_off"][bad], pk["pred_off"][bad + 1]
    assert r.status[bad] == 2
    assert np.isnan(r.nll[bad]) and np.isnan(r.grad[bad]).all()
    assert b > a and all(np.isnan(getattr(r, k)[a:b]).all() for k in PRED)


# ---------------------------------------------------------------------------------------------------------------------
# 4. what a fit leaves behind
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_ls", [0, 1, 2])
def test_results_after_a_fit_belong_to_the_returned_theta(eng, max_ls):
    """L-BFGS, 30 iterations at most, on 12 ragged tiles (M 7 .. 97, P 0 .. 65) inside a box on the length scales and the
    kernel variance: at every tile's returned theta, -nll, grad and the predictions are numpy's at that theta.  That is
    the check that the last evaluation, and the factors Li, LB and c that predict() reads, are those of the accepted
    parameters and not of a rejected line-search trial.  max_ls = 0 is the default of 20 evaluations per line search;
    with 1 or 2 a search gives up early, the optimiser goes back to the accepted point, and the factors in the workspace
    are those of the rejected trial until the final evaluation replaces them."""
    tiles, th0 = ec.fit_batch()
    pk = ec.pack(tiles)
    r = eng.sgpr_fit_predict_batch(D=ec.FIT_D, kernel=ec.FIT_KID, theta0=th0, lo=ec.FIT_LO, hi=ec.FIT_HI, optimiser="lbfgs",
                                   max_iter=30, max_ls=max_ls, want_grad=True, **pk)
    assert np.isin(r.status, (0, 1, 6)).all(), r.status
    if max_ls == 0:
        assert (r.n_eval > 2).all() and (r.n_iter >= 1).all()
    if max_ls == 1:
        assert (r.status == 6).any(), r.status      # some search did give up, or this case shows nothing (seen: 10 of 12)
    for t, tile in enumerate(tiles):
        th = r.theta[t]
        assert np.all(th[:3] > ec.FIT_LO[:3]) and np.all(th[:3] < ec.FIT_HI[:3]) and th[3] > 1e-6
        if max_ls == 0:
            assert np.max(np.abs(th - th0)) > 1e-3      # the fit moved: theta0's factors would not pass below
        ec.check_tile(r, t, pk["pred_off"], ec.FIT_KID, tile, th, cond_max=ec.COND_MAX)


@pytest.mark.parametrize("which", ["box", "fixed"])
def test_converged_fits_with_a_box_and_with_fixed_parameters_match_scipy(eng, which):
    """test_gpu_sgpr.py::test_converged_fits_match_scipy, its tolerances and preconditions, through the optimiser options it
    leaves out: a finite box (sigmoid transform) that is inactive at the optimum, and `trainable` fixing the likelihood
    variance and one length scale, which come back bit-equal to theta0."""
    c = ec.converged_case(which)
    X, y, Z, th0, D = c["X"], c["y"], c["Z"], c["theta0"], c["D"]
    r = eng.sgpr_fit_predict_batch(D=D, obs_off=[0, len(X)], X=X, y=y, pred_off=[0, 0], Xs=np.zeros((0, D)), z_off=[0, len(Z)],
                                   Z=Z, theta0=th0, lo=c["lo"], hi=c["hi"], trainable=c["trainable"], kernel=c["kid"],
                                   optimiser="lbfgs", max_iter=2000, ftol=1e-15, gtol=1e-9, want_grad=True)
    assert r.status[0] in (0, 6), r.status
    ctr = X.mean(0)
    th_s, el_s, res = sn.fit_scipy(c["kid"], X - ctr, y, Z - ctr, th0, c["lo"], c["hi"], c["trainable"])
    assert np.max(np.abs(res.jac)) <= 1e-5, res.message
    assert ec.cond_kuu(c["kid"], Z - ctr, th_s) < 1e5
    np.testing.assert_allclose(r.theta[0], th_s, rtol=1e-5)
    assert abs(-r.nll[0] - el_s) <= 1e-8 * abs(el_s)
    if c["trainable"] is not None:
        fixed = ~c["trainable"]
        assert r.theta[0][fixed].tobytes() == th0[fixed].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. Adam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "fixed"])
def test_adam_end_point_matches_numpy_adam(eng, which):
    """20 steps at lr 0.1, and 13 steps at lr 0.03 with the likelihood variance fixed, against oracle.adam_minimise on
    u -> (-ELBO, -dELBO/dtheta dtheta/du) built from sgpr_numpy (sgpr_edge_cases.adam_numpy).  The bounds are those of the
    exact-GP fp64 Adam test (tests/test_gpu_adam.py): theta to 1e-8 relative, the objective to 1e-9.  A wrong step moves
    u by about lr * 1e-2."""
    kid, D, tiles, th0, tr, steps, lr = ec.adam_batch(which)
    pk = ec.pack(tiles)
    r = eng.sgpr_fit_predict_batch(D=D, kernel=kid, theta0=th0, trainable=tr, optimiser="adam", max_iter=steps, adam_lr=lr, **pk)
    assert (r.status == 1).all() and (r.n_eval == steps + 1).all() and (r.n_iter == steps).all()
    for t, tile in enumerate(tiles):
        th, f, ok = ec.adam_numpy(kid, tile, th0, tr, steps, lr)
        assert ok and ec.cond_kuu(kid, ec.centred(tile)[2], th) <= ec.COND_MAX
        print(f"adam {which} tile {t}: theta rel {np.max(np.abs(r.theta[t] - th) / np.abs(th)):.3e} "
              f"objective {abs(r.nll[t] - f) / max(1.0, abs(f)):.3e}")
        assert r.theta[t][~tr].tobytes() == th0[~tr].tobytes()
        np.testing.assert_allclose(r.theta[t], th, rtol=1e-8, atol=1e-12)
        assert abs(r.nll[t] - f) <= 1e-9 * max(1.0, abs(f))


# ---------------------------------------------------------------------------------------------------------------------
# 6. device-resident inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimiser", ["none", "lbfgs"])
def test_device_tensors_give_the_bytes_of_host_arrays(eng, optimiser):
    """A ragged batch centred on the host (so that the host path's own centring subtracts exactly 0), once as numpy arrays
    and once as torch device tensors, which the engine takes as they are: the same bytes in every field."""
    import torch
    kid, D, pk, th0 = ec.centred_exact_batch()
    kw = dict(D=D, kernel=kid, theta0=th0, optimiser=optimiser, max_iter=12, want_grad=True,
              obs_off=pk["obs_off"], pred_off=pk["pred_off"], z_off=pk["z_off"])
    rh = eng.sgpr_fit_predict_batch(X=pk["X"], y=pk["y"], Xs=pk["Xs"], Z=pk["Z"], **kw)
    dev = torch.device("cuda", 0)
    rd = eng.sgpr_fit_predict_batch(**{k: torch.from_numpy(pk[k]).to(dev) for k in ("X", "y", "Xs", "Z")}, **kw)
    assert np.isfinite(rh.nll).all() and len(rh.f_mean) == pk["pred_off"][-1]
    for k in FIELDS + ("n_iter",):
        assert getattr(rh, k).tobytes() == getattr(rd, k).tobytes(), k
    for k in PRED:
        assert isinstance(getattr(rd, k), torch.Tensor)
        assert getattr(rh, k).tobytes() == getattr(rd, k).cpu().numpy().tobytes(), k
