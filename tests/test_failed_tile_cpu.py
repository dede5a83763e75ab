"""CPU: the failed-tile recipes of tests/failed_tile_cases.py are what they claim, and its check trips on every way a kernel could
break the contract.  tests/test_gpu_failed_tile.py runs the recipes on the device."""
import dataclasses

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import failed_tile_cases as ft
import variant_numpy as vn
from failed_tile_cases import Tile
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go

# every (N, z, dtype) a GPU test places recipe Z at
Z_F64 = [(200, z) for z in (1, 15, 16, 17, 63, 64, 65, 127, 128, 191, 192, 199)] + [(1100, z) for z in (1, 64, 1099)] + [(20, 1)]
Z_F32 = [(200, z) for z in (1, 31, 32, 33, 127, 128, 199)]
Z_CASES = [(N, z, "f64") for N, z in Z_F64] + [(N, z, "f32") for N, z in Z_F32]


def _fails(K):
    try:
        np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return True
    return False


@pytest.mark.parametrize("N,z,dtype", Z_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("D", [2, 3])
def test_recipe_z_is_an_exact_zero_pivot_at_row_z(N, z, dtype, D):
    """K_y = diag(I, 1 1^T) to the last bit, in the precision of the call: the leading z x z minor factorises, the next does
    not.  float32: inputs and K_y rounded to it, as the fp32 kernels hold them."""
    X, y, Xs, th = ft.tile_z(N, z, D, 5, 1, dtype)
    np_dt = ft.NP[dtype]
    Xr = X.astype(np_dt)
    assert (Xr.astype(np.float64) == X).all() and (X % 40.0 == 0.0).all()
    K = go.kernel_matrix(0, Xr.astype(np.float64), Xr.astype(np.float64), th[:D], th[D]).astype(np_dt)
    K = K + np.eye(N, dtype=np_dt) * np_dt(th[D + 1])
    assert K.dtype == np_dt
    blk = np.zeros((N, N), dtype=bool)
    blk[z - 1:, z - 1:] = True
    blk[np.arange(N), np.arange(N)] = True
    assert (K[blk] == 1.0).all() and (K[~blk] == 0.0).all()
    np.linalg.cholesky(K[:z, :z])
    assert _fails(K[:z + 1, :z + 1])
    assert np.isfinite(y).all() and np.isfinite(Xs).all() and th[D + 1] > 0.0


@pytest.mark.parametrize("row", ft.Q_ROWS)
@pytest.mark.parametrize("z", [1, 15, 16, 17, 63, 64, 65, 127, 128, 191, 192, 199])
def test_recipe_q_fails_at_row_z_and_not_before(row, z):
    D, row = 2, ft.ROWS[row]
    X, y, Xs, th = ft.tile_data(Tile("Q", 200, 17, z, 300 + z), D, row.kernel)
    assert np.isnan(X[z, 0]) and np.isfinite(np.delete(X, z, axis=0)).all() and np.isfinite(y).all()
    theta = np.concatenate([th, [] if row.extra is None else [row.extra]])
    K = vn.K_y(vn.RQ if row.name == "rq" else vn.NOISE, row.kernel, X, theta, None if row.name == "rq" else np.zeros(200))
    assert np.isfinite(K[:z, :z]).all() and np.isnan(K[z, z])
    np.linalg.cholesky(K[:z, :z])
    assert not (K[z, z] > 0.0)                                # what diag_step tests


@pytest.mark.parametrize("row", ["plain", "rq", "matern32", "matern52"])
@pytest.mark.parametrize("z", [0, 100, 199])
def test_recipe_y_factorises_and_has_a_nan_objective(row, z):
    D, row = 2, ft.ROWS[row]
    X, y, Xs, th = ft.tile_data(Tile("Y", 200, 17, z, 400 + z), D, row.kernel)
    assert np.isnan(y[z]) and np.isfinite(np.delete(y, z)).all() and np.isfinite(X).all()
    if row.name == "rq":
        K = vn.K_y(vn.RQ, row.kernel, X, np.concatenate([th, [row.extra]]))
    else:
        K = go.kernel_matrix(ft.KID[row.kernel], X, X, th[:D], th[D]) + th[D + 1] * np.eye(200)
    # the objective of gp_oracle.nll_and_grad, whose own triangular solve refuses a NaN before it computes
    L = np.linalg.cholesky(K)
    zz = solve_triangular(L, y, lower=True, check_finite=False)
    nll = 0.5 * zz @ zz + np.log(np.diag(L)).sum() + 0.5 * 200 * np.log(2 * np.pi)
    assert np.isfinite(L).all() and np.isfinite(zz[:z]).all() and np.isnan(nll)


def test_statuses_are_the_headers():
    from gpsat_amd import _lib as L
    assert [L.STATUS[s] for s in (ft.NOT_PD, ft.NAN, ft.SKIPPED, ft.NOT_OPTIMISED)] == ["not_pd", "nan", "skipped", "not_optimised"]
    assert ft.expected_counts(ft.NOT_PD, "none") == (0, 0) and ft.expected_counts(ft.NAN, "none") == (0, 0)
    assert ft.expected_counts(ft.NOT_PD, "lbfgs") == (0, 0) and ft.expected_counts(ft.NAN, "lbfgs") == (1, 0)


def test_every_field_of_the_result_has_a_layout():
    """A new output of BatchResult has to be given an axis before check_failed_batch runs again."""
    assert {f.name for f in dataclasses.fields(BatchResult)} == set(ft.LAYOUT)


# ---- the check trips
TILES = [Tile("good", 40, 5, seed=1), Tile("Z", 20, 3, 1, 2), Tile("good", 9, 4, seed=3), Tile("empty", 0, 2, seed=4),
         Tile("Y", 30, 6, 7, 5), Tile("good", 40, 5, seed=1)]
FAMILIES = {"plain": ["f_mean", "f_var", "y_var", "nll", "grad"], "full_cov": ["f_cov"], "pred_grad": ["f_grad", "f_grad_var"],
            "pred_grad_hess": ["f_grad", "f_grad_var", "f_hess", "f_hess_var", "f_lap", "f_lap_var"],
            "cv_joint": ["cv_mean", "cv_f_var", "cv_y_var", "cv_lpd"]}


def fake_result(b):
    """A result that obeys the contract: every tile's outputs are drawn from its own seed, a failed tile's are NaN."""
    D, H, T = b["D"], b["theta0"].shape[1], b["T"]
    kw = dict(b["row"].kw)
    Ns, Ps = np.diff(b["obs_off"]), np.diff(b["pred_off"])
    m = D * (D + 1) // 2
    width = {"f_mean": 1, "f_var": 1, "y_var": 1}
    if kw.get("pred_grad"):
        width.update(f_grad=D, f_grad_var=D)
    if kw.get("pred_hess"):
        width.update(f_hess=m, f_hess_var=m, f_lap=1, f_lap_var=1)
    per_tile = {k: [] for k in ("theta", "nll", "grad", "status", "n_eval", "n_iter", "f_cov", "cv_mean", "cv_f_var", "cv_y_var", "cv_lpd", *width)}
    folds = []
    for t, tile in enumerate(b["tiles"]):
        rng = np.random.default_rng(tile.seed)
        bad = t in b["failed"]
        draw = (lambda *s: np.full(s, np.nan)) if bad else (lambda *s: rng.standard_normal(s))
        per_tile["theta"].append(b["theta0"][t])
        per_tile["nll"].append(draw(1))
        per_tile["grad"].append(draw(1, H))
        per_tile["status"].append(b["failed"].get(t, 4 if Ns[t] == 0 else 5))
        per_tile["n_eval"].append(0)
        per_tile["n_iter"].append(0)
        for k, w in width.items():
            per_tile[k].append(draw(Ps[t], w) if w > 1 or k in ("f_grad", "f_hess") else draw(Ps[t]))
        per_tile["f_cov"].append(draw(Ps[t] * Ps[t]))
        for k in ("cv_mean", "cv_f_var", "cv_y_var"):
            per_tile[k].append(draw(Ns[t]))
        folds.append(-(-int(Ns[t]) // 7))
        per_tile["cv_lpd"].append(draw(folds[-1]))
    cat = {k: np.concatenate(v) if np.ndim(v[0]) else np.array(v) for k, v in per_tile.items()}
    out = dict(theta=np.array(per_tile["theta"]), nll=cat["nll"], grad=cat["grad"], status=cat["status"].astype(np.int32),
               n_eval=cat["n_eval"].astype(np.int32), n_iter=cat["n_iter"].astype(np.int32), **{k: cat[k] for k in width})
    if kw.get("full_cov"):
        out.update(f_cov=cat["f_cov"], cov_off=np.concatenate([[0], np.cumsum(Ps * Ps)]))
    if b["row"].cv:
        out.update(cv_mean=cat["cv_mean"], cv_f_var=cat["cv_f_var"], cv_y_var=cat["cv_y_var"])
        if kw.get("cv_joint"):
            out.update(cv_lpd=cat["cv_lpd"], cv_fold_off=np.concatenate([[0], np.cumsum(folds)]))
    if kw.get("pred_hess"):
        out["hess_pairs"] = [(a, c) for a in range(D) for c in range(a, D)]
    return BatchResult(**out)


def _pair(row):
    b = ft.make(TILES, 2, ft.ROWS[row])
    keep = [t for t in range(b["T"]) if t not in b["failed"]]
    return b, fake_result(b), fake_result(ft.subset(b, keep))


@pytest.mark.parametrize("row", sorted(FAMILIES))
def test_the_check_passes_a_result_that_obeys_the_contract(row):
    b, r, alone = _pair(row)
    assert b["failed"] == {1: ft.NOT_PD, 4: ft.NAN}
    for name in FAMILIES[row]:
        assert name in ft.outputs(r)
    ft.check_failed_batch(r, b, b["failed"], alone)
    assert ft.statuses(r) == "status 2 x 1, status 3 x 1, status 4 x 1, status 5 x 3"


@pytest.mark.parametrize("row,name", [(row, name) for row in sorted(FAMILIES) for name in FAMILIES[row]])
@pytest.mark.parametrize("t", [1, 4])
def test_one_finite_value_in_a_nan_slot_trips_the_check(row, name, t):
    b, r, alone = _pair(row)
    axis = ft.LAYOUT[name]
    off = ft._offsets(b["obs_off"], b["pred_off"], r)
    a, e = int(off[axis][t]), int(off[axis][t + 1])
    v = getattr(r, name)
    if name == "f_cov":
        P = int(b["pred_off"][t + 1] - b["pred_off"][t])
        v[a + 1 * P + 2] = 0.25                                 # off the diagonal
    elif name == "f_hess_var":
        v[e - 1, -1] = 0.25                                     # the last element of the slice
    else:
        v[a] = 0.25                                             # the first
    with pytest.raises(AssertionError, match=rf"tile {t}: {name} "):
        ft.check_failed_batch(r, b, b["failed"], alone)


def test_a_wrong_status_trips_the_check():
    for t, wrong in ((1, ft.NAN), (4, ft.NOT_PD), (1, 5)):
        b, r, alone = _pair("plain")
        r.status[t] = wrong
        with pytest.raises(AssertionError, match=rf"tile {t}: status"):
            ft.check_failed_batch(r, b, b["failed"], alone)
    for field, msg in (("n_eval", "n_eval"), ("n_iter", "n_iter")):
        b, r, alone = _pair("plain")
        getattr(r, field)[4] = 1
        with pytest.raises(AssertionError, match=rf"tile 4: {msg}"):
            ft.check_failed_batch(r, b, b["failed"], alone)
    b, r, alone = _pair("plain")
    r.theta[1, 0] = np.nextafter(r.theta[1, 0], 2.0)
    with pytest.raises(AssertionError, match="tile 1: theta"):
        ft.check_failed_batch(r, b, b["failed"], alone)


@pytest.mark.parametrize("row,name", [(row, name) for row in sorted(FAMILIES) for name in FAMILIES[row]] + [("plain", "theta"), ("plain", "status")])
def test_one_changed_byte_in_a_neighbour_trips_the_check(row, name):
    """The last element of the tile in front of a failed one and the first of the tile behind it."""
    for t, last in ((0, True), (2, False), (3, True)):
        b, r, alone = _pair(row)
        axis = ft.LAYOUT[name]
        off = ft._offsets(b["obs_off"], b["pred_off"], r)
        a, e = int(off[axis][t]), int(off[axis][t + 1])
        if e == a:
            continue
        v = np.asarray(getattr(r, name))
        raw = v.reshape(-1).view(np.uint8)
        item = v.itemsize * (v.size // len(v))
        raw[(e * item - 1) if last else a * item] ^= 1          # one bit of one byte
        with pytest.raises(AssertionError, match=rf"tile {t}: {name} differs"):
            ft.check_failed_batch(r, b, b["failed"], alone)


def test_an_output_without_a_layout_trips_the_check():
    b, r, alone = _pair("plain")

    @dataclasses.dataclass
    class More(BatchResult):
        f_new: object = None
    more = More(**{f.name: getattr(r, f.name) for f in dataclasses.fields(r)}, f_new=np.zeros(3))
    with pytest.raises(AssertionError, match="f_new"):
        ft.check_failed_batch(more, b, b["failed"], alone)
