"""Tiles that fail, as data, and the one check every failed-tile test uses.  No GPU is needed here:
tests/test_failed_tile_cpu.py proves the recipes and that the check trips, tests/test_gpu_failed_tile.py runs them.

Three recipes make a tile fail at a chosen row z (0-based):

  Z  an exactly zero pivot at row z, 1 <= z < N.  RBF, kernel variance 1, length scales 1, likelihood variance below the
     resolution of 1 (SN2_Z).  Rows 0 .. z-2 are isolated points on a line along coordinate 0, 40 length scales apart (every
     kernel value between two of them is exp(-800) = 0 exactly), rows z-1 .. N-1 are copies of one more such point, so
     K_y = diag(I, 1 1^T) exactly: pivot z-1 is 1 and pivot z is fma(-1, 1, 1) = 0 whichever block or panel border lies
     between the two rows.  The kernels' diag_step tests !(p > 0.0), and its reciprocal of 1 -- v_rcp plus one Newton step,
     fma(1, fma(-1, 1, 1), 1) -- is exactly 1, so no rounding stands between the recipe and the zero.  All coordinates are
     multiples of 40, centred on 0 and below 2^24 in magnitude: fp32 holds them exactly.
  Q  a NaN coordinate in row z, any kernel.  Pivots before z never read row z; pivot z is NaN and !(p > 0.0) catches it.  Neither
     the C ABI nor engine.py looks at X for finite values (gpsat_capi.cpp checks theta0, the bounds and obs_var only).
  Y  a NaN in y[z].  The factor succeeds and the objective is NaN.

What the kernels answer (gpsat_opt.h tile_out_finished, evaluate of gpsat_kernels.hip / gpsat_kernels_f64.hip): a failed factor
leaves nll = +inf inside the kernel, hence GPSAT_STATUS_NOT_PD (Z and Q); a NaN objective gives GPSAT_STATUS_NAN (Y).  Either
way nll and grad are NaN and n_iter is 0.  theta is theta0 with optimiser="none"; with an optimiser it is theta0 after one
trip through the parameter transform (the columns that are not trainable: theta0's bits).  n_eval is 0 with
optimiser="none" (no evaluation is ever counted there); with an optimiser it counts the evaluations that ran to their end,
so 0 for a failed factor and 1 for a NaN objective.
"""
import dataclasses
from collections import namedtuple

import numpy as np

from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult

NOT_PD, NAN, SKIPPED, NOT_OPTIMISED = 2, 3, 4, 5
SN2_Z = {"f64": 1e-300, "f32": 1e-12}                  # as test_gpu_cv_joint and test_gpu_parity make a tile singular
NP = {"f32": np.float32, "f64": np.float64}
KID = {"RBF": 0, "Matern12": 1, "Matern32": 2, "Matern52": 3, "RationalQuadratic": 0}      # what synthetic draws y from
STATUS_OF = {"Z": NOT_PD, "Q": NOT_PD, "Y": NAN}

# kind: "good", "empty", "Z", "Q", "Y", or "H" (the head of a Z tile: its rows in front of row z, which must factorise); z: the row
# that fails; seed: of everything drawn
Tile = namedtuple("Tile", "kind N P z seed", defaults=(None, 0))


@dataclasses.dataclass(frozen=True)
class Row:
    """One row of the fp64 table of gpsat_amd/variants.py (or the plain call with another kernel), as fit_predict_batch takes it."""
    name: str
    kernel: str = "RBF"
    kw: tuple = ()               # keywords of fit_predict_batch
    extra: float = None          # the row's own column of theta (alpha, c), the same in every tile
    noise: bool = False          # obs_var per row
    cv: bool = False             # fold labels arange(N) // 7 per tile

    def __repr__(self):
        return self.name


ROWS = {r.name: r for r in [
    Row("plain"), Row("matern32", "Matern32"), Row("matern52", "Matern52"),
    Row("full_cov", kw=(("full_cov", True),)),
    Row("rq", "RationalQuadratic", extra=1.5),
    Row("mean", kw=(("mean", "constant"),), extra=-0.7),
    Row("noise", noise=True),
    Row("cv", cv=True), Row("cv_joint", cv=True, kw=(("cv_joint", True),)),
    Row("pred_grad", kw=(("pred_grad", True),)),
    Row("pred_hess", kw=(("pred_hess", True),)),                                   # every coordinate and the Laplacian
    Row("pred_grad_hess", kw=(("pred_grad", True), ("pred_hess", True))),
]}
Q_ROWS = ("rq", "matern32", "matern52")            # kernels whose values do not underflow to 0: recipe Q places the failure


def good_theta(seed, D):
    """theta of a tile that succeeds: test_gpu_build_matrix._theta (length scales on the data's scale, sf2 / sn2 in [2, 4])."""
    from test_gpu_build_matrix import _theta
    return _theta(np.random.default_rng(seed), 1, D)[0]


def tile_z(N, z, D, P, seed, dtype="f64"):
    """Recipe Z: (X, y, Xs, theta)."""
    assert 1 <= z < N
    rng = np.random.default_rng(seed)
    pos = 40.0 * (np.arange(z) - z // 2)
    X = np.zeros((N, D))
    X[:z, 0] = pos
    X[z - 1:, 0] = pos[z - 1]
    assert np.abs(X).max() < 2.0 ** 24
    return X, rng.standard_normal(N), rng.uniform(-3.0, 3.0, (P, D)), np.array([1.0] * D + [1.0, SN2_Z[dtype]])


def tile_data(tile, D, kernel, dtype="f64"):
    """(X, y, Xs, theta without the row's own column) of one Tile."""
    if tile.kind == "Z":
        return tile_z(tile.N, tile.z, D, tile.P, tile.seed, dtype)
    if tile.kind == "H":
        X, y, Xs, th = tile_z(tile.N, tile.z, D, tile.P, tile.seed, dtype)
        return X[:tile.z], y[:tile.z], Xs, th
    N = 0 if tile.kind == "empty" else tile.N
    X, y, Xs, _ = syn.make_tile(tile.seed, N, tile.P, D, KID[kernel])
    if tile.kind == "Q":
        X[tile.z, 0] = np.nan
    if tile.kind == "Y":
        y[tile.z] = np.nan
    return X, y, Xs, good_theta(tile.seed, D)


def make(tiles, D, row, dtype="f64"):
    """The packed batch of ``tiles`` for ``row``: the arrays of fit_predict_batch, theta0 [T, H], ``failed`` (tile -> the status
    read above) and, where the row reads them, obs_var (0 in a Z tile: nothing may lift its pivot) and the fold labels."""
    parts = [tile_data(t, D, row.kernel, dtype) for t in tiles]
    Ns, Ps = [len(p[0]) for p in parts], [len(p[2]) for p in parts]
    th = np.array([np.concatenate([p[3], [] if row.extra is None else [row.extra]]) for p in parts])
    b = dict(T=len(tiles), D=D, dtype=dtype, row=row, tiles=list(tiles), theta0=th,
             obs_off=np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64), pred_off=np.concatenate([[0], np.cumsum(Ps)]).astype(np.int64),
             X=np.concatenate([p[0] for p in parts]).astype(NP[dtype]), y=np.concatenate([p[1] for p in parts]).astype(NP[dtype]),
             Xs=np.concatenate([p[2] for p in parts]).reshape(-1, D).astype(NP[dtype]),
             failed={i: STATUS_OF[t.kind] for i, t in enumerate(tiles) if t.kind in STATUS_OF})
    if row.noise:
        v = []
        for t, n in zip(tiles, Ns):
            rng = np.random.default_rng(t.seed + 77)
            u = rng.uniform(0.0, 0.3, n)
            u[rng.uniform(size=n) < 0.2] = 0.0
            v.append(np.zeros(n) if t.kind == "Z" else u)
        b["obs_var"] = np.concatenate(v)
    if row.cv:
        b["fold"] = np.concatenate([np.arange(n) // 7 for n in Ns]).astype(np.int32)
    return b


def subset(b, keep):
    """The batch of the tiles ``keep`` of ``b``, in that order."""
    return make([b["tiles"][t] for t in keep], b["D"], b["row"], b["dtype"])


def replicate(tiles, rep):
    """``tiles`` ``rep`` times over."""
    return [t for _ in range(rep) for t in tiles]


def call_kw(b):
    kw = dict(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=b["theta0"],
              kernel=b["row"].kernel, dtype=b["dtype"], **dict(b["row"].kw))
    if "obs_var" in b:
        kw["obs_var"] = b["obs_var"]
    if "fold" in b:
        kw["cv_fold"] = b["fold"]
    return kw


def run(e, b, **kw):
    return e.fit_predict_batch(**call_kw(b), **{"optimiser": "none", "want_grad": True, **kw})


def lengthscales_only(b):
    """``trainable`` that leaves the variances (and the row's own parameter) at theta0: a Z tile then fails at theta0 itself,
    K_y = diag(I, 1 1^T) whatever the transform's rounding does to a length scale of 1."""
    D, H = b["D"], b["theta0"].shape[1]
    return np.array([1] * D + [0] * (H - D), dtype=np.uint8)


# ---- the check
# Every field of BatchResult and the axis its elements run along: a tile's part of it is one slice of that axis.  None: not an
# output of a tile (offset tables, the column list of f_hess, timings).  A field that is missing here fails the check.
LAYOUT = {
    "theta": "tile", "nll": "tile", "status": "tile", "n_eval": "tile", "grad": "tile", "n_iter": "tile", "f_start": "tile",
    "f_mean": "pred", "f_var": "pred", "y_var": "pred", "f_grad": "pred", "f_grad_var": "pred",
    "f_hess": "pred", "f_hess_var": "pred", "f_lap": "pred", "f_lap_var": "pred",
    "f_cov": "cov",
    "cv_mean": "obs", "cv_f_var": "obs", "cv_y_var": "obs",
    "cv_lpd": "fold", "cv_theta": "fold", "cv_nll": "fold", "cv_status": "fold", "cv_n_eval": "fold", "cv_n_iter": "fold",
    "cv_n_obs": "fold", "cv_shift": "fold", "cv_label": "fold",
    "cov_off": None, "cv_fold_off": None, "hess_pairs": None, "kernel_ms": None, "total_ms": None,
}
NAN_AXES = ("pred", "cov", "obs", "fold")         # per point, per pair of points, per observation, per fold: NaN in a failed tile


def expected_counts(status, optimiser):
    """(n_eval, n_iter) of a tile that fails at theta0 (the module's docstring)."""
    return (1 if optimiser != "none" and status == NAN else 0), 0


def outputs(r):
    """The outputs a result carries, with their axes; an output without a layout is an error."""
    out = {}
    for f in dataclasses.fields(r):
        if getattr(r, f.name) is None:
            continue
        assert f.name in LAYOUT, f"{f.name}: an output of BatchResult that failed_tile_cases.LAYOUT does not know"
        if LAYOUT[f.name] is not None:
            out[f.name] = LAYOUT[f.name]
    return out


def _offsets(obs_off, pred_off, r):
    T = len(obs_off) - 1
    off = {"tile": np.arange(T + 1), "pred": np.asarray(pred_off), "obs": np.asarray(obs_off)}
    if r.cov_off is not None:
        off["cov"] = np.asarray(r.cov_off)
    if r.cv_fold_off is not None:
        off["fold"] = np.asarray(r.cv_fold_off)
    return off


def _part(r, name, off, axis, t):
    return np.asarray(getattr(r, name))[int(off[axis][t]):int(off[axis][t + 1])]


def check_failed_batch(r, batch, failed, good_alone, optimiser="none", trainable=None):
    """``r``: the result of ``batch``; ``failed``: tile -> expected status; ``good_alone``: the result of subset(batch, the other
    tiles).  A failed tile has its status, NaN in every element of every per-point, per-observation and per-fold output, of
    its block of f_cov, of nll and of grad, and the theta / n_eval / n_iter of the module's docstring; every other tile has,
    in every output, the bytes it has in ``good_alone``.  An AssertionError names the tile and the output."""
    T = batch["T"]
    keep = [t for t in range(T) if t not in failed]
    names = outputs(r)
    assert set(outputs(good_alone)) == set(names), (sorted(outputs(good_alone)), sorted(names))
    off = _offsets(batch["obs_off"], batch["pred_off"], r)
    Ns, Ps = np.diff(batch["obs_off"])[keep], np.diff(batch["pred_off"])[keep]
    off1 = _offsets(np.concatenate([[0], np.cumsum(Ns)]), np.concatenate([[0], np.cumsum(Ps)]), good_alone)
    for name, axis in names.items():
        assert len(np.asarray(getattr(r, name))) == off[axis][-1], f"{name}: {len(getattr(r, name))} entries, {off[axis][-1]} expected"
    for t, want in failed.items():
        assert r.status[t] == want, f"tile {t}: status {r.status[t]}, {want} expected"
        for name, axis in names.items():
            if axis in NAN_AXES or name in ("nll", "grad"):
                part = _part(r, name, off, axis, t)
                assert np.isnan(part).all(), f"tile {t}: {name} holds {int((~np.isnan(part)).sum())} values that are not NaN in a failed tile"
        th0 = batch["theta0"][t]
        moved = np.zeros(len(th0), dtype=bool) if optimiser == "none" else np.ones(len(th0), dtype=bool) if trainable is None \
            else np.asarray(trainable, dtype=bool)
        fixed = ~moved
        assert r.theta[t][fixed].tobytes() == th0[fixed].tobytes(), f"tile {t}: theta {r.theta[t]} is not theta0 {th0}"
        np.testing.assert_allclose(r.theta[t], th0, rtol=1e-14, atol=0, err_msg=f"tile {t}: theta")      # the transform and back
        n_eval, n_iter = expected_counts(want, optimiser)
        assert r.n_eval[t] == n_eval, f"tile {t}: n_eval {r.n_eval[t]}, {n_eval} expected"
        assert r.n_iter[t] == n_iter, f"tile {t}: n_iter {r.n_iter[t]}, {n_iter} expected"
    for k, t in enumerate(keep):
        for name, axis in names.items():
            got, alone = _part(r, name, off, axis, t), _part(good_alone, name, off1, axis, k)
            assert got.dtype == alone.dtype and got.tobytes() == alone.tobytes(), \
                f"tile {t}: {name} differs from the bytes of the batch without the failed tiles"
    if r.hess_pairs is not None:
        assert r.hess_pairs == good_alone.hess_pairs


def statuses(r):
    """One line for the log: how many tiles ended with which status."""
    st, n = np.unique(np.asarray(r.status), return_counts=True)
    return ", ".join(f"status {int(s)} x {int(c)}" for s, c in zip(st, n))
