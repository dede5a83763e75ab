"""GPU: the six variant rows of the fp64 tile kernel -- rq, mean, noise, cv, grad, hess -- at the sizes only the plain row has
been run at (tests/test_gpu_build_matrix.py::test_fp64_builds_and_teams_match_oracle): the last tile of the 4-wave build, the
first of the 8-wave build and the largest tile the ABI accepts, gpsat_max_tile_obs.  run_tiles gives every variant one
workgroup per tile, so the large tiles here run the one-workgroup 8-wave path with the longest k-loops, the largest workspace
stride and, above 224 blocks, the second formula of xvec_blocks.  Then the derivative rows at the numerical edges the plain row
is held to (duplicated inputs, inputs one fp32 ulp apart, length scales of 1e-10 and 1.2e4).

No bound is new.  Every output is held to its row's restatement by its row's check, imported from the row's own test module:
variant_cases.check_tile (objective 1e-9 max(1, |nll|) N, gradient rtol 1e-7 with atol 1e-8 (max|g| + 1), mean 1e-9 max(|y|max, 1),
variances 1e-10), test_gpu_pred_grad.check_grad_tile (l_a |.| <= 1e-9 max(|y|max, 1), l_a^2 |.| <= 3e-10),
test_gpu_pred_hess.check_hess_tile (l_a l_b |.| <= 1e-9 max(|y|max, 1), l_a^2 l_b^2 |.| <= 2.5e-9, Laplacian 1e-9 max(|y|max, 1) S and
1e-10 (25/3) (2 sum wl^2 + S^2)) and test_gpu_cv._check (mean 1e-9 max(|y|max, 1), variances 1e-10, y_var - f_var = sn2 to 1e-12).
tests/test_variant_sizes_cpu.py holds the restatements themselves, at these inputs, to a tenth of each of those bounds
against a second fp64 route, and pins the size ladder.

Every tile prints its errors in units of their bounds (a line starting with SIZES) before it is held to them; DESIGN.md
section 31 records the largest.
"""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest

import cv_numpy as cvn
import pred_grad_numpy as pg
import pred_hess_numpy as ph
import test_gpu_build_matrix as bm
import test_gpu_pred_grad as tg
import test_gpu_pred_hess as th_
import variant_numpy as vn
from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from test_gpu_cv import _check as check_cv_deletion
from variant_cases import FIELDS, MEAN, NOISE, RQ, check_tile, eng, eng8, run  # noqa: F401 (eng, eng8: the fixtures)

pytestmark = pytest.mark.gpu

ROWS = ("rq", "mean", "noise", "cv", "grad", "hess")
ROW_D = {"rq": (1, 2, 3), "mean": (1, 2, 3), "noise": (1, 2, 3, 4), "cv": (1, 2, 3, 4), "grad": (1, 2, 3, 4), "hess": (1, 2, 3, 4)}
CASE = {"rq": RQ, "mean": MEAN, "noise": NOISE, "grad": tg.GRAD, "hess": th_.HESS}
GRAD_KERNEL = {1: "Matern32", 2: "RBF", 3: "Matern52", 4: "Matern32"}
HESS_KERNEL = {1: "Matern52", 2: "RBF", 3: "Matern52", 4: "RBF"}
ROW_AND_D = [(row, D) for row in ROWS for D in ROW_D[row]]
CV_FIELDS = ("cv_mean", "cv_f_var", "cv_y_var")
PER_ROW = set(CV_FIELDS)
PER_POINT = set(th_.PER_POINT)
N_DELETED = 6                                              # folds checked by deletion: the largest and five drawn by seed


def ladder(D):
    """(nd4, Nmax): the last tile of the 4-wave build and the largest tile the ABI accepts."""
    return 16 * bm.D4_NB[D], L.max_tile_obs("f64", D)


def kernel_of(row, D):
    if row == "rq":
        return vn.RQ_KERNEL
    return {"grad": GRAD_KERNEL, "hess": HESS_KERNEL}[row][D] if row in ("grad", "hess") else bm.NAMES[bm.C_KID[D]]


def hess_spec(D):
    return {"dims": list(range(D)), "lap_weight": th_.W4[:D]}


def cv_labels(N, rng, D):
    """A small tile: leave-one-out.  Else run_labels permuted, with one fold of exactly gpsat_max_cv_fold rows scattered over
    the tile."""
    if N <= 17:
        return np.arange(N, dtype=np.int32)
    lab = rng.permutation(cvn.run_labels(N, rng, 1, 64))
    lab[rng.permutation(N)[:L.max_cv_fold("f64", D)]] = lab.max() + 1
    return lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def inputs(row, D, which):
    """Batch "A" ([nd4, 17]: the 4-wave build) or "B" ([nd4 + 1, Nmax], at the row's largest D with Nmax - 15 between them: the
    8-wave build) of a row, and its theta: length scales in [1.5, 6] and sf2 / sn2 in [2, 4] (test_gpu_build_matrix._theta), the
    row's extra parameter from its case's x_large.  Drawn once, for every test that reads it (and for the CPU module)."""
    nd4, Nmax = ladder(D)
    if which == "A":
        Ns, Ps = [nd4, 17], [40, 17]
    elif D == ROW_D[row][-1]:
        Ns, Ps = [nd4 + 1, Nmax - 15, Nmax], [17, 5, 40]
    else:
        Ns, Ps = [nd4 + 1, Nmax], [17, 40]
    T = len(Ns)
    seed = 20000 + 1000 * ROWS.index(row) + 100 * D + (0 if which == "A" else 10)
    rng = np.random.default_rng(seed)
    kernel = kernel_of(row, D)
    if row == "cv":
        b = syn.make_batch(T, Ns, Ps, D, L.KERNEL_IDS[kernel], base_seed=seed, dtype=np.float64)
        b["kernel"] = kernel
        theta = bm._theta(rng, T, D)
        b["cv_fold"] = np.concatenate([cv_labels(N, rng, D) for N in Ns])
    else:
        case = CASE[row]
        b = case.batch(T, Ns, Ps, D, kernel, seed)
        theta = bm._theta(rng, T, D)
        if case.variant.extra:
            theta = np.column_stack([theta, np.resize(case.x_large, T)])
    return b, theta


def pack(parts):
    """Tiles (batch, theta, t) packed into a batch of their own, with the row's per-observation inputs."""
    b0 = parts[0][0]
    sl = [(b, slice(int(b["obs_off"][t]), int(b["obs_off"][t + 1])), slice(int(b["pred_off"][t]), int(b["pred_off"][t + 1])))
          for b, _, t in parts]
    out = dict(D=b0["D"], kernel=b0["kernel"], T=len(parts),
               obs_off=np.concatenate([[0], np.cumsum([o.stop - o.start for _, o, _ in sl])]),
               pred_off=np.concatenate([[0], np.cumsum([p.stop - p.start for _, _, p in sl])]),
               X=np.concatenate([b["X"][o] for b, o, _ in sl]), y=np.concatenate([b["y"][o] for b, o, _ in sl]),
               Xs=np.concatenate([b["Xs"][p] for b, _, p in sl]))
    for k in ("obs_var", "cv_fold"):
        if k in b0:
            out[k] = np.concatenate([b[k][o] for b, o, _ in sl])
    return out, np.array([th[t] for _, th, t in parts])


def run_row(row, e, b, theta, **kw):
    if row == "cv":
        return e.fit_predict_batch(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"], theta0=theta,
                                   kernel=b["kernel"], dtype="f64", optimiser="none", want_grad=True, cv_fold=b["cv_fold"], **kw)
    return run(CASE[row], e, b, theta, **kw)


def row_kw(row, D, which):
    """grad: pred_grad=True alone (its case's keyword).  hess: every coordinate, unequal Laplacian weights; in batch A with
    pred_grad=True beside it, so that the combined call crosses the build border too."""
    if row != "hess":
        return {}
    return dict(pred_hess=hess_spec(D), **({"pred_grad": True} if which == "A" else {}))


def fields_of(row, kw):
    out = FIELDS
    if row == "cv":
        out += CV_FIELDS
    if row == "grad" or kw.get("pred_grad"):
        out += ("f_grad", "f_grad_var")
    if row == "hess":
        out += ("f_hess", "f_hess_var", "f_lap", "f_lap_var")
    return out


# ---- the references, computed once per tile: the row's checks call them through their modules
def _key(a):
    if isinstance(a, np.ndarray):
        return (a.shape, a.dtype.str, a.tobytes())
    return tuple(_key(v) for v in a) if isinstance(a, (list, tuple)) else a


def _memo(fn):
    seen = {}

    @functools.wraps(fn)
    def cached(*args, **kw):
        k = (tuple(_key(a) for a in args), tuple(sorted((n, _key(v)) for n, v in kw.items())))
        if k not in seen:
            seen[k] = fn(*args, **kw)
        return seen[k]
    return cached


MEMO = {(mod, name): _memo(getattr(mod, name)) for mod, name in ((vn, "nll_and_grad"), (vn, "predict"), (pg, "predict_grad"),
                                                                  (ph, "predict_hess"), (cvn, "closed_form"))}


@pytest.fixture(autouse=True)
def one_reference_per_tile(monkeypatch):
    """The restatements behind check_tile, check_grad_tile and check_hess_tile answer a repeated question from memory (the
    figures printed here and the assertions ask the same one); nobody writes into what they return."""
    for (mod, name), fn in MEMO.items():
        monkeypatch.setattr(mod, name, fn)


def _tile(b, t):
    return slice(int(b["obs_off"][t]), int(b["obs_off"][t + 1])), slice(int(b["pred_off"][t]), int(b["pred_off"][t + 1]))


def shared_figures(case, r, b, t, theta):
    """The errors check_tile bounds, each in units of its bound."""
    o, p = _tile(b, t)
    X, y, D = b["X"][o], b["y"][o], b["D"]
    v = b["obs_var"][o] if case.variant is vn.NOISE else None
    nll, g = vn.nll_and_grad(case.variant, b["kernel"], X, y, theta, v)
    f, fv, yv = vn.predict(case.variant, b["kernel"], X, y, b["Xs"][p], theta, v)
    return {"nll": abs(r.nll[t] - nll) / (1e-9 * max(1.0, abs(nll)) * len(y)),
            "grad": (np.abs(r.grad[t] - g) / (1e-7 * np.abs(g) + 1e-8 * (np.abs(g).max() + 1))).max(),
            "f_mean": np.abs(r.f_mean[p] - f).max() / (1e-9 * max(np.abs(y).max(), 1.0)),
            "f_var": np.abs(r.f_var[p] - fv).max() / 1e-10, "y_var": np.abs(r.y_var[p] - yv).max() / 1e-10}


def deleted_folds(labels, seed):
    """The largest fold and five more, drawn by seed."""
    ids, counts = np.unique(labels, return_counts=True)
    big = ids[np.argmax(counts)]
    rest = np.random.default_rng(seed).permutation(ids[ids != big])[:N_DELETED - 1]
    return np.concatenate([[big], rest])


def cv_closed_figures(r, b, t, theta):
    """Every row of the tile against cv_numpy.closed_form, in units of test_gpu_cv._check's bounds."""
    o, _ = _tile(b, t)
    y, D, lab = b["y"][o], b["D"], b["cv_fold"][o]
    m0, f0, y0 = cvn.closed_form(L.KERNEL_IDS[b["kernel"]], b["X"][o], y, theta, lab)
    mean, fvar, yvar = (np.asarray(v)[o] for v in (r.cv_mean, r.cv_f_var, r.cv_y_var))
    assert np.isfinite(m0).all() and np.isfinite(mean).all() and np.isfinite(fvar).all() and np.isfinite(yvar).all()
    return {"cv_mean": np.abs(mean - m0).max() / (1e-9 * max(np.abs(y).max(), 1.0)), "cv_f_var": np.abs(fvar - f0).max() / 1e-10,
            "cv_y_var": np.abs(yvar - y0).max() / 1e-10, "cv_sn2": np.abs(yvar - fvar - theta[D + 1]).max() / 1e-12}


def check_cv_tile(r, b, t, theta, what):
    """cv_numpy.closed_form for every row, to the bounds of test_gpu_cv._check; then _check itself -- deletion -- for the largest
    fold and five more (for every fold of a tile of at most 17 rows): the rows of the other folds travel as never held out."""
    o, _ = _tile(b, t)
    fig = cv_closed_figures(r, b, t, theta)
    print("SIZES", what, f"N={o.stop - o.start}", " ".join(f"{k}={v:.3g}" for k, v in fig.items()), flush=True)
    assert max(fig.values()) <= 1.0, (what, t, fig)
    lab = b["cv_fold"][o]
    N = len(lab)
    keep = np.ones(N, dtype=bool) if N <= 17 else np.isin(lab, deleted_folds(lab, N))
    part = SimpleNamespace(**{f: np.where(keep, np.asarray(getattr(r, f))[o], np.nan) for f in CV_FIELDS})
    check_cv_deletion(part, 0, N, b["X"][o], b["y"][o], theta, L.KERNEL_IDS[b["kernel"]], np.where(keep, lab, -1), f"{what} tile {t}")
    return fig


def check_row_tile(row, r, b, t, theta, kw, what):
    """One tile against its row's restatement, by its row's checks; returns the errors in units of their bounds."""
    o, _ = _tile(b, t)
    if row == "cv":
        return check_cv_tile(r, b, t, theta, what)
    case = CASE[row]
    fig = shared_figures(case, r, b, t, theta)
    failed = []                                            # the derivative checks record their errors, then assert: print first
    if row == "grad" or kw.get("pred_grad"):
        tg.WORST.update(grad=0.0, var=0.0)
        try:
            tg.check_grad_tile(r, b, t, theta, what)
        except AssertionError as e:
            failed.append(e)
        fig.update(f_grad=tg.WORST["grad"] / 1e-9, f_grad_var=tg.WORST["var"] / 3e-10)
    if row == "hess":
        th_.WORST.update(hess=0.0, var=0.0, lap=0.0, lap_var=0.0)
        try:
            th_.check_hess_tile(r, b, t, theta, kw["pred_hess"], what)
        except AssertionError as e:
            failed.append(e)
        fig.update(f_hess=th_.WORST["hess"] / 1e-9, f_hess_var=th_.WORST["var"] / 2.5e-9, f_lap=th_.WORST["lap"] / 1e-9,
                   f_lap_var=th_.WORST["lap_var"] / 1e-10)
    print("SIZES", what, f"N={o.stop - o.start}", " ".join(f"{k}={v:.3g}" for k, v in fig.items()), flush=True)
    if failed:
        raise failed[0]
    check_tile(case, r, b, t, theta, what)
    return fig


# ---- 1. every row across the build border and up to the largest tile
@pytest.mark.parametrize("row,D", ROW_AND_D, ids=[f"{row}-D{D}" for row, D in ROW_AND_D])
def test_row_across_the_build_border_and_at_the_largest_tile(eng, row, D):
    """Batch A: the last tile of the 4-wave build beside a 17-row tile.  Batch B: the first tile of the 8-wave build and the
    largest tile the ABI accepts (at the row's largest D also Nmax - 15, whose last block holds one row).  Status 5 for every
    tile, every output within its row's bounds of its row's restatement."""
    nd4, Nmax = ladder(D)
    for which in "AB":
        b, theta = inputs(row, D, which)
        Ns = np.diff(b["obs_off"]).tolist()
        assert Ns == ([nd4, 17] if which == "A" else [nd4 + 1] + ([Nmax - 15] if D == ROW_D[row][-1] else []) + [Nmax])
        kw = row_kw(row, D, which)
        t0 = time.perf_counter()
        r = run_row(row, eng, b, theta, **kw)
        print("SIZES", f"{row} D={D} batch {which}: the call took {time.perf_counter() - t0:.3f} s, the kernel {r.kernel_ms:.1f} ms", flush=True)
        assert (r.status == 5).all(), (which, r.status)
        np.testing.assert_array_equal(r.theta, theta)
        for t in range(len(Ns)):
            check_row_tile(row, r, b, t, theta[t], kw, f"{row} D={D} batch {which} {b['kernel']}")


# ---- 2. the largest tile has the bits it has in batch B wherever its workspace lies
@pytest.mark.parametrize("row", ROWS)
def test_largest_tile_same_bits_alone_and_behind_a_small_tile(eng, row):
    """The workspace stride and the exchange area are largest here: an offset that depended on the tile's position in the
    launch would show in the bytes."""
    D = ROW_D[row][-1]
    b, theta = inputs(row, D, "B")
    a, tha = inputs(row, D, "A")
    t = b["T"] - 1
    kw = row_kw(row, D, "B")
    r = run_row(row, eng, b, theta, **kw)
    assert (r.status == 5).all()
    o, p = _tile(b, t)
    for what, parts in (("alone", [(b, theta, t)]), ("behind a 17-row tile", [(a, tha, 1), (b, theta, t)])):
        b1, th1 = pack(parts)
        r1 = run_row(row, eng, b1, th1, **kw)
        o1, p1 = _tile(b1, len(parts) - 1)
        for name in fields_of(row, kw):
            whole, got = np.asarray(getattr(r, name)), np.asarray(getattr(r1, name))
            want, got = (whole[o], got[o1]) if name in PER_ROW else (whole[p], got[p1]) if name in PER_POINT else (whole[[t]], got[[-1]])
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (row, what, name)


# ---- 3. the derivative rows at the numerical edges of test_numerical_edges_both_dtypes_both_builds
@pytest.mark.parametrize("kid", [0, 2, 3], ids=lambda k: bm.NAMES[k])
def test_derivative_rows_at_the_numerical_edges(eng, eng8, kid):
    """The four tiles of test_gpu_build_matrix._edge_batch in fp64 -- every coordinate twice, pairs one fp32 ulp apart, a length
    scale of 1e-10 (1 / (l_a l_b) = 1e20 beside a kernel value that has underflowed to 0), a length scale of 1.2e4 -- on both
    builds, with pred_grad and (RBF, Matern52) pred_hess over every coordinate with unequal weights.  The bounds are scaled by
    l_a and l_a l_b, so they mean something at both ends."""
    D = kid + 1
    b32, theta = bm._edge_batch(D, kid)
    kernel = bm.NAMES[kid]
    b = dict(b32, kernel=kernel, X=b32["X"].astype(np.float64), y=b32["y"].astype(np.float64), Xs=b32["Xs"].astype(np.float64),
             obs_var=np.zeros(len(b32["y"])))
    hess = kernel in ph.KERNELS
    kw = {"pred_grad": True, **({"pred_hess": hess_spec(D)} if hess else {})}
    for e_, what in ((eng, "4-wave"), (eng8, "8-wave")):
        r = run(th_.HESS if hess else tg.GRAD, e_, b, theta, **kw)
        for t in range(b["T"]):
            o, p = _tile(b, t)
            # the restatement's Cholesky succeeds on every one of these tiles (numpy raises where it does not)
            np.linalg.cholesky(vn.K_y(vn.NOISE, kernel, b["X"][o], theta[t], b["obs_var"][o]))
            assert r.status[t] == 5, (what, t, r.status[t])
            outs = {n: np.asarray(getattr(r, n))[p] for n in fields_of("hess" if hess else "grad", kw) if n in PER_POINT}
            for n, v in outs.items():
                assert np.isfinite(v).all(), (what, t, n)
            check_row_tile("hess" if hess else "grad", r, b, t, theta[t], kw, f"edges {kernel} {what} tile {t}")
            assert (outs["f_grad_var"] > 0).all(), (what, t)
            assert not hess or (outs["f_hess_var"] > 0).all(), (what, t)
