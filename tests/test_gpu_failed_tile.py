"""GPU: a tile that fails is held to the other half of the contract of include/gpsat_hip.h -- its status, NaN in every output --
in every row of the fp64 table of gpsat_amd/variants.py, on the 4-wave and the 8-wave build and under teams, and in the fp32
builds; and no other tile of the batch moves a bit.  The recipes (Z: an exactly zero pivot at a chosen
row, Q: a NaN coordinate, Y: a NaN observation), the statuses read from the code and the one check every test here uses are
tests/failed_tile_cases.py; tests/test_failed_tile_cpu.py proves them on the CPU.  The good tiles' agreement with the
restatements is held by the rows' own modules: nothing here has a tolerance of its own, except the priors of the tiles
without observations in test_fills_at_more_points_than_threads, which are held to the rows' existing bounds.
"""
import re

import numpy as np
import pytest

import pred_grad_numpy as pg
import pred_hess_numpy as ph
import variant_numpy as vn
from failed_tile_cases import (NAN, NOT_PD, Q_ROWS, ROWS, Tile, check_failed_batch, lengthscales_only, make, outputs, replicate, run,
                               statuses, subset)
from test_gpu_build_matrix import eng, eng8, n_cu  # noqa: F401 (the fixtures)

pytestmark = pytest.mark.gpu

ZS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 191, 192, 199)      # N = 200: 13 blocks of 16, panels of 4 + 4 + 4 + 1 block rows
YS = (0, 100, 199)
ALL_ROWS = sorted(ROWS)


def _bytes(x):
    return np.ascontiguousarray(np.asarray(x)).tobytes()


def _same(a, b, what):
    """Every output of two results of one batch, bit for bit (a NaN of a fill is one bit pattern)."""
    assert set(outputs(a)) == set(outputs(b)), what
    for name in outputs(a):
        assert _bytes(getattr(a, name)) == _bytes(getattr(b, name)), (what, name)


def _hold(e, b, what, alone_env=None, **kw):
    """Run ``b`` and the batch of its good tiles; check_failed_batch.  ``alone_env``: called before the good tiles run."""
    keep = [t for t in range(b["T"]) if t not in b["failed"]]
    r = run(e, b, **kw)
    if alone_env:
        alone_env()
    alone = run(e, subset(b, keep), **kw)
    print(f"{what}: {statuses(r)}; kernel {r.kernel_ms:.2f} ms")
    assert np.isin(alone.status, (0, 1, 4, 5, 6)).all(), alone.status
    check_failed_batch(r, b, b["failed"], alone, optimiser=kw.get("optimiser", "none"), trainable=kw.get("trainable"))
    return r, alone


def _between(failed):
    """The failed tiles with a good tile of N = 200 and one of N = 17 between them, P = 17 each."""
    k = -(-len(failed) // 3)
    return failed[:k] + [Tile("good", 200, 17, seed=21)] + failed[k:2 * k] + [Tile("good", 17, 17, seed=22)] + failed[2 * k:]


# ---- 1. where the pivot fails
@pytest.mark.parametrize("row", ALL_ROWS)
@pytest.mark.parametrize("build", ["d4", "w8"])
def test_a_pivot_that_fails_at_any_row(eng, eng8, build, row):
    """Twelve tiles of N = 200 that fail inside the first block, across a block border, at the last row of a panel, at the first
    row of the second and the third panel (the look-ahead sums in use), in the lone block row of the ragged last panel and at the
    last row: recipe Z, and recipe Q for the kernels that do not underflow."""
    kind = "Q" if row in Q_ROWS else "Z"
    b = make(_between([Tile(kind, 200, 17, z, 1000 + z) for z in ZS]), 2, ROWS[row])
    assert len(b["failed"]) == 12 and set(b["failed"].values()) == {NOT_PD}
    _hold({"d4": eng, "w8": eng8}[build], b, f"pivot {kind} {row} {build}")


@pytest.mark.parametrize("build", ["d4", "w8"])
def test_the_rows_in_front_of_the_zero_pivot_factorise(eng, eng8, build):
    """The other half of "fails at row z": the first z rows of every Z tile above, as tiles of their own, succeed -- K_y is the
    identity there, so the objective is y'y / 2 + z log(2 pi) / 2, held to the plain row's bound (1e-9 max(1, |nll|) N)."""
    b = make([Tile("H", 200, 17, z, 1000 + z) for z in ZS], 2, ROWS["plain"])
    assert not b["failed"] and (np.diff(b["obs_off"]) == ZS).all()
    r = run({"d4": eng, "w8": eng8}[build], b)
    print(f"heads {build}: {statuses(r)}")
    assert (r.status == 5).all()
    for t, z in enumerate(ZS):
        y = b["y"][b["obs_off"][t]:b["obs_off"][t + 1]]
        nll = 0.5 * y @ y + 0.5 * z * np.log(2.0 * np.pi)
        assert abs(r.nll[t] - nll) <= 1e-9 * max(1.0, abs(nll)) * z, (z, r.nll[t], nll)
    for name in outputs(r):
        assert np.isfinite(np.asarray(getattr(r, name))).all(), name


# ---- 2. the other way to fail
@pytest.mark.parametrize("row", ALL_ROWS)
@pytest.mark.parametrize("build", ["d4", "w8"])
def test_a_nan_objective_behind_a_factor_that_succeeds(eng, eng8, build, row):
    b = make(_between([Tile("Y", 200, 17, z, 2000 + z) for z in YS]), 2, ROWS[row])
    assert len(b["failed"]) == 3 and set(b["failed"].values()) == {NAN}
    _hold({"d4": eng, "w8": eng8}[build], b, f"objective Y {row} {build}")


# ---- 3. the tile behind a failed one
@pytest.mark.parametrize("row", ["plain", "pred_grad_hess", "cv"])
@pytest.mark.parametrize("build", ["d4", "w8"])
def test_the_tile_a_workgroup_takes_behind_a_failed_one(eng, eng8, monkeypatch, build, row):
    """[good A, failed (Z at the second panel), good B, failed (Y), good A again] on ONE workgroup (GPSAT_DEBUG_GRID=1, which
    gpsat_plan.h honours for either precision): sh->fail, the look-ahead sums and the z / alpha areas are the workgroup's own,
    and the good tiles return the bytes they return on workgroups of their own.  Then over three L-BFGS iterations (length
    scales trained, so that the failed tiles fail at theta0), unsliced and with the tile queue sliced after every evaluation
    and after every third: a suspended good tile is resumed behind a failed one."""
    e = {"d4": eng, "w8": eng8}[build]
    A = Tile("good", 200, 17, seed=31)
    b = make([A, Tile("Z", 200, 17, 65, 33), Tile("good", 200, 17, seed=32), Tile("Y", 200, 17, 100, 34), A], 2, ROWS[row])
    assert b["failed"] == {1: NOT_PD, 3: NAN}
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")

    def one_workgroup():
        monkeypatch.setenv("GPSAT_DEBUG_GRID", "1")

    def own_workgroups():
        monkeypatch.delenv("GPSAT_DEBUG_GRID")

    def two_copies(r):
        off = {"tile": np.arange(6), "pred": b["pred_off"], "obs": b["obs_off"], "fold": r.cv_fold_off}
        for name, axis in outputs(r).items():
            v = np.asarray(getattr(r, name))
            assert _bytes(v[off[axis][0]:off[axis][1]]) == _bytes(v[off[axis][4]:off[axis][5]]), name

    one_workgroup()
    r, _ = _hold(e, b, f"queue {row} {build} none", alone_env=own_workgroups)
    two_copies(r)
    kw = dict(optimiser="lbfgs", max_iter=3, trainable=lengthscales_only(b))
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "0")
    one_workgroup()
    rl, alone = _hold(e, b, f"queue {row} {build} lbfgs", alone_env=own_workgroups, **kw)
    two_copies(rl)
    assert (alone.n_eval > 1).all() and (alone.n_iter >= 1).all()
    one_workgroup()
    for seg in ("1", str(3 * 13 ** 3)):
        monkeypatch.setenv("GPSAT_DEBUG_SEG", seg)
        rs = run(e, b, **kw)
        print(f"queue {row} {build} lbfgs slice {seg}: {statuses(rs)}")
        check_failed_batch(rs, b, b["failed"], alone, optimiser="lbfgs", trainable=kw["trainable"])
        _same(rs, rl, f"slice {seg}")


# ---- 4. teams
@pytest.mark.parametrize("kind,z", [("Z", 1), ("Z", 64), ("Z", 1099), ("Y", 500)], ids=lambda v: str(v))
def test_a_team_unwinds_from_a_failed_tile(eng, monkeypatch, capfd, n_cu, kind, z):
    """[1100 failed, 1100 good, 0, 1100 failed] (1100 = 68 blocks + 12 rows): the failure in the first panel, a middle panel, the
    last row of the ragged last panel, or in the objective.  The owner publishes tc->fail, every member leaves the panel loop at
    the barrier behind part (B) and meets the owner at the next command; the next tile and the empty one are the team's too.
    Team sizes 1, 2, 5, 16 and the library's choice return the same bytes; size 1 passes the check."""
    tiles = [Tile(kind, 1100, 60, z, 41), Tile("good", 1100, 60, seed=42), Tile("empty", 0, 60, seed=43), Tile(kind, 1100, 60, z, 44)]
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_TEAM_STATS", "1")
    for row, kw in (("full_cov", {}), ("plain", dict(optimiser="lbfgs", max_iter=2))):
        b = make(tiles, 3, ROWS[row])
        if kw:
            kw["trainable"] = lengthscales_only(b)
        res, lines = {}, []
        for team in ("1", "2", "5", "16", None):
            if team is None:
                monkeypatch.delenv("GPSAT_DEBUG_TEAM")
            else:
                monkeypatch.setenv("GPSAT_DEBUG_TEAM", team)
            capfd.readouterr()
            res[team] = run(eng, b, **kw)
            err = capfd.readouterr().err
            m = re.search(r"gpsat team 0 \(size (\d+)\)", err)
            if team == "1":
                assert m is None, err
            else:
                assert m is not None and int(m.group(1)) == (min(16, n_cu // len(tiles)) if team is None else int(team)), err
            lines.append(f"team {team} {kind} z={z} {row}: {statuses(res[team])}; kernel {res[team].kernel_ms:.2f} ms")
        with capfd.disabled():                           # (the reads above would swallow it)
            print("\n".join(lines))
        for team in ("2", "5", "16", None):
            _same(res["1"], res[team], f"team {team}")
        monkeypatch.setenv("GPSAT_DEBUG_TEAM", "1")
        alone = run(eng, subset(b, [1, 2]), **kw)
        check_failed_batch(res["1"], b, b["failed"], alone, optimiser=kw.get("optimiser", "none"), trainable=kw.get("trainable"))
        assert alone.status[1] == 4 and alone.status[0] in ((0, 1) if kw else (5,))


# ---- 5. the fills at more points than threads
FILLS = {"pred_grad": (4, (1, 16, 17, 600)), "pred_grad_hess": (3, (1, 16, 17, 600)), "full_cov": (2, (1, 17, 70))}


@pytest.mark.parametrize("row", sorted(FILLS))
@pytest.mark.parametrize("build", ["d4", "w8"])
def test_fills_at_more_points_than_threads(eng, eng8, build, row):
    """The NaN fill of a failed tile and the prior fill of a tile without observations stride by the workgroup's threads over
    P x columns elements (P x P for the covariance): P = 1, 16, 17 and past any workgroup's thread count, a failed and an empty
    tile of each side by side and a good tile last, so that every slice has a neighbour on both sides whose bytes are known.
    The priors against the rows' own restatements at the rows' own bounds (test_gpu_pred_grad, test_gpu_pred_hess
    check_hess_tile, variant_cases.check_tile and check_full_cov)."""
    D, Ps = FILLS[row]
    tiles = [t for i, P in enumerate(Ps) for t in (Tile("Z", 20, P, 1, 50 + i), Tile("empty", 0, P, seed=60 + i))]
    b = make(tiles + [Tile("good", 33, 9, seed=70)], D, ROWS[row])
    r, _ = _hold({"d4": eng, "w8": eng8}[build], b, f"fills {row} {build}")
    for t, tile in enumerate(b["tiles"]):
        if tile.kind != "empty":
            continue
        th, (pa, pe) = b["theta0"][t], b["pred_off"][t:t + 2]
        P, Xs = int(pe - pa), b["Xs"][pa:pe]
        assert r.status[t] == 4 and P == tile.P
        np.testing.assert_array_equal(r.f_mean[pa:pe], 0.0)
        np.testing.assert_array_equal(r.f_var[pa:pe], th[D])
        np.testing.assert_array_equal(r.y_var[pa:pe], th[D] + th[D + 1])
        if r.f_grad is not None:
            fg, fgv = pg.predict_grad("RBF", np.zeros((0, D)), np.zeros(0), Xs, th)
            np.testing.assert_array_equal(r.f_grad[pa:pe], fg)
            np.testing.assert_array_equal(r.f_grad_var[pa:pe], fgv)
        if r.f_hess is not None:
            ref = ph.predict_hess("RBF", np.zeros((0, D)), np.zeros(0), Xs, th)
            np.testing.assert_array_equal(r.f_hess[pa:pe], 0.0)
            np.testing.assert_allclose(r.f_hess_var[pa:pe], ref[1], rtol=2e-15, atol=0)
            np.testing.assert_array_equal(r.f_lap[pa:pe], 0.0)
            np.testing.assert_allclose(r.f_lap_var[pa:pe], ref[3], rtol=4e-15, atol=0)
        if r.f_cov is not None:
            Cv = np.asarray(r.f_cov[r.cov_off[t]:r.cov_off[t + 1]]).reshape(P, P)
            np.testing.assert_allclose(Cv, vn.kernel_matrix(vn.NOISE, "RBF", Xs, Xs, th), rtol=0, atol=1e-9)
            np.testing.assert_array_equal(Cv, Cv.T)
            np.testing.assert_allclose(np.diag(Cv), r.f_var[pa:pe], rtol=0, atol=1e-9)


# ---- 6. fp32, the benchmarked path
@pytest.mark.parametrize("coop", ["0", "2"])
@pytest.mark.parametrize("build", ["w4", "w8"])
def test_fp32_pivot_that_fails_at_any_row(eng, eng8, n_cu, monkeypatch, build, coop):
    """Recipe Z in blocks of 32: inside the first block, across a block border, deep in the tile and at the last row.  The
    8-wave build directly; the 4-wave build with the batch replicated to at least one tile per CU.  Cooperation off and
    forced (the cooperative code path belongs to the 8-wave build; on the 4-wave build the knob must change nothing)."""
    tiles = _between([Tile("Z", 200, 17, z, 3000 + z) for z in (1, 31, 32, 33, 127, 128, 199)])
    rep = -(-n_cu // len(tiles)) if build == "w4" else 1
    b = make(replicate(tiles, rep), 2, ROWS["plain"], dtype="f32")
    assert len(b["failed"]) == 7 * rep and (build == "w8" or b["T"] >= n_cu)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_COOP", coop)
    r, _ = _hold({"w4": eng, "w8": eng8}[build], b, f"fp32 {build} coop {coop}")
    assert r.f_mean.dtype == np.float32
