"""CPU: the inputs of tests/test_gpu_sgpr_edges.py (tests/sgpr_edge_cases.py) meet the conditions that make its comparisons
sharp -- cond(Kuu) <= 1e3 for every generated tile, the shape coverage of the boundary batches, SciPy's preconditions for
the converged fits, numpy's own failure on the poisoned tiles.  Nothing here needs a GPU."""
import numpy as np
import pytest

import sgpr_edge_cases as ec
import sgpr_numpy as sn


def _conds(kid, tiles, th, jitter=sn.JITTER):
    return [ec.cond_kuu(kid, ec.centred(t)[2], th, jitter) for t in tiles]


def test_boundary_batches_cover_every_m_with_every_relation_of_n_and_p():
    seen = {M: dict(lt=0, eq=0, gt=0, p0=0, pp=0, ns=set(), ps=set()) for M in ec.MS}
    for kid in range(4):
        for D in range(1, 5):
            shapes = ec.boundary_shapes(kid, D)
            assert len(shapes) == ec.TILES_PER_BATCH
            order = [N * M * M for N, M, P in shapes]
            assert order != sorted(order) and order != sorted(order, reverse=True)      # not sorted by size
            assert len({M for _, M, _ in shapes}) >= 8                                   # a ragged batch
            for N, M, P in shapes:
                s = seen[M]
                s["lt"] += N < M; s["eq"] += N == M; s["gt"] += N > M
                s["p0"] += P == 0; s["pp"] += P > 0
                s["ns"].add(N); s["ps"].add(P)
                assert N >= 1 and (N < 1000 or N % 4 != 0)
    for M, s in seen.items():
        assert min(s["lt"], s["eq"], s["gt"], s["p0"], s["pp"]) >= 1, (M, s)
        assert s["ps"] == set(ec.PS), (M, s)
        assert {1, 2, 3, 5, max(M - 1, 1), M, M + 1} <= s["ns"] and max(s["ns"]) in ec.N_BIG, (M, s)


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_boundary_batches_are_well_conditioned(kid, D):
    tiles, th = ec.boundary_batch(kid, D)
    assert [(len(t[0]), len(t[2]), len(t[3])) for t in tiles] == ec.boundary_shapes(kid, D)
    assert max(_conds(kid, tiles, th)) <= ec.COND_MAX


@pytest.mark.parametrize("kid", [0, 1, 2, 3])
def test_chunk_batches_are_well_conditioned(kid):
    tiles, th = ec.chunk_batch(kid)
    Ps = [len(t[3]) for t in tiles]
    assert sorted(Ps) == sorted(2 * ec.CHUNK_PS) and {0, 1, 511, 512, 513, 1100} == set(Ps)
    assert [len(t[2]) for t in tiles] == [97, 1] * 8
    inner = [i for i in range(1, len(Ps) - 1) if Ps[i] == 0]
    assert inner and all(Ps[i - 1] > 0 or Ps[i + 1] > 0 for i in inner)              # P = 0 between the others
    assert max(_conds(kid, tiles, th)) <= ec.COND_MAX


def test_tiny_batch_special_tiles_fail_in_numpy_and_the_rest_are_well_conditioned():
    tiles, th, special = ec.tiny_batch()
    assert len(tiles) == 600 and len(special) == 12
    assert {"empty", "nan_y", "nan_x"} == set(special.values())
    assert 0 in special and 599 in special and any(100 < t < 500 for t in special)     # not only at the ends
    healthy = [t for t in range(len(tiles)) if t not in special]
    assert max(_conds(ec.TINY_KID, [tiles[t] for t in healthy], th)) <= ec.COND_MAX
    for t in healthy:
        X, y, Z, Xs = tiles[t]
        assert np.isfinite(X).all() and np.isfinite(y).all() and 20 <= len(X) <= 60 and 4 <= len(Z) <= 12 and 2 <= len(Xs) <= 4
    for t, kind in special.items():
        X, y, Z, Xs = tiles[t]
        assert len(Z) >= 1 and len(Xs) >= 1
        if kind == "empty":
            assert len(X) == 0 and len(y) == 0
            continue
        assert np.isnan(y).sum() == (kind == "nan_y") and np.isnan(X).sum() == (kind == "nan_x")
        c = np.nanmean(X, axis=0)                       # numpy at the poisoned tile: NaN or an exception, never a number
        try:
            el = sn.elbo(ec.TINY_KID, X - c, y, Z - c, th)
        except np.linalg.LinAlgError:
            continue
        assert np.isnan(el), (t, kind, el)


def test_zero_pivot_tile_is_exact_and_numpy_refuses_it():
    tiles, th, bad = ec.zero_pivot_batch()
    assert th[2] == 1.0 and 1.0 + ec.ZERO_PIVOT_JITTER == 1.0
    Xc, y, Zc, Pc = ec.centred(tiles[bad])
    assert (Zc[1] == Zc[0]).all()
    with pytest.raises(np.linalg.LinAlgError):
        sn.elbo(0, Xc, y, Zc, th, ec.ZERO_PIVOT_JITTER)
    rest = [t for i, t in enumerate(tiles) if i != bad]
    assert max(_conds(0, rest, th, ec.ZERO_PIVOT_JITTER)) <= ec.COND_MAX


def test_fit_batch_stays_well_conditioned_inside_its_box():
    tiles, th0 = ec.fit_batch()
    Ms, Ps = [len(t[2]) for t in tiles], [len(t[3]) for t in tiles]
    assert min(Ms) == 7 and max(Ms) == 97 and min(Ps) == 0 and max(Ps) == 65 and len(tiles) == 12
    corner = np.where(np.isfinite(ec.FIT_HI), ec.FIT_HI, th0)
    assert max(_conds(ec.FIT_KID, tiles, th0)) <= ec.COND_MAX
    assert max(_conds(ec.FIT_KID, tiles, corner)) <= ec.COND_MAX


@pytest.mark.parametrize("which", ["box", "fixed"])
def test_converged_cases_meet_scipys_preconditions(which):
    c = ec.converged_case(which)
    ctr = c["X"].mean(0)
    th, el, res = sn.fit_scipy(c["kid"], c["X"] - ctr, c["y"], c["Z"] - ctr, c["theta0"], c["lo"], c["hi"], c["trainable"])
    assert np.max(np.abs(res.jac)) <= 1e-5, res.message
    assert ec.cond_kuu(c["kid"], c["Z"] - ctr, th) < 1e5
    if which == "box":                                  # the box is inactive: the optimum is well inside it
        box = np.isfinite(c["lo"])
        assert box.sum() == c["D"] + 1
        assert np.all(th[box] > 2 * c["lo"][box]) and np.all(th[box] < 0.5 * c["hi"][box]), th
    else:
        fixed = ~c["trainable"]
        assert fixed.sum() == 2 and fixed[-1] and fixed[:c["D"]].sum() == 1
        assert th[fixed].tobytes() == c["theta0"][fixed].tobytes()


@pytest.mark.parametrize("which", ["all", "fixed"])
def test_adam_batches_are_well_conditioned_along_the_numpy_path(which):
    kid, D, tiles, th0, tr, steps, lr = ec.adam_batch(which)
    assert (which == "fixed") == (not tr.all())
    assert max(_conds(kid, tiles, th0)) <= ec.COND_MAX
    th, f, ok = ec.adam_numpy(kid, tiles[0], th0, tr, steps, lr)
    assert ok and np.isfinite(f) and th[~tr].tobytes() == th0[~tr].tobytes()
    assert np.max(np.abs(th[tr] - th0[tr])) > 1e-2      # the steps move theta far more than any bound of the comparison
    assert ec.cond_kuu(kid, ec.centred(tiles[0])[2], th) <= ec.COND_MAX


def test_centred_exact_batch_is_left_alone_by_centring():
    from gpsat_amd.engine import centre_tiles
    kid, D, pk, th0 = ec.centred_exact_batch()
    X, Xs, Z = centre_tiles(pk["X"], pk["Xs"], pk["obs_off"], pk["pred_off"], pk["Z"], pk["z_off"])
    assert X.tobytes() == pk["X"].tobytes() and Xs.tobytes() == pk["Xs"].tobytes() and Z.tobytes() == pk["Z"].tobytes()
    tiles = [(pk["X"][pk["obs_off"][t]:pk["obs_off"][t + 1]], None, pk["Z"][pk["z_off"][t]:pk["z_off"][t + 1]], None)
             for t in range(len(pk["obs_off"]) - 1)]
    assert max(ec.cond_kuu(kid, t[2], th0) for t in tiles) <= ec.COND_MAX
    assert len({len(t[0]) for t in tiles}) == len(tiles)        # ragged
