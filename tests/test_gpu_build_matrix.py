"""GPU: every device code path the C API can choose, checked against the fp64 oracle up to the largest tile it accepts.

gpsat_fit_predict_batch picks the build from properties of the BATCH (gpsat_capi.cpp): the fp32 4-wave build (T >= CUs and
the largest tile's LDS <= 80 KiB), the fp32 8-wave build (larger tiles, or T < CUs; cooperative helpers on idle workgroups),
the fp64 4-wave build (`d4`: LDS of its layout <= 80 KiB), the fp64 8-wave build, and fp64 teams (NB >= 64, 2T <= CUs).
Each is run here at fixed parameters with gradients, on every (D, kernel) instantiation where it matters, and held to the
bounds the suite already states:
    fp32        tests/test_gpu_parity.py `_check_eval` (DESIGN.md "Numerics")
    fp64        objective 1e-9 |NLL| N, gradient 1e-7 relative, f* 1e-9 max|y|, f*_var 1e-10 (test_fp64_objective_gradient_predict)
    full cov    3e-5 (fp32) / 1e-9 (fp64) times sf2 / 0.8 (test_full_cov_ragged_batch_matches_oracle)
Parameters keep sf2 / sn2 <= 4 (test_ill_conditioned_truth_parameters holds the fp32 bounds there).
"""
import re

import numpy as np
import pytest

from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from oracle import gp_oracle as go
from test_gpu_parity import _check_eval, _oracle_eval

pytestmark = pytest.mark.gpu

NAMES = {0: "RBF", 1: "Matern12", 2: "Matern32", 3: "Matern52"}
FIELDS = ("theta", "nll", "grad", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var")
# Largest tile of the 4-wave builds, in blocks (fp32: 32 observations, fp64: 16): the last NB with the 4-wave LDS layout
# (gpsat_kernels.hip shared_bytes, gpsat_kernels_f64.hip shared_bytes_f64_w4) within 80 KiB, i.e. two workgroups per CU
W4_NB = {1: 51, 2: 37, 3: 28, 4: 23}
D4_NB = {1: 61, 2: 49, 3: 41, 4: 35}


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng8():
    """One workgroup per CU: the 8-wave builds whatever the batch."""
    from gpsat_amd.engine import Engine
    e = Engine(0, workgroups_per_cu=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _theta(rng, T, D):
    """length scales on the data's scale, sf2 / sn2 in [2, 4]"""
    sf2 = rng.uniform(0.3, 1.0, T)
    return np.column_stack([rng.uniform(1.5, 6.0, (T, D)), sf2, sf2 / rng.uniform(2.0, 4.0, T)])


def _run(e, b, th, kid, **kw):
    kw.setdefault("optimiser", "none")
    kw.setdefault("want_grad", True)
    return e.fit_predict_batch(D=b["D"], obs_off=b["obs_off"], X=b["X"], y=b["y"], pred_off=b["pred_off"], Xs=b["Xs"],
                               theta0=th, kernel=NAMES[kid], **kw)


def _replicate(b, th, rep):
    """the batch `rep` times over (tile t of copy k is tile t + k T)"""
    Ns, Ps = np.diff(b["obs_off"]), np.diff(b["pred_off"])
    big = dict(b, T=b["T"] * rep, X=np.tile(b["X"], (rep, 1)), y=np.tile(b["y"], rep), Xs=np.tile(b["Xs"], (rep, 1)),
               obs_off=np.concatenate([[0], np.cumsum(np.tile(Ns, rep))]),
               pred_off=np.concatenate([[0], np.cumsum(np.tile(Ps, rep))]))
    return big, np.tile(th, (rep, 1))


def _bits(x):
    return np.ascontiguousarray(np.asarray(x)).tobytes()


def _same(a, b, what):
    for f in FIELDS:
        assert _bits(getattr(a, f)) == _bits(getattr(b, f)), (what, f)


def _replicas_identical(r, T, P_per_copy, rep):
    """every copy of the batch returns the bits of the first copy"""
    for f in ("theta", "nll", "grad", "status"):
        v = np.asarray(getattr(r, f))
        first = v[:T]
        for k in range(1, rep):
            assert _bits(v[k * T:(k + 1) * T]) == _bits(first), (f, k)
    for f in ("f_mean", "f_var", "y_var"):
        v = np.asarray(getattr(r, f))
        for k in range(1, rep):
            assert _bits(v[k * P_per_copy:(k + 1) * P_per_copy]) == _bits(v[:P_per_copy]), (f, k)


def _check_f64(r, b, t, theta, kid, ref=None):
    N = int(b["obs_off"][t + 1] - b["obs_off"][t])
    pa, pe = b["pred_off"][t], b["pred_off"][t + 1]
    nll, g, f, fv, yv, ymax = ref if ref is not None else _oracle_eval(b, t, theta, kid)
    assert abs(r.nll[t] - nll) <= 1e-9 * max(1.0, abs(nll)) * max(N, 1), (N, r.nll[t], nll)
    np.testing.assert_allclose(r.grad[t], g, rtol=1e-7, atol=1e-8 * (np.abs(g).max() + 1), err_msg=f"N={N}")
    np.testing.assert_allclose(r.f_mean[pa:pe], f, rtol=0, atol=1e-9 * max(ymax, 1.0), err_msg=f"N={N}")
    np.testing.assert_allclose(r.f_var[pa:pe], fv, rtol=0, atol=1e-10, err_msg=f"N={N}")


def _check_cov(r, b, th, kid, tol):
    for t in range(b["T"]):
        a, e = b["obs_off"][t], b["obs_off"][t + 1]
        pa, pe = b["pred_off"][t], b["pred_off"][t + 1]
        P = int(pe - pa)
        if P == 0:
            continue
        C = np.asarray(r.f_cov[r.cov_off[t]:r.cov_off[t + 1]], dtype=np.float64).reshape(P, P)
        ref, _ = go.predict_cov(kid, b["X"][a:e].astype(np.float64), b["y"][a:e].astype(np.float64),
                                b["Xs"][pa:pe].astype(np.float64), th[t])
        np.testing.assert_allclose(C, ref, rtol=0, atol=tol * th[t, b["D"]] / 0.8, err_msg=f"tile {t}")
        np.testing.assert_array_equal(C, C.T)
        np.testing.assert_allclose(np.diag(C), np.asarray(r.f_var[pa:pe], dtype=np.float64), rtol=0, atol=tol)


# ------------------------------------------------------------------------------------------------------------------
# a. fp32 4-wave build: all 16 (D, kernel) instantiations
# ------------------------------------------------------------------------------------------------------------------
def _w4_batch(D, kid):
    lim = 32 * W4_NB[D]
    Ns = [1, 2, 31, 32, 33, 63, 64, 65, 500, lim - 1, lim, 200]
    Pv = [0, 1, 31, 32, 33, 255, 256, 257]
    Ps = [Pv[(i + D + kid) % len(Pv)] for i in range(len(Ns))]
    b = syn.make_batch(len(Ns), Ns, Ps, D, kid, base_seed=1000 * D + 100 * kid)
    return b, _theta(np.random.default_rng(10 * D + kid), len(Ns), D)


@pytest.mark.parametrize("kid", [0, 1, 2, 3], ids=lambda k: NAMES[k])
@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_four_wave_build_every_instantiation_matches_oracle(eng, eng8, n_cu, D, kid):
    """A ragged batch of 12 distinct tiles -- N from 1 to the 4-wave limit, P across the 32-row chunk boundaries --
    replicated to at least one tile per CU, so that the default engine runs the 4-wave build.  Every distinct tile against
    the oracle, every copy bit-identical to the first, the same bits from the 8-wave build."""
    b, th = _w4_batch(D, kid)
    T = b["T"]
    rep = -(-n_cu // T)
    big, thb = _replicate(b, th, rep)
    r = _run(eng, big, thb, kid)
    assert (r.status == 5).all() and (r.theta == thb).all()
    for t in range(T):
        _check_eval(r, b, t, th[t], kid)
    _replicas_identical(r, T, int(b["pred_off"][-1]), rep)
    _same(r, _run(eng8, big, thb, kid), "4-wave vs 8-wave build")


def _kloop_batch(D, kid):
    """every block count from 1 to 9, with the last block holding one observation and full"""
    Ns = [n for nb in range(1, 10) for n in (32 * nb - 31, 32 * nb)]
    Pv = [0, 1, 31, 32, 33, 64, 65, 96]
    Ps = [Pv[i % len(Pv)] for i in range(len(Ns))]
    b = syn.make_batch(len(Ns), Ns, Ps, D, kid, base_seed=6000 + 100 * D + 10 * kid)
    return b, _theta(np.random.default_rng(60 + 10 * D + kid), len(Ns), D)


@pytest.mark.parametrize("D,kid", [(3, 0), (2, 2)], ids=["D3-RBF", "D2-Matern32"])
def test_four_wave_build_every_small_block_count_matches_oracle(eng, eng8, n_cu, D, kid):
    """The k-loops are software pipelines of depth 2, 3 and 4 over n = 2 x (block rows) half steps: prologue, rotation and
    tail depend on n modulo the depth and on n < depth - 1, and an odd block count leaves the last panel without its second
    column.  18 tiles, NB = 1 .. 9 with the last block holding one observation or full, P across the chunk boundaries
    (and none), replicated to at least one tile per CU (the 4-wave build).  Every distinct tile against the oracle, every
    copy bit-identical to the first, the same bits from the 8-wave build."""
    b, th = _kloop_batch(D, kid)
    T = b["T"]
    assert T == 18 and sorted({-(-int(n) // 32) for n in np.diff(b["obs_off"])}) == list(range(1, 10))
    rep = -(-n_cu // T)
    big, thb = _replicate(b, th, rep)
    r = _run(eng, big, thb, kid)
    assert (r.status == 5).all() and (r.theta == thb).all()
    for t in range(T):
        _check_eval(r, b, t, th[t], kid)
    _replicas_identical(r, T, int(b["pred_off"][-1]), rep)
    _same(r, _run(eng8, big, thb, kid), "4-wave vs 8-wave build")


def test_four_wave_build_full_covariance_matches_oracle(eng, n_cu):
    D, kid = 3, 0
    b, th = _w4_batch(D, kid)
    T = b["T"]
    big, thb = _replicate(b, th, -(-n_cu // T))
    r = _run(eng, big, thb, kid, full_cov=True, want_grad=False)
    r0 = _run(eng, big, thb, kid, want_grad=False)
    np.testing.assert_array_equal(r.f_mean, r0.f_mean)
    np.testing.assert_array_equal(r.f_var, r0.f_var)
    assert _bits(r.f_cov[:r.cov_off[T]]) == _bits(r.f_cov[r.cov_off[T]:2 * r.cov_off[T]])
    r.cov_off = r.cov_off[:T + 1]
    _check_cov(r, b, th, kid, 3e-5)


# ------------------------------------------------------------------------------------------------------------------
# b. fp32 8-wave build above the 4-wave limit, up to gpsat_max_tile_obs: NB = 101 .. 128 at D = 1, 2
# ------------------------------------------------------------------------------------------------------------------
B_KID = {1: 0, 2: 1, 3: 2, 4: 3}          # every kernel at the largest tile of one D


def _w8_sizes(D):
    lim = L.max_tile_obs("f32", D)
    return sorted({32 * W4_NB[D] + 1, 1025, 2049, lim} | ({3200} if 3200 <= lim else set()))


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_eight_wave_build_up_to_the_tile_limit_matches_oracle(eng, D):
    kid = B_KID[D]
    Ns = _w8_sizes(D)
    b = syn.make_batch(len(Ns), Ns, [40, 33, 64, 1, 96][:len(Ns)], D, kid, base_seed=2000 + 10 * D)
    th = _theta(np.random.default_rng(20 + D), len(Ns), D)
    r = _run(eng, b, th, kid)
    assert (r.status == 5).all()
    for t in range(len(Ns)):
        _check_eval(r, b, t, th[t], kid)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_largest_fp32_tile_cooperative_modes_and_short_fit(eng, monkeypatch, capfd, D):
    """The largest fp32 tile alone in a launch: helpers attach (GPSAT_DEBUG_COOP_STATS), and cooperation off / on / forced
    returns the same bits over a short L-BFGS run, whose end point matches the oracle."""
    kid = B_KID[D]
    N = L.max_tile_obs("f32", D)
    b = syn.make_batch(1, N, 50, D, kid, base_seed=3000 + D)
    th = _theta(np.random.default_rng(30 + D), 1, D)
    lo, hi = syn.default_bounds(1, D)
    lo[:, D:], hi[:, D:] = 0.1, 0.4            # variances boxed: sf2 / sn2 <= 4 wherever the fit goes
    th[:, D:] = [0.3, 0.15]
    kw = dict(optimiser="lbfgs", max_iter=4, lo=lo, hi=hi)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    res = {}
    for mode in (0, 1, 2):
        monkeypatch.setenv("GPSAT_DEBUG_COOP", str(mode))
        monkeypatch.setenv("GPSAT_DEBUG_COOP_STATS", "1")
        capfd.readouterr()
        res[mode] = _run(eng, b, th, kid, **kw)
        err = capfd.readouterr().err
        m = re.search(r"gpsat coop: grid (\d+) T 1: cooperative evaluations (\d+), helper phases (\d+), helper groups \(sweep\) (\d+)", err)
        if mode == 0:
            assert m is None, err
        else:
            assert m is not None, err
            grid, ev, phases, groups = map(int, m.groups())
            assert grid > 1 and ev > 0, err
            if mode == 1:
                assert phases > 0 and groups > 0, err          # helpers really ran groups of the sweep
    _same(res[0], res[1], "cooperation off vs on")
    _same(res[0], res[2], "cooperation off vs forced")
    r = res[0]
    assert r.status[0] in (0, 1) and r.n_eval[0] > 1
    _check_eval(r, b, 0, r.theta[0], kid)


# ------------------------------------------------------------------------------------------------------------------
# c. fp64: the d4 / 8-wave boundary and teams
# ------------------------------------------------------------------------------------------------------------------
C_KID = {1: 3, 2: 2, 3: 1, 4: 0}


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_fp64_builds_and_teams_match_oracle(eng, monkeypatch, capfd, n_cu, D):
    """The largest d4 tile (a batch of its own: the largest tile picks the build), then the 8-wave build from one block
    above it to gpsat_max_tile_obs: one workgroup per tile, the team the library chooses (4 tiles, NB >= 64), 16 and 5."""
    kid = C_KID[D]
    nd4 = 16 * D4_NB[D]
    rng = np.random.default_rng(40 + D)
    # d4 build: the boundary tile with small ones
    Ns4 = [nd4, 1, 17, 300]
    b4 = syn.make_batch(len(Ns4), Ns4, [33, 2, 16, 0], D, kid, base_seed=4000 + 10 * D, dtype=np.float64)
    th4 = _theta(rng, len(Ns4), D)
    r4 = _run(eng, b4, th4, kid, dtype="f64")
    assert (r4.status == 5).all()
    for t in range(len(Ns4)):
        _check_f64(r4, b4, t, th4[t], kid)
    # 8-wave build
    Ns = [nd4 + 1, 1024, 2047, L.max_tile_obs("f64", D)]
    b = syn.make_batch(len(Ns), Ns, [17, 64, 5, 40], D, kid, base_seed=4100 + 10 * D, dtype=np.float64)
    th = _theta(rng, len(Ns), D)
    refs = [_oracle_eval(b, t, th[t], kid) for t in range(len(Ns))]
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_TEAM_STATS", "1")
    for team in ("1", None, "16", "5"):
        if team is None:
            monkeypatch.delenv("GPSAT_DEBUG_TEAM", raising=False)
        else:
            monkeypatch.setenv("GPSAT_DEBUG_TEAM", team)
        capfd.readouterr()
        r = _run(eng, b, th, kid, dtype="f64")
        err = capfd.readouterr().err
        m = re.search(r"gpsat team 0 \(size (\d+)\)", err)
        if team == "1":
            assert m is None, err
        else:
            assert m is not None and int(m.group(1)) == (min(16, n_cu // len(Ns)) if team is None else int(team)), err
        assert (r.status == 5).all(), (team, r.status)
        for t in range(len(Ns)):
            _check_f64(r, b, t, th[t], kid, refs[t])


def test_fp64_eight_wave_full_covariance_matches_oracle(eng):
    D, kid = 2, 3
    Ns, Ps = [900, 1200, 1000, 800], [63, 64, 65, 200]
    assert min(Ns) > 16 * D4_NB[D]
    b = syn.make_batch(len(Ns), Ns, Ps, D, kid, base_seed=5000, dtype=np.float64)
    th = _theta(np.random.default_rng(50), len(Ns), D)
    r = _run(eng, b, th, kid, dtype="f64", full_cov=True)
    assert (r.status == 5).all()
    for t in range(len(Ns)):
        _check_f64(r, b, t, th[t], kid)
    _check_cov(r, b, th, kid, 1e-9)


# ------------------------------------------------------------------------------------------------------------------
# d. numerical edges: duplicated and near-duplicated inputs (Matern at r = 0, where kfun clamps r), extreme length scales
# ------------------------------------------------------------------------------------------------------------------
def _edge_batch(D, kid):
    """four tiles, coordinates and observations fp32-representable (the fp32 and fp64 runs see the same data):
    every coordinate twice (sn2 = 0.01 sf2); pairs one fp32 ulp apart (sn2 = 0.01 sf2); length scale 1e-10 (the lower
    edge of the reference's known-answer box); length scale 1e3 x the data span"""
    rng = np.random.default_rng(700 + 10 * D + kid)
    n = 40
    base = rng.uniform(-6.0, 6.0, (n, D)).astype(np.float32)
    near = np.empty((2 * n, D), np.float32)
    near[0::2], near[1::2] = base, np.nextafter(base, np.float32(np.inf))
    tiles = [np.repeat(base, 2, axis=0), near, rng.uniform(-6.0, 6.0, (70, D)).astype(np.float32),
             rng.uniform(-6.0, 6.0, (70, D)).astype(np.float32)]
    X = np.concatenate(tiles)
    y = (np.sin(X[:, 0]) + 0.1 * rng.standard_normal(len(X))).astype(np.float32)
    Ps = [9, 33, 12, 5]
    Xs = rng.uniform(-5.0, 5.0, (sum(Ps), D)).astype(np.float32)
    th = np.array([[1.5] * D + [1.0, 0.01], [1.5] * D + [1.0, 0.01], [1e-10] * D + [0.8, 0.25], [1.2e4] * D + [0.8, 0.25]])
    b = dict(T=4, D=D, obs_off=np.concatenate([[0], np.cumsum([len(x) for x in tiles])]),
             pred_off=np.concatenate([[0], np.cumsum(Ps)]), X=X, y=y, Xs=Xs)
    return b, th


@pytest.mark.parametrize("kid", [0, 1, 2, 3], ids=lambda k: NAMES[k])
def test_numerical_edges_both_dtypes_both_builds(eng, eng8, n_cu, kid):
    D = kid + 1
    b, th = _edge_batch(D, kid)
    T = b["T"]
    refs = [_oracle_eval(b, t, th[t], kid) for t in range(T)]
    b64 = dict(b, X=b["X"].astype(np.float64), y=b["y"].astype(np.float64), Xs=b["Xs"].astype(np.float64))
    big, thb = _replicate(b, th, -(-n_cu // T))          # fp32: at least one tile per CU -> 4-wave build
    runs = {"f32 4-wave": (b, _run(eng, big, thb, kid)), "f32 8-wave": (b, _run(eng8, b, th, kid)),
            "f64 d4": (b64, _run(eng, b64, th, kid, dtype="f64")), "f64 8-wave": (b64, _run(eng8, b64, th, kid, dtype="f64"))}
    for name, (bb, r) in runs.items():
        for t in range(T):
            if not np.isfinite(refs[t][0]):                       # the fp64 Cholesky fails too: reported, not garbage
                assert r.status[t] == 2, (name, t, r.status[t])
                continue
            assert r.status[t] == 5, (name, t, r.status[t])
            pa, pe = bb["pred_off"][t], bb["pred_off"][t + 1]
            for v in (r.nll[t:t + 1], r.grad[t], r.f_mean[pa:pe], r.f_var[pa:pe], r.y_var[pa:pe]):
                assert np.isfinite(v).all(), (name, t)
            if name.startswith("f32"):
                _check_eval(r, bb, t, th[t], kid)
            else:
                _check_f64(r, bb, t, th[t], kid, refs[t])
