"""Inputs and checks shared by tests/test_gpu_sgpr.py, tests/test_gpu_sgpr_edges.py (GPU) and tests/test_sgpr_edges_cpu.py
(no GPU): well-conditioned sparse-GP tiles at every size boundary of gpsat_sgpr.hip, and the comparison of one
Engine.sgpr_fit_predict_batch result with the numpy restatement (sgpr_numpy.py).

Conditioning.  The comparison bound is 1e-9 + 64 eps cond(Kuu) relative (check_tile).  Inducing points half a length scale
apart reach cond(Kuu) = 2.5e8, which makes that 3.6e-6: too loose to see one dropped row.  lattice_tile draws the inducing
points from a jittered lattice of spacing 2.25 with length scales in [0.8, 1.5], where cond(Kuu + 1e-6 I) stays below 1e3
(tests/test_sgpr_edges_cpu.py asserts it for every tile generated here), so the bound is 1e-9 relative in effect.

A tile is the tuple (X [N, D], y [N], Z [M, D], Xs [P, D]) in uncentred coordinates; the engine and the checks centre it
by the mean observation coordinate."""
import numpy as np

import sgpr_numpy as sn
from oracle import gp_oracle as go

EPS = np.finfo(np.float64).eps
SPACING, JIT = 2.25, 0.2            # lattice spacing, and the jitter of a node as a fraction of it
S, SN2 = 1.3, 0.2                   # kernel variance and likelihood variance of every fixed-theta case
COND_MAX = 1e3

# section 1: every boundary of the 32 x 32 MFMA tiles (two 16-row halves, 8 waves), of mm's groups of 8 rows and of the
# 512 threads that own one column each
MS = [2, 7, 8, 9, 15, 17, 31, 32, 33, 47, 49, 64, 65, 96, 97, 255, 257, 511, 512, 513, 600]
PS = [0, 1, 7, 63, 64, 65]
N_BIG = [1997, 1998, 1999, 2001, 2002, 2003]      # "near 2000", none a multiple of the 4-row MFMA step
TILES_PER_BATCH = 11                # 16 batches x 11 = 176 slots: each of the 21 M occurs 8 or 9 times


def cond_kuu(kid, Z, th, jitter=sn.JITTER):
    D = Z.shape[1]
    return np.linalg.cond(go.kernel_matrix(kid, Z, Z, th[:D], th[D]) + jitter * np.eye(len(Z)))


def theta_of(rng, D):
    return np.concatenate([rng.uniform(0.8, 1.5, D), [S], [SN2]])


def lattice_tile(rng, N, M, D, P):
    """M inducing points on a random subset of the nodes of a D-dimensional lattice (spacing 2.25, every node moved by up to
    0.2 spacings per coordinate), X and Xs uniform over the lattice's cells, y a smooth function of X plus noise."""
    n = int(np.ceil(M ** (1.0 / D)))
    while n ** D < M:
        n += 1
    nodes = rng.permutation(n ** D)[:M]
    idx = np.stack(np.unravel_index(nodes, (n,) * D), axis=1).astype(np.float64)
    Z = SPACING * (idx + rng.uniform(-JIT, JIT, (M, D)))
    lo, hi = -0.5 * SPACING, (n - 0.5) * SPACING
    X = rng.uniform(lo, hi, (N, D))
    y = np.sin(X.sum(1)) + 0.3 * rng.normal(size=N)
    return X, y, Z, rng.uniform(lo, hi, (P, D))


def pack(tiles):
    off = lambda k: np.concatenate([[0], np.cumsum([len(t[k]) for t in tiles])]).astype(np.int64)
    cat = lambda k: np.concatenate([t[k] for t in tiles])
    return dict(obs_off=off(0), X=cat(0), y=cat(1), z_off=off(2), Z=cat(2), pred_off=off(3), Xs=cat(3))


def centred(tile):
    X, y, Z, Xs = tile
    c = X.mean(0) if len(X) else np.zeros(X.shape[1])
    return X - c, y, Z - c, Xs - c


# --------------------------------------------------------------------------------------------------------------------
# the comparison with numpy
# --------------------------------------------------------------------------------------------------------------------
def reference(kid, tile, th, want_grad=True, jitter=sn.JITTER):
    """What numpy gives for one tile at th, with everything the bounds of check_tile need."""
    Xc, y, Zc, Pc = centred(tile)
    ref = dict(el=sn.elbo(kid, Xc, y, Zc, th, jitter), cond=cond_kuu(kid, Zc, th, jitter))
    ref["f"], ref["fv"], ref["yv"] = sn.predict(kid, Xc, y, Zc, Pc, th, jitter)
    if want_grad:
        ref["g"] = sn.elbo_grad(kid, Xc, y, Zc, th, jitter)
        ref["gscale"] = sn.grad_rounding_scale(kid, Xc, y, Zc, th, jitter)
    return ref


def check_tile(r, t, pred_off, kid, tile, th, want_grad=True, jitter=sn.JITTER, ref=None, cond_max=None):
    """Tile t of the result r against numpy at th (the accuracy bounds stated at the head of tests/test_gpu_sgpr.py).
    want_grad=False: r.grad is not read.  ref: reference(...) computed before.  cond_max: also require cond(Kuu) <= it."""
    D = tile[0].shape[1]
    ref = reference(kid, tile, th, want_grad, jitter) if ref is None else ref
    what = f"kernel {kid} D {D} N {len(tile[0])} M {len(tile[2])} P {len(tile[3])} tile {t}"
    if cond_max is not None:
        assert ref["cond"] <= cond_max, (what, ref["cond"])
    cnd = 64 * EPS * ref["cond"]
    a, b = pred_off[t], pred_off[t + 1]
    el, f = ref["el"], ref["f"]
    assert abs(-r.nll[t] - el) <= (1e-9 + cnd) * abs(el), (what, -r.nll[t], el)
    if want_grad:
        g = ref["g"]
        gtol = 1e-7 * np.max(np.abs(g)) + cnd * ref["gscale"]
        assert np.all(np.abs(-r.grad[t] - g) <= gtol), (what, -r.grad[t] - g, gtol)
    assert b - a == len(f), what
    if b > a:
        assert np.max(np.abs(r.f_mean[a:b] - f)) <= (1e-9 + cnd) * max(1.0, np.max(np.abs(f))), what
        assert np.max(np.abs(r.f_var[a:b] - ref["fv"])) <= (1e-9 + cnd) * th[D], what
        assert np.max(np.abs(r.y_var[a:b] - ref["yv"])) <= (1e-9 + cnd) * th[D], what


def check_fixed(eng, kid, D, tiles, th, want_grad=True, jitter=sn.JITTER, only=None, refs=None, cond_max=None):
    """One call at fixed theta (optimiser "none") over the tiles; every tile (or those in ``only``) has status 5 and meets
    check_tile.  The engine's jitter argument is 0 for the default, so the default is passed as 0."""
    pk = pack(tiles)
    r = eng.sgpr_fit_predict_batch(D=D, kernel=kid, theta0=th, optimiser="none", want_grad=want_grad,
                                   jitter=0.0 if jitter == sn.JITTER else jitter, **pk)
    only = range(len(tiles)) if only is None else only
    assert (r.status[list(only)] == 5).all(), r.status
    for t in only:
        check_tile(r, t, pk["pred_off"], kid, tiles[t], th, want_grad, jitter, None if refs is None else refs[t], cond_max)
    return r


# --------------------------------------------------------------------------------------------------------------------
# section 1: the ragged batch of one (kernel, D)
# --------------------------------------------------------------------------------------------------------------------
def _n_of(M, cat, m):
    return [1, 2, 3, 5, max(M - 1, 1), M, M + 1, N_BIG[m % 6]][cat]


def boundary_shapes(kid, D):
    """(N, M, P) of the 11 tiles of batch 4 kid + D - 1.  Slot k = 11 batch + i of the 176 takes M number m = 5 k mod 21 (a
    stride coprime to 21: every run of 21 slots holds every M once, and a batch mixes sizes); at its j-th occurrence
    (j = k div 21) an M takes N number (j + m) mod 8 of {1, 2, 3, 5, M - 1, M, M + 1, ~2000} and P number (j + 3 m) mod 6
    of PS.  Eight occurrences give every M every N and every P; the order within the batch is then shuffled."""
    b = 4 * kid + D - 1
    shapes = []
    for i in range(TILES_PER_BATCH):
        k = TILES_PER_BATCH * b + i
        m, j = (5 * k) % len(MS), k // len(MS)
        M = MS[m]
        shapes.append((_n_of(M, (j + m) % 8, m), M, PS[(j + 3 * m) % len(PS)]))
    order = np.random.default_rng(900 + b).permutation(len(shapes))
    return [shapes[i] for i in order]


def boundary_batch(kid, D):
    rng = np.random.default_rng(1000 + 100 * kid + D)
    tiles = [lattice_tile(rng, N, M, D, P) for N, M, P in boundary_shapes(kid, D)]
    return tiles, theta_of(rng, D)


# --------------------------------------------------------------------------------------------------------------------
# section 2: prediction chunks of NT = 512 points
# --------------------------------------------------------------------------------------------------------------------
CHUNK_PS = [1, 0, 511, 0, 512, 513, 0, 1100]


def chunk_batch(kid):
    D = 2
    rng = np.random.default_rng(2000 + kid)
    tiles = [lattice_tile(rng, N, M, D, P) for M, N in ((97, 300), (1, 40)) for P in CHUNK_PS]
    order = [0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15]          # M = 97 and M = 1 alternate
    return [tiles[i] for i in order], theta_of(rng, D)


# --------------------------------------------------------------------------------------------------------------------
# section 3: 600 tiny tiles, 12 of them empty or poisoned
# --------------------------------------------------------------------------------------------------------------------
TINY_KID, TINY_D, TINY_T = 3, 2, 600
TINY_SPECIAL = {0: "empty", 1: "nan_y", 57: "nan_x", 58: "empty", 131: "nan_y", 256: "empty", 257: "nan_x", 258: "nan_y",
                400: "nan_x", 511: "empty", 598: "nan_y", 599: "nan_x"}


def tiny_batch():
    """(tiles, theta, special): special maps a tile's index to "empty" (N = 0), "nan_y" (one y is NaN) or "nan_x" (one
    coordinate of one X is NaN).  The other 588 tiles are healthy."""
    rng = np.random.default_rng(3000)
    tiles = []
    for t in range(TINY_T):
        N, M, P = int(rng.integers(20, 61)), int(rng.integers(4, 13)), int(rng.integers(2, 5))
        X, y, Z, Xs = lattice_tile(rng, N, M, TINY_D, P)
        kind = TINY_SPECIAL.get(t)
        if kind == "empty":
            X, y = X[:0], y[:0]
        elif kind == "nan_y":
            y[int(rng.integers(N))] = np.nan
        elif kind == "nan_x":
            X[int(rng.integers(N)), int(rng.integers(TINY_D))] = np.nan
        tiles.append((X, y, Z, Xs))
    return tiles, theta_of(rng, TINY_D), dict(TINY_SPECIAL)


ZERO_PIVOT_JITTER = 1e-30


def zero_pivot_batch():
    """(tiles, theta, bad) for RBF with kernel variance exactly 1: tile ``bad`` has Z[1] == Z[0], so with jitter 1e-30 the
    factorisation of Kuu meets K00 = 1 + 1e-30 = 1, L10 = 1 and the pivot 1 - 1 = 0 exactly."""
    D = 2
    rng = np.random.default_rng(3100)
    tiles = [lattice_tile(rng, N, M, D, 4) for N, M in ((30, 5), (41, 9), (25, 6), (50, 12), (33, 7))]
    bad = 2
    X, y, Z, Xs = tiles[bad]
    Z[1] = Z[0]
    th = np.concatenate([rng.uniform(0.8, 1.5, D), [1.0], [SN2]])
    return tiles, th, bad


# --------------------------------------------------------------------------------------------------------------------
# section 4: fits
# --------------------------------------------------------------------------------------------------------------------
FIT_KID, FIT_D = 2, 2
FIT_SHAPES = [(120, 33, 7), (60, 7, 0), (300, 97, 65), (45, 17, 1), (200, 64, 0), (97, 96, 63), (150, 31, 64), (80, 9, 7),
              (250, 65, 0), (33, 32, 1), (140, 47, 65), (110, 15, 63)]
# a box on the length scales and the kernel variance keeps every iterate where cond(Kuu) stays small: the CPU module
# asserts cond(Kuu) <= 1e3 at the corner (all length scales and the kernel variance at their upper bounds)
FIT_LO = np.array([0.4, 0.4, 0.05, np.nan])
FIT_HI = np.array([1.6, 1.6, 20.0, np.nan])


def fit_batch():
    rng = np.random.default_rng(4000)
    tiles = [lattice_tile(rng, N, M, FIT_D, P) for N, M, P in FIT_SHAPES]
    return tiles, np.array([1.0, 1.0, 1.0, 0.3])


def converged_case(which):
    """Two single-tile fits that SciPy L-BFGS-B brings to |jac| <= 1e-5 at cond(Kuu) < 1e5 (asserted by the CPU module),
    built like the tiles of test_gpu_sgpr.py::test_converged_fits_match_scipy.  Returns a dict with kid, D, X, y, Z, theta0
    and the lo / hi / trainable arguments (None where unused).
    "box": D = 3, Matern-3/2, a finite box on the length scales and the kernel variance that is inactive at the optimum.
    "fixed": D = 2, Matern-5/2, the likelihood variance and the second length scale fixed at theta0."""
    kid, D, side, seed = {"box": (2, 3, 4, 4101), "fixed": (3, 2, 5, 4202)}[which]
    rng = np.random.default_rng(seed)
    N, M = 400, 30
    X = rng.uniform(0, side, (N, D))
    y = np.sin(1.3 * X.sum(1)) + 0.2 * rng.normal(size=N)
    Z = X[rng.permutation(N)[:M]]
    case = dict(kid=kid, D=D, X=X, y=y, Z=Z, lo=None, hi=None, trainable=None)
    if which == "box":
        case["theta0"] = np.concatenate([np.full(D, 0.7), [1.0], [0.3]])
        case["lo"] = np.concatenate([np.full(D, 0.05), [0.01], [np.nan]])
        case["hi"] = np.concatenate([np.full(D, 30.0), [100.0], [np.nan]])
    else:
        case["theta0"] = np.array([0.7, 0.9, 1.0, 0.05])
        case["trainable"] = np.array([1, 0, 1, 0], bool)
    return case


# --------------------------------------------------------------------------------------------------------------------
# section 5: Adam
# --------------------------------------------------------------------------------------------------------------------
def adam_batch(which):
    """(kid, D, tiles, theta0, trainable, steps, lr): 20 steps at 0.1 with everything trainable, or 13 steps at 0.03 with
    the likelihood variance fixed."""
    kid, D, steps, lr, seed = {"all": (0, 3, 20, 0.1, 5001), "fixed": (2, 2, 13, 0.03, 5002)}[which]
    rng = np.random.default_rng(seed)
    tiles = [lattice_tile(rng, N, M, D, P) for N, M, P in ((90, 17, 3), (200, 33, 0), (64, 9, 5), (150, 65, 2))]
    th0 = np.ones(D + 2) if which == "all" else np.array([1.5, 0.7, 0.8, 0.2])
    tr = np.ones(D + 2, bool) if which == "all" else np.array([1, 1, 1, 0], bool)
    return kid, D, tiles, th0, tr, steps, lr


def adam_numpy(kid, tile, th0, trainable, steps, lr, jitter=sn.JITTER):
    """go.adam_minimise on u -> (-ELBO, -dELBO/dtheta dtheta/du) of the centred tile, softplus transforms with the shift
    rule of sgpr_numpy.fit_scipy.  Returns (theta, -ELBO at theta, ok)."""
    Xc, y, Zc, _ = centred(tile)
    H = len(th0)
    nan = np.full(H, np.nan)
    shift = np.where(np.arange(H) == H - 1, 1e-6, 0.0)
    u0 = go.u_from_theta(th0, nan, nan, shift)

    def th_of(uf):
        u = u0.copy()
        u[trainable] = uf
        return np.where(trainable, go.theta_from_u(u, nan, nan, shift), th0)

    def fun(uf):
        th = th_of(uf)
        g = -sn.elbo_grad(kid, Xc, y, Zc, th, jitter) * go.dtheta_du(th, nan, nan, shift)
        return -sn.elbo(kid, Xc, y, Zc, th, jitter), g[trainable]

    uf, ok, _ = go.adam_minimise(fun, u0[trainable], steps, lr)
    th = th_of(uf)
    return th, -sn.elbo(kid, Xc, y, Zc, th, jitter), ok


# --------------------------------------------------------------------------------------------------------------------
# section 6: a batch that centring leaves alone
# --------------------------------------------------------------------------------------------------------------------
def centred_exact_batch():
    """A ragged batch, centred with engine.centre_tiles and then put on the grid of multiples of 2^-20 with every tile's
    coordinate sums exactly zero (sums of such numbers are exact in fp64, whatever their order).  Centring it again
    subtracts exactly 0, so the host path (which centres) and the device path (which does not) see the same bits.
    Returns (kid, D, packed batch, theta0)."""
    from gpsat_amd.engine import centre_tiles
    kid, D = 1, 3
    rng = np.random.default_rng(6000)
    tiles = [lattice_tile(rng, N, M, D, P) for N, M, P in ((70, 9, 3), (1, 2, 0), (400, 33, 65), (33, 32, 1), (150, 17, 0),
                                                           (90, 65, 7))]
    pk = pack(tiles)
    X, Xs, Z = centre_tiles(pk["X"], pk["Xs"], pk["obs_off"], pk["pred_off"], pk["Z"], pk["z_off"])
    q = 2.0 ** 20
    X, Xs, Z = (np.round(a * q) / q for a in (X, Xs, Z))
    for t in range(len(tiles)):
        a, e = pk["obs_off"][t], pk["obs_off"][t + 1]
        X[a] -= X[a:e].sum(0)
    pk.update(X=np.ascontiguousarray(X), Xs=np.ascontiguousarray(Xs), Z=np.ascontiguousarray(Z))
    return kid, D, pk, np.array([1.0, 1.2, 0.9, 1.3, 0.2])
