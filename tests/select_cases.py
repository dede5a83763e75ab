"""Seeded recipes for device tile selection at every launch seam of gpsat_select.hip, and the one check they share.

A case is a table, the experts' reference locations, the criteria and (with an interval criterion) the per-expert bounds --
the arguments of Engine.select_batch.  `check_selection(off, idx, case)` holds a returned CSR pair to the NumPy restatement
(tests/select_numpy.py) exactly: every expert, no tolerance.  tests/test_select_cases_cpu.py proves the recipes (they reach
what they claim, the restatement equals the host selector on them, wrong variants trip the check);
tests/test_gpu_select_seams.py runs them on the device.

The radius of a ball belongs to the criterion, not to the expert, so the "everything" expert of a recipe is a second
criteria set on the same table and experts: `everything(case)`, one ball of radius 1e200 (r*r is +inf).

Columns of the general tables: 0 x, 1 y, 2 t (whole days), 3 z (used by no criterion), 4 the day as an interval code."""
import functools
import hashlib
from fractions import Fraction

import numpy as np

import select_numpy

SUB = 1024                    # rows per bounding box (SEL_SUB)
BIN_FROM = 65536              # tables of at least this many rows are binned when the criteria give a grid
SIZES_M = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537]
SIZES_T = [1, 7, 8, 9, 31, 32, 33, 65]
T_PAIR = (7, 33)              # every M runs at these two
M_PAIR = (4097, 65537)        # every T runs at these two
R_BALL = 3e5
STD = [("cmp", 2, "<=", 4.0), ("cmp", 2, ">=", -4.0), ("ball", [0, 1], "<=", R_BALL)]
COMPS = [">=", ">", "==", "<", "<="]
NEIGHBOUR = {">=": ">", ">": "==", "==": "<", "<": "<=", "<=": ">="}


class Case:
    def __init__(self, name, points, refs, criteria, bounds=None, bins=False, same=(), empty=(), family="", notes=None):
        self.name, self.criteria, self.family = name, list(criteria), family
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.refs = np.ascontiguousarray(refs, dtype=np.float64)
        self.bounds = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64)
        self.bins = bins                      # does select_bin_dims give a grid for this table (asked only from BIN_FROM rows)?
        self.same = list(same)                # pairs of experts with one reference location: identical lists
        self.empty = list(empty)              # experts far outside the table: empty lists
        self.notes = notes or {}              # what the recipe planted, for tests/test_select_cases_cpu.py
        self.points.setflags(write=False)
        self.refs.setflags(write=False)

    M = property(lambda self: self.points.shape[0])
    T = property(lambda self: self.refs.shape[0])
    binned = property(lambda self: self.bins and self.M >= BIN_FROM)
    finite = property(lambda self: bool(np.isfinite(self.points).all() and np.isfinite(self.refs).all()))

    def args(self):
        return self.points, self.refs, self.criteria, self.bounds

    def __repr__(self):
        return f"Case({self.name}: M={self.M}, T={self.T})"


_EXPECTED = {}


def expected(case):
    """The restatement's (off, idx) of a case, computed once and shared (read-only)."""
    if case.name not in _EXPECTED:
        off, idx = select_numpy.select(*case.args())
        off.setflags(write=False)
        idx.setflags(write=False)
        _EXPECTED[case.name] = (off, idx)
    return _EXPECTED[case.name]


def check_selection(off, idx, case):
    """Every expert of `case`: the CSR pair is well formed and equals the restatement's exactly."""
    off, idx = np.asarray(off), np.asarray(idx)
    n = case.name
    assert off.shape == (case.T + 1,), f"{n}: off has shape {off.shape}, want ({case.T + 1},)"
    assert off[0] == 0, f"{n}: off[0] = {off[0]}"
    assert (np.diff(off) >= 0).all(), f"{n}: off decreases at expert {int(np.argmax(np.diff(off) < 0))}"
    assert off[-1] == len(idx), f"{n}: off[-1] = {off[-1]} but {len(idx)} indices"
    if len(idx) > 1:
        rising = np.ones(len(idx), dtype=bool)
        rising[1:] = np.diff(idx.astype(np.int64)) > 0
        rising[off[:-1][off[:-1] < len(idx)]] = True               # a list's first entry has no predecessor
        assert rising.all(), f"{n}: a list is not strictly ascending at position {int(np.argmin(rising))}"
    w_off, w_idx = expected(case)
    if not np.array_equal(off, w_off):
        e = int(np.argmax(np.diff(off) != np.diff(w_off)))
        raise AssertionError(f"{n}: expert {e} has {off[e + 1] - off[e]} rows, the restatement {w_off[e + 1] - w_off[e]}")
    if not np.array_equal(idx, w_idx):
        j = int(np.argmax(idx != w_idx))
        e = int(np.searchsorted(off, j, side="right") - 1)
        raise AssertionError(f"{n}: expert {e}, entry {j - off[e]}: row {idx[j]}, the restatement has {w_idx[j]}")
    for a, b in case.same:
        assert np.array_equal(idx[off[a]:off[a + 1]], idx[off[b]:off[b + 1]]), f"{n}: experts {a} and {b} share a location"
    for e in case.empty:
        assert off[e + 1] == off[e], f"{n}: the distant expert {e} selected {off[e + 1] - off[e]} rows"


def bin_dims(criteria, points):
    """The columns select_bin_dims (gpsat_select_plan.h) makes a grid of: a two-sided window's column, then the ball columns, at
    most three, each once; a column without a finite range and a cell width that is no positive finite number are passed over."""
    dims = []

    def add(col, cell):
        if len(dims) >= 3 or not (cell > 0.0) or not np.isfinite(cell) or col in dims:
            return
        x = points[:, col]
        x = x[~np.isnan(x)]
        if len(x) == 0 or not np.isfinite(x.min()) or not np.isfinite(x.max()):
            return
        dims.append(col)

    cmps = [c for c in criteria if c[0] == "cmp"]
    for _, col, comp, val in cmps:
        if comp in ("<", "<="):
            for _, col2, comp2, val2 in cmps:
                if comp2 in (">=", ">") and col2 == col and val > val2:
                    add(col, 0.5 * (val - val2))
    for c in criteria:
        if c[0] == "ball":
            for col in c[1]:
                add(col, float(c[3]))
    return dims


def everything(case, comp="<="):
    """The same table and experts under one ball of radius 1e200: r*r is +inf, so "<=" takes every row whose squared distance is
    no NaN and "<" every row whose squared distance is finite -- every chunk, sub-chunk and 64-row group is walked in full."""
    balls = [c for c in case.criteria if c[0] == "ball"]
    cols = list(balls[0][1]) if balls else [case.criteria[0][1]]
    crit = [("ball", cols, comp, 1e200)]
    tag = "all" if comp == "<=" else "all_strict"
    return Case(f"{case.name}/{tag}", case.points, case.refs, crit, bins=bool(bin_dims(crit, case.points)), same=case.same,
                family="everything", notes={"of": case.name})


# ---- general tables ---------------------------------------------------------------------------------------------------
def _density(M):
    """(half width of the x, y square, days): small tables are dense enough that experts select rows."""
    return (6e5, 12) if M < 4000 else ((1e6, 20) if M < 60000 else (2e6, 40))


def _table(rng, M, ordered=False):
    span, days = _density(M)
    t = rng.integers(0, days, M).astype(np.float64)
    if ordered:
        t.sort()
    return np.stack([rng.uniform(-span, span, M), rng.uniform(-span, span, M), t, rng.standard_normal(M), t.copy()], axis=1)


def _experts(rng, T, M):
    """T reference locations: with T >= 2 expert 1 lies far outside the table, with T >= 3 the last repeats expert 0."""
    span, days = _density(M)
    refs = np.stack([rng.uniform(-0.9 * span, 0.9 * span, T), rng.uniform(-0.9 * span, 0.9 * span, T),
                     rng.integers(3, days - 3, T).astype(np.float64), np.zeros(T), np.zeros(T)], axis=1)
    same, empty = [], []
    if T >= 2:
        refs[1, :2] = [9e8, -9e8]
        empty = [1]
    if T >= 3:
        refs[T - 1] = refs[0]
        same = [(0, T - 1)]
    return refs, same, empty


def size_cases():
    """Every M at two values of T and every T at two values of M, under the window-and-ball set; odd positions are day-ordered."""
    pairs = [(M, T) for M in SIZES_M for T in T_PAIR]
    pairs += [(M, T) for T in SIZES_T for M in M_PAIR if (M, T) not in pairs]
    out = []
    for k, (M, T) in enumerate(pairs):
        rng = np.random.default_rng([11, M, T])
        pts = _table(rng, M, ordered=bool(k % 2))
        refs, same, empty = _experts(rng, T, M)
        out.append(Case(f"size_M{M}_T{T}", pts, refs, STD, bins=M > 0, same=same, empty=empty, family="size"))
    return out


# ---- exact ties -------------------------------------------------------------------------------------------------------
def _outward(x, c):
    return np.nextafter(x, np.inf if x > c else -np.inf)


def tie_ball_case(ncols, comp):
    """Integer-valued rows at exactly r from integer centres (Pythagorean triples and quadruples times 1e4: every difference,
    square and sum is exact in fp64), each with a sibling one ulp further out in one coordinate."""
    if ncols == 2:
        r = 1105e4
        shapes = [(3 * 221, 4 * 221), (5 * 85, 12 * 85), (8 * 65, 15 * 65)]                   # (3,4,5) (5,12,13) (8,15,17)
        # |centre| well above r: a coordinate's ulp must be no smaller than its difference's, or the outward step rounds away
        centres = [(30000001.0, -45000017.0), (-38000003.0, 41000023.0), (40000000.0, 33000011.0)]
    else:
        r = 21e4
        shapes = [(1 * 7, 2 * 7, 2 * 7), (2 * 3, 3 * 3, 6 * 3)]                               # (1,2,2,3) (2,3,6,7)
        centres = [(1234567.0, -7654321.0, 3000017.0), (-2000003.0, 3000017.0, -1000003.0), (40000000.0, 1000003.0, 5000011.0)]
    rng = np.random.default_rng([12, ncols])
    rows, on, out_ = [], [], []                                  # on / out_: (expert, row) planted at r / one ulp outside
    for e, c in enumerate(centres):
        for sh in shapes:
            for rot in range(ncols):
                leg = [sh[(m + rot) % ncols] * 1e4 for m in range(ncols)]
                for signs in range(2 ** ncols):
                    p = [c[m] + (leg[m] if (signs >> m) & 1 else -leg[m]) for m in range(ncols)]
                    on.append((e, len(rows)))
                    rows.append(list(p))
                    for k in range(ncols):                       # one coordinate one ulp outward: the first, counted from a
                        q = list(p)                              # start that rotates, whose ulp is large enough to move the sum
                        m_ = (rot + signs + k) % ncols
                        q[m_] = _outward(p[m_], c[m_])
                        if ball_unfused(q, c) > r * r:
                            break
                    else:
                        raise AssertionError(f"no coordinate of {p} moves the squared distance about {c}")
                    out_.append((e, len(rows)))
                    rows.append(q)
    rows = np.array(rows)
    filler = np.array([c for c in centres])[rng.integers(0, 3, 160)] + np.round(rng.uniform(-1.5 * r, 1.5 * r, (160, ncols)))
    rows = np.concatenate([rows, filler])
    assert np.abs(rows).max() < 2 ** 26
    M = len(rows)
    pts = np.zeros((M, 5))
    pts[:, :ncols] = rows
    pts[:, 3] = rng.standard_normal(M)
    T = 9
    refs = np.zeros((T, 5))
    refs[:3, :ncols] = centres
    refs[3, :ncols] = 6e7                                        # far outside
    refs[4:8, :ncols] = np.array(centres)[rng.integers(0, 3, 4)] + np.round(rng.uniform(-r, r, (4, ncols)))
    refs[8] = refs[0]
    name = f"tie_ball{ncols}_{'strict' if comp == '<' else 'incl'}"
    return Case(name, pts, refs, [("ball", list(range(ncols)), comp, r)], bins=True, same=[(0, 8)], empty=[3], family="ties",
                notes={"on": on, "outside": out_})


def tie_cmp_case(comp):
    """Rows equal to ref + val AS ROUNDED (ref 0.1, val 0.2: 0.30000000000000004), their two neighbours, rows y with
    y - ref == val but y != ref + val, and +0.0 / -0.0 against a right-hand side of 0.0."""
    rng = np.random.default_rng([13, COMPS.index(comp)])
    val = 0.2
    ref0 = np.concatenate([[0.1, 0.7, 1.1, -0.2, 0.3], rng.uniform(0.0, 1.0, 4)])
    rows, on, sub_only = [], [], []
    for e, rf in enumerate(ref0):
        y = rf + val
        on.append((e, len(rows)))
        rows += [y, np.nextafter(y, np.inf), np.nextafter(y, -np.inf)]
        z = y
        for _ in range(4):
            z = np.nextafter(z, -np.inf)
        for _ in range(9):                                      # y - 4 ulps .. y + 4 ulps
            if z != y and z - rf == val:
                sub_only.append((e, len(rows)))
                rows.append(z)
            z = np.nextafter(z, np.inf)
    rows += [0.0, -0.0, 0.3, 0.30000000000000004, 0.9, 0.8999999999999999]
    rows += list(rng.uniform(-0.5, 1.5, 40))
    M = len(rows)
    pts = np.stack([np.array(rows), rng.standard_normal(M)], axis=1)
    refs = np.stack([ref0, np.zeros(len(ref0))], axis=1)
    return Case(f"tie_cmp_{COMPS.index(comp)}", pts, refs, [("cmp", 0, comp, val)], family="ties",
                notes={"on": on, "sub_only": sub_only, "comp": comp})


# ---- rows that separate the reference's arithmetic from its near misses -----------------------------------------------
def ball_unfused(x, c):
    s = 0.0
    for a, b in zip(x, c):
        d = a - b
        s = s + d * d
    return s


def ball_fused(x, c):
    """fma(d, d, s): the exact d*d + s, rounded once."""
    s = 0.0
    for a, b in zip(x, c):
        d = a - b
        s = float(Fraction(d) * Fraction(d) + Fraction(s))
    return s


def ball_reversed(x, c):
    return ball_unfused(x[::-1], c[::-1])


@functools.lru_cache(maxsize=None)
def separating_rows(ncols, alt, comp="<=", directions=300):
    """Seeded search: points on the sphere of radius R_BALL about a centre of magnitude 1e6, the first coordinate walked
    -6..+6 ulps; kept where the reference-order sum and the alternative fall on different sides of r*r under `comp` (the two
    sums are neighbours, so a row that separates them under "<=" has one of them equal to r*r and does not under "<").
    Returns [(centre, row, inside by the reference order)]."""
    other = {"fma": ball_fused, "rev": ball_reversed}[alt]
    rng = np.random.default_rng([14, ncols, ["fma", "rev"].index(alt), comp == "<"])
    r2 = R_BALL * R_BALL
    inside = (lambda s: s < r2) if comp == "<" else (lambda s: s <= r2)
    out = []
    for _ in range(directions):
        c = rng.uniform(-2e6, 2e6, ncols)
        u = rng.standard_normal(ncols)
        x = c + u / np.linalg.norm(u) * R_BALL
        for k in range(-6, 7):
            y = x.copy()
            for _ in range(abs(k)):
                y[0] = np.nextafter(y[0], np.inf if k > 0 else -np.inf)
            a, b = ball_unfused(y, c), other(y, c)
            if inside(a) != inside(b):
                out.append((tuple(c), tuple(y), bool(inside(a))))
    return out


SEP_KEEP = 12           # separating rows kept per alternative (the recipes commit to at least 8)


def _sep_pick(ncols, alt, n=SEP_KEEP, comp="<="):
    """n separating rows of distinct centres, inside and outside alternating as far as the search gave both."""
    rows = separating_rows(ncols, alt, comp)
    seen, ins, outs = set(), [], []
    for c, y, a in rows:
        if c not in seen:
            seen.add(c)
            (ins if a else outs).append((c, y, a))
    pick = []
    while len(pick) < n and (ins or outs):
        if ins:
            pick.append(ins.pop(0))
        if outs and len(pick) < n:
            pick.append(outs.pop(0))
    return pick


def separating_case(ncols, comp):
    alts = ["fma"] if ncols == 2 else ["fma", "rev"]
    rng = np.random.default_rng([15, ncols])
    rows, centres, planted = [], [], {}
    for alt in alts:
        planted[alt] = []
        for c, y, _ in _sep_pick(ncols, alt, comp=comp):
            planted[alt].append((len(centres), len(rows)))
            centres.append(c)
            rows.append(y)
    cs = np.array(centres)
    u = rng.standard_normal((200, ncols))
    near = cs[rng.integers(0, len(cs), 200)] + u / np.linalg.norm(u, axis=1)[:, None] * R_BALL * rng.uniform(0.999, 1.001, (200, 1))
    rows = np.concatenate([np.array(rows), near])
    M, T = len(rows), len(cs)
    pts = np.zeros((M, 5))
    pts[:, :ncols] = rows
    refs = np.zeros((T, 5))
    refs[:, :ncols] = cs
    name = f"sep_ball{ncols}_{'strict' if comp == '<' else 'incl'}"
    return Case(name, pts, refs, [("ball", list(range(ncols)), comp, R_BALL)], bins=True, family="separating", notes={"planted": planted})


# ---- box ends ---------------------------------------------------------------------------------------------------------
BOX_RHS = 24.0


def _blocks_to_table(blocks, layout, rng):
    """Blocks of SUB rows (the last may be shorter) laid out in the given order ("ordered") or with the full blocks permuted
    and the rows inside every block shuffled ("shuffled": the boxes stay, the order goes)."""
    order = list(range(len(blocks)))
    if layout == "shuffled":
        full = [k for k in order if len(blocks[k]) == SUB]
        perm = list(rng.permutation(full))
        order = perm + [k for k in order if len(blocks[k]) != SUB]
        blocks = [b[rng.permutation(len(b))] for b in blocks]
    starts, pos = {}, 0
    for k in order:
        starts[k] = pos
        pos += len(blocks[k])
    return np.concatenate([blocks[k] for k in order]), starts


def box_cmp_case(comp, layout, single):
    """One column against a right-hand side of 24 (ref 20 + val 4).  Sub-chunks: values below; max alone equal to 24; constant
    24; min alone equal to 24; values above; a short tail.  `single`: one expert, so that no other expert of the wave makes the
    wave stream a sub-chunk that this one's box test gave up."""
    rng = np.random.default_rng([16, COMPS.index(comp), layout == "shuffled", single])
    low = np.sort(rng.uniform(5.0, 19.5, SUB))
    mx = np.sort(rng.uniform(20.0, 23.99, SUB))
    mx[-1] = BOX_RHS
    const = np.full(SUB, BOX_RHS)
    mn = np.sort(rng.uniform(24.01, 28.0, SUB))
    mn[0] = BOX_RHS
    high = np.sort(rng.uniform(28.5, 40.0, SUB))
    tail = np.sort(rng.uniform(40.0, 41.0, 100))
    blocks = [low, mx, const, mn, high, tail]
    col, starts = _blocks_to_table(blocks, layout, rng)
    M = len(col)
    pts = np.stack([rng.standard_normal(M), col], axis=1)
    rf = [20.0] if single else [20.0, 19.5, 16.0, 24.0, 20.0, 36.5, 1.0, 37.0, 20.5]
    refs = np.stack([np.zeros(len(rf)), np.array(rf)], axis=1)
    name = f"box_cmp_{COMPS.index(comp)}_{layout}_{'one' if single else 'nine'}"
    subs = {k: starts[j] // SUB for k, j in (("max_alone", 1), ("constant", 2), ("min_alone", 3))}
    return Case(name, pts, refs, [("cmp", 1, comp, 4.0)], family="box", same=[] if single else [(0, 4)],
                notes={"subs": subs, "comp": comp})


def box_ball_case(layout, single=None):
    """Sub-chunks made of 1024 copies of one separating row: the box is that point, so the skip test has to reproduce the row's own
    arithmetic.  `single` = k: only the expert of the k-th such sub-chunk."""
    rng = np.random.default_rng([17, layout == "shuffled"])
    pick = _sep_pick(3, "fma", 6)
    span = 2e6
    blocks = [rng.uniform(-span, span, (SUB, 3))] + [np.tile(np.array(y), (SUB, 1)) for _, y, _ in pick] + [rng.uniform(-span, span, (100, 3))]
    rows, starts = _blocks_to_table(blocks, layout, rng)
    M = len(rows)
    pts = np.zeros((M, 5))
    pts[:, :3] = rows
    cs = np.array([c for c, _, _ in pick])
    experts = list(range(len(pick))) if single is None else [single]
    refs = np.zeros((len(experts), 5))
    refs[:, :3] = cs[experts]
    subs = {f"copies_{k}": starts[k + 1] // SUB for k in experts if pick[k][2]}          # the ones that ARE selected
    name = f"box_ball_{layout}_{'six' if single is None else 'one%d' % single}"
    return Case(name, pts, refs, [("ball", [0, 1, 2], "<=", R_BALL)], bins=True, family="box",
                notes={"subs": subs, "inside": [pick[k][2] for k in experts]})


# ---- non-finite values ------------------------------------------------------------------------------------------------
def _nonfinite_table():
    rng = np.random.default_rng([18])
    M = 5 * SUB + 37
    pts = _table(rng, M)
    bad = [np.nan, np.inf, -np.inf]
    for col in (0, 1, 2, 3, 4):
        rows = rng.choice(M, 45, replace=False)
        pts[rows, col] = np.array(bad)[np.arange(45) % 3]
    pts[2 * SUB:3 * SUB, 0] = np.nan                 # a whole sub-chunk of NaN in x: nothing selectable where x is used
    pts[3 * SUB:4 * SUB, 3] = np.nan                 # a whole sub-chunk of NaN in z, which no criterion uses
    T = 17
    refs, same, empty = _experts(rng, T, M)
    refs[2, 0], refs[3, 0], refs[4, 0] = np.nan, np.inf, -np.inf
    refs[5, 2], refs[6, 2], refs[7, 2] = np.nan, np.inf, -np.inf
    refs[8, 1] = np.nan
    lo = rng.integers(0, 10, T).astype(np.float64)
    hi = lo + rng.integers(0, 5, T)
    lo[9], hi[9] = -np.inf, np.inf
    lo[10], hi[10] = np.nan, 5.0
    lo[11], hi[11] = 2.0, np.nan
    hi[12] = lo[12] - 1
    bounds = np.stack([lo, hi], axis=1)[:, None, :]
    bounds[T - 1] = bounds[0]
    return pts, refs, same, bounds


def nonfinite_cases():
    pts, refs, same, bounds = _nonfinite_table()
    sets = {"std": STD, "std_strict": STD[:2] + [("ball", [0, 1], "<", R_BALL)],
            "ball2": [("ball", [0, 1], "<=", R_BALL)], "ball2_strict": [("ball", [0, 1], "<", R_BALL)],
            "ball3": [("ball", [0, 1, 2], "<=", R_BALL)], "ball1": [("ball", [0], "<=", 1e5)],
            "t_only": [("cmp", 2, ">=", -4.0)],                                  # x unused: the NaN sub-chunk is selectable
            "ivl": [("ball", [0, 1], "<=", R_BALL), ("interval", 4, 0)], "ivl_only": [("interval", 4, 0)]}
    for comp in COMPS:
        sets[f"cmp_{COMPS.index(comp)}"] = [("cmp", 0, comp, 1e5)]
    out = []
    for tag, crit in sets.items():
        out.append(Case(f"nonfinite_{tag}", pts, refs, crit, bounds=bounds if "ivl" in tag else None,
                        bins=bool(bin_dims(crit, pts)), same=same, family="nonfinite"))
    # a ball of radius 0 over duplicated points: the duplicates of the centre, or nothing when strict
    rng = np.random.default_rng([19])
    p0 = np.zeros((300, 5))
    p0[:, :2] = rng.integers(0, 6, (300, 2))
    r0 = np.zeros((9, 5))
    r0[:, :2] = rng.integers(0, 6, (9, 2))
    r0[8] = r0[0]
    for comp in ("<=", "<"):
        out.append(Case(f"radius0_{'strict' if comp == '<' else 'incl'}", p0, r0, [("ball", [0, 1], comp, 0.0)], same=[(0, 8)],
                        family="nonfinite"))
    # coordinates of 1e300: the squares overflow
    M = 2 * SUB + 52
    pv = np.zeros((M, 5))
    pv[:, :2] = rng.uniform(-2e6, 2e6, (M, 2))
    pv[rng.choice(M, 40, replace=False), 0] = 1e300
    pv[rng.choice(M, 40, replace=False), 1] = -1e300
    pv[SUB:2 * SUB, 0] = 1e300
    rv = np.zeros((9, 5))
    rv[:, :2] = rng.uniform(-1.8e6, 1.8e6, (9, 2))
    rv[2, 0] = 1e300
    rv[3, 1] = -1e300
    rv[4, :2] = [1e300, -1e300]
    rv[8] = rv[0]
    for comp in ("<=", "<"):
        out.append(Case(f"overflow_{'strict' if comp == '<' else 'incl'}", pv, rv, [("ball", [0, 1], comp, R_BALL)], bins=True,
                        same=[(0, 8)], family="nonfinite"))
    return out


# ---- the binning threshold --------------------------------------------------------------------------------------------
def threshold_cases():
    """The same content just below BIN_FROM rows and at it, under criteria sets that give a grid and sets that do not."""
    rng = np.random.default_rng([20])
    full = _table(rng, BIN_FROM)
    r33, same33, empty33 = _experts(rng, 33, BIN_FROM)
    r7, same7, empty7 = _experts(rng, 7, BIN_FROM)
    r65, same65, _ = _experts(rng, 65, BIN_FROM)
    r65[2:12, 0] = [2.1e6, -2.1e6, 5e6, -5e6, 2.2e6, 1.9e6, 2.0e6, -2.0e6, 2.29e6, -2.31e6]     # outside the table's range
    r65[12:16, 2] = [-3.0, 43.0, 100.0, -100.0]
    lo = rng.integers(0, 36, 33).astype(np.float64)
    b33 = np.stack([lo, lo + rng.integers(0, 9, 33)], axis=1)[:, None, :]
    b33[32] = b33[0]                                   # the repeated expert repeats its bounds
    flat = full.copy()
    flat[:, 1] = 7.5                                   # max == min: one cell, inv_cell 0
    rflat = r33.copy()
    rflat[:, 1] = 7.5 + np.array([0.0, 1e4, 3e4])[np.arange(33) % 3]
    rflat[32] = rflat[0]
    nan = full.copy()
    for col in (0, 1, 2):
        nan[rng.choice(BIN_FROM - 1, 700, replace=False), col] = np.nan
    inf = full.copy()
    inf[rng.choice(BIN_FROM - 1, 10, replace=False), 0] = np.array([np.inf, -np.inf])[np.arange(10) % 2]
    E33, E7 = (r33, same33, empty33), (r7, same7, empty7)
    # tag: (table, (refs, same, empty), criteria, bounds, gives a grid)
    sets = {
        "win_ball": (full, E33, STD, None, True),
        "ball1": (full, E33, [("ball", [0], "<=", 2e4)], None, True),
        "ball2": (full, E7, [("ball", [0, 1], "<=", R_BALL)], None, True),
        "ball3": (full, E33, [("ball", [0, 1, 2], "<", R_BALL)], None, True),
        "ivl_ball": (full, E33, [("ball", [0, 1], "<=", R_BALL), ("interval", 4, 0)], b33, True),
        "degenerate": (flat, (rflat, same33, empty33), [("ball", [0, 1], "<=", 2e4)], None, True),
        "nan_rows": (nan, E33, STD, None, True),
        "cell_cap": (full, E33, [("ball", [0], "<=", 1e3)], None, True),           # 4e6 / 1e3 cells asked, 1024 given
        "outside": (full, (r65, same65, []), STD, None, True),
        "inf_ball2": (inf, E33, [("ball", [0, 1], "<=", R_BALL)], None, True),      # x passed over, y binned
        "one_sided": (full, E7, [("cmp", 2, ">=", 12.0)], None, False),
        "two_one_sided": (full, E33, [("cmp", 0, ">", 1e6), ("cmp", 1, "<", -1e6)], None, False),
        "inf_ball1": (inf, E33, [("ball", [0], "<=", 2e4)], None, False),           # its only column has no finite range
    }
    out = []
    for tag, (tab, (refs, same, empty), crit, bounds, grid) in sets.items():
        for M in (BIN_FROM - 1, BIN_FROM):
            out.append(Case(f"thr_{tag}_M{M}", tab[:M], refs, crit, bounds=bounds, bins=grid, same=same,
                            empty=empty if any(c[0] == "ball" for c in crit) else [], family="threshold"))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every recipe, each followed by its "everything" criteria set (strict as well where rows are not finite)."""
    base = size_cases()
    base += [tie_ball_case(n, comp) for n in (2, 3) for comp in ("<=", "<")] + [tie_cmp_case(comp) for comp in COMPS]
    base += [separating_case(n, comp) for n in (2, 3) for comp in ("<=", "<")]
    base += [box_cmp_case(comp, layout, single) for comp in COMPS for layout in ("ordered", "shuffled") for single in (False, True)]
    base += [box_ball_case(layout) for layout in ("ordered", "shuffled")]
    base += [box_ball_case("ordered", single=k) for k in range(4)]
    base += nonfinite_cases() + threshold_cases()
    out, seen = [], set()
    for c in base:
        out.append(c)
        for comp in ("<=", "<") if (not c.finite or c.name.startswith("overflow")) else ("<=",):
            ev = everything(c, comp)                   # one per distinct content: criteria sets of one table share theirs
            key = (hashlib.sha1(ev.points.tobytes()).digest(), hashlib.sha1(ev.refs.tobytes()).digest(), repr(ev.criteria))
            if key not in seen:
                seen.add(key)
                out.append(ev)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case_names():
    return [c.name for c in all_cases()]


def by_name(name):
    return {c.name: c for c in all_cases()}[name]
