"""The selection recipes and their check, proven without a GPU (tests/select_cases.py, tests/select_numpy.py):
the restatement equals the host selector (LocalSelector's cKDTree.query_ball_point, max_dist_bool for strict balls) on every
case whose rows and experts are finite; the recipes reach the sizes and plant the rows they claim; and a restatement with one
deliberate error -- each of the ways a selection kernel goes wrong -- trips check_selection on a case the test names."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import select_cases as sc
import select_numpy as sn
from gpsat_amd.local_experts import LocalSelector, max_dist_bool

CASES = sc.all_cases()


# ---- the restatement against the host selector ------------------------------------------------------------------------
def _host_lists(case):
    """Every expert's rows by the host code: LocalSelector for compares, inclusive balls and intervals, max_dist_bool for strict
    balls (the two places the device kernel's predicates come from)."""
    names = [f"c{k}" for k in range(case.points.shape[1])]
    df = pd.DataFrame(case.points, columns=names)
    ls, strict, codes = [], [], []
    for crit in case.criteria:
        if crit[0] == "cmp":
            ls.append({"col": names[crit[1]], "comp": crit[2], "val": crit[3]})
        elif crit[0] == "ball" and crit[2] == "<":
            strict.append(crit)
        elif crit[0] == "ball":
            ls.append({"col": [names[c] for c in crit[1]], "comp": "<=", "val": crit[3]})
        else:
            assert crit[2] == len(codes)
            codes.append(case.points[:, crit[1]])
    off, idx = LocalSelector(df, ls, interval_codes=np.array(codes) if codes else None).select(
        pd.DataFrame(case.refs, columns=names), bounds=case.bounds)
    lists = sn.from_csr(off, idx)
    with np.errstate(all="ignore"):
        for _, cols, _, r in strict:
            for e in range(case.T):
                keep = max_dist_bool(case.points[:, cols], case.refs[e, cols], r)
                lists[e] = lists[e][keep[lists[e]]]
    return lists


def _kdtree_refuses(case):
    """cKDTree.query_ball_point raises ("floating point overflow") on a table whose squares overflow, so for an inclusive ball
    over 1e300 coordinates the reference has no answer; the strict ball of such a table goes through max_dist_bool."""
    return np.abs(case.points).max(initial=0.0) > 1e150 and any(c[0] == "ball" and c[2] != "<" for c in case.criteria)


def test_kdtree_refuses_only_the_overflowing_inclusive_balls():
    refused = [c.name for c in CASES if c.finite and _kdtree_refuses(c)]
    assert refused == ["overflow_incl", "overflow_incl/all"]
    with pytest.raises(ValueError, match="overflow"):
        _host_lists(sc.by_name("overflow_incl"))


@pytest.mark.parametrize("case", [c for c in CASES if c.finite and not _kdtree_refuses(c)], ids=lambda c: c.name)
def test_restatement_equals_host_selector(case):
    off, idx = sc.expected(case)
    want = _host_lists(case)
    for e in range(case.T):
        np.testing.assert_array_equal(idx[off[e]:off[e + 1]], want[e], err_msg=f"{case.name}: expert {e}")
    sc.check_selection(off, idx, case)                   # and the restatement passes its own check, hints included


def test_every_case_passes_its_own_check_and_states_its_grid():
    for case in CASES:
        sc.check_selection(*sc.expected(case), case)
        assert case.bins == bool(sc.bin_dims(case.criteria, case.points)), case.name
    # the binning rule as gpsat_select_plan.h words it, on the cases that matter for it
    grid = {c.name: sc.bin_dims(c.criteria, c.points) for c in CASES if c.family == "threshold"}
    assert grid["thr_win_ball_M65536"] == [2, 0, 1] and grid["thr_ball3_M65536"] == [0, 1, 2]
    assert grid["thr_ivl_ball_M65536"] == [0, 1] and grid["thr_degenerate_M65536"] == [0, 1]
    assert grid["thr_inf_ball2_M65536"] == [1] and grid["thr_inf_ball1_M65536"] == []
    assert grid["thr_one_sided_M65536"] == [] and grid["thr_two_one_sided_M65536"] == []


# ---- what the recipes commit to ---------------------------------------------------------------------------------------
def test_sizes_are_produced():
    size = [c for c in CASES if c.family == "size"]
    got = {(c.M, c.T) for c in size}
    for M in sc.SIZES_M:
        assert {T for m, T in got if m == M} >= set(sc.T_PAIR), M
    for T in sc.SIZES_T:
        assert {m for m, t in got if t == T} >= set(sc.M_PAIR), T
    assert max(c.M for c in CASES) == 65537 and max(c.T for c in CASES) == 65
    # every recipe has its "everything" set, by content (criteria sets of one table share it)
    alls = {(c.points.tobytes(), c.refs.tobytes()) for c in CASES if c.family == "everything"}
    for c in CASES:
        assert (c.points.tobytes(), c.refs.tobytes()) in alls, c.name
    for c in CASES:
        if c.family == "everything" and c.finite and not c.name.startswith("overflow"):
            off, idx = sc.expected(c)
            assert np.array_equal(idx, np.tile(np.arange(c.M, dtype=np.int32), c.T)), c.name


def test_threshold_pairs_share_their_content():
    thr = {c.name: c for c in CASES if c.family == "threshold"}
    assert len(thr) == 26
    for name, c in thr.items():
        if name.endswith("_M65536"):
            below = thr[name[:-len("65536")] + "65535"]
            assert c.M == 65536 and below.M == 65535 and c.binned == c.bins and not below.binned
            assert np.array_equal(c.points[:65535], below.points, equal_nan=True) and np.array_equal(c.refs, below.refs, equal_nan=True)
            lo, li = sc.expected(below)
            ho, hi = sc.expected(c)
            for e in range(c.T):                                    # the same lists but for the one row more
                h = hi[ho[e]:ho[e + 1]]
                assert np.array_equal(h[h < 65535], li[lo[e]:lo[e + 1]])
    assert sum(c.bins for c in thr.values()) == 20 and sum(c.binned for c in thr.values()) == 10


def test_planted_ties():
    for n in (2, 3):
        incl, strict = sc.by_name(f"tie_ball{n}_incl"), sc.by_name(f"tie_ball{n}_strict")
        assert len(incl.notes["on"]) >= 48
        for case, takes in ((incl, True), (strict, False)):
            lists = sn.from_csr(*sc.expected(case))
            for e, row in case.notes["on"]:
                assert (row in lists[e]) == takes, (case.name, e, row)
            for e, row in case.notes["outside"]:
                assert row not in lists[e], (case.name, e, row)
            pts = case.points[:, :n]
            assert (pts == np.round(pts)).sum() >= pts.size - len(case.notes["outside"]) and np.abs(pts).max() < 2 ** 26
    takes = {">=": (1, 1, 0), ">": (0, 1, 0), "==": (1, 0, 0), "<": (0, 0, 1), "<=": (1, 0, 1)}     # at rhs, one ulp above, below
    n_sub = 0
    for comp in sc.COMPS:
        case = sc.by_name(f"tie_cmp_{sc.COMPS.index(comp)}")
        lists = sn.from_csr(*sc.expected(case))
        for e, row in case.notes["on"]:
            assert [int(row + k in lists[e]) for k in range(3)] == list(takes[comp]), (comp, e)
        n_sub += len(case.notes["sub_only"])
        x = case.points[:, 0]
        zeros = np.nonzero(x == 0.0)[0]
        assert len(zeros) >= 2 and 0 < np.signbit(x[zeros]).sum() < len(zeros)          # +0.0 and -0.0
        assert all((z in lists[3]) == (comp in (">=", "==", "<=")) for z in zeros)       # expert 3: -0.2 + 0.2 == 0.0
    assert n_sub >= 5


# ---- restatements with one deliberate error ---------------------------------------------------------------------------
class BallOpen(sn.Restatement):                     # "<" where "<=" is meant
    def ball(self, xs, cs, comp, r):
        return sn.Restatement.ball(self, xs, cs, "<", r)


class BallClosed(sn.Restatement):                   # "<=" where the strict ball is meant
    def ball(self, xs, cs, comp, r):
        return sn.Restatement.ball(self, xs, cs, "<=", r)


class Fused(sn.Restatement):
    """s = fma(d, d, s): exact through Fraction for the rows near the surface (further out a fused sum, at most a few ulps from
    the plain one, cannot change sides)."""
    def ball_sum(self, xs, cs):
        s = sn.Restatement.ball_sum(self, xs, cs)
        with np.errstate(all="ignore"):
            near = np.nonzero(np.abs(s - sc.R_BALL ** 2) <= 1e-9 * sc.R_BALL ** 2)[0]
        for i in near:
            f = 0.0
            for x, c in zip(xs, cs):
                d = float(x[i]) - float(c)
                f = float(Fraction(d) * Fraction(d) + Fraction(f))
            s[i] = f
        return s


class Reversed(sn.Restatement):
    def ball_sum(self, xs, cs):
        return sn.Restatement.ball_sum(self, xs[::-1], cs[::-1])


class Float32(sn.Restatement):
    def cmp(self, x, ref, comp, val):
        return sn.COMPS[comp](x.astype(np.float32), np.float32(ref) + np.float32(val))

    def ball(self, xs, cs, comp, r):
        s = np.zeros(len(xs[0]), np.float32)
        for x, c in zip(xs, cs):
            d = x.astype(np.float32) - np.float32(c)
            s = s + d * d
        r2 = np.float32(r) * np.float32(r)
        return (s < r2) if comp == "<" else (s <= r2)


class SubtractRef(sn.Restatement):                  # x - ref <comp> val
    def cmp(self, x, ref, comp, val):
        return sn.COMPS[comp](x - ref, val)


def neighbour_of(comp):
    class Neighbour(sn.Restatement):
        def cmp(self, x, ref, c, val):
            return sn.Restatement.cmp(self, x, ref, sc.NEIGHBOUR[c] if c == comp else c, val)
    return Neighbour


class NanInside(sn.Restatement):
    def cmp(self, x, ref, comp, val):
        return sn.Restatement.cmp(self, x, ref, comp, val) | np.isnan(x)

    def ball(self, xs, cs, comp, r):
        return sn.Restatement.ball(self, xs, cs, comp, r) | np.isnan(self.ball_sum(xs, cs))

    def interval(self, x, lo, hi):
        return sn.Restatement.interval(self, x, lo, hi) | np.isnan(x)


def _trips(case_name, off, idx):
    case = sc.by_name(case_name)
    with pytest.raises(AssertionError, match=case_name.replace("/", ".")):
        sc.check_selection(off, idx, case)


def _differs(case_name, variant):
    """How many (expert, row) memberships the variant gets wrong on the case; the check must trip on it."""
    case = sc.by_name(case_name)
    with np.errstate(all="ignore"):
        off, idx = variant().select(*case.args())
    w_off, w_idx = sc.expected(case)
    n = sum(len(np.setxor1d(a, b)) for a, b in zip(sn.from_csr(off, idx), sn.from_csr(w_off, w_idx)))
    if n:
        _trips(case_name, off, idx)
    return n


PREDICATE_MUTANTS = [
    ("ball < for <=", BallOpen, ["tie_ball2_incl", "tie_ball3_incl", "radius0_incl", "overflow_incl/all"]),
    ("ball <= for <", BallClosed, ["tie_ball2_strict", "tie_ball3_strict", "radius0_strict", "overflow_incl/all_strict"]),
    ("fused accumulation", Fused, ["sep_ball2_incl", "sep_ball3_incl", "sep_ball2_strict", "sep_ball3_strict", "box_ball_ordered_six"]),
    ("reversed columns", Reversed, ["sep_ball3_incl", "sep_ball3_strict"]),
    ("float32", Float32, ["sep_ball2_incl", "tie_ball2_incl", "tie_cmp_2", "sep_ball3_incl"]),
    ("x - ref <comp> val", SubtractRef, [f"tie_cmp_{k}" for k in range(5)]),
    ("NaN inside", NanInside, ["nonfinite_std", "nonfinite_ball2", "nonfinite_cmp_0", "nonfinite_cmp_3", "nonfinite_ivl_only",
                               "nonfinite_std/all", "thr_nan_rows_M65536"]),
] + [(f"{comp} read as {sc.NEIGHBOUR[comp]}", neighbour_of(comp), [f"tie_cmp_{sc.COMPS.index(comp)}", f"nonfinite_cmp_{sc.COMPS.index(comp)}",
                                                                    f"box_cmp_{sc.COMPS.index(comp)}_ordered_one"]) for comp in sc.COMPS]


@pytest.mark.parametrize("what,variant,cases", PREDICATE_MUTANTS, ids=[m[0] for m in PREDICATE_MUTANTS])
def test_wrong_predicates_trip_the_check(what, variant, cases):
    for name in cases:
        assert _differs(name, variant) > 0, f"{what}: {name} does not tell it from the restatement"


def test_separating_rows_are_committed():
    """At least 8 planted rows per alternative on which the alternative arithmetic decides the other way."""
    for name, alt, variant in (("sep_ball2_incl", "fma", Fused), ("sep_ball3_incl", "fma", Fused), ("sep_ball3_incl", "rev", Reversed),
                               ("sep_ball2_strict", "fma", Fused), ("sep_ball3_strict", "fma", Fused), ("sep_ball3_strict", "rev", Reversed)):
        case = sc.by_name(name)
        planted = case.notes["planted"][alt]
        assert len(planted) >= 8
        got = sn.from_csr(*variant().select(*case.args()))
        want = sn.from_csr(*sc.expected(case))
        assert sum((row in got[e]) != (row in want[e]) for e, row in planted) >= 8, (name, alt)
    for n, alt, comp in ((2, "fma", "<="), (3, "fma", "<="), (3, "rev", "<="), (2, "fma", "<"), (3, "fma", "<"), (3, "rev", "<")):
        rows = sc.separating_rows(n, alt, comp)
        assert len(rows) >= 8 and 0 < sum(a for _, _, a in rows) < len(rows)
    assert any(sc.by_name("box_ball_ordered_six").notes["inside"]) and not all(sc.by_name("box_ball_ordered_six").notes["inside"])


def _drop(case, rows_of):
    """The restatement's lists with rows_of(e, list) -> bool mask of entries to drop."""
    lists = [l[~rows_of(e, l)] for e, l in enumerate(sn.from_csr(*sc.expected(case)))]
    return sn.to_csr(lists)


STRUCTURE_CASES = ["size_M4097_T9", "size_M65537_T33", "size_M4097_T9/all", "size_M65537_T33/all", "size_M1025_T7/all",
                   "thr_win_ball_M65536/all"]


@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_dropped_rows_trip_the_check(name):
    case = sc.by_name(name)
    M = case.M
    n_sub = (M + sc.SUB - 1) // sc.SUB
    is_all = name.endswith("/all")
    tripped = 0
    for what, lo, hi in [("first sub-chunk", 0, sc.SUB), ("a middle sub-chunk", (n_sub // 2) * sc.SUB, (n_sub // 2 + 1) * sc.SUB),
                         ("the last, partial sub-chunk", (n_sub - 1) * sc.SUB, M), ("the last 64-row group", (M - 1) // 64 * 64, M),
                         ("the last row", M - 1, M)]:
        off, idx = _drop(case, lambda e, l: (l >= lo) & (l < hi))
        changed = not np.array_equal(idx, sc.expected(case)[1])
        assert changed or not is_all, f"{name}: {what} holds no selected row"
        if changed:
            _trips(name, off, idx)
            tripped += 1
    assert tripped >= (5 if is_all else 1), name


def test_disordered_lists_trip_the_check():
    for name in ("size_M4097_T9", "size_M65537_T33/all", "thr_win_ball_M65536"):
        case = sc.by_name(name)
        off, idx = sc.expected(case)
        e = int(np.argmax(np.diff(off) >= 2))
        swapped = idx.copy()
        swapped[[off[e], off[e] + 1]] = swapped[[off[e] + 1, off[e]]]             # two entries of one list
        _trips(name, off, swapped)
        lists = sn.from_csr(off, idx)
        b = next((k for k in range(1, case.T) if not np.array_equal(lists[k], lists[0])), None)
        assert (b is None) == name.endswith("/all")
        if b is not None:
            lists[0], lists[b] = lists[b], lists[0]                               # two experts' lists
            _trips(name, *sn.to_csr(lists))
    # equal lengths, so only the indices tell
    case = sc.by_name("size_M4097_T9/all")
    off, idx = sc.expected(case)
    shifted = idx.copy()
    shifted[off[2]] = shifted[off[2] + 1]                                         # a repeated row: not strictly ascending
    _trips(case.name, off, shifted)


def test_skipped_box_end_sub_chunks_trip_the_check():
    """Each sub-chunk whose box END equals the right-hand side (or whose box is one separating point), taken as skippable."""
    n = 0
    for case in CASES:
        if case.family != "box":
            continue
        lists = sn.from_csr(*sc.expected(case))
        for what, sub in case.notes["subs"].items():
            lo, hi = sub * sc.SUB, (sub + 1) * sc.SUB
            holds = any(((l >= lo) & (l < hi)).any() for l in lists)
            if "comp" in case.notes:              # which box ends must be selected, which stay empty
                comp = case.notes["comp"]
                must = {"constant": comp in (">=", "==", "<="), "max_alone": comp in (">=", "==", "<", "<="),
                        "min_alone": comp in (">=", ">", "==", "<=")}[what]
                e0 = ((lists[0] >= lo) & (lists[0] < hi)).sum()           # expert 0: right-hand side 24
                assert (e0 > 0) == must, (case.name, what)
                if what == "constant":
                    assert e0 == (sc.SUB if must else 0), (case.name, what)
            else:
                assert holds, (case.name, what)
            if holds:
                _trips(case.name, *_drop(case, lambda e, l: (l >= lo) & (l < hi)))
                n += 1
    assert n >= 40
