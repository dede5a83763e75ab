"""GPU: device tile selection (gpsat_select.hip and the host steps of gpsat_select_batch_ex) held to the NumPy restatement at
every launch seam -- every expert of every recipe of tests/select_cases.py, exactly: the integer CSR arrays must be equal.

Which recipes are binned is stated by the recipes from the rule of select_bin_dims (`Case.bins`, proven against a restatement
of that rule in tests/test_select_cases_cpu.py); the library has no switch that reports it.  Tables of 65 536 rows and more
run with the binning on and off and must return the same bytes; the whole list runs forwards on one handle and backwards on
a fresh one, because the buffers and the two-call cache live in the handle."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import select_cases as sc

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
LARGE = [c for c in CASES if c.M >= sc.BIN_FROM]


def _run(engine, case):
    return engine.select_batch(case.points, case.refs, case.criteria, bounds=case.bounds)


def _binning(on):
    mp = pytest.MonkeyPatch()
    mp.setenv("GPSAT_DEVELOPER", "1")
    if on:
        mp.delenv("GPSAT_DEBUG_NO_BINNING", raising=False)
    else:
        mp.setenv("GPSAT_DEBUG_NO_BINNING", "1")
    return mp


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def forward(eng):
    """Every case in list order on one handle, binning as shipped."""
    mp = _binning(True)
    try:
        return {c.name: _run(eng, c) for c in CASES}
    finally:
        mp.undo()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_expert_equals_the_restatement(forward, case):
    sc.check_selection(*forward[case.name], case)


def test_backwards_on_a_fresh_handle_returns_the_same_bytes(forward):
    from gpsat_amd.engine import Engine
    mp = _binning(True)
    e = Engine(0)
    try:
        for case in reversed(CASES):
            off, idx = _run(e, case)
            assert off.tobytes() == forward[case.name][0].tobytes() and idx.tobytes() == forward[case.name][1].tobytes(), case.name
    finally:
        e.close()
        mp.undo()


def test_binning_off_returns_the_same_bytes(eng, forward):
    """The tables that are large enough to be binned, with GPSAT_DEBUG_NO_BINNING: the cases whose criteria give a grid took
    the sort / deal / map back / segmented sort path in `forward` and the plain path here; the others took the plain path twice."""
    assert sum(c.binned for c in LARGE) >= 20 and sum(not c.binned for c in LARGE) >= 3
    assert {c.T % 8 for c in LARGE if c.binned} >= {1, 7, 0}           # the dealing order with and without a part-filled wave
    mp = _binning(False)
    try:
        for case in LARGE:
            off, idx = _run(eng, case)
            sc.check_selection(off, idx, case)
            assert off.tobytes() == forward[case.name][0].tobytes() and idx.tobytes() == forward[case.name][1].tobytes(), case.name
    finally:
        mp.undo()


def test_one_row_across_the_binning_threshold(forward):
    """The same content at 65 535 rows (never binned) and at 65 536 (binned where the criteria give a grid)."""
    pairs = [(c, sc.by_name(c.name.replace("_M65536", "_M65535"))) for c in CASES if c.family == "threshold" and c.M == sc.BIN_FROM]
    assert len(pairs) == 13
    for at, below in pairs:
        (ao, ai), (bo, bi) = forward[at.name], forward[below.name]
        for e in range(at.T):
            a = ai[ao[e]:ao[e + 1]]
            assert np.array_equal(a[a < sc.BIN_FROM - 1], bi[bo[e]:bo[e + 1]]), (at.name, e)


# ---- the Python entry points above Engine.select_batch ----------------------------------------------------------------
def _names(case):
    return [f"c{k}" for k in range(case.points.shape[1])]


DEVICE_SELECTOR_CASES = ["size_M1_T7", "size_M4097_T9", "size_M65537_T33", "tie_ball2_incl", "tie_cmp_2", "sep_ball3_incl",
                         "box_cmp_0_shuffled_nine", "box_ball_ordered_six", "nonfinite_std", "nonfinite_ivl",
                         "thr_win_ball_M65536", "thr_ivl_ball_M65536", "thr_ball3_M65536", "thr_one_sided_M65535"]


@pytest.mark.parametrize("name", DEVICE_SELECTOR_CASES)
def test_device_selector(eng, forward, name):
    from gpsat_amd.local_experts import DeviceSelector
    case = sc.by_name(name)
    names = _names(case)
    ls, codes, strict = [], [], False
    for crit in case.criteria:
        if crit[0] == "cmp":
            ls.append({"col": names[crit[1]], "comp": crit[2], "val": crit[3]})
        elif crit[0] == "ball":
            ls.append({"col": [names[c] for c in crit[1]], "comp": crit[2], "val": crit[3]})
            strict = strict or crit[2] == "<"
        else:
            codes.append(case.points[:, crit[1]])
    ds = DeviceSelector(pd.DataFrame(case.points, columns=names), ls, eng, strict_ball=strict,
                        interval_codes=np.array(codes) if codes else None)
    off, idx = ds.select(pd.DataFrame(case.refs, columns=names), bounds=case.bounds)
    sc.check_selection(off, idx, case)
    assert off.tobytes() == forward[name][0].tobytes() and idx.tobytes() == forward[name][1].tobytes()


STRICT_BALL_CASES = [c.name for c in CASES if len(c.criteria) == 1 and c.criteria[0][0] == "ball" and c.criteria[0][2] == "<"]


@pytest.mark.parametrize("name", STRICT_BALL_CASES)
def test_prediction_locations_batch(eng, name):
    """max_dist of PredictionLocations is the strict ball: the rows gathered for every expert are the restatement's rows."""
    from gpsat_amd.local_experts import PredictionLocations
    case = sc.by_name(name)
    _, cols, _, r = case.criteria[0]
    names = [f"c{k}" for k in cols]
    pl = PredictionLocations(method="from_dataframe", coords_col=names, df=pd.DataFrame(case.points[:, cols], columns=names), max_dist=r)
    got = pl.batch(case.refs[:, cols], engine=eng)
    w_off, w_idx = sc.expected(case)
    np.testing.assert_array_equal(got.off, w_off, err_msg=name)
    assert got.cat.tobytes() == np.ascontiguousarray(case.points[w_idx][:, cols]).tobytes(), name


def test_strict_ball_cases_are_the_planted_ones():
    assert {"tie_ball2_strict", "tie_ball3_strict", "sep_ball2_strict", "sep_ball3_strict", "radius0_strict", "overflow_strict",
            "nonfinite_ball2_strict", "thr_ball3_M65536", "overflow_incl/all_strict", "nonfinite_std/all_strict"} <= set(STRICT_BALL_CASES)


# ---- the C ABI: a fill call whose capacity is too small ---------------------------------------------------------------
def test_too_small_capacity_is_refused_and_the_handle_stays_good(eng):
    from gpsat_amd import _lib as L
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                      # noqa: E731
    for name in ("size_M4097_T9", "thr_win_ball_M65536"):
        case = sc.by_name(name)
        w_off, w_idx = sc.expected(case)
        total = int(w_off[-1])
        assert total > 1
        sp = L.GpsatSelectSpec()
        sp.n_crit = len(case.criteria)
        for k, (kind, cols, comp, val) in enumerate(case.criteria):
            cl = [cols] if kind == "cmp" else list(cols)
            sp.kind[k], sp.comp[k], sp.ncols[k], sp.val[k] = (0 if kind == "cmp" else 1), L.COMP_IDS[comp], len(cl), float(val)
            for m, c_ in enumerate(cl):
                sp.cols[k][m] = int(c_)
        pc = np.ascontiguousarray(case.points.T)
        refs = np.ascontiguousarray(case.refs)
        M, Cc, T = case.M, case.points.shape[1], case.T
        call = lambda off, idx, cap: eng._lib.gpsat_select_batch(eng._h, C.byref(sp), M, Cc, p(pc), T, p(refs), p(off),   # noqa: E731
                                                                 None if idx is None else p(idx), cap)
        # (a) the fill call of a two-call selection, which the cache would have answered
        off = np.zeros(T + 1, np.int64)
        assert call(off, None, 0) == 0
        np.testing.assert_array_equal(off, w_off)
        small = np.full(total, -7, np.int32)
        assert call(off, small, total - 1) != 0
        assert b"capacity" in eng._lib.gpsat_last_error()
        assert (small == -7).all()                                                  # nothing was written
        sc.check_selection(*_run(eng, case), case)                                  # the next selection on the handle
        # (b) a fill call with nothing remembered: counted afresh, refused before the fill
        off2 = np.zeros(T + 1, np.int64)
        assert call(off2, small, total - 1) != 0
        assert (small == -7).all()
        np.testing.assert_array_equal(off2, w_off)                                  # the sizes are still reported
        full = np.empty(total, np.int32)
        assert call(off2, full, total) == 0
        sc.check_selection(off2, full, case)
        sc.check_selection(*_run(eng, case), case)

