"""GPU: the per-tile memo of evaluations (gpsat_kernels.hip, KernelArgs::memo) changes no bit of any output.

A line-search evaluation whose D + 2 parameter floats the tile has evaluated before is answered from the memo instead of being
computed.  The batches here keep every tile iterating at the fp32 noise floor (`ftol = gtol = -1`, 40 iterations), where the
line search bisects its bracket below one fp32 ulp and then evaluates the same floats until `max_ls`: repeats are certain, and
so are tiles whose last line-search evaluation is one.  Every run is compared byte for byte with the run without the memo
(`GPSAT_DEBUG_EVAL_CACHE=0`) on the 4-wave build, which computes every evaluation.
"""
import functools
import os
import re
import tempfile

import numpy as np
import pytest

from gpsat_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var")
CASES = {"rbf-d3": (3, 0, 7_100_000), "matern32-d2": (2, 2, 7_200_000)}
T, P, REP = 96, 40, 3          # 96 distinct tiles, three times over: 288 tiles >= CUs, so that the default engine takes the 4-wave build
KNOBS = ("GPSAT_DEVELOPER", "GPSAT_DEBUG_EVAL_CACHE", "GPSAT_DEBUG_EVAL_CACHE_STATS", "GPSAT_DEBUG_SEG", "GPSAT_DEBUG_GRID")
STATS = re.compile(r"gpsat eval cache: T (\d+): memo (on|off), evaluations (\d+), answered from the memo (\d+), of those the previous "
                   r"key again (\d+), tiles with such an evaluation (\d+), tiles that finished on one (\d+)")


@functools.lru_cache(maxsize=None)
def _batch(case):
    D, kid, seed = CASES[case]
    Ns = np.tile([33, 64, 97, 160], T // 4)
    b = syn.make_batch(T, Ns, P, D, kid, base_seed=seed)
    lo, hi = syn.default_bounds(T, D)
    rep = lambda v: np.tile(v, (REP,) + (1,) * (np.ndim(v) - 1))
    off = lambda o: np.concatenate([[0], np.cumsum(np.tile(np.diff(o), REP))])
    return dict(D=D, obs_off=off(b["obs_off"]), X=rep(b["X"]), y=rep(b["y"]), pred_off=off(b["pred_off"]), Xs=rep(b["Xs"]),
                theta0=np.ones((T * REP, D + 2)), lo=rep(lo), hi=rep(hi), kernel=kid, optimiser="lbfgs", max_iter=40,
                ftol=-1.0, gtol=-1.0)


@functools.lru_cache(maxsize=None)
def _run(case, wg_per_cu, memo, sliced):
    """One launch (computed once, shared by the tests): its outputs as bytes per field, and the memo statistics it printed."""
    from gpsat_amd.engine import Engine
    env = {"GPSAT_DEVELOPER": "1", "GPSAT_DEBUG_EVAL_CACHE": "1" if memo else "0", "GPSAT_DEBUG_EVAL_CACHE_STATS": "1",
           "GPSAT_DEBUG_SEG": "1" if sliced else "0"}
    if sliced:
        env["GPSAT_DEBUG_GRID"] = "48"            # six tiles per resident workgroup: tiles wait in the ring, slices are taken
    saved = {k: os.environ.get(k) for k in KNOBS}
    eng = Engine(0, workgroups_per_cu=wg_per_cu)
    fd2 = os.dup(2)
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        with tempfile.TemporaryFile() as tmp:
            os.dup2(tmp.fileno(), 2)
            try:
                r = eng.fit_predict_batch(**_batch(case))
            finally:
                os.dup2(fd2, 2)
            tmp.seek(0)
            err = tmp.read().decode(errors="replace")
    finally:
        os.close(fd2)
        eng.close()
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert "re-running" not in err, err
    m = STATS.findall(err)
    assert len(m) == 1, err
    names = ("T", "memo", "evaluations", "hits", "hits_prev", "tiles_hit", "tiles_finished_on_hit")
    stats = {n: (v if n == "memo" else int(v)) for n, v in zip(names, m[0])}
    out = {f: np.ascontiguousarray(np.asarray(getattr(r, f))) for f in FIELDS}
    return out, stats


def _same(a, b, what):
    for f in FIELDS:
        x, y = a[f], b[f]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, f)
        if x.tobytes() != y.tobytes():
            rows = len(a["nll"])
            bad = np.nonzero((x.reshape(rows, -1).view(np.uint8) != y.reshape(rows, -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError(f"{what}: `{f}` differs for {len(bad)} tiles (first: {list(bad[:6])})")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("wg_per_cu", [0, 1], ids=["4-wave", "8-wave"])
def test_memo_on_equals_memo_off(case, wg_per_cu):
    ref, ref_stats = _run(case, 0, False, False)          # every evaluation computed, 4-wave build
    off, off_stats = _run(case, wg_per_cu, False, False)
    on, on_stats = _run(case, wg_per_cu, True, False)
    print(case, wg_per_cu, "off:", off_stats, "on:", on_stats)
    # the conditions of the test: the memo answered evaluations, a tile ended its line search on one, and off is off
    assert on_stats["memo"] == "on" and on_stats["hits"] >= 1, on_stats
    assert on_stats["tiles_finished_on_hit"] >= 1, on_stats
    assert off_stats["memo"] == "off" and off_stats["hits"] == 0 and off_stats["tiles_hit"] == 0, off_stats
    assert on_stats["T"] == T * REP and on_stats["evaluations"] == off_stats["evaluations"] == int(ref["n_eval"].sum())
    assert np.isfinite(ref["nll"]).all()
    _same(ref, off, "memo off against the 4-wave build's")
    _same(ref, on, "memo on against memo off")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("wg_per_cu", [0, 1], ids=["4-wave", "8-wave"])
def test_memo_survives_slicing(case, wg_per_cu):
    """A slice of one evaluation on 48 resident workgroups: a tile is suspended after every computed evaluation and resumed by
    another workgroup, which finds the tile's memo in device memory and no factor of the tile in its own workspace."""
    ref, _ = _run(case, 0, False, False)
    unsliced, _ = _run(case, wg_per_cu, True, False)
    sliced, st = _run(case, wg_per_cu, True, True)
    print(case, wg_per_cu, "sliced:", st)
    assert st["hits"] >= 1 and st["tiles_finished_on_hit"] >= 1, st
    assert st["evaluations"] == int(ref["n_eval"].sum())
    _same(ref, unsliced, "memo on, unsliced, against memo off")
    _same(ref, sliced, "memo on, one evaluation per slice, against memo off")
