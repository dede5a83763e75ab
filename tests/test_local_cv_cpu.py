"""CPU: the orchestrator's cross-validation tables do not depend on how a run is cut into waves and engine calls, and the
fold layout of a tile (gpsat_amd/local_cv.py) against a plain loop."""
import numpy as np
import pandas as pd
import pytest

import test_cv_cpu
import test_cv_refit_cpu
from gpsat_amd.local_experts import BatchedLocalExpertOI
from test_cv_glue_cpu import CvGlueEngine
from test_cv_joint_cpu import JointEngine

BY = {"by": ["track"]}
FLAVOURS = {      # name: (configs, engine, constructor keywords, experts, cv rows, tables beside the plain run's)
    "loo": (test_cv_cpu._configs, test_cv_cpu.OracleCvEngine, dict(cv="loo"), 18, 2526, {"cv_preds"}),
    "by": (test_cv_cpu._configs, test_cv_cpu.OracleCvEngine, dict(cv=BY), 18, 2526, {"cv_preds"}),
    "joint": (test_cv_cpu._configs, JointEngine, dict(cv=BY, cv_joint=True), 18, 2526, {"cv_preds", "cv_folds"}),
    "glue": (test_cv_cpu._configs, CvGlueEngine, dict(cv=BY, cv_glue={"inference_radius": 4.0}), 18, 2526,
             {"cv_preds", "cv_glued", "cv_scores"}),
    "refit": (test_cv_refit_cpu._configs, test_cv_refit_cpu.OracleRefitEngine, dict(cv=dict(BY, refit=True)), 8, 727,
              {"cv_preds", "cv_params"}),
}
CUTS = [dict(store_every=7), dict(store_every=5, engine_chunk=3), dict(engine_chunk=1)]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_cv_tables_do_not_depend_on_waves_and_calls(flavour):
    """Every table of a run in several waves, in waves of several calls, and in calls of one tile is the one-wave run's,
    exactly (run_time, the seconds of the call, excepted): the per-wave accumulation and the whole-run concatenation."""
    configs, engine, kw, n_experts, n_rows, cv_tables = FLAVOURS[flavour]
    loc, data, model, pred, _ = configs()

    def run(**cut):
        out = BatchedLocalExpertOI(loc, data, model, pred, engine=engine(), dtype="f64", **kw).run(None, **cut)
        return {name: tab.drop(columns=["run_time"], errors="ignore") for name, tab in out.items()}
    one = run()
    assert cv_tables <= set(one) and len(one["run_details"]) == n_experts and len(one["cv_preds"]) == n_rows
    assert "cv_rows_skipped" in one["run_details"].columns and all(len(one[name]) for name in cv_tables)
    for cut in CUTS:
        got = run(**cut)
        assert list(got) == list(one), cut
        for name, tab in one.items():
            pd.testing.assert_frame_equal(got[name], tab, check_exact=True, obj=f"{name} with {cut}")


def _layout_by_loop(labels):
    codes = sorted({int(v) for v in labels if v >= 0})
    first = [next(i for i, v in enumerate(labels) if v == c) for c in codes]
    size = [sum(1 for v in labels if v == c) for c in codes]
    row_fold = [codes.index(int(v)) if v >= 0 else -1 for v in labels]
    return codes, first, size, row_fold


@pytest.mark.parametrize("labels", [
    [7, 2, 2, 40, 7, 2, 1000000],                   # gaps between the labels
    [-1, 5, -1, 3, 5, -3, 3, 3, -1],                # rows that are never held out, among and around the folds
    [4, 9, 4, 4, 0],                                # folds of one row
    [-1, -1, -2],                                   # no row is ever held out
    [],                                             # an empty tile
    [3],
    list(np.random.default_rng(0).integers(-2, 6, 97)),
], ids=["gaps", "negative", "one-row-fold", "none-held-out", "empty", "one-row", "random"])
def test_fold_layout_against_a_loop(labels):
    from gpsat_amd.local_cv import fold_layout
    lay = fold_layout(np.asarray(labels, dtype=np.int32))
    codes, first, size, row_fold = _layout_by_loop(labels)
    for got, want in zip((lay.codes, lay.first, lay.size, lay.row_fold), (codes, first, size, row_fold)):
        assert got.ndim == 1 and got.dtype.kind == "i"
        np.testing.assert_array_equal(got, np.asarray(want, dtype=np.int64))
