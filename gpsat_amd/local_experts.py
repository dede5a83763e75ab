"""BatchedLocalExpertOI -- the batched counterpart of the per-tile body of the reference's orchestrator.

Reference: ``LocalExpertOI.run`` (GPSat/local_experts.py:761-1279) loops serially over expert locations and, per
tile, selects observations (``DataLoader.local_data_select``, GPSat/dataloader.py:2352-2447), builds the
prediction coordinates (``PredictionLocations``, GPSat/prediction_locations.py:18-43,72-115,208-281), constructs a
model, applies constraints, optimises, evaluates the objective, predicts and appends rows to result tables
(``dict_of_array_to_table``, GPSat/local_experts.py:691-747) every ``store_every`` tiles (:500-548).

Here the SAME four config dicts are accepted (the in-memory subset listed below).  The work is organised as

  pass 1  tile membership for ALL expert locations (fp64, the reference's comparison semantics: ``ref + val``
          offsets, inclusive radius for observations, strict ``<`` for prediction locations, source row order;
          one GPU call with ``device_select=True``), scaling / de-meaning and the per-tile parameter vectors
          (defaults, loaded parameters, box constraints with move-within-tol) as whole-array operations -- no per-tile
          model object, no per-tile DataFrame;
  shard   with ``world_size > 1`` the global tile list is split by ``sharding.partition_tiles`` (LPT on
          E*N^3 + N^2*P); every rank packs and runs only its own tiles; no data-path collective;
  pass 2  waves of ``store_every`` expert locations, each cut per model profile into calls of ``engine_chunk`` tiles that
          go out on up to ``engine_workers`` engines while the next calls are packed; tables assembled with array
          operations and flushed to the store as one append-only, atomically committed part per wave (when a wave is
          one profile, its preds rows are written as pieces as its calls return) -- a fault at tile 99 999 loses at
          most the running wave, and a re-run resumes after the last committed wave (the reference's resume contract,
          local_experts.py:475-497,908-912);
  gather  with ``world_size > 1`` ONE gather (``sharding.gather_results``: RCCL over xGMI on the GPU node) returns
          per-tile hyper-parameters + predictions to rank 0, which assembles the tables in the reference's expert order.

Tables (``run_details``, ``preds``, ``lengthscales``, ``kernel_variance``, ``likelihood_variance``, ``expert_locs``,
``oi_config``; columns ``_dim_0``, ``f*``, ``f*_var``, ``y_var``, ``f_bar``, ``pred_loc_<c>`` ...) carry the expert
coordinates as (Multi)Index like the reference's.  The store is a directory of Apache Parquet parts (pandas pickles
when pyarrow is absent; pytables / HDF5 is not a dependency of this backend -- ``export_parquet`` / ``export_hdf5``).

Supported config subset (anything else raises ``NotImplementedError`` -- never a silent fallback):
  expert_loc_config : {"source": DataFrame | csv/parquet path, "sort_by": optional col(s)}
  data_config       : {"data_source": DataFrame | path, "obs_col": str, "coords_col": [..],
                       "local_select": [{"col", "comp", "val"}, ...],
                       "global_select": [static {"col","comp","val"} | dynamic {"loc_col","src_col","func"}]}
  pred_loc_config   : {"method": "expert_loc"} | {"method": "from_dataframe", "df": DataFrame, "max_dist": float,
                       "local_select": optional} | {"method": "from_source", "load_kwargs": {"source": DataFrame | path},
                       "max_dist": ..} | {"method": "shift_arrays", "<coord>": array, ...}
  model_config      : {"oi_model": "HipGPRModel" | "GPflowGPRModel" | "HipSGPRModel" | "GPflowSGPRModel" |
                                   {"path_to_model", "model_name"},
                       "init_params", "constraints", "optim_kwargs", "pred_kwargs", "params_to_store",
                       "load_params": {"file": store dir | dict of tables, "table_suffix": str, "param_names": [..],
                                       "index_adjust": {col: {"func": callable | "lambda ..."}}} |
                                      {<param>: value, ...}  (set directly on every tile)}
Dynamic ``global_select`` entries (``get_where_list``, GPSat/dataloader.py:2893-2978): for every ``local_select`` entry on
``loc_col`` an expert keeps the rows with ``src_col <comp> func(ref[loc_col], val)`` (pandas' comparison; ``func`` a callable or
a ``"lambda ..."`` string evaluated with ``np`` and ``pd``, called once per distinct ``(ref[loc_col], val)`` with the value
``rl.iloc[0, :].to_dict()`` gives).  ``src_col`` is rank-coded once per run and every threshold becomes a half-open rank interval,
so the criterion is exact for any ordered dtype; the entries on one ``src_col`` make one interval per expert, a device criterion of
its own (at most 4 device criteria in all).
Sparse experts (``oi_model`` GPflowSGPRModel / HipSGPRModel, fp64): the main profile runs through
``gpsat_sgpr_fit_predict_batch`` with no per-tile observation limit; ``init_params`` may hold ``num_inducing_points``
(default 500) and ``inducing_seed`` (default 0); every expert's inducing points are those HipSGPRModel picks
(``select_inducing_points`` with the expert's position in the expert locations), stored in the table ``inducing_points``
(``_dim_0`` inducing index, ``_dim_1`` coordinate, scaled coordinates); ``objective_value`` is the ELBO.  The replacement
profile stays an exact GP.
RationalQuadratic experts (``init_params.kernel == "RationalQuadratic"``, exact GP, fp64: ``dtype`` None or "f64", at most 3
coordinate columns): a fourth parameter, ``kernel_alpha`` (``init_params.kernel_kwargs.alpha``, default 1), with a table of its
own that is stored by default, read by ``load_params`` (file or direct value), carried in the ``previous`` running mean and
accepted by ``constraints``.
Experts with a trainable constant mean (``init_params.mean_function == "Constant"``, ``init_params.mean_func_kwargs.c``,
default 0; GPflow's mean_functions.Constant) are the same kind of profile -- one extra named parameter, here the table
``mean_constant`` (in scaled observation units), under the same rules: fp64, at most 3 coordinate columns, stored, loaded,
averaged and constrained like the others.  ``mean_function`` None and "Zero" are the zero mean; other names are not built.
Known noise variances per observation (``data_config["obs_var_col"]``, a column of the data source with every row's noise
variance in raw observation units, e.g. ``std**2 / count`` of binned data): the column travels with the observations into
every tile, is divided by ``obs_scale**2`` and is added to the diagonal of K beside ``likelihood_variance``; it is not
trained and no table changes.  Exact-GP experts in fp64 (``dtype`` None then means fp64).
What each of these kinds of expert, ``cv`` and ``pred_kwargs.full_cov`` cannot be combined with is the table of
gpsat_amd/variants.py; the constructor refuses such a config with the table's reason.
``replacement_*`` model settings for tiles below ``replacement_threshold`` observations are honoured (one engine call
per model profile and wave).  ``pred_kwargs.full_cov=True`` adds the table ``preds_2`` (``_dim_0``, ``_dim_1``, ``f*_cov``,
``y_cov``: what ``dict_of_array_to_table(concat=True, table="preds")`` makes of the 2-D arrays of the prediction dict,
local_experts.py:691-747, gpflow_models.py:245-263).
``pred_kwargs.gradient=True`` (exact-GP experts, fp64: ``dtype`` None then means fp64; kernels RBF, Matern32, Matern52; DESIGN.md
section 24) adds to ``preds``, for every column ``<c>`` of ``coords_col``, ``f*_grad_<c>`` and ``f*_grad_var_<c>``: the derivative
of the posterior mean with respect to that coordinate of the prediction location, and the posterior variance of the derivative.
Their units are those in which ``f*`` is stored there -- divided by ``obs_scale`` -- per RAW unit of the coordinate (``coords_scale``
is undone; with ``pred_kwargs.apply_scale=False`` the coordinate's unit is the one the prediction locations are given in): the
slope of the raw field is ``obs_scale * f*_grad_<c>``, its variance ``obs_scale**2 * f*_grad_var_<c>``.  The option holds for
the whole run (a replacement profile predicts the same columns), no other table changes, and the glue does not combine
these columns.  The constructor refuses what HipGPRModel.predict(gradient=True) refuses: fp32, Matern12 / RationalQuadratic
(also as a replacement profile's kernel), a constant mean, ``obs_var_col``, ``cv``, SGPR experts and ``full_cov``.
``pred_kwargs.hessian=True`` or a list of names from ``coords_col`` (exact-GP experts, fp64: ``dtype`` None then means fp64; kernels
RBF and Matern52), alone or beside ``gradient``, adds to ``preds``, for the pairs ``<a>``, ``<b>`` of those
columns in the order of ``coords_col`` (a, then b from a on), ``f*_hess_<a>_<b>`` and ``f*_hess_var_<a>_<b>``, the second derivative
of the posterior mean and its posterior variance, and ``f*_lap`` / ``f*_lap_var``, the sum of the ``f*_hess_<a>_<a>`` -- the
Laplacian over those columns -- with its own variance (which holds the covariances between them).  Units as ``gradient``'s: those
``f*`` is stored in, per RAW unit of each of the two coordinates.  The constructor refuses what it refuses for ``gradient``, and
Matern32 as well: the derivative of a Matern-3/2 process is not mean-square differentiable.  The glue does not combine these
columns (the second derivatives of the glued map need the second-order terms of the weights).
``load_params.previous=True`` (local_experts.py:1059-1064,1200-1217: every tile starts from an exponential moving average,
rho = 0.95, of the optima of the successfully optimised tiles before it) is a serial cross-tile dependency; its batched
definition here is CALL-LAGGED: all tiles of one engine call start from the average as it stood when the call was
issued, and the average is then advanced over that call's tiles in expert order.  ``engine_chunk=1`` reproduces the
reference's serial recurrence exactly; larger chunks trade its freshness for batching (sharded runs keep one average
per rank).
``cv="loo"`` / ``cv={"by": [columns of the data source]}`` (constructor; exact experts, ``dtype="f64"``, one shard): every
tile also predicts each of its own rows from the tile's other folds (the row alone / the rows with equal values in the ``by``
columns), at the tile's final parameters, from the factor it already has (theta is not fitted again
without the fold).  Table ``cv_preds``, committed with the waves like ``preds``: expert index; ``_dim_0`` the row's position in
the tile, ``obs_index`` its index label in the globally selected frame, the ``by`` columns, ``pred_loc_<c>`` its coordinates,
the observation under ``obs_col`` (raw), ``f*``, ``f*_var``, ``y_var`` and ``f_bar`` in the units of ``preds``: the held-out
prediction of the raw observation is ``f_bar + obs_scale * f*`` with variance ``obs_scale**2 * y_var``.  A fold above
``gpsat_max_cv_fold`` rows, and a row with a missing value in a ``by`` column, is not held out (NaN rows, counted in
``run_details.cv_rows_skipped``).
``cv={"by": [...], "refit": True, "start": "theta0" | "full"}`` (``dtype`` fp32 or fp64): every fold is FITTED AGAIN without
its rows, as the reference's cross-validation runs do (Engine.fit_predict_batch ``cv_refit``): the rows
a fold leaves are de-meaned again when the model's ``obs_mean`` is "local", a fold that leaves fewer than the run's
``min_obs`` rows is not fitted (its rows are NaN and counted in ``cv_rows_skipped``), and a fold has no size limit.
``cv_preds`` keeps its columns, ``f*`` still in the units of the tile's ``f_bar``.  Table ``cv_params``, committed with the
waves like ``cv_preds``, has one row per fold: expert index; the ``by`` columns' values; ``num_obs`` (rows fitted);
``lengthscales_<k>``, ``kernel_variance``, ``likelihood_variance`` in the units of the parameter tables;
``objective_value``; ``optimise_success``; and ``f_bar``, the de-meaning constant of the fold's own fit (the tile's plus
``obs_scale`` times the mean of the remaining rows).
``cv_glue={"inference_radius": r, "R": 3, "max_dist": d | None, "xprt_loc_cols": [...] | None}`` (constructor; needs ``cv``,
either kind): a row is predicted by every expert that selects it, and after the run these rows are glued into ONE held-out
prediction per observation, as the reference glues the overlapping predictions of its cross-validation runs (DESIGN.md
section 19; ``postprocessing.glue_cv_predictions``, the grouping and the weighted sums on the device): table ``cv_glued``
(``obs_index``, the ``by`` columns, ``pred_loc_<c>``, the raw observation, ``f*``, ``f*_var``, ``y_var`` in RAW units,
``n_experts``, ``z``), keyed on the observation's positional row in the selected frame, and table ``cv_scores``
(``postprocessing.score_cv_predictions``: overall and per combination of the ``by`` columns).  ``max_dist`` leaves out the
experts at that distance or beyond in ``xprt_loc_cols`` (default: the first two coordinate columns).  Both tables are of
the experts THIS run fitted: a resumed run glues what it ran, ``glue_cv_predictions`` on the store glues everything.
``cv_joint=True`` (constructor; needs ``cv={"by": [...]}``, with or without ``"refit"``; a refit run in fp64 only): the joint
log predictive density of every held-out fold, log N(obs_G; mean, covariance of the fold given the expert's other rows)
(Engine.fit_predict_batch ``cv_joint``).  Table ``cv_folds``, committed with the waves like
``cv_preds``, has one row per expert and fold: expert index; the ``by`` columns' values; ``n`` (rows of the fold); ``lpd`` in
RAW observation units (the device's value minus n log ``obs_scale``); and ``lpd_marginal``, the sum of the fold's univariate
terms from that expert's own ``cv_preds`` rows in raw units, so that the two stand side by side.  The other tables keep
their columns.  Refused with ``cv="loo"``: a one-row fold's joint density is the marginal one that ``cv_scores`` holds.
The code behind ``cv``, ``cv_glue`` and ``cv_joint`` is gpsat_amd/local_cv.py.
"""
from __future__ import annotations

import json
import os
import queue
import re
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from dataclasses import make_dataclass
from typing import Dict, List, Optional

import numpy as np
import pandas as pd
from scipy.spatial import cKDTree

from . import _lib as L
from . import local_cv as LC
from . import sharding
from . import variants as V
from .models import (HipGPRModel, HipSGPRModel, LIKELIHOOD_VARIANCE_LOWER_BOUND, SGPR_MODEL_NAMES, clamp_within,
                     select_inducing_points)

_COMPS = {">=": np.greater_equal, ">": np.greater, "==": np.equal, "<": np.less, "<=": np.less_equal}


def _profile_variants(init_params):
    """The rows of variants.VARIANTS that a model profile's ``init_params`` ask for: RationalQuadratic's alpha, or the constant
    of mean_function "Constant" -- ONE extra named parameter behind the reference's three."""
    ip = init_params or {}
    mf = ip.get("mean_function")
    if mf is not None and (not isinstance(mf, str) or mf not in ("Zero", "Constant")):
        raise NotImplementedError(f"init_params.mean_function {mf!r}: None, 'Zero' and 'Constant' are built")
    return ["rq"] * (ip.get("kernel") == "RationalQuadratic") + ["mean"] * (mf == "Constant")


MODEL_NAME = f"{HipGPRModel.__module__}.{HipGPRModel.__name__}"[:64]
SGPR_MODEL_NAME = f"{HipSGPRModel.__module__}.{HipSGPRModel.__name__}"[:64]
SGPR_INIT_KEYS = ("num_inducing_points", "inducing_seed")
DTYPES = ("f32", "f64")


# ----------------------------------------------------------------------------------------------------------
# selection (fp64, reference semantics)
# ----------------------------------------------------------------------------------------------------------
def _as_list(v):
    return [v] if isinstance(v, str) else list(v)


def _load_frame(src):
    if isinstance(src, pd.DataFrame):
        return src
    if isinstance(src, str):
        if src.endswith(".parquet"):
            return pd.read_parquet(src)
        if src.endswith(".csv"):
            return pd.read_csv(src)
    raise NotImplementedError(f"data source {type(src)}: this backend takes DataFrames, .csv or .parquet paths")


def data_select(df, selects):
    """Static row selection (GPSat/dataloader.py: data_select with {"col","comp","val"} entries)."""
    keep = np.ones(len(df), dtype=bool)
    for s in selects or []:
        if not {"col", "comp", "val"} <= set(s):
            raise NotImplementedError("only static global_select entries {col, comp, val} are supported")
        assert s["comp"] in _COMPS, f"comp: {s['comp']} is not valid"
        keep &= _COMPS[s["comp"]](df[s["col"]].values, s["val"])
    return df.loc[keep]


_DYNAMIC_KEYS = ["loc_col", "src_col", "func"]


def split_global_select(selects):
    """(static, dynamic) entries of a ``global_select`` list (GPSat/dataloader.py:2944-2960): an entry with col, comp and val
    is static, any other must have loc_col, src_col and func."""
    static, dynamic = [], []
    for gs in selects or []:
        if all(c in gs for c in ["col", "comp", "val"]):
            static.append(gs)
        else:
            assert all(c in gs for c in _DYNAMIC_KEYS), \
                f"dynamic where had keys: {list(gs.keys())}, must have: {_DYNAMIC_KEYS} "
            dynamic.append(gs)
    return static, dynamic


def _rank_interval(u: pd.Series, comp: str, c):
    """Positions of the sorted distinct values ``u`` for which pandas' ``u <comp> c`` holds, as a half-open interval."""
    m = np.asarray(_PD_COMPS[comp](u, c).to_numpy(dtype=bool, na_value=False))
    nz = np.flatnonzero(m)
    if len(nz) == 0:
        return 0.0, 0.0
    if nz[-1] + 1 - nz[0] != len(nz):
        raise NotImplementedError(f"dynamic global_select: '{comp} {c!r}' does not select one contiguous run of the sorted "
                                  f"values of its src_col")
    return float(nz[0]), float(nz[-1] + 1)


_PD_COMPS = {">=": lambda x, y: x >= y, ">": lambda x, y: x > y, "==": lambda x, y: x == y, "<": lambda x, y: x < y,
             "<=": lambda x, y: x <= y}


class DynamicSelect:
    """The dynamic ``global_select`` entries of a config as per-expert rank intervals (GPSat/dataloader.py:2893-2978,
    local_experts.py:426-472,971-985).

    Every ``local_select`` entry whose ``col`` is an entry's ``loc_col`` adds the criterion
    ``df[src_col] <comp> func(ref[loc_col], val)`` (``comp``, ``val`` from the local entry); an entry no local entry matches adds
    nothing.  ``src_col`` is rank-coded once (``code`` = position in its sorted distinct non-null values, null -> NaN) and the
    rows a threshold keeps are found by pandas' own comparison on the distinct values: a rank interval ``[lo, hi)``.  All
    criteria on one ``src_col`` are intersected, so an expert keeps a row iff ``lo <= code < hi`` -- bit for bit what the
    comparisons on the frame keep, for any ordered dtype."""

    def __init__(self, dynamic: List[dict], local_select: Optional[List[dict]], df: pd.DataFrame, loc_columns):
        self.items = []                          # (src_col, func, comp, val, loc_col)
        for gs in dynamic:
            assert local_select is not None, f"dynamic where provide: {gs}, however local_select is: {type(local_select)}"
            assert all(c in gs for c in _DYNAMIC_KEYS), \
                f"dynamic where had keys: {list(gs.keys())}, must have: {_DYNAMIC_KEYS} "
            loc_col = gs["loc_col"]
            assert loc_col in loc_columns, f"loc_col: {loc_col} not in ref_loc: {list(loc_columns)}"
            func = gs["func"]
            if isinstance(func, str):
                func = eval(func, {"np": np, "pd": pd})          # as the reference: eval with np and pd in scope
            if not callable(func):
                raise NotImplementedError(f"dynamic global_select func must be callable or a 'lambda ...' string: {gs['func']!r}")
            for ls in local_select:
                if isinstance(ls["col"], str) and ls["col"] == loc_col:
                    assert gs["src_col"] in df, f"col: '{gs['src_col']}' is not in coords: {list(df.columns)}"
                    assert ls["comp"] in _PD_COMPS, f"comp: {ls['comp']} is not valid"
                    self.items.append((gs["src_col"], func, ls["comp"], ls["val"], loc_col))
        self.src_cols = list(dict.fromkeys(it[0] for it in self.items))
        self.df = df
        self._codes = None

    def codes(self):
        """[n_src, M] fp64 rank codes (NaN for null) and, per src_col, its sorted distinct values (a Series)."""
        if self._codes is None:
            codes, uniq = np.empty((len(self.src_cols), len(self.df))), []
            for j, sc in enumerate(self.src_cols):
                cd, u = pd.factorize(self.df[sc], sort=True)
                codes[j] = np.where(cd < 0, np.nan, cd.astype(np.float64))
                uniq.append(pd.Series(u))
            self._codes = (codes, uniq)
        return self._codes

    def bounds(self, refs: pd.DataFrame) -> np.ndarray:
        """[T, n_src, 2] rank interval {lo, hi} of every expert (row of ``refs``) and src_col."""
        T = len(refs)
        out = np.empty((T, len(self.src_cols), 2))
        out[:, :, 0], out[:, :, 1] = -np.inf, np.inf
        if T == 0:
            return out
        _, uniq = self.codes()
        boxed = {}
        for src, func, comp, val, loc_col in self.items:
            if loc_col not in boxed:
                # the value the reference passes: rl.iloc[0, :].to_dict()[loc_col], once per distinct value
                ecode, _ = pd.factorize(refs[loc_col], use_na_sentinel=False)
                first = np.unique(ecode, return_index=True)[1]
                row_dtype = refs.iloc[int(first[0])].dtype
                if isinstance(row_dtype, np.dtype) and row_dtype.kind in "biuf":
                    col = refs[loc_col].to_numpy().astype(row_dtype)
                    vals = [col[i].item() for i in first]
                else:
                    vals = [refs.iloc[int(i)].to_dict()[loc_col] for i in first]
                boxed[loc_col] = (ecode, vals)
            ecode, vals = boxed[loc_col]
            j = self.src_cols.index(src)
            iv = np.array([_rank_interval(uniq[j], comp, func(v, val)) for v in vals]).reshape(-1, 2)[ecode]
            out[:, j, 0] = np.maximum(out[:, j, 0], iv[:, 0])
            out[:, j, 1] = np.minimum(out[:, j, 1], iv[:, 1])
        return out


class LocalSelector:
    """``DataLoader.local_data_select`` for many reference locations against one frame.

    1-D criteria: ``df[col] <comp> ref[col] + val``; multi-column criteria: Euclidean ball through
    ``KDTree.query_ball_point(x=ref[cols], r=val)`` -- inclusive of points exactly at ``r`` whatever ``comp`` says
    (GPSat/dataloader.py:2413-2444).  The KD-tree is built once (the reference rebuilds it per tile on the same
    frame).  Returns boolean masks, so source row order is kept (dataloader.py:2447).  ``interval_codes`` [n, M]: columns
    that ``select`` also restricts per expert to ``bounds[e, j, 0] <= code < bounds[e, j, 1]`` (``DynamicSelect``)."""

    def __init__(self, df: pd.DataFrame, local_select: List[dict], interval_codes: Optional[np.ndarray] = None):
        self.df = df
        self.interval_codes = interval_codes
        self.local_select = local_select or []
        self._trees = {}
        self._cols = {}
        for idx, ls in enumerate(self.local_select):
            col, comp = ls["col"], ls["comp"]
            if isinstance(col, str):
                assert col in df, f"col: {col} is not in data - {df.columns}"
                assert comp in _COMPS, f"comp: {comp} is not valid"
                self._cols[col] = df[col].values
            else:
                assert comp in ["<", "<="], "for multi dimensional values only less than comparison handled"
                for c_ in col:
                    assert c_ in df, f"column: {c_} is not in df.columns: {df.columns}"
                self._trees[idx] = cKDTree(df.loc[:, col].values)

    def mask(self, ref: Dict[str, float]) -> np.ndarray:
        select = np.ones(len(self.df), dtype=bool)
        for idx, ls in enumerate(self.local_select):
            col, comp = ls["col"], ls["comp"]
            if isinstance(col, str):
                assert col in ref, f"col: {col} is not in reference_location - {ref.keys()}"
                select &= _COMPS[comp](self._cols[col], ref[col] + ls["val"])
            else:
                for c_ in col:
                    assert c_ in ref, f"col: {col} is not in reference_location - {ref.keys()}"
                ids = self._trees[idx].query_ball_point(x=[ref[c_] for c_ in col], r=ls["val"])
                m = np.zeros(len(self.df), dtype=bool)
                m[ids] = True
                select &= m
        return select

    def select(self, refs: pd.DataFrame, bounds: Optional[np.ndarray] = None):
        """CSR (off [T+1], idx) of selected row POSITIONS for every row of ``refs`` (same layout as DeviceSelector)."""
        cols = list(refs.columns)
        vals = refs.values
        chunks, off = [], np.zeros(len(refs) + 1, dtype=np.int64)
        for i in range(len(refs)):
            m = self.mask(dict(zip(cols, vals[i])))
            if self.interval_codes is not None:
                for j, code in enumerate(self.interval_codes):
                    m &= (bounds[i, j, 0] <= code) & (code < bounds[i, j, 1])
            ids = np.nonzero(m)[0]
            chunks.append(ids)
            off[i + 1] = off[i] + len(ids)
        return off, (np.concatenate(chunks) if chunks else np.zeros(0, np.int64)).astype(np.int64)


class DeviceSelector:
    """The same membership as ``LocalSelector`` / ``max_dist_bool`` for ALL reference locations in one GPU call
    (``gpsat_select_batch``: fp64 predicates with the reference's arithmetic, bit-exact, source row order).

    ``local_select`` entries as in the reference; ``strict_ball=True`` gives the prediction-location semantics
    (strict ``<`` on the squared distance, GPSat/prediction_locations.py:37,43); ``interval_codes`` as for ``LocalSelector``
    (one interval criterion each, kind 2 of gpsat_select_batch_ex)."""

    def __init__(self, df: pd.DataFrame, local_select: List[dict], engine, strict_ball: bool = False,
                 interval_codes: Optional[np.ndarray] = None):
        self.engine = engine
        cols = []
        for ls in local_select:
            for c_ in ([ls["col"]] if isinstance(ls["col"], str) else list(ls["col"])):
                assert c_ in df, f"column: {c_} is not in df.columns: {df.columns}"
                if c_ not in cols:
                    cols.append(c_)
        self.cols = cols
        self.points = df.loc[:, cols].values.astype(np.float64)
        self.points_cm = np.ascontiguousarray(self.points.T)          # what the C ABI takes: column-major, made once
        self.n_ivl = 0 if interval_codes is None else len(interval_codes)
        if self.n_ivl:
            self.points_cm = np.ascontiguousarray(np.concatenate([self.points_cm, np.asarray(interval_codes, np.float64)]))
        self.criteria = []
        for ls in local_select:
            if isinstance(ls["col"], str):
                assert ls["comp"] in _COMPS, f"comp: {ls['comp']} is not valid"
                self.criteria.append(("cmp", cols.index(ls["col"]), ls["comp"], ls["val"]))
            else:
                assert ls["comp"] in ["<", "<="], "for multi dimensional values only less than comparison handled"
                if len(ls["col"]) > 3:
                    raise NotImplementedError("device ball selection takes 1..3 columns")
                self.criteria.append(("ball", [cols.index(c_) for c_ in ls["col"]], "<" if strict_ball else "<=", ls["val"]))
        for j in range(self.n_ivl):
            self.criteria.append(("interval", len(cols) + j, j))
        if self.n_ivl and len(self.criteria) > L.SEL_MAXCRIT:
            raise NotImplementedError(f"device selection takes at most {L.SEL_MAXCRIT} criteria (GPSAT_SEL_MAXCRIT); this "
                                      f"one needs {len(self.criteria)}: {len(local_select)} local_select entries and "
                                      f"{self.n_ivl} dynamic global_select interval(s)")

    def select(self, refs: pd.DataFrame, bounds: Optional[np.ndarray] = None):
        """refs: one row per expert with (at least) the columns used by the criteria; bounds [T, n_ivl, 2] with
        ``interval_codes``.  Returns CSR (off [T+1], idx [off[-1]]) of selected row POSITIONS of the frame, ascending per expert."""
        for c_ in self.cols:
            assert c_ in refs, f"col: {c_} is not in reference_location - {list(refs.columns)}"
        r = refs.loc[:, self.cols].values.astype(np.float64)
        if self.n_ivl:
            r = np.concatenate([r, np.zeros((len(r), self.n_ivl))], axis=1)      # the code columns have no reference value
        return self.engine.select_batch(None, r, self.criteria, points_cm=self.points_cm,
                                        bounds=bounds if self.n_ivl else None)


def max_dist_bool(loc: np.ndarray, ref_loc: np.ndarray, max_dist: float) -> np.ndarray:
    """``_max_dist_bool`` (GPSat/prediction_locations.py:18-43): per-dimension pre-filter, then the STRICT test
    sum((loc - ref)^2) < max_dist^2, in fp64."""
    d = loc - ref_loc[None, :]
    m2 = max_dist * max_dist
    out = np.all(d * d < m2, axis=1)
    d2 = np.sum(d ** 2, axis=1)
    return out & (d2 < m2)


class PredictionLocations:
    """Prediction coordinates per expert (GPSat/prediction_locations.py:72-115,182-281):

    ``expert_loc``      the expert location itself;
    ``shift_arrays``    the mesh of per-coordinate shift arrays (``<coord>=array`` keywords, missing coordinates shift
                        by 0; built once, :182-206) added to the expert location;
    ``from_dataframe``  rows of a frame within ``max_dist`` (strict) over the columns present in the frame; dimensions
                        missing from the frame are filled from the expert location (:262-271); optional
                        ``local_select`` afterwards (:106-111);
    ``from_source``     ``load_kwargs={"source": DataFrame | csv | parquet}`` loaded once, duplicates dropped, then as
                        ``from_dataframe`` (:83-101)."""

    def __init__(self, method="expert_loc", coords_col=None, df=None, max_dist=None, local_select=None,
                 load_kwargs=None, Xout=None, **kw):
        self.coords_col = list(coords_col)
        if method == "from_source":
            assert load_kwargs is not None, \
                "calling PredictionLocations object with method='from_source', however 'load_kwargs' is missing"
            extra = set(load_kwargs) - {"source"}
            if extra:
                raise NotImplementedError(f"from_source load_kwargs {sorted(extra)}: only 'source' is supported")
            df = _load_frame(load_kwargs["source"]).drop_duplicates()
            method = "from_dataframe"
        if method not in ("expert_loc", "from_dataframe", "shift_arrays"):
            raise ValueError(f"prediction location method '{method}' is not implemented")
        self.method, self.max_dist, self.local_select = method, max_dist, local_select
        if method == "shift_arrays":
            unknown = set(kw) - set(self.coords_col)
            if unknown:
                raise NotImplementedError(f"shift_arrays: {sorted(unknown)} are not coordinate columns")
            if Xout is None:
                axes = [np.atleast_1d(np.asarray(kw.get(c, np.zeros(1)), dtype=np.float64)) for c in self.coords_col]
                for a in axes:
                    assert a.ndim == 1
                mesh = np.meshgrid(*axes, indexing="ij")
                Xout = np.stack([m.reshape(-1) for m in mesh], axis=1)
            self.shifts = np.asarray(Xout, dtype=np.float64)
            assert self.shifts.ndim == 2 and self.shifts.shape[1] == len(self.coords_col)
        elif kw:
            raise NotImplementedError(f"unsupported pred_loc_config keys: {sorted(kw)}")
        if method == "from_dataframe":
            df = _load_frame(df)
            self.found = [c for c in self.coords_col if c in df.columns]
            self.fc_loc = [self.coords_col.index(c) for c in self.found]
            self.vals = df.loc[:, self.found].values.astype(np.float64)
            self.missing = [i for i, c in enumerate(self.coords_col) if c not in self.found]
            self._sel = LocalSelector(pd.DataFrame(self.vals, columns=self.found), local_select) if local_select else None

    def __call__(self, expert_loc: np.ndarray) -> np.ndarray:
        """expert_loc: (D,) fp64 in the order of coords_col.  Returns (P, D) fp64."""
        if self.method == "expert_loc":
            return expert_loc[None, :].copy()
        if self.method == "shift_arrays":
            return self.shifts + expert_loc[None, :]
        b = max_dist_bool(self.vals, expert_loc[self.fc_loc], self.max_dist) if self.max_dist is not None \
            else np.ones(len(self.vals), dtype=bool)
        if self._sel is not None:
            b = b & self._sel.mask({c: expert_loc[i] for i, c in enumerate(self.coords_col)})
        return self._rows(np.nonzero(b)[0], expert_loc)

    def _rows(self, ids, expert_loc):
        out = np.empty((len(ids), len(self.coords_col)))
        out[:, self.fc_loc] = self.vals[ids]
        out[:, self.missing] = expert_loc[self.missing]
        return out

    def batch(self, locs: np.ndarray, engine=None):
        """All experts at once: a ``RaggedRows`` (``[i]`` is expert i's (P_i, D) array).  With an engine the ``max_dist``
        filter of ``from_dataframe`` runs as ONE ``gpsat_select_batch`` call (strict ball, bit-identical membership) and the
        coordinates are gathered in one piece (a Python-level gather per expert cost 4 us x 16 384 experts = 0.07 s)."""
        D = len(self.coords_col)
        if self.method == "from_dataframe" and engine is not None and self.max_dist is not None and self._sel is None \
                and 1 <= len(self.found) <= 3:
            frame = pd.DataFrame(self.vals, columns=self.found)
            ds = DeviceSelector(frame, [{"col": list(self.found), "comp": "<", "val": self.max_dist}], engine,
                                strict_ball=True)
            off, idx = ds.select(pd.DataFrame(locs[:, self.fc_loc], columns=self.found))
            cat = np.empty((len(idx), D))
            cat[:, self.fc_loc] = self.vals[idx]
            if self.missing:
                cat[:, self.missing] = np.repeat(locs[:, self.missing], np.diff(off), axis=0)
            return RaggedRows(cat, off)
        rows = [self(locs[i]) for i in range(len(locs))]
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        return RaggedRows(np.concatenate(rows) if len(rows) else np.zeros((0, D)), off)


class RaggedRows:
    """Row blocks of unequal length kept back to back: ``cat`` (sum P_i, D) and ``off`` (T + 1).  Reads like a list of
    arrays; ``take`` gathers the blocks of many items without a Python loop."""

    def __init__(self, cat: np.ndarray, off: np.ndarray):
        self.cat, self.off = cat, np.asarray(off, dtype=np.int64)
        self.counts = np.diff(self.off)

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, i):
        return self.cat[self.off[i]:self.off[i + 1]]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def take(self, items) -> np.ndarray:
        """The blocks of ``items`` (positions, any order) back to back."""
        items = np.asarray(items, dtype=np.int64)
        if len(items) == 0:
            return self.cat[:0]
        if bool(np.all(np.diff(items) == 1)):
            return self.cat[self.off[items[0]]:self.off[items[-1] + 1]]
        cnt = self.counts[items]
        tot = int(cnt.sum())
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        rows = np.arange(tot) - np.repeat(start, cnt) + np.repeat(self.off[items], cnt)
        return self.cat[rows]


# ----------------------------------------------------------------------------------------------------------
# result tables (GPSat/local_experts.py:691-747, GPSat/utils.py:1437-1495) and their store
# ----------------------------------------------------------------------------------------------------------
def _index_for(coords_col, loc_rows: np.ndarray):
    if len(coords_col) == 1:
        return pd.Index(loc_rows[:, 0], name=coords_col[0])
    return pd.MultiIndex.from_arrays([loc_rows[:, i] for i in range(loc_rows.shape[1])], names=coords_col)


def _index_for_repeated(coords_col, loc_rows: np.ndarray, counts):
    """``_index_for(coords_col, np.repeat(loc_rows, counts, axis=0))`` without factorising the repeated rows: the levels come
    from the (few) distinct locations, the codes are repeated (a tenth of the time for the 210 k rows of a preds table)."""
    counts = np.asarray(counts)
    if len(coords_col) == 1 or len(loc_rows) == 0:
        return _index_for(coords_col, np.repeat(loc_rows, counts, axis=0))
    levels, codes = [], []
    for i in range(loc_rows.shape[1]):
        c_, l_ = pd.factorize(loc_rows[:, i], sort=True)
        levels.append(l_)
        codes.append(np.repeat(c_, counts))
    return pd.MultiIndex(levels=levels, codes=codes, names=coords_col, verify_integrity=False)


_PART_RE = re.compile(r"^(?P<table>[^.].*)\.w(?P<k>\d{6})\.r(?P<r>\d{3})(\.p(?P<piece>\d{2}))?\.(?P<ext>parquet|pkl)$")
_PIECE_ROWS = 65536            # a table of a wave longer than this is written as up to _PIECE_MAX row pieces, in parallel
_PIECE_MAX = 4
_writers = []


def _writer_pool():
    if not _writers:
        from concurrent.futures import ThreadPoolExecutor
        _writers.append(ThreadPoolExecutor(max_workers=_PIECE_MAX))
    return _writers[0]
_MARK_RE = re.compile(r"^_wave\.w(?P<k>\d{6})\.r(?P<r>\d{3})\.ok$")
_WHOLE_RE = re.compile(r"^(?P<table>[^.].*)\.(?P<ext>parquet|pkl)$")


def _have_pyarrow():
    try:
        import pyarrow  # noqa: F401
        return True
    except Exception:
        return False


def _read_part(path):
    if path.endswith(".parquet"):
        df = pd.read_parquet(path)
        # pandas keeps the (Multi)Index in the parquet metadata; a frame written without rows comes back the same way
        return df
    return pd.read_pickle(path)


class ResultStore:
    """Directory store of table parts: Apache Parquet (pyarrow) by default -- readable by ``pandas.read_parquet`` /
    pyarrow / any parquet tool, independent of the pandas version, safe to load -- or pandas pickles (``fmt="pickle"``,
    and the fallback when pyarrow is absent; stores written by earlier versions stay readable).  HDF5 / pytables, the
    reference's container, is not a dependency of this backend (``export_hdf5`` converts when pytables is installed).

    Append-only: every flush (``write_wave``) adds ONE new part per table, ``<table>.w<k>.r<rank>.<ext>`` -- a long table
    (the predictions of a wave) as up to four row pieces ``<table>.w<k>.r<rank>.p<j>.<ext>`` written by as many threads
    (pyarrow releases the GIL; the parquet writer itself is single-threaded) and read back in order -- and
    commits the wave by writing the marker ``_wave.w<k>.r<rank>.ok`` last (files are written to a temporary name and
    renamed, so a part is either complete or absent).  Parts without their marker -- a run killed mid-flush -- are
    ignored by readers and removed by the next run.  Nothing already written is ever re-read or re-written by an
    append (the reference's HDFStore.append, local_experts.py:526-548).  ``put`` writes a whole table
    (``<table>.<ext>``, the HDFStore.put(append=False) of the smoothing step)."""

    def __init__(self, path: Optional[str], rank: int = 0, fmt: Optional[str] = None):
        self.path = path
        self.rank = int(rank)
        if fmt is None:
            fmt = "parquet" if _have_pyarrow() else "pickle"
        if fmt not in ("parquet", "pickle"):
            raise ValueError("fmt must be 'parquet' or 'pickle'")
        if fmt == "parquet" and not _have_pyarrow():
            raise ImportError("fmt='parquet' needs pyarrow")
        self.fmt = fmt
        self.ext = "parquet" if fmt == "parquet" else "pkl"
        self._open_k = None
        if path:
            os.makedirs(path, exist_ok=True)

    def _whole(self, table):
        """Path of the whole-table file of ``table`` (either format), or None."""
        for ext in ("parquet", "pkl"):
            f = os.path.join(self.path, f"{table}.{ext}")
            if os.path.exists(f):
                return f
        return None

    def _scan(self):
        parts, marks = {}, set()
        for f in os.listdir(self.path):
            if f.startswith(".tmp."):                       # unfinished temporary of some flush: never a table part
                continue
            m = _MARK_RE.match(f)
            if m:
                marks.add((int(m["k"]), int(m["r"])))
                continue
            m = _PART_RE.match(f)
            if m:
                parts.setdefault(m["table"], []).append((int(m["k"]), int(m["r"]), f))
        return parts, marks

    def drop_uncommitted(self):
        """Remove part files of this rank that no marker commits (left by a run that died during a flush), and this rank's
        stale temporaries."""
        if not self.path:
            return
        parts, marks = self._scan()
        for plist in parts.values():
            for k, r, f in plist:
                if r == self.rank and (k, r) not in marks:
                    os.remove(os.path.join(self.path, f))
        # temporaries carry their writer's RANK (`.tmp.r<rank>.<pid>.<name>`): a rank only ever removes its own -- ranks that
        # share the directory from different PID namespaces or hosts (one container per rank, NFS) cannot see each other's
        # PIDs, and a late starter must not delete another rank's file in flight.  Temporaries of older versions
        # (`.tmp.<pid>.<name>`) are removed once they are an hour old.
        mine = f".tmp.r{self.rank}."
        for f in os.listdir(self.path):
            stale = False
            if f.startswith(mine):
                pid = f[len(mine):].split(".")[0]
                stale = not (pid.isdigit() and int(pid) == os.getpid())
            elif f.startswith(".tmp.") and not f.startswith(".tmp.r"):
                try:
                    stale = time.time() - os.path.getmtime(os.path.join(self.path, f)) > 3600.0
                except OSError:
                    stale = False
            if stale:
                try:
                    os.remove(os.path.join(self.path, f))
                except FileNotFoundError:
                    pass

    def _atomic_write(self, df, name):
        tmp = os.path.join(self.path, f".tmp.r{self.rank}.{os.getpid()}.{name}")
        if name.endswith(".parquet"):
            # pyarrow directly, without dictionary encoding and column statistics: a part is written once and read whole, and
            # the encoder's dictionaries and min / max passes were four fifths of pandas' to_parquet on the preds table
            # (0.149 -> 0.032 s for 210 k rows; the file is also 13 % smaller)
            import pyarrow as pa
            import pyarrow.parquet as pq
            pq.write_table(pa.Table.from_pandas(df, preserve_index=True), tmp, compression="snappy", use_dictionary=False,
                           write_statistics=False)
        else:
            df.to_pickle(tmp)
        os.replace(tmp, os.path.join(self.path, name))

    def _wave_number(self):
        """The number of the wave being written (fixed by its first piece or, without pieces, by ``write_wave``)."""
        if self._open_k is None:
            _, marks = self._scan()
            self._open_k = 1 + max([kk for kk, r in marks if r == self.rank], default=0)
        return self._open_k

    def write_piece(self, name: str, j: int, df: pd.DataFrame):
        """Row piece ``j`` (0, 1, ...; in row order) of table ``name`` of the wave that the next ``write_wave`` commits: the
        rows of a long table that are ready before the wave is (the predictions of an engine call), written while the wave
        still runs.  Uncommitted like any part until the marker is there."""
        if not self.path or df is None or not len(df):
            return
        assert 0 <= j < 100
        self._atomic_write(df, f"{name}.w{self._wave_number():06d}.r{self.rank:03d}.p{j:02d}.{self.ext}")

    def write_wave(self, tables: Dict[str, pd.DataFrame], prewritten=None):
        """One committed part per non-empty table (``prewritten``: {table: rows} of the tables whose rows went out as
        ``write_piece`` pieces -- they are committed by the same marker)."""
        if not self.path:
            return
        prewritten = dict(prewritten or {})
        tables = {k: v for k, v in tables.items() if v is not None and len(v)}
        if not tables and not prewritten:
            self._open_k = None
            return
        k = self._wave_number()
        self._open_k = None
        jobs = []
        for name, df in tables.items():
            if name in prewritten:
                continue
            stem = f"{name}.w{k:06d}.r{self.rank:03d}"
            npiece = min(_PIECE_MAX, -(-len(df) // _PIECE_ROWS)) if self.fmt == "parquet" else 1
            if npiece <= 1:
                jobs.append((df, f"{stem}.{self.ext}"))
            else:
                cut = np.linspace(0, len(df), npiece + 1).astype(np.int64)
                jobs += [(df.iloc[cut[j]:cut[j + 1]], f"{stem}.p{j:02d}.{self.ext}") for j in range(npiece)]
        if len(jobs) == 1:
            self._atomic_write(*jobs[0])
        elif jobs:
            for f_ in [_writer_pool().submit(self._atomic_write, d_, n_) for d_, n_ in jobs]:
                f_.result()
        mark = os.path.join(self.path, f"_wave.w{k:06d}.r{self.rank:03d}.ok")
        with open(mark + ".tmp", "w") as f:
            rows = {n: int(len(d)) for n, d in tables.items()}
            rows.update({n: int(r) for n, r in prewritten.items()})
            f.write(json.dumps({"tables": sorted(rows), "rows": rows}))
        os.replace(mark + ".tmp", mark)

    def append(self, table, df: pd.DataFrame):
        self.write_wave({table: df})

    def put(self, table, df: pd.DataFrame):
        """Whole-table write: replaces the table and every part of it."""
        if not self.path:
            return
        parts, _ = self._scan()
        for _, _, f in parts.get(table, []):
            os.remove(os.path.join(self.path, f))
        old = self._whole(table)
        self._atomic_write(df, f"{table}.{self.ext}")
        if old is not None and not old.endswith("." + self.ext):
            os.remove(old)

    def read(self, table) -> Optional[pd.DataFrame]:
        if not self.path:
            return None
        parts, marks = self._scan()
        pieces = []
        whole = self._whole(table)
        if whole is not None:
            pieces.append(_read_part(whole))
        for k, r, f in sorted(parts.get(table, [])):
            if (k, r) in marks:
                pieces.append(_read_part(os.path.join(self.path, f)))
        if not pieces:
            return None
        return pieces[0] if len(pieces) == 1 else pd.concat(pieces)

    def table_names(self) -> List[str]:
        if not self.path:
            return []
        parts, marks = self._scan()
        names = {t for t, pl in parts.items() if any((k, r) in marks for k, r, _ in pl)}
        for f in os.listdir(self.path):
            if f.startswith(".tmp.") or _PART_RE.match(f):
                continue
            m = _WHOLE_RE.match(f)
            if m:
                names.add(m["table"])
        return sorted(names)

    def tables(self) -> Dict[str, pd.DataFrame]:
        return {t: self.read(t) for t in self.table_names()}


def export_parquet(store_path: str, out_dir: str, expert_order: bool = True) -> List[str]:
    """ONE parquet file per table (``<out_dir>/<table>.parquet``, rows in expert order), from a store of either format:
    what a consumer outside this package reads with ``pandas.read_parquet``.  Counterpart of handing the reference's
    HDF5 results file to downstream tooling (``get_results_from_h5file``, GPSat/local_experts.py:1467-1620)."""
    if not _have_pyarrow():
        raise ImportError("export_parquet needs pyarrow")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name, df in get_results(store_path, expert_order=expert_order).items():
        if df is None:
            continue
        f = os.path.join(out_dir, f"{name}.parquet")
        df.to_parquet(f, engine="pyarrow", index=True)
        written.append(f)
    cfgs = [f for f in os.listdir(store_path) if f.startswith("oi_config") and f.endswith(".json")]
    for f in cfgs:
        with open(os.path.join(store_path, f)) as src, open(os.path.join(out_dir, f), "w") as dst:
            dst.write(src.read())
    return written


def export_hdf5(store_path: str, h5_path: str, expert_order: bool = True):
    """The store as ONE HDF5 file in the reference's layout (``pd.HDFStore`` tables keyed by table name, appendable
    format with data columns), for GPSat's own readers (``get_results_from_h5file``, GPSat/local_experts.py:1467).  Needs
    pytables, which is not a dependency of this backend: raises ImportError when it is absent (it is absent from the
    build and GPU images, so this path has not been executed there)."""
    try:
        import tables  # noqa: F401
    except Exception as e:                                   # pragma: no cover
        raise ImportError("export_hdf5 needs pytables (pip install tables)") from e
    with pd.HDFStore(h5_path, mode="w") as st:               # pragma: no cover
        for name, df in get_results(store_path, expert_order=expert_order).items():
            if df is not None and len(df):
                st.put(name, df, format="table", data_columns=True)


def get_results(store_path: str, expert_order: bool = False) -> Dict[str, pd.DataFrame]:
    """Counterpart of ``get_results_from_h5file`` (GPSat/local_experts.py:1467): all tables of a store.  With
    ``expert_order=True`` the rows of every table are put in the order of the ``expert_locs`` table (a sharded run
    commits its parts in (wave, rank) order)."""
    tabs = ResultStore(store_path).tables()
    if expert_order:
        xl = next((v for k, v in tabs.items() if k.startswith("expert_locs")), None)
        if xl is not None:
            for k, v in tabs.items():
                if k.startswith("expert_locs") or v.index.names != xl.index.names or len(v) == 0:
                    continue
                pos = xl.index.get_indexer(v.index)
                tabs[k] = v.iloc[np.argsort(pos, kind="stable")]
    return tabs


def check_prev_oi_config(prev_oi_config: dict, oi_config: dict, skip_valid_checks_on=None):
    """What ``GPSat.utils.check_prev_oi_config`` (utils.py:1276-1327) is documented to do: raise when a key of the
    current configuration, other than those in ``skip_valid_checks_on``, differs from the one a previous run stored
    for the same tables.  (The reference's final ``assert len(bad_keys)`` tests the opposite of its docstring.)"""
    skip = set(skip_valid_checks_on or [])
    bad = [k for k, v in oi_config.items() if k not in skip and prev_oi_config.get(k) != v]
    assert not bad, f"the following keys did not have values that matched exactly: {bad}"


def _adjust_func(spec):
    f = spec.get("func") if isinstance(spec, dict) else spec
    if callable(f):
        return f
    if isinstance(f, str) and f.lstrip().startswith("lambda"):
        return eval(f)                                     # the reference's config_func does the same (utils.py:311)
    raise NotImplementedError("load_params.index_adjust takes {col: {'func': callable or 'lambda x: ...'}}")


# The per-tile result matrix ``fixed`` [n, H + _N_RES] (H = variants.n_hyper parameters) holds, after the parameters, these columns at
# ``H + <name>``.  It stays one float64 matrix so that ``sharding.gather_arrays`` carries it in one piece.
_NLL, _STATUS, _N_EVAL, _N_ITER, _SECONDS, _OBS_MEAN = range(6)
_N_RES = 6


# One model profile (main, replacement) as a run uses it: what a model decides without the tile's rows (default parameters,
# box, trainable mask, the clamp's (slice, tol) pairs, scales, local mean) and the profile's engine and predict settings.
_Profile = make_dataclass("_Profile", [
    "theta_default", "lo", "hi", "trainable", "clamp", "coords_scale", "obs_scale", "local_mean", "unconstrained_noise",
    "device", "sgpr", "n_inducing", "inducing_seed", "kernel", "max_iter", "eng_kw", "optimiser", "apply_scale", "full_cov",
    "pred_grad", "pred_hess"])


def _pred_hess_arg(pf):
    """Engine.fit_predict_batch's ``pred_hess`` for a profile: its coordinates, and Laplacian weights 1 / coords_scale_a^2 (1
    without apply_scale) on them, so that the Laplacian is taken in the raw coordinates."""
    cs = np.asarray(pf.coords_scale if pf.apply_scale else np.ones_like(pf.coords_scale), dtype=np.float64).reshape(-1)
    return {"dims": list(pf.pred_hess), "lap_weight": [1.0 / cs[a] ** 2 if a in pf.pred_hess else 0.0 for a in range(len(cs))]}


# Pass 1: the expert locations of a run -- item i is expert ex[i] at locs[i]; its observation rows are idx[off[i]:off[i + 1]]
# of coords_all / obs_all (fp64), its prediction coordinates pcs[i]; kind 0 skipped silently, 1 stub row, 2 tile, 3 error
# row; prof_id indexes profiles; theta0, lo, hi [T, H] its start parameters and box.
_Plan = make_dataclass("_Plan", [
    "ex", "locs", "off", "idx", "n_obs", "pcs", "n_pred", "kind", "prof_id", "profiles", "theta0", "lo", "hi", "save_params",
    "want_cov", "coords_all", "obs_all", "config_id", "table_suffix", "optimise", "predict", "var_all", "min_obs"])
# var_all: the noise variance of every row of obs_all (data_config["obs_var_col"], raw observation units), or None;
# min_obs: the run's option (a tile below it is a stub row; a refitted cv fold that leaves fewer rows is not fitted)


# ----------------------------------------------------------------------------------------------------------
# the batched orchestrator
# ----------------------------------------------------------------------------------------------------------
class BatchedLocalExpertOI:
    def __init__(self, expert_loc_config: dict, data_config: dict, model_config: dict, pred_loc_config: dict,
                 engine=None, device_select: bool = False, dtype: Optional[str] = None, cv=None, cv_glue=None, cv_joint=False):
        self.config = {"locations": _jsonable(expert_loc_config), "data": _jsonable(data_config),
                       "model": _jsonable(model_config), "pred_loc": _jsonable(pred_loc_config)}
        self.dtype = self._ask_variants(data_config, model_config, dtype, cv)
        # cross-validation (local_cv.py): ``cv`` the parsed options, None in a run without it
        self.cv = LC.parse_options(cv, cv_glue, cv_joint, data_config, self.dtype)
        self.cv_glue = self.cv.glue if self.cv is not None else None
        if self.cv_glue is not None:
            self.config["cv_glue"] = dict(self.cv_glue)
        if self.cv is not None and self.cv.joint:
            self.config["cv_joint"] = True
        self._load_data(data_config)
        self._load_expert_locs(expert_loc_config, data_config, device_select)
        self._set_profiles(model_config)
        self._set_load_params(model_config.get("load_params"))
        # ---- prediction locations (local_experts.py:254-264)
        plc = dict(pred_loc_config or {"method": "expert_loc"})
        self.pred_loc = PredictionLocations(coords_col=self.coords_col, **plc)
        from .engine import default_engine
        self.engine = engine if engine is not None else default_engine()
        self.engine_workers = 2          # engines (HIP streams) that take the chunks of a wave in turn; see _ShardRunner.run
        self._extra_engines = []
        self.pack_threads = 4            # host threads that pack one engine call's arrays
        self._pack_pool = None
        # tile membership for all experts in one GPU call (bit-identical to the host selector)
        self.device_select = device_select
        self.timings = {}

    def _ask_variants(self, data_config, model_config, dtype, cv):
        """Which rows of variants.VARIANTS the four configs ask for, and whether the table allows them together at this
        dtype and number of coordinate columns.  Sets ``sgpr``, ``rq``, ``extra``, ``param_names``, ``H`` and ``obs_var_col``;
        returns the run's dtype."""
        om = model_config.get("oi_model", "HipGPRModel")
        name = om["model_name"] if isinstance(om, dict) else om
        if name not in ("HipGPRModel", "GPflowGPRModel") + SGPR_MODEL_NAMES:
            raise NotImplementedError(f"oi_model '{name}': the batched backend builds the exact-GP and SGPR experts only")
        self.sgpr = name in SGPR_MODEL_NAMES
        # known noise variances per observation: a column of the data source that travels with the observations
        self.obs_var_col = data_config.get("obs_var_col")
        if self.obs_var_col is not None and not isinstance(self.obs_var_col, str):
            raise ValueError(f"data_config.obs_var_col must be one column name, got {self.obs_var_col!r}")
        self._variants = _profile_variants(model_config.get("init_params"))
        kind = self._variants + ["noise"] * (self.obs_var_col is not None) + ["sgpr"] * self.sgpr
        # dtype None: fp32 for exact-GP experts, fp64 for the kinds of expert that are built in fp64 only (an explicit fp32
        # is refused below)
        # pred_kwargs.gradient (either profile's) holds for the run: the gradient of the posterior mean beside every prediction
        self.pred_grad = any(bool((model_config.get(k) or {}).get("gradient", False)) for k in ("pred_kwargs", "replacement_pred_kwargs"))
        # pred_kwargs.hessian in the same way: True, or names from coords_col -- kept as sorted coordinate indices, None: not asked
        self.pred_hess = None
        for k in ("pred_kwargs", "replacement_pred_kwargs"):
            hs = (model_config.get(k) or {}).get("hessian", False)
            if self.pred_hess is None and hs is not False and hs is not None:
                cc = list(data_config["coords_col"])
                names = cc if hs is True else ([hs] if isinstance(hs, str) else list(hs))
                if not names or any(n not in cc for n in names):
                    raise ValueError(f"{k}.hessian: True, or names from coords_col {cc}, got {hs!r}")
                self.pred_hess = sorted(set(cc.index(n) for n in names))
        if dtype is None:
            dtype = "f32" if all("f32" in V.VARIANTS[k].dtypes for k in kind) and not self.pred_grad and self.pred_hess is None else "f64"
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f32', 'f64' (the reference's precision) or None")
        # one check per model profile: the main one carries the kind of expert; the replacement stays a plain exact GP
        held_out = [] if cv is None else ["cv_refit" if isinstance(cv, dict) and cv.get("refit") else "cv"]
        replaced = ["replacement"] * (model_config.get("replacement_threshold") is not None)
        profiles = [(kind, model_config.get("pred_kwargs"))]
        if replaced:
            profiles.append((_profile_variants(model_config.get("replacement_init_params")), model_config.get("replacement_pred_kwargs")))
        D = len(data_config["coords_col"])
        for asked, pk in profiles:
            why = V.why_refused(asked + held_out + replaced + ["full_cov"] * bool((pk or {}).get("full_cov", False)), dtype, D,
                                dims="coordinate columns")
            if why:
                raise NotImplementedError(why)
        if self.pred_grad or self.pred_hess is not None:
            main_ip = model_config.get("init_params") or {}
            rip = model_config.get("replacement_init_params")
            kernels = [main_ip.get("kernel", "Matern32")] + [(main_ip if rip is None else rip).get("kernel", "Matern32")] * bool(replaced)
            refusal = V.why_refused_pred_grad if self.pred_hess is None else V.why_refused_pred_hess
            for (asked, pk), kern in zip(profiles, kernels):
                why = refusal(asked + held_out + ["full_cov"] * bool((pk or {}).get("full_cov", False)), dtype, kern)
                if why:
                    raise NotImplementedError(why)
        row = next((V.VARIANTS[k] for k in self._variants if V.VARIANTS[k].param), None)
        self.extra = (row.param, row.arg) if row else None          # the ONE extra named parameter and what asks for it
        self.rq = "rq" in self._variants
        self.param_names = V.param_names(self._variants)
        self.H = V.n_hyper(D, self._variants)
        return dtype

    def _load_data(self, data_config):
        """The globally selected frame (local_experts.py:266-290) and, with ``cv`` by columns, the fold code of every row."""
        self.obs_col = data_config["obs_col"]
        self.coords_col = list(data_config["coords_col"])
        if isinstance(self.obs_col, (list, tuple)):
            assert len(self.obs_col) == 1
            self.obs_col = self.obs_col[0]
        self.local_select = data_config.get("local_select", [])
        static_gs, self._dynamic_gs = split_global_select(data_config.get("global_select"))
        df = data_select(_load_frame(data_config["data_source"]), static_gs)
        self.df = df
        if self.obs_var_col is not None and self.obs_var_col not in df.columns:
            raise KeyError(f"obs_var_col: column {self.obs_var_col!r} is not in the data source")
        self._cv_codes = LC.fold_codes(df, self.cv.by) if self.cv is not None else None

    def _load_expert_locs(self, expert_loc_config, data_config, device_select):
        """Expert locations (local_experts.py:349-422) and the dynamic global_select entries as per-expert rank intervals."""
        xl = _load_frame(expert_loc_config["source"])
        if expert_loc_config.get("sort_by") is not None:
            xl = xl.sort_values(expert_loc_config["sort_by"])
        for k in expert_loc_config:
            if k not in ("source", "sort_by"):
                raise NotImplementedError(f"expert_loc_config key '{k}' is not supported by the batched backend")
        self.expert_locs = xl.reset_index(drop=True)
        self.dynamic = DynamicSelect(self._dynamic_gs, data_config.get("local_select"), self.df, self.expert_locs.columns) \
            if self._dynamic_gs else None
        if self.dynamic is not None and not self.dynamic.items:
            self.dynamic = None                   # no local_select entry on its loc_col: it adds nothing
        if device_select and self.dynamic is not None and len(self.local_select) + len(self.dynamic.src_cols) > L.SEL_MAXCRIT:
            raise NotImplementedError(f"device_select=True takes at most {L.SEL_MAXCRIT} selection criteria (GPSAT_SEL_MAXCRIT); "
                                      f"this config needs {len(self.local_select) + len(self.dynamic.src_cols)}: "
                                      f"{len(self.local_select)} local_select entries and {len(self.dynamic.src_cols)} "
                                      f"dynamic global_select interval(s), one per src_col")

    def _set_profiles(self, model_config):
        """The model profiles of a run (local_experts.py:292-346) and the parameter tables it stores."""
        self.init_params = dict(model_config.get("init_params") or {})
        self.constraints = model_config.get("constraints")
        self.optim_kwargs = dict(model_config.get("optim_kwargs") or {})
        self.pred_kwargs = dict(model_config.get("pred_kwargs") or {})
        # replacement model for tiles with fewer than `replacement_threshold` observations (local_experts.py:339-346,
        # 1021-1041): same defaults as the reference -- init_params / constraints fall back to the main ones,
        # optim_kwargs / pred_kwargs to {}
        self.replacement_threshold = model_config.get("replacement_threshold")
        self.profiles = {"main": dict(init_params=self.init_params, constraints=self.constraints,
                                      optim_kwargs=self.optim_kwargs, pred_kwargs=self.pred_kwargs, sgpr=self.sgpr)}
        if self.sgpr:
            if self.optim_kwargs.get("train_inducing_points", False):
                raise NotImplementedError("train_inducing_points=True is not built: the inducing points stay fixed")
            M, Mmax = int(self.init_params.get("num_inducing_points", 500)), L.max_inducing("f64", len(self.coords_col))
            if not 1 <= M <= Mmax:
                raise ValueError(f"num_inducing_points={M}: 1..{Mmax} are built (gpsat_max_inducing)")
        if self.replacement_threshold is not None:
            rm = model_config.get("replacement_model")
            rname = rm["model_name"] if isinstance(rm, dict) else rm
            if rname not in (None, "HipGPRModel", "GPflowGPRModel"):
                raise NotImplementedError(f"replacement_model '{rname}': the batched backend builds the exact-GP expert only")
            rip = model_config.get("replacement_init_params")
            rco = model_config.get("replacement_constraints")
            main_ip = {k: v for k, v in self.init_params.items() if k not in SGPR_INIT_KEYS}
            self.profiles["replacement"] = dict(
                sgpr=False,
                init_params=main_ip if rip is None else dict(rip),
                constraints=self.constraints if rco is None else rco,
                optim_kwargs=dict(model_config.get("replacement_optim_kwargs") or {}),
                pred_kwargs=dict(model_config.get("replacement_pred_kwargs") or {}))
        stored = self.param_names + ["inducing_points"] * self.sgpr
        self.params_to_store = model_config.get("params_to_store") or stored
        bad = [p_ for p_ in self.params_to_store if p_ not in stored]
        if bad:
            raise NotImplementedError(f"params_to_store {bad}: not a parameter of this model")

    def _set_load_params(self, lp):
        """``load_params`` as the run reads it: ``use_previous``, and the file / direct values without ``previous``."""
        if self.sgpr and lp is not None:
            if lp.get("previous"):
                raise NotImplementedError("load_params.previous=True is not built for sparse (SGPR) experts")
            if "inducing_points" in (lp.get("param_names") or []) or "inducing_points" in lp:
                raise NotImplementedError("loading inducing_points is not built: every expert picks its own "
                                          "(num_inducing_points / inducing_seed); load the three hyper-parameters only")
        # load_params.previous (local_experts.py:1059-1064): start every tile from the running average of earlier optima.
        # What the reference's load_params does with the combinations (local_experts.py:553-609: `if file is not None: ...
        # elif previous is not None: param_dict = previous_params`):
        #   file + previous            the FILE's parameters are set, the running average is carried along and never used;
        #   previous + direct values   the direct values are never applied (previous=True: the running average;
        #                              previous=False: nothing is set at all);
        # and `previous` among the keys makes _same_param_table False (:749-758), i.e. parameters are always stored.
        self.use_previous = False
        self._lp_keys = set(lp) if lp is not None else set()
        self.load_params = lp
        if lp is not None and lp.get("file") is None and lp.get("previous") is not None:
            self.use_previous = bool(lp["previous"])
            self.load_params = None
        elif lp is not None and "previous" in lp:
            self.load_params = {k: v for k, v in lp.items() if k not in ("previous", "previous_params")}

    def _template(self, pf, optimise, predict) -> _Profile:
        """The profile's record: HipGPRModel's defaults, scales, box and trainable mask from one throw-away model on a
        two-row frame, as the reference itself does to read param_names (postprocessing.py:202-211)."""
        kernel = pf["init_params"].get("kernel", "Matern32")
        if kernel not in L.KERNEL_IDS:
            raise NotImplementedError(f"kernel {kernel!r}")
        D = len(self.coords_col)
        dummy = pd.DataFrame({**{c: [0.0, 1.0] for c in self.coords_col}, self.obs_col: [0.0, 1.0]})
        ip = {k: v for k, v in pf["init_params"].items() if k not in SGPR_INIT_KEYS}
        m = HipGPRModel(data=dummy, obs_col=self.obs_col, coords_col=self.coords_col, engine=self.engine,
                        verbose=False, dtype=self.dtype, **ip)
        theta_default = m._theta.copy()
        cons = None
        if pf["constraints"] is not None:
            cons = {k: dict(v) for k, v in pf["constraints"].items()}
            if pf["init_params"].get("coords_scale", None) is not None and "lengthscales" in cons:
                cons["lengthscales"]["scale"] = True           # local_experts.py:1113-1114
            m.set_parameter_constraints(cons, move_within_tol=True, tol=1e-2)
        ok = pf["optim_kwargs"]
        m._fix_hyperparameters(list(ok.get("fixed_params") or []))
        # per constrained slice: the tolerance the clamp uses (gpflow_models.py:471-479 with run()'s tol = 1e-2)
        clamp = [(m._slice(pn), float(c.get("tol", 1e-2))) for pn, c in (cons or {}).items() if c.get("move_within_tol", True)]
        return _Profile(
            theta_default=theta_default, lo=m._lo.copy(), hi=m._hi.copy(), trainable=m._trainable.copy(), clamp=clamp,
            coords_scale=np.broadcast_to(m.coords_scale, (1, D)).astype(np.float64),
            obs_scale=float(m.obs_scale.reshape(-1)[0]),
            local_mean=isinstance(pf["init_params"].get("obs_mean"), str) and pf["init_params"]["obs_mean"] == "local",
            unconstrained_noise=not np.isfinite(m._lo[m._slice("likelihood_variance")]).any(), device=str(m.gpu_name)[:64], sgpr=bool(pf.get("sgpr")),
            n_inducing=int(pf["init_params"].get("num_inducing_points", 500)),
            inducing_seed=int(pf["init_params"].get("inducing_seed", 0)), kernel=kernel, max_iter=int(ok.get("max_iter", 10_000)),
            eng_kw={**{k: ok[k] for k in ("max_ls", "ftol", "gtol", "adam_lr") if k in ok}, **m._variant_args()},
            optimiser=ok.get("optimiser", "lbfgs") if optimise else "none", apply_scale=pf["pred_kwargs"].get("apply_scale", True),
            full_cov=bool(pf["pred_kwargs"].get("full_cov", False)) and predict, pred_grad=self.pred_grad and predict,
            pred_hess=self.pred_hess if predict else None)

    def _loaded_theta(self, tabs, locs, theta, unconstrained_noise):
        """Overwrite rows of ``theta`` [T, H] with the stored parameters of each expert location.  Returns the mask of
        tiles for which at least one parameter was found (the others are skipped, local_experts.py:1099-1101)."""
        cc, D = self.coords_col, len(self.coords_col)
        found_any = np.zeros(len(locs), dtype=bool)
        look = locs.copy()
        for col, spec in (self.load_params.get("index_adjust") or {}).items():
            j, f = cc.index(col), _adjust_func(spec)
            look[:, j] = [f(v) for v in look[:, j]]
        key = _index_for(cc, look)
        slots = V.slots(D, self._variants)
        for pn, tab in tabs.items():
            start, width = slots[pn]
            colvals = np.full((len(locs), width), np.nan)
            for k in range(width):
                sub = tab[tab["_dim_0"] == k] if "_dim_0" in tab.columns else tab
                sub = sub[~sub.index.duplicated(keep="first")]
                pos = sub.index.get_indexer(key)
                col = sub[pn].values.astype(np.float64)
                colvals[:, k] = np.where(pos >= 0, col[np.clip(pos, 0, max(len(col) - 1, 0))], np.nan) if len(col) else np.nan
            good = ~np.isnan(colvals).any(axis=1)             # NaN -> parameter dropped (local_experts.py:670-679)
            if pn == "likelihood_variance" and unconstrained_noise:
                low = good & (colvals[:, 0] < LIKELIHOOD_VARIANCE_LOWER_BOUND)
                if low.any():
                    warnings.warn("likelihood_variance below variance_lower_bound: set to the bound (gpflow_models.py:404-409)")
                colvals[low, 0] = LIKELIHOOD_VARIANCE_LOWER_BOUND
            theta[good, start:start + width] = colvals[good]
            found_any |= good
        return found_any

    # ------------------------------------------------------------------------------------------------------
    def run(self, store_path: Optional[str] = None, optimise: bool = True, predict: bool = True, min_obs: int = 3,
            table_suffix: str = "", max_tiles_per_call: Optional[int] = None, store_every: Optional[int] = None,
            check_config_compatible: bool = True, skip_valid_checks_on: Optional[List[str]] = None,
            rank: Optional[int] = None, world_size: Optional[int] = None, gather: bool = True,
            engine_chunk: Optional[int] = None):
        """See the module docstring.  ``store_every``: expert locations per flushed wave (default 4096; ``max_tiles_per_call``
        is the older name of the same knob).  ``engine_chunk``: tiles per engine call inside a wave (default 1024: with two
        engines the kernel of one call runs while the other call's arrays are copied and unpacked, and the tail of one kernel
        is filled by the next -- 4096 experts 18.0 -> 19.3 k tiles/s, 16 384 experts 19.5 -> 22.2 k against calls of 4096):
        while the GPU works on one call the host packs the next (gather, scale, de-mean, centre, cast).  ``rank`` /
        ``world_size``: tile-sharded run, one process per GPU (default: taken from an initialised ``torch.distributed``
        group, else 0 / 1); with ``gather=True`` rank 0 returns the global tables in expert order, the other ranks their own
        shard's (``gather="always"`` runs the exchange in a group of one rank too).  ``world_size > 1`` with ``rank=None``
        and no process group runs all the LOGICAL shards one after the other on this process's engine and merges them with
        the routine that closes the gather -- the one-GPU rehearsal of the multi-GPU path."""
        t_start = time.perf_counter()
        d_rank, d_world = _dist_rank_world()
        logical = world_size is not None and world_size > 1 and rank is None and d_world == 1
        if logical:
            rank = 0
        elif rank is None or world_size is None:
            rank, world_size = d_rank, d_world
        in_group = (not logical) and world_size > 1 and d_world == world_size
        if self.cv is not None and world_size > 1:
            raise NotImplementedError("cv: held-out predictions are not built for sharded runs (world_size > 1, real or logical)")
        if world_size > 1 and not logical and not in_group and gather:
            # explicit rank / world_size without a process group of that size: the caller synchronises the ranks itself
            # (nothing here can separate reading the resume state from rank 0's writes, and nothing can gather)
            raise RuntimeError(f"run(rank={rank}, world_size={world_size}, gather=True) needs an initialised "
                               f"torch.distributed group of {world_size} ranks (found {d_world}); pass gather=False to run "
                               f"this rank's shard on its own (start the ranks only after the store directory exists)")
        store = ResultStore(store_path, rank=rank)
        wave_n = int(store_every or max_tiles_per_call or 4096)
        chunk_n = max(1, int(engine_chunk or 1024))
        config_id, ex = self._open_store(store, table_suffix, check_config_compatible, skip_valid_checks_on, in_group,
                                         {"optimise": optimise, "predict": predict, "min_obs": min_obs,
                                          "table_suffix": table_suffix, "store_every": wave_n, "dtype": self.dtype})
        self.timings["setup_s"] = time.perf_counter() - t_start
        self.timings["flush_wait_s"] = 0.0
        plan = self._plan(ex, store_path, optimise, predict, min_obs, table_suffix, config_id)
        # shard: LPT on the cost model over the items of this run; silently skipped locations produce nothing
        tile = plan.kind == 2
        parts = sharding.partition_tiles(np.where(tile, plan.n_obs, 0), np.where(tile, plan.n_pred if predict else 0, 0),
                                         world_size) if world_size > 1 else [np.arange(len(ex), dtype=np.int64)]
        parts = [p_[plan.kind[p_] != 0] for p_ in parts]
        self.timings.update(engine_s=0.0, engine_call_s=0.0, kernel_s=0.0, tables_s=0.0, flush_s=0.0)
        self.timings["calls"] = []          # per engine call: (job, tiles, start, end, kernel seconds), times from the start of run()
        shards, got, whole = [], None, []
        try:
            if logical:
                # every logical shard on this engine, merged by the routine that closes the gather
                for r_ in range(world_size):
                    st_r = ResultStore(store_path, rank=r_)
                    st_r.drop_uncommitted()
                    shards.append(_ShardRunner(self, plan, parts[r_], st_r, wave_n, chunk_n, t_start).run())
                got = self._merge(plan, shards)
            else:
                shards.append(_ShardRunner(self, plan, parts[rank] if world_size > 1 else parts[0], store, wave_n, chunk_n,
                                           t_start).run())
                if gather and (world_size > 1 or (gather == "always" and d_world == 1 and _dist_initialised())):
                    got = self._gather(plan, shards[0], world_size, rank)          # None on the ranks other than 0
            if got is not None:
                all_items = np.nonzero(plan.kind != 0)[0]
                out = self._tables(plan, all_items, got[0][all_items], got[1], got[2])
            else:
                sh = shards[0]
                out = sh.tables if sh.tables is not None else self._tables(plan, sh.items, sh.fixed, sh.preds, sh.cov)
                if sh.cv is not None:
                    whole = sh.cv.finish(out, whole_run=sh.tables is None)
        finally:
            tf = time.perf_counter()                               # also after a fault: what was committed is on disk
            for sh in reversed(shards):
                while sh.flush:
                    sh.flush.pop().result()
            self.timings["flush_wait_s"] += time.perf_counter() - tf
        for name in whole:                                         # whole tables (cv_glued, cv_scores), behind the waves' commits
            store.put(name, out[name])
        self.run_seconds = time.perf_counter() - t_start
        self.timings["total_s"] = self.run_seconds
        return out

    def _open_store(self, store, table_suffix, check_config_compatible, skip_valid_checks_on, in_group, run_kwargs):
        """expert_locs and config bookkeeping (local_experts.py:873-903; rank 0 owns the shared files) and resume: the config
        id and the positions of the expert locations not yet in run_details (local_experts.py:475-497,908-912)."""
        cc, xl = self.coords_col, self.expert_locs
        config_id, done = 1, None
        if store.path:
            store.drop_uncommitted()
            cfg_file = os.path.join(store.path, f"oi_config{table_suffix}.json")
            prev = json.load(open(cfg_file)) if os.path.exists(cfg_file) else []
            if prev and check_config_compatible:
                check_prev_oi_config(prev[-1]["config"], self.config, skip_valid_checks_on)
            config_id = len(prev) + 1
            done = store.read(f"run_details{table_suffix}")          # resume state, read before any rank writes
            if in_group:
                import torch.distributed as dist
                dist.barrier()
            if store.rank == 0:
                prev.append({"idx": config_id, "datetime": time.strftime("%Y-%m-%d %H:%M:%S"), "config": self.config,
                             "run_kwargs": run_kwargs})
                with open(cfg_file + ".tmp", "w") as f:
                    json.dump(prev, f)
                os.replace(cfg_file + ".tmp", cfg_file)
                if store.read(f"expert_locs{table_suffix}") is None:
                    store.put(f"expert_locs{table_suffix}", xl.set_index(cc))
        todo = np.ones(len(xl), dtype=bool)
        if done is not None and len(done):
            todo = ~np.asarray(_index_for(cc, xl[cc].values.astype(np.float64)).isin(done.index))
        return config_id, np.nonzero(todo)[0]

    # ---------------- pass 1: membership, prediction coordinates, parameter vectors (whole-array) ----------------
    def _plan(self, ex, store_path, optimise, predict, min_obs, table_suffix, config_id) -> _Plan:
        cc = self.coords_col
        locs = self.expert_locs[cc].values.astype(np.float64)[ex]
        off, idx, pcs = self._select(self.expert_locs.iloc[ex], locs)
        t0 = time.perf_counter()
        n_obs, n_pred = np.diff(off), pcs.counts.astype(np.int64)
        kind, prof_id = self._kinds(n_obs, n_pred, min_obs)
        profiles = [self._template(self.profiles[pname], optimise, predict) for pname in self.profiles]
        theta0, lo, hi, save_params = self._start_params(profiles, prof_id, kind, locs, store_path, table_suffix, optimise)
        self.timings["params_s"] = time.perf_counter() - t0
        coords_all, obs_all = self.df.loc[:, cc].values.astype(np.float64), self.df[self.obs_col].values.astype(np.float64)
        assert not np.isnan(coords_all).any(), "nans found in coords"
        assert not np.isnan(obs_all).any(), "nans found in obs"
        var_all = None
        if self.obs_var_col is not None:
            var_all = self.df[self.obs_var_col].values.astype(np.float64)
            assert not np.isnan(var_all).any(), "nans found in obs_var"
            assert np.isfinite(var_all).all() and not (var_all < 0).any(), "obs_var must be finite and not negative"
        return _Plan(ex=ex, locs=locs, off=off, idx=idx, n_obs=n_obs, pcs=pcs, n_pred=n_pred, kind=kind, prof_id=prof_id,
                     profiles=profiles, theta0=theta0, lo=lo, hi=hi, save_params=save_params, coords_all=coords_all,
                     want_cov=any(pf.full_cov for pf in profiles), obs_all=obs_all, config_id=config_id,
                     table_suffix=table_suffix, optimise=optimise, predict=predict, var_all=var_all, min_obs=int(min_obs))

    def _select(self, refs, locs):
        """Membership CSR (off, idx) of every expert in ``refs`` and its prediction coordinates; with ``device_select`` the
        prediction locations are built on a second engine (another HIP stream) while the first selects the observations."""
        t0 = time.perf_counter()
        sel_engines = self._engine_pool(2) if (self.device_select and len(locs)) else [self.engine]
        sel_pool = ThreadPoolExecutor(max_workers=1) if len(sel_engines) > 1 else None
        pcs_f = sel_pool.submit(self.pred_loc.batch, locs, sel_engines[1]) if sel_pool is not None else None
        self.timings["dynamic_select_s"] = 0.0
        if len(self.local_select):
            codes = bounds = None
            if self.dynamic is not None:
                td = time.perf_counter()          # rank coding of the src_cols and the func calls
                codes, bounds = self.dynamic.codes()[0], self.dynamic.bounds(refs)
                self.timings["dynamic_select_s"] = time.perf_counter() - td
            sel = DeviceSelector(self.df, self.local_select, self.engine, interval_codes=codes) if self.device_select \
                else LocalSelector(self.df, self.local_select, interval_codes=codes)
            off, idx = sel.select(refs, bounds=bounds)
        else:
            off, idx = np.arange(len(locs) + 1, dtype=np.int64) * len(self.df), np.tile(np.arange(len(self.df)), len(locs))
        if pcs_f is not None:
            pcs = pcs_f.result()
            sel_pool.shutdown(wait=True)
        else:
            pcs = self.pred_loc.batch(locs, self.engine if self.device_select else None) if len(locs) \
                else RaggedRows(np.zeros((0, len(self.coords_col))), np.zeros(1, dtype=np.int64))
        self.timings["select_s"] = time.perf_counter() - t0
        return off, idx, pcs

    def _kinds(self, n_obs, n_pred, min_obs):
        """Item kinds -- 0 skipped silently (no prediction locations, local_experts.py:962-965), 1 stub row (N < min_obs,
        :988-1012), 2 tile, 3 error row (tile larger than the kernels take) -- and model profiles (:1021-1041)."""
        kind = np.full(len(n_obs), 2, dtype=np.int8)
        is_repl = (n_obs < self.replacement_threshold) if self.replacement_threshold is not None \
            else np.zeros(len(n_obs), dtype=bool)
        prof_names = list(self.profiles)
        prof_id = np.where(is_repl, prof_names.index("replacement") if "replacement" in prof_names else 0, 0)
        sgpr_prof = np.array([bool(self.profiles[p_].get("sgpr")) for p_ in prof_names])
        # largest tile the exact kernels take (gpsat_max_tile_obs): larger ones get an explicit error row instead of failing
        # the whole batch.  Sparse tiles have no such limit (the kernel counts rows in 32-bit integers).
        max_obs = L.max_tile_obs(self.dtype, len(self.coords_col))
        kind[np.where(sgpr_prof[prof_id], n_obs > 2 ** 31 - 1, n_obs > max_obs)] = 3
        kind[n_obs < min_obs] = 1
        kind[n_pred == 0] = 0
        if (kind == 3).any():
            warnings.warn(f"{int((kind == 3).sum())} expert locations select more observations than the kernels take "
                          f"(exact GP: {max_obs}): not run (error row in run_details)")
        return kind, prof_id

    def _start_params(self, profiles, prof_id, kind, locs, store_path, table_suffix, optimise):
        """theta0, lo, hi [T, H] and the mask of items whose parameters are stored: the profile's defaults, then ``load_params``
        (a file's tables -- an item with nothing loadable is skipped, kind 0 -- or direct values), then the move within tol."""
        D, save_params = len(self.coords_col), np.ones(len(kind), dtype=bool)
        theta0, lo, hi = (np.array([getattr(pf, f) for pf in profiles], dtype=np.float64)[prof_id]
                          for f in ("theta_default", "lo", "hi"))
        lp = self.load_params
        if lp is not None and lp.get("file") is not None:
            # the tables, read ONCE per run and indexed by expert coordinates (local_experts.py:553-689)
            src, tsuf = lp.get("file"), lp.get("table_suffix", "")   # load_params(table_suffix="") default, :561
            reader, tabs = None if isinstance(src, dict) else ResultStore(src), {}
            for pn in lp.get("param_names") or self.param_names:
                assert pn in self.param_names, f"provide param name:{pn}\nis not in param_names:{self.param_names}"
                tab = src.get(f"{pn}{tsuf}") if isinstance(src, dict) else reader.read(f"{pn}{tsuf}")
                if tab is not None and len(tab):
                    tabs[pn] = tab
            for pi, pf in enumerate(profiles):
                m_ = np.nonzero((prof_id == pi) & (kind == 2))[0]
                th = theta0[m_]
                got = self._loaded_theta(tabs, locs[m_], th, pf.unconstrained_noise)
                theta0[m_] = th
                kind[m_[~got]] = 0                              # nothing loadable: tile skipped (:1099-1101)
            same = (lp.get("file") == store_path and lp.get("table_suffix", None) == table_suffix and
                    self._lp_keys <= {"file", "table_suffix"})           # _same_param_table, :749-758
            save_params[:] = not (same and not optimise)        # local_experts.py:1090-1097
        elif lp is not None:
            # parameters given directly (load_params(**param_dict), local_experts.py:553-604)
            direct = {k: v for k, v in lp.items() if k in self.param_names}
            if not direct:
                raise NotImplementedError("load_params needs 'file' or parameter values")
            for pn, v in direct.items():
                v = np.asarray(v, dtype=np.float64).reshape(-1)
                start, width = V.slots(D, self._variants)[pn]
                theta0[:, start:start + width] = v if pn == "lengthscales" else v[0]
        for pi, pf in enumerate(profiles):                      # move within tol of the box (gpflow_models.py:471-479)
            m_ = prof_id == pi
            for sl, tol in pf.clamp:
                theta0[m_, sl] = clamp_within(theta0[m_, sl], pf.lo[sl], pf.hi[sl], tol)
        return theta0, lo, hi, save_params

    # ---------------- pass 2 helpers: one engine call's arrays; merge / gather of the shards ----------------
    def _pack_job(self, plan, pf, ids):
        """Host-side intake of one engine call (a1 of the reference in fp64): gather the tiles' rows, scale, de-mean, centre,
        cast -- by `pack_threads` threads, each writing its range of tiles (NumPy releases the GIL in gathers and arithmetic)."""
        D = len(self.coords_col)
        Ns = plan.n_obs[ids]
        o_off = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
        Ps = plan.n_pred[ids] if plan.predict else np.zeros(len(ids), dtype=np.int64)
        p_off = np.concatenate([[0], np.cumsum(Ps)]).astype(np.int64)
        out_dt = np.float32 if self.dtype == "f32" else np.float64
        X, y = np.empty((int(o_off[-1]), D), dtype=out_dt), np.empty(int(o_off[-1]), dtype=out_dt)
        Xs, mean = np.empty((int(p_off[-1]), D), dtype=out_dt), np.zeros(len(ids))
        var = np.empty(int(o_off[-1]), dtype=np.float64) if plan.var_all is not None else None
        consecutive = len(ids) > 0 and bool(np.all(np.diff(ids) == 1))
        idx, off = plan.idx, plan.off

        def sub(a, b):
            sl = ids[a:b]
            if consecutive:
                rows = idx[off[sl[0]]:off[sl[-1] + 1]]
            else:
                rows = np.concatenate([idx[off[i]:off[i + 1]] for i in sl])
            ns, oo = Ns[a:b], o_off[a:b + 1] - o_off[a]
            Xd = plan.coords_all[rows] / pf.coords_scale        # base_model.py:243
            yv_ = plan.obs_all[rows]
            if pf.local_mean:
                mean[a:b] = np.add.reduceat(yv_, oo[:-1]) / ns
            yd = (yv_ - np.repeat(mean[a:b], ns)) / pf.obs_scale   # base_model.py:244-245
            if plan.predict:
                Xsd = plan.pcs.take(sl)
                if pf.apply_scale:
                    Xsd = Xsd / pf.coords_scale
            else:
                Xsd = np.zeros((0, D))
            if self.dtype == "f32" and len(Xd):
                # what the engine does with fp64 host arrays for the fp32 kernels (per-tile centring, then the cast), done
                # here so that it too overlaps the previous call
                from .engine import centre_tiles
                Xd, Xsd = centre_tiles(Xd, Xsd, oo, p_off[a:b + 1] - p_off[a])
            X[o_off[a]:o_off[b]] = Xd
            y[o_off[a]:o_off[b]] = yd
            if var is not None:
                var[o_off[a]:o_off[b]] = plan.var_all[rows] / pf.obs_scale ** 2      # the rows of y, in y's scaled units
            Xs[p_off[a]:p_off[b]] = Xsd

        nsub = max(1, min(self.pack_threads, len(ids) // 128))
        bounds = np.linspace(0, len(ids), nsub + 1).astype(np.int64)
        if nsub == 1:
            sub(0, len(ids))
        else:
            for f_ in [self._sub_pool().submit(sub, int(bounds[j]), int(bounds[j + 1])) for j in range(nsub)]:
                f_.result()
        out = dict(o_off=o_off, X=X, y=y, p_off=p_off, Xs=Xs, mean=mean)
        if var is not None:
            out["obs_var"] = var
        if self.cv is not None:
            out["cv_fold"], out["cv_skipped"] = LC.call_labels(self, plan, ids, Ns)
        if pf.sgpr:
            # per tile the inducing points HipSGPRModel picks: a seeded subset of the tile's scaled coordinates
            Zs = [select_inducing_points(X[o_off[j]:o_off[j + 1]], pf.n_inducing, pf.inducing_seed, int(plan.ex[i]))
                  for j, i in enumerate(ids)]
            out["z_off"] = np.concatenate([[0], np.cumsum([len(z) for z in Zs])]).astype(np.int64)
            out["Z"] = np.concatenate(Zs) if Zs else np.zeros((0, D))
        return out

    def _cov_counts(self, plan, items, counts):
        """Full-covariance rows per item: P^2 where the item's profile wants ``full_cov``, else 0."""
        return np.where(np.array([plan.profiles[p].full_cov for p in plan.prof_id[items]], dtype=bool), counts ** 2, 0)

    def _merge(self, plan, shards):
        """(fixed, preds, cov) of all items in expert order from the logical shards, by the routine that closes the gather."""
        n = len(plan.ex)
        fixed_g, preds_g, _ = sharding.assemble_global([(s.fixed, s.preds, s.counts, s.items) for s in shards], n)
        cov_g = sharding.assemble_global([(s.fixed, s.cov, self._cov_counts(plan, s.items, s.counts), s.items)
                                          for s in shards], n)[1] if plan.want_cov else None
        return fixed_g, preds_g, cov_g

    def _gather(self, plan, sh, world_size, rank):
        """ONE exchange of per-tile results (RCCL over xGMI on the GPU node; gather="always": also in a group of ONE rank --
        the one-GPU rehearsal of the exchange on RCCL): (fixed, preds, cov) of all items on rank 0, None on the others."""
        n, dev_id = len(plan.ex), getattr(self.engine, "device_id", None)
        got = sharding.gather_arrays(sh.fixed, sh.preds, sh.counts, sh.items, n, world_size, rank, dev_id)
        # the P x P blocks travel the same way (counts P^2)
        got_c = sharding.gather_arrays(sh.fixed, sh.cov, self._cov_counts(plan, sh.items, sh.counts), sh.items, n,
                                       world_size, rank, dev_id) if plan.want_cov else None
        return None if rank != 0 else (got[0], got[1], got_c[1] if got_c is not None else None)

    def _sub_pool(self):
        if self._pack_pool is None:
            self._pack_pool = ThreadPoolExecutor(max_workers=self.pack_threads)
        return self._pack_pool

    def _engine_pool(self, n):
        """The engine given to the constructor plus up to n - 1 more on the same device, created on first use and kept (an
        engine that is not a gpsat_amd Engine -- the CPU tests' stand-ins -- is used alone)."""
        from .engine import Engine
        if n > 1 and isinstance(self.engine, Engine):
            try:
                while len(self._extra_engines) < n - 1:
                    self._extra_engines.append(Engine(self.engine.device_id))
            except Exception as e:                                   # not enough memory for a second workspace, ...
                warnings.warn(f"only {1 + len(self._extra_engines)} engine(s) for the chunks of a wave: {e}")
        return [self.engine] + self._extra_engines[:max(0, n - 1)]

    # ------------------------------------------------------------------------------------------------------
    def _preds_frame(self, plan, items, f_bar, pred_cat):
        """The ``preds`` table of the plan's ``items`` (``pred_cat``: the predictions of the tiles among them, back to back)."""
        cc, items = self.coords_col, np.asarray(items, dtype=np.int64)
        tile = plan.kind[items] == 2
        cnt = np.where(tile, plan.pcs.counts[items], 0).astype(np.int64)
        tot = int(cnt.sum())
        assert tot == len(pred_cat), (tot, len(pred_cat))
        raw = plan.pcs.take(items[tile]) if tot else np.zeros((0, len(cc)))
        dim0 = np.arange(tot) - np.repeat(np.concatenate([[0], np.cumsum(cnt)])[:-1], cnt)
        pr = {"_dim_0": dim0, "f*": pred_cat[:, 0], "f*_var": pred_cat[:, 1], "y_var": pred_cat[:, 2],
              "f_bar": np.repeat(f_bar, cnt)}
        if self.pred_grad:                                         # behind the three: D gradients, then their D variances
            for ci, c_ in enumerate(cc):
                pr[f"f*_grad_{c_}"] = pred_cat[:, 3 + ci]
                pr[f"f*_grad_var_{c_}"] = pred_cat[:, 3 + len(cc) + ci]
        if self.pred_hess is not None:                             # behind those: the pairs, their variances, the Laplacian and its
            pairs = V.pred_hess_pairs(self.pred_hess)
            h0 = 3 + 2 * len(cc) * bool(self.pred_grad)
            for k, (a, b) in enumerate(pairs):
                pr[f"f*_hess_{cc[a]}_{cc[b]}"] = pred_cat[:, h0 + k]
                pr[f"f*_hess_var_{cc[a]}_{cc[b]}"] = pred_cat[:, h0 + len(pairs) + k]
            pr["f*_lap"] = pred_cat[:, h0 + 2 * len(pairs)]
            pr["f*_lap_var"] = pred_cat[:, h0 + 2 * len(pairs) + 1]
        for ci, c_ in enumerate(cc):
            pr[f"pred_loc_{c_}"] = raw[:, ci]
        return pd.DataFrame(pr, index=_index_for_repeated(cc, plan.locs[items], cnt))

    def _tables(self, plan, items, fixed, pred_cat, cov_cat=None, with_preds=True):
        """Reference-layout tables of the plan's ``items`` (rows of ``fixed`` align with them; ``pred_cat`` / ``cov_cat``: their
        tiles' predictions / covariance blocks back to back), pure array assembly (GPSat/local_experts.py:691-747).
        ``with_preds=False``: the caller has written the preds rows as pieces and builds that frame itself."""
        cc = self.coords_col
        D, H = len(cc), self.H
        items = np.asarray(items, dtype=np.int64)
        n, locs, tile = len(items), plan.locs[items], plan.kind[items] == 2
        profs = [plan.profiles[p] for p in plan.prof_id[items]]
        out = {"run_details": pd.DataFrame({
            "_dim_0": np.zeros(n, dtype=np.int64), "num_obs": plan.n_obs[items].astype(np.int64),
            "run_time": np.where(tile, fixed[:, H + _SECONDS], np.nan),
            "objective_value": np.where(tile, fixed[:, H + _NLL], np.nan),
            "parameters_optimised": np.full(n, bool(plan.optimise)),
            "optimise_success": tile & bool(plan.optimise) & (fixed[:, H + _STATUS] == 0),
            "model": np.array([SGPR_MODEL_NAME if pf.sgpr else MODEL_NAME for pf in profs], dtype=object),
            "device": np.array([pf.device if t else "" for pf, t in zip(profs, tile)], dtype=object),
            "config_id": np.full(n, plan.config_id, dtype=np.int64)}, index=_index_for(cc, locs))}
        sp = tile & plan.save_params[items]
        slots = V.slots(D, self._variants)
        for pn in self.params_to_store:
            if pn == "inducing_points":
                # [M, D] per expert: _dim_0 inducing index, _dim_1 coordinate (dict_of_array_to_table of a 2-D array)
                zs = []
                for j, i in enumerate(items):
                    if sp[j] and profs[j].sgpr:          # the points HipSGPRModel picks for the same rows (scaled coordinates)
                        Xd = plan.coords_all[plan.idx[plan.off[i]:plan.off[i + 1]]] / profs[j].coords_scale
                        zs.append((j, select_inducing_points(Xd, profs[j].n_inducing, profs[j].inducing_seed, int(plan.ex[i]))))
                cnt = np.array([z.size for _, z in zs], dtype=np.int64)
                out[pn] = pd.DataFrame({
                    "_dim_0": np.concatenate([np.repeat(np.arange(len(z)), z.shape[1]) for _, z in zs]) if zs else np.zeros(0, np.int64),
                    "_dim_1": np.concatenate([np.tile(np.arange(z.shape[1]), len(z)) for _, z in zs]) if zs else np.zeros(0, np.int64),
                    pn: np.concatenate([z.reshape(-1) for _, z in zs]) if zs else np.zeros(0)},
                    index=_index_for_repeated(cc, locs[[j for j, _ in zs]] if zs else np.zeros((0, D)), cnt))
                continue
            start, width = slots[pn]
            vals = fixed[sp, start:start + width].reshape(-1)
            out[pn] = pd.DataFrame({"_dim_0": np.tile(np.arange(width), int(sp.sum())), pn: vals},
                                   index=_index_for_repeated(cc, locs[sp], np.full(int(sp.sum()), width)))
        if not plan.predict:
            out["preds"] = pd.DataFrame()
        elif with_preds:
            out["preds"] = self._preds_frame(plan, items, fixed[:, H + _OBS_MEAN], pred_cat)
            if cov_cat is not None:
                # 2-D arrays of the prediction dict -> table "preds_2" with _dim_0, _dim_1 (row-major), local_experts.py:735-745
                cnt = np.where(tile, plan.pcs.counts[items], 0).astype(np.int64)
                c2 = self._cov_counts(plan, items, cnt)
                assert int(c2.sum()) == len(cov_cat), (int(c2.sum()), len(cov_cat))
                blk = cnt[c2 > 0]
                if len(blk):
                    d0 = np.concatenate([np.repeat(np.arange(c), c) for c in blk])
                    d1 = np.concatenate([np.tile(np.arange(c), c) for c in blk])
                    out["preds_2"] = pd.DataFrame({"_dim_0": d0, "_dim_1": d1, "f*_cov": cov_cat[:, 0], "y_cov": cov_cat[:, 1]},
                                                  index=_index_for(cc, np.repeat(locs, c2, axis=0)))
        return {f"{k}{plan.table_suffix}": v for k, v in out.items()}


def _cat(rows, width):
    return np.concatenate(rows) if rows else np.zeros((0, width))


class _ShardRunner:
    """Pass 2 of one shard (one ``run()`` per runner).  A wave of ``wave_n`` items (the flush unit) is cut per model profile
    into engine calls (jobs) of at most ``chunk_n`` tiles; helper threads pack the next calls' arrays while the GPU works on
    the current one, one writer thread flushes the waves in order.  Per-tile results do not depend on how tiles are batched
    (tests/test_gpu_parity.py::test_ragged_batch_tile_indexing_is_bit_exact).  ``run()`` returns the runner holding the
    result: ``fixed`` rows in the order of ``items``, ``preds`` / ``cov`` rows of its tiles back to back, prediction rows
    per item (``counts``), the only wave's ``tables`` (else None) and the ``flush`` in flight."""

    def __init__(self, oi: BatchedLocalExpertOI, plan: _Plan, items, store: ResultStore, wave_n, chunk_n, t_start):
        self.oi, self.plan, self.items, self.store, self.t_start = oi, plan, items, store, t_start
        self.H = oi.H
        # f*, f*_var, y_var[, D gradients, D variances][, the pairs' second derivatives, their variances, the Laplacian, its variance]
        self.pred_width = (3 + 2 * len(oi.coords_col) * bool(oi.pred_grad)
                           + (0 if oi.pred_hess is None else 2 * len(V.pred_hess_pairs(oi.pred_hess)) + 2))
        self.waves = [items[w0:w0 + wave_n] for w0 in range(0, len(items), wave_n)]
        self.jobs, self.jobs_of_wave = [], {}          # jobs: (wave, profile, positions within the wave, items)
        for wi, w in enumerate(self.waves):
            for pi in range(len(plan.profiles)):
                loc_ids = np.nonzero((plan.kind[w] == 2) & (plan.prof_id[w] == pi))[0]
                for c0 in range(0, len(loc_ids), chunk_n):
                    self.jobs_of_wave.setdefault(wi, []).append(len(self.jobs))
                    self.jobs.append((wi, pi, loc_ids[c0:c0 + chunk_n], w[loc_ids[c0:c0 + chunk_n]]))
        # The predictions are most of a wave's bytes: when a wave's tiles run as consecutive calls of ONE model profile (the
        # rows of its preds table are then the calls' rows back to back), every call's rows go to the store as a row piece
        # as soon as the call returns, and the wave's flush is left with the small tables and the marker.
        self.incremental = {wi: bool(store.path) and plan.predict and len(ks) <= 64 and len({self.jobs[k][1] for k in ks}) == 1
                            for wi, ks in self.jobs_of_wave.items()}
        self.preds_name = f"preds{plan.table_suffix}"
        self.open, self.closed = {}, 0         # the open waves' (fixed, preds per item, cov rows per item); waves closed
        self.piece_futs, self.packs = {}, {}   # wave -> writes of its preds pieces; job -> its packed arrays (future)
        self.rows = ([], [], [])               # fixed, preds, cov of the closed waves
        self.tables, self.flush = None, []     # the only wave's tables; the flush queued last
        self.cv = LC.Collector(oi, plan) if oi.cv is not None else None       # the held-out results and their tables
        self.free_engines, self.flusher = queue.Queue(), ThreadPoolExecutor(max_workers=1)
        self.counts = np.where(plan.kind[items] == 2, plan.n_pred[items] if plan.predict else 0, 0).astype(np.int64)

    def run(self) -> "_ShardRunner":
        # Engine calls of consecutive chunks are issued from `n_eng` threads, each with an engine (HIP stream, workspace)
        # of its own: the second call's kernel is queued on the GPU while the first one runs and its workgroups take
        # over the CUs the first one's tail leaves idle; packing, the copies and the unpacking of one call overlap the
        # kernel of the other.  `load_params.previous` makes every call depend on the one before: one engine then.
        engines = self.oi._engine_pool(1 if self.oi.use_previous else self.oi.engine_workers)
        for e_ in engines:
            self.free_engines.put(e_)
        with ThreadPoolExecutor(max_workers=len(engines)) as packer, ThreadPoolExecutor(max_workers=len(engines)) as callers:
            try:
                if self.oi.use_previous:
                    self._run_previous(packer)
                else:
                    self._run_pipelined(packer, callers, len(engines))
                self._close_waves_to(len(self.waves))
            except BaseException:
                # after a fault the flush of the last complete wave is on disk before the fault propagates: a committed
                # wave survives whatever happens to the next one
                while self.flush:
                    self.flush.pop().result()
                self.flusher.shutdown(wait=True)
                raise
        # the last queued flush goes on while the caller's tables are assembled (run() waits for it), then the writer ends
        self.flusher.shutdown(wait=False)
        self.fixed, self.preds = _cat(self.rows[0], self.H + _N_RES), _cat(self.rows[1], self.pred_width)
        self.cov = _cat(self.rows[2], 2) if self.plan.want_cov else None
        return self

    def _pack(self, packer, k):
        if k < len(self.jobs):
            self.packs[k] = packer.submit(self.oi._pack_job, self.plan, self.plan.profiles[self.jobs[k][1]], self.jobs[k][3])

    def _run_pipelined(self, packer, callers, n_eng):
        """Calls from ``n_eng`` engine threads; packs and calls are queued ``n_eng + 1`` jobs ahead."""
        calls = {}

        def submit(k):
            if k < len(self.jobs):
                self._pack(packer, k)
                calls[k] = callers.submit(self._call, k)
        for k in range(n_eng + 1):
            submit(k)
        for k, job in enumerate(self.jobs):
            self._close_waves_to(job[0])
            te = time.perf_counter()
            pk, r, call_s = calls.pop(k).result()
            submit(k + n_eng + 1)
            self._scatter(k, pk, r, call_s, time.perf_counter() - te)

    def _run_previous(self, packer):
        """``load_params.previous``: serial calls on one engine, packs two jobs ahead; every call starts from the running average
        of earlier optima (rho = 0.95, local_experts.py:1200-1217), first the first model's defaults (:1053-1054)."""
        theta = None
        for k in range(2):
            self._pack(packer, k)
        for k, (wi, pi, _, ids) in enumerate(self.jobs):
            self._close_waves_to(wi)
            pf = self.plan.profiles[pi]
            te = time.perf_counter()
            if theta is None:
                theta = pf.theta_default.copy()
            th_call = np.tile(theta, (len(ids), 1))
            for sl, tol in pf.clamp:                                  # set_parameters(prev), then the constraints' clamp
                th_call[:, sl] = clamp_within(th_call[:, sl], pf.lo[sl], pf.hi[sl], tol)
            pk, r, call_s = self._call(k, th_call)
            for kk in range(len(ids)):                                # expert order; only successful optimisations, no NaN
                if pf.optimiser != "none" and r.status[kk] == 0 and self.plan.save_params[ids[kk]] \
                        and not np.isnan(r.theta[kk]).any():
                    theta = 0.95 * theta + 0.05 * r.theta[kk]
            self._pack(packer, k + 2)
            self._scatter(k, pk, r, call_s, time.perf_counter() - te)

    def _call(self, k, th_override=None):
        """Job k on a free engine: (packed arrays, engine result, seconds of the call)."""
        p, pf, ids = self.plan, self.plan.profiles[self.jobs[k][1]], self.jobs[k][3]
        pk = self.packs.pop(k).result()
        kw = dict(D=len(self.oi.coords_col), obs_off=pk["o_off"], X=pk["X"], y=pk["y"], pred_off=pk["p_off"], Xs=pk["Xs"], lo=p.lo[ids],
                  hi=p.hi[ids], trainable=pf.trainable, kernel=pf.kernel, optimiser=pf.optimiser, max_iter=pf.max_iter,
                  **pf.eng_kw)
        if "obs_var" in pk:
            kw["obs_var"] = pk["obs_var"]
        eng_ = self.free_engines.get()
        try:
            te = time.perf_counter()
            if pf.sgpr:
                r = eng_.sgpr_fit_predict_batch(z_off=pk["z_off"], Z=pk["Z"], theta0=p.theta0[ids], dtype="f64", **kw)
            else:
                if self.oi.cv is not None:
                    kw.update(LC.engine_kw(self.oi.cv, pk["cv_fold"], pf.local_mean, p.min_obs))
                r = eng_.fit_predict_batch(theta0=p.theta0[ids] if th_override is None else th_override, dtype=self.oi.dtype,
                                           **kw, **({"full_cov": True} if pf.full_cov else {}),
                                           **({"pred_grad": True} if pf.pred_grad else {}),
                                           **({"pred_hess": _pred_hess_arg(pf)} if pf.pred_hess is not None else {}))
            t1 = time.perf_counter()
            self.oi.timings["calls"].append((k, len(ids), round(te - self.t_start, 4), round(t1 - self.t_start, 4),
                                             round(r.kernel_ms * 1e-3, 4)))
            return pk, r, t1 - te
        finally:
            self.free_engines.put(eng_)

    def _scatter(self, k, pk, r, call_s, waited_s):
        """Job k's results into its wave: fixed columns, preds slices (and the call's preds piece to the store when the wave's
        predictions go out as pieces), full-covariance blocks with ``y_cov``.  The wave closes after its last job."""
        tm = self.oi.timings
        tm["engine_s"] += waited_s                                 # what the main thread waited for this call
        tm["engine_call_s"] += call_s                              # the calls themselves (they overlap)
        tm["kernel_s"] += r.kernel_ms * 1e-3
        wi, pi, loc_ids, ids = self.jobs[k]
        p, pf, H = self.plan, self.plan.profiles[pi], self.H
        fixed, preds, covs = self._wave(wi)
        fixed[loc_ids, :H] = r.theta
        fixed[loc_ids, H + _NLL] = -r.nll if pf.sgpr else r.nll        # SGPR: the ELBO (gpflow_models.py:860-862)
        fixed[loc_ids, H + _STATUS] = r.status
        fixed[loc_ids, H + _N_EVAL] = r.n_eval
        fixed[loc_ids, H + _N_ITER] = r.n_iter if getattr(r, "n_iter", None) is not None else np.nan
        fixed[loc_ids, H + _SECONDS] = call_s / len(ids)
        fixed[loc_ids, H + _OBS_MEAN] = pk["mean"]
        if self.cv is not None:
            self.cv.take(wi, len(self.waves[wi]), loc_ids, pk, r)
        if p.predict:
            pr = np.stack([np.asarray(r.f_mean, dtype=np.float64), np.asarray(r.f_var, dtype=np.float64),
                           np.asarray(r.y_var, dtype=np.float64)], axis=1)
            if pf.pred_grad:
                # per RAW coordinate unit, in the units f* is stored in: the model's gradient with coords_scale undone
                cs = pf.coords_scale if pf.apply_scale else np.ones_like(pf.coords_scale)
                pr = np.concatenate([pr, np.asarray(r.f_grad, dtype=np.float64) / cs, np.asarray(r.f_grad_var, dtype=np.float64) / cs ** 2], axis=1)
            if pf.pred_hess is not None:
                # the same for the second derivatives: 1 / (cs_a cs_b) per pair; the Laplacian's weights (_pred_hess_arg) made it raw
                cs = np.asarray(pf.coords_scale if pf.apply_scale else np.ones_like(pf.coords_scale), dtype=np.float64).reshape(-1)
                sc = np.array([cs[a] * cs[b] for a, b in r.hess_pairs])
                pr = np.concatenate([pr, np.asarray(r.f_hess, dtype=np.float64) / sc, np.asarray(r.f_hess_var, dtype=np.float64) / sc ** 2,
                                     np.asarray(r.f_lap, dtype=np.float64)[:, None], np.asarray(r.f_lap_var, dtype=np.float64)[:, None]], axis=1)
            p_off = pk["p_off"]
            for kk, j in enumerate(loc_ids):
                preds[j] = pr[p_off[kk]:p_off[kk + 1]]
            if self.incremental.get(wi):
                piece = self.oi._preds_frame(p, ids, pk["mean"], pr)
                self.piece_futs.setdefault(wi, []).append(
                    self.flusher.submit(self.store.write_piece, self.preds_name, self.jobs_of_wave[wi].index(k), piece))
            if pf.full_cov:
                fc = np.asarray(r.f_cov, dtype=np.float64)
                for kk, j in enumerate(loc_ids):
                    P_ = int(p_off[kk + 1] - p_off[kk])
                    fcov = fc[r.cov_off[kk]:r.cov_off[kk + 1]].reshape(P_, P_)
                    ycov = fcov.copy()                             # y_cov = f*_cov + diag(y_var - f*_var), gpflow_models.py:250-254
                    seg = pr[p_off[kk]:p_off[kk + 1]]
                    ycov[np.arange(P_), np.arange(P_)] += seg[:, 2] - seg[:, 1]
                    covs[j] = np.stack([fcov.reshape(-1), ycov.reshape(-1)], axis=1)
        if self.jobs_of_wave[wi][-1] == k:
            self._close_waves_to(wi + 1)

    def _wave(self, wi):
        """The state of wave wi, opened on first use: (fixed, preds per item, covariance rows per item)."""
        if wi not in self.open:
            n = len(self.waves[wi])
            self.open[wi] = (np.full((n, self.H + _N_RES), np.nan), [np.zeros((0, self.pred_width))] * n, [np.zeros((0, 2))] * n)
        return self.open[wi]

    def _close_waves_to(self, w):
        """Close the waves before ``w`` in order (waves without a single model tile -- stubs, error rows -- included)."""
        while self.closed < w:
            self._close_wave(self.closed)
            self.closed += 1

    def _close_wave(self, wi):
        oi, p, items = self.oi, self.plan, self.waves[wi]
        self._wave(wi)                                             # a wave without model tiles opens here
        fixed, preds, covs = self.open.pop(wi)
        tt = time.perf_counter()
        pred_cat, cov_cat = _cat(preds, self.pred_width), _cat(covs, 2) if p.want_cov else None
        pieces = self.piece_futs.pop(wi, [])
        # the predictions went out as pieces: the wave's flush needs the small tables only, and the wave's preds frame is
        # built (after the flush is queued) only where it is returned -- the only wave of a run
        lazy = bool(pieces) and not p.want_cov
        tables = oi._tables(p, items, fixed, pred_cat, cov_cat, with_preds=not lazy)
        if self.cv is not None:
            self.cv.close_wave(wi, items, fixed[:, self.H + _OBS_MEAN], tables)
        oi.timings["tables_s"] += time.perf_counter() - tt
        tf = time.perf_counter()
        # commit: these experts are done.  The parts are written by the writer thread while the next wave runs (one writer,
        # waves in order, marker last); a flush that fails surfaces when the next one is queued or at the end
        if self.flush:
            self.flush.pop().result()

        def commit(tables=dict(tables), n_pred_rows=len(pred_cat)):
            for f_ in pieces:                                      # done by now (one writer, in order): a failed piece fails the wave
                f_.result()
            self.store.write_wave(tables, prewritten={self.preds_name: n_pred_rows} if pieces else {})
        self.flush.append(self.flusher.submit(commit))
        oi.timings["flush_s"] += time.perf_counter() - tf
        if len(self.waves) == 1:
            if lazy:
                tt = time.perf_counter()
                tables[self.preds_name] = oi._preds_frame(p, items, fixed[:, self.H + _OBS_MEAN], pred_cat)
                oi.timings["tables_s"] += time.perf_counter() - tt
            self.tables = tables                                   # the only wave's tables ARE the shard's tables
        for rows, a in zip(self.rows, (fixed, pred_cat, cov_cat)):
            rows.append(a)


def _dist_initialised():
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized()
    except Exception:
        return False


def _dist_rank_world():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


def _jsonable(cfg):
    def conv(v):
        if isinstance(v, pd.DataFrame):
            return f"<DataFrame {v.shape[0]}x{v.shape[1]}>"
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, (np.integer, np.floating)):
            return v.item()
        if callable(v):
            return getattr(v, "__name__", repr(v))
        return v
    return conv(cfg or {})
