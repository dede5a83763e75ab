"""Post-processing of local-expert results on the MI355X: hyper-parameter smoothing and gluing of overlapping
predictions.  Host-side mirror of GPSat/postprocessing.py (``smooth_hyperparameters`` :117-375,
``glue_local_predictions`` / ``_1d`` / ``_2d`` :447-577): same argument names and meaning, tables in / tables out; the
arithmetic runs in gpsat_post.hip through the C ABI (``gpsat_smooth_batch`` / ``gpsat_glue_batch``).  Beside them, for the
held-out predictions of a run with ``cv``: ``glue_cv_predictions`` (one glued prediction per observation, grouped by an
integer key on the device, ``gpsat_glue_keyed_batch``) and ``score_cv_predictions``.  No CPU fallback:
without the HIP library these functions raise."""
import copy
import json
import os
import re
from typing import Dict, List, Optional, Union

import numpy as np
import pandas as pd

from .engine import default_engine
from .local_experts import ResultStore

GLUE_MAXVARS = 4


def smooth_hyperparameters(result_file: Union[str, Dict[str, pd.DataFrame]], params_to_smooth: List[str],
                           smooth_config_dict: Dict[str, dict], xy_dims: List[str] = ("x", "y"),
                           coords_col: Optional[List[str]] = None, reference_table_suffix: str = "",
                           table_suffix: str = "_SMOOTHED", output_file: Optional[str] = None,
                           all_params: Optional[List[str]] = None, engine=None,
                           save_config_file: bool = True) -> Dict[str, pd.DataFrame]:
    """Smooth hyper-parameter tables ``<param><reference_table_suffix>`` of a result store (directory path, or a dict of
    tables) with a 2-D Gaussian over ``xy_dims``, one slice per unique combination of the other coordinates and
    ``_dim_*`` columns; values are clipped to ``smooth_config[param]["max"/"min"]`` first; NaN results are dropped;
    parameters not smoothed are copied.  Writes ``<param><reference_table_suffix><table_suffix>`` tables to
    ``output_file`` (a store directory; default: the input store) and returns them
    (GPSat/postprocessing.py:215-343).  With ``save_config_file`` and a store on disk, the configurations recorded by the
    runs that produced the tables (``oi_config<reference_table_suffix>.json``) are re-emitted as the predict-only
    configuration of the next step -- ``run_kwargs.optimise = False``, ``table_suffix`` and ``store_path`` pointing at
    the smoothed tables, ``model.load_params = {"file", "table_suffix"}`` -- in
    ``<store>/oi_config<reference_table_suffix><table_suffix>_predict.json`` (GPSat/postprocessing.py:350-380); its path
    is returned under the key ``"__config_file__"``."""
    eng = engine or default_engine()
    tables = result_file if isinstance(result_file, dict) else ResultStore(result_file).tables()
    if all_params is None:
        all_params = [p for p in ("lengthscales", "kernel_variance", "likelihood_variance")
                      if f"{p}{reference_table_suffix}" in tables]
    missing = [p for p in params_to_smooth if p not in smooth_config_dict]
    if missing:
        raise NotImplementedError(f"parameters {missing} have no entry in smooth_config_dict")
    x_col, y_col = xy_dims
    out = {}
    for param in params_to_smooth:
        name = f"{param}{reference_table_suffix}"
        if name not in tables:
            raise NotImplementedError(f"parameter: {name} is not in tables: {list(tables.keys())}")
        df = tables[name].reset_index()
        cc = coords_col or [c for c in tables[name].index.names if c is not None]
        cfg = smooth_config_dict[param]
        org_cols = df.columns.tolist()
        other_dims = [c for c in cc if c not in xy_dims] + [c for c in df.columns if re.search(r"^_dim_\d", c)]
        pieces = []
        groups = df.groupby(other_dims, sort=False) if other_dims else [((), df)]
        for _, sub in groups:
            sub = sub.copy()
            vals = sub[param].values.astype(np.float64)
            if cfg.get("max") is not None:
                vals[vals > cfg["max"]] = cfg["max"]
            if cfg.get("min") is not None:
                vals[vals < cfg["min"]] = cfg["min"]
            sub[param] = eng.smooth_batch(sub[x_col].values, sub[y_col].values, vals, cfg["l_x"], cfg["l_y"])
            pieces.append(sub.dropna(subset=[param, x_col, y_col])[org_cols])
        out[f"{name}{table_suffix}"] = pd.concat(pieces).set_index(cc)
    for param in all_params:
        if param in params_to_smooth:
            continue
        name = f"{param}{reference_table_suffix}"
        if name in tables:
            out[f"{name}{table_suffix}"] = tables[name].copy(True)
    dest = output_file if output_file is not None else (result_file if isinstance(result_file, str) else None)
    if dest is not None:
        store = ResultStore(dest)
        for k, v in out.items():
            store.put(k, v)                                 # overwrite, like store.put(append=False)
        if save_config_file and isinstance(result_file, str):
            cfg_in = os.path.join(result_file, f"oi_config{reference_table_suffix}.json")
            if os.path.exists(cfg_in):
                new_suffix = f"{reference_table_suffix}{table_suffix}"
                derived = []
                for entry in json.load(open(cfg_in)):
                    oic = copy.deepcopy(entry.get("config", entry))
                    run_kwargs = dict(entry.get("run_kwargs", {}))
                    run_kwargs.update(optimise=False, table_suffix=new_suffix, store_path=dest)
                    model = dict(oic.get("model", {}))
                    model["load_params"] = {"file": dest, "table_suffix": new_suffix}
                    oic["model"] = model
                    oic["run_kwargs"] = run_kwargs
                    derived.append(oic)
                cfg_out = os.path.join(dest, f"oi_config{new_suffix}_predict.json")
                with open(cfg_out, "w") as f:
                    json.dump(derived, f, indent=4)
                out["__config_file__"] = cfg_out
    return out


def _glue(preds_df, pred_loc_cols, xprt_loc_cols, vars_to_glue, inference_radius, R, engine):
    eng = engine or default_engine()
    if isinstance(vars_to_glue, str):
        vars_to_glue = [vars_to_glue]
    if not 1 <= len(vars_to_glue) <= GLUE_MAXVARS:
        raise ValueError(f"1..{GLUE_MAXVARS} variables can be glued per call")
    pred = np.stack([preds_df[c].values.astype(np.float64) for c in pred_loc_cols])
    xprt = np.stack([preds_df[c].values.astype(np.float64) for c in xprt_loc_cols])
    vals = np.stack([preds_df[v].values.astype(np.float64) for v in vars_to_glue])
    # group rows by prediction location: sorted unique keys (what groupby(...).sum() returns), stable order inside
    uniq, inv = np.unique(pred.T, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    seg = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum(np.bincount(inv, minlength=len(uniq)), out=seg[1:])
    if isinstance(inference_radius, dict):                 # per-expert radius, keyed by expert location (:490-493)
        assert len(xprt_loc_cols) == 1, "a dict of inference radii is a 1-D option in the reference"
        assert len(inference_radius) == len(np.unique(xprt[0]))
        sigma = np.array([inference_radius[loc] for loc in xprt[0]], dtype=np.float64)[order] / R
    elif isinstance(inference_radius, (int, float)):
        sigma = inference_radius / R
    else:
        raise TypeError("inference_radius must be int, float or dict")
    glued = eng.glue_batch(seg, pred[:, order], xprt[:, order], vals[:, order], sigma)
    out = pd.DataFrame({c: uniq[:, i] for i, c in enumerate(pred_loc_cols)})
    for i, v in enumerate(vars_to_glue):
        out[v] = glued[i]
    return out


def _cv_layout(columns):
    """(by columns, pred_loc columns, observation column) of a ``cv_preds`` / ``cv_glued`` table, from the order in which the
    orchestrator lays them out: ..., obs_index, <by>, pred_loc_<c>..., <obs>, f*, ..."""
    cols = list(columns)
    ploc = [c for c in cols if c.startswith("pred_loc_")]
    if "obs_index" not in cols or "f*" not in cols or not ploc:
        raise ValueError(f"not a table of held-out predictions: columns {cols}")
    by = cols[cols.index("obs_index") + 1:cols.index(ploc[0])]
    return by, ploc, cols[cols.index("f*") - 1]


def _glue_cv_frame(cvp, key, xprt_loc_cols, inference_radius, R, max_dist, obs_scale, engine):
    """``cv_glued`` of one ``cv_preds`` table.  ``key``: the group of every row (int64; None: from ``obs_index``)."""
    eng = engine or default_engine()
    if isinstance(inference_radius, bool) or not isinstance(inference_radius, (int, float, np.integer, np.floating)):
        raise TypeError("inference_radius must be one number: per-expert radii are not built for held-out predictions")
    by, ploc, obs_col = _cv_layout(cvp.columns)
    coords = [c[len("pred_loc_"):] for c in ploc]
    xcols = list(coords[:2]) if xprt_loc_cols is None else ([xprt_loc_cols] if isinstance(xprt_loc_cols, str) else list(xprt_loc_cols))
    if not 1 <= len(xcols) <= 2 or any(c not in coords or c not in cvp.index.names for c in xcols):
        raise ValueError(f"xprt_loc_cols must be 1 or 2 of the coordinate columns {coords}, got {xcols}")
    n = len(cvp)
    f, fv, yv, fbar = (cvp[c].values.astype(np.float64) for c in ("f*", "f*_var", "y_var", "f_bar"))
    osc = float(obs_scale)
    vals = np.stack([fbar + osc * f, osc * osc * fv, osc * osc * yv])      # raw units
    oi = cvp["obs_index"].values
    if key is None:
        if np.issubdtype(oi.dtype, np.integer) and (n == 0 or oi.min() >= 0):
            key = oi.astype(np.int64)
        else:
            key = pd.factorize(oi)[0].astype(np.int64)
    key = np.where(np.isnan(f), -1, np.asarray(key, dtype=np.int64))      # not held out, skipped fold, failed tile
    pred = np.stack([cvp[f"pred_loc_{c}"].values.astype(np.float64) for c in xcols])
    xprt = np.stack([cvp.index.get_level_values(c).values.astype(np.float64) for c in xcols])
    keys, counts, out = eng.glue_keyed_batch(key, pred, xprt, vals, float(inference_radius) / R, max_dist)
    # carried columns: the value of the key's first row
    rows = np.nonzero(key >= 0)[0]
    first = np.zeros(len(keys), dtype=np.int64)
    first[np.searchsorted(keys, key[rows])[::-1]] = rows[::-1]           # repeated positions: the last assignment stays
    fr = {c: cvp[c].values[first] for c in ["obs_index"] + by + ploc + [obs_col]}
    fr.update({"f*": out[0], "f*_var": out[1], "y_var": out[2], "n_experts": counts.astype(np.int64)})
    with np.errstate(invalid="ignore", divide="ignore"):
        fr["z" if obs_col != "z" else "z_score"] = (fr[obs_col].astype(np.float64) - out[0]) / np.sqrt(out[2])
    return pd.DataFrame(fr)


def glue_cv_predictions(result: Union[str, Dict[str, pd.DataFrame]], xprt_loc_cols: Optional[List[str]], inference_radius: float,
                        R=3, max_dist: Optional[float] = None, obs_scale: float = 1.0, table_suffix: str = "",
                        engine=None) -> pd.DataFrame:
    """One held-out prediction per observation: table ``cv_preds<table_suffix>`` of a run with ``cv`` (a dict of tables or
    a store path) holds one row per expert that selected the observation; they are glued as the reference glues the
    overlapping predictions of its cross-validation runs (``glue_local_predictions_1d`` / ``_2d``,
    GPSat/postprocessing.py:447-577) -- weights ``normpdf(pred_loc; expert_loc, inference_radius / R)`` in
    ``xprt_loc_cols``, 1 or 2 of the coordinate columns (None: the first two) -- with the grouping on the device
    (``Engine.glue_keyed_batch``).  Every row is first converted to raw units with the model's ``obs_scale``: mean
    ``f_bar + obs_scale f*``, variances times ``obs_scale**2``.  Rows whose ``f*`` is NaN (not held out, skipped fold,
    failed tile) take no part.  ``max_dist``: a row takes part only if its expert lies nearer than that in
    ``xprt_loc_cols`` (strictly).  The group is ``obs_index``, used as it is when its dtype is a non-negative integer and
    factorised otherwise.  Returns ``cv_glued``, a row per held-out observation in ascending key order: ``obs_index``, the
    ``by`` columns, ``pred_loc_<c>``, the raw observation, ``f*``, ``f*_var``, ``y_var`` (raw units), ``n_experts`` (rows
    that took part; 0: all of them beyond ``max_dist``, the values are NaN) and ``z = (obs - f*) / sqrt(y_var)`` (named
    ``z_score`` when the observation column itself is called ``z``)."""
    tables = result if isinstance(result, dict) else ResultStore(result).tables()
    name = f"cv_preds{table_suffix}"
    if name not in tables:
        raise KeyError(f"table {name} is not in {list(tables.keys())}: run with cv=...")
    return _glue_cv_frame(tables[name], None, xprt_loc_cols, inference_radius, R, max_dist, obs_scale, engine)


def score_cv_predictions(cv_glued: pd.DataFrame, by: Optional[List[str]] = None) -> pd.DataFrame:
    """``cv_scores`` of a ``cv_glued`` table: one row overall (the ``by`` columns NaN / None) and, with ``by``, one per
    combination of those columns.  ``n`` rows scored, ``n_missing`` rows left out (no expert took part, or a NaN among
    observation, mean and variance), ``bias`` = mean(f* - obs), ``rmse`` and ``nll`` as the reference's ``utils.rmse`` and
    ``utils.nll`` with ``sig = sqrt(y_var)`` (the nll as the mean per row instead of the total), ``mean_z2``.  Host NumPy."""
    by = [] if by is None else ([by] if isinstance(by, str) else list(by))
    _, _, obs_col = _cv_layout(cv_glued.columns)
    y, mu, var = (cv_glued[c].values.astype(np.float64) for c in (obs_col, "f*", "y_var"))
    ok = (cv_glued["n_experts"].values > 0) & ~(np.isnan(y) | np.isnan(mu) | np.isnan(var))

    def score(rows):
        use = rows[ok[rows]]
        rec = {"n": len(use), "n_missing": len(rows) - len(use)}
        if len(use) == 0:
            rec.update(bias=np.nan, rmse=np.nan, nll=np.nan, mean_z2=np.nan)
            return rec
        yy, mm, sig = y[use], mu[use], np.sqrt(var[use])
        rec["bias"] = float(np.mean(mm - yy))
        rec["rmse"] = float(np.sqrt(np.mean((yy - mm) ** 2)))
        rec["nll"] = float(np.mean(np.log(sig * np.sqrt(2 * np.pi)) + (yy - mm) ** 2 / (2 * sig ** 2)))
        rec["mean_z2"] = float(np.mean(((yy - mm) / sig) ** 2))
        return rec

    recs = [dict({c: None for c in by}, **score(np.arange(len(cv_glued))))]
    if by:
        for kv, sub in cv_glued.reset_index(drop=True).groupby(by, sort=True):
            kv = kv if isinstance(kv, tuple) else (kv,)
            recs.append(dict(zip(by, kv), **score(sub.index.values)))
    return pd.DataFrame(recs, columns=by + ["n", "n_missing", "bias", "rmse", "nll", "mean_z2"])


def _location_keys(pred):
    """Rows grouped by prediction location without sorting the rows: pred [ndim, R] -> (key [R], loc [n, ndim]).  The
    locations are factorised (a hash pass per axis), only the unique ones are sorted -- lexicographically, the order
    ``np.unique(axis=0)`` gives ``_glue`` -- and a row's key is the rank of its location.  A NaN coordinate: key -1."""
    ndim = pred.shape[0]
    code, uniq = pd.factorize(pred[0])                      # NaN: code -1
    code = code.astype(np.int64)
    if ndim == 2:                                           # a pair of codes as one integer, factorised again
        c1, u1 = pd.factorize(pred[1])
        n1 = max(len(u1), 1)
        code, pairs = pd.factorize(np.where((code < 0) | (c1 < 0), -1, code * n1 + c1))
        pairs = np.asarray(pairs, dtype=np.int64)
        real = pairs >= 0
        loc = np.stack([uniq[pairs[real] // n1], u1[pairs[real] % n1]], axis=1)
    else:
        real = np.ones(len(uniq), dtype=bool)
        loc = np.asarray(uniq, dtype=np.float64)[:, None]
    order = np.lexsort(loc.T[::-1])                         # the first column is the primary key
    rank = np.full(len(real) + 1, -1, dtype=np.int64)       # the last entry: what code -1 finds
    rank[np.nonzero(real)[0][order]] = np.arange(len(order))
    return rank[code], loc[order]


def _glue_local_derivatives(order, preds_df, pred_loc_cols, xprt_loc_cols, inference_radius, R, *, value_col, grad_cols, mean_col,
                            obs_scale, also_glue, max_dist, engine, hess_cols=None, other_coords=None):
    """``glue_local_gradient`` (``order`` 1: ``hess_cols`` and ``other_coords`` are not read) and ``glue_local_hessian``
    (``order`` 2): the arguments normalised and refused under the order's noun, the columns of ``preds_df`` in raw units,
    the rows keyed by prediction location, one device call of that order, and the frame."""
    with_hess = order == 2
    noun = "Hessian" if with_hess else "gradient"
    eng = engine or default_engine()
    pcols = [pred_loc_cols] if isinstance(pred_loc_cols, str) else list(pred_loc_cols)
    xcols = [xprt_loc_cols] if isinstance(xprt_loc_cols, str) else list(xprt_loc_cols)
    if isinstance(inference_radius, bool) or not isinstance(inference_radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"inference_radius must be one number: per-expert radii are not built for the glued {noun}")
    if not 1 <= len(pcols) <= 2:
        raise ValueError(f"the glued {noun} takes 1 or 2 glue axes, got pred_loc_cols {pcols}")
    if len(xcols) != len(pcols):
        raise ValueError(f"xprt_loc_cols {xcols} and pred_loc_cols {pcols} must name the same number of glue axes")
    axes = [c[len("pred_loc_"):] if c.startswith("pred_loc_") else c for c in pcols]
    if grad_cols is None:
        grad_cols = [f"{value_col}_grad_{c}" for c in axes]
    gcols = [grad_cols] if isinstance(grad_cols, str) else list(grad_cols)
    if len(gcols) != len(pcols):
        raise ValueError(f"grad_cols {gcols} must name one gradient column per glue axis {pcols}")
    hcols, pairs, tcols = [], [], {}
    if with_hess:
        pairs = [(a, b) for a in range(len(axes)) for b in range(a, len(axes))]   # the order of variants.pred_hess_pairs
        if hess_cols is None:
            hess_cols = [f"{value_col}_hess_{axes[a]}_{axes[b]}" for a, b in pairs]
        hcols = [hess_cols] if isinstance(hess_cols, str) else list(hess_cols)
        if len(hcols) != len(pairs):
            raise ValueError(f"hess_cols {hcols} must name one column per pair a <= b of the glue axes {pcols}: {len(pairs)}")
        others = [] if other_coords is None else ([other_coords] if isinstance(other_coords, str) else list(other_coords))
        if any(t in axes for t in others):
            raise ValueError(f"other_coords {others} must not name a glue axis {axes}")
        tcols = {t: ([f"{value_col}_grad_{t}", f"{value_col}_hess_{t}_{t}"], [f"{value_col}_hess_{c}_{t}" for c in axes]) for t in others}
    extra = [] if also_glue is None else ([also_glue] if isinstance(also_glue, str) else list(also_glue))
    needed = (pcols + xcols + [value_col] + gcols + hcols + ([mean_col] if mean_col is not None else [])
              + [c for plain, mixed in tcols.values() for c in plain + mixed] + extra)
    missing = [c for c in needed if c not in preds_df.columns]
    if missing:
        raise ValueError(f"preds_df has no column {missing} (columns: {list(preds_df.columns)})")
    col = lambda c: preds_df[c].values.astype(np.float64)
    pred, xprt = np.stack([col(c) for c in pcols]), np.stack([col(c) for c in xcols])
    osc = float(obs_scale)
    val = osc * col(value_col) if mean_col is None else col(mean_col) + osc * col(value_col)
    grad = np.stack([osc * col(c) for c in gcols])
    key, loc = _location_keys(pred)
    sigma = float(inference_radius) / R
    n = len(loc)

    def placed(keys, rows):                                 # by key: every location has one, so this is the identity
        out = np.full(rows.shape[:-1] + (n,), np.nan)
        out[..., keys] = rows
        return out

    if with_hess:
        hess = np.stack([osc * col(c) for c in hcols])
        keys, counts, gval, ggrad, ghess = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad, hess, sigma, max_dist)
    else:
        keys, counts, gval, ggrad = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma, max_dist)
    fr = {c: loc[:, i] for i, c in enumerate(pcols)}
    fr[value_col] = placed(keys, gval)
    fr.update({c: placed(keys, ggrad)[i] for i, c in enumerate(gcols)})
    if with_hess:
        ghess = placed(keys, ghess)
        fr.update({c: ghess[k] for k, c in enumerate(hcols)})
        fr[f"{value_col}_lap"] = sum(ghess[k] for k, (a, b) in enumerate(pairs) if a == b)
    n_experts = np.zeros(n, dtype=np.int64)
    n_experts[keys] = counts
    fr["n_experts"] = n_experts
    for t, (plain, mixed) in tcols.items():
        keys, _, out = eng.glue_keyed_batch(key, pred, xprt, np.stack([osc * col(c) for c in plain]), sigma, max_dist)
        fr.update({c: placed(keys, out)[j] for j, c in enumerate(plain)})
        keys, _, _, out = eng.glue_keyed_grad_batch(key, pred, xprt, osc * col(plain[0]), np.stack([osc * col(c) for c in mixed]), sigma, max_dist)
        fr.update({c: placed(keys, out)[j] for j, c in enumerate(mixed)})
    for i in range(0, len(extra), GLUE_MAXVARS):
        names = extra[i:i + GLUE_MAXVARS]
        keys, _, out = eng.glue_keyed_batch(key, pred, xprt, np.stack([col(c) for c in names]), sigma, max_dist)
        fr.update({c: placed(keys, out)[j] for j, c in enumerate(names)})
    return pd.DataFrame(fr)


def glue_local_gradient(preds_df: pd.DataFrame, pred_loc_cols: List[str], xprt_loc_cols: List[str], inference_radius: float,
                        R=3, value_col: str = "f*", grad_cols: Optional[List[str]] = None, mean_col: Optional[str] = "f_bar",
                        obs_scale: float = 1.0, also_glue: Optional[List[str]] = None, max_dist: Optional[float] = None,
                        engine=None) -> pd.DataFrame:
    """The glued map with its exact slope.  Overlapping local predictions are glued as ``glue_local_predictions_1d`` / ``_2d``
    glue them, ``F(p) = sum w_i(p) f_i(p) / sum w_i(p)`` with ``w_i = normpdf(p; expert_i, inference_radius / R)`` per glue
    axis -- and the weights depend on ``p``, so the slope of ``F`` is not the glued slope: beside ``sum w~_i df_i/dp`` it has
    the term ``sum (dw~_i/dp) f_i`` (``w~ = w / sum w``), of the size (disagreement of neighbouring experts) x (their spacing)
    / sigma^2.  Gluing ``f*_grad_<c>`` with ``glue_local_predictions_2d`` returns the first term only, which is the gradient
    of nothing; this returns both (``Engine.glue_keyed_grad_batch``, grouped on the device).

    ``pred_loc_cols`` / ``xprt_loc_cols``: the 1 or 2 glue axes, as columns of ``preds_df`` (prediction and expert location).
    ``grad_cols``: the gradient of ``value_col`` along each glue axis, by default ``f*_grad_<c>`` (``pred_grad`` of the run)
    with ``<c>`` the ``pred_loc_cols`` name without a leading ``pred_loc_``.  The glued field is in raw units:
    ``mean_col + obs_scale * value_col`` (``mean_col=None``: no mean) with gradient ``obs_scale * grad_cols`` -- the slope is
    only exact when every expert's own de-meaning constant is inside the value, since experts that disagree by a constant
    tilt the glued map.  ``max_dist``: a row takes part only if its expert lies nearer than that (strictly).

    ``also_glue``: further columns glued with the plain rule on the same rows (``Engine.glue_keyed_batch``, GLUE_MAXVARS per
    call), unscaled: ``f*_var``, ``f*_grad_var_<c>``, and the gradient along a coordinate that is no glue axis (``t``), where
    the weights do not depend on it and the plain rule is exact.  A glued variance is the reference's convention, a
    weighted average of variances; it is not the variance of the glued slope.

    Returns one row per unique prediction location, the rows and their order those of ``glue_local_predictions_1d`` /
    ``_2d``: the ``pred_loc_cols``, ``value_col``, the ``grad_cols``, ``n_experts`` (rows that took part; 0: NaN values) and
    the ``also_glue`` columns."""
    return _glue_local_derivatives(1, preds_df, pred_loc_cols, xprt_loc_cols, inference_radius, R, value_col=value_col, grad_cols=grad_cols,
                                   mean_col=mean_col, obs_scale=obs_scale, also_glue=also_glue, max_dist=max_dist, engine=engine)


def glue_local_hessian(preds_df: pd.DataFrame, pred_loc_cols: List[str], xprt_loc_cols: List[str], inference_radius: float,
                       R=3, value_col: str = "f*", grad_cols: Optional[List[str]] = None, hess_cols: Optional[List[str]] = None,
                       mean_col: Optional[str] = "f_bar", obs_scale: float = 1.0, other_coords: Optional[List[str]] = None,
                       also_glue: Optional[List[str]] = None, max_dist: Optional[float] = None, engine=None) -> pd.DataFrame:
    """The glued map with its exact slope and its exact second derivatives: what relative vorticity, strain and Okubo-Weiss
    of the glued map are made of.  ``glue_local_gradient`` one order up: the weights of ``F(p) = sum w_i(p) f_i(p) / sum
    w_i(p)`` move with ``p``, so beside ``sum w~_i d2f_i/dp_a dp_b`` the second derivative of ``F`` has the terms with
    ``dw~_i/dp`` times the experts' slopes and ``d2w~_i/dp_a dp_b`` times their values -- of the size (disagreement of
    neighbouring experts) / sigma^2 and (disagreement of their slopes) x (their spacing) / sigma^2.  Gluing
    ``f*_hess_<a>_<b>`` with ``glue_local_predictions_2d`` returns the first term only, the Hessian of nothing; this returns
    all of them (``Engine.glue_keyed_hess_batch``, grouped on the device).

    ``pred_loc_cols`` / ``xprt_loc_cols``, ``grad_cols``, ``mean_col``, ``obs_scale``, ``max_dist`` and ``also_glue``: as in
    ``glue_local_gradient``.  ``hess_cols``: the second derivatives of ``value_col`` for the pairs a <= b of the glue axes in
    the order of ``variants.pred_hess_pairs`` -- (0,0), (0,1), (1,1) -- by default ``f*_hess_<a>_<b>`` (``pred_hess`` of the
    run).  The glued field is in raw units: ``mean_col + obs_scale * value_col``, every derivative times ``obs_scale``.

    ``other_coords``: coordinates that are no glue axis (``["t"]``), whose derivatives are wanted as well; the weights do not
    depend on them.  Per such ``t`` the columns ``f*_grad_t``, ``f*_hess_t_t`` and ``f*_hess_<c>_t`` for every glue axis
    ``c`` are read.  ``dF/dt = sum w~_i df_i/dt`` and ``d2F/dt2 = sum w~_i d2f_i/dt2`` because ``w~`` does not move with
    ``t``: the plain rule (``Engine.glue_keyed_batch``) is exact for them.  ``d2F/dp_c dt`` is the slope along ``c`` of the
    glued map of the field ``df/dt``, whose own slope along ``c`` is ``f*_hess_<c>_t``: the ``out_grad`` of
    ``Engine.glue_keyed_grad_batch`` on ``f*_grad_t`` with those columns as its gradient, which is exact for the reason
    ``glue_local_gradient`` is.  All three times ``obs_scale``, without the mean (a constant in ``t``).

    Returns one row per unique prediction location, the rows and their order those of ``glue_local_predictions_1d`` /
    ``_2d``: the ``pred_loc_cols``, ``value_col``, the ``grad_cols``, the ``hess_cols``, ``<value_col>_lap`` (the sum of the
    glued ``f*_hess_<a>_<a>`` over the glue axes, formed on the host), ``n_experts`` (rows that took part; 0: NaN values),
    the columns of the ``other_coords`` and the ``also_glue`` columns."""
    return _glue_local_derivatives(2, preds_df, pred_loc_cols, xprt_loc_cols, inference_radius, R, value_col=value_col, grad_cols=grad_cols,
                                   mean_col=mean_col, obs_scale=obs_scale, also_glue=also_glue, max_dist=max_dist, engine=engine,
                                   hess_cols=hess_cols, other_coords=other_coords)


def glue_local_predictions_1d(preds_df: pd.DataFrame, pred_loc_col: str, xprt_loc_col: str,
                              vars_to_glue: Union[str, List[str]], inference_radius: float, R=3, engine=None):
    """GPSat/postprocessing.py:476-524: one row per unique prediction location, each variable the normal-pdf-weighted
    (std = inference_radius / R, centred on the expert location) average of the overlapping local predictions."""
    return _glue(preds_df, [pred_loc_col], [xprt_loc_col], vars_to_glue, inference_radius, R, engine)


def glue_local_predictions_2d(preds_df: pd.DataFrame, pred_loc_cols: List[str], xprt_loc_cols: List[str],
                              vars_to_glue: Union[str, List[str]], inference_radius: float, R=3, engine=None):
    """GPSat/postprocessing.py:526-577: as 1-D with the product of the two per-axis weights."""
    return _glue(preds_df, list(pred_loc_cols), list(xprt_loc_cols), vars_to_glue, inference_radius, R, engine)
