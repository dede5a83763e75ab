"""The cross-validation of BatchedLocalExpertOI (gpsat_amd/local_experts.py; its module docstring has the user's view of
``cv``, ``cv_glue`` and ``cv_joint``): the parsed options, the fold labels of an engine call, the fold layout of a tile and
the collector that takes the calls' held-out results into the tables ``cv_preds``, ``cv_params``, ``cv_folds``, ``cv_glued``
and ``cv_scores`` and the ``run_details`` column ``cv_rows_skipped``.

Fold layout: the engine numbers the folds of a tile in ascending order of their int label, as ``np.unique`` orders them
(``gpsat_cv_refit_count``); rows with a label < 0 belong to no fold.  ``fold_layout`` is the one statement of that convention
on this side of the C ABI: every per-fold array of an engine result is read with it."""
from dataclasses import make_dataclass

import numpy as np
import pandas as pd

from . import _lib as L
from . import local_experts as LE          # the table helpers; each of the two modules reads the other's names at call time only
from . import variants as V


# What a run with cv was asked for.  by: the columns whose equal values make a fold ([]: leave-one-out); refit: None, or
# {"start": "theta0" | "full"} -- every fold is fitted again without its rows; joint: the joint density per fold (table
# cv_folds); glue: None, or the cv_glue option with its defaults filled in.
CvOptions = make_dataclass("CvOptions", ["by", "refit", "joint", "glue"], frozen=True)


def parse_options(cv, cv_glue, cv_joint, data_config, dtype):
    """The constructor's ``cv``, ``cv_glue`` and ``cv_joint`` (local_experts.py's module docstring) as one CvOptions, checked;
    None without ``cv``: nothing of a run differs."""
    refit = glue = None
    if isinstance(cv, dict) and "refit" in cv:
        if not set(cv) <= {"by", "refit", "start"}:
            raise ValueError("cv must be None, 'loo', {'by': [column, ...]} or {'by': [...], 'refit': True, 'start': 'theta0' | 'full'}")
        if cv.get("by") in (None, "loo") or len(LE._as_list(cv["by"])) == 0:
            raise NotImplementedError("cv: refit is not built for leave-one-out through the orchestrator: give {'by': [column, ...]}")
        if cv.get("start", "theta0") not in ("theta0", "full"):
            raise ValueError(f"cv: start must be 'theta0' or 'full', got {cv.get('start')!r}")
        if cv["refit"]:
            refit = {"start": cv.get("start", "theta0")}
        elif "start" in cv:
            raise ValueError("cv: start is an option of refit=True")
    elif not (cv is None or cv == "loo" or (isinstance(cv, dict) and set(cv) == {"by"} and len(LE._as_list(cv["by"])) > 0)):
        raise ValueError("cv must be None, 'loo' or {'by': [column, ...]}")
    if cv_glue is not None:
        if cv is None:
            raise ValueError("cv_glue glues the held-out predictions of a run with cv: give cv='loo' or cv={'by': [...]} too")
        if not isinstance(cv_glue, dict) or "inference_radius" not in cv_glue or \
                not set(cv_glue) <= {"inference_radius", "R", "max_dist", "xprt_loc_cols"}:
            raise ValueError("cv_glue must be None or {'inference_radius': r, 'R': 3, 'max_dist': d | None, 'xprt_loc_cols': [...] | None}")
        r = cv_glue["inference_radius"]
        if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not (r > 0 and np.isfinite(r)):
            raise ValueError(f"cv_glue: inference_radius must be one finite positive number, got {r!r}")
        coords = list(data_config["coords_col"])
        cols = cv_glue.get("xprt_loc_cols")
        cols = coords[:2] if cols is None else LE._as_list(cols)
        if not 1 <= len(cols) <= 2 or any(c not in coords for c in cols):
            raise ValueError(f"cv_glue: xprt_loc_cols must be 1 or 2 of the coordinate columns {coords}, got {cols}")
        md = cv_glue.get("max_dist")
        if md is not None and not (md == md):
            raise ValueError("cv_glue: max_dist is NaN")
        glue = {"inference_radius": float(r), "R": float(cv_glue.get("R", 3)), "max_dist": None if md is None else float(md),
                "xprt_loc_cols": list(cols)}
    if cv_joint:
        if cv is None:
            raise ValueError("cv_joint is the joint density of the held-out folds of a run with cv: give cv={'by': [...]} too")
        if cv == "loo":
            raise ValueError("cv_joint: the joint density of a leave-one-out fold is the marginal one, which cv_scores already "
                             "holds (cv_glue); give cv={'by': [column, ...]}")
        if refit is not None and dtype == "f32":
            raise NotImplementedError("cv_joint with refitted folds is built in fp64 only: pass dtype='f64'")
    if cv is None:
        return None
    return CvOptions(by=[] if cv == "loo" else LE._as_list(cv["by"]), refit=refit, joint=bool(cv_joint), glue=glue)


def fold_codes(df, by):
    """One code per distinct combination of the ``by`` columns over the whole selected frame: equal codes inside a tile are
    one fold; -1: a missing value in a ``by`` column, such a row is never held out.  None for leave-one-out."""
    missing = [c for c in by if c not in df.columns]
    if missing:
        raise KeyError(f"cv: columns {missing} are not in the data source")
    if not by:
        return None
    codes = pd.factorize(pd.MultiIndex.from_frame(df[by]) if len(by) > 1 else df[by[0]])[0].astype(np.int64)
    codes[df[by].isna().any(axis=1).values] = -1
    return codes


def engine_kw(opts, labels, recentre, min_obs):
    """Engine.fit_predict_batch's keywords for one call whose rows have the fold ``labels`` of ``call_labels``."""
    refit = {} if opts.refit is None else {"cv_refit": dict(opts.refit, recentre=bool(recentre), min_obs=min_obs)}
    return {"cv_fold": labels, **refit, **({"cv_joint": True} if opts.joint else {})}


def call_labels(oi, plan, ids, Ns):
    """The fold labels of one engine call's rows ("loo", or int32 [sum N]) and, per tile, the rows that are not held out
    because their fold is above the kernel's limit (label -1)."""
    skipped = np.zeros(len(ids), dtype=np.int64)
    if not oi.cv.by:
        return "loo", skipped
    rows = np.concatenate([plan.idx[plan.off[i]:plan.off[i + 1]] for i in ids]) if len(ids) else np.zeros(0, dtype=np.int64)
    tile = np.repeat(np.arange(len(ids), dtype=np.int64), Ns)
    code = oi._cv_codes[rows]
    known = code >= 0
    key = tile * (int(oi._cv_codes.max(initial=0)) + 1) + np.where(known, code, 0)
    _, inv, cnt = np.unique(key[known], return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    labels = np.full(len(rows), -1, dtype=np.int32)
    labels[known] = inv
    big = np.zeros(len(rows), dtype=bool)
    if len(inv) and oi.cv.refit is None:       # a refitted fold is a prediction set: no limit
        big[known] = cnt[inv] > L.max_cv_fold("f64", len(oi.coords_col))
    labels[big] = -1
    skip = big | ~known
    np.add.at(skipped, tile[skip], 1)
    return labels, skipped




# The folds of one tile, in the engine's order: codes [F] the ascending labels, first [F] the position in the tile of each
# fold's first row, size [F] its rows, row_fold [N] the fold of every row (-1: never held out).
FoldLayout = make_dataclass("FoldLayout", ["codes", "first", "size", "row_fold"], frozen=True)


def fold_layout(labels):
    """The FoldLayout of one tile from the int labels of its rows."""
    labels = np.asarray(labels)
    held = np.flatnonzero(labels >= 0)
    codes, pos, inv, size = np.unique(labels[held], return_index=True, return_inverse=True, return_counts=True)
    row_fold = np.full(len(labels), -1, dtype=np.int64)
    row_fold[held] = inv.reshape(-1)
    return FoldLayout(codes.astype(np.int64), held[pos], size.astype(np.int64), row_fold)


# One tile's held-out results.  rows [N, 3]: f*, f*_var, y_var of its rows, in the tile's order; skipped: its rows that were not
# held out; lay: its FoldLayout (no folds where the run needs none).  Per fold, in the layout's order: lpd [F], the joint density
# in the units of the tile's y (cv_joint); fit [F, H + _N_FIT], the fold's own fit (refit) -- one float64 matrix, so that a wave's
# folds are one concatenation: the H parameters, then the columns below at ``H + <name>``.
TileCv = make_dataclass("TileCv", ["rows", ("skipped", int, 0), ("lay", FoldLayout, fold_layout(np.zeros(0, dtype=np.int32))),
                                   ("lpd", object, None), ("fit", object, None)])
# objective, status (_NOT_FITTED: the fold leaves fewer than min_obs rows), rows fitted, mean of those rows in the units of f*
_OBJECTIVE, _FIT_STATUS, _N_FITTED, _SHIFT = range(4)
_N_FIT, _NOT_FITTED = 4, 4
_NO_TILE = TileCv(rows=np.zeros((0, 3)))          # an item that is not a tile (a stub, an error row)


class Collector:
    """The held-out results of one shard (one per ``_ShardRunner`` of a run with cv): ``take`` files an engine call's records
    under their wave, ``close_wave`` makes the wave's tables of them, ``finish`` the whole run's, then the glue and the scores."""

    def __init__(self, oi, plan):
        self.oi, self.plan, self.opts = oi, plan, oi.cv
        self.open = {}                                  # wave -> its items' records
        self.frames = {n_: [] for n_ in ["cv_preds"] + ["cv_folds"] * oi.cv.joint + ["cv_params"] * (oi.cv.refit is not None)}
        self.skipped, self.positions = [], []            # per closed wave: skipped rows per item; positional rows of its cv_preds

    def take(self, wi, n_items, loc_ids, pk, r):
        """The results ``r`` of one engine call (packed arrays ``pk``) for the items ``loc_ids`` of wave ``wi`` (``n_items`` long)."""
        recs, opts, o_off, H = self.open.setdefault(wi, [_NO_TILE] * n_items), self.opts, pk["o_off"], self.oi.H
        cv3 = np.stack([np.asarray(r.cv_mean, dtype=np.float64), np.asarray(r.cv_f_var, dtype=np.float64),
                        np.asarray(r.cv_y_var, dtype=np.float64)], axis=1)
        if opts.refit is not None:
            fit = np.column_stack([r.cv_theta, r.cv_nll, r.cv_status, r.cv_n_obs, r.cv_shift])     # the columns of TileCv.fit
        for kk, j in enumerate(loc_ids):
            rec = recs[j] = TileCv(rows=cv3[o_off[kk]:o_off[kk + 1]], skipped=int(pk["cv_skipped"][kk]))
            if not opts.joint and opts.refit is None:
                continue
            rec.lay = fold_layout(pk["cv_fold"][o_off[kk]:o_off[kk + 1]])
            f = slice(r.cv_fold_off[kk], r.cv_fold_off[kk + 1])
            assert f.stop - f.start == len(rec.lay.codes), "the engine numbers the folds of a tile as fold_layout does"
            if opts.joint:
                rec.lpd = r.cv_lpd[f]
            if opts.refit is not None:
                rec.fit = fit[f]
                # the rows of a fold that was not fitted are NaN and count as skipped: the tile's rows less the rows it leaves
                not_fitted = rec.fit[:, H + _FIT_STATUS] == _NOT_FITTED
                rec.skipped += int((len(rec.rows) - rec.fit[not_fitted, H + _N_FITTED]).sum())

    def close_wave(self, wi, items, f_bar, tables):
        """Wave ``wi`` (its ``items``; ``f_bar``: per item the tile's de-meaning constant) into the wave's ``tables``."""
        p, recs = self.plan, self.open.pop(wi, [_NO_TILE] * len(items))      # a wave without a single tile was never opened
        items, f_bar = np.asarray(items, dtype=np.int64), np.asarray(f_bar, dtype=np.float64)
        # the positional row in the selected frame of every row of the records, back to back
        pos = np.concatenate([np.zeros(0, dtype=np.int64)] + [p.idx[p.off[i]:p.off[i + 1]] for i, rec in zip(items, recs) if len(rec.rows)])
        frames = {"cv_preds": self._preds_frame(items, recs, f_bar, pos)}
        if self.opts.joint:
            frames["cv_folds"] = self._folds_frame(items, recs, f_bar)
        if self.opts.refit is not None:
            frames["cv_params"] = self._params_frame(items, recs, f_bar)
        for name, fr in frames.items():
            self.frames[name].append(fr)
        self.skipped.append(np.array([rec.skipped for rec in recs], dtype=np.int64))
        self.positions.append(pos)
        self._into(tables, {name: [fr] for name, fr in frames.items()}, self.skipped[-1])

    def finish(self, tables, whole_run):
        """The end of a run.  ``whole_run``: it had several waves (or none) and ``tables`` lack the cv tables, which come from the
        waves' frames.  Then ``cv_glued`` and ``cv_scores`` of the run's ``cv_preds``: one glued held-out prediction per
        observation, keyed on the observation's positional row in the selected frame, in raw units by the profile's ``obs_scale``
        (postprocessing.glue_cv_predictions).  Returns the names of the tables that go to the store whole, behind the waves' commits."""
        p, g = self.plan, self.opts.glue
        if whole_run:
            self._into(tables, self.frames, np.concatenate(self.skipped) if self.skipped else np.zeros(0, dtype=np.int64))
        if g is None:
            return []
        from . import postprocessing as post
        cvp, glued, scores = tables[f"cv_preds{p.table_suffix}"], pd.DataFrame(), pd.DataFrame()
        if len(cvp):
            key = np.concatenate(self.positions) if len(self.positions) else np.zeros(0, dtype=np.int64)
            assert len(key) == len(cvp)
            glued = post._glue_cv_frame(cvp, key, g["xprt_loc_cols"], g["inference_radius"], g["R"], g["max_dist"],
                                        p.profiles[0].obs_scale, self.oi.engine)
            scores = post.score_cv_predictions(glued, by=self.opts.by or None)
        tables[f"cv_glued{p.table_suffix}"], tables[f"cv_scores{p.table_suffix}"] = glued, scores
        return [f"cv_glued{p.table_suffix}", f"cv_scores{p.table_suffix}"] if len(glued) else []

    def _into(self, tables, frames, skipped):
        """The cv tables of ``frames`` ({table: frames}) and the run_details column ``cv_rows_skipped`` into ``tables``."""
        for name, fl in frames.items():
            fl = [f_ for f_ in fl if len(f_)]
            tables[f"{name}{self.plan.table_suffix}"] = pd.concat(fl) if len(fl) > 1 else (fl[0] if fl else pd.DataFrame())
        rd = tables[f"run_details{self.plan.table_suffix}"]
        assert len(rd) == len(skipped)
        rd["cv_rows_skipped"] = skipped

    def _preds_frame(self, items, recs, f_bar, rows):
        """Table ``cv_preds``: expert coordinates as the index, like ``preds``, and the values in the units of ``preds`` -- the
        observation is ``f_bar + obs_scale f*`` plus noise.  ``rows``: the records' rows in the selected frame."""
        oi, p = self.oi, self.plan
        cnt = np.array([len(rec.rows) for rec in recs], dtype=np.int64)
        vals = LE._cat([rec.rows for rec in recs if len(rec.rows)], 3)
        fr = {"_dim_0": np.arange(int(cnt.sum())) - np.repeat(np.concatenate([[0], np.cumsum(cnt)])[:-1], cnt),
              "obs_index": oi.df.index.values[rows], **{c_: oi.df[c_].values[rows] for c_ in self.opts.by},
              **{f"pred_loc_{c_}": p.coords_all[rows, ci] for ci, c_ in enumerate(oi.coords_col)}, oi.obs_col: p.obs_all[rows],
              "f*": vals[:, 0], "f*_var": vals[:, 1], "y_var": vals[:, 2], "f_bar": np.repeat(f_bar, cnt)}
        return pd.DataFrame(fr, index=LE._index_for_repeated(oi.coords_col, p.locs[items], cnt))

    def _fold_frame(self, items, recs, columns):
        """A table with one row per expert and fold: the ``by`` values (those of the fold's first row), then ``columns``."""
        p, cnt = self.plan, np.array([len(rec.lay.first) for rec in recs], dtype=np.int64)
        first = np.concatenate([np.zeros(0, dtype=np.int64)] + [p.idx[p.off[i] + rec.lay.first] for i, rec in zip(items, recs)])
        fr = {c_: self.oi.df[c_].values[first] for c_ in self.opts.by}
        return pd.DataFrame({**fr, **columns}, index=LE._index_for_repeated(self.oi.coords_col, p.locs[items], cnt))

    def _params_frame(self, items, recs, f_bar):
        """Table ``cv_params``: the fold's own fit; ``f_bar``: its own de-meaning constant, the tile's plus obs_scale x shift."""
        oi, p, H = self.oi, self.plan, self.oi.H
        cnt = np.array([len(rec.lay.first) for rec in recs], dtype=np.int64)
        v = LE._cat([rec.fit for rec in recs if len(rec.lay.first)], H + _N_FIT)
        fr = {"num_obs": v[:, H + _N_FITTED].astype(np.int64)}
        for pn, (start, width) in V.slots(len(oi.coords_col), oi._variants).items():
            for k in range(width):
                fr[f"{pn}_{k}" if pn == "lengthscales" else pn] = v[:, start + k]
        fr["objective_value"] = v[:, H + _OBJECTIVE]
        fr["optimise_success"] = bool(p.optimise) & (v[:, H + _FIT_STATUS] == 0)
        osc = np.array([p.profiles[k].obs_scale for k in p.prof_id[items]], dtype=np.float64)
        fr["f_bar"] = np.repeat(f_bar, cnt) + np.repeat(osc, cnt) * v[:, H + _SHIFT]
        return self._fold_frame(items, recs, fr)

    def _folds_frame(self, items, recs, f_bar):
        """Table ``cv_folds``.  ``lpd``: the joint density of the observations in raw units, the device's minus n log(obs_scale);
        ``lpd_marginal``: the sum of the fold's univariate terms log N(obs; f_bar + obs_scale f*, obs_scale^2 y_var) from the
        expert's own cv_preds rows, to set beside it."""
        p, lpd, marg = self.plan, [np.zeros(0)], [np.zeros(0)]
        for i, rec, fb in zip(items, recs, f_bar):
            if not len(rec.lay.first):
                continue
            s = float(p.profiles[p.prof_id[i]].obs_scale)
            mean, var = fb + s * rec.rows[:, 0], s * s * rec.rows[:, 2]
            term = -0.5 * (p.obs_all[p.idx[p.off[i]:p.off[i + 1]]] - mean) ** 2 / var - 0.5 * np.log(2.0 * np.pi * var)
            held = rec.lay.row_fold >= 0
            lpd.append(np.asarray(rec.lpd, dtype=np.float64) - rec.lay.size * np.log(s))
            marg.append(np.bincount(rec.lay.row_fold[held], weights=term[held], minlength=len(rec.lay.first)))
        return self._fold_frame(items, recs, {"n": np.concatenate([rec.lay.size for rec in recs]), "lpd": np.concatenate(lpd),
                                              "lpd_marginal": np.concatenate(marg)})
