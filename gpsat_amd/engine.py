"""Batched local-expert GP engine: thin host wrapper over the C ABI (include/gpsat_hip.h).

``Engine.fit_predict_batch`` is the packed-ragged counterpart of the per-tile body of
LocalExpertOI.run (GPSat/local_experts.py:1043-1159): all tiles of a wave are fitted and
predicted by ONE call / one kernel launch.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from . import variants as V


class GpsatError(RuntimeError):
    pass


@dataclass
class BatchResult:
    theta: np.ndarray      # [T, H] learned parameters (l_1..l_D, kernel_variance, likelihood_variance[, alpha: RationalQuadratic | c: mean="constant"])
    nll: np.ndarray        # [T] objective = negative log marginal likelihood
    status: np.ndarray     # [T] see _lib.STATUS
    n_eval: np.ndarray     # [T] objective+gradient evaluations used by the optimiser
    f_mean: object         # [sum P] numpy (host mode) or torch tensor (device mode)
    f_var: object
    y_var: object
    grad: np.ndarray | None = None   # [T, H] dNLL/dtheta at theta (when requested)
    f_cov: object = None   # full_cov: flat [sum P_t^2] (numpy / torch as f_mean); tile t = f_cov[cov_off[t]:cov_off[t+1]].reshape(P_t, P_t)
    cov_off: np.ndarray | None = None
    n_iter: np.ndarray | None = None   # [T] optimiser iterations completed (scipy nit)
    f_start: np.ndarray | None = None  # [T, S] multi-start: final objective of every start (+inf: its first evaluation failed)
    cv_mean: object = None  # [sum N] held-out predictions (cv_fold given): "f*" of every row from the other folds of its tile
    cv_f_var: object = None
    cv_y_var: object = None
    # cv_refit: one entry per fold, folds of a tile numbered by ascending label; fold k of tile t is entry cv_fold_off[t] + k
    cv_fold_off: np.ndarray | None = None   # [T+1]
    cv_theta: np.ndarray | None = None      # [F, H] parameters fitted without the fold (NaN: the fold was not fitted)
    cv_nll: np.ndarray | None = None        # [F]
    cv_status: np.ndarray | None = None     # [F] see _lib.STATUS; 4 = too few rows left (min_obs)
    cv_n_eval: np.ndarray | None = None     # [F]
    cv_n_iter: np.ndarray | None = None     # [F]
    cv_n_obs: np.ndarray | None = None      # [F] rows the fold leaves
    cv_shift: np.ndarray | None = None      # [F] mean of those rows, in the units of y (0 without recentre)
    cv_label: np.ndarray | None = None      # [F]
    # cv_joint (either flavour, with cv_fold_off): the joint log predictive density of every fold, in the units of the tile's y
    cv_lpd: np.ndarray | None = None        # [F] NaN: the fold's rows are NaN, or the fold was not fitted
    # pred_grad: the gradient of the posterior mean with respect to the prediction point and its posterior variance per
    # component, [sum P, D] each (numpy / torch as f_mean), in the units of y (y^2) per unit of X; None unless asked for
    f_grad: object = None
    f_grad_var: object = None
    # pred_hess: the second derivatives of the posterior mean for the pairs a <= b of the chosen coordinates (hess_pairs, the
    # columns) and their posterior variances, [sum P, m(m+1)/2] each; the weighted Laplacian and its variance, [sum P] (None
    # without weights); numpy / torch as f_mean, in the units of y (y^2) per unit of X squared (to the fourth)
    f_hess: object = None
    f_hess_var: object = None
    f_lap: object = None
    f_lap_var: object = None
    hess_pairs: list | None = None
    kernel_ms: float = 0.0
    total_ms: float = 0.0


@dataclass
class BinResult:
    """Sparse result of Engine.bin_batch: one record per non-empty cell, ascending ``keys``."""
    keys: np.ndarray       # [n] int64, (gid (ny-1) + iy)(nx-1) + ix
    gid: np.ndarray        # [n] int64 group
    iy: np.ndarray         # [n] int64 bin along y (0 in one dimension)
    ix: np.ndarray         # [n] int64 bin along x
    stats: dict            # statistic name -> [n] fp64
    kernel_ms: float = 0.0
    total_ms: float = 0.0


def centre_tiles(X, Xs, obs_off, pred_off, Z=None, z_off=None):
    """Subtract every tile's mean coordinate from its observations and prediction points (fp64), and from its inducing
    points ``Z`` (CSR ``z_off``) when given: the result is then (X, Xs, Z).

    The covariance functions are stationary, so the model is unchanged; what changes is the rounding of the cast to
    fp32 that follows: GPSat coordinates are typically far from the origin (t ~ 18 000 days against length scales of a
    few days), where fp32 resolves the scaled coordinate to ~1e-3 only.  Centred, the cast error is relative to the
    tile's own extent."""
    Ns, Ps = np.diff(obs_off), np.diff(pred_off)
    nz = Ns > 0
    c = np.zeros((len(Ns), X.shape[1]))
    if nz.any():
        c[nz] = np.add.reduceat(X, obs_off[:-1][nz], axis=0) / Ns[nz, None]
    out = X - np.repeat(c, Ns, axis=0), Xs - np.repeat(c, Ps, axis=0)
    return out if Z is None else out + (Z - np.repeat(c, np.diff(z_off), axis=0),)


def factorise_folds(fold, N=None):
    """Fold labels of any hashable kind -> int32 codes [N].  ``fold``: array-like of N labels, or a 2-D array whose equal rows
    form a fold.  Integer labels below 0 keep their meaning (never held out) and are returned as -1; None / NaN labels
    likewise.  Codes are dense and ascend with the first appearance of a label."""
    import pandas as pd
    a = np.asarray(fold)
    if a.ndim == 2:
        keys = pd.MultiIndex.from_arrays([a[:, k] for k in range(a.shape[1])]) if a.shape[1] != 1 else pd.Index(a[:, 0])
        never = np.zeros(len(a), dtype=bool)
    elif a.ndim == 1:
        keys = pd.Index(a)
        never = (a < 0) if np.issubdtype(a.dtype, np.integer) else np.asarray(pd.isna(a))
    else:
        raise ValueError(f"fold labels must be 1-D, or 2-D with one row per observation; got shape {a.shape}")
    if N is not None and len(a) != N:
        raise ValueError(f"{len(a)} fold labels for {N} rows")
    codes = np.asarray(pd.factorize(keys)[0], dtype=np.int64)
    codes[never] = -1
    if (codes >= 0).any():                       # dense again after the never-held-out labels left
        codes[codes >= 0] = pd.factorize(codes[codes >= 0])[0]
    return codes.astype(np.int32)


# cv_refit: the default budget of one library call, in expanded rows (the sum over all folds of the rows each fold leaves).
# A call holds (D + 1) elements per expanded row on the device: at D = 3, 2^25 rows are 0.5 GiB in fp32 and 1 GiB in fp64.
CV_REFIT_MAX_EXPANDED_ROWS = 1 << 25


def cv_refit_options(cv_refit) -> dict:
    """``cv_refit`` of Engine.fit_predict_batch (True, or a dict) as a dict with every key set."""
    opts = {"start": "theta0", "recentre": True, "min_obs": 1, "max_expanded_rows": CV_REFIT_MAX_EXPANDED_ROWS}
    if cv_refit is True:
        return opts
    if not isinstance(cv_refit, dict):
        raise GpsatError(f"cv_refit must be True or a dict with keys out of {sorted(opts)}, got {cv_refit!r}")
    unknown = sorted(set(cv_refit) - set(opts))
    if unknown:
        raise GpsatError(f"cv_refit: unknown keys {unknown}; known: {sorted(opts)}")
    opts.update(cv_refit)
    if opts["start"] not in L.CV_START_IDS:
        raise GpsatError(f"cv_refit: start must be 'theta0' or 'full', got {opts['start']!r}")
    if int(opts["max_expanded_rows"]) < 1:
        raise GpsatError("cv_refit: max_expanded_rows must be at least 1")
    return opts


NP_DTYPES = {"f32": np.float32, "f64": np.float64}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bulk_ptr(a):
    """Pointer to a bulk input or output: host numpy, or a device tensor."""
    return _ptr(a) if isinstance(a, np.ndarray) else a.data_ptr()


def _alloc(n, dtype, beside=None, at_least=0):
    """An output of ``n`` elements (at least ``at_least``) of ``dtype``: numpy on the host, or a torch tensor beside the
    device tensor ``beside`` -- there of one element at least, so that its pointer is valid.  Callers hand out ``[:n]``."""
    if beside is None:
        return np.empty(max(n, at_least), dtype=NP_DTYPES[dtype])
    import torch
    return torch.empty(max(n, 1), dtype=beside.dtype, device=beside.device)


def _pred_hess_spec(pred_hess, D):
    """``pred_hess`` of fit_predict_batch as (sorted coordinate indices, the D Laplacian weights or None for no Laplacian)."""
    spec = {} if pred_hess is True else pred_hess
    if not isinstance(spec, dict) or set(spec) - {"dims", "lap_weight"}:
        raise GpsatError('pred_hess: True, or a dict with "dims" and / or "lap_weight"')
    dims = list(range(D)) if spec.get("dims") is None else sorted(set(int(a) for a in spec["dims"]))
    if not dims or dims[0] < 0 or dims[-1] >= D:
        raise GpsatError(f"pred_hess: dims must name at least one coordinate index in 0..{D - 1}, got {spec.get('dims')!r}")
    if "lap_weight" not in spec:
        return dims, [1.0 if a in dims else 0.0 for a in range(D)]
    if spec["lap_weight"] is None:
        return dims, None
    w = [float(c) for c in np.asarray(spec["lap_weight"], dtype=np.float64).reshape(-1)]
    if len(w) != D:
        raise GpsatError(f"pred_hess: lap_weight has one weight per coordinate, {D}, got {len(w)}")
    if any(not (c >= 0.0 and np.isfinite(c)) for c in w):
        raise GpsatError("pred_hess: lap_weight must be finite and >= 0")
    if any(c > 0.0 and a not in dims for a, c in enumerate(w)):
        raise GpsatError("pred_hess: lap_weight is set for a coordinate outside dims")
    return dims, (w if any(c > 0.0 for c in w) else None)


def _fold_labels(cv_fold, sumN):
    """``cv_fold`` as the C ABI takes it: None for "loo", else contiguous int32 labels [sumN]."""
    if isinstance(cv_fold, str) and cv_fold == "loo":
        return None
    raw = np.asarray(cv_fold).reshape(-1)
    if not np.issubdtype(raw.dtype, np.integer):
        raise GpsatError(f"cv_fold: integer labels wanted, got dtype {raw.dtype} (factorise_folds makes them)")
    if raw.size and (int(raw.max()) > 2 ** 31 - 1 or int(raw.min()) < -2 ** 31):
        raise GpsatError("cv_fold: labels must fit int32 (the C ABI's label type); factorise_folds makes dense codes")
    labels = np.ascontiguousarray(raw, dtype=np.int32)
    if labels.shape != (sumN,):
        raise GpsatError(f"cv_fold: {labels.size} labels for {sumN} rows")
    return labels


def _host_meta(D, offs, theta0, lo, hi, trainable, H=None):
    """The CSR offset tables as contiguous int64, theta0 / lo / hi as [T, H] fp64 (no bounds: NaN) and trainable as [H] uint8.
    ``H``: hyper-parameters per tile (variants.n_hyper), by default those of the plain call."""
    offs = [np.ascontiguousarray(o, dtype=np.int64) for o in offs]
    T, H = len(offs[0]) - 1, (V.n_hyper(D) if H is None else int(H))
    if not all(len(o) == T + 1 for o in offs):
        raise GpsatError(f"offset tables of {[len(o) for o in offs]} entries: all need T + 1 = {T + 1}")

    def per_tile(a):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (T, H)))
    lo = np.full((T, H), np.nan) if lo is None else per_tile(lo)
    hi = np.full((T, H), np.nan) if hi is None else per_tile(hi)
    trainable = np.ones(H, dtype=np.uint8) if trainable is None else \
        np.ascontiguousarray(np.asarray(trainable).astype(bool).astype(np.uint8))
    if trainable.shape != (H,):
        raise GpsatError(f"trainable has shape {trainable.shape}: ({H},) is expected, one flag per hyper-parameter")
    return offs, per_tile(theta0), lo, hi, trainable


class Engine:
    """One engine per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device_id: int = 0, workgroups_per_cu: int = 0):
        self._lib = L.get_lib()
        opts = L.GpsatOpts()
        opts.workgroups_per_cu = int(workgroups_per_cu)
        h = C.c_void_p()
        rc = self._lib.gpsat_create(int(device_id), C.byref(opts), C.byref(h))
        if rc != 0:
            raise GpsatError(f"gpsat_create failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        self._h = h
        buf = C.create_string_buffer(256)
        self._lib.gpsat_device_name(self._h, buf, 256)
        self.device_name = buf.value.decode()
        self.device_id = device_id

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpsat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_tensor(self, name, t, dtype, numel=None, at_least=None):
        """One bulk argument of a device-mode call: a contiguous torch tensor of the call's dtype on the engine's GPU, of
        exactly ``numel`` elements (an input) or of ``at_least`` elements (an output).  Raises GpsatError naming ``name``."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise GpsatError(f"{name}: device mode needs torch tensors for every bulk argument, got {type(t).__name__}")
        if not t.is_cuda or t.device.index != self.device_id:
            raise GpsatError(f"{name}: lives on {t.device}, the engine on cuda:{self.device_id}")
        want = torch.float32 if dtype == "f32" else torch.float64
        if t.dtype != want:
            raise GpsatError(f"{name}: has dtype {t.dtype}, the call's dtype {dtype!r} needs {want}")
        if not t.is_contiguous():
            raise GpsatError(f"{name}: device mode needs a contiguous tensor (shape {tuple(t.shape)}, strides {t.stride()})")
        if numel is not None and t.numel() != numel:
            raise GpsatError(f"{name}: has {t.numel()} elements, {numel} expected")
        if at_least is not None and t.numel() < at_least:
            raise GpsatError(f"{name}: has {t.numel()} elements, at least {at_least} (sum P) are written")

    def _device_io(self, inputs, dtype, sumP, out):
        """Device mode: check the input tensors (name -> (tensor, elements)), take or allocate the three prediction outputs
        and wait for the caller's stream.  Returns (f_mean, f_var, y_var), flat."""
        import torch
        for tname, (t_, n) in inputs.items():
            self._check_tensor(tname, t_, dtype, numel=n)
        if out is None:
            out = tuple(_alloc(sumP, dtype, inputs["X"][0]) for _ in range(3))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 3:
                raise GpsatError(f"out: three tensors (f_mean, f_var, y_var) are expected, got "
                                 f"{len(out) if isinstance(out, (tuple, list)) else type(out).__name__}")
            for oname, o in zip(("f_mean", "f_var", "y_var"), out):
                self._check_tensor(f"out ({oname})", o, dtype, at_least=sumP)
            out = tuple(o if o.dim() == 1 else o.view(-1) for o in out)
        torch.cuda.current_stream(inputs["X"][0].device).synchronize()   # inputs must be complete before our stream reads them
        return out

    def _stage(self, D, dtype, sumN, sumP, X, y, Xs, out, more=None):
        """The bulk inputs and the three prediction outputs as the library takes them: (device_mode, (X, y, Xs), preds).
        Device mode (``X`` is not a numpy array): the tensors, and those of ``more`` (name -> (tensor, elements)), are
        checked and handed on as views of shape (sumN, D), (sumN,) and (sumP, D), whatever shape the caller gave them.
        Host mode: X, y and Xs are cast to ``dtype`` and laid out contiguously; ``out`` is refused."""
        if not isinstance(X, np.ndarray):
            preds = self._device_io({"X": (X, sumN * D), "y": (y, sumN), "Xs": (Xs, sumP * D), **(more or {})}, dtype, sumP, out)
            return True, (X.view(sumN, D), y.view(sumN), Xs.view(sumP, D)), preds
        if out is not None:
            raise GpsatError("out: preallocated outputs belong to device mode (X, y, Xs as torch tensors on the GPU); with numpy "
                             "inputs the predictions are returned as new numpy arrays")
        np_dt = NP_DTYPES[dtype]
        data = (np.ascontiguousarray(X, dtype=np_dt).reshape(sumN, D), np.ascontiguousarray(y, dtype=np_dt).reshape(sumN),
                np.ascontiguousarray(Xs, dtype=np_dt).reshape(sumP, D))
        return False, data, tuple(_alloc(sumP, dtype) for _ in range(3))

    @staticmethod
    def _fill_batch(D, dtype, device_mode, meta, data, preds, kernel, optimiser, max_iter, max_ls, ftol, gtol, adam_lr, want_grad):
        """GpsatBatch over ``meta`` (_host_meta's result), the inputs ``data`` = (X, y, Xs) and the outputs ``preds`` =
        (f_mean, f_var, y_var), with fresh per-tile result arrays.  Returns (batch, results): ``results`` are BatchResult
        fields; the caller keeps ``meta``, ``data`` and ``preds`` alive until the library call has returned."""
        (obs_off, pred_off, *_), theta0, lo, hi, trainable = meta
        T, H = len(obs_off) - 1, theta0.shape[1]
        res = dict(theta=np.empty((T, H), dtype=np.float64), nll=np.empty(T, dtype=np.float64),
                   grad=np.empty((T, H), dtype=np.float64) if want_grad else None, status=np.empty(T, dtype=np.int32),
                   n_eval=np.empty(T, dtype=np.int32), n_iter=np.zeros(T, dtype=np.int32))
        b = L.GpsatBatch()
        b.T, b.D, b.dtype = T, D, (L.F32 if dtype == "f32" else L.F64)
        b.kernel = L.KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
        b.memory = L.MEM_DEVICE if device_mode else L.MEM_HOST
        b.optimiser = L.OPT_IDS[optimiser] if not isinstance(optimiser, int) else optimiser
        b.max_iter, b.max_ls = int(max_iter), int(max_ls)
        b.ftol, b.gtol, b.adam_lr = float(ftol), float(gtol), float(adam_lr)
        b.obs_off, b.pred_off = _ptr(obs_off), _ptr(pred_off)
        b.theta0, b.lo, b.hi, b.trainable = _ptr(theta0), _ptr(lo), _ptr(hi), _ptr(trainable)
        b.X, b.y, b.Xs = (_bulk_ptr(a) for a in data)
        b.theta, b.nll, b.grad = _ptr(res["theta"]), _ptr(res["nll"]), _ptr(res["grad"])
        b.status, b.n_eval, b.n_iter = _ptr(res["status"]), _ptr(res["n_eval"]), _ptr(res["n_iter"])
        b.f_mean, b.f_var, b.y_var = (_bulk_ptr(a) for a in preds)
        b.cov_off, b.f_cov = None, None
        return b, res

    def _result(self, rc, name, res, preds, sumP, **more) -> BatchResult:
        """Raise on a failed call; otherwise the BatchResult with the call's timing."""
        if rc != 0:
            raise GpsatError(f"{name} failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        km, tm = C.c_double(), C.c_double()
        self._lib.gpsat_last_timing(self._h, C.byref(km), C.byref(tm))
        fm, fv, yv = preds if len(preds[0]) == sumP else (a[:sumP] for a in preds)     # device outputs hold at least one element
        return BatchResult(f_mean=fm, f_var=fv, y_var=yv, kernel_ms=km.value, total_ms=tm.value, **res, **more)

    @staticmethod
    def _check_call(dtype, kernel, mean, obs_var, cv_fold, cv_refit, n_starts, full_cov, cv_joint=False):
        """The rows of variants.VARIANTS the call asks for, and the options of ``cv_refit`` (None without it).  Raises for
        what the wrapper refuses itself; what one library call can express is left to the library's own message."""
        if cv_joint and cv_fold is None:
            raise GpsatError("cv_joint is the joint density of the held-out folds: it needs cv_fold")
        if cv_joint and dtype == "f32" and cv_refit not in (None, False):
            raise GpsatError("cv_joint with cv_refit is built in fp64 only (the g x g factorisation of an fp32 covariance would "
                             "need a tolerance nobody has measured): pass dtype='f64'")
        if dtype not in NP_DTYPES:
            raise GpsatError(f"dtype {dtype!r}: use 'f32' or 'f64'")
        if mean not in L.MEAN_IDS:
            raise GpsatError(f"mean {mean!r}: use None or 'constant'")
        refit = None if cv_refit is None or cv_refit is False else cv_refit_options(cv_refit)
        on = {"noise": obs_var is not None, "cv": cv_fold is not None and refit is None, "cv_refit": refit is not None,
              "multistart": n_starts is not None, "full_cov": bool(full_cov)}
        asked = L.theta_variants(kernel, mean) + [k for k in on if on[k]]
        why = V.why_refused(asked, dtype, None, host_only=True)
        if why:
            raise GpsatError(why)
        if refit is not None and cv_fold is None:
            raise GpsatError("cv_refit needs the fold labels: cv_fold is None")
        if refit is not None and isinstance(cv_fold, str):
            raise GpsatError(f"cv_refit is not built for cv_fold={cv_fold!r}: give integer fold labels")
        return asked, refit

    @staticmethod
    def _check_widths(asked, kernel, D, **arrays):
        """theta0 / lo / hi / trainable of a variant with a parameter of its own: say which width is expected, by name."""
        names = V.param_names(asked)
        if len(names) == len(V.BASE_PARAMS):
            return
        H = V.n_hyper(D, asked)
        for pname, a in arrays.items():
            shp = None if a is None else np.shape(a)
            if shp is not None and (len(shp) not in ((1,) if pname == "trainable" else (1, 2)) or shp[-1] != H):
                raise GpsatError(f"{pname} has shape {shp}: kernel {kernel!r}" + (" with mean='constant'" if "mean" in asked else "")
                                 + f" with D = {D} has H = D + {H - D} = {H} parameters per tile ({', '.join(names)}), so (H,)"
                                 + ("" if pname == "trainable" else " or (T, H)") + " is expected")

    def _entry(self, asked):
        """(row key, name) of the library call that carries ``asked``: the one row with an entry point of its own, else
        the plain call."""
        key = next((k for k in asked if V.VARIANTS[k].entry), None)
        name = V.VARIANTS[key].entry if key else V.PLAIN_ENTRY
        if not hasattr(self._lib, name):
            raise GpsatError(f"this libgpsat_hip.so has no {name} ({V.VARIANTS[key].label})")
        return key, name

    @staticmethod
    def _extension(key, T, H, sumN, dtype, beside, n_starts, starts, obs_var, labels):
        """The extension struct of row ``key``, the BatchResult fields it fills and what else the struct points to (the
        caller holds all three until the library call has returned)."""
        ext, fields, keep = getattr(L, V.VARIANTS[key].struct)(), {}, None
        if key == "multistart":
            S = int(n_starts)
            ext.n_starts, ext.transform = S, L.TRANSFORM_LOG
            if starts is not None and S > 1:
                keep = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(T, S - 1, H))
            fields["f_start"] = np.full((T, max(S, 1)), np.nan)
            ext.starts, ext.f_start = _ptr(keep), _ptr(fields["f_start"])
        elif key == "noise":
            ext.obs_var = _bulk_ptr(obs_var)
        elif key == "mean":
            ext.kind = L.MEAN_CONSTANT
        elif key == "cv":
            cvo = tuple(_alloc(sumN, dtype, beside) for _ in range(3))
            ext.fold = _ptr(labels)
            ext.cv_mean, ext.cv_f_var, ext.cv_y_var = (_bulk_ptr(a) for a in cvo)
            fields.update(cv_mean=cvo[0][:sumN], cv_f_var=cvo[1][:sumN], cv_y_var=cvo[2][:sumN])
        return ext, fields, keep

    def _cv_fold_off(self, T, obs_off, labels):
        """Folds per tile as CSR offsets [T+1], as gpsat_cv_refit_count numbers them; ``labels`` None (leave-one-out): fold k
        of a tile is its row k, so the offsets are ``obs_off``.  Returns (fold_off, expanded rows or None)."""
        if labels is None:
            return np.array(obs_off, dtype=np.int64), None
        fold_off = np.zeros(T + 1, dtype=np.int64)
        rows = C.c_int64(0)
        rc = self._lib.gpsat_cv_refit_count(T, _ptr(obs_off), _ptr(labels), _ptr(fold_off), C.byref(rows))
        if rc != 0:
            raise GpsatError(f"gpsat_cv_refit_count failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        return fold_off, rows.value

    def _joint_entry(self, key):
        name = V.JOINT_ENTRY[key]
        if not hasattr(self._lib, name):
            raise GpsatError(f"this libgpsat_hip.so has no {name} (cv_joint: the joint density of every held-out fold)")
        return name

    def fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, theta0, lo=None, hi=None,
                          trainable=None, kernel="Matern32", optimiser="lbfgs", max_iter=10_000,
                          max_ls=0, ftol=0.0, gtol=0.0, adam_lr=0.0, want_grad=False,
                          out=None, dtype="f32", full_cov=False, n_starts=None, starts=None, cv_fold=None,
                          cv_refit=None, mean=None, obs_var=None, cv_joint=False, pred_grad=False, pred_hess=False) -> BatchResult:
        """
        X [sumN, D], y [sumN], Xs [sumP, D]: numpy arrays (host mode) or contiguous torch.cuda tensors (device
        mode; outputs are then torch tensors, optionally preallocated via ``out`` = (f_mean, f_var, y_var)).
        Device mode returns the bits of host mode in every field, reads the inputs without changing them and writes
        nothing of the caller's but ``out[i][:sumP]``.  Every bulk argument (X, y, Xs, obs_var, and Z of the sparse call)
        must be a contiguous tensor of the call's dtype on this engine's GPU with exactly sumN D, sumN, sumP D (sumN, sumM D)
        elements, in any shape: rows are taken in the order of the flat memory.  ``out``: exactly three such tensors of at
        least sumP elements each (larger is allowed, the rest is left alone; the result holds the ``[:sumP]`` views of the
        same storage).  Anything else raises GpsatError naming the argument before the library is called, as does
        ``out`` with numpy inputs: host mode returns new arrays.
        ``dtype``: "f32" (default; fp32 MFMA kernels) or "f64" (the reference's native precision, fp64 MFMA
        kernels); host arrays are cast, device tensors must already have that dtype.  Offsets / theta0 / bounds
        are always host numpy (fp64).  ``full_cov``: also return the P_t x P_t posterior covariance of every tile
        (predict(full_cov=True), gpflow_models.py:245-263).
        ``n_starts`` (an int): multi-start bounded L-BFGS-B in log space (gpsat_fit_predict_batch_ms): theta0 and the
        ``starts`` [T, n_starts - 1, H] (constrained space) per tile, the best final objective wins; ``f_start`` of the
        result holds every start's final objective.  None: the optimisers of gpsat_fit_predict_batch.
        ``cv_fold``: "loo", or an int array [sum N] of fold labels (rows of one tile with equal label >= 0 are held out
        together, a negative label is never held out): also return, per row, the prediction from the other folds of its
        tile at the returned parameters (gpsat_fit_predict_batch_cv, fp64 only) as ``cv_mean``, ``cv_f_var``, ``cv_y_var``.
        None: gpsat_fit_predict_batch, as ever.
        ``cv_refit`` (with integer ``cv_fold`` labels; both dtypes, a fold of any size): True, or a dict with keys out of
        ``start`` ("theta0": every fold starts from the tile's theta0, a fresh run as the reference makes; "full": from the
        tile's fitted parameters), ``recentre`` (True: the rows a fold leaves are de-meaned again by their own mean),
        ``min_obs`` (a fold that leaves fewer rows is not fitted: status 4, NaN rows) and ``max_expanded_rows``.  Every
        fold is then FITTED AGAIN without its rows (gpsat_fit_predict_batch_cv_refit): ``cv_mean`` (in the units of the
        tile's y), ``cv_f_var`` and ``cv_y_var`` are the refitted model's predictions at the held-out rows, and
        ``cv_fold_off``, ``cv_theta``, ``cv_nll``, ``cv_status``, ``cv_n_eval``, ``cv_n_iter``, ``cv_n_obs``, ``cv_shift``
        and ``cv_label`` describe every fold.  When the folds' remaining rows sum to more than ``max_expanded_rows``
        (default CV_REFIT_MAX_EXPANDED_ROWS = 2^25 rows: (D + 1) elements each on the device, 0.5 GiB in fp32 and 1 GiB
        in fp64 at D = 3), consecutive ranges of tiles are run by one library call each and the results concatenated; a
        single tile above the budget is an error.  Refused with cv_fold="loo".
        ``cv_joint`` (with ``cv_fold``, either flavour; with ``cv_refit`` fp64 only): also ``cv_lpd`` [F], the joint log
        predictive density log N(y_G; mean, covariance of the held-out fold) of every fold in the units of the tile's y, and
        ``cv_fold_off`` [T+1] (gpsat_fit_predict_batch_cv_joint / _cv_refit_joint).  NaN where the
        fold's rows are NaN or the fold was not fitted.  Without ``cv_refit`` every other field has the bits of the call
        without it.  With ``cv_refit`` the folds' batch returns its posterior covariances for it: a tile's folds count
        sum g^2 elements against ``max_expanded_rows`` as well, at D + 1 elements per row, and the predictions need not
        have the bits of the call without ``cv_joint``.
        ``kernel="RationalQuadratic"``: one more hyper-parameter per tile, H = D + 3 with alpha last, so theta0 / lo / hi are
        (H,) or (T, H) and trainable is (H,); fp64 and D <= 3 only.
        ``mean="constant"`` (gpsat_fit_predict_batch_mean): a trainable constant mean c, GPflow's mean_functions.Constant --
        y ~ N(c 1, K + sn2 I).  One more hyper-parameter per tile, H = D + 3 with c last and in the units of y, so theta0 / lo /
        hi are (H,) or (T, H) and trainable is (H,); c is unconstrained with NaN bounds (any finite value) and boxed with finite
        ones, ``f_mean`` includes it and a tile without observations predicts c of theta0.  fp64 and D <= 3 only, with
        either optimiser.  None: the zero-mean model, as ever.
        ``obs_var`` [sumN] (gpsat_fit_predict_batch_noise): known noise variances per observation, float64, numpy or a device
        tensor as the other bulk inputs are -- y ~ N(0, K + sn2 I + diag(obs_var)), finite and >= 0, not trained.  theta and H
        are those of the plain call; likelihood_variance is what obs_var does not explain (fix it through ``trainable`` to
        trust obs_var alone) and ``y_var`` = ``f_var`` + likelihood_variance.  fp64 only, D <= 4, with either optimiser.  All
        zeros return the bits of the plain call; None is the plain call.
        ``pred_grad`` (gpsat_fit_predict_batch_grad): also ``f_grad`` and ``f_grad_var`` [sum P, D], the
        gradient of the posterior mean with respect to the prediction point, d f*(x*) / dx*_a, and the posterior variance of
        that derivative, in the units of y (y^2) per unit of X -- numpy arrays or device tensors as ``f_mean`` is.  Every other
        field has the bits of the call without it.  A tile without observations returns the prior at theta0 (0 and
        kernel_variance gg(0) / l_a^2, gg(0) = 1 RBF, 3 Matern32, 5/3 Matern52), a tile that is not positive definite NaN.
        fp64, RBF / Matern32 / Matern52 (Matern12 is not mean-square differentiable), D <= 4, either optimiser; refused beside
        mean, obs_var, cv_fold / cv_refit, n_starts and full_cov.
        ``pred_hess`` (gpsat_fit_predict_batch_hess): True, or {"dims": coordinate indices (default: all),
        "lap_weight": D weights c_a >= 0, 0 outside dims (default: 1 on dims; None: no Laplacian)}.  Also ``f_hess`` and
        ``f_hess_var`` [sum P, m(m+1)/2], d2 f*(x*) / dx*_a dx*_b and its posterior variance for the pairs a <= b of dims in the
        order of ``hess_pairs``, and ``f_lap`` / ``f_lap_var`` [sum P], sum_a c_a d2 f*/dx*_a^2 and its variance (which holds the
        covariances between the second derivatives, not returned otherwise).  Every other field has the bits of the call
        without it.  A tile without observations returns the prior at theta0, a tile that is not positive definite NaN.  fp64,
        RBF / Matern52 (the derivative of a Matern32 process is not mean-square differentiable), D <= 4, either optimiser;
        refused beside what pred_grad is refused beside -- but not beside pred_grad itself, which then comes from the same call.
        Which of these arguments cannot be combined is the table of gpsat_amd/variants.py: a pairing
        that one library call cannot express is refused here, any other by the library with its own message.
        """
        if pred_grad or pred_hess:
            on = {"mean": mean not in (None, "zero"), "noise": obs_var is not None, "cv_refit": cv_refit not in (None, False),
                  "cv": cv_fold is not None and cv_refit in (None, False), "multistart": n_starts is not None, "full_cov": bool(full_cov),
                  "rq": kernel in ("RationalQuadratic", L.KERNEL_RQ)}
            names = {v: k for k, v in L.KERNEL_IDS.items()}
            refusal = V.why_refused_pred_hess if pred_hess else V.why_refused_pred_grad
            why = refusal([k for k in on if on[k]], dtype, kernel if isinstance(kernel, str) else names.get(int(kernel)))
            if why:
                raise GpsatError(why)
        if pred_hess:
            hess_dims, lap_w = _pred_hess_spec(pred_hess, D)
        asked, refit = self._check_call(dtype, kernel, mean, obs_var, cv_fold, cv_refit, n_starts, full_cov, cv_joint)
        self._check_widths(asked, kernel, D, theta0=theta0, lo=lo, hi=hi, trainable=trainable)
        meta = _host_meta(D, (obs_off, pred_off), theta0, lo, hi, trainable, V.n_hyper(D, asked))
        obs_off, pred_off = meta[0]
        T, H, sumN, sumP = len(obs_off) - 1, meta[1].shape[1], int(obs_off[-1]), int(pred_off[-1])
        if isinstance(X, np.ndarray):
            if obs_var is not None:
                if np.size(obs_var) != sumN:
                    raise GpsatError(f"obs_var: {np.size(obs_var)} variances for {sumN} rows")
                obs_var = np.ascontiguousarray(obs_var, dtype=np.float64).reshape(sumN)
            if dtype == "f32" and sumN > 0 and np.asarray(X).dtype == np.float64:
                # fp64 coordinates handed to the fp32 kernels: centre per tile before the cast (see centre_tiles)
                X, Xs = centre_tiles(np.asarray(X, dtype=np.float64).reshape(sumN, D),
                                     np.asarray(Xs, dtype=np.float64).reshape(sumP, D), obs_off, pred_off)
        device_mode, data, preds = self._stage(D, dtype, sumN, sumP, X, y, Xs, out,
                                               None if obs_var is None else {"obs_var": (obs_var, sumN)})
        beside = data[0] if device_mode else None
        run = (kernel, optimiser, max_iter, max_ls, ftol, gtol, adam_lr, want_grad)
        b, res = self._fill_batch(D, dtype, device_mode, meta, data, preds, *run)
        fields = {}
        if full_cov:
            Pt = np.diff(pred_off)
            cov_off = np.concatenate([[0], np.cumsum(Pt * Pt)]).astype(np.int64)
            fc = _alloc(int(cov_off[-1]), dtype, beside, at_least=1)
            b.cov_off, b.f_cov = _ptr(cov_off), _bulk_ptr(fc)
            fields.update(cov_off=cov_off, f_cov=fc[:int(cov_off[-1])])
        key, name = self._entry(asked)
        labels = None if cv_fold is None else _fold_labels(cv_fold, sumN)
        if refit:
            return self._cv_refit(D, dtype, device_mode, meta, data, preds, labels, refit, run, bool(cv_joint))
        args = [self._h, C.byref(b)]
        if key:
            ext, more, keep = self._extension(key, T, H, sumN, dtype, beside, n_starts, starts, obs_var, labels)
            fields.update(more)
            args.append(C.byref(ext))
        if cv_joint and key == "cv":
            name = self._joint_entry(key)
            fold_off, _ = self._cv_fold_off(T, obs_off, labels)
            lpd = np.full(int(fold_off[-1]), np.nan)
            jt = L.GpsatCvJoint()
            jt.fold_off, jt.fold_lpd = _ptr(fold_off), _ptr(lpd)
            fields.update(cv_fold_off=fold_off, cv_lpd=lpd)
            args.append(C.byref(jt))
        if pred_hess:
            name = V.PRED_HESS_ENTRY
            if not hasattr(self._lib, name):
                raise GpsatError(f"this libgpsat_hip.so has no {name} ({V.PRED_HESS_LABEL})")
            pairs = V.pred_hess_pairs(hess_dims)
            ph = getattr(L, V.PRED_HESS_STRUCT)()
            ph.dims = sum(1 << a for a in hess_dims)
            ho = tuple(_alloc(sumP * len(pairs), dtype, beside) for _ in range(2))
            ph.f_hess, ph.f_hess_var = (_bulk_ptr(a) for a in ho)
            fields.update(f_hess=ho[0][:sumP * len(pairs)].reshape(sumP, len(pairs)),
                          f_hess_var=ho[1][:sumP * len(pairs)].reshape(sumP, len(pairs)), hess_pairs=pairs)
            if lap_w is not None:
                for a in range(D):
                    ph.lap_weight[a] = lap_w[a]
                lo_ = tuple(_alloc(sumP, dtype, beside) for _ in range(2))
                ph.f_lap, ph.f_lap_var = (_bulk_ptr(a) for a in lo_)
                fields.update(f_lap=lo_[0][:sumP], f_lap_var=lo_[1][:sumP])
            args.append(C.byref(ph))
        elif pred_grad:
            name = V.PRED_GRAD_ENTRY
            if not hasattr(self._lib, name):
                raise GpsatError(f"this libgpsat_hip.so has no {name} ({V.PRED_GRAD_LABEL})")
            pg = getattr(L, V.PRED_GRAD_STRUCT)()
            args.append(C.byref(pg))
        if pred_grad:                   # the gradient's two outputs: fields of the second derivatives' struct, or of its own
            go = tuple(_alloc(sumP * D, dtype, beside) for _ in range(2))
            wants = ph if pred_hess else pg
            wants.f_grad, wants.f_grad_var = (_bulk_ptr(a) for a in go)
            fields.update(f_grad=go[0][:sumP * D].reshape(sumP, D), f_grad_var=go[1][:sumP * D].reshape(sumP, D))
        rc = getattr(self._lib, name)(*args)
        return self._result(rc, name, res, preds, sumP, **fields)

    @staticmethod
    def _joint_cov_rows(D, T, obs_off, labels):
        """cv_joint with cv_refit: what a tile's folds add to the budget of expanded rows -- the derived batch returns a g x g
        covariance per fold, sum g^2 elements, counted at the D + 1 elements an expanded row holds (rounded up)."""
        tile = np.repeat(np.arange(T, dtype=np.int64), np.diff(obs_off))
        held = labels >= 0
        key = tile[held] * (int(labels.max(initial=0)) + 1) + labels[held].astype(np.int64)
        uk, g = np.unique(key, return_counts=True)
        elems = np.bincount(uk // (int(labels.max(initial=0)) + 1), weights=(g * g).astype(np.float64), minlength=T).astype(np.int64)
        return -(-elems // (D + 1))

    def _cv_refit(self, D, dtype, device_mode, meta, data, preds, labels, opts, run, joint=False) -> BatchResult:
        """gpsat_fit_predict_batch_cv_refit over consecutive ranges of tiles, each within ``max_expanded_rows``; ``joint``:
        gpsat_fit_predict_batch_cv_refit_joint, whose covariances count against the same budget."""
        (obs_off, pred_off), theta0, lo, hi, trainable = meta
        X, y, Xs = data
        T, H = len(obs_off) - 1, theta0.shape[1]
        sumN, sumP = int(obs_off[-1]), int(pred_off[-1])
        entry = self._joint_entry("cv_refit") if joint else "gpsat_fit_predict_batch_cv_refit"
        fold_off, n_rows = self._cv_fold_off(T, obs_off, labels)
        # expanded rows per tile: every fold leaves N - g rows, so F N - (rows that are held out at all)
        held = np.bincount(np.repeat(np.arange(T), np.diff(obs_off))[labels >= 0], minlength=T)
        per_tile = np.diff(fold_off) * np.diff(obs_off) - held
        if int(per_tile.sum()) != n_rows:
            raise GpsatError(f"cv_refit: {int(per_tile.sum())} expanded rows counted here, {n_rows} by gpsat_cv_refit_count")
        if joint:
            per_tile = per_tile + self._joint_cov_rows(D, T, obs_off, labels)
        budget = int(opts["max_expanded_rows"])
        ranges, t0, acc = [], 0, 0
        for t in range(T):
            if per_tile[t] > budget:
                raise GpsatError(f"cv_refit: tile {t} alone expands to {int(per_tile[t])} rows" +
                                 (" (its folds' covariances for cv_joint included)" if joint else "") +
                                 f", above max_expanded_rows = {budget}")
            if acc + per_tile[t] > budget:
                ranges.append((t0, t))
                t0, acc = t, 0
            acc += int(per_tile[t])
        ranges.append((t0, T))
        F = int(fold_off[-1])
        cvo = tuple(_alloc(sumN, dtype, X if device_mode else None) for _ in range(3))
        fo = dict(cv_theta=np.full((F, H), np.nan), cv_nll=np.full(F, np.nan), cv_shift=np.full(F, np.nan),
                  cv_status=np.full(F, 4, dtype=np.int32), cv_n_eval=np.zeros(F, dtype=np.int32), cv_n_iter=np.zeros(F, dtype=np.int32),
                  cv_n_obs=np.zeros(F, dtype=np.int32), cv_label=np.zeros(F, dtype=np.int32))
        if joint:
            fo["cv_lpd"] = np.full(F, np.nan)
        parts, km, tm = [], 0.0, 0.0
        for t0, t1 in ranges:
            a, e, pa, pe, f0, f1 = (int(v) for v in (obs_off[t0], obs_off[t1], pred_off[t0], pred_off[t1], fold_off[t0], fold_off[t1]))
            sub_meta = ((np.ascontiguousarray(obs_off[t0:t1 + 1] - a), np.ascontiguousarray(pred_off[t0:t1 + 1] - pa)),
                        np.ascontiguousarray(theta0[t0:t1]), np.ascontiguousarray(lo[t0:t1]), np.ascontiguousarray(hi[t0:t1]), trainable)
            sub_preds = tuple(p_[pa:pe] if pe > pa else p_[:1] for p_ in preds) if device_mode else tuple(p_[pa:pe] for p_ in preds)
            b, res = self._fill_batch(D, dtype, device_mode, sub_meta, (X[a:e], y[a:e], Xs[pa:pe]), sub_preds, *run)
            sub_off = np.ascontiguousarray(fold_off[t0:t1 + 1] - f0)
            sub_lab = np.ascontiguousarray(labels[a:e])
            cv = L.GpsatCvRefit()
            cv.fold, cv.fold_off = _ptr(sub_lab), _ptr(sub_off)
            cv.start, cv.recentre, cv.min_obs = L.CV_START_IDS[opts["start"]], int(bool(opts["recentre"])), int(opts["min_obs"])
            cv.cv_mean, cv.cv_f_var, cv.cv_y_var = (_bulk_ptr(c_[a:e] if e > a else c_[:1]) for c_ in cvo)
            sub_fo = {k: v[f0:f1] for k, v in fo.items()}          # views: the library writes into the whole arrays
            cv.fold_theta, cv.fold_nll, cv.fold_shift = _ptr(sub_fo["cv_theta"]), _ptr(sub_fo["cv_nll"]), _ptr(sub_fo["cv_shift"])
            cv.fold_status, cv.fold_n_eval, cv.fold_n_iter = _ptr(sub_fo["cv_status"]), _ptr(sub_fo["cv_n_eval"]), _ptr(sub_fo["cv_n_iter"])
            cv.fold_n_obs, cv.fold_label = _ptr(sub_fo["cv_n_obs"]), _ptr(sub_fo["cv_label"])
            more = ()
            if joint:
                jt = L.GpsatCvJoint()
                jt.fold_off, jt.fold_lpd = _ptr(sub_off), _ptr(sub_fo["cv_lpd"])
                more = (C.byref(jt),)
            rc = getattr(self._lib, entry)(self._h, C.byref(b), C.byref(cv), *more)
            r = self._result(rc, entry, res, sub_preds, pe - pa)
            parts.append(res)
            km, tm = km + r.kernel_ms, tm + r.total_ms
        res = {k: (None if parts[0][k] is None else np.concatenate([p_[k] for p_ in parts])) for k in parts[0]}
        fm, fv, yv = (p_[:sumP] for p_ in preds)
        return BatchResult(f_mean=fm, f_var=fv, y_var=yv, kernel_ms=km, total_ms=tm, **res, cv_mean=cvo[0][:sumN], cv_f_var=cvo[1][:sumN],
                           cv_y_var=cvo[2][:sumN], cv_fold_off=fold_off, **fo)

    def sgpr_fit_predict_batch(self, *, D, obs_off, X, y, pred_off, Xs, z_off, Z, theta0, lo=None, hi=None,
                               trainable=None, kernel="Matern32", optimiser="lbfgs", max_iter=10_000, max_ls=0,
                               ftol=0.0, gtol=0.0, adam_lr=0.0, want_grad=False, jitter=0.0, out=None,
                               dtype="f64", full_cov=False, obs_var=None) -> BatchResult:
        """Sparse GP experts (gpsat_sgpr_fit_predict_batch): GPflow SGPR with fixed inducing points Z [sumM, D] per tile
        (CSR ``z_off`` [T+1]).  Arguments and result as ``fit_predict_batch``, except: fp64 only, no ``full_cov``, no
        per-tile observation limit, ``nll`` is the negative ELBO.  Host coordinates are centred per tile (X, Xs and Z by
        the tile's mean observation coordinate) before the call; device tensors are taken as they are."""
        why = V.why_refused(["sgpr"] + ["noise"] * (obs_var is not None) + ["full_cov"] * bool(full_cov), dtype, None)
        if why:
            raise NotImplementedError(why)
        meta = _host_meta(D, (obs_off, pred_off, z_off), theta0, lo, hi, trainable)
        obs_off, pred_off, z_off = meta[0]
        sumN, sumP, sumM = int(obs_off[-1]), int(pred_off[-1]), int(z_off[-1])
        if isinstance(X, np.ndarray):
            X, Xs, Z = centre_tiles(np.asarray(X, dtype=np.float64).reshape(sumN, D), np.asarray(Xs, dtype=np.float64).reshape(sumP, D),
                                    obs_off, pred_off, np.asarray(Z, dtype=np.float64).reshape(sumM, D), z_off)
            Z = np.ascontiguousarray(Z)
        device_mode, data, preds = self._stage(D, dtype, sumN, sumP, X, y, Xs, out, {"Z": (Z, sumM * D)})
        b, res = self._fill_batch(D, dtype, device_mode, meta, data, preds, kernel, optimiser, max_iter, max_ls, ftol, gtol,
                                  adam_lr, want_grad)
        sp = L.GpsatSparse()
        sp.z_off, sp.Z, sp.jitter = _ptr(z_off), _bulk_ptr(Z), float(jitter)
        rc = self._lib.gpsat_sgpr_fit_predict_batch(self._h, C.byref(b), C.byref(sp))
        return self._result(rc, "gpsat_sgpr_fit_predict_batch", res, preds, sumP)

    def select_batch(self, points: np.ndarray, refs: np.ndarray, criteria, points_cm: np.ndarray = None,
                     bounds: np.ndarray = None):
        """Batched tile selection on the GPU (gpsat_select_batch, or gpsat_select_batch_ex when ``bounds`` is given).

        points [M, C] fp64, refs [T, C] fp64 (same column numbering); criteria: list of
        ("cmp", col, comp, val)  ->  points[:, col] <comp> refs[:, col] + val
        ("ball", [cols], comp, r) -> Euclidean ball, comp "<=" (inclusive) or "<" (strict)
        ("interval", col, j)     ->  bounds[:, j, 0] <= points[:, col] < bounds[:, j, 1]  (per expert; NaN never inside)
        bounds: [T, n_bounds, 2] fp64, required by "interval" criteria.
        Returns (off [T+1] int64, idx [off[-1]] int32): selected rows per expert in source order."""
        refs = np.ascontiguousarray(refs, dtype=np.float64)
        T = refs.shape[0]
        if points_cm is not None:                                      # the table already column-major [C][M] (kept by the caller)
            pts_cm = np.ascontiguousarray(points_cm, dtype=np.float64)
            Cc, M = pts_cm.shape
        else:
            points = np.asarray(points, dtype=np.float64)
            M, Cc = points.shape
            pts_cm = np.ascontiguousarray(points.T)                   # column-major [C][M]
        assert refs.shape[1] == Cc
        sp = L.GpsatSelectSpec()
        if not 1 <= len(criteria) <= L.SEL_MAXCRIT:
            raise GpsatError(f"1..{L.SEL_MAXCRIT} criteria supported")
        sp.n_crit = len(criteria)
        nb = 0
        if bounds is not None:
            bounds = np.ascontiguousarray(bounds, dtype=np.float64)
            if bounds.ndim != 3 or bounds.shape[0] != T or bounds.shape[2] != 2 or bounds.shape[1] < 1:
                raise GpsatError(f"bounds must be [T={T}, n_bounds >= 1, 2], got {bounds.shape}")
            nb = bounds.shape[1]
        for k, crit in enumerate(criteria):
            if crit[0] == "interval":
                _, col, j = crit
                if not 0 <= int(j) < nb:
                    raise GpsatError(f"interval criterion {k}: bound pair {j} not in bounds (n_bounds={nb})")
                sp.kind[k], sp.comp[k], sp.ncols[k] = 2, 0, 1
                sp.cols[k][0], sp.cols[k][1] = int(col), int(j)
                continue
            kind, cols, comp, val = crit
            sp.kind[k] = 0 if kind == "cmp" else 1
            sp.comp[k] = L.COMP_IDS[comp]
            cl = [cols] if kind == "cmp" else list(cols)
            sp.ncols[k] = len(cl)
            for m_, c_ in enumerate(cl):
                sp.cols[k][m_] = int(c_)
            sp.val[k] = float(val)
        off = np.zeros(T + 1, dtype=np.int64)
        pb = _ptr(bounds) if nb else None
        rc = self._lib.gpsat_select_batch_ex(self._h, C.byref(sp), M, Cc, _ptr(pts_cm), T, _ptr(refs), nb, pb, _ptr(off), None, 0)
        if rc != 0:
            raise GpsatError(f"gpsat_select_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        idx = np.empty(int(off[-1]), dtype=np.int32)
        if len(idx):
            rc = self._lib.gpsat_select_batch_ex(self._h, C.byref(sp), M, Cc, _ptr(pts_cm), T, _ptr(refs), nb, pb, _ptr(off),
                                                 _ptr(idx), len(idx))
            if rc != 0:
                raise GpsatError(f"gpsat_select_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        return off, idx

    def smooth_batch(self, x, y, vals, l_x: float, l_y: float) -> np.ndarray:
        """Gaussian smoothing of one hyper-parameter field on the GPU (gpsat_smooth_batch; replaces
        gaussian_2d_weight, GPSat/postprocessing.py:22-52, with x0, y0 = x, y as smooth_hyperparameters calls it)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        assert x.shape == y.shape == vals.shape and x.ndim == 1
        out = np.empty_like(vals)
        rc = self._lib.gpsat_smooth_batch(self._h, len(x), _ptr(x), _ptr(y), _ptr(vals), float(l_x), float(l_y), _ptr(out))
        if rc != 0:
            raise GpsatError(f"gpsat_smooth_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        return out

    def glue_batch(self, seg, pred, xprt, vals, sigma) -> np.ndarray:
        """Weighted combination of overlapping predictions (gpsat_glue_batch): rows already sorted into segments
        seg [G+1]; pred, xprt [ndim, R]; vals [nvars, R]; sigma scalar or per row [R]; returns [nvars, G]."""
        seg = np.ascontiguousarray(seg, dtype=np.int64)
        pred = np.ascontiguousarray(pred, dtype=np.float64)
        xprt = np.ascontiguousarray(xprt, dtype=np.float64)
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        ndim, R = pred.shape
        nvars = vals.shape[0]
        assert xprt.shape == pred.shape and vals.shape[1] == R
        G = len(seg) - 1
        out = np.empty((nvars, G), dtype=np.float64)
        srow = None
        if np.ndim(sigma) > 0:
            srow = np.ascontiguousarray(sigma, dtype=np.float64)
            assert srow.shape == (R,)
        rc = self._lib.gpsat_glue_batch(self._h, R, G, ndim, nvars, _ptr(seg), _ptr(pred), _ptr(xprt), _ptr(vals),
                                        0.0 if srow is not None else float(sigma), _ptr(srow) if srow is not None else None,
                                        _ptr(out))
        if rc != 0:
            raise GpsatError(f"gpsat_glue_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        return out

    def _glue_keyed(self, entry, key, pred, xprt, cols, sigma, max_dist):
        """What the keyed glues share.  entry: the C entry point; cols: its value columns in the order of its arguments,
        as (array, rows) with [R] behind the rows -- rows 0: none, [R] alone; a function of ndim; or None: the array's own first
        axis, which the entry point takes behind ndim; every column has an output of its own shape with [G] behind the rows.
        Returns (keys [G], counts [G]) and those outputs."""
        if not hasattr(self._lib, entry):
            raise GpsatError(f"{L.LIB_PATH} does not export {entry}: rebuild the library (there is no host fallback)")
        key = np.ascontiguousarray(key, dtype=np.int64)
        pred = np.ascontiguousarray(pred, dtype=np.float64)
        xprt = np.ascontiguousarray(xprt, dtype=np.float64)
        ndim, R = pred.shape
        assert key.shape == (R,) and xprt.shape == pred.shape
        cols = [(np.ascontiguousarray(c, dtype=np.float64), rows) for c, rows in cols]
        dims = [c.shape[0] for c, rows in cols if rows is None]
        cols = [(c, c.shape[:1] if rows is None else (rows(ndim),) if callable(rows) else ()) for c, rows in cols]
        assert all(c.shape == lead + (R,) for c, lead in cols)
        srow = None
        if np.ndim(sigma) > 0:
            srow = np.ascontiguousarray(sigma, dtype=np.float64)
            assert srow.shape == (R,)
        md = float("inf") if max_dist is None else float(max_dist)
        # capacity R always suffices; only the first G records of the outputs are ever written (untouched pages cost nothing)
        keys, counts = np.empty(R, dtype=np.int64), np.empty(R, dtype=np.int32)
        outs = [np.empty(lead + (R,), dtype=np.float64) for _, lead in cols]
        n = C.c_int64(0)
        rc = getattr(self._lib, entry)(self._h, R, ndim, *dims, _ptr(key), _ptr(pred), _ptr(xprt), *(_ptr(c) for c, _ in cols),
                                       0.0 if srow is not None else float(sigma), _ptr(srow) if srow is not None else None,
                                       md, R, C.byref(n), _ptr(keys), _ptr(counts), *(_ptr(o) for o in outs))
        if rc != 0:
            raise GpsatError(f"{entry} failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        n = int(n.value)
        return (keys[:n].copy(), counts[:n].copy()) + tuple(o[..., :n].copy() for o in outs)

    def glue_keyed_batch(self, key, pred, xprt, vals, sigma, max_dist=None):
        """Weighted combination of overlapping predictions grouped by an integer key on the device
        (gpsat_glue_keyed_batch): rows in any order; key [R] (negative: the row is ignored); pred, xprt [ndim, R];
        vals [nvars, R]; sigma scalar or per row [R]; max_dist: rows at that distance from their expert or beyond stay
        out (None: no limit).  Returns (keys [G] ascending, counts [G] rows that took part, out [nvars, G])."""
        return self._glue_keyed("gpsat_glue_keyed_batch", key, pred, xprt, [(vals, None)], sigma, max_dist)

    def glue_keyed_grad_batch(self, key, pred, xprt, val, grad, sigma, max_dist=None):
        """The glued value and the exact slope of the glued map per key (gpsat_glue_keyed_grad_batch): the arguments of
        glue_keyed_batch with one value column val [R] and its gradient grad [ndim, R] along the glue axes.  Returns
        (keys [G] ascending, counts [G], out_val [G], out_grad [ndim, G]); out_val holds the bytes glue_keyed_batch returns
        for val, out_grad the derivative of that formula with respect to the prediction location, the term from the
        weights' own dependence on it included."""
        return self._glue_keyed("gpsat_glue_keyed_grad_batch", key, pred, xprt, [(val, 0), (grad, lambda ndim: ndim)], sigma, max_dist)

    def glue_keyed_hess_batch(self, key, pred, xprt, val, grad, hess, sigma, max_dist=None):
        """The glued value, the exact slope and the exact second derivatives of the glued map per key
        (gpsat_glue_keyed_hess_batch): the arguments of glue_keyed_grad_batch and hess [npair, R], the second derivatives of
        val for the pairs a <= b of the glue axes in the order of variants.pred_hess_pairs, (0,0), (0,1), (1,1).  Returns
        (keys [G] ascending, counts [G], out_val [G], out_grad [ndim, G], out_hess [npair, G]); out_val and out_grad hold the
        bytes glue_keyed_grad_batch returns, out_hess the second derivative of that formula with respect to the prediction
        location, the terms from the weights' first and second derivatives included."""
        return self._glue_keyed("gpsat_glue_keyed_hess_batch", key, pred, xprt,
                                [(val, 0), (grad, lambda ndim: ndim), (hess, lambda ndim: ndim * (ndim + 1) // 2)], sigma, max_dist)

    def glue_keyed_timing(self):
        """(sort, run detection, reduce) milliseconds of the last glue_keyed_batch, glue_keyed_grad_batch or
        glue_keyed_hess_batch on this engine."""
        ms = np.zeros(3)
        rc = self._lib.gpsat_glue_keyed_timing(self._h, _ptr(ms))
        if rc != 0:
            raise GpsatError(f"gpsat_glue_keyed_timing failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        return tuple(ms)

    def bin_batch(self, x, y, v, gid, n_groups, x_edges, y_edges, statistics, x_hi=None, y_hi=None) -> BinResult:
        """Binned statistics of raw observations, all groups in one call (gpsat_bin_batch; scipy.stats.binned_statistic_2d
        per group, bit for bit).  x, y, v: [R] (y None: one dimension, y_edges is not read); gid: [R] groups 0..n_groups-1 or
        None (one group); x_edges, y_edges: the bin edges as np.linspace made them; statistics: names out of count, sum,
        mean, std, min, max, median.  x_hi / y_hi: inclusive upper limit of the last bin, by default scipy's rounded
        right-edge rule (dataprep.right_edge_limit)."""
        if not hasattr(self._lib, "gpsat_bin_batch"):
            raise GpsatError(f"{L.LIB_PATH} does not export gpsat_bin_batch: rebuild the library (there is no host fallback)")
        from .dataprep import right_edge_limit
        names = [statistics] if isinstance(statistics, str) else list(statistics)
        unknown = [s for s in names if s not in L.BIN_STATS]
        if unknown or not names:
            raise GpsatError(f"statistics {unknown or names}: choose from {list(L.BIN_STATS)}")
        mask = 0
        for s in names:
            mask |= L.BIN_STATS[s]
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        R = x.shape[0]
        assert x.ndim == 1 and v.shape == (R,)
        if R > 2**31 - 1:
            raise GpsatError(f"bin_batch takes at most 2^31 - 1 rows per call, got {R}: bin the table in parts of whole groups")
        ex = np.ascontiguousarray(x_edges, dtype=np.float64)
        xh = right_edge_limit(ex) if x_hi is None else float(x_hi)
        ey, yh, ny = None, 0.0, 0
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            assert y.shape == (R,)
            ey = np.ascontiguousarray(y_edges, dtype=np.float64)
            yh = right_edge_limit(ey) if y_hi is None else float(y_hi)
            ny = len(ey)
        G = int(n_groups)
        if gid is not None:
            gid = np.ascontiguousarray(gid, dtype=np.int32)
            assert gid.shape == (R,)
        elif G > 1:
            raise GpsatError("gid is None: n_groups must be 1")
        rows_y = max(ny - 1, 1)
        cap = int(min(R, G * max(len(ex) - 1, 0) * rows_y))
        keys = np.empty(cap, dtype=np.int64)
        out = np.empty((bin(mask).count("1"), cap), dtype=np.float64)
        n = C.c_int64(0)
        rc = self._lib.gpsat_bin_batch(self._h, R, _ptr(x), _ptr(y), _ptr(v), _ptr(gid), G, len(ex), _ptr(ex), xh, ny, _ptr(ey), yh,
                                       mask, cap, C.byref(n), _ptr(keys), _ptr(out))
        if rc != 0:
            raise GpsatError(f"gpsat_bin_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        n = int(n.value)
        keys = keys[:n].copy()
        order = [s for s in L.BIN_STATS if L.BIN_STATS[s] & mask]             # output rows: ascending bit
        stats = {s: out[order.index(s), :n].copy() for s in names}
        nxb = len(ex) - 1
        cell, ix = np.divmod(keys, nxb) if nxb > 0 else (keys, keys)
        g, iy = np.divmod(cell, rows_y)
        km, tm = C.c_double(0.0), C.c_double(0.0)
        self._lib.gpsat_last_timing(self._h, C.byref(km), C.byref(tm))
        return BinResult(keys=keys, gid=g, iy=iy, ix=ix, stats=stats, kernel_ms=km.value, total_ms=tm.value)

    def _prep_inputs(self, name, arrays, group=None):
        """The [n] fp64 columns of a project_batch / track_batch call (and the int32 group codes) as the library takes them:
        (device_mode, columns, group, n).  NumPy arrays are laid out contiguously; device tensors are checked, not copied."""
        if not hasattr(self._lib, name):
            raise GpsatError(f"{L.LIB_PATH} does not export {name}: rebuild the library (there is no host fallback)")
        device_mode = not isinstance(arrays[0], np.ndarray) and hasattr(arrays[0], "data_ptr")
        if device_mode:
            import torch
            n = arrays[0].numel()
            for k, t_ in enumerate(arrays):
                self._check_tensor(f"{name}: column {k}", t_, "f64", numel=n)
            if group is not None:
                if not isinstance(group, torch.Tensor) or group.dtype != torch.int32 or not group.is_contiguous() or \
                        group.device != arrays[0].device or group.numel() != n:
                    raise GpsatError(f"{name}: group must be a contiguous int32 tensor of {n} codes beside the columns")
            torch.cuda.current_stream(arrays[0].device).synchronize()      # inputs must be complete before our stream reads them
        else:
            arrays = [np.ascontiguousarray(a_, dtype=np.float64).reshape(-1) for a_ in arrays]
            n = arrays[0].shape[0]
            if any(a_.shape != (n,) for a_ in arrays):
                raise GpsatError(f"{name}: columns of {[a_.shape[0] for a_ in arrays]} rows")
            if group is not None:
                group = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
                if group.shape != (n,):
                    raise GpsatError(f"{name}: {group.shape[0]} group codes for {n} rows")
        if n > 2**31 - 1:
            raise GpsatError(f"{name} takes at most 2^31 - 1 rows per call, got {n}")
        return device_mode, list(arrays), group, n

    def _prep_timing(self):
        km, tm = C.c_double(0.0), C.c_double(0.0)
        self._lib.gpsat_last_timing(self._h, C.byref(km), C.byref(tm))
        self.last_prep_ms = (km.value, tm.value)

    def project_batch(self, in0, in1, direction="forward", lon_0=0.0, lat_0=90.0):
        """Lambert azimuthal equal-area projection on WGS84, polar aspects (gpsat_project_batch).  direction "forward":
        in0, in1 = lon, lat in degrees -> (x, y) in metres; "inverse": x, y -> (lon, lat).  in0, in1: [n] NumPy arrays or
        fp64 device tensors; the outputs are of the same kind.  (kernel, total) ms of the call: ``last_prep_ms``."""
        if direction not in L.PROJECT_IDS:
            raise GpsatError(f"direction {direction!r}: choose from {list(L.PROJECT_IDS)}")
        dev, (a0, a1), _, n = self._prep_inputs("gpsat_project_batch", [in0, in1])
        if dev:
            import torch
            o0, o1 = torch.empty(max(n, 1), dtype=a0.dtype, device=a0.device), torch.empty(max(n, 1), dtype=a0.dtype, device=a0.device)
        else:
            o0, o1 = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        p = L.GpsatProject(n=n, direction=L.PROJECT_IDS[direction], memory=L.MEM_DEVICE if dev else L.MEM_HOST,
                           lon_0=float(lon_0), lat_0=float(lat_0), in0=_bulk_ptr(a0), in1=_bulk_ptr(a1), out0=_bulk_ptr(o0),
                           out1=_bulk_ptr(o1))
        rc = self._lib.gpsat_project_batch(self._h, C.byref(p))
        if rc != 0:
            raise GpsatError(f"gpsat_project_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        self._prep_timing()
        return o0[:n], o1[:n]

    def track_batch(self, cols, group=None, cut_off=0.0, start_track=0, mode="cut"):
        """Distance to the previous row of the same group and the track number of every row (gpsat_track_batch).
        cols: 1..3 columns [n] (NumPy or fp64 device tensors); group: int32 codes [n] in order of first appearance, -1 for a
        row in no group, or None.  The rows are taken group by group, in the order given inside a group.  Returns
        (delta, track, order), all in the order taken: order[i] is the source row taken i-th; rows of code -1 come last with
        delta NaN and track -1.  mode "cut": track = start_track + the flags so far (delta > cut_off, or the first row of a
        later group); mode "given": the same on distances that are there already (cols[0] is delta, a group's first row
        included); mode "runs": track = rows since cols[0] last changed (delta is None)."""
        if mode not in L.TRACK_MODES:
            raise GpsatError(f"mode {mode!r}: choose from {list(L.TRACK_MODES)}")
        cols = list(cols)
        if not 1 <= len(cols) <= (3 if mode == "cut" else 1):
            raise GpsatError(f"track_batch takes 1..3 columns (mode 'runs' and 'given': one), got {len(cols)}")
        dev, cols, group, n = self._prep_inputs("gpsat_track_batch", cols, group)
        runs = mode == "runs"
        if dev:
            import torch
            where = dict(device=cols[0].device)
            delta = None if runs else torch.empty(max(n, 1), dtype=torch.float64, **where)
            track, order = torch.empty(max(n, 1), dtype=torch.int32, **where), torch.empty(max(n, 1), dtype=torch.int32, **where)
        else:
            delta = None if runs else np.empty(n, dtype=np.float64)
            track, order = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        t = L.GpsatTrack(n=n, n_cols=len(cols), memory=L.MEM_DEVICE if dev else L.MEM_HOST,
                         group=None if group is None else _bulk_ptr(group), cut_off=float(cut_off), start_track=int(start_track),
                         mode=L.TRACK_MODES[mode], out_delta=None if runs else _bulk_ptr(delta), out_track=_bulk_ptr(track),
                         out_order=_bulk_ptr(order))
        for k, c_ in enumerate(cols):
            t.cols[k] = c_.data_ptr() if dev else c_.ctypes.data
        rc = self._lib.gpsat_track_batch(self._h, C.byref(t))
        if rc != 0:
            raise GpsatError(f"gpsat_track_batch failed ({rc}): {self._lib.gpsat_last_error().decode()}")
        self._prep_timing()
        return (None if runs else delta[:n]), track[:n], order[:n]


_default_engine = None


def default_engine() -> Engine:
    """Process-wide engine on LOCAL_RANK's GPU (one process per GPU)."""
    global _default_engine
    if _default_engine is None:
        import os
        _default_engine = Engine(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_engine
