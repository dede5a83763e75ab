"""What the device-mode tests (tests/test_gpu_device_mode.py) share: the carved allocation with its guard bands, the comparison
of a device-mode BatchResult with the host-mode one field by field, the ragged batches and the launch plan of a batch.

Device mode (gpsat_amd/engine.py, GPSAT_MEM_DEVICE): the kernels read the caller's tensors and write the predictions into the
caller's ``out``.  The contract: the bits of host mode in every field, nothing written outside
``out[i][:sumP]``, the inputs untouched.
"""
import ctypes as C
import dataclasses

import numpy as np

from gpsat_amd import _lib as L
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult
from oracle import gp_oracle as go
from test_abi import _PlanInput, _TilePlan           # the ctypes mirrors of gpsat::PlanInput / gpsat::TilePlan

KERNELS = ["RBF", "Matern12", "Matern32", "Matern52"]
NP = {"f32": np.float32, "f64": np.float64}
GUARD = 64                                            # elements of sentinel between neighbours and at both ends
SENTINEL = -7777.25                                   # exact in fp32 and fp64; no kernel here produces it
RESULT_FIELDS = [f.name for f in dataclasses.fields(BatchResult) if f.name not in ("kernel_ms", "total_ms")]
DEVICE_FIELDS = ("f_mean", "f_var", "y_var", "f_cov", "cv_mean", "cv_f_var", "cv_y_var")
TALLY = {}                                            # case family -> [device runs compared, fields compared, fields None in both]


class Carved:
    """``arrays`` (name -> numpy array of the call's dtype) and ``outs`` (name -> elements) as views into ONE device allocation:
    every view starts at an odd element offset (no more alignment than the element size, which is all host staging gives y
    and Xs either) and a band of GUARD sentinel elements lies between neighbours and at both ends; the outputs are filled
    with the sentinel too.  An input without elements is a tensor of its own without storage (data_ptr() == 0): that is what
    a caller without prediction points hands over."""

    def __init__(self, arrays, outs, dtype, device):
        import torch
        self.np_dt = NP[dtype]
        t_dt = torch.float32 if dtype == "f32" else torch.float64
        pos, self.where = GUARD + 1, {}
        for name, n in [(k, int(np.size(v))) for k, v in arrays.items()] + [(k, int(n)) for k, n in outs.items()]:
            assert pos % 2 == 1
            self.where[name] = (pos, n)
            pos += n + GUARD
            pos += 1 - pos % 2
        self.image = np.full(pos, SENTINEL, dtype=self.np_dt)          # what the allocation holds before the call
        for name, v in arrays.items():
            a, n = self.where[name]
            assert np.asarray(v).dtype == self.np_dt, (name, np.asarray(v).dtype)
            self.image[a:a + n] = np.asarray(v).reshape(-1)
        self.buf = torch.tensor(self.image, device=device)             # a copy, in an allocation of its own
        assert self.buf.dtype == t_dt and self.buf.data_ptr() % 64 == 0
        self.inputs, self.outs = {}, {}
        for name, v in arrays.items():
            a, n = self.where[name]
            self.inputs[name] = self.buf[a:a + n].view(np.shape(v)) if n else torch.empty(np.shape(v), dtype=t_dt, device=device)
            assert n == 0 or self.inputs[name].data_ptr() == self.buf.data_ptr() + a * self.image.itemsize
        for name, n in outs.items():
            a, _ = self.where[name]
            self.outs[name] = self.buf[a:a + n]

    def verify(self, written):
        """After the call.  ``written``: the leading elements of every output the call may have changed (sumP).  Asserts that
        every guard band still holds its fill, every input the bytes that were uploaded, and every output beyond ``written``
        the sentinel.  Returns the allocation as it is now (numpy)."""
        now = self.buf.cpu().numpy()
        regions, end = [], 0
        for name, (a, n) in self.where.items():                       # in the order of the layout
            regions.append((f"the guard band before {name}", end, a))
            is_out = name in self.outs
            regions.append((f"the output {name} beyond its first {written} elements" if is_out else f"the input {name}",
                            a + (min(written, n) if is_out else 0), a + n))
            end = a + n
        regions.append(("the guard band at the end", end, len(now)))
        assert sum(e - a for _, a, e in regions) + sum(min(written, n) for k, (a, n) in self.where.items() if k in self.outs) == len(now)
        for what, a, e in regions:
            bad = np.flatnonzero(now[a:e].view(np.uint8) != self.image[a:e].view(np.uint8))
            assert bad.size == 0, f"{what} was written to: {bad.size} bytes differ, the first at element {a + bad[0] // now.itemsize} of the allocation"
        return now


def to_numpy(r):
    """The BatchResult with every tensor downloaded."""
    import torch
    return dataclasses.replace(r, **{k: getattr(r, k).cpu().numpy() for k in DEVICE_FIELDS if isinstance(getattr(r, k), torch.Tensor)})


def same_result(host, dev, device_id, family, what=""):
    """Every field of the device-mode result ``dev`` against the host-mode result ``host``: None where that is None, else the
    same dtype, shape and bytes; prediction outputs are torch tensors on the engine's device.  Counted in TALLY[family]."""
    import torch
    tally = TALLY.setdefault(family, [0, 0, 0])
    tally[0] += 1
    for name in RESULT_FIELDS:
        h, d = getattr(host, name), getattr(dev, name)
        if h is None:
            assert d is None, (what, name)
            tally[2] += 1
            continue
        assert d is not None, (what, name)
        if name in DEVICE_FIELDS:
            assert isinstance(d, torch.Tensor) and d.is_cuda and d.device.index == device_id, (what, name, type(d))
            d = d.cpu().numpy()
        else:
            assert isinstance(d, np.ndarray), (what, name, type(d))
        h = np.asarray(h)
        assert h.dtype == d.dtype and h.shape == d.shape, (what, name, h.dtype, d.dtype, h.shape, d.shape)
        assert h.tobytes() == d.tobytes(), f"{what}: {name} differs between host and device mode in " \
                                           f"{int((np.ascontiguousarray(h).view(np.uint8) != np.ascontiguousarray(d).view(np.uint8)).sum())} bytes"
        tally[1] += 1


def make_batch(dtype, Ns, Ps, D=3, kid=2, seed=4000):
    """synthetic.make_tile tiles in the call's dtype (host fp32 runs are given float32 arrays: fp64 input would be re-centred),
    as the dict the helpers of tests/variant_cases.py read."""
    b = syn.make_batch(len(Ns), Ns, Ps, D, kid, base_seed=seed, dtype=NP[dtype])
    b["kernel"] = KERNELS[kid]
    return b


# the smallest shapes at which indexing goes wrong: around the block (32 in fp32, 16 in fp64), an empty tile in the middle,
# tiles without prediction points
RAGGED_N = {"f32": [1, 31, 32, 0, 33, 100], "f64": [1, 15, 16, 0, 17, 100]}
RAGGED_P = [0, 1, 33, 7, 0, 32]
EMPTY = 3


def ragged(dtype, D=3, kid=2, seed=4000):
    return make_batch(dtype, RAGGED_N[dtype], RAGGED_P, D, kid, seed)


def meta_of(b):
    return dict(D=b["D"], obs_off=b["obs_off"], pred_off=b["pred_off"])


def run_pair(eng, b, dtype, kw, family, out="exact", more=(), entry="fit_predict_batch", flat=False, what=""):
    """The call in host mode and in device mode on a carved allocation; every field compared, the allocation verified.
    ``out``: None (the engine allocates), "exact" (sumP elements; one where sumP == 0) or "over" (sumP + 37).  ``more``: the
    bulk inputs beyond X, y, Xs (obs_var, Z).  ``flat``: the device tensors are one-dimensional.
    Returns (host result, device result downloaded, device result, Carved)."""
    import torch
    call = getattr(eng, entry)
    names = ("X", "y", "Xs") + tuple(more)
    host = call(**meta_of(b), **{k: b[k] for k in names}, **kw)
    sumP = int(b["pred_off"][-1])
    n_out = {None: 0, "exact": max(sumP, 1), "over": sumP + 37}[out]
    c = Carved({k: (np.ascontiguousarray(b[k]).reshape(-1) if flat else np.ascontiguousarray(b[k])) for k in names},
               {} if out is None else {k: n_out for k in ("f_mean", "f_var", "y_var")}, dtype, torch.device("cuda", eng.device_id))
    dev = call(**meta_of(b), **c.inputs, **({} if out is None else {"out": tuple(c.outs.values())}), **kw)
    c.verify(sumP)
    same_result(host, dev, eng.device_id, family, what)
    if out is not None:
        for k in ("f_mean", "f_var", "y_var"):
            assert getattr(dev, k).data_ptr() == c.outs[k].data_ptr() or sumP == 0, (what, k)
            assert getattr(dev, k).shape == (sumP,), (what, k)
    return host, to_numpy(dev), dev, c


# ---- the fp64 reference at the project's bounds, for what tests/variant_cases.check_tile does not cover
def check_cov_tile(r, b, t, theta, dtype):
    """Tile t of a full_cov result: the bounds of tests/test_gpu_parity.py::test_full_cov_ragged_batch_matches_oracle."""
    D, kid = b["D"], KERNELS.index(b["kernel"])
    a, e, pa, pe = (int(v) for v in (b["obs_off"][t], b["obs_off"][t + 1], b["pred_off"][t], b["pred_off"][t + 1]))
    P = pe - pa
    Cv = np.asarray(r.f_cov[r.cov_off[t]:r.cov_off[t + 1]], dtype=np.float64).reshape(P, P)
    if P == 0:
        return
    Xs = b["Xs"][pa:pe].astype(np.float64)
    ref = go.kernel_matrix(kid, Xs, Xs, theta[:D], theta[D]) if e == a else \
        go.predict_cov(kid, b["X"][a:e].astype(np.float64), b["y"][a:e].astype(np.float64), Xs, theta)[0]
    tol = 1e-9 if dtype == "f64" else 3e-5
    np.testing.assert_allclose(Cv, ref, rtol=0, atol=tol * theta[D] / 0.8 * 1.0)
    np.testing.assert_array_equal(Cv, Cv.T)
    np.testing.assert_allclose(np.diag(Cv), np.asarray(r.f_var[pa:pe], dtype=np.float64), rtol=0, atol=tol)


def check_refit_fold(r, b, labels, t, dtype):
    """Every fitted fold of tile t of a cv_refit result (recentre on) against the oracle at the parameters the call returned
    for the fold: tests/test_gpu_cv_refit.py::test_against_the_oracle (a) in fp64 -- mean 1e-9 max(|y|max, 1), variances
    1e-10, the shift 1e-15 max(|y|max, 1) -- and in fp32 the fp64 -> fp32 prediction bounds of tests/test_gpu_parity.py
    (mean 2e-3 |y|max, f*_var 2e-3 sf2 + 1e-6).  Returns the folds checked."""
    D, kid = b["D"], KERNELS.index(b["kernel"])
    a, e = int(b["obs_off"][t]), int(b["obs_off"][t + 1])
    X, y, lab = b["X"][a:e].astype(np.float64), b["y"][a:e].astype(np.float64), labels[a:e]
    ymax, n = max(float(np.abs(b["y"]).max()), 1.0), 0
    for k, v in enumerate(np.unique(lab[lab >= 0])):
        f, G = int(r.cv_fold_off[t]) + k, lab == v
        assert r.cv_label[f] == v and r.cv_n_obs[f] == (~G).sum()
        if r.cv_status[f] in (2, 3, 4):
            continue
        shift = float(y[~G].mean())
        assert abs(r.cv_shift[f] - shift) <= 1e-15 * ymax
        fm, fv, yv = go.predict(kid, X[~G], y[~G] - shift, X[G], r.cv_theta[f])
        rows = a + np.flatnonzero(G)
        err = (np.abs(r.cv_mean[rows] - (fm + shift)).max(), np.abs(r.cv_f_var[rows] - fv).max(), np.abs(r.cv_y_var[rows] - yv).max())
        print(f"refit {dtype} tile {t} fold {f}: mean {err[0]:.2e} f_var {err[1]:.2e} y_var {err[2]:.2e}")
        if dtype == "f64":
            assert err[0] <= 1e-9 * ymax and err[1] <= 1e-10 and err[2] <= 1e-10
        else:
            assert err[0] <= 2e-3 * np.abs(y).max() and err[1] <= 2e-3 * r.cv_theta[f][D] + 1e-6
        n += 1
    return n


# ---- the launch plan of a batch, from gpsat::plan_tiles on the same offsets
BUILD_F32_W4, BUILD_F32_W8, BUILD_F64_W8, BUILD_F64_W4 = 0, 1, 2, 3
KNOBS = ("team", "coop", "coop_xcd", "coop_min_nb", "coop_hdiv", "grid", "seg", "defer")      # gpsat::DevKnobs, in order


def plan_of(b, dtype, num_cu, optimiser, max_iter, wg_per_cu=2, solo=0, knobs=None):
    """gpsat::plan_tiles for the batch as gpsat_fit_predict_batch asks it (no full covariance): a dict of TilePlan."""
    fn = getattr(L.load(), "_ZN5gpsat10plan_tilesERKNS_9PlanInputERNS_8TilePlanE")
    fn.restype, fn.argtypes = C.c_bool, [C.POINTER(_PlanInput), C.POINTER(_TilePlan)]
    off = np.ascontiguousarray(b["obs_off"], dtype=np.int64)
    pin = _PlanInput(T=len(off) - 1, D=b["D"], f64=int(dtype == "f64"), obs_off=off.ctypes.data_as(C.POINTER(C.c_int64)), maxP=0,
                     want_cov=0, has_pred=int(b["pred_off"][-1] > 0), optimiser=L.OPT_IDS[optimiser], max_iter=max_iter,
                     num_cu=num_cu, wg_per_cu=wg_per_cu, solo=solo, unsliced=0)
    for name, v in (knobs or {}).items():
        pin.knobs[KNOBS.index(name)].set, pin.knobs[KNOBS.index(name)].v = 1, int(v)
    plan = _TilePlan()
    assert fn(C.byref(pin), C.byref(plan))
    return {n: getattr(plan, n) for n, _ in _TilePlan._fields_}
