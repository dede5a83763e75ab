"""Raw rows to the columns the pipeline starts from, on the GPU: lon / lat to EASE2 metres and back, and track numbers.

The names and signatures are the reference's (GPSat/utils.py): ``WGS84toEASE2`` / ``EASE2toWGS84`` (there: pyproj,
"+proj=laea +lat_0=.. +lon_0=.. +ellps=WGS84") and ``diff_distance`` / ``guess_track_num`` / ``track_num_for_date`` (there:
numba loops), as ``examples/generate_track_id.py`` uses them.  Every number comes from the device
(``Engine.project_batch`` / ``Engine.track_batch``, gpsat_amd/csrc/gpsat_prep.hip); there is no host fallback, and what the
kernels are not built for raises.

Differences that are on purpose: only the polar aspects (``lat_0`` = 90 or -90) and WGS84; the inverse is
exact to rounding where PROJ truncates a series (its documented latitude differs by 9.5e-10 degrees); scalars come back as
Python floats, arrays and Series as NumPy arrays.
"""
from __future__ import annotations

import warnings

import numpy as np


def _engine():
    from .engine import default_engine
    return default_engine()


def _project(direction, a, b, lon_0, lat_0, engine):
    scalar = np.ndim(a) == 0 and np.ndim(b) == 0
    a64, b64 = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    shape = a64.shape
    o0, o1 = (engine or _engine()).project_batch(a64.reshape(-1), b64.reshape(-1), direction, lon_0, lat_0)
    if scalar:
        return float(o0[0]), float(o1[0])
    return np.asarray(o0).reshape(shape), np.asarray(o1).reshape(shape)


def WGS84toEASE2(lon, lat, return_vals="both", lon_0=0, lat_0=90, engine=None):
    """lon, lat in decimal degrees -> EASE2 (x, y) in metres; ``return_vals``: "both", "x" or "y"."""
    valid_return_vals = ['both', 'x', 'y']
    assert return_vals in valid_return_vals, f"return_val: {return_vals} is not in valid set: {valid_return_vals}"
    x, y = _project("forward", lon, lat, lon_0, lat_0, engine)
    return {"both": (x, y), "x": x, "y": y}[return_vals]


def EASE2toWGS84(x, y, return_vals="both", lon_0=0, lat_0=90, engine=None):
    """EASE2 x, y in metres -> (lon, lat) in decimal degrees, lon in (-180, 180]; ``return_vals``: "both", "lon" or "lat"."""
    valid_return_vals = ['both', 'lon', 'lat']
    assert return_vals in valid_return_vals, f"return_val: {return_vals} is not in valid set: {valid_return_vals}"
    lon, lat = _project("inverse", x, y, lon_0, lat_0, engine)
    return {"both": (lon, lat), "lon": lon, "lat": lat}[return_vals]


def WGS84toEASE2_New(*args, **kwargs):
    warnings.warn("WGS84toEASE2_New will be removed in future versions. Use `WGS84toEASE2` instead.", DeprecationWarning, stacklevel=2)
    return WGS84toEASE2(*args, **kwargs)


def EASE2toWGS84_New(*args, **kwargs):
    warnings.warn("EASE2toWGS84_New will be removed in future versions. Use `EASE2toWGS84` instead.", DeprecationWarning, stacklevel=2)
    return EASE2toWGS84(*args, **kwargs)


def diff_distance(x, p=2, k=1, default_val=np.nan, engine=None):
    """Euclidean distance of every row of ``x`` ([n] or [n, C], C <= 3) to the row before it; the first row gets
    ``default_val``.  Built for p = 2 and k = 1, what the track assignment uses."""
    if p != 2 or k != 1:
        raise NotImplementedError(f"diff_distance is built for p=2, k=1 (got p={p}, k={k}): there is no host fallback")
    x = np.asarray(x, dtype=np.float64)
    if len(x.shape) == 1:
        x = x[:, None]
    assert len(x.shape) == 2, f"x must be 2d, len(x.shape) = {len(x.shape)}"
    if not 1 <= x.shape[1] <= 3:
        raise NotImplementedError(f"diff_distance is built for 1..3 columns, got {x.shape[1]}")
    if x.shape[0] == 0:
        return np.full(0, default_val, dtype=np.float64)
    delta, _, _ = (engine or _engine()).track_batch([np.ascontiguousarray(x[:, c]) for c in range(x.shape[1])])
    out = np.array(delta, dtype=np.float64)
    out[0] = default_val
    return out


def guess_track_num(x, thresh, start_track=0, engine=None):
    """A track number per row: it goes up by one wherever ``x`` (the distance to the previous row, as diff_distance makes it)
    exceeds ``thresh``; NaN does not.  Returned as fp64, as the reference's."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if x.shape[0] == 0:
        return np.full(0, np.nan)
    if not np.isfinite(thresh):
        raise NotImplementedError("guess_track_num: thresh must be finite")
    _, track, _ = (engine or _engine()).track_batch([x], cut_off=float(thresh), start_track=int(start_track), mode="given")
    return np.asarray(track, dtype=np.float64)


def track_num_for_date(x, engine=None):
    """Rows since the value of ``x`` last changed (0 where a row differs from the one before it), as fp64."""
    x = np.asarray(x)
    if x.shape[0] == 0:
        return np.full(0, np.nan)
    x64 = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if np.issubdtype(x.dtype, np.integer) and not (x64.astype(x.dtype) == x.reshape(-1)).all():
        raise NotImplementedError("track_num_for_date: integers beyond 2^53 do not survive the device's fp64 column")
    _, run, _ = (engine or _engine()).track_batch([x64], mode="runs")
    return np.asarray(run, dtype=np.float64)
