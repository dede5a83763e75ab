"""NumPy restatement of gpsat_amd/csrc/gpsat_prep.hip: what the new tests hold the device to.

Projection: Lambert azimuthal equal-area on the WGS84 ellipsoid, polar aspects, Snyder's formulas (3-12, 24-23, 24-25; the
inverse by Newton's iteration on q(phi) = q, 3-16, written in the angle from the nearer pole), the operations in the kernel's
order.  Tracks: the loops of the reference's
guess_track_num, track_num_for_date and TrackId.add_tracks written out one row after the other, no numba, no vectorising --
slow and plain on purpose."""
import numpy as np

A = 6378137.0
F = 1.0 / 298.257223563
E2 = F * (2.0 - F)
E = np.sqrt(E2)
ONE_M_E2 = 1.0 - E2
INV_2E = 1.0 / (2.0 * E)
QP = ONE_M_E2 * (1.0 / ONE_M_E2 - np.log((1.0 - E) / (1.0 + E)) * INV_2E)
DEG = np.pi / 180.0
RAD = 180.0 / np.pi
NEWTON_MAX = 8


def authalic_q(s):
    es = E * s
    return ONE_M_E2 * (s / (1.0 - E2 * s * s) - np.log((1.0 - es) / (1.0 + es)) * INV_2E)


def _aspect(lat_0):
    assert lat_0 in (90, -90), "polar aspects only"
    return lat_0 < 0


def laea_forward(lon, lat, lon_0=0.0, lat_0=90.0):
    """(x, y) in metres of lon, lat in degrees."""
    south = _aspect(lat_0)
    lon, lat = np.broadcast_arrays(np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        s = np.sin(lat * DEG)
        q = authalic_q(s)
        d = np.maximum(QP + q if south else QP - q, 0.0)
        d = np.where(s == (-1.0 if south else 1.0), 0.0, d)          # the pole itself, whatever the last bit of the logarithm
        rho = A * np.sqrt(d)
        dl = (lon - lon_0) * DEG
        x = rho * np.sin(dl)
        y = rho * np.cos(dl) if south else -(rho * np.cos(dl))
    bad = np.isnan(lon) | np.isnan(lat)
    return np.where(bad, np.nan, x), np.where(bad, np.nan, y)


# q_p to twice the working precision (mpmath, 50 digits): QP + QP_LO is the true value, QP the fp64 formula's
QP_TRUE_HI, QP_TRUE_LO = 1.9955310875028367, 9.345699910345638e-17
QP_LO = (QP_TRUE_HI - QP) + QP_TRUE_LO
HALF_PI_HI, HALF_PI_LO = 1.5707963267948966, 6.123233995736766e-17


def _two_prod(a, b):
    """a b = p + e exactly (Dekker's split; the kernel has fma for it)."""
    p = a * b
    c = 134217729.0
    ah = c * a - (c * a - a)
    bh = c * b - (c * b - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def pole_distance(x, y):
    """delta = q_p - |q| of the point, measured from the NEARER pole, and whether that is the far one.  (rho / a)^2 is carried
    in two doubles: beyond the equator 2 q_p - (rho / a)^2 is a difference of numbers near 4 and its error decides phi."""
    p1, e1 = _two_prod(x, x)
    p2, e2 = _two_prod(y, y)
    sh, se = _two_sum(p1, p2)
    sl = se + (e1 + e2)
    a2 = A * A                                   # an integer below 2^53: exact
    q1 = sh / a2
    m, me = _two_prod(q1, a2)
    q2 = (((sh - m) - me) + sl) / a2
    far = q1 > QP
    near_delta = q1 + q2
    far_delta = (2.0 * QP - q1) + (2.0 * QP_LO - q2)          # the first difference is exact (Sterbenz)
    return np.where(far, far_delta, near_delta), far


def pole_g(psi):
    """q_p - q(90 degrees - psi) without a cancellation: with s = cos(psi), u = 1 - s = 2 sin^2(psi / 2),
    u (1 + e^2 s) / (1 - e^2 s^2) + (1 - e^2) / e atanh(e u / (1 - e^2 s)); and its derivative."""
    h = np.sin(0.5 * psi)
    u = 2.0 * h * h
    sc = 1.0 - u
    z = E * u / (1.0 - E2 * sc)
    w = 1.0 - E2 * sc * sc
    g = u * (1.0 + E2 * sc) / w + (ONE_M_E2 / E) * (0.5 * np.log1p(2.0 * z / (1.0 - z)))
    dg = 2.0 * ONE_M_E2 * np.sin(psi) / (w * w)
    return g, dg


def laea_inverse(x, y, lon_0=0.0, lat_0=90.0):
    """(lon, lat) in degrees of x, y in metres; lon in (-180, 180].  The latitude is found as the angle psi from the nearer
    pole: Newton's iteration on q_p - q(phi) = delta (Snyder 3-16 written in psi), which has no cancellation at either pole."""
    south = _aspect(lat_0)
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    x, y = x.astype(np.float64), y.astype(np.float64)
    lon, lat = np.full(x.shape, np.nan), np.full(x.shape, np.nan)
    pole = -90.0 if south else 90.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rx, ry = x / A, y / A
        r2 = rx * rx + ry * ry
        nan = np.isnan(x) | np.isnan(y)
        out = ~nan & (r2 > 2.0 * QP)
        zero = ~nan & (r2 == 0.0)
        rest = ~nan & ~out & ~zero
        lon[out], lat[out] = np.inf, np.inf
        lon[zero], lat[zero] = lon_0, pole
        delta, far = pole_distance(x[rest], y[rest])
        delta = np.maximum(delta, 0.0)
        psi = 2.0 * np.arcsin(np.sqrt(np.minimum(delta / (2.0 * QP), 1.0)))          # the authalic angle: within 0.4 %
        live = delta > 0.0
        for _ in range(NEWTON_MAX):
            if not live.any():
                break
            p = psi[live]
            g, dg = pole_g(p)
            step = (g - delta[live]) / dg
            p = p - step
            psi[live] = p
            idx = np.flatnonzero(live)
            live[idx[np.abs(step) <= 2.0 ** -53 * np.abs(p)]] = False
        phi = (HALF_PI_HI - psi) + HALF_PI_LO                  # from the nearer pole back to the latitude
        phi = np.where(far != south, -phi, phi)
        lat[rest] = phi * RAD
        lo = lon_0 + np.arctan2(x[rest], y[rest] if south else -y[rest]) * RAD
        lon[rest] = lo - 360.0 * np.ceil((lo - 180.0) / 360.0)
    return lon, lat


# ---- tracks: the reference's loops
def diff_distance(x, default_val=np.nan):
    """Distance of every row of x [n] or [n, C] to the row before it (p = 2, k = 1): difference, square, sum from the left,
    root; the first row gets default_val."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    out = np.full(x.shape[0], default_val, dtype=np.float64)
    for i in range(1, x.shape[0]):
        s = None
        for c in range(x.shape[1]):
            df = x[i, c] - x[i - 1, c]
            sq = df * df
            s = sq if s is None else s + sq
        out[i] = np.sqrt(s)
    return out


def guess_track_num(x, thresh, start_track=0):
    """One number per row, fp64 as the reference returns it: the count goes up by one at every row whose value lies above
    thresh (a NaN does not), the row included."""
    current, numbers = start_track, []
    for value in x:
        current += 1 if value > thresh else 0
        numbers.append(float(current))
    return np.array(numbers, dtype=np.float64)


def track_num_for_date(x):
    """Rows since the value last changed (a row that differs from the one before it, NaN included, gets 0), fp64."""
    since, counts = 0, []
    for i, value in enumerate(x):
        since = since + 1 if i > 0 and value == x[i - 1] else 0
        counts.append(float(since))
    return np.array(counts, dtype=np.float64)


def tracks_by_group(cols, codes, cut_off, start_track=0):
    """The group loop of TrackId.add_tracks over rows that are already sorted: groups in ascending code (the codes are numbered
    in order of first appearance), per group diff_distance and guess_track_num, the next group starting one above the last
    group's largest track.  cols [n, C]; codes [n] (-1: in no group) or None.  Returns (order, delta, track): the source rows
    in the order the loop emits them, rows of code -1 last with delta NaN and track -1."""
    cols = np.asarray(cols, dtype=np.float64)
    if cols.ndim == 1:
        cols = cols[:, None]
    n = cols.shape[0]
    codes = np.zeros(n, dtype=np.int64) if codes is None else np.asarray(codes)
    order, delta, track = [], [], []
    for g in sorted(set(int(c) for c in codes if c >= 0)):
        rows = np.flatnonzero(codes == g)
        d = diff_distance(cols[rows])
        tr = guess_track_num(d, cut_off, start_track).astype(np.int64)
        start_track = int(tr.max()) + 1
        order.append(rows), delta.append(d), track.append(tr)
    rest = np.flatnonzero(codes < 0)
    order.append(rest), delta.append(np.full(len(rest), np.nan)), track.append(np.full(len(rest), -1, dtype=np.int64))
    return (np.concatenate(order).astype(np.int64), np.concatenate(delta).astype(np.float64), np.concatenate(track).astype(np.int64))


class NumpyPrepEngine:
    """A device-free stand-in for Engine.project_batch / Engine.track_batch: the host logic of gpsat_amd.prep and
    DataPrep.assign_tracks runs on it in the CPU tests."""

    def project_batch(self, in0, in1, direction="forward", lon_0=0.0, lat_0=90.0):
        fn = laea_forward if direction == "forward" else laea_inverse
        return fn(in0, in1, lon_0, lat_0)

    def track_batch(self, cols, group=None, cut_off=0.0, start_track=0, mode="cut"):
        cols = np.stack([np.asarray(c, dtype=np.float64) for c in cols], axis=1)
        if mode == "cut":
            order, delta, track = tracks_by_group(cols, group, cut_off, start_track)
            return delta, track.astype(np.int32), order.astype(np.int32)
        n = cols.shape[0]
        codes = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group)
        order, delta, out = [], [], []
        for g in sorted(set(int(c) for c in codes if c >= 0)):
            rows = np.flatnonzero(codes == g)
            order.append(rows), delta.append(cols[rows, 0])
            if mode == "runs":
                out.append(track_num_for_date(cols[rows, 0]))
            else:
                out.append(guess_track_num(cols[rows, 0], cut_off, start_track))
                start_track = int(out[-1].max()) + 1
        rest = np.flatnonzero(codes < 0)
        order.append(rest), delta.append(np.full(len(rest), np.nan)), out.append(np.full(len(rest), -1.0))
        return (None if mode == "runs" else np.concatenate(delta), np.concatenate(out).astype(np.int32),
                np.concatenate(order).astype(np.int32))
