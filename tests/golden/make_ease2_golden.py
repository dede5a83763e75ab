"""Writes tests/golden/kat_ease2.npz: known answers of the polar Lambert azimuthal equal-area projection on the WGS84 ellipsoid
from mpmath at 50 digits and 10 guard digits (Snyder 3-12, 24-23, 24-25; the inverse by Newton's iteration at that precision until the step is
below 1e-45).  Run from the repository root:  python tests/golden/make_ease2_golden.py

Forward: (lon, lat, lon_0, lat_0) -> x, y, each rounded once to fp64.  Inverse: its INPUT is that rounded (x, y) -- a point in
its own right -- and inv_lon, inv_lat are its exact coordinates, rounded once; inv_ok is false where the point lies within
1e-9 of the disc's edge (the opposite pole), where the inverse may call it outside."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60          # 50, and 10 to spare: next to the pole the inverse's Newton step carries the rounding divided by cos(phi)
A = mp.mpf(6378137)
F = 1 / mp.mpf("298.257223563")
E2 = F * (2 - F)
E = mp.sqrt(E2)


def q_of(phi):
    s = mp.sin(phi)
    return (1 - E2) * (s / (1 - E2 * s * s) - mp.log((1 - E * s) / (1 + E * s)) / (2 * E))


QP = q_of(mp.pi / 2)


def forward(lon, lat, lon_0, south):
    q = q_of(mp.radians(mp.mpf(lat)))
    rho = A * mp.sqrt(max(QP + q if south else QP - q, 0))       # at the pole: 0, not the 1e-100 of pi's last digit
    dl = mp.radians(mp.mpf(lon) - mp.mpf(lon_0))
    return rho * mp.sin(dl), (rho * mp.cos(dl) if south else -rho * mp.cos(dl))


def inverse(x, y, lon_0, south):
    x, y = mp.mpf(x), mp.mpf(y)
    r2 = (x * x + y * y) / (A * A)
    if r2 == 0:
        return mp.mpf(lon_0), mp.mpf(-90 if south else 90)
    q = -(QP - r2) if south else QP - r2
    phi = mp.asin(q / QP)
    for _ in range(200):
        s, c = mp.sin(phi), mp.cos(phi)
        w = 1 - E2 * s * s
        step = w * w / (2 * c) * (q / (1 - E2) - s / w + mp.log((1 - E * s) / (1 + E * s)) / (2 * E))
        phi += step
        if abs(step) < mp.mpf(10) ** -45:
            break
    else:
        raise RuntimeError("Newton's iteration did not settle")
    lon = mp.mpf(lon_0) + mp.degrees(mp.atan2(x, y if south else -y))
    lon -= 360 * mp.ceil((lon - 180) / 360)
    return lon, mp.degrees(phi)


def points():
    rng = np.random.default_rng(20261020)
    lats = [90.0, 89.9999999, 89.9999, 89.99, 89.0, 85.0, 75.0, 60.0, 45.0, 30.0, 10.0, 1e-7, 0.0, -1e-7, -10.0, -30.0, -60.0, -89.0,
            -89.9999999, -90.0]
    lons = [-180.0, -179.9999999, -105.01621, -90.0, -1e-9, 0.0, 37.5, 90.0, 153.434948822922, 180.0]
    rows = []
    for lat_0 in (90.0, -90.0):
        for k, lat in enumerate(lats):
            for lon in (lons[k % len(lons)], lons[(3 * k + 1) % len(lons)], lons[(7 * k + 2) % len(lons)]):
                rows.append((lon, lat, (0.0, -45.0, 100.0)[k % 3], lat_0))
        for _ in range(90):
            lat = float(np.degrees(np.arcsin(rng.uniform(-1.0, 1.0))))
            rows.append((float(rng.uniform(-180.0, 180.0)), lat, float(rng.choice([0.0, -45.0, 100.0])), lat_0))
    return rows


def main():
    rows = points()
    cols = {k: [] for k in ("lon", "lat", "lon_0", "lat_0", "x", "y", "inv_lon", "inv_lat", "inv_ok")}
    for lon, lat, lon_0, lat_0 in rows:
        south = lat_0 < 0
        x, y = forward(lon, lat, lon_0, south)
        xf, yf = float(x), float(y)
        r2 = (mp.mpf(xf) ** 2 + mp.mpf(yf) ** 2) / (A * A)
        ok = bool(r2 < 2 * QP * (1 - mp.mpf(10) ** -9))
        il, ip = inverse(xf, yf, lon_0, south) if ok else (mp.nan, mp.nan)
        for k, v in zip(cols, (lon, lat, lon_0, lat_0, xf, yf, float(il), float(ip), ok)):
            cols[k].append(v)
    out = {k: np.array(v, dtype=bool if k == "inv_ok" else np.float64) for k, v in cols.items()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_ease2.npz")
    np.savez(path, **out)
    print(f"{path}: {len(rows)} points, {int(out['inv_ok'].sum())} with an inverse")


if __name__ == "__main__":
    main()
