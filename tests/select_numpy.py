"""Tile selection restated in plain NumPy fp64: what gpsat_select_batch_ex (gpsat_amd/csrc/gpsat_select.hip) must return.

One expert at a time, vectorised over the rows, no KD-tree, no boxes, no chunks, no binning:
  ("cmp", col, comp, val)    x[col] <comp> (ref[col] + val)
  ("ball", cols, comp, r)    s = 0.0; for each column in order: d = x - c; s = s + d*d;  s <= r*r  (s < r*r when comp is "<")
  ("interval", col, j)       bounds[e, j, 0] <= x[col] < bounds[e, j, 1]
d*d and the addition are separate NumPy operations (nothing fuses), and everything runs under np.errstate(all="ignore"), so
NaN and inf follow the IEEE comparisons: a NaN never compares true.  The criteria are ANDed in their order; once fewer than a
quarter of the rows are left the next predicates are evaluated on those rows alone, which changes no boolean.  The result is the CSR pair (off [T+1] int64, idx int32)
of Engine.select_batch: every expert's row positions ascending.

`Restatement` keeps each predicate in a method of its own, so that tests/test_select_cases_cpu.py can derive deliberately
wrong variants from it; `select` is the function the tests compare the device with."""
import numpy as np

COMPS = {">=": np.greater_equal, ">": np.greater, "==": np.equal, "<": np.less, "<=": np.less_equal}


class Restatement:
    def cmp(self, x, ref, comp, val):
        return COMPS[comp](x, ref + val)

    def ball_sum(self, xs, cs):
        """xs: the criterion's columns, cs: the expert's values in them, same order."""
        s = np.zeros(len(xs[0]) if len(xs) else 0)
        for x, c in zip(xs, cs):
            d = x - c
            dd = d * d
            s = s + dd
        return s

    def ball(self, xs, cs, comp, r):
        s = self.ball_sum(xs, cs)
        r2 = np.float64(r) * np.float64(r)
        return (s < r2) if comp == "<" else (s <= r2)

    def interval(self, x, lo, hi):
        return (lo <= x) & (x < hi)

    def rows(self, cols, ref, criteria, bounds_e=None):
        """Ascending row positions of one expert.  cols: the table's columns, each contiguous; ref [C]; bounds_e [n_bounds, 2].
        The criteria are ANDed in their order; once few rows are left, the next predicates are evaluated on those rows alone
        (the same operations on the same values, so the same booleans -- it only spares work on tables of millions of rows)."""
        M = len(cols[0])
        rows, m = None, None                      # the rows still in play (None: all), and which of them passed so far
        with np.errstate(all="ignore"):
            for crit in criteria:
                col = (lambda c: cols[c]) if rows is None else (lambda c: cols[c][rows])
                if crit[0] == "cmp":
                    _, c, comp, val = crit
                    ok = self.cmp(col(c), ref[c], comp, np.float64(val))
                elif crit[0] == "ball":
                    _, cs, comp, r = crit
                    ok = self.ball([col(c) for c in cs], [ref[c] for c in cs], comp, r)
                elif crit[0] == "interval":
                    _, c, j = crit
                    ok = self.interval(col(c), bounds_e[j, 0], bounds_e[j, 1])
                else:
                    raise ValueError(f"unknown criterion {crit[0]!r}")
                m = ok if m is None else (m & ok)
                if 4 * np.count_nonzero(m) < len(m):
                    rows = np.nonzero(m)[0] if rows is None else rows[m]
                    m = None
        if m is not None:
            rows = np.nonzero(m)[0] if rows is None else rows[m]
        return np.arange(M) if rows is None else rows

    def select(self, points, refs, criteria, bounds=None, points_cm=None):
        """points [M, C] (or points_cm [C, M]), refs [T, C], bounds [T, n_bounds, 2]."""
        cols = np.ascontiguousarray(np.asarray(points, dtype=np.float64).T if points_cm is None else points_cm, dtype=np.float64)
        refs = np.asarray(refs, dtype=np.float64)
        return to_csr([self.rows(cols, refs[e], criteria, None if bounds is None else bounds[e]) for e in range(refs.shape[0])])


def to_csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    for e, ids in enumerate(lists):
        off[e + 1] = off[e] + len(ids)
    idx = np.concatenate(lists).astype(np.int32) if len(lists) else np.zeros(0, np.int32)
    return off, idx.astype(np.int32)


def from_csr(off, idx):
    return [np.asarray(idx[off[e]:off[e + 1]]) for e in range(len(off) - 1)]


def select(points, refs, criteria, bounds=None, points_cm=None):
    """(off, idx) as Engine.select_batch(points, refs, criteria, bounds=bounds) returns them."""
    return Restatement().select(points, refs, criteria, bounds, points_cm)


def select_frames(df, local_select, refs, strict_ball=False, interval_codes=None, bounds=None):
    """The restatement over frames, as DeviceSelector(df, local_select, engine, strict_ball, interval_codes).select(refs, bounds)
    is called: local_select entries of the reference's form, one interval criterion per row of interval_codes."""
    names = []
    for ls in local_select:
        for c in ([ls["col"]] if isinstance(ls["col"], str) else ls["col"]):
            if c not in names:
                names.append(c)
    criteria = []
    for ls in local_select:
        if isinstance(ls["col"], str):
            criteria.append(("cmp", names.index(ls["col"]), ls["comp"], ls["val"]))
        else:
            criteria.append(("ball", [names.index(c) for c in ls["col"]], "<" if strict_ball else "<=", ls["val"]))
    cols = [df[c].to_numpy(dtype=np.float64) for c in names]
    r = refs.loc[:, names].to_numpy(dtype=np.float64)
    for j, code in enumerate([] if interval_codes is None else interval_codes):
        criteria.append(("interval", len(cols), j))
        cols.append(np.asarray(code, dtype=np.float64))
        r = np.concatenate([r, np.zeros((len(r), 1))], axis=1)
    return select(None, r, criteria, bounds=bounds, points_cm=np.array(cols))
