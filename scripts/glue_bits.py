"""The bits of the keyed glues: one SHA-256 per output array of a fixed, seeded set of small calls, to compare two builds
of the library (run it on each and diff the listings; GPSAT_LIB picks the library).

glue_keyed_batch, glue_keyed_grad_batch and glue_keyed_hess_batch share one walk: a team of W lanes per key gathers the
key's rows through the sort's permutation, lane l adds rows l, l + W, ..., a xor tree joins the lanes.  The rows are the
smallest set that reaches every path of it, not a workload's:
  groups of 1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65 and 130 rows, three of each: below, at and above every team width and more
      than two strides of the widest; with the two groups below 38 keys, no multiple of 256 / W for any W, so that a
      workgroup has teams past the last group;
  the rows of all groups scattered by a seeded permutation, 25 rows with a negative key among them;
  a group with a row exactly at the limit (differences 3000 and 4000, max_dist 5000: exact in fp64, and the limit is strict)
      and one at 5000 and 0, and a group whose every row lies outside (count 0, NaN outputs);
  NaN in the value alone, in one gradient component alone, in one second derivative alone, each in a row of a group of its
      own, and a group whose every value is NaN;
every team width 1, 4, 8, 16, 32, 64 (GPSAT_DEBUG_GLUE_TEAM in developer mode) for each entry point, ndim 1 and 2, a scalar
sigma and sigma per row, no limit and max_dist 5000, and for glue_keyed_batch 1 to 4 columns.  Then the returns without a
launch: no row, and every key negative.

The NaN rule, asserted for every output so that two builds cannot agree on poisoned arrays: a record is NaN exactly where
its count is 0.  A NaN among the inputs never reaches an output -- a row whose value, gradient component or second derivative
is NaN stays out of the sums that would read it while its weight stays in the denominator, so a group whose every value is
NaN glues to 0.

    python scripts/glue_bits.py > listing.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["GPSAT_DEVELOPER"] = "1"             # GPSAT_DEBUG_GLUE_TEAM below is read in developer mode only

from gpsat_amd.engine import Engine             # noqa: E402

SIZES = (1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 130)
WIDTHS = (1, 4, 8, 16, 32, 64)
MAX_DIST = 5000.0


def rows():
    """key [R], pred and xprt [2, R], val [R], grad [2, R], hess [3, R], sigma_rows [R] and the keys of the limit group and
    of the group outside the limit."""
    rng = np.random.default_rng(20)
    sizes = [s for s in SIZES for _ in range(3)] + [4, 3]
    keys = 5 + 3 * rng.permutation(len(sizes))                 # distinct, not contiguous, in no order
    at_limit, outside = int(keys[-2]), int(keys[-1])
    key = np.concatenate([np.repeat(keys, sizes), rng.choice([-1, -7], 25)]).astype(np.int64)
    R = len(key)
    xprt = 3.0e6 + np.round(rng.uniform(-2.0e5, 2.0e5, (2, R)))  # whole metres: the differences below are exact
    diff = np.round(rng.uniform(-6000.0, 6000.0, (2, R)))
    first = np.concatenate([[0], np.cumsum(sizes)])
    a = first[-3]
    diff[:, a:a + 4] = [[3000.0, 5000.0, 1000.0, -2000.0], [4000.0, 0.0, -1500.0, 500.0]]
    b = first[-2]
    diff[:, b:b + 3] = [[7000.0, -6500.0, 6000.0], [0.0, 2500.0, -5000.0]]
    pred = xprt + diff
    val, grad, hess = rng.normal(0.0, 1.0, R), rng.normal(0.0, 1e-3, (2, R)), rng.normal(0.0, 1e-6, (3, R))
    g7, g8, g9, g3, g130 = (first[sizes.index(s)] for s in (7, 8, 9, 3, 130))
    val[g7 + 2] = np.nan                                         # the value alone
    grad[0, g8 + 5] = np.nan                                     # one gradient component alone
    grad[1, g130 + 77] = np.nan
    hess[0, g9 + 1] = np.nan                                     # one second derivative alone
    hess[2, g9 + 6] = np.nan
    val[g3:g3 + 3] = np.nan                                      # every value of a group
    sigma_rows = rng.uniform(2000.0, 3000.0, R)
    order = rng.permutation(R)
    pick = lambda x: np.ascontiguousarray(x[..., order])
    return tuple(pick(x) for x in (key, pred, xprt, val, grad, hess, sigma_rows)) + (at_limit, outside)


def listing(name, counts, outs):
    for label, v in outs.items():
        v = np.asarray(v)
        if v.dtype == np.float64:
            assert (np.isnan(v) == (counts == 0)).all(), f"{name}.{label}: NaN where the count is not 0, or a number where it is"
        print(f"{name}.{label} {v.dtype}{list(v.shape)} {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()}")


def calls(eng, key, pred, xprt, val, grad, hess, sigma, md):
    """(name, result as a dict) of each entry point on these rows; ndim is pred's"""
    nd = pred.shape[0]
    cols = np.stack([val, grad[0], hess[0], grad[1]])           # every column holds a NaN somewhere
    for nv in (1, 2, 3, 4):
        k, c, out = eng.glue_keyed_batch(key, pred, xprt, cols[:nv], sigma, md)
        yield f"o0.nv{nv}", dict(keys=k, counts=c, out=out)
    k, c, v, g = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad[:nd], sigma, md)
    yield "o1", dict(keys=k, counts=c, out_val=v, out_grad=g)
    k, c, v, g, h = eng.glue_keyed_hess_batch(key, pred, xprt, val, grad[:nd], hess[:nd * (nd + 1) // 2], sigma, md)
    yield "o2", dict(keys=k, counts=c, out_val=v, out_grad=g, out_hess=h)


def main():
    eng = Engine(0)
    key, pred, xprt, val, grad, hess, sigma_rows, at_limit, outside = rows()
    want_keys = np.unique(key[key >= 0])
    try:
        for w in WIDTHS:
            os.environ["GPSAT_DEBUG_GLUE_TEAM"] = str(w)
            for nd in (1, 2):
                for sn, sigma in (("scalar", 2500.0), ("rows", sigma_rows)):
                    for ln, md in (("nolimit", None), ("limit", MAX_DIST)):
                        for cn, r in calls(eng, key, pred[:nd], xprt[:nd], val, grad, hess, sigma, md):
                            name = f"W{w}.nd{nd}.{sn}.{ln}.{cn}"
                            assert np.array_equal(r["keys"], want_keys), name
                            c = dict(zip(r["keys"].tolist(), r["counts"].tolist()))
                            # strict: 3000, 4000 is at 5000 in two dimensions and inside in one; 5000, 0 is outside in both
                            assert (c[at_limit], c[outside]) == ((4, 3) if md is None else (3 if nd == 1 else 2, 0)), (name, c[at_limit], c[outside])
                            listing(name, r["counts"], r)
        # returns without a launch, at the product's width
        os.environ.pop("GPSAT_DEBUG_GLUE_TEAM", None)
        none = key[:0], pred[:, :0], xprt[:, :0], val[:0], grad[:, :0], hess[:, :0]
        for cn, r in calls(eng, *none, 2500.0, None):
            listing(f"R0.{cn}", r["counts"], r)
        for cn, r in calls(eng, np.full_like(key, -3), pred, xprt, val, grad, hess, sigma_rows, MAX_DIST):
            assert len(r["keys"]) == 0, cn
            listing(f"negative.{cn}", r["counts"], r)
    finally:
        os.environ.pop("GPSAT_DEBUG_GLUE_TEAM", None)
        eng.close()


if __name__ == "__main__":
    main()
