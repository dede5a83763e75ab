"""The inputs of the keyed-glue pins (tests/golden/key_runs_pins.npz): deterministic rows for gpsat_glue_keyed_batch and
gpsat_glue_keyed_grad_batch at the sizes and key patterns at which the shared sort-and-run-heads stage can go wrong.
tests/golden/make_key_runs_pins.py stores the outputs of these cases; tests/test_gpu_key_runs.py compares with them."""
import zlib

import numpy as np

SIZES = [1, 63, 64, 65, 255, 256, 257]        # either side of a wave and of a block of 256 rows
# mixed: several groups, every key >= 0 (no sentinel run); neg: the same with rows of negative key (the sentinel run is
# there); allneg: every key negative (the call returns G = 0 before the device is asked); one: one group; each: one row per
# group; key0: the largest key is 0 (sentinel 1, the sort runs over one bit); big: the largest key is 2^62 (63 bits sorted)
KINDS = ["mixed", "neg", "allneg", "one", "each", "key0", "big"]
CASES = [(kind, R) for kind in KINDS for R in SIZES]
SIGMA = 1.75


def name(kind, R):
    return f"{kind}_{R}"


def keys_of(kind, R, rng):
    n_groups = max(1, R // 8)
    if kind in ("mixed", "neg", "allneg", "big"):
        key = rng.integers(0, n_groups, R).astype(np.int64) * 3 + 1
        if kind == "big":
            key = np.where(key == key.max(), 2 ** 62, key * (2 ** 40 + 7))
        if kind == "neg" and R > 1:
            key[rng.random(R) < 0.25] = -1
            key[R // 2] = -7                  # at least one ignored row, and at least one kept
            key[0] = 1
        if kind == "allneg":
            key = -1 - key
    elif kind == "one":
        key = np.full(R, 5, dtype=np.int64)
    elif kind == "each":
        key = rng.permutation(R).astype(np.int64) * 2
    else:                                     # key0
        key = np.zeros(R, dtype=np.int64)
        if R > 1:
            key[rng.random(R) < 0.3] = -1
            key[R - 1] = -3
            key[0] = 0
    return key


def case(kind, R):
    """key [R], pred and xprt [ndim, R], val [R], grad [ndim, R], sigma (per row at odd R).  One axis for `each`, two otherwise."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + R)
    ndim = 1 if kind == "each" else 2
    key = keys_of(kind, R, rng)
    centre = rng.uniform(0.0, 100.0, (ndim, 2 ** 10))
    pred = centre[:, np.abs(key) % 2 ** 10]                 # rows of a key share their prediction location
    xprt = pred + rng.uniform(-4.0, 4.0, (ndim, R))
    val = rng.normal(3.0, 1.0, R)
    grad = rng.normal(0.0, 1.0, (ndim, R))
    if R > 8:
        val[3] = np.nan
        grad[0, 5] = np.nan
    sigma = rng.uniform(1.0, 3.0, R) if R % 2 else SIGMA
    return key, np.ascontiguousarray(pred), xprt, val, grad, sigma


FIELDS = ["out_key", "out_count", "out", "val_key", "val_count", "out_val", "out_grad"]      # per group; crc and G per case


def outputs(eng, kind, R):
    """What the two entry points return for one case, by field."""
    key, pred, xprt, val, grad, sigma = a = case(kind, R)
    keys, counts, out = eng.glue_keyed_batch(key, pred, xprt, val[None], sigma)
    vkeys, vcounts, out_val, out_grad = eng.glue_keyed_grad_batch(key, pred, xprt, val, grad, sigma)
    return {"crc": np.uint32(checksum(a)), "G": np.int64(len(keys)), "out_key": keys, "out_count": counts, "out": out,
            "val_key": vkeys, "val_count": vcounts, "out_val": out_val, "out_grad": out_grad}


def pack(records):
    """The records of CASES, in that order, as one array per field."""
    pins = {k: np.array([r[k] for r in records]) for k in ("crc", "G")}
    pins.update({k: np.concatenate([np.asarray(r[k]).reshape(-1) for r in records]) for k in FIELDS})
    return pins


def unpack(pins):
    """{(kind, R): record} of a packed file; out is [1, G] and out_grad [ndim, G] again."""
    at, recs = dict.fromkeys(FIELDS, 0), {}
    for (kind, R), crc, G in zip(CASES, pins["crc"], pins["G"]):
        G, ndim = int(G), 1 if kind == "each" else 2
        r = {"crc": crc, "G": G}
        for k in FIELDS:
            n = G * (ndim if k == "out_grad" else 1)
            r[k] = pins[k][at[k]: at[k] + n]
            at[k] += n
        r["out"], r["out_grad"] = r["out"].reshape(1, G), r["out_grad"].reshape(ndim, G)
        recs[(kind, R)] = r
    assert all(at[k] == len(pins[k]) for k in FIELDS)
    return recs


def checksum(args):
    """One number for the bytes of a case's inputs: the pins hold it, so that a changed generator is told from a changed library."""
    crc = 0
    for a in args:
        crc = zlib.crc32(np.ascontiguousarray(a, dtype=None if isinstance(a, np.ndarray) else np.float64).tobytes(), crc)
    return crc
