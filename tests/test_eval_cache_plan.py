"""The device memory of the evaluation memo (KernelArgs::memo) is sized by gpsat::eval_cache_bytes, a pure function next to
gpsat::plan_tiles in gpsat_plan.h, and gpsat_capi.cpp reserves what it says: no GPU needed."""
import ctypes as C
import os
import re

from gpsat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsat_amd", "csrc")


def _fn():
    fn = getattr(L.load(), "_ZN5gpsat16eval_cache_bytesEiiiiii")
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * 6
    return fn


def _memo_words():
    """MEMO_WORDS as gpsat_kernels.h states it: a header, then MEMO_K entries of 6 key floats, an fp64 objective and 6 fp64 sums"""
    src = open(os.path.join(CSRC, "gpsat_kernels.h")).read()
    m = re.search(r"constexpr int MEMO_K = (\d+), MEMO_HDR = (\d+), MEMO_ENTRY = 6 \+ 2 \+ 12;", src)
    assert m and "constexpr int MEMO_WORDS = MEMO_HDR + MEMO_K * MEMO_ENTRY;" in src
    k, hdr = int(m.group(1)), int(m.group(2))
    assert k == 4 and hdr >= 6
    return hdr + k * 20


def test_eval_cache_bytes():
    fn, words = _fn(), _memo_words()
    lbfgs, adam, none = L.OPT_LBFGS, L.OPT_ADAM, L.OPT_NONE
    # (T, f64, optimiser, max_iter, multistart, switched off)
    assert fn(4096, 0, lbfgs, 20, 0, 0) == 4096 * words * 4          # the headline batch: 1.4 MB
    assert fn(1, 0, lbfgs, 1, 0, 0) == words * 4
    assert fn(100_000, 0, lbfgs, 20, 0, 0) == 100_000 * words * 4
    for args in [(4096, 1, lbfgs, 20, 0, 0),       # fp64: the key would be the fp64 theta
                 (4096, 0, adam, 20, 0, 0), (4096, 0, none, 20, 0, 0), (4096, 0, lbfgs, 0, 0, 0),
                 (4096, 0, lbfgs, 20, 1, 0),       # multi-start L-BFGS-B
                 (4096, 0, lbfgs, 20, 0, 1),       # GPSAT_DEBUG_EVAL_CACHE=0
                 (0, 0, lbfgs, 20, 0, 0)]:
        assert fn(*args) == 0, args


def test_the_reservation_is_the_function_s():
    src = open(os.path.join(CSRC, "gpsat_capi.cpp")).read()
    body = src[src.index("int setup_eval_cache("):]
    body = body[:body.index("\n}\n")]
    assert "gpsat::eval_cache_bytes(b->T, f64, b->optimiser, b->max_iter, ms_on," in body
    assert "h->memo.reserve(64 + bytes)" in body and "MEMO_WORDS" not in body
    assert src.count("setup_eval_cache(") == 2      # defined once, called by run_tiles
