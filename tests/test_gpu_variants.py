"""GPU: the contract every variant of the exact fp64 expert is held to -- RationalQuadratic (GPSAT_KERNEL_RQ), the constant mean
(gpsat_fit_predict_batch_mean) and known noise variances (gpsat_fit_predict_batch_noise) -- against the fp64 restatement
tests/variant_numpy.py, parametrised over the cases of tests/variant_cases.py, which also states the bounds (check_tile).
The fixed-parameter and full-covariance tests keep their names and cases in tests/test_gpu_rq.py, tests/test_gpu_mean.py and
tests/test_gpu_noise.py, beside what only one variant has; their bodies are variant_cases.check_fixed_parameters and
check_full_cov.
"""
import numpy as np
import pytest

from variant_cases import CASES, FIELDS, check_tile, eng, one, ragged_inputs, run, same  # noqa: F401 (eng: the fixture)

pytestmark = pytest.mark.gpu


# ---- 1. a large tile beside a small one
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_large_tile_takes_the_eight_wave_build(eng, case):
    """A tile whose LDS does not fit twice into a CU runs on the 8-wave build (gpsat_plan.h), next to a small one."""
    b = case.batch(2, [1200, 90], [24, 9], 3, "Matern32", 7300)
    th = case.theta(np.random.default_rng(12), 2, 3, case.x_large)
    r = run(case, eng, b, th)
    for t in range(2):
        check_tile(case, r, b, t, th[t], "8-wave build by LDS")


# ---- 2. a ragged, unsorted batch
@pytest.fixture(scope="module", params=CASES, ids=repr)
def ragged(request, eng):
    """Per variant: its case, the ragged batch, theta0, the result."""
    b, th = ragged_inputs(request.param)
    return request.param, b, th, run(request.param, eng, b, th)


def test_ragged_batch(ragged):
    case, b, th, r = ragged
    case.check_ragged(b, r)
    for t in range(case.ragged_T):
        check_tile(case, r, b, t, th[t], "ragged")


# ---- 3. the same bits alone, inside the batch, on a second call and with the time-sliced queue
def test_same_bits_alone_in_the_batch_and_again(eng, ragged):
    case, b, th, r = ragged
    same(run(case, eng, b, th), r, "second call")
    for t in case.alone:
        r1 = run(case, eng, one(b, t), th[[t]])
        pa, pe = b["pred_off"][t], b["pred_off"][t + 1]
        for name in FIELDS:
            whole = getattr(r, name)
            part = whole[pa:pe] if name in ("f_mean", "f_var", "y_var") else whole[[t]]
            assert np.asarray(getattr(r1, name)).tobytes() == np.asarray(part).tobytes(), (t, name)


def test_time_sliced_optimisation_is_bit_identical(eng, ragged, monkeypatch):
    """As tests/test_gpu_parity.py::test_time_sliced_optimisation_is_bit_identical forces the queue: suspended after every
    evaluation, after every third of a 200-point tile, or never.  The optimiser state of a resumed tile travels intact, its
    extra parameter included: a residual formed from the c, or a diagonal from the v, of the tile the workgroup ran in between
    would change the bits.  One tile of the batch run alone returns the bits it has inside it."""
    case, b, th, _ = ragged
    T, D = case.ragged_T, b["D"]
    lo, hi = case.bounds(T, D)
    th0 = case.start(th)
    kw = dict(lo=lo, hi=hi, optimiser="lbfgs", max_iter=12)
    monkeypatch.setenv("GPSAT_DEVELOPER", "1")
    monkeypatch.setenv("GPSAT_DEBUG_SEG", "0")
    r0 = run(case, eng, b, th0, **kw)
    assert r0.n_eval.max() > 6
    case.check_sliced(r0, th0, D)
    for seg in ("1", str(3 * 14 ** 3)):
        monkeypatch.setenv("GPSAT_DEBUG_SEG", seg)
        same(run(case, eng, b, th0, **kw), r0, f"slice {seg}")
    monkeypatch.delenv("GPSAT_DEBUG_SEG")
    t = 17
    r1 = run(case, eng, one(b, t), th0[[t]], lo=lo[[t]], hi=hi[[t]], optimiser="lbfgs", max_iter=12)
    assert r1.theta.tobytes() == r0.theta[[t]].tobytes() and r1.nll.tobytes() == r0.nll[[t]].tobytes()
    assert r1.f_mean.tobytes() == r0.f_mean[b["pred_off"][t]:b["pred_off"][t + 1]].tobytes()
    case.after_sliced(eng, b, th0, kw, r0)
