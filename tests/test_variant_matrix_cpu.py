"""Every pairing of the expert variants and call extensions, at every host layer that can express it.

The nine kinds (RationalQuadratic, constant mean, per-observation noise, held-out predictions, refitted cross-validation,
multi-start, sparse, replacement profile, full covariance) are driven alone, in every unordered pair, in fp32 and with four
input dimensions through Engine (no handle: a recording stand-in for the library), the per-tile models (an engine that only
records) and BatchedLocalExpertOI (construction).  EXPECTED is the outcome of this enumeration at the commit before
gpsat_amd/variants.py existed (`python tests/test_variant_matrix_cpu.py` prints it): "lib" / "engine" / "built" where the layer
goes on to the library call / the engine call / a constructed orchestrator, else the exception type.  A refactor of the host
layer has to reproduce it; the table of gpsat_amd/variants.py has to agree with it.
"""
import itertools

import numpy as np
import pandas as pd
import pytest

from gpsat_amd import _lib as L
from gpsat_amd.engine import Engine
from gpsat_amd.local_experts import BatchedLocalExpertOI
from gpsat_amd.models import HipGPRModel, HipSGPRModel, HipSklearnGPRModel

ROWS = ["rq", "mean", "noise", "cv", "cv_refit", "multistart", "sgpr", "replacement", "full_cov"]
CASES = [(r,) for r in ROWS] + list(itertools.combinations(ROWS, 2)) + [(r, "f32") for r in ROWS] + [(r, "D4") for r in ROWS]
N = 10
# What a layer has no way to say.  Engine: the sparse call is a function of its own without these arguments, and a
# replacement profile is the orchestrator's; cv_refit is cv_fold with one more argument, so "both" is cv_refit.
# Models: a model class is exact, sparse or sklearn; there is no replacement; cross_validate takes no full_cov.
INEXPRESSIBLE = {
    "engine": {("replacement",), ("cv", "cv_refit"), ("replacement", "f32"), ("replacement", "D4")}
    | {tuple(sorted((a, "replacement"), key=ROWS.index)) for a in ROWS if a != "replacement"}
    | {tuple(sorted((a, "sgpr"), key=ROWS.index)) for a in ("mean", "cv", "cv_refit", "multistart")},
    "model": {("replacement",), ("cv", "cv_refit"), ("multistart", "sgpr"), ("cv", "full_cov"), ("cv_refit", "full_cov"),
              ("replacement", "f32"), ("replacement", "D4")}
    | {tuple(sorted((a, "replacement"), key=ROWS.index)) for a in ROWS if a != "replacement"},
    "orchestrator": {("cv", "cv_refit"), ("multistart", "sgpr")},
}


class _Reached(Exception):
    pass


class _RecordingLib:
    """Stands where the shared library would: every symbol exists, and calling one ends the case."""

    def __getattr__(self, name):
        def call(*a):
            raise _Reached(name)
        return call


class _RecordingEngine:
    device_name, device_id = "no device (host logic only)", 0

    def fit_predict_batch(self, **kw):
        raise _Reached("fit_predict_batch")

    sgpr_fit_predict_batch = fit_predict_batch


def _tile(D):
    rng = np.random.default_rng(D)
    return rng.uniform(0.0, 4.0, (N, D)), rng.standard_normal(N), rng.uniform(0.0, 0.1, N)


def _engine(case):
    D, on = 4 if "D4" in case else 2, set(case)
    X, y, v = _tile(D)
    eng = object.__new__(Engine)
    eng._lib, eng._h = _RecordingLib(), None
    kw = dict(D=D, obs_off=[0, N], X=X, y=y, pred_off=[0, 3], Xs=X[:3], optimiser="none", dtype="f32" if "f32" in on else "f64",
              theta0=np.ones(D + 2 + len(on & {"rq", "mean"})))
    if "sgpr" in on:                                        # the sparse call lays out D + 2 parameters whatever the kernel
        kw.update(z_off=[0, 4], Z=X[:4], theta0=np.ones(D + 2))
    kw.update({"kernel": "RationalQuadratic"} if "rq" in on else {})
    kw.update({"mean": "constant"} if "mean" in on else {})
    kw.update({"obs_var": v} if "noise" in on else {})
    kw.update({"cv_fold": "loo"} if "cv" in on else {})
    kw.update({"cv_fold": np.arange(N, dtype=np.int32) % 3, "cv_refit": True} if "cv_refit" in on else {})
    kw.update({"n_starts": 2} if "multistart" in on else {})
    kw.update({"full_cov": True} if "full_cov" in on else {})
    (eng.sgpr_fit_predict_batch if "sgpr" in on else eng.fit_predict_batch)(**kw)


def _model(case):
    D, on = 4 if "D4" in case else 2, set(case)
    X, y, v = _tile(D)
    cls = HipSklearnGPRModel if "multistart" in on else HipSGPRModel if "sgpr" in on else HipGPRModel
    kw = dict(coords=X, obs=y, engine=_RecordingEngine(), dtype="f32" if "f32" in on else "f64")
    kw.update({"kernel": "RationalQuadratic"} if "rq" in on else {})
    kw.update({"mean_function": "Constant"} if "mean" in on else {})
    kw.update({"obs_var": v} if "noise" in on else {})
    kw.update({"num_inducing_points": 4} if "sgpr" in on else {})
    m = cls(**kw)
    if "cv" in on or "cv_refit" in on:
        m.cross_validate(refit="cv_refit" in on)
    elif "full_cov" in on:
        m.predict(X[:3], full_cov=True)
    else:
        m.get_objective_function_value()


def _orchestrator(case):
    D, on = 4 if "D4" in case else 2, set(case)
    X, y, v = _tile(D)
    cc = [f"x{k}" for k in range(D)]
    df = pd.DataFrame({**{c: X[:, k] for k, c in enumerate(cc)}, "y": y, "var": v, "g": np.arange(N) % 3})
    init = {**({"kernel": "RationalQuadratic"} if "rq" in on else {}), **({"mean_function": "Constant"} if "mean" in on else {}),
            **({"num_inducing_points": 4} if "sgpr" in on else {})}
    model = {"oi_model": "sklearnGPRModel" if "multistart" in on else "HipSGPRModel" if "sgpr" in on else "HipGPRModel",
             "init_params": init, **({"replacement_threshold": 5} if "replacement" in on else {}),
             **({"pred_kwargs": {"full_cov": True}} if "full_cov" in on else {})}
    data = {"data_source": df, "obs_col": "y", "coords_col": cc, "local_select": [],
            **({"obs_var_col": "var"} if "noise" in on else {})}
    cv = {"by": ["g"], "refit": True} if "cv_refit" in on else "loo" if "cv" in on else None
    BatchedLocalExpertOI({"source": df[cc].iloc[:1]}, data, model, {"method": "expert_loc"}, engine=_RecordingEngine(),
                         dtype="f32" if "f32" in on else "f64", cv=cv)
    raise _Reached("built")


LAYERS = {"engine": (_engine, "lib"), "model": (_model, "engine"), "orchestrator": (_orchestrator, "built")}


def outcome(layer, case):
    run, went_on = LAYERS[layer]
    try:
        run(case)
    except _Reached:
        return went_on
    except Exception as e:                                   # the refusal's type is the result
        return type(e).__name__
    raise AssertionError(f"{layer} {case}: the stand-ins did not end the case")


def enumerate_all():
    return {layer: {c: outcome(layer, c) for c in CASES if c not in INEXPRESSIBLE[layer]} for layer in LAYERS}


EXPECTED = {}   # filled below by the literal matrix


def _matrix(layer, text):
    """'case outcome' lines -> EXPECTED[layer]."""
    EXPECTED[layer] = {}
    for line in text.strip().splitlines():
        *case, res = line.split()
        EXPECTED[layer][tuple(case)] = res


_matrix("engine", """
rq lib
mean lib
noise lib
cv lib
cv_refit lib
multistart lib
sgpr lib
full_cov lib
rq mean GpsatError
rq noise GpsatError
rq cv lib
rq cv_refit lib
rq multistart lib
rq sgpr lib
rq full_cov lib
mean noise GpsatError
mean cv GpsatError
mean cv_refit GpsatError
mean multistart GpsatError
mean full_cov lib
noise cv GpsatError
noise cv_refit GpsatError
noise multistart GpsatError
noise sgpr NotImplementedError
noise full_cov lib
cv multistart GpsatError
cv full_cov lib
cv_refit multistart GpsatError
cv_refit full_cov GpsatError
multistart full_cov lib
sgpr full_cov NotImplementedError
rq f32 lib
mean f32 lib
noise f32 GpsatError
cv f32 lib
cv_refit f32 lib
multistart f32 lib
sgpr f32 NotImplementedError
full_cov f32 lib
rq D4 lib
mean D4 lib
noise D4 lib
cv D4 lib
cv_refit D4 lib
multistart D4 lib
sgpr D4 lib
full_cov D4 lib
""")
_matrix("model", """
rq engine
mean engine
noise engine
cv engine
cv_refit engine
multistart engine
sgpr engine
full_cov engine
rq mean NotImplementedError
rq noise NotImplementedError
rq cv NotImplementedError
rq cv_refit NotImplementedError
rq multistart NotImplementedError
rq sgpr NotImplementedError
rq full_cov engine
mean noise NotImplementedError
mean cv NotImplementedError
mean cv_refit NotImplementedError
mean multistart engine
mean sgpr NotImplementedError
mean full_cov engine
noise cv NotImplementedError
noise cv_refit NotImplementedError
noise multistart NotImplementedError
noise sgpr NotImplementedError
noise full_cov engine
cv multistart NotImplementedError
cv sgpr NotImplementedError
cv_refit multistart NotImplementedError
cv_refit sgpr NotImplementedError
multistart full_cov engine
sgpr full_cov NotImplementedError
rq f32 NotImplementedError
mean f32 NotImplementedError
noise f32 NotImplementedError
cv f32 engine
cv_refit f32 engine
multistart f32 engine
sgpr f32 NotImplementedError
full_cov f32 engine
rq D4 NotImplementedError
mean D4 NotImplementedError
noise D4 engine
cv D4 engine
cv_refit D4 engine
multistart D4 engine
sgpr D4 engine
full_cov D4 engine
""")
_matrix("orchestrator", """
rq built
mean built
noise built
cv built
cv_refit built
multistart NotImplementedError
sgpr built
replacement built
full_cov built
rq mean NotImplementedError
rq noise NotImplementedError
rq cv NotImplementedError
rq cv_refit NotImplementedError
rq multistart NotImplementedError
rq sgpr NotImplementedError
rq replacement NotImplementedError
rq full_cov built
mean noise NotImplementedError
mean cv NotImplementedError
mean cv_refit NotImplementedError
mean multistart NotImplementedError
mean sgpr NotImplementedError
mean replacement NotImplementedError
mean full_cov built
noise cv NotImplementedError
noise cv_refit NotImplementedError
noise multistart NotImplementedError
noise sgpr NotImplementedError
noise replacement NotImplementedError
noise full_cov built
cv multistart NotImplementedError
cv sgpr NotImplementedError
cv replacement built
cv full_cov NotImplementedError
cv_refit multistart NotImplementedError
cv_refit sgpr NotImplementedError
cv_refit replacement built
cv_refit full_cov NotImplementedError
multistart replacement NotImplementedError
multistart full_cov NotImplementedError
sgpr replacement built
sgpr full_cov NotImplementedError
replacement full_cov built
rq f32 NotImplementedError
mean f32 NotImplementedError
noise f32 NotImplementedError
cv f32 NotImplementedError
cv_refit f32 built
multistart f32 NotImplementedError
sgpr f32 NotImplementedError
replacement f32 built
full_cov f32 built
rq D4 NotImplementedError
mean D4 NotImplementedError
noise D4 built
cv D4 built
cv_refit D4 built
multistart D4 NotImplementedError
sgpr D4 built
replacement D4 built
full_cov D4 built
""")


@pytest.mark.parametrize("layer", list(LAYERS))
def test_every_pair_ends_as_it_did_before_the_table(layer):
    got = {c: outcome(layer, c) for c in EXPECTED[layer]}
    assert got == EXPECTED[layer], {c: (got[c], EXPECTED[layer][c]) for c in got if got[c] != EXPECTED[layer][c]}


def test_nothing_is_left_out_silently():
    for layer in LAYERS:
        assert set(EXPECTED[layer]) | INEXPRESSIBLE[layer] == set(CASES), layer
        assert not set(EXPECTED[layer]) & INEXPRESSIBLE[layer], layer
    assert len(CASES) == 9 + 36 + 9 + 9
    everywhere = set.intersection(*INEXPRESSIBLE.values())
    # one call is cv or its refit; a model, and an orchestrator's oi_model, is multi-start (sklearn) or sparse
    assert everywhere == {("cv", "cv_refit"), ("multistart", "sgpr")}


def _refused_somewhere(case):
    """Some layer that can express ``case`` refuses it, although it goes on with every single row of the case."""
    rows = [r for r in case if r in ROWS]
    for layer, (_, went_on) in LAYERS.items():
        exp = EXPECTED[layer]
        if case in exp and exp[case] != went_on and all(exp.get((r,)) == went_on for r in rows):
            return True
    return False


def test_the_table_agrees_with_the_matrix():
    V = pytest.importorskip("gpsat_amd.variants")
    assert list(V.VARIANTS) == ROWS
    for a, b in itertools.combinations(ROWS, 2):
        assert (b in V.VARIANTS[a].excludes) == (a in V.VARIANTS[b].excludes), (a, b)
        if (a, b) in set.intersection(*INEXPRESSIBLE.values()):
            assert b in V.VARIANTS[a].excludes, (a, b)        # two entry points of their own: no call carries both
            continue
        assert (b in V.VARIANTS[a].excludes) == _refused_somewhere((a, b)), (a, b)
        assert (V.why_refused([a, b], "f64", 2) is not None) == (b in V.VARIANTS[a].excludes), (a, b)
    for r in ROWS:
        assert ("f32" not in V.VARIANTS[r].dtypes) == _refused_somewhere((r, "f32")), r
        assert (V.VARIANTS[r].max_D < 4) == _refused_somewhere((r, "D4")), r
        assert (V.why_refused([r], "f32", 2) is None) == ("f32" in V.VARIANTS[r].dtypes)
        assert (V.why_refused([r], "f64", 4) is None) == (V.VARIANTS[r].max_D >= 4)
        assert V.why_refused([r], "f64", 2) is None


def test_layout_agrees_everywhere():
    """H, the names and the slots of the table, _lib.n_hyper, the library's own host functions and the model's theta."""
    V = pytest.importorskip("gpsat_amd.variants")
    lib = L.get_lib()
    calls = {"rq": ("RationalQuadratic", None), "mean": ("Matern32", "constant"), None: ("Matern32", None)}
    for D, (row, (kernel, mean)) in itertools.product((1, 2, 3, 4), calls.items()):
        asked = [row] if row else []
        names, H, slots = V.param_names(asked), V.n_hyper(D, asked), V.slots(D, asked)
        assert H == D + 2 + bool(row) == L.n_hyper(kernel, D, mean) == sum(w for _, w in slots.values())
        assert list(slots) == names and names[:3] == ["lengthscales", "kernel_variance", "likelihood_variance"]
        assert names[3:] == ([V.VARIANTS[row].param] if row else [])
        assert [s for s, _ in slots.values()] == [0] + list(range(D, H)) and slots["lengthscales"] == (0, D)
        built = row is None or D <= V.VARIANTS[row].max_D
        want = H if built else 0                              # the library answers 0 for what it does not build
        assert lib.gpsat_n_hyper_mean(L.KERNEL_IDS[kernel], D, L.MEAN_IDS[mean]) == want
        if mean is None:
            assert lib.gpsat_n_hyper(L.KERNEL_IDS[kernel], D) == want
        if built:
            X, y, _ = _tile(D)
            m = HipGPRModel(coords=X, obs=y, engine=_RecordingEngine(), dtype="f64", kernel=kernel,
                            mean_function="Constant" if mean else None)
            assert m._theta.shape == (H,) and m.param_names == names
            assert [m._slice(n) for n in names] == [slice(s, s + w) for s, w in slots.values()]


if __name__ == "__main__":
    for layer_, res_ in enumerate_all().items():
        print(f'_matrix("{layer_}", """')
        for c_, r_ in res_.items():
            print(" ".join(c_), r_)
        print('""")')
