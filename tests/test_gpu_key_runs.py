"""GPU: the keyed sort-and-run-heads stage (gpsat_key_runs.hip) through its three users, at the sizes and key patterns at
which it can go wrong (tests/key_runs_cases.py): either side of a wave and of a block of 256 rows, with and without the
sentinel's run, nothing but the sentinel's run, one group, one row per group, a sort over one bit and over 63.

The keyed glues: the BYTES of tests/golden/key_runs_pins.npz, which tests/golden/make_key_runs_pins.py stored from the library
as it was before the three copies of the stage became one.  Binning and the grouped tracks are pinned to references already
(scipy bit for bit; tests/prep_numpy.py): the checks of tests/test_gpu_binning.py and tests/test_gpu_prep.py at these sizes."""
import os

import numpy as np
import pytest

import key_runs_cases as kc
from test_gpu_binning import check_all
from test_gpu_prep import check_tracks
from test_prep_cpu import sorted_rows

pytestmark = pytest.mark.gpu
ROWS = [1, 255, 256, 257]


@pytest.fixture(scope="module")
def eng():
    from gpsat_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def pins(golden_dir):
    return kc.unpack(np.load(os.path.join(golden_dir, "key_runs_pins.npz")))


@pytest.mark.parametrize("kind,R", kc.CASES)
def test_keyed_glues_return_the_pinned_bytes(eng, pins, kind, R):
    want = pins[(kind, R)]
    assert kc.checksum(kc.case(kind, R)) == int(want["crc"]), "the case's inputs are not those the pins were made from"
    got = kc.outputs(eng, kind, R)
    assert int(got["G"]) == want["G"]
    for k in kc.FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_the_pins_cover_what_they_are_for(pins):
    """The sentinel's run present, absent and alone; one group; one row per group; one bit and 63 bits sorted."""
    for R in kc.SIZES:
        key = {kind: kc.case(kind, R)[0] for kind in kc.KINDS}
        assert (key["mixed"] >= 0).all() and (key["allneg"] < 0).all() and pins[("allneg", R)]["G"] == 0
        assert pins[("one", R)]["G"] == 1 and pins[("each", R)]["G"] == R and pins[("each", R)]["out_count"].tolist() == [1] * R
        assert key["key0"].max() == 0 and pins[("key0", R)]["out_key"].tolist() == [0]
        assert key["big"].max() == 2 ** 62 and pins[("big", R)]["out_key"][-1] == 2 ** 62
        if R > 1:
            assert (key["neg"] < 0).any() and (key["neg"] >= 0).any() and (key["key0"] < 0).any()
            assert pins[("neg", R)]["out_count"].sum() == (key["neg"] >= 0).sum()
        if R > 16:
            assert 1 < pins[("mixed", R)]["G"] < R and 1 < pins[("big", R)]["G"] < R


@pytest.mark.parametrize("where", ["inside", "some outside", "all outside"])
@pytest.mark.parametrize("R", ROWS)
def test_binning_against_scipy(eng, R, where):
    """All rows outside the grid: every run is the sentinel's, behind a sort that did run (the keyed glues return before it)."""
    rng = np.random.default_rng(R + len(where))
    lo, hi = {"inside": (-100.0, 100.0), "some outside": (-130.0, 130.0), "all outside": (150.0, 400.0)}[where]
    x, y, v = rng.uniform(lo, hi, R), rng.uniform(lo, hi, R), rng.uniform(-1e3, 1e3, R)
    e = np.linspace(-100, 100, 11)
    outside = (x < -100) | (x > 100) | (y < -100) | (y > 100)
    assert outside.all() if where == "all outside" else not outside.any() if where == "inside" else (R == 1 or 0 < outside.sum() < R)
    res = check_all(eng, x, y, v, e, e)
    assert res.stats["count"].sum() == R - outside.sum()
    res = check_all(eng, x, None, v, e, None, ["count", "mean", "std"])
    assert res.stats["count"].sum() == ((x >= -100) & (x <= 100)).sum()


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("R", ROWS)
def test_grouped_tracks_against_the_group_loop(eng, R, nulls):
    cols, codes = sorted_rows(np.random.default_rng(R + nulls), R, min(R, 5))
    if nulls:
        codes = np.where(np.arange(R) % 3 == 1, -1, codes) if R > 1 else np.full(R, -1)
    t = check_tracks(eng, cols, codes, 20.0, start_track=2)
    assert ((t == -1) == (np.sort(codes < 0))).all()          # rows in no group come last
