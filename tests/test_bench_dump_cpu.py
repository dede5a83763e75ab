"""CPU: bench.py's --dump-outputs writer and the inputs it is compared on -- the same tiles whatever the host's BLAS thread
count, every output of the step written in float32 / float64, and a fixed sample of tiles within the size bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from gpsat_amd import synthetic as syn
from gpsat_amd.engine import BatchResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(T, P, D, dt=np.float32, seed=0):
    rng = np.random.default_rng(seed)
    return BatchResult(theta=rng.uniform(0.1, 5, (T, D + 2)), nll=rng.normal(0, 100, T), status=rng.integers(0, 2, T).astype(np.int32),
                       n_eval=rng.integers(5, 40, T).astype(np.int32), f_mean=rng.standard_normal(T * P).astype(dt),
                       f_var=rng.uniform(0, 1, T * P).astype(dt), y_var=rng.uniform(0, 1, T * P).astype(dt),
                       n_iter=rng.integers(3, 20, T).astype(np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_dump_writes_every_output_of_the_step(tmp_path, dt):
    T, P, D = 12, 7, 3
    r = _result(T, P, D, dt)
    bench.dump_outputs(str(tmp_path), r, np.arange(T + 1) * P)
    got = _load(str(tmp_path))
    assert set(got) == {"theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var"}
    for k in ("theta", "nll", "status", "n_eval", "n_iter"):
        assert got[k].dtype == np.float64
        np.testing.assert_array_equal(got[k], getattr(r, k))
    for k in ("f_mean", "f_var", "y_var"):
        assert got[k].dtype == dt
        np.testing.assert_array_equal(got[k], getattr(r, k))


def test_dump_over_the_bound_is_a_fixed_sample_of_whole_tiles(tmp_path):
    T, D = 300, 3
    Pt = np.random.default_rng(1).integers(0, 40, T)                 # ragged predictions, some tiles without any
    pred_off = np.concatenate([[0], np.cumsum(Pt)])
    r = _result(T, 40, D)
    budget = 40_000
    shapes = bench.dump_outputs(str(tmp_path / "a"), r, pred_off, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), r, pred_off, budget=budget)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= budget
    assert {k: list(v.shape) for k, v in a.items()} == shapes
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["tile_index"].astype(np.int64)
    assert 0 < len(idx) < T and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["theta"], r.theta[idx])
    np.testing.assert_array_equal(a["n_eval"], r.n_eval[idx])
    rows = np.concatenate([np.arange(pred_off[t], pred_off[t + 1]) for t in idx])
    np.testing.assert_array_equal(a["f_var"], r.f_var[rows])


def test_bench_inputs_do_not_depend_on_the_blas_thread_count():
    from threadpoolctl import threadpool_limits
    jobs = [(1_000_000 + t, 500, 50, 3, 0) for t in range(4)] + [(100 + t, 1024, 50, 3, 2) for t in range(2)]
    with threadpool_limits(1):
        want = [syn.make_tile(*j[:3], D=j[3], kid=j[4]) for j in jobs]
    with threadpool_limits(8):
        for workers in (1, 3):
            got = bench.gen_tiles(jobs, workers)
            for g, w in zip(got, want):
                for x, y in zip(g, w):
                    np.testing.assert_array_equal(x, y)


def test_steps_below_one_are_refused_before_the_gpu_is_touched():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr


LEGS = ("cpu_tiles", "no_host_leg", "no_quality", "no_other_workloads")


def test_a_plain_run_has_no_leg_beyond_the_headline_and_full_has_them_all():
    """Every leg of the benchmark outside setting up, warming up, the timed steps, --dump-outputs and the result line is
    decided by these four arguments (bench.main reads nothing else for them)."""
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not plain.full and [getattr(plain, k) for k in LEGS] == [0, True, True, True]
    # the legs' own switches and sizes change nothing without --full
    same = bench.parse_args(["--cpu-tiles", "64", "--no-sklearn"])
    assert [getattr(same, k) for k in LEGS] == [0, True, True, True]
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert full.full and [getattr(full, k) for k in LEGS] == [-1, False, False, False] and not full.no_sklearn
    # ... and take their leg out of a full run as before
    part = bench.parse_args(["--full", "--cpu-tiles", "0", "--no-host-leg", "--no-other-workloads"])
    assert [getattr(part, k) for k in LEGS] == [0, True, False, True]
    for k in ("steps", "warmup", "tiles", "nobs", "npred", "dim", "kernel", "optimiser", "max_iter", "workload", "dump_outputs"):
        assert getattr(plain, k) == getattr(full, k)                # the timed workload is the same one
