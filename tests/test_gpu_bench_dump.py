"""GPU: bench.py --dump-outputs on the timed path -- `--steps` sets the timed steps, `ms_per_step` is one of them, and two
runs with the same workload dump the same bits (the inputs depend on the arguments only; launches are bit-reproducible,
tests/test_gpu_reproducible.py).  bench.py runs as a child process, as it is run by hand: once plainly, which runs no leg
beyond the headline and spends little time outside its steps, and once with the legs' own switches, which change nothing."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, P = 64, 500
OUTSIDE_STEPS_S = 30.0          # what a plain run may spend outside its warm-up and timed steps, start to exit


def _bench(out_dir, steps, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--tiles", str(T), "--npred", str(P), *extra, "--dump-outputs", str(out_dir)]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return r, wall - (steps + 1) * r["ms_per_step"] * 1e-3


def test_dump_outputs_of_the_timed_path(tmp_path):
    r2, _ = _bench(tmp_path / "a", 2, ("--cpu-tiles", "0", "--no-host-leg", "--no-quality", "--no-other-workloads"))
    r3, outside = _bench(tmp_path / "b", 3)
    print(f"plain run: {outside:.1f} s outside its steps")
    assert outside < OUTSIDE_STEPS_S
    for r in (r2, r3):
        assert r["host_to_host_ms"] is None and not {"cpu_baseline", "quality", "other_workloads"} & set(r)
        assert r["metric"] == "local-expert tiles/sec (fit+predict)" and r["unit"] == "tiles/s" and r["higher_is_better"] is True
        assert r["dtype"] == "f32" and r["roofline"]["kernel_ms"] > 0
    for r, steps in ((r2, 2), (r3, 3)):
        assert r["steps"] == steps and r["ms_per_step"] > 0
        assert r["value"] * r["ms_per_step"] * 1e-3 == pytest.approx(T, rel=1e-2)        # tiles per second x one step = T
    names = {"theta", "nll", "status", "n_eval", "n_iter", "f_mean", "f_var", "y_var"}
    assert set(f[:-4] for f in os.listdir(tmp_path / "a")) == names
    for k in names:
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a))
        np.testing.assert_array_equal(a, b)
    assert np.load(tmp_path / "a" / "f_mean.npy").shape == (T * P,)
    assert np.load(tmp_path / "a" / "theta.npy").shape == (T, 5)
    assert not np.isin(np.load(tmp_path / "a" / "status.npy"), (2, 3)).any()          # no tile failed
