"""CPU: the host side of gpsat_select_batch_ex and gpsat_bin_batch (gpsat_amd/csrc/gpsat_select_plan.h, gpsat_bin_plan.h) -- the
checks of the criteria, row chunks, binning dimensions, expert order, scan, two-call cache; the checks, buffer layout and scalars
of the binning -- driven by tests/select_bin_host_check.cpp under the host sanitizers.

tests/golden/select_bin_plan.txt holds what the statements of gpsat_capi.cpp gave for the same cases before they became these
functions: they were compiled verbatim behind the new signatures (the handle, its buffers and the copies replaced by stand-ins
that record sizes and addresses) and printed by this same driver -- computed by that code, not by the functions under test."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from gpsat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "select_bin_plan.txt")
SECTIONS = ("chunks", "check_spec", "bin_dims", "expert_order", "scan", "bin_check", "bin_layout", "bin_scales")
# the least number of cases of every section (the cases the functions were split out with)
MIN_CASES = dict(chunks=60, check_spec=24, bin_dims=26, expert_order=5, scan=5, bin_check=37, bin_layout=56, bin_scales=9)
RECORDED_WITH = (1024, 1024)                 # select_sub_rows(), bin_long_rows() when the golden file was recorded


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _by_section(text):
    out = {s: [] for s in SECTIONS + ("cache",)}
    for ln in text.splitlines():
        out[ln.split(":")[0].split()[0]].append(ln)
    return out


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    """tests/select_bin_host_check.cpp built with the address and undefined-behaviour sanitizers, and what it prints for the
    library's own select_sub_rows() / bin_long_rows()."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("selbin") / "select_bin_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gpsat_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "select_bin_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip(f"{cxx} has no sanitizer runtime: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr
    lib = L.load()
    sizes = (lib._ZN5gpsat15select_sub_rowsEv(), lib._ZN5gpsat13bin_long_rowsEv())
    assert sizes == RECORDED_WITH, "the kernels' sub-chunk / long-cell sizes changed: record tests/golden/select_bin_plan.txt again"
    r = subprocess.run([exe, str(sizes[0]), str(sizes[1])], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr            # a sanitizer report or a failed internal check ends it non-zero
    return _by_section(r.stdout)


@pytest.mark.parametrize("section", SECTIONS)
def test_host_steps_give_what_the_entry_points_computed(host_output, section):
    want = _by_section(open(GOLDEN).read())[section]
    assert len(want) >= MIN_CASES[section]
    got = host_output[section]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_select_cache_forgets_on_any_changed_argument(host_output):
    """SelectCache: after remember(), matches() is false when any one remembered argument differs -- sizes, each table's address,
    each field of the criteria, each element of the tables' contents -- and after forget().  Checked inside the driver."""
    assert len(host_output["cache"]) == 1
    n = int(host_output["cache"][0].split()[1])
    assert n >= 7 + 1 + 4 * 7 + 1 + 10 + 6 + 2 + 1

