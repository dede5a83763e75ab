"""CPU: the C-ABI library loads and exports every symbol include/gpsat_hip.h declares; the ctypes
mirror of gpsat_batch has the C layout.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from gpsat_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpsat_hip.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpsat_[a-z_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = L.load()
    names = _declared_functions()
    assert len(names) >= 8
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gpsat_hip.h but not exported"
    assert sorted(L.EXPORTS) == names
    assert lib.gpsat_version() == L.ABI_VERSION


def test_header_constants_match_binding():
    src = open(HEADER).read()
    def const(name):
        return int(re.search(rf"#define\s+{name}\s+(-?\d+)", src).group(1))
    assert const("GPSAT_ABI_VERSION") == L.ABI_VERSION
    assert const("GPSAT_KERNEL_RBF") == L.KERNEL_IDS["RBF"]
    assert const("GPSAT_KERNEL_MATERN12") == L.KERNEL_IDS["Matern12"]
    assert const("GPSAT_KERNEL_MATERN32") == L.KERNEL_IDS["Matern32"]
    assert const("GPSAT_KERNEL_MATERN52") == L.KERNEL_IDS["Matern52"]
    assert (const("GPSAT_OPT_NONE"), const("GPSAT_OPT_LBFGS"), const("GPSAT_OPT_ADAM")) == (0, 1, 2)
    assert (const("GPSAT_MEM_HOST"), const("GPSAT_MEM_DEVICE")) == (L.MEM_HOST, L.MEM_DEVICE)


MAX_TILE_OBS = {"f32": (4096, 4096, 3168, 2592), "f64": (4096, 3392, 2832, 2416)}     # D = 1 .. 4


def test_max_tile_obs_table_is_pinned():
    """gpsat_max_tile_obs decides which tiles the orchestrator sends: the whole table, and 0 outside it."""
    lib = L.load()
    for dtype, code in (("f32", 0), ("f64", 1)):
        assert tuple(lib.gpsat_max_tile_obs(code, D) for D in range(1, 5)) == MAX_TILE_OBS[dtype]
        assert tuple(L.max_tile_obs(dtype, D) for D in range(1, 5)) == MAX_TILE_OBS[dtype]
        assert lib.gpsat_max_tile_obs(code, 0) == 0 and lib.gpsat_max_tile_obs(code, 5) == 0
    for D in range(0, 6):
        assert lib.gpsat_max_tile_obs(2, D) == 0 and lib.gpsat_max_tile_obs(-1, D) == 0


def test_fp32_tile_limit_fits_the_sweep_flags():
    """phase_pt writes colrow[0 .. NB-1] (NB = ceil(N / 32)) into arrays of GPSAT_PT_MAXNB words: no fp32 tile the ABI
    accepts may have more block columns than that."""
    src = open(os.path.join(ROOT, "gpsat_amd", "csrc", "gpsat_kernels.h")).read()
    maxnb = int(re.search(r"#define\s+GPSAT_PT_MAXNB\s+(\d+)", src).group(1))
    cap = int(re.search(r"#define\s+GPSAT_MAX_TILE_OBS\s+(\d+)", src).group(1))
    assert 32 * maxnb >= cap
    lib = L.load()
    for D in range(1, 5):
        assert 0 < lib.gpsat_max_tile_obs(0, D) <= 32 * maxnb
        assert max(lib.gpsat_max_tile_obs(0, D), lib.gpsat_max_tile_obs(1, D)) <= cap
    # the flag words are declared with that size, and nowhere with a literal
    csrc = os.path.join(ROOT, "gpsat_amd", "csrc")
    decls = [re.findall(r"\bcolrow\[([^\]]*)\];", open(os.path.join(csrc, f)).read()) for f in ("gpsat_opt.h", "gpsat_coop.h")]
    assert decls == [["GPSAT_PT_MAXNB"], ["GPSAT_PT_MAXNB"]], decls
    srcs = "".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".cpp", ".hip", ".h")))
    assert len(re.findall(r"#define\s+GPSAT_PT_MAXNB\b", srcs)) == 1


def test_four_wave_thresholds_of_the_build_matrix():
    """tests/test_gpu_build_matrix.py sizes its 4-wave batches from W4_NB / D4_NB: the largest tile (blocks) whose 4-wave LDS
    layout fits 80 KiB, the rule by which gpsat::plan_tiles (gpsat_plan.h) picks the 4-wave builds.  If the layouts drift, those
    batches would quietly run on the 8-wave builds; this fails instead."""
    from test_gpu_build_matrix import D4_NB, W4_NB
    lib = L.load()
    for name, table in (("_ZN5gpsat12shared_bytesEii", W4_NB), ("_ZN5gpsat19shared_bytes_f64_w4Eii", D4_NB)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_size_t, [C.c_int, C.c_int]
        got = {D: max(nb for nb in range(1, 512) if fn(D, nb) <= 80 * 1024) for D in range(1, 5)}
        assert got == table, (name, got)


def test_struct_layout_matches_c(tmp_path):
    """Compile a tiny C program against the header and compare sizeof/offsetof with ctypes."""
    fields = [f[0] for f in L.GpsatBatch._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gpsat_hip.h"', 'int main(){',
            'printf("%zu\\n", sizeof(gpsat_batch));']
    for f in fields:
        prog.append(f'printf("%zu\\n", offsetof(gpsat_batch, {f}));')
    prog.append('printf("%zu\\n", sizeof(gpsat_opts)); return 0;}')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.GpsatBatch)
    for f, off in zip(fields, vals[1:-1]):
        assert getattr(L.GpsatBatch, f).offset == off, f
    assert vals[-1] == C.sizeof(L.GpsatOpts)


def test_no_device_is_reported_not_faked():
    """Without a GPU the library says so; the product path never falls back to the CPU."""
    lib = L.load()
    if lib.gpsat_device_count() > 0:
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = lib.gpsat_create(0, None, C.byref(h))
    assert rc != 0 and not h.value
    assert b"no HIP device" in lib.gpsat_last_error()
    from gpsat_amd.engine import Engine, GpsatError
    with pytest.raises(GpsatError):
        Engine(0)


def test_product_package_never_imports_oracle():
    """The oracle is test infrastructure: nothing under gpsat_amd/ may import it."""
    pkg = os.path.join(ROOT, "gpsat_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "gp_oracle" not in txt, f


def test_developer_knobs_are_gated():
    """No environment variable changes what the shipped library does unless GPSAT_DEVELOPER=1 is set: every GPSAT_DEBUG_*
    knob goes through dev_env(), and the only plain getenv in the native sources is the one that reads GPSAT_DEVELOPER."""
    src = os.path.join(ROOT, "gpsat_amd", "csrc")
    plain = []
    for f in os.listdir(src):
        if f.endswith((".cpp", ".hip", ".h")):
            for ln, line in enumerate(open(os.path.join(src, f)), 1):
                if "getenv(" in line and "dev_env(" not in line.split("getenv(")[0][-12:]:
                    plain.append((f, ln, line.strip()))
    assert all('"GPSAT_DEVELOPER"' in l or "return std::getenv(name)" in l for _, _, l in plain), plain
    assert len(plain) == 2, plain


class _Knob(C.Structure):
    _fields_ = [("set", C.c_int), ("v", C.c_int)]


class _PlanInput(C.Structure):               # gpsat::PlanInput (gpsat_amd/csrc/gpsat_plan.h)
    _fields_ = [("T", C.c_int), ("D", C.c_int), ("f64", C.c_int), ("obs_off", C.POINTER(C.c_int64)), ("maxP", C.c_longlong),
                ("want_cov", C.c_int), ("has_pred", C.c_int), ("optimiser", C.c_int), ("max_iter", C.c_int), ("num_cu", C.c_int),
                ("wg_per_cu", C.c_int), ("solo", C.c_int), ("unsliced", C.c_int), ("knobs", _Knob * 8)]


class _TilePlan(C.Structure):                # gpsat::TilePlan
    _fields_ = [(n, C.c_int) for n in ("build", "NBmax", "PCcov", "grid", "team", "coop", "coop_min_nb", "coop_hdiv", "coop_force",
                                       "seg_cost", "state_words", "pq_slots")] + \
               [(n, C.c_size_t) for n in ("smem", "ws_stride", "ring_cap", "pq_stride")]


# build: 0 fp32 4-wave, 1 fp32 8-wave, 2 fp64 8-wave, 3 fp64 4-wave.  The values are those of the launch rules as they stood
# inside fit_predict_impl before they became gpsat::plan_tiles (computed by that code, not by the function under test).
_COMMON = dict(PCcov=0, coop_min_nb=12, coop_hdiv=12, coop_force=0)
MEASURED_PLANS = {
    "configs1": (dict(f64=0, Ns=[500] * 4096, optimiser=1, max_iter=20),
                 dict(build=0, NBmax=16, grid=512, team=1, coop=0, seg_cost=16384, state_words=772, pq_slots=4096, smem=67120,
                      ws_stride=418816, ring_cap=8192, pq_stride=141568)),
    "configs2": (dict(f64=0, Ns="ragged", optimiser=1, max_iter=20),
                 dict(build=1, NBmax=64, grid=256, team=1, coop=1, seg_cost=0, state_words=772, pq_slots=0, smem=122416,
                      ws_stride=5317632, ring_cap=0, pq_stride=0)),
    "configs4": (dict(f64=1, Ns=[2000] * 1024, optimiser=0, max_iter=0),
                 dict(build=2, NBmax=125, grid=256, team=1, coop=0, seg_cost=0, state_words=636, pq_slots=0, smem=123904,
                      ws_stride=5066496, ring_cap=0, pq_stride=0)),
    "f64fit": (dict(f64=1, Ns=[500] * 4096, optimiser=1, max_iter=20),
               dict(build=3, NBmax=32, grid=512, team=1, coop=0, seg_cost=131072, state_words=636, pq_slots=0, smem=75008,
                    ws_stride=411904, ring_cap=8192, pq_stride=0)),
    # fewer tiles than CUs: the 8-wave build with cooperative tiles, the grid widened by three helpers per tile
    "64 tiles of 1500": (dict(f64=0, Ns=[1500] * 64, optimiser=1, max_iter=20),
                         dict(build=1, NBmax=47, grid=256, team=1, coop=1, seg_cost=0, state_words=772, pq_slots=0, smem=102832,
                              ws_stride=3089408, ring_cap=0, pq_stride=0)),
    "fp64 teams": (dict(f64=1, Ns=[2000] * 16, optimiser=1, max_iter=20),
                   dict(build=2, NBmax=125, grid=256, team=16, coop=0, seg_cost=0, state_words=636, pq_slots=0, smem=123904,
                        ws_stride=5066496, ring_cap=0, pq_stride=0)),
}


@pytest.mark.parametrize("name", list(MEASURED_PLANS))
def test_launch_plan_of_the_measured_shapes(name):
    """gpsat::plan_tiles decides build, grid, teams, cooperative tiles, time slicing and the deferred-prediction pool from host
    data alone: its plan for the shapes the project measures (bench.py's workloads, D = 3, 500 predictions per tile), on 256
    CUs with the default two workgroups per CU and no developer knob."""
    import numpy as np
    lib = L.load()
    fn = getattr(lib, "_ZN5gpsat10plan_tilesERKNS_9PlanInputERNS_8TilePlanE")
    fn.restype, fn.argtypes = C.c_bool, [C.POINTER(_PlanInput), C.POINTER(_TilePlan)]
    case, want = MEASURED_PLANS[name]
    Ns = case["Ns"]
    if isinstance(Ns, str):                  # bench.py --workload configs2
        Ns = np.random.default_rng(0).choice([128, 256, 384, 512, 768, 1024, 1536, 2048], 4096)
    off = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
    pin = _PlanInput(T=len(Ns), D=3, f64=case["f64"], obs_off=off.ctypes.data_as(C.POINTER(C.c_int64)), maxP=0, want_cov=0, has_pred=1,
                     optimiser=case["optimiser"], max_iter=case["max_iter"], num_cu=256, wg_per_cu=2, solo=0, unsliced=0)
    plan = _TilePlan()
    assert fn(C.byref(pin), C.byref(plan))
    got = {n: getattr(plan, n) for n, _ in _TilePlan._fields_}
    assert got == {**_COMMON, **want}, got
