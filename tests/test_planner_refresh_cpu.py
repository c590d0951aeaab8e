"""CPU: the additive ABI of the planner's live-update path (include/pp2.h:
pp2_planner_refresh, pp2_planner_refresh_info, pp2_planner_root_belief,
pp2_planner_rand_calls, pp2_fib_resolve), its Python mirrors, and the journal
of model updates behind it (csrc/pp2_journal.h).

tests/planner_journal_check.cpp holds the journal's ring to its statement: no
rectangles for the current serial, the k rectangle pairs of k updates back,
"unknown" beyond the capacity, wrap-around of the ring and of the serial.  It
is built here with the host compiler and -fsanitize=address,undefined as its
own executable; nothing loaded into Python runs under a sanitizer.  The GPU
side: test_gpu_planner_refresh.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")

NEW = {
    "pp2_planner_refresh": r"int pp2_planner_refresh\(pp2_planner\* p\);",
    "pp2_planner_refresh_info": r"int pp2_planner_refresh_info\(pp2_planner\* p, long long\* refreshes, "
                                r"long long\* incremental,\s+long long\* full, "
                                r"long long\* cells_patched\);",
    "pp2_planner_root_belief": r"int pp2_planner_root_belief\(pp2_planner\* p, float\* belief\);",
    "pp2_planner_rand_calls": r"int pp2_planner_rand_calls\(pp2_planner\* p, uint64_t\* calls\);",
    "pp2_fib_resolve": r"int pp2_fib_resolve\(pp2_ctx\* ctx, int max_sweeps, int\* sweeps, "
                       r"float\* final_norm\);",
}


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def test_journal_host_program(tmp_path):
    exe = str(tmp_path / "planner_journal_check")
    build = subprocess.run(
        [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
         os.path.join(ROOT, "tests", "planner_journal_check.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases hold" in run.stdout


def test_journal_capacity_is_named():
    text = open(os.path.join(CSRC, "pp2_journal.h")).read()
    m = re.search(r"constexpr int kJournalCap = (\d+);", text)
    assert m and int(m.group(1)) >= 2
    assert "#include" not in text, "the journal is plain host code with no dependencies"
    internal = open(os.path.join(CSRC, "pp2_internal.h")).read()
    assert re.search(r"constexpr int kPlannerPatchCells = \d+;", internal)


def test_abi_is_additive():
    from path_planning_2d_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    lib = _lib.load()
    assert lib.pp2_abi_version() == 4
    for name, decl in NEW.items():
        assert re.search(decl, text), f"{name}: declaration"
        assert name in _lib.exported_symbols(), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name])
    assert "create a new one" not in text
    assert re.search(r"PP2_ESTATE until pp2_planner_refresh", text)


def test_binding_argument_types():
    from path_planning_2d_amd import _lib
    S = _lib.SIGNATURES
    ll = ctypes.POINTER(ctypes.c_longlong)
    assert S["pp2_planner_refresh"] == [ctypes.c_void_p]
    assert S["pp2_planner_refresh_info"] == [ctypes.c_void_p, ll, ll, ll, ll]
    assert S["pp2_planner_root_belief"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    assert S["pp2_planner_rand_calls"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    assert S["pp2_fib_resolve"] == S["pp2_fib_solve"]


def test_python_surface():
    from path_planning_2d_amd.core import GridContext
    from path_planning_2d_amd.planner import QVTreePlanner
    for name in ("refresh", "refresh_info", "root_belief", "rand_calls"):
        assert callable(getattr(QVTreePlanner, name)), name
    assert callable(GridContext.fib_resolve)


def test_null_arguments_are_errors_not_crashes():
    """No device here: every new entry point returns PP2_EINVAL on null."""
    from path_planning_2d_amd import _lib
    lib = _lib.load()
    assert lib.pp2_planner_refresh(None) == 1
    assert lib.pp2_planner_refresh_info(None, None, None, None, None) == 1
    assert lib.pp2_planner_root_belief(None, None) == 1
    assert lib.pp2_planner_rand_calls(None, None) == 1
    assert lib.pp2_fib_resolve(None, 0, None, None) == 1
    with pytest.raises(_lib.Pp2Error):
        _lib.call("pp2_planner_refresh", None)


def test_demo_compiles_with_werror(tmp_path):
    """examples/pp2_pomdp_replan_demo.c is C99 against pp2.h alone."""
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = os.path.join(ROOT, "examples", "pp2_pomdp_replan_demo.c")
    includes = re.findall(r'#include "([^"]+)"', open(src).read())
    assert includes == ["pp2.h"], includes
    obj = str(tmp_path / "demo.o")
    build = subprocess.run(
        [cc, "-std=c99", "-pedantic", "-O2", "-Wall", "-Wextra", "-Werror", "-I",
         os.path.join(ROOT, "include"), "-c", "-o", obj, src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pp2_pomdp_replan_demo" in mk
