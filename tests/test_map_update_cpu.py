"""CPU: the live map / goal update's additive ABI (include/pp2.h "live
updates": pp2_map_update, pp2_goal_set, pp2_map_get, pp2_map_update_info,
pp2_mdp_resolve, PP2_TUNE_MAP_INCREMENTAL) and the windowed form of the masked
admission (pp2_masked.h, pp2::masked_admit_window) that an update runs instead
of the whole-plane masked_admit.

tests/masked_window_check.cpp holds the windowed form to the rule's own
statement on 12 x 16 code planes of generated dictionaries: every window
position on admitted planes, the window of a map change against masked_admit
on the changed plane, and one deliberately wrong cell inside the window, just
below it and in the row above it.  It is built here with the host compiler and
-fsanitize=address,undefined as its own executable; nothing loaded into Python
runs under a sanitizer.  The GPU side: test_gpu_map_update.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")

NEW = {
    "pp2_map_update": r"int pp2_map_update\(pp2_ctx\* ctx, uint32_t x0, uint32_t y0, uint32_t w, "
                      r"uint32_t h,\s+const uint8_t\* patch\);",
    "pp2_goal_set": r"int pp2_goal_set\(pp2_ctx\* ctx, int32_t gx, int32_t gy\);",
    "pp2_map_get": r"int pp2_map_get\(pp2_ctx\* ctx, uint8_t\* map, int32_t\* gx, int32_t\* gy\);",
    "pp2_map_update_info": r"int pp2_map_update_info\(pp2_ctx\* ctx, long long\* updates, "
                           r"long long\* incremental,\s+long long\* rebuilds, "
                           r"int\* entries_added\);",
    "pp2_mdp_resolve": r"int pp2_mdp_resolve\(pp2_ctx\* ctx, int max_sweeps, int\* sweeps,\s+"
                       r"double\* final_norm\);",
}


def test_masked_window_host_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "masked_window_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
         os.path.join(ROOT, "tests", "masked_window_check.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases hold" in run.stdout


def test_abi_is_additive():
    from path_planning_2d_amd import _lib
    from path_planning_2d_amd.core import GridContext
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    m = re.search(r"^#define PP2_TUNE_MAP_INCREMENTAL (\d+)\b", text, re.M)
    assert m and int(m.group(1)) == GridContext.TUNE_MAP_INCREMENTAL == 16
    keys = [int(v) for v in re.findall(r"^#define PP2_TUNE_\w+ (\d+)\b", text, re.M)]
    assert len(keys) == len(set(keys)), "tuning keys are distinct"
    lib = _lib.load()
    assert lib.pp2_abi_version() == 4
    for name, decl in NEW.items():
        assert re.search(decl, text), f"{name}: declaration"
        assert name in _lib.exported_symbols(), name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name])


def test_binding_argument_types():
    from path_planning_2d_amd import _lib
    S = _lib.SIGNATURES
    u8p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    ll = ctypes.POINTER(ctypes.c_longlong)
    assert S["pp2_map_update"] == [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [u8p]
    assert S["pp2_goal_set"] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    assert S["pp2_map_get"] == [ctypes.c_void_p, u8p, i32p, i32p]
    assert S["pp2_map_update_info"] == [ctypes.c_void_p, ll, ll, ll, ctypes.POINTER(ctypes.c_int)]
    assert S["pp2_mdp_resolve"] == S["pp2_mdp_solve"]


def test_python_surface():
    from path_planning_2d_amd.core import GridContext
    for name in ("map_update", "goal_set", "map_get", "mdp_resolve", "map_update_info"):
        assert callable(getattr(GridContext, name)), name


def test_null_context_is_an_error_not_a_crash():
    """No device here: every new entry point returns a status on a null context."""
    from path_planning_2d_amd import _lib
    lib = _lib.load()
    patch = np.zeros(1, np.uint8)
    p = patch.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.pp2_map_update(None, 0, 0, 1, 1, p) == 1
    assert lib.pp2_goal_set(None, 0, 0) == 1
    assert lib.pp2_map_get(None, None, None, None) == 1
    assert lib.pp2_map_update_info(None, None, None, None, None) == 1
    assert lib.pp2_mdp_resolve(None, 0, None, None) == 1
    with pytest.raises(_lib.Pp2Error):
        _lib.call("pp2_goal_set", None, 1, 1)
