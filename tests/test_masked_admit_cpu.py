"""CPU: the admission rule of the resident loop's masked-support form
(path_planning_2d_amd/csrc/pp2_masked.h, pp2::masked_admit) is a plain host
function of (code plane, row stride, rows, dictionary).  tests/
masked_admit_check.cpp feeds it made-up models -- admitted ones (a map with a
walled-in free cell, free cells in a corner and on an edge, the goal next to
an occupied cell; no occupied cell; every cell occupied), each rejection (one
off-centre weight changed, a zero weight towards a free cell, a blocked cell
whose cost differs by action, one action's side weight changed everywhere, the
goal on an occupied cell) and the off-grid cases (the halo rows, the pad
columns, x = -1 / x = row stride, a code outside the dictionary) -- built here
with the host compiler and -fsanitize=address,undefined as its own executable.

Also: the additive ABI of the switch and the query.
"""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")


def test_masked_admit_host_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "masked_admit_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
         os.path.join(ROOT, "tests", "masked_admit_check.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases hold" in run.stdout


def test_masked_abi_is_additive():
    from path_planning_2d_amd import _lib
    from path_planning_2d_amd.core import GridContext
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    m = re.search(r"^#define PP2_TUNE_RESIDENT_MASKED (\d+)\b", text, re.M)
    assert m and int(m.group(1)) == GridContext.TUNE_RESIDENT_MASKED == 15
    keys = [int(v) for v in re.findall(r"^#define PP2_TUNE_\w+ (\d+)\b", text, re.M)]
    assert len(keys) == len(set(keys)), "tuning keys are distinct"
    assert re.search(r"\bint pp2_resident_masked\(pp2_ctx\* ctx, int\* admitted, int\* launches\);",
                     text)
    assert "pp2_resident_masked" in _lib.exported_symbols()
    lib = _lib.load()
    assert lib.pp2_resident_masked is not None
