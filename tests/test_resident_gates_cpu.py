"""CPU: the path gates of the sparse rows, the tile-resident loop and the
tile-resident sweeps (path_planning_2d_amd/csrc/pp2_dict_props.h) are plain
host functions of the dictionary rows, gamma and a few context switches and
state flags.  tests/resident_gates_check.cpp feeds them made-up dictionaries --
a generated-like one, then one violation at a time: an on-support T entry
negative, -0, +-inf or NaN; an L entry likewise; a cost -0, negative, inf, NaN
or overflowing; gamma 1.0, negative, NaN; an off-support T entry; 17 classes
for one action; 33 L vectors; the belief or the values flag false; each switch
-- and asserts the truth table row by row, built here with the host compiler
and -fsanitize=address,undefined as its own executable.

The program also carries the predicates as they stood before the header
(no sign or finiteness test of T on the sweep gate and on the sparse rows, no
flag for the values) and prints the rows those get wrong; the list is pinned
here, as the record of what the table catches.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")


@pytest.fixture(scope="module")
def checker_output(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("gates") / "resident_gates_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
         os.path.join(ROOT, "tests", "resident_gates_check.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_truth_table_holds(checker_output):
    assert "all rows hold" in checker_output
    assert "FAIL" not in checker_output
    m = re.search(r"^(\d+) rows, 0 failures$", checker_output, re.M)
    assert m and int(m.group(1)) >= 40


def test_rows_the_earlier_predicates_got_wrong(checker_output):
    """The earlier sweep gate and sparse rows admitted every on-support T
    violation, and nothing looked at the values' state."""
    was = set(re.findall(r"^before: (.+) was 1, want 0$", checker_output, re.M))
    assert not re.search(r"^before: .+ was 0, want 1$", checker_output, re.M)
    want = set()
    for t in ("negative", "-0", "+inf", "NaN", "-inf", "negative NaN"):
        for where in ("main", "side"):
            for col in ("sweep", "sparse"):
                want.add(f"on-support T {t} ({where}) / {col}")
    for col in ("loop", "sweep", "sparse"):
        want.add(f"clean, values flag false / {col}")
    assert was == want


def test_header_is_plain_host_code():
    text = open(os.path.join(CSRC, "pp2_dict_props.h")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
