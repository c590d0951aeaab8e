"""CPU: the shortest-path field's reference (tests/path_reference.py) agrees
with itself -- heap Dijkstra and whole-grid Jacobi end on the same bits, and
the result satisfies the defining equations cell by cell --, the hand-written
values of the definition, and the host-side surface of the feature: the six
symbols, the Python argument checks, the A* ROS adapter and the demo compile.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import path_reference as R
from path_planning_2d_amd import _lib
from path_planning_2d_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pp2_path_solve", "pp2_path_get", "pp2_path_control", "pp2_path_trace",
           "pp2_path_info", "pp2_episodes_set_action_table"]


def _cases():
    for name in ("map_3x3", "map_5x5", "map_10x10", "sparse_map_100x40"):
        yield name, R.golden_case(name)
    yield "synth_40x100", (R.freed(S.synth_grid(40, 100, 3)), (0, 0))
    yield "serpentine_33x70", (R.serpentine(33, 70), (0, 0))


@pytest.mark.parametrize("name,case", list(_cases()), ids=[n for n, _ in _cases()])
def test_dijkstra_equals_jacobi_and_is_the_fixpoint(name, case):
    grid, goal = case
    Dd = R.dijkstra(grid, goal)
    Dj, _ = R.jacobi(grid, goal)
    assert np.array_equal(R.bits(Dd), R.bits(Dj))
    R.check_fixpoint(Dd, grid, goal)
    A = R.actions(Dd, grid, goal)
    fin = np.isfinite(Dd)
    assert (A[~fin] == 4).all()
    assert int((A[fin] == 4).sum()) == (1 if R.goal_ok(grid, goal) else 0)


def test_synth_40x100_has_an_unreachable_free_cell():
    grid = R.freed(S.synth_grid(40, 100, 3))
    D = R.dijkstra(grid, (0, 0))
    assert int(np.isfinite(D).sum()) == int((grid != 1).sum()) - 1


def test_serpentine_is_one_corridor():
    grid = R.serpentine(33, 70)
    D = R.dijkstra(grid, (0, 0))
    A = R.actions(D, grid, (0, 0))
    far = int(np.argmax(np.where(np.isfinite(D), D, -1)))
    cells, length = R.trace(A, D, far)
    # 17 lanes of 70 cells: the path runs the length of each (it cuts the
    # corners at the 16 gaps diagonally)
    assert 17 * 68 <= len(cells) <= 17 * 70 + 16 and length == D.reshape(-1)[far]
    assert cells[-1] == 0 and (np.diff(D.reshape(-1)[cells]) < 0).all()


def test_hand_written_open_3x3():
    """Open 3 x 3, goal in the corner (0, 0)."""
    f = np.float32
    r2 = R.C_DIAG
    assert r2.view(np.uint32) == 0x3FB504F3 and r2 == f(np.sqrt(f(2.0)))
    grid = np.zeros((3, 3), np.uint8)
    D = R.dijkstra(grid, (0, 0))
    want = np.array([[f(0), f(1), f(2)],
                     [f(1), r2, f(r2 + f(1))],
                     [f(2), f(r2 + f(1)), f(r2 + r2)]], np.float32)
    assert np.array_equal(R.bits(D), R.bits(want))
    R.check_fixpoint(D, grid, (0, 0))
    A = R.actions(D, grid, (0, 0))
    # (x, y) = (1, 2), two rows and one column from the goal: fl(1 + sqrt 2)
    # through move 0 (to (0, 1)) and fl(sqrt 2 + 1) through move 1 (to
    # (1, 1)) are the same number; the lower u wins
    assert f(D[1, 0] + r2) == f(D[1, 1] + f(1))
    assert A[2, 1] == 0
    assert A.tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 0]]


def test_degenerate_goals_of_the_reference():
    grid = np.zeros((4, 5), np.uint8)
    grid[2, 3] = 1
    for goal in ((3, 2), (-1, -1), (5, 0)):
        D = R.dijkstra(grid, goal)
        assert np.isinf(D).all() and (R.actions(D, grid, goal) == 4).all()
        R.check_fixpoint(D, grid, goal)


def test_symbols_declared_exported_bound():
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % s, header, re.M), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert re.search(r"#define PP2_TABLE_MDP\s+0\b", header)
    assert re.search(r"#define PP2_TABLE_PATH\s+1\b", header)
    assert lib.pp2_abi_version() == 4 and _lib.PP2_ABI_VERSION == 4


class _NoLibrary:
    """Stands in for the handle: any use would be a library call."""
    rows, width = 4, 5

    @property
    def _h(self):
        raise AssertionError("the library was reached")


def test_argument_errors_do_not_reach_the_library():
    from path_planning_2d_amd import EpisodeBatch, GridContext
    ctx = _NoLibrary()
    for start in (-1, 20, (5, 0), (0, 4), (-1, 0), (1, 2, 3)):
        with pytest.raises(ValueError):
            GridContext.path_trace(ctx, start)
    for table in ("astar", "MDP", 1, None, 2):
        with pytest.raises(ValueError):
            EpisodeBatch.set_action_table(ctx, table)


def test_astar_ros_adapter_compiles():
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    stubs = os.path.join(ROOT, "tests", "ros_stubs")
    src = os.path.join(ROOT, "ros", "src", "astar", "path_planning_2d_pp2.cpp")
    cmd = [cxx, "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
           "-Wno-unused-parameter",
           "-I", os.path.join(ROOT, "ros", "include"),
           "-I", stubs, "-I", os.path.join(stubs, "path_planning_2d"),
           "-I", os.path.join(ROOT, "include"), src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_astar_demo_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    lib_dir = os.path.join(ROOT, "path_planning_2d_amd")
    if not os.path.exists(os.path.join(lib_dir, "libpp2_hip.so")):
        pytest.skip("library not built")
    exe = tmp_path / "demo"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "examples", "pp2_astar_demo.c"),
                    "-L", lib_dir, "-lpp2_hip"], check=True)
    assert exe.exists()


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    n = ctypes.c_int(0)
    assert lib.pp2_path_solve(None, 1, None, None, None) != 0
    assert lib.pp2_path_get(None, None, None) != 0
    assert lib.pp2_path_trace(None, 0, None, 0, ctypes.byref(n), None) != 0
    assert lib.pp2_path_info(None, None, None, None, None, None, None) != 0
    assert lib.pp2_path_control(None, None, None, None) != 0
    assert lib.pp2_episodes_set_action_table(None, 0) != 0
