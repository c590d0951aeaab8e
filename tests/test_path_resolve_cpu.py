"""CPU: the warm re-solve of the shortest-path field (pp2_path_resolve).

The method's reference (tests/path_resolve_reference.py: raise what no longer
stands, then relax) ends on the bits of Dijkstra on the new map, over seeded
random grids with mixed patches and on every construction the GPU tests use;
relaxing the stale field without the raise does not, on each construction built
to catch an under-raise -- which is what shows that the GPU cases can fail.
Then the figures the constructions are quoted with, the pending list's host
program (tests/path_pending_check.cpp, built here with the host compiler and
-fsanitize=address,undefined as its own executable; nothing loaded into Python
runs under a sanitizer), and the host-side surface: symbols, null handles, the
example.  The GPU side: test_gpu_path_resolve.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import path_reference as R
import path_resolve_reference as WR
from path_planning_2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")
SYMBOLS = ["pp2_path_resolve", "pp2_path_resolve_info"]
TILE = (32, 64)

CASES = dict(WR.constructions())


@pytest.fixture(scope="module")
def solved():
    """name -> (old D, old A, D of the new map), once."""
    out = {}
    for name, c in CASES.items():
        D, A = R.field(c["grid"], c["goal"])
        out[name] = (D, A, R.dijkstra(c["grid_new"], c["goal"]))
    return out


def random_case(rng):
    H, W = int(rng.integers(6, 30)), int(rng.integers(6, 36))
    grid = (rng.random((H, W)) < rng.uniform(0.1, 0.4)).astype(np.uint8)
    free = np.flatnonzero(grid.reshape(-1) != 1)
    g = int(rng.choice(free))
    goal = (g % W, g // W)
    new = grid.copy()
    for _ in range(int(rng.integers(1, 5))):
        h, w = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        kind = rng.integers(0, 3)
        patch = (np.ones((h, w)) if kind == 0 else np.zeros((h, w)) if kind == 1
                 else rng.random((h, w)) < 0.5)
        new[y0:y0 + h, x0:x0 + w] = patch
    new[goal[1], goal[0]] = 0          # the goal cell's occupancy stays
    return grid, new, goal


def test_warm_resolve_equals_dijkstra_on_random_grids():
    rng = np.random.default_rng(2024)
    wrong = 0
    for i in range(60):
        grid, new, goal = random_case(rng)
        D, A = R.field(grid, goal)
        want = R.dijkstra(new, goal)
        got = WR.warm_resolve(D, A, new)
        assert np.array_equal(R.bits(got), R.bits(want)), i
        wrong += not np.array_equal(R.bits(WR.relax_without_raise(D, new)), R.bits(want))
        # a second update on top of the re-solved field
        A1 = R.actions(got, new, goal)
        new2 = new.copy()
        new2[rng.integers(0, new.shape[0]), :] ^= (rng.random(new.shape[1]) < 0.3)
        new2[goal[1], goal[0]] = 0
        got2 = WR.warm_resolve(got, A1, new2)
        assert np.array_equal(R.bits(got2), R.bits(R.dijkstra(new2, goal))), i
    assert wrong > 20, wrong           # the raise is not decoration


@pytest.mark.parametrize("name", list(CASES))
def test_constructions_warm_resolve_equals_dijkstra(solved, name):
    c = CASES[name]
    D, A, want = solved[name]
    assert np.array_equal(R.bits(WR.warm_resolve(D, A, c["grid_new"])), R.bits(want))
    # the goal cell's occupancy is not among the changes
    gx, gy = c["goal"]
    assert c["grid"][gy, gx] != 1 and c["grid_new"][gy, gx] != 1


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["diamond"]])
def test_constructions_fail_without_the_raise(solved, name):
    c = CASES[name]
    D, _, want = solved[name]
    assert not np.array_equal(R.bits(WR.relax_without_raise(D, c["grid_new"])), R.bits(want))


@pytest.mark.parametrize("name", list(CASES))
def test_construction_figures(solved, name):
    c = CASES[name]
    D, A, want = solved[name]
    S = WR.raised_set(D, A, c["grid_new"])
    free_raised = S & (c["grid_new"] != 1)
    assert WR.raised_count(D, A, c["grid_new"]) == int(free_raised.sum()) == c["raised"]
    # the set is closed, holds the seeds, and never the goal
    seeds = np.isfinite(D) & (c["grid_new"] == 1)
    assert (S[seeds]).all() and not S[c["goal"][1], c["goal"][0]]
    assert np.isfinite(D[S]).all()
    if "finite" in c:
        assert (int(np.isfinite(D).sum()), int(np.isfinite(want).sum())) == c["finite"]
    tiles = WR.tiles_of(free_raised, *TILE)
    if "tiles" in c:
        assert tiles == c["tiles"]
    if "ntiles" in c:
        assert len(tiles) == c["ntiles"]
    # every update is a rectangle on the grid and changes some occupancy
    H, W = c["grid"].shape
    g = c["grid"].copy()
    for x0, y0, p in c["updates"]:
        h, w = p.shape
        assert 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H
        assert ((g[y0:y0 + h, x0:x0 + w] == 1) != (p == 1)).any()
        g[y0:y0 + h, x0:x0 + w] = p
    assert np.array_equal(g, c["grid_new"])


def test_corner_handoff_leaves_through_one_diagonal(solved):
    c = CASES["corner"]
    D, A, want = solved["corner"]
    # every cell outside tile (0, 0) descends through (64, 32) -> (63, 31)
    assert A[32, 64] == 0
    assert np.isinf(want[32:, :]).all()
    assert np.isinf(want[:32, 65:]).all()
    # inside tile (0, 0) nothing but the seed changes
    keep = np.ones((32, 64), bool)
    keep[31, 63] = False
    assert np.array_equal(R.bits(D[:32, :64][keep]), R.bits(want[:32, :64][keep]))


def test_pending_host_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "path_pending_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe,
         os.path.join(ROOT, "tests", "path_pending_check.cpp")],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases hold" in run.stdout


def test_pending_capacity_is_named():
    text = open(os.path.join(CSRC, "pp2_path_pending.h")).read()
    m = re.search(r"constexpr int kPathPendingCap = (\d+);", text)
    assert m and int(m.group(1)) == 16
    text = open(os.path.join(CSRC, "pp2_path.h")).read()
    m = re.search(r"constexpr int kPathSeedRects = (\d+);", text)
    assert m and int(m.group(1)) == 16


def test_symbols_declared_exported_bound():
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % s, header, re.M), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert len(_lib.SIGNATURES["pp2_path_resolve"]) == 6
    assert len(_lib.SIGNATURES["pp2_path_resolve_info"]) == 6
    assert lib.pp2_abi_version() == 4 and _lib.PP2_ABI_VERSION == 4
    assert re.search(r"#define PP2_ABI_VERSION\s+4\b", header)
    from path_planning_2d_amd import GridContext
    assert callable(GridContext.path_resolve) and callable(GridContext.path_resolve_info)


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    w = ctypes.c_int(7)
    assert lib.pp2_path_resolve(None, 1, None, None, None, None) != 0
    assert lib.pp2_path_resolve(None, 1, None, None, None, ctypes.byref(w)) != 0
    assert lib.pp2_path_resolve_info(None, None, None, None, None, None) != 0
    assert lib.pp2_path_resolve_info(None, ctypes.byref(w), None, None, None, None) != 0
    assert w.value == 7


def test_astar_replan_demo_compiles(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    lib_dir = os.path.join(ROOT, "path_planning_2d_amd")
    if not os.path.exists(os.path.join(lib_dir, "libpp2_hip.so")):
        pytest.skip("library not built")
    exe = tmp_path / "demo"
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "include"), "-o", str(exe),
                    os.path.join(ROOT, "examples", "pp2_astar_replan_demo.c"),
                    "-L", lib_dir, "-lpp2_hip"], check=True)
    assert exe.exists()
