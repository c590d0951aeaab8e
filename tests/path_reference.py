"""NumPy reference of the shortest-path field (include/pp2.h "shortest-path
field"): D by heap Dijkstra and by whole-grid Jacobi relaxation, both with
np.float32 adds; ``check_fixpoint``, which verifies the defining equations
cell by cell without either solver; A_path by the definition's scan; the
trace; and the serpentine generator of the many-round cases.

Grids are uint8 [H, W] with 1 = occupied; goals are (gx, gy); cells are
y * W + x.  Move u in {0..8} \\ {4} displaces by (u % 3 - 1, u // 3 - 1).
"""
from __future__ import annotations

import heapq
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "tests", "golden", "maps")
GOLDEN = os.path.join(ROOT, "tests", "golden")

INF = np.float32(np.inf)
C_AXIS = np.float32(1.0)
C_DIAG = np.array([0x3FB504F3], np.uint32).view(np.float32)[0]  # fp32 sqrt 2
MOVES = [u for u in range(9) if u != 4]
# (u, dx, dy, cost) in the scan's order
OFF = [(u, u % 3 - 1, u // 3 - 1, C_DIAG if (u % 3 != 1 and u // 3 != 1) else C_AXIS)
       for u in MOVES]


def goal_ok(grid, goal) -> bool:
    H, W = grid.shape
    gx, gy = int(goal[0]), int(goal[1])
    return 0 <= gx < W and 0 <= gy < H and grid[gy, gx] != 1


def dijkstra(grid, goal) -> np.ndarray:
    H, W = grid.shape
    D = np.full((H, W), INF, np.float32)
    if not goal_ok(grid, goal):
        return D
    gx, gy = int(goal[0]), int(goal[1])
    D[gy, gx] = 0
    pq = [(0.0, gy, gx)]
    while pq:
        d, y, x = heapq.heappop(pq)
        if np.float32(d) != D[y, x]:
            continue
        for _, dx, dy, c in OFF:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and grid[yy, xx] != 1:
                nd = np.float32(D[y, x] + c)
                if nd < D[yy, xx]:
                    D[yy, xx] = nd
                    heapq.heappush(pq, (float(nd), yy, xx))
    return D


def _candidates(D):
    """cand[k][y, x] = fl32(D(x + off_u) + c_u) for the k-th move of the scan
    (+inf off the grid)."""
    H, W = D.shape
    P = np.full((H + 2, W + 2), INF, np.float32)
    P[1:-1, 1:-1] = D
    return [(P[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] + c).astype(np.float32)
            for _, dx, dy, c in OFF]


def relax_once(D, grid) -> np.ndarray:
    best = D.copy()
    for cand in _candidates(D):
        best = np.minimum(best, cand)
    best[grid == 1] = INF
    return best


def jacobi(grid, goal):
    """(D, sweeps): whole-grid relaxation from +inf until a sweep changes no bit."""
    H, W = grid.shape
    D = np.full((H, W), INF, np.float32)
    if goal_ok(grid, goal):
        D[int(goal[1]), int(goal[0])] = 0
    n = 0
    while True:
        N = relax_once(D, grid)
        n += 1
        if np.array_equal(N.view(np.uint32), D.view(np.uint32)):
            return D, n
        D = N


def check_fixpoint(D, grid, goal) -> None:
    """The defining equations, cell by cell (plain loops, no solver)."""
    H, W = grid.shape
    D = np.asarray(D, np.float32).reshape(H, W)
    ok = goal_ok(grid, goal)
    gx, gy = int(goal[0]), int(goal[1])
    for y in range(H):
        for x in range(W):
            bits = D[y, x].view(np.uint32)
            if grid[y, x] == 1:
                assert bits == 0x7F800000, (x, y, "occupied cells hold +inf")
                continue
            if ok and (x, y) == (gx, gy):
                assert bits == 0, (x, y, "the goal holds +0")
                continue
            best = INF
            for _, dx, dy, c in OFF:
                xx, yy = x + dx, y + dy
                if 0 <= xx < W and 0 <= yy < H and grid[yy, xx] != 1:
                    best = min(best, np.float32(D[yy, xx] + c))
            assert bits == np.float32(best).view(np.uint32), (x, y, float(D[y, x]), float(best))


def actions(D, grid, goal) -> np.ndarray:
    """A_path [H, W] uint8 by the definition's scan."""
    H, W = grid.shape
    D = np.asarray(D, np.float32).reshape(H, W)
    best = np.full((H, W), INF, np.float32)
    A = np.full((H, W), 4, np.uint8)
    for (u, _, _, _), cand in zip(OFF, _candidates(D)):
        take = cand < best
        best = np.where(take, cand, best)
        A[take] = u
    A[~np.isfinite(D)] = 4
    if goal_ok(grid, goal):
        A[int(goal[1]), int(goal[0])] = 4
    return A


def trace(A, D, start: int):
    """(cells, length): the walk of A_path from ``start``; no cells from a
    start with D = +inf."""
    H, W = A.shape
    A1, D1 = A.reshape(-1), np.asarray(D, np.float32).reshape(-1)
    if not np.isfinite(D1[start]):
        return np.zeros(0, np.int32), D1[start]
    cells = [int(start)]
    while A1[cells[-1]] != 4:
        u = int(A1[cells[-1]])
        cells.append(cells[-1] + (u // 3 - 1) * W + (u % 3 - 1))
        assert len(cells) <= H * W
    return np.array(cells, np.int32), D1[start]


def field(grid, goal):
    """(D, A_path) of the reference."""
    D = dijkstra(grid, goal)
    return D, actions(D, grid, goal)


def serpentine(H: int, W: int) -> np.ndarray:
    """Walls on the odd rows, one gap each, alternating between the last and
    the first column: one corridor through every even row."""
    g = np.zeros((H, W), np.uint8)
    for k, y in enumerate(range(1, H, 2)):
        g[y, :] = 1
        g[y, W - 1 if k % 2 == 0 else 0] = 0
    return g


def golden_case(name: str):
    """(grid, goal) of a golden map and the goal of its golden model."""
    grid = np.load(os.path.join(MAPS, f"{name}.npy"), allow_pickle=False)
    m = np.load(os.path.join(GOLDEN, f"model_{name}.npz"), allow_pickle=False)
    return grid, (int(m["goal"][0]), int(m["goal"][1]))


def freed(grid) -> np.ndarray:
    g = grid.copy()
    g[0, 0] = 0
    return g


def bits(D) -> np.ndarray:
    return np.ascontiguousarray(D, np.float32).view(np.uint32)
