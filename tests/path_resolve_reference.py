"""NumPy reference of the shortest-path field's warm re-solve
(pp2_path_resolve; DESIGN.md §2.3 "Warm re-solve"), on top of
tests/path_reference.py: the raised set of an old field under a new map, the
re-solve itself (raise, then whole-grid relaxation from that state), the same
relaxation without the raise (what the raise is there to prevent), and the
constructions the CPU and GPU tests share.

(D, A) is a converged field of an earlier map and the same goal; grid_new is
the map now, uint8 [H, W] with 1 = occupied.
"""
from __future__ import annotations

import numpy as np

import path_reference as R


def raised_set(D, A, grid_new) -> np.ndarray:
    """bool [H, W]: the least set that holds the seeds (cells with finite D
    that are occupied now) and every free finite non-goal cell whose old parent
    x + off[A(x)] is in it.  The seeds are part of the set; ``raised_count``
    leaves them out."""
    H, W = D.shape
    fin = np.isfinite(D)
    S = fin & (grid_new == 1)
    if not S.any():
        return S
    A1 = A.reshape(-1).astype(np.int64)
    cells = np.arange(H * W, dtype=np.int64)
    parent = cells + (A1 // 3 - 1) * W + (A1 % 3 - 1)
    child = (fin & (grid_new != 1) & (A != 4)).reshape(-1)   # (A == 4: the goal)
    S1 = S.reshape(-1).copy()
    while True:
        new = child & ~S1 & S1[parent]
        if not new.any():
            return S1.reshape(H, W)
        S1 |= new


def raised_count(D, A, grid_new) -> int:
    """What pp2_path_resolve_info reports: raised cells that are still free."""
    return int((raised_set(D, A, grid_new) & (grid_new != 1)).sum())


def relax_to_quiet(D, grid) -> np.ndarray:
    while True:
        N = R.relax_once(D, grid)
        if np.array_equal(R.bits(N), R.bits(D)):
            return D
        D = N


def warm_resolve(D, A, grid_new) -> np.ndarray:
    """Raise, then whole-grid relaxation from that state."""
    D1 = D.copy()
    D1[raised_set(D, A, grid_new)] = R.INF
    return relax_to_quiet(D1, grid_new)


def relax_without_raise(D, grid_new) -> np.ndarray:
    """The wrong method: newly occupied cells to +inf, then relaxation alone."""
    D1 = D.copy()
    D1[grid_new == 1] = R.INF
    return relax_to_quiet(D1, grid_new)


def tiles_of(mask, tr, tc):
    """The (tile row, tile column) pairs that own a cell of ``mask``."""
    ys, xs = np.nonzero(mask)
    return sorted(set(zip((ys // tr).tolist(), (xs // tc).tolist())))


def synth(H, W, seed):
    from path_planning_2d_amd import synthetic as S
    return R.freed(S.synth_grid(H, W, seed))


# ---------------------------------------------------------------- constructions
# Each: dict(grid, goal, updates=[(x0, y0, patch), ...] in map_update's
# arguments, grid_new, raised, and what else the issue quotes).  The figures
# assume the 32 x 64 tile.
def _apply(grid, updates):
    g = grid.copy()
    for x0, y0, p in updates:
        g[y0:y0 + p.shape[0], x0:x0 + p.shape[1]] = p
    return g


def _case(grid, goal, updates, **kw):
    updates = [(int(x0), int(y0), np.ascontiguousarray(p, np.uint8)) for x0, y0, p in updates]
    return dict(grid=grid, goal=goal, updates=updates, grid_new=_apply(grid, updates), **kw)


def _window(grid, x0, y0, x1, y1, edit):
    """One update of the inclusive window: its cells of ``grid`` after edit(g)."""
    g = grid.copy()
    edit(g)
    return (x0, y0, g[y0:y1 + 1, x0:x1 + 1])


def corner_grid():
    g = np.zeros((65, 127), np.uint8)
    g[32, :64] = 1
    g[:32, 64] = 1
    return g


def corner_handoff(free_too=False):
    """Tile (0, 0) reaches the rest only through (63, 31) -> (64, 32)."""
    g = corner_grid()
    if not free_too:
        return _case(g, (0, 0), [(63, 31, np.array([[1]]))], raised=6111, finite=(8159, 2047),
                     tiles=[(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], diamond=True)

    def edit(n):
        n[31, 63] = 1
        n[32, 0] = 0      # the wall cell (x, y) = (0, 32): another way round
    return _case(g, (0, 0), [_window(g, 0, 31, 63, 32, edit)],
                 raised=6111, finite=(8159, 8159), diamond=True)


def corner_handoff_raised():
    """The hand-off again, with the corner cell (63, 31) not a seed but a
    raised cell: walls at (62, 31) and (63, 30) leave it the one parent
    (62, 30), which the update occupies.  The seed is seen by tile (0, 0)
    alone, so the raise reaches tile (1, 1) only if the raise round itself
    marks the corner tile."""
    g = corner_grid()
    g[31, 62] = 1
    g[30, 63] = 1
    return _case(g, (0, 0), [(62, 30, np.array([[1]]))], raised=6112, finite=(8157, 2044),
                 tiles=[(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], diamond=True)


def bars_next_to_the_goal():
    g = np.zeros((65, 127), np.uint8)
    gx, gy = 32, 48
    return _case(g, (gx, gy),
                 [(gx + 2, gy - 2, np.ones((5, 1))), (gx - 2, gy - 3, np.ones((1, 5)))],
                 raised=6336, ntiles=6, diamond=True)


def single_tile(k):
    H, W = [(31, 65), (32, 64), (33, 63)][k]
    g = synth(H, W, 11 + k)
    # 3 rows x 2 columns, centred on the middle row, from the column at W / 3
    return _case(g, (0, 0), [(W // 3, H // 2 - 1, np.ones((3, 2)))], raised=[63, 147, 4][k],
                 diamond=True)


def corridor(which):
    g = R.serpentine(65, 70)
    if which == "a":
        return _case(g, (0, 0), [(3, 0, np.array([[1]]))], raised=2338, finite=(2342, 3),
                     diamond=True)

    def edit(n):
        n[1, 69] = 1
        n[1, 0] = 0
    return _case(g, (0, 0), [_window(g, 0, 1, 69, 1, edit)], raised=2271, finite=(2342, 2342),
                 diamond=False)


def freed_only():
    g = synth(97, 131, 5)
    return _case(g, (0, 0), [(60, 40, np.zeros((10, 10)))], raised=0, finite=(10176, 10200),
                 diamond=False)


def mixed_97x131():
    g = synth(97, 131, 5)

    def edit(n):
        n[30:36, 62:66] = 1
        n[31:34, 128:131] = 1
        n[60:70, 10:12] = 0
    return _case(g, (0, 0), [_window(g, 10, 30, 130, 69, edit)], raised=1479, ntiles=5,
                 diamond=True)


def constructions():
    yield "corner", corner_handoff()
    yield "corner_and_freed", corner_handoff(True)
    yield "corner_raised", corner_handoff_raised()
    yield "bars", bars_next_to_the_goal()
    for k in range(3):
        yield f"single_tile_{k}", single_tile(k)
    yield "corridor_a", corridor("a")
    yield "corridor_b", corridor("b")
    yield "freed_only", freed_only()
    yield "mixed", mixed_97x131()
