"""Cases of the device-memory belief placement (a helper module like
episodes_reference.py, not a test): ``large_case()``, the one definition of the
smallest kind of grid the LDS placement refuses, which both
tests/test_episodes_global_cpu.py and tests/test_gpu_episodes_global.py use,
and ``pick_starts()``, the seven starts of such a grid.
"""
from __future__ import annotations

import numpy as np

LARGE_SHAPE = (130, 140, 7)   # H, W, synth_grid's seed
LARGE_GOAL = (0, 0)
LARGE_GAMMA = 0.95
LARGE_HORIZON = 10
LARGE_SEED = 77


def pick_starts(grid) -> np.ndarray:
    """7 starts of a grid whose goal is cell 0: the goal; the first four free
    cells with max(x, y) <= 3 other than cell 0; free[len(free) // 2]; the last
    cell if it is free, else the last free cell."""
    H, W = grid.shape
    flat = grid.reshape(-1)
    free = np.flatnonzero(flat == 0)
    near = [int(c) for c in free if c != 0 and max(c % W, c // W) <= 3][:4]
    assert len(near) == 4, "fewer than four free cells next to the goal"
    last = H * W - 1 if flat[H * W - 1] == 0 else int(free[-1])
    return np.array([0] + near + [int(free[len(free) // 2]), last], np.int32)


def large_case() -> dict:
    """synth_grid(130, 140, 7) with cell (0, 0) freed, goal (0, 0), gamma 0.95,
    uniform b0, horizon 10, seed 77 and ``pick_starts``' 7 starts: about 198 KB
    of LDS per episode against the 160 KiB a workgroup may have."""
    from path_planning_2d_amd import synthetic as S
    H, W, seed = LARGE_SHAPE
    grid = S.synth_grid(H, W, seed)
    grid[0, 0] = 0
    return {"grid": grid, "goal": LARGE_GOAL, "gamma": LARGE_GAMMA,
            "b0": S.uniform_belief(grid), "starts": pick_starts(grid), "seed": LARGE_SEED,
            "horizon": LARGE_HORIZON}
