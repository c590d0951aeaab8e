"""Seeded inputs shared by the tests that pin the oracle (test_ref_pin_cpu.py)
and the device kernels (test_gpu_ref_pin.py) to the reference's own kernels
built for the host (oracle/ref.py).  Everything here is a pure function of
(H, W): both modules see the same grids, beliefs and alphas.
"""
import numpy as np

# H x W.  One cell, one row, one column, the smallest grid with an interior
# cell, and two sizes that are no multiple of any block or tile.
CPU_SHAPES = [(1, 1), (1, 7), (5, 1), (3, 3), (33, 65), (40, 100)]
# The device kernels' edges: widths one below, at and one above the 256-lane
# block span at one cell per lane (255, 256, 257) and at four (1023, 1024,
# 1025); with rows padded to a multiple of 4 the same widths sit one below,
# at and one above a padded row width.
GPU_SHAPES = [(1, 1), (1, 7), (5, 1), (3, 3), (33, 65),
              (2, 255), (2, 256), (3, 257), (2, 1023), (2, 1024), (3, 1025)]


def shape_id(hw):
    return f"{hw[0]}x{hw[1]}"


def goals(H, W):
    """(gx, gy): the far corner and an interior cell (the same cell on a grid
    too small to have both)."""
    return [(W - 1, H - 1), (W // 2, H // 2)]


def grid(H, W):
    """About 25 % occupied, both goal cells free."""
    rng = np.random.default_rng(1000 * H + W)
    g = (rng.random((H, W)) < 0.25).astype(np.uint8)
    for gx, gy in goals(H, W):
        g[gy, gx] = 0
    return g


def belief(g, seed=0):
    """A seeded belief supported on the free cells, summing to 1."""
    rng = np.random.default_rng(7 + seed + 31 * g.size)
    b = rng.random(g.size) * (g.reshape(-1) == 0)
    return (b / b.sum()).astype(np.float32)


def fib_alphas(H, W):
    """Seeded alphas [hw, 9] of mixed sign."""
    rng = np.random.default_rng(11 + 17 * H + W)
    return rng.uniform(-20.0, 20.0, (H * W, 9)).astype(np.float32)


def pbvi_alphas(H, W, S=5):
    """Seeded PBVI alpha vectors [S, hw] of mixed sign."""
    rng = np.random.default_rng(13 + 19 * H + W)
    return rng.uniform(-20.0, 20.0, (S, H * W)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
