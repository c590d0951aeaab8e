"""The cases of tests/test_gpu_rollout_exact.py and their exact emulation.

Shared by the GPU module (which runs every case on the device) and by
tests/test_oracle.py (which asserts, on the emulated planes alone, that every
case contains what it is meant to exercise).  A case is a grid, a model, and
per root belief a batch of (u, z) sequences; ``emulate`` chains
``oracle.rollout_chain_f16`` over every copy once and caches the result."""
import functools
from collections import namedtuple

import numpy as np

from conftest import GAMMA  # noqa: F401  (re-exported for the GPU module)

# model: "gen" (generated: sparse-coded), "offsupport" (one T entry outside its
# action's support: full-coded) or "overflow" (every cell distinct: the
# dictionary overflows, automatic dense).  batch: "random", "same" (every copy
# takes action 7) or "nine" (copy c takes action c at every step).
Case = namedtuple("Case", "H W copies depth model batch roots seed")

GEOMS = [(1, 9), (2, 16), (3, 300), (5, 264), (70, 260), (33, 64), (64, 256), (35, 512),
         (37, 50)]
# trajectory seed per geometry: 7, but 28 on 1 x 9, where seed 7 leaves only 8 %
# of the positive stored cells fp16-subnormal (the CPU sensitivity test in
# test_oracle.py asks for 10 %; seed 28 gives 16 %)
SEEDS = {g: 28 if g == (1, 9) else 7 for g in GEOMS}
OFF_ACTION = 4  # the stay action reads the off-support entry T[cell][4][0]


def geom_case(H, W):
    return Case(H, W, 13, 3, "gen", "random", "all", SEEDS[(H, W)])


def extra_cases():
    out = {}
    for n in (1, 2, 3, 5):
        out[f"33x64-copies{n}"] = Case(33, 64, n, 3, "gen", "random", "uniform", 7)
    out["33x64-same-action"] = Case(33, 64, 13, 3, "gen", "same", "uniform", 7)
    out["33x64-nine-actions"] = Case(33, 64, 9, 3, "gen", "nine", "uniform", 7)
    out["33x64-depth1"] = Case(33, 64, 13, 1, "gen", "random", "uniform", 7)
    out["33x64-depth2"] = Case(33, 64, 13, 2, "gen", "random", "uniform", 7)
    return out


def model_cases():
    return {f"{H}x{W}-{m}": Case(H, W, 13, 3, m, "random", "uniform", 7)
            for H, W in ((37, 50), (5, 264)) for m in ("offsupport", "overflow")}


GEOM_CASES = {f"{H}x{W}": geom_case(H, W) for H, W in GEOMS}
EXTRA_CASES = extra_cases()
MODEL_CASES = model_cases()
ALL_CASES = {**GEOM_CASES, **EXTRA_CASES, **MODEL_CASES}


def hot_cells(H, W):
    """(name, y, x) of the one-hot roots: the grid's first and last cell (halo
    rows, the row's last dword) and, with two segments, both sides of the
    segment boundary in a middle row (the segment-edge dwords)."""
    out = [("hot-first", 0, 0), ("hot-last", H - 1, W - 1)]
    if W > 256:
        out += [("hot-col255", H // 2, 255), ("hot-col256", H // 2, 256)]
    return out


def off_cell(H, W):
    return (H // 2) * W + W // 2  # the cell whose T row gets the off-support entry


@functools.lru_cache(maxsize=None)
def grid_of(H, W):
    """Synthetic 20 %-occupied grid with the one-hot cells, the off-support
    cell and their 3 x 3 neighbourhoods free."""
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(H, W, seed=1000 * H + W)
    oc = off_cell(H, W)
    for _, y, x in hot_cells(H, W) + [("off", oc // W, oc % W)]:
        grid[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0
    grid.setflags(write=False)
    return grid


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict: grid, goal, T, L, R, Cc (reference layouts), alphas [cells][9] for
    the leaf bound, and runs: [(root name, b0, us, zs)] with us, zs
    [depth][copies]."""
    from oracle import oracle as O
    from path_planning_2d_amd import synthetic as S
    H, W = case.H, case.W
    grid = grid_of(H, W)
    goal = S.synth_goal(grid)
    T, L, R = O.model_pomdp(grid, goal)
    _, Cc = O.model_mdp(grid, goal)
    if case.model == "offsupport":
        T = T.copy()
        T[off_cell(H, W), OFF_ACTION, 0] = np.float32(0.25)  # stay: support is {4} only
    elif case.model == "overflow":
        rng = np.random.default_rng(0)
        T = (T * (1.0 + 1e-3 * rng.random(T.shape))).astype(np.float32)
    rng = np.random.default_rng(H * W)
    alphas = (-20.0 * (0.5 + rng.random((H * W, 9)))).astype(np.float32)
    roots = [("uniform", S.uniform_belief(grid))]
    if case.roots == "all":
        for name, y, x in hot_cells(H, W):
            b = np.zeros(H * W, np.float32)
            b[y * W + x] = 1.0
            roots.append((name, b))
    runs = []
    for i, (name, b0) in enumerate(roots):
        us, zs = S.rollout_trajectories(grid, b0, case.copies, case.depth, seed=case.seed + i)
        if case.batch == "same":
            us[:] = 7
        elif case.batch == "nine":
            us[:] = np.arange(9, dtype=np.uint8)[None, :]
        elif case.model == "offsupport":
            us[:, ::2] = OFF_ACTION
        runs.append((name, b0, us, zs))
    return {"grid": grid, "goal": goal, "T": T, "L": L, "R": R, "Cc": Cc, "alphas": alphas,
            "runs": runs}


@functools.lru_cache(maxsize=None)
def emulate(case):
    """{root name: [rollout_chain_f16 result of copy c, plus "leaf_upper"]}."""
    from oracle import oracle as O
    inp = inputs(case)
    a64 = inp["alphas"].astype(np.float64)
    out = {}
    for name, b0, us, zs in inp["runs"]:
        per_copy = []
        for c in range(case.copies):
            e = O.rollout_chain_f16(case.H, case.W, inp["T"], inp["L"], inp["R"], b0,
                                    us[:, c], zs[:, c])
            h = e["plane"].astype(np.float64)
            e["leaf_upper"] = float(((h @ a64) / h.sum()).max())
            per_copy.append(e)
        out[name] = per_copy
    return out


F16_MIN_NORMAL = 2.0 ** -14


def stored_planes(case, root=None):
    """Every emulated stored plane of the case (all copies, all steps) as
    float32 [n][H][W]; only the runs from ``root`` if given."""
    em = emulate(case)
    return np.array([p.astype(np.float32).reshape(case.H, case.W)
                     for name, copies in em.items() if root in (None, name)
                     for e in copies for p in e["planes"]])
