"""CPU: the forward occupancy's NumPy reference (tests/occupancy_reference.py)
checked on its own before the GPU tests rely on it -- the fp32 chain against
the fp64 one within the a priori rounding bound, the adjoint identity against
the policy evaluator's fp64 chain, the one-step identity -- and the new ABI.
"""
import re

import numpy as np
import pytest

import occupancy_reference as R
import path_reference as PR
import policy_reference as PolR
from conftest import GAMMA
from oracle import oracle as O
from path_planning_2d_amd import _lib

F32 = np.float32


def tables(grid, goal, T, C):
    H, W = grid.shape
    _, A, _, _ = O.mdp_solve(H, W, GAMMA, T, C)
    _, Apath = PR.field(grid, goal)
    return {"mdp": A.reshape(H, W), "path": Apath}


def uniform_free(grid):
    free = grid == 0
    return (free / F32(free.sum())).astype(np.float32)


# ---------------------------------------------------------------- 1. fp32 chain vs fp64 chain
@pytest.mark.parametrize("name", ["map_5x5", "map_10x10"])
@pytest.mark.parametrize("table", ["mdp", "path"])
def test_reference_within_the_forward_bound_of_the_f64_chain(name, table):
    """H steps of at most ten roundings each on non-negative terms: the fp32
    result is within H * 10 * 2^-24 * |value| of the fp64 chain, plus
    H * 10 flushes of at most 2^-126."""
    Hn = 32
    grid, goal = PR.golden_case(name)
    H, W = grid.shape
    T, C = O.model_mdp(grid, goal)
    pi = tables(grid, goal, T, C)[table]
    b0 = uniform_free(grid)
    got = R.evaluate(T, pi, goal, b0, H, W, Hn)
    want = R.chain_f64(T, pi, goal, b0, H, W, Hn)
    for g, w, what in zip(got, want, ("D", "V", "curve")):
        bound = Hn * 10 * 2.0 ** -24 * np.abs(w) + Hn * 10 * 2.0 ** -126
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= bound).all(), f"{what}: worst err/bound {np.max(err / bound):.3f}"
    assert got[2][-1] > 0 and got[1].max() > 0  # mass arrives and visits are counted


# ---------------------------------------------------------------- 2. the adjoint identity
@pytest.mark.parametrize("name", ["map_5x5", "map_10x10", "sparse_map_100x40"])
def test_adjoint_identity_in_f64(name):
    """<b0, P_H> is the mass at the goal after H steps and <b0, N_H> the total
    of the visit field, against the policy evaluator's fp64 chain."""
    Hn = 40
    grid, goal = PR.golden_case(name)
    H, W = grid.shape
    T, C = O.model_mdp(grid, goal)
    pi = tables(grid, goal, T, C)["mdp"]
    b0 = uniform_free(grid)
    _, V, curve = R.chain_f64(T, pi, goal, b0, H, W, Hn)
    _, P, N = PolR.chain_f64(T, C, pi, GAMMA, goal, H, W, Hn)
    b = b0.astype(np.float64)
    bp, bn = float((b * P).sum()), float((b * N).sum())
    print(f"{name}: <b0,P> {bp!r} curve[H] {curve[Hn]!r}; <b0,N> {bn!r} sum V {V.sum()!r}")
    assert bp > 0 and bn > 0
    assert abs(curve[Hn] - bp) <= 1e-12 * bp
    assert abs(V.sum() - bn) <= 1e-12 * bn
    assert (np.diff(curve) >= 0).all(), "the arrival curve never falls"


# ---------------------------------------------------------------- 3. one step
def test_one_step_identity():
    """A one-hot b0 at a cell off the goal: D_1 is that cell's T row for its
    action, scattered to its neighbours, in bits; V_1 is b0."""
    grid, goal = PR.golden_case("map_10x10")
    H, W = grid.shape
    T, C = O.model_mdp(grid, goal)
    pi = tables(grid, goal, T, C)["mdp"]
    gcell = goal[1] * W + goal[0]
    free = [c for c in np.flatnonzero(grid.reshape(-1) == 0) if c != gcell]
    spread = 0
    for cell in (free[0], free[len(free) // 2], free[-1], gcell - 1):
        assert cell != gcell
        b0 = np.zeros(H * W, F32)
        b0[cell] = 1.0
        D, V, curve = R.evaluate(T, pi, goal, b0, H, W, 1)
        want = np.zeros((H, W), F32)
        y, x = divmod(int(cell), W)
        for i in range(9):
            yy, xx = y + i // 3 - 1, x + i % 3 - 1
            if 0 <= yy < H and 0 <= xx < W:
                want[yy, xx] = T[cell, pi.reshape(-1)[cell], i]
        np.testing.assert_array_equal(R.bits(D), R.bits(want))
        np.testing.assert_array_equal(R.bits(V).reshape(-1), R.bits(b0))
        assert R.bits(curve)[0] == 0 and R.bits(curve)[1] == R.bits(want[goal[1], goal[0]])
        spread += int((want > 0).sum() > 1)
    assert spread, "some row spreads over more than one neighbour"


# ---------------------------------------------------------------- 4. ABI
OCC_SYMBOLS = ("pp2_occupancy_evaluate", "pp2_occupancy_get", "pp2_occupancy_info")


def test_occupancy_abi():
    text = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    for s in OCC_SYMBOLS:
        assert re.search(rf"^int {s}\s*\(", text, re.M), f"{s} not in pp2.h"
        assert s in _lib.SIGNATURES, f"{s} not in _lib.py"
        assert hasattr(lib, s), f"{s} not exported"
    assert len(_lib.SIGNATURES["pp2_occupancy_evaluate"]) == 7
    assert len(_lib.SIGNATURES["pp2_occupancy_get"]) == 4
    assert len(_lib.SIGNATURES["pp2_occupancy_info"]) == 11
    assert re.search(r"#define PP2_ABI_VERSION 4\b", text) and lib.pp2_abi_version() == 4
    for name, v in (("AUTO", 0), ("PLANES", 1), ("TILES", 2)):
        assert re.search(rf"#define PP2_OCC_{name}\s+{v}\b", text)
