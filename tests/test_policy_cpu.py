"""CPU: the policy evaluator's NumPy reference (tests/policy_reference.py)
checked on its own before the GPU tests rely on it -- the fmaf emulation
against libm bit for bit, the fp32 chain against the fp64 one within the
a priori rounding bound, the one-step identities -- and the new ABI.
"""
import ctypes
import re
from fractions import Fraction

import numpy as np
import pytest

import path_reference as PR
import policy_reference as R
from conftest import GAMMA
from oracle import oracle as O
from path_planning_2d_amd import _lib

F32 = np.float32


# ---------------------------------------------------------------- 1. fmaf
@pytest.fixture(scope="module")
def libm_fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float
    return np.frompyfunc(lambda a, b, c: libm.fmaf(float(a), float(b), float(c)), 3, 1)


def libm_ftz(fm, a, b, c):
    """libm's fmaf with flush-to-zero applied on both sides."""
    a, b, c = R.ftz(a), R.ftz(b), R.ftz(c)
    return R.ftz(fm(a, b, c).astype(np.float32))


def assert_same_bits(got, want, a, b, c):
    bad = np.flatnonzero(R.bits(got) != R.bits(want))
    assert bad.size == 0, (
        f"{bad.size} differ; first: fmaf({float(a[bad[0]]).hex()}, {float(b[bad[0]]).hex()}, "
        f"{float(c[bad[0]]).hex()}) = {float(got[bad[0]]).hex()}, libm {float(want[bad[0]]).hex()}")


def random_triples(n, seed):
    """Finite fp32 triples: random bit patterns with the exponents kept where
    neither the product nor the sum overflows, a third of them with c close
    to -a * b (cancellation) and a third with c far above the product (the
    product decides the rounding of c's last bit)."""
    rng = np.random.default_rng(seed)

    def rnd(lo, hi):
        sign = rng.integers(0, 2, n, dtype=np.uint32) << 31
        expo = rng.integers(lo + 127, hi + 127, n, dtype=np.uint32) << 23
        return (sign | expo | rng.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)

    a, b, c = rnd(-30, 30), rnd(-30, 30), rnd(-60, 60)
    k = n // 3
    prod = (a.astype(np.float64) * b).astype(np.float32)
    ulps = rng.integers(-4, 5, k).astype(np.int32)
    c[:k] = -((prod[:k].view(np.int32) + ulps).view(np.float32))
    c[k:2 * k] = prod[k:2 * k] * F32(2.0) ** rng.integers(20, 28, k).astype(np.float32)
    return a, b, c


def test_fmaf_matches_libm_on_random_triples(libm_fmaf):
    a, b, c = random_triples(120000, 7)
    assert a.size >= 100000
    got = R.fmaf_ieee(a, b, c)
    want = libm_fmaf(a, b, c).astype(np.float32)
    assert_same_bits(got, want, a, b, c)
    assert_same_bits(R.fmaf_ftz(a, b, c), libm_ftz(libm_fmaf, a, b, c), a, b, c)


def tie_triples():
    """c = +-X (1 + k 2^-23) and a * b = +-X 2^-24 (1 - 2^-46): the exact sum
    lies 2^-70 X off the midpoint of two fp32 neighbours, too little for fp64
    to keep, so fl64(a * b + c) IS the midpoint."""
    a, b, c = [], [], []
    for e in (-20, -3, 0, 5, 40):
        X = F32(2.0) ** F32(e)
        for k in range(8):
            for sp in (1, -1):
                for sc in (1, -1):
                    a.append(F32(1) + F32(2.0) ** F32(-23))
                    b.append(F32(sp) * (F32(1) - F32(2.0) ** F32(-23)) * X * F32(2.0) ** F32(-24))
                    c.append(F32(sc) * X * (F32(1) + F32(k) * F32(2.0) ** F32(-23)))
    return np.array(a, F32), np.array(b, F32), np.array(c, F32)


def test_fmaf_matches_libm_on_fp32_ties(libm_fmaf):
    a, b, c = tie_triples()
    # the construction does what it says, in exact arithmetic
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        s = float(a[i]) * float(b[i]) + float(c[i])
        assert Fraction(s) != exact
        lo = np.float32(s)
        other = np.nextafter(lo, F32(np.inf) if float(lo) < s else F32(-np.inf))
        if float(lo) != s:  # s between two fp32 values: exactly half way
            assert Fraction(s) * 2 == Fraction(float(lo)) + Fraction(float(other))
    want = libm_fmaf(a, b, c).astype(np.float32)
    assert_same_bits(R.fmaf_ieee(a, b, c), want, a, b, c)
    # ... and bites: rounding fl64(a * b + c) to fp32 gets some of them wrong
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (R.bits(naive) != R.bits(want)).sum() >= a.size // 8


def test_fmaf_flushes_subnormals_like_libm_with_ftz(libm_fmaf):
    sub = np.array([1, 0x7FFFFF, 0x400000], np.uint32).view(np.float32)  # subnormal operands
    a = np.array([2.0 ** -100, 2.0 ** -100, sub[0], 3.0, sub[1], 1.5, -(2.0 ** -70), 1.0, 2.0 ** -126],
                 F32)
    b = np.array([2.0 ** -30, 2.0 ** -26, 2.0 ** 100, sub[2], 2.0, 2.0 ** -126, 2.0 ** -60, 2.0 ** -126,
                  0.75], F32)
    c = np.array([0.0, 0.0, 1.0, 2.0 ** -120, sub[0], -(2.0 ** -126), 0.0, -sub[1], 2.0 ** -127], F32)
    got = R.fmaf_ftz(a, b, c)
    assert_same_bits(got, libm_ftz(libm_fmaf, a, b, c), a, b, c)
    assert R.bits(got)[0] == 0 and got[2] == 1.0           # result / operand flushed
    assert R.bits(got)[6] == 0x80000000                    # a flushed result keeps its sign
    # random triples down in the flush range
    rng = np.random.default_rng(3)
    n = 20000
    def rnd():
        return ((rng.integers(0, 2, n, dtype=np.uint32) << 31) |
                (rng.integers(0, 8, n, dtype=np.uint32) << 23) |
                rng.integers(0, 1 << 23, n, dtype=np.uint32)).view(np.float32)
    a, c = rnd(), rnd()
    b = (rng.random(n) * 4 - 2).astype(np.float32)
    assert_same_bits(R.fmaf_ftz(a, b, c), libm_ftz(libm_fmaf, a, b, c), a, b, c)


# ---------------------------------------------------------------- 2. fp32 chain vs fp64 chain
def tables(grid, goal, T, C):
    H, W = grid.shape
    _, A, _, _ = O.mdp_solve(H, W, GAMMA, T, C)
    _, Apath = PR.field(grid, goal)
    return {"mdp": A.reshape(H, W), "path": Apath}


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
    got = R.evaluate(T, C, pi, GAMMA, goal, H, W, Hn)
    want = R.chain_f64(T, C, pi, GAMMA, goal, H, W, Hn)
    for g, w, what in zip(got, want, "GPN"):
        bound = Hn * 10 * 2.0 ** -24 * np.abs(w) + Hn * 10 * 2.0 ** -126
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= bound).all(), f"{what}: worst err/bound {np.max(err / bound):.3f}"
    assert got[1].max() == 1.0 and got[2].max() > 1.0  # the goal is there and steps are counted


# ---------------------------------------------------------------- 3. one step
def test_one_step_identities():
    grid, goal = PR.golden_case("map_10x10")
    H, W = grid.shape
    T, C = O.model_mdp(grid, goal)
    pi = tables(grid, goal, T, C)["mdp"]
    G, P, N = R.evaluate(T, C, pi, GAMMA, goal, H, W, 1)
    gcell = goal[1] * W + goal[0]
    off = np.arange(H * W) != gcell
    u = pi.reshape(-1)
    np.testing.assert_array_equal(R.bits(G).reshape(-1)[off], R.bits(C[np.arange(H * W), u])[off])
    assert G.reshape(-1)[gcell] == 0 and N.reshape(-1)[gcell] == 0 and P.reshape(-1)[gcell] == 1
    np.testing.assert_array_equal(N.reshape(-1)[off], 1.0)
    want = np.zeros(H * W, F32)
    for cell in np.flatnonzero(off):
        dx, dy = goal[0] - cell % W, goal[1] - cell // W
        if abs(dx) <= 1 and abs(dy) <= 1:
            want[cell] = T[cell, u[cell], (dy + 1) * 3 + dx + 1]
    want[gcell] = 1.0
    np.testing.assert_array_equal(R.bits(P).reshape(-1), R.bits(want))
    assert (want[off] > 0).any()


# ---------------------------------------------------------------- 4. ABI
POLICY_SYMBOLS = ("pp2_policy_set_table", "pp2_policy_evaluate", "pp2_policy_get",
                  "pp2_policy_info")


def test_policy_abi():
    text = open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    for s in POLICY_SYMBOLS:
        assert re.search(rf"^int {s}\s*\(", text, re.M), f"{s} not in pp2.h"
        assert s in _lib.SIGNATURES, f"{s} not in _lib.py"
        assert hasattr(lib, s), f"{s} not exported"
    assert len(_lib.SIGNATURES["pp2_policy_evaluate"]) == 6
    assert len(_lib.SIGNATURES["pp2_policy_info"]) == 11
    assert re.search(r"#define PP2_ABI_VERSION 4\b", text) and lib.pp2_abi_version() == 4
    assert re.search(r"#define PP2_TABLE_USER 2\b", text)
    for name, v in (("AUTO", 0), ("PLANES", 1), ("TILES", 2)):
        assert re.search(rf"#define PP2_POLICY_{name}\s+{v}\b", text)
