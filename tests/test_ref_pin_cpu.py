"""The CPU oracle against the reference's own kernels built for the host.

oracle/pp2_oracle*.c restate the reference's CUDA kernels by hand; every GPU
parity test, the golden fixtures and smoke() rest on that restatement.  Here
it is compared, bit for bit, with the kernels' own text compiled for the host
with a*b+c contracted to fma (oracle/ref.py, variant "fma": the reference's
nvcc --use_fast_math arithmetic), and the committed fixtures are recomputed
from that library alone.  A second build without contraction ("nofma") must
differ, or the first proved nothing about where the fmas sit.

All comparisons are bit equality.  The module skips only where the libraries
under oracle/_ref/ were not built.
"""
import numpy as np
import pytest

from conftest import GAMMA, golden, golden_map
from oracle import ref as REF
from ref_pin_cases import (CPU_SHAPES, belief, bits, fib_alphas, goals, grid, pbvi_alphas,
                           shape_id)

pytestmark = pytest.mark.skipif(not REF.available(),
                                reason="oracle/_ref libraries are not built")

FLT_MIN = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def models(oracle):
    """(H, W, goal index) -> the reference library's T, L, R, C, made once."""
    cache = {}

    def get(H, W, k=0):
        if (H, W, k) not in cache:
            g = grid(H, W)
            T, L, R = REF.model_pomdp(g, goals(H, W)[k])
            Tm, C = REF.model_mdp(g, goals(H, W)[k])
            for a in (T, L, R, Tm, C):
                a.setflags(write=False)
            cache[(H, W, k)] = (g, T, L, R, Tm, C)
        return cache[(H, W, k)]
    return get


@pytest.mark.parametrize("k", [0, 1], ids=["corner", "interior"])
@pytest.mark.parametrize("hw", CPU_SHAPES, ids=shape_id)
def test_model_tensors(oracle, models, hw, k):
    H, W = hw
    g, T, L, R, Tm, C = models(H, W, k)
    To, Lo, Ro = oracle.model_pomdp(g, goals(H, W)[k])
    Tmo, Co = oracle.model_mdp(g, goals(H, W)[k])
    np.testing.assert_array_equal(To, T)
    np.testing.assert_array_equal(Lo, L)
    np.testing.assert_array_equal(Ro, R)
    np.testing.assert_array_equal(Tmo, Tm)
    np.testing.assert_array_equal(Co, C)


@pytest.mark.parametrize("k", [0, 1], ids=["corner", "interior"])
@pytest.mark.parametrize("hw", CPU_SHAPES, ids=shape_id)
def test_bellman_sweeps(oracle, models, hw, k):
    H, W = hw
    _, _, _, _, Tm, C = models(H, W, k)
    J = Jo = np.zeros(H * W, np.float32)
    for s in range(12):
        J, A = REF.mdp_sweep(H, W, GAMMA, Tm, C, J)
        Jo, Ao = oracle.mdp_sweep(H, W, GAMMA, Tm, C, Jo)
        np.testing.assert_array_equal(bits(Jo), bits(J), err_msg=f"J, sweep {s + 1}")
        np.testing.assert_array_equal(Ao, A, err_msg=f"A, sweep {s + 1}")


@pytest.mark.parametrize("hw", CPU_SHAPES, ids=shape_id)
def test_belief_update_all_pairs(oracle, models, hw):
    H, W = hw
    g, T, L = models(H, W)[:3]
    b = belief(g)
    for u in range(9):
        for z in range(16):
            want = REF.belief_update(H, W, T, L, b, u, z)
            got = oracle.belief_update(H, W, T, L, b, u, z)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"u={u} z={z}")


@pytest.mark.parametrize("hw", CPU_SHAPES, ids=shape_id)
def test_fib_sweeps(oracle, models, hw):
    H, W = hw
    _, T, L, R = models(H, W)[:4]
    a = ao = np.zeros((H * W, 9), np.float32)
    for s in range(4):
        a = REF.fib_sweep(H, W, GAMMA, T, L, R, a)
        ao = oracle.fib_sweep(H, W, GAMMA, T, L, R, ao)
        np.testing.assert_array_equal(bits(ao), bits(a), err_msg=f"sweep {s + 1}")
    a0 = fib_alphas(H, W)
    assert (a0 > 0).any() and (a0 < 0).any()
    np.testing.assert_array_equal(bits(oracle.fib_sweep(H, W, GAMMA, T, L, R, a0)),
                                  bits(REF.fib_sweep(H, W, GAMMA, T, L, R, a0)))


@pytest.mark.parametrize("hw", [(3, 3), (33, 65)], ids=shape_id)
def test_gamma_ao_all_pairs(oracle, models, hw):
    H, W = hw
    _, T, L = models(H, W)[:3]
    al = pbvi_alphas(H, W, 5)
    for a in range(9):
        for o in range(16):
            want = REF.pbvi_gamma_ao(H, W, GAMMA, T, L, a, o, al)
            got = oracle.pbvi_gamma_ao(H, W, GAMMA, T, L, a, o, al)
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"a={a} o={o}")


def test_denormal_range_belief_flushes(oracle):
    """A belief scaled until the products T * b fall below FLT_MIN, flushed
    on both sides: the oracle's explicit flushes against FTZ / DAZ."""
    H, W = 9, 13
    g = grid(H, W)
    T, L, _ = REF.model_pomdp(g, goals(H, W)[0])
    b = belief(g)
    # the largest product 0.7 * max(b) lands just below FLT_MIN; most terms
    # are subnormal, the smallest beliefs are subnormal inputs themselves
    bs = (b.astype(np.float64) * (float(FLT_MIN) / float(b.max()))).astype(np.float32)
    assert ((bs > 0) & (bs < FLT_MIN)).any() and (0.7 * bs.max() < FLT_MIN)
    nonzero = 0
    for scale in (1.0, 4.0, 64.0):  # all flushed / straddling FLT_MIN / mostly above
        bb = (bs * np.float32(scale)).astype(np.float32)
        for u in range(9):
            for z in (0, 5, 10, 15):
                want = REF.belief_update(H, W, T, L, bb, u, z, ftz=True)
                got = oracle.belief_update(H, W, T, L, bb, u, z, ftz=True)
                np.testing.assert_array_equal(bits(got), bits(want),
                                              err_msg=f"scale={scale} u={u} z={z}")
                assert not ((want != 0) & (np.abs(want) < FLT_MIN)).any()
                nonzero += int((want != 0).sum())
    assert nonzero > 0
    # without the flush the same inputs give subnormal results on both sides
    want = REF.belief_update(H, W, T, L, bs, 4, 0, ftz=False)
    got = oracle.belief_update(H, W, T, L, bs, 4, 0, ftz=False)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert ((want != 0) & (np.abs(want) < FLT_MIN)).any()


def test_calls_restore_mxcsr():
    """The flush mode is set for the call only: the calling thread's MXCSR is
    what it was, and its own arithmetic still produces subnormals."""
    g = grid(3, 3)
    before = REF.mxcsr()
    T, L, _ = REF.model_pomdp(g, (1, 1), ftz=True)
    REF.belief_update(3, 3, T, L, belief(g), 0, 0, ftz=True)
    assert REF.mxcsr() == before
    assert before & 0x8040 == 0, "the test process itself runs with FTZ or DAZ set"
    tiny = np.float32(FLT_MIN)
    assert tiny * np.float32(0.5) > 0


# ---- the committed fixtures, recomputed from the reference library alone -----
MODEL_MAPS = ["map_3x3", "map_5x5", "map_10x10", "map_100x40", "sparse_map_100x40",
              "tile64_sparse_map_100x40"]


@pytest.mark.parametrize("name", MODEL_MAPS)
def test_golden_model_from_reference(name):
    g = golden("model", name)
    m = golden_map(name)
    T, L, R = REF.model_pomdp(m, tuple(g["goal"]))
    Tm, C = REF.model_mdp(m, tuple(g["goal"]))
    np.testing.assert_array_equal(g["T"], T)
    np.testing.assert_array_equal(g["T"], Tm)  # one T serves both models in the fixtures
    np.testing.assert_array_equal(g["L"], L)
    np.testing.assert_array_equal(g["R"], R)
    np.testing.assert_array_equal(g["C"], C)


@pytest.mark.parametrize("name", ["map_10x10", "sparse_map_100x40",
                                  "tile64_sparse_map_100x40"])
def test_golden_mdp_from_reference(name):
    m = golden_map(name)
    H, W = m.shape
    Tm, C = REF.model_mdp(m, tuple(golden("model", name)["goal"]))
    J = np.zeros(H * W, np.float32)
    for _ in range(7):
        J, A = REF.mdp_sweep(H, W, GAMMA, Tm, C, J)
    g = golden("mdp", name)
    np.testing.assert_array_equal(bits(g["J7"]), bits(J))
    np.testing.assert_array_equal(g["A7"], A)


@pytest.mark.parametrize("name", ["map_10x10", "sparse_map_100x40"])
def test_golden_fib_state_from_reference(oracle, name):
    """The 3-sweep FIB state test_fib_bit_exact holds the device to (the
    oracle's, from the fixture model) is the reference library's own."""
    m = golden_map(name)
    H, W = m.shape
    g = golden("model", name)
    T, L, R = REF.model_pomdp(m, tuple(g["goal"]))
    a = ao = np.zeros((H * W, 9), np.float32)
    for _ in range(3):
        a = REF.fib_sweep(H, W, GAMMA, T, L, R, a)
        ao = oracle.fib_sweep(H, W, GAMMA, g["T"], g["L"], g["R"], ao)
    np.testing.assert_array_equal(bits(ao), bits(a))


# ---- the pin is falsifiable ----------------------------------------------------
def test_uncontracted_build_differs(models):
    """Built without fma contraction the same kernels must give other bits
    somewhere in the Bellman values, the belief and the FIB alphas.  If they
    do not, the "fma" build did not contract and the equalities above do not
    pin the oracle's fma placement."""
    H, W = 33, 65
    g, T, L, R, Tm, C = models(H, W)
    J = Jn = np.zeros(H * W, np.float32)
    for _ in range(12):
        J, _ = REF.mdp_sweep(H, W, GAMMA, Tm, C, J)
        Jn, _ = REF.mdp_sweep(H, W, GAMMA, Tm, C, Jn, variant="nofma")
    assert (bits(J) != bits(Jn)).any(), "Bellman values: fma and nofma builds agree"
    b = belief(g)
    differs = False
    for u in range(9):
        bf = REF.belief_update(H, W, T, L, b, u, 0)
        bn = REF.belief_update(H, W, T, L, b, u, 0, variant="nofma")
        differs |= bool((bits(bf) != bits(bn)).any())
    assert differs, "belief: fma and nofma builds agree"
    a = an = np.zeros((H * W, 9), np.float32)
    for _ in range(4):
        a = REF.fib_sweep(H, W, GAMMA, T, L, R, a)
        an = REF.fib_sweep(H, W, GAMMA, T, L, R, an, variant="nofma")
    assert (bits(a) != bits(an)).any(), "FIB alphas: fma and nofma builds agree"
