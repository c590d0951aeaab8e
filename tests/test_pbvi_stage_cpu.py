"""CPU: the stage references of the PBVI backup (pbvi_stage_cases.py) before
test_gpu_pbvi_stages.py holds the device kernels to them.

* orc_fma_chain_nt, the one statement of the pinned Sgemm chain, against an
  exact fused multiply-add: Fraction product and sum, rounded once to float32
  by an integer round-to-nearest-even -- on chains with subnormal operands and
  sums, ties, exact and near cancellation and signed zeros.
* The stage references chained reproduce the oracle's warm-started backup bit
  for bit on every case of the table, and the cases hold what they are for:
  ties that the first of two duplicate alphas has to win, dots that stay
  subnormal, and -0 results of Gamma_ao at edge cells.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref as REF
from pbvi_stage_cases import (CASES, ROW_TINY, bits, case, case_id, ref_backup_stages,
                              ref_gamma_ao)


# ------------------------------------------------------------ exact fma
def rne_f32(q: Fraction) -> np.float32:
    """q != 0 rounded to the nearest float32, ties to even, subnormals kept;
    a result below half the smallest subnormal is a zero of q's sign."""
    neg = q < 0
    n, d = abs(q).numerator, abs(q).denominator
    e = n.bit_length() - d.bit_length()  # 2^(e-1) < |q| < 2^(e+1)
    if (n << max(0, -e)) < (d << max(0, e)):
        e -= 1                           # 2^e <= |q| < 2^(e+1)
    qe = max(e, -126) - 23               # exponent of the last kept bit
    num, den = (n << max(0, -qe)), (d << max(0, qe))
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    assert m <= 1 << 24 and qe + 24 <= 128
    v = float(m) * 2.0 ** qe             # exact in double: m <= 2^24, qe >= -149
    return np.float32(-v if neg else v)


def exact_fma(a, b, c) -> np.float32:
    fa, fb, fc = Fraction(float(a)), Fraction(float(b)), Fraction(float(c))
    s = fa * fb + fc
    if s != 0:
        return rne_f32(s)
    # an exact zero: -0 only as the sum of two negative zeros
    pneg = bool(np.signbit(a)) != bool(np.signbit(b))
    neg = fa * fb == 0 and pneg and bool(np.signbit(c))
    return np.float32(-0.0 if neg else 0.0)


def word(v) -> int:
    return int(np.array(v, np.float32).reshape(1).view(np.uint32)[0])


def test_rne_helper():
    f = np.float32
    assert rne_f32(Fraction(1)) == f(1)
    assert rne_f32(Fraction(1) + Fraction(1, 1 << 24)) == f(1)                       # tie -> even
    assert rne_f32(Fraction(1) + Fraction(3, 1 << 24)) == f(1) + f(2.0 ** -22)       # tie -> even (up)
    assert rne_f32(Fraction(1) + Fraction(1, 1 << 24) + Fraction(1, 1 << 60)) == f(1) + f(2.0 ** -23)
    assert bits(rne_f32(Fraction(1, 1 << 149))) == 1                                 # smallest subnormal
    assert bits(rne_f32(Fraction(1, 1 << 150))) == 0                                 # tie -> even: +0
    assert bits(rne_f32(Fraction(-1, 1 << 151))) == 0x80000000
    assert bits(rne_f32(Fraction(3, 1 << 150))) == 2                                 # tie -> even (up)
    assert bits(rne_f32(Fraction((1 << 24) - 1, 1 << 150) + Fraction(1, 1 << 150))) == 0x00800000
    assert bits(exact_fma(f(-0.0), f(3), f(-0.0))) == 0x80000000
    assert bits(exact_fma(f(0.0), f(0.0), f(-0.0))) == 0
    assert bits(exact_fma(f(2), f(-3), f(6))) == 0


def chain_inputs():
    """A [3, n], B [11, n], n = 2000: eleven B rows take both the eight-wide
    walk of orc_fma_chain_nt and its tail."""
    rng = np.random.default_rng(4242)
    n, M, N = 2000, 3, 11
    f = np.float32

    def block(m):
        a = np.empty((M, m), np.float32)
        b = np.empty((N, m), np.float32)
        return a, b

    parts = []
    # sums that stay subnormal: products near 2^-140
    a, b = block(400)
    a[:] = np.ldexp(rng.random(a.shape), -70)
    b[:] = np.ldexp(rng.uniform(-1, 1, b.shape), -70)
    parts.append((a, b))
    # subnormal operands against ordinary ones
    a, b = block(300)
    a[:] = rng.random(a.shape) * 1e-3
    a[:, ::3] = f(1e-42)
    a[:, 1::7] = f(7e-39)
    b[:] = rng.uniform(-20, 20, b.shape)
    parts.append((a, b))
    # small integers: exact sums, many of them exactly zero
    a, b = block(300)
    a[:] = rng.integers(-2, 3, a.shape)
    b[:] = rng.integers(-2, 3, b.shape)
    a[:, ::5] = f(-0.0)
    parts.append((a, b))
    # wide exponent range, mixed sign: absorption and cancellation
    a, b = block(n - 1000 - 15)
    a[:] = np.ldexp(rng.uniform(-1, 1, a.shape), rng.integers(-30, 30, a.shape))
    b[:] = np.ldexp(rng.uniform(-1, 1, b.shape), rng.integers(-30, 30, b.shape))
    parts.append((a, b))
    A = np.concatenate([p[0] for p in parts], axis=1)
    Bm = np.concatenate([p[1] for p in parts], axis=1)
    # the head of chain (0, 0), by hand: ties both ways, an exact
    # cancellation, a difference only a fused product keeps, an underflow to -0
    head = [(1, 1),                       # acc = 1
            (2.0 ** -12, 2.0 ** -12),     # + 2^-24: tie, stays 1
            (1, 2.0 ** -23),              # 1 + 2^-23
            (2.0 ** -12, 2.0 ** -12),     # tie, up to 1 + 2^-22
            (-1, 1 + 2.0 ** -22),         # exact cancellation: +0
            (-(2.0 ** -100), 2.0 ** -100),  # -2^-200: -0
            (0, 5),                       # +0 + -0 = +0
            (1, -1),                      # -1
            (1 + 2.0 ** -12, 1 - 2.0 ** -12),  # 1 - 2^-24 - 1 = -2^-24, exactly
            (2.0 ** -75, 2.0 ** -75),     # + 2^-150 onto -2^-24: absorbed
            (1, 2.0 ** -24),              # back to +0
            (2.0 ** -75, 2.0 ** -75),     # 2^-150: tie at half the smallest subnormal -> +0
            (3 * 2.0 ** -75, 2.0 ** -75),  # 3 * 2^-150 -> 2 * 2^-149
            (2.0 ** -63, 2.0 ** -63),     # + 2^-126: subnormal to normal, 2^-126 + 2^-148
            (-(2.0 ** -63), 2.0 ** -63)]  # and back to the subnormal 2^-148
    head_a = np.array([h[0] for h in head], np.float32)
    head_b = np.array([h[1] for h in head], np.float32)
    assert np.array_equal(head_a.astype(np.float64), [h[0] for h in head])
    assert np.array_equal(head_b.astype(np.float64), [h[1] for h in head])
    ha = np.zeros((M, len(head)), np.float32)  # the other chains stay at +0 through the head
    hb = np.zeros((N, len(head)), np.float32)
    ha[0], hb[0] = head_a, head_b
    A = np.concatenate([ha, A], axis=1)
    Bm = np.concatenate([hb, Bm], axis=1)
    assert A.shape == (M, n) and Bm.shape == (N, n)
    return np.ascontiguousarray(A), np.ascontiguousarray(Bm)


def test_fma_chain_nt_is_the_exact_fma_chain(oracle):
    A, B = chain_inputs()
    got = oracle.fma_chain_nt(A, B)
    want = np.empty_like(got)
    seen_sub = seen_negzero = 0
    head = []
    for i in range(A.shape[0]):
        for k in range(B.shape[0]):
            acc = np.float32(0.0)
            for x in range(A.shape[1]):
                acc = exact_fma(A[i, x], B[k, x], acc)
                seen_sub += 0 < abs(float(acc)) < 2.0 ** -126
                seen_negzero += word(acc) == 0x80000000
                if (i, k) == (0, 0) and x < 15:
                    head.append(word(acc))
            want[i, k] = acc
    # the hand-made head went where it was meant to
    f = word
    assert head == [f(1), f(1), f(1 + 2.0 ** -23), f(1 + 2.0 ** -22), 0, 0x80000000, 0, f(-1),
                    f(-(2.0 ** -24)), f(-(2.0 ** -24)), 0, 0, 2, 0x00800002, 2], \
        [hex(h) for h in head]
    assert seen_sub > 10000 and seen_negzero > 0
    np.testing.assert_array_equal(bits(got), bits(want))
    # and a changed order is seen: the chain is not a sum in any order
    rev = oracle.fma_chain_nt(A[:, ::-1], B[:, ::-1])
    assert (bits(rev) != bits(want)).any()


# ------------------------------------------------------------ the table
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_stage_references_chain_to_the_oracle_backup(oracle, c):
    cs = case(*c)
    T, L, R = cs.model(oracle)
    S = cs.S
    ties = {}       # (first, second index at a row's maximum) -> rows
    stats = {"sub": 0, "first_wins": 0}

    def visit(a, o, G, Cm, kstar):
        at_top = Cm == Cm.max(axis=1)[:, None]
        for i in np.nonzero(at_top.sum(axis=1) > 1)[0]:
            k = np.nonzero(at_top[i])[0]
            ties[int(k[0]), int(k[1])] = ties.get((int(k[0]), int(k[1])), 0) + 1
            stats["first_wins"] += int(kstar[i] == k[0])
        if S > 7:
            row = np.abs(Cm[7].astype(np.float64))
            stats["sub"] += int(((row > 0) & (row < 2.0 ** -126)).sum())

    st = ref_backup_stages(oracle, cs.H, cs.W, T, L, R, cs.B, cs.A0, visit)
    al, act = cs.backup(oracle)
    np.testing.assert_array_equal(st["actions"], act)
    np.testing.assert_array_equal(bits(st["alphas"]), bits(al))
    # the case holds what it is for: ties that the first duplicate has to win
    # -- in different lanes of the argmax, in one lane, in one lane a pass apart
    assert stats["first_wins"] == sum(ties.values())
    if S > 7:
        assert ties.get((6, 7), 0) > 0, ties
        assert stats["sub"] >= 144, stats  # dots of the 2^-125 row stay subnormal
    if S > 68:
        assert ties.get((4, 68), 0) > 0, ties
    if S > 128:
        assert ties.get((127, 128), 0) > 0, ties
    if S > 582:
        assert ties.get((70, 582), 0) > 0, ties


@pytest.mark.parametrize("c", [c for c in CASES if c[2] > ROW_TINY], ids=case_id)
def test_tiny_alpha_row_gives_negative_zero_at_edge_cells(oracle, c):
    """Gamma_ao of the +-1e-36 row: products underflow, flush to -0, and where
    the cell's last in-grid neighbour comes before an off-grid one (the grid's
    last row and last column) nothing turns the -0 back: the reference's
    kernel skips off-grid terms.  Without this the -0 parity of the device
    kernel would be checked on no value.  Checked on the oracle and, where
    oracle/_ref is built, on the reference's own kernel."""
    cs = case(*c)
    T, L, _ = cs.model(oracle)
    H, W = cs.H, cs.W
    edge = np.zeros((H, W), bool)
    edge[H - 1, :] = True
    edge[:, W - 1] = True
    edge = edge.reshape(-1)
    for src in [None] + ([REF] if REF.available() else []):
        n = 0
        for a in range(9):
            for o in (a, 15 - a):
                G = ref_gamma_ao(oracle, src, H, W, T, L, a, o, cs.A0[ROW_TINY:ROW_TINY + 1])
                n += int((bits(G[0])[edge] == 0x80000000).sum())
        assert n > 0, "oracle" if src is None else "oracle/_ref"
