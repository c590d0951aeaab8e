"""NumPy restatement of the policy evaluator's definition (include/pp2.h
"policy evaluation"), written from the header text: the three outcome planes
of a fixed action table after H steps, in the definition's exact fp32
flush-to-zero arithmetic (``evaluate``) and as the same recurrence in fp64
without flushing (``chain_f64``, a semantic check).

T is [H*W, 9, 9], C [H*W, 9] (pp2_model_download's layouts), pi [H*W] or
[H, W] with entries <= 8, goal (gx, gy); cells are y * W + x and neighbour i
of a cell is displaced by (i % 3 - 1, i // 3 - 1).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
TINY = np.finfo(np.float32).tiny  # 2^-126, the smallest normal


def ftz(x) -> np.ndarray:
    """Subnormal fp32 values become zero of the same sign."""
    x = np.array(x, np.float32, copy=True)
    sub = (np.abs(x) < TINY) & (x != 0)
    x[sub] = np.copysign(F32(0), x[sub])
    return x


def fmaf_ieee(a, b, c) -> np.ndarray:
    """fl32(a * b + c) with ONE rounding (round to nearest even), vectorised.

    Why it is exact: a and b carry 24 significant bits, so p = a * b has at
    most 48 and is exact in fp64 (its exponent is far inside fp64's range).
    s = fl64(p + c) is rounded to 53 bits, and Knuth's TwoSum gives the error
    e = (p + c) - s exactly (no overflow here, so TwoSum is error-free under
    round-to-nearest).  Rounding s straight to fp32 could round twice: when s
    lands on an fp32 tie (or e pulled it there) the second rounding no longer
    knows on which side of the tie the exact sum lies.  So s is first turned
    into the *round-to-odd* fp64 value of the exact sum: if e == 0 it is s;
    otherwise the exact sum lies strictly between s and its fp64 neighbour in
    the direction of e, and round-to-odd is whichever of the two has an odd
    last significand bit (exactly one does).  Rounding a round-to-odd value of
    p + 2 or more bits to p bits with round-to-nearest-even gives the correctly
    rounded result (Boldo and Melquiond, "Emulation of a FMA and correctly
    rounded sums", 2008): an odd last bit is never a tie and never lies on the
    wrong side of one.  53 >= 24 + 2, also in fp32's subnormal range, where
    fewer bits are kept.
    """
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c64 = np.asarray(c, np.float32).astype(np.float64)
    p, c64 = np.broadcast_arrays(p, c64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    nudge = (e != 0) & even & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(nudge, np.nextafter(s, toward), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def fmaf_ftz(a, b, c) -> np.ndarray:
    """fmaf under flush-to-zero: subnormal operands read as zero, a subnormal
    result is flushed."""
    return ftz(fmaf_ieee(ftz(a), ftz(b), ftz(c)))


def mul_ftz(a, b) -> np.ndarray:
    return ftz(ftz(a) * ftz(b))


def _shift(plane, i, zero):
    """plane(x + off_i) per cell, `zero` off the grid."""
    H, W = plane.shape
    dx, dy = i % 3 - 1, i // 3 - 1
    out = np.full((H, W), zero, plane.dtype)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = plane[ys, xs]
    return out


def _rows(T, C, pi, H, W):
    hw = H * W
    pi = np.asarray(pi, np.uint8).reshape(hw)
    assert pi.max(initial=0) <= 8
    idx = np.arange(hw)
    Tu = np.asarray(T, np.float32).reshape(hw, 9, 9)[idx, pi]  # [hw, 9]
    Cu = np.asarray(C, np.float32).reshape(hw, 9)[idx, pi]
    return Tu.reshape(H, W, 9), Cu.reshape(H, W)


def _goal_mask(goal, H, W):
    m = np.zeros((H, W), bool)
    gx, gy = int(goal[0]), int(goal[1])
    if 0 <= gx < W and 0 <= gy < H:
        m[gy, gx] = True
    return m


def evaluate(T, C, pi, gamma, goal, H, W, horizon):
    """(G, P, N) as [H, W] float32 after `horizon` steps, the definition's bits."""
    Tu, Cu = _rows(T, C, pi, H, W)
    gT = mul_ftz(np.float32(gamma), Tu)
    goal_m = _goal_mask(goal, H, W)
    G = np.zeros((H, W), np.float32)
    N = np.zeros((H, W), np.float32)
    P = goal_m.astype(np.float32)
    for _ in range(int(horizon)):
        g = Cu.copy()
        p = np.zeros((H, W), np.float32)
        n = np.ones((H, W), np.float32)
        for i in range(9):
            g = fmaf_ftz(gT[:, :, i], _shift(G, i, F32(0)), g)
            p = fmaf_ftz(Tu[:, :, i], _shift(P, i, F32(0)), p)
            n = fmaf_ftz(Tu[:, :, i], _shift(N, i, F32(0)), n)
        g[goal_m], p[goal_m], n[goal_m] = F32(0), F32(1), F32(0)
        G, P, N = g, p, n
    return G, P, N


def chain_f64(T, C, pi, gamma, goal, H, W, horizon):
    """The same recurrence in fp64 from the fp32 model, no flushing."""
    Tu, Cu = _rows(T, C, pi, H, W)
    Tu, Cu = Tu.astype(np.float64), Cu.astype(np.float64)
    gT = float(np.float32(gamma)) * Tu
    goal_m = _goal_mask(goal, H, W)
    G = np.zeros((H, W))
    N = np.zeros((H, W))
    P = goal_m.astype(np.float64)
    for _ in range(int(horizon)):
        g, p, n = Cu.copy(), np.zeros((H, W)), np.ones((H, W))
        for i in range(9):
            g = g + gT[:, :, i] * _shift(G, i, 0.0)
            p = p + Tu[:, :, i] * _shift(P, i, 0.0)
            n = n + Tu[:, :, i] * _shift(N, i, 0.0)
        g[goal_m], p[goal_m], n[goal_m] = 0.0, 1.0, 0.0
        G, P, N = g, p, n
    return G, P, N


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
