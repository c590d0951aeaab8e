"""NumPy restatement of the forward occupancy's definition (include/pp2.h
"occupancy"), written from the header text: the distribution D after H steps
of a fixed action table from a start distribution b0, the expected visits V
before arrival and the arrival curve, in the definition's exact fp32
flush-to-zero arithmetic (``evaluate``) and as the same recurrence in fp64
without flushing (``chain_f64``, a semantic check).

T is [H*W, 9, 9] (pp2_model_download's layout), pi [H*W] or [H, W] with entries
<= 8, goal (gx, gy), b0 [H*W] or [H, W]; cells are y * W + x, neighbour i of a
cell is displaced by off_i = (i % 3 - 1, i // 3 - 1), and destination y gathers
from the sources x = y - off_i.
"""
from __future__ import annotations

import numpy as np

from policy_reference import _shift, bits, fmaf_ftz, ftz  # noqa: F401  (bits: for the tests)

F32 = np.float32


def canonical_b0(b0, H, W):
    """b0 as the definition reads it: -0 and subnormals are +0."""
    b = np.array(b0, np.float32, copy=True).reshape(H, W)
    assert not np.isnan(b).any() and (b >= 0).all() and (b <= 1).all()
    return np.abs(ftz(b))


def _rows(T, pi, H, W):
    """Tu[y, x, i] = T[cell][pi[cell]][i]."""
    hw = H * W
    pi = np.asarray(pi, np.uint8).reshape(hw)
    assert pi.max(initial=0) <= 8
    return np.asarray(T, np.float32).reshape(hw, 9, 9)[np.arange(hw), pi].reshape(H, W, 9)


def _goal(goal, H, W):
    gx, gy = int(goal[0]), int(goal[1])
    return (gy, gx) if 0 <= gx < W and 0 <= gy < H else None


def _from_source(plane, i, zero):
    """plane(y - off_i) per cell y, `zero` where the source is off the grid:
    the shift by off_{8 - i} = -off_i."""
    return _shift(plane, 8 - i, zero)


def evaluate(T, pi, goal, b0, H, W, horizon):
    """(D, V, curve): D and V as [H, W] float32 after `horizon` steps, curve
    [horizon + 1], the definition's bits."""
    Tu = _rows(T, pi, H, W)
    g = _goal(goal, H, W)
    # the weight of source x = y - off_i into y is entry i of x's row; a source
    # off the grid contributes fmaf(+0, +0, d)
    wts = [_from_source(np.ascontiguousarray(Tu[:, :, i]), i, F32(0)) for i in range(9)]
    D = canonical_b0(b0, H, W)
    V = np.zeros((H, W), np.float32)
    curve = np.zeros(int(horizon) + 1, np.float32)
    if g:
        curve[0] = D[g]
    for k in range(1, int(horizon) + 1):
        S = D.copy()
        d = np.zeros((H, W), np.float32)
        if g:
            S[g] = F32(0)
            d[g] = D[g]
        V = ftz(ftz(V) + ftz(S))
        for i in range(9):
            d = fmaf_ftz(wts[i], _from_source(S, i, F32(0)), d)
        D = d
        if g:
            curve[k] = D[g]
    return D, V, curve


def chain_f64(T, pi, goal, b0, H, W, horizon):
    """The same recurrence in fp64 from the fp32 model and b0, no flushing."""
    Tu = _rows(T, pi, H, W).astype(np.float64)
    g = _goal(goal, H, W)
    wts = [_from_source(np.ascontiguousarray(Tu[:, :, i]), i, 0.0) for i in range(9)]
    D = canonical_b0(b0, H, W).astype(np.float64)
    V = np.zeros((H, W))
    curve = np.zeros(int(horizon) + 1)
    if g:
        curve[0] = D[g]
    for k in range(1, int(horizon) + 1):
        S = D.copy()
        d = np.zeros((H, W))
        if g:
            S[g] = 0.0
            d[g] = D[g]
        V = V + S
        for i in range(9):
            d = d + wts[i] * _from_source(S, i, 0.0)
        D = d
        if g:
            curve[k] = D[g]
    return D, V, curve
