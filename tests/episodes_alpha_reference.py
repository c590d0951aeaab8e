"""Free-running NumPy restatement of an alpha-vector episode (include/pp2.h
"episodes", "Alpha runs"; a helper module like episodes_reference.py, on which
it is built, not a test).  An alpha episode is an episode of
``episodes_reference`` with step 1 replaced: V_k = <b, alpha_k> in the pinned
Q-dot order for K vectors, best = 0 and ``if V_best < V_k: best = k`` in
ascending k, u = actions[best].  Everything else -- cost, motion, observation,
belief, rescale, goal -- is restated from there, rounding by rounding, so
results are compared as bit patterns.

``main_fib_alphas()`` is the FIB set of the main case (``R.main_case()``) from
the oracle, shared by the CPU tests.
"""
from __future__ import annotations

import numpy as np

import episodes_reference as R
from oracle import oracle as O

ftz = R.ftz


def adot_pinned(b_pad: np.ndarray, a_pad: np.ndarray) -> np.ndarray:
    """V[K] in the pinned order (``R.qdot_pinned`` for K planes): b_pad [NP],
    a_pad [K, NP] padded planes.  Non-finite entries take part as they are."""
    a_pad = np.asarray(a_pad, np.float32)
    K, npad = a_pad.shape
    nj = (npad + 1023) // 1024
    b = np.zeros(nj * 1024, np.float32)
    b[:npad] = b_pad
    q = np.zeros((K, nj * 1024), np.float32)
    q[:, :npad] = a_pad
    b = b.reshape(nj, 256, 4)
    q = q.reshape(K, nj, 256, 4)
    acc = np.zeros((K, 256), np.float32)
    lanes = np.arange(256)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nj):
            for k in range(4):
                acc = ftz(acc + ftz(b[j, :, k][None, :] * q[:, j, :, k]))
        for o in (32, 16, 8, 4, 2, 1):
            acc = ftz(acc + acc[:, lanes ^ o])
        w = acc[:, ::64]
        return ftz(ftz(ftz(w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])


def pick(V) -> int:
    """evaluateFibCpu / evaluatePbviCpu's winner: the first maximum; a NaN sum
    never displaces the incumbent, a NaN V[0] is never displaced."""
    best = 0
    for k in range(1, len(V)):
        if V[best] < V[k]:
            best = k
    return best


def run_alpha_episode(m: R.Model, alphas, actions, b0, start: int, horizon: int, seed: int,
                      e: int, wp: int | None = None) -> dict:
    """Episode e of an alpha batch.  alphas: [K, hw] fp32, actions: [K]."""
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    a_pad = R.pad_plane(np.asarray(alphas, np.float32).reshape(-1, H * W), H, W, wp)
    actions = np.asarray(actions)
    b = np.array(b0, np.float32).reshape(-1)
    s = int(start)
    G, d = np.float32(0.0), np.float32(1.0)
    out = {"actions": [], "observations": [], "cells": [], "sums": [], "best_index": [],
           "best_sum": []}
    steps, status = horizon, 0
    if s == m.goal_cell:
        steps, status = 0, 1
    k = 0
    while status == 0 and k < horizon:
        # 1. control
        V = adot_pinned(R.pad_plane(ftz(b), H, W, wp), a_pad)
        best = pick(V)
        u = int(actions[best])
        out["sums"].append(V)
        out["best_index"].append(best)
        out["best_sum"].append(V[best])
        # 2. cost (the MDP cost, as for every policy)
        G = ftz(np.float32(G + ftz(np.float32(d * m.C[s, u]))))
        d = ftz(np.float32(d * m.gamma))
        # 3. motion
        i = R._scan(m.T[s, u], R.uniform(seed, e, 2 * k), 4)
        x, y = s % W + i % 3 - 1, s // W + i // 3 - 1
        if 0 <= x < W and 0 <= y < H:
            s = y * W + x
        # 4. observation
        z = R._scan(m.L[s], R.uniform(seed, e, 2 * k + 1), 15)
        out["actions"].append(u)
        out["observations"].append(z)
        out["cells"].append(s)
        # 5. belief
        raw = O.belief_update(H, W, m.T, m.L, b, u, z)
        top = raw.max()
        if not (np.isfinite(top) and top > 0):
            b, status, steps = raw, 2, k + 1
            break
        e2 = int(np.clip(np.frexp(top)[1] - 1, -126, 126))
        b = ftz(raw * np.float32(2.0 ** -e2))
        # 6. goal
        if s == m.goal_cell:
            status, steps = 1, k + 1
        k += 1
    out.update(steps=steps, status=status, cost=G, final_cell=s, belief=b)
    return out


def run_alpha_batch(m: R.Model, alphas, actions, b0, starts, horizon: int, seed: int,
                    wp: int | None = None) -> dict:
    """What ``R.run_batch`` returns (qsums [horizon, E, 9]: the nine V_k when
    K = 9, the caller decides whether the run records them; mode_cells -1),
    plus ``best_index`` / ``best_sum`` [horizon, E] (steps not taken: -1, 0)
    and ``sums``, per episode the list of its steps' V[K]."""
    E = len(starts)
    K = np.asarray(alphas).reshape(-1, m.H * m.W).shape[0]
    r = {"steps": np.zeros(E, np.int32), "status": np.zeros(E, np.uint8),
         "cost": np.zeros(E, np.float32), "final_cell": np.zeros(E, np.int32),
         "beliefs": np.zeros((E, m.H * m.W), np.float32), "ties": np.zeros(E, np.int64),
         "actions": np.full((horizon, E), 255, np.uint8),
         "observations": np.full((horizon, E), 255, np.uint8),
         "cells": np.full((horizon, E), -1, np.int32),
         "qsums": np.zeros((horizon, E, 9), np.float32),
         "mode_cells": np.full((horizon, E), -1, np.int32),
         "best_index": np.full((horizon, E), -1, np.int32),
         "best_sum": np.zeros((horizon, E), np.float32), "sums": []}
    for e in range(E):
        o = run_alpha_episode(m, alphas, actions, b0, int(starts[e]), horizon, seed, e, wp)
        n = len(o["actions"])
        r["steps"][e], r["status"][e] = o["steps"], o["status"]
        r["cost"][e], r["final_cell"][e] = o["cost"], o["final_cell"]
        r["beliefs"][e] = o["belief"]
        r["sums"].append(o["sums"])
        if n:
            r["actions"][:n, e] = o["actions"]
            r["observations"][:n, e] = o["observations"]
            r["cells"][:n, e] = o["cells"]
            r["best_index"][:n, e] = o["best_index"]
            r["best_sum"][:n, e] = np.array(o["best_sum"], np.float32)
            if K == 9:
                r["qsums"][:n, e] = np.array(o["sums"], np.float32)
    return r


def main_fib_alphas(case=None):
    """(model, alphas [9, hw], actions 0..8) of the main case: the oracle's FIB
    solve of sparse_map_100x40 with goal (95, 34)."""
    case = R.main_case() if case is None else case
    grid = case["grid"]
    H, W = grid.shape
    m = R.Model(grid, case["goal"], case["gamma"])
    _, _, Rw = O.model_pomdp(grid, case["goal"])
    a, _, _ = O.fib_solve(H, W, m.gamma, m.T, m.L, Rw)
    return m, np.ascontiguousarray(a.T), np.arange(9, dtype=np.uint8)
