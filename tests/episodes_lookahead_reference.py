"""Free-running NumPy restatement of a lookahead episode (include/pp2.h
"episodes", "Lookahead runs"; a helper module built on episodes_reference.py
and episodes_alpha_reference.py, not a test).  A lookahead episode is an alpha
episode with step 1 replaced by the one-step lookahead

    Q_u = dot(b, Rp_u) + fl(gamma * sum_z max_k dot(raw_uz, alpha_k)),

raw_uz the oracle's unnormalised belief update of the stored b by (u, z), every
dot in the pinned Q-dot order, the first maximum over k (``AR.pick``'s rule),
the sum over z ascending from +0 and the first maximum over u.  Everything
else is restated from the alpha episode, rounding by rounding, so results are
compared as bit patterns.
"""
from __future__ import annotations

import numpy as np

import episodes_alpha_reference as AR
import episodes_reference as R
from oracle import oracle as O

ftz = R.ftz

LOOK_HORIZON = 12


def look_case(case=None) -> dict:
    """The lookahead tests' cut of ``R.main_case()``: horizon 12 and eight
    starts -- the case's first six and two of its starts near the goal (its
    first eight alone reach no goal within 12 steps)."""
    case = dict(R.main_case() if case is None else case)
    case["starts"] = np.concatenate([case["starts"][:6], case["starts"][-2:]]).astype(np.int32)
    case["horizon"] = LOOK_HORIZON
    return case


def adot_pinned_zk(x_pad: np.ndarray, a_pad: np.ndarray) -> np.ndarray:
    """V[Z, K] = ``AR.adot_pinned(x_pad[z], a_pad)`` for every z at once:
    x_pad [Z, NP], a_pad [K, NP] padded planes."""
    x_pad = np.asarray(x_pad, np.float32)
    a_pad = np.asarray(a_pad, np.float32)
    Z, npad = x_pad.shape
    K = a_pad.shape[0]
    nj = (npad + 1023) // 1024
    x = np.zeros((Z, nj * 1024), np.float32)
    x[:, :npad] = x_pad
    q = np.zeros((K, nj * 1024), np.float32)
    q[:, :npad] = a_pad
    x = x.reshape(Z, 1, nj, 256, 4)
    q = q.reshape(1, K, nj, 256, 4)
    acc = np.zeros((Z, K, 256), np.float32)
    lanes = np.arange(256)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nj):
            for k in range(4):
                acc = ftz(acc + ftz(x[:, :, j, :, k] * q[:, :, j, :, k]))
        for o in (32, 16, 8, 4, 2, 1):
            acc = ftz(acc + acc[:, :, lanes ^ o])
        w = acc[:, :, ::64]
        return ftz(ftz(ftz(w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3])


def pick_rows(V: np.ndarray) -> np.ndarray:
    """``AR.pick`` of every row of V[Z, K]."""
    idx = np.zeros(V.shape[0], np.int64)
    rows = np.arange(V.shape[0])
    with np.errstate(invalid="ignore"):
        for k in range(1, V.shape[1]):
            idx = np.where(V[rows, idx] < V[:, k], k, idx)
    return idx


def lookahead_control(m: R.Model, Rw, a_pad, b, wp: int | None = None):
    """(u, Q[9], rew[9], M[9, 16], idx[9, 16]) of the stored belief b [hw]:
    Rw [hw, 9] the POMDP stage rewards, a_pad [K, NP] the padded alpha planes."""
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    r_pad = R.pad_plane(np.asarray(Rw, np.float32).reshape(H * W, 9).T, H, W, wp)
    b = np.asarray(b, np.float32).reshape(-1)
    rew = AR.adot_pinned(R.pad_plane(ftz(b), H, W, wp), r_pad)
    Q = np.zeros(9, np.float32)
    M = np.zeros((9, 16), np.float32)
    idx = np.zeros((9, 16), np.int32)
    rows = np.arange(16)
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(9):
            raw = np.stack([O.belief_update(H, W, m.T, m.L, b, u, z) for z in range(16)])
            V = adot_pinned_zk(R.pad_plane(raw, H, W, wp), a_pad)
            i = pick_rows(V)
            idx[u], M[u] = i, V[rows, i]
            S = np.float32(0.0)
            for z in range(16):
                S = ftz(np.float32(S + M[u, z]))
            Q[u] = ftz(np.float32(rew[u] + ftz(np.float32(m.gamma * S))))
    return AR.pick(Q), Q, rew, M, idx


def run_lookahead_episode(m: R.Model, Rw, alphas, b0, start: int, horizon: int, seed: int,
                          e: int, wp: int | None = None) -> dict:
    """Episode e of a lookahead batch.  alphas: [K, hw] fp32, Rw: [hw, 9]."""
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    a_pad = R.pad_plane(np.asarray(alphas, np.float32).reshape(-1, H * W), H, W, wp)
    b = np.array(b0, np.float32).reshape(-1)
    s = int(start)
    G, d = np.float32(0.0), np.float32(1.0)
    out = {"actions": [], "observations": [], "cells": [], "q": [], "rewards": [],
           "leaf_max": [], "leaf_index": []}
    steps, status = horizon, 0
    if s == m.goal_cell:
        steps, status = 0, 1
    k = 0
    while status == 0 and k < horizon:
        # 1. control
        u, Q, rew, M, idx = lookahead_control(m, Rw, a_pad, b, wp)
        out["q"].append(Q)
        out["rewards"].append(rew)
        out["leaf_max"].append(M)
        out["leaf_index"].append(idx)
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


def run_lookahead_batch(m: R.Model, Rw, alphas, b0, starts, horizon: int, seed: int,
                        wp: int | None = None) -> dict:
    """What ``R.run_batch`` returns (qsums [horizon, E, 9]: the nine Q_u;
    mode_cells -1), plus the lookahead trace ``q``, ``rewards`` [horizon, E, 9]
    and ``leaf_max``, ``leaf_index`` [horizon, E, 9, 16] (steps not taken: 0, 0,
    0, -1)."""
    E = len(starts)
    r = {"steps": np.zeros(E, np.int32), "status": np.zeros(E, np.uint8),
         "cost": np.zeros(E, np.float32), "final_cell": np.zeros(E, np.int32),
         "beliefs": np.zeros((E, m.H * m.W), np.float32),
         "actions": np.full((horizon, E), 255, np.uint8),
         "observations": np.full((horizon, E), 255, np.uint8),
         "cells": np.full((horizon, E), -1, np.int32),
         "qsums": np.zeros((horizon, E, 9), np.float32),
         "mode_cells": np.full((horizon, E), -1, np.int32),
         "q": np.zeros((horizon, E, 9), np.float32),
         "rewards": np.zeros((horizon, E, 9), np.float32),
         "leaf_max": np.zeros((horizon, E, 9, 16), np.float32),
         "leaf_index": np.full((horizon, E, 9, 16), -1, np.int32)}
    for e in range(E):
        o = run_lookahead_episode(m, Rw, alphas, b0, int(starts[e]), horizon, seed, e, wp)
        n = len(o["actions"])
        r["steps"][e], r["status"][e] = o["steps"], o["status"]
        r["cost"][e], r["final_cell"][e] = o["cost"], o["final_cell"]
        r["beliefs"][e] = o["belief"]
        if n:
            r["actions"][:n, e] = o["actions"]
            r["observations"][:n, e] = o["observations"]
            r["cells"][:n, e] = o["cells"]
            r["q"][:n, e] = np.array(o["q"], np.float32)
            r["qsums"][:n, e] = r["q"][:n, e]
            r["rewards"][:n, e] = np.array(o["rewards"], np.float32)
            r["leaf_max"][:n, e] = np.array(o["leaf_max"], np.float32)
            r["leaf_index"][:n, e] = np.array(o["leaf_index"], np.int32)
    return r
