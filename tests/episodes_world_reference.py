"""Free-running NumPy restatement of an episode segment whose world differs
from the believed map, and of a resumed segment (include/pp2.h "episodes",
"The world" and "Resumed segments"; a helper module built on
episodes_reference.py, episodes_alpha_reference.py and
episodes_lookahead_reference.py, not a test).

One step loop, ``run_segment``, serves every policy: ``control`` is a callable
``b -> (u, trace values)`` built from the believed model by one of the
``*_control`` factories below.  Steps 1 and 5 use the believed model
``m_policy``; the goal tests, the cost and the two sampling scans use the
world ``m_world``; the discount uses ``m_policy.gamma``.  Every rounding is the
one of ``episodes_reference.run_episode``, so with ``m_world is m_policy`` the
results are those of ``R.run_batch`` / ``run_alpha_batch`` /
``run_lookahead_batch`` bit for bit.
"""
from __future__ import annotations

import numpy as np

import episodes_reference as R
from episodes_alpha_reference import adot_pinned, pick
from episodes_lookahead_reference import lookahead_control
from episodes_reference import Model, _scan, ftz, qdot_pinned, uniform
from oracle import oracle as O

_FLT_MAX = np.float32(np.finfo(np.float32).max)


def goal_cell(m: Model) -> int:
    """y * W + x of the model's goal, -1 when it lies off the grid (no goal)."""
    gx, gy = m.goal
    return gy * m.W + gx if 0 <= gx < m.W and 0 <= gy < m.H else -1


# ---------------------------------------------------------------- step 1
def mode_control(m: Model, A):
    A = np.asarray(A).reshape(-1)

    def control(b):
        bf = ftz(b)
        cand = np.where(bf > 0, bf, np.float32(0.0))
        top = cand.max()
        cell = int(cand.argmax()) if top > 0 else 0
        return int(A[cell]), {"mode_cells": cell}
    return control


def qmdp_control(m: Model, Q, wp: int | None = None):
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    q_pad = R.pad_plane(np.asarray(Q, np.float32).reshape(H * W, 9).T, H, W, wp)

    def control(b):
        S = qdot_pinned(R.pad_plane(ftz(b), H, W, wp), q_pad)
        best, u = _FLT_MAX, 0
        for a in range(9):
            if S[a] < best:
                best, u = S[a], a
        return u, {"qsums": S}
    return control


def alpha_control(m: Model, alphas, actions, wp: int | None = None):
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    a_pad = R.pad_plane(np.asarray(alphas, np.float32).reshape(-1, H * W), H, W, wp)
    actions = np.asarray(actions)
    K = a_pad.shape[0]

    def control(b):
        V = adot_pinned(R.pad_plane(ftz(b), H, W, wp), a_pad)
        best = pick(V)
        tr = {"best_index": best, "best_sum": V[best]}
        if K == 9:
            tr["qsums"] = V
        return int(actions[best]), tr
    return control


def look_control(m: Model, Rw, alphas, wp: int | None = None):
    H, W = m.H, m.W
    wp = R.row_stride(W) if wp is None else wp
    a_pad = R.pad_plane(np.asarray(alphas, np.float32).reshape(-1, H * W), H, W, wp)

    def control(b):
        u, Q, rew, M, idx = lookahead_control(m, Rw, a_pad, b, wp)
        return u, {"qsums": Q, "q": Q, "rewards": rew, "leaf_max": M, "leaf_index": idx}
    return control


# ---------------------------------------------------------------- one segment
def fresh_state(b0, start: int) -> dict:
    """An episode before its first segment: what a run (not a resume) starts from."""
    return {"s": int(start), "b": np.array(b0, np.float32).reshape(-1), "G": np.float32(0.0),
            "d": np.float32(1.0), "steps": 0, "status": 0, "fresh": True}


def run_segment(m_policy: Model, m_world: Model, control, state: dict, horizon: int, seed: int,
                e: int):
    """(state after, trace of the segment) of episode e.  A fresh state takes
    the initial goal test; any other state with status != 0 is returned as it
    is.  The trace is a list of per-step dicts, indexed by the local step."""
    mp, mw = m_policy, m_world
    H, W = mp.H, mp.W
    goal = goal_cell(mw)
    st = dict(state)
    trace = []
    if st["fresh"]:
        st["fresh"] = False
        if st["s"] == goal:
            st["status"] = 1
            return st, trace
    if st["status"] != 0:
        return st, trace
    s, b, G, d, k0 = st["s"], st["b"], st["G"], st["d"], st["steps"]
    steps, status = k0 + horizon, 0
    for j in range(horizon):
        k = k0 + j
        # 1. control: the believed model
        u, tr = control(b)
        # 2. cost: the world's C, the batch context's gamma
        G = ftz(np.float32(G + ftz(np.float32(d * mw.C[s, u]))))
        d = ftz(np.float32(d * mp.gamma))
        # 3. motion: the world's T
        i = _scan(mw.T[s, u], uniform(seed, e, 2 * k), 4)
        x, y = s % W + i % 3 - 1, s // W + i // 3 - 1
        if 0 <= x < W and 0 <= y < H:
            s = y * W + x
        # 4. observation: the world's L
        z = _scan(mw.L[s], uniform(seed, e, 2 * k + 1), 15)
        tr.update(actions=u, observations=z, cells=s)
        trace.append(tr)
        # 5. belief: the believed model
        raw = O.belief_update(H, W, mp.T, mp.L, b, u, z)
        top = raw.max()
        if not (np.isfinite(top) and top > 0):
            b, status, steps = raw, 2, k + 1
            break
        e2 = int(np.clip(np.frexp(top)[1] - 1, -126, 126))
        b = ftz(raw * np.float32(2.0 ** -e2))
        # 6. goal: the world's
        if s == goal:
            status, steps = 1, k + 1
            break
    st.update(s=s, b=b, G=G, d=d, steps=steps, status=status)
    return st, trace


# ---------------------------------------------------------------- batches
_TRACE_FILL = {"actions": (255, np.uint8, ()), "observations": (255, np.uint8, ()),
               "cells": (-1, np.int32, ()), "qsums": (0, np.float32, (9,)),
               "mode_cells": (-1, np.int32, ()), "best_index": (-1, np.int32, ()),
               "best_sum": (0, np.float32, ()), "q": (0, np.float32, (9,)),
               "rewards": (0, np.float32, (9,)), "leaf_max": (0, np.float32, (9, 16)),
               "leaf_index": (-1, np.int32, (9, 16))}


def run_batch_segment(m_policy: Model, m_world: Model, control, states, horizon: int,
                      seed: int) -> dict:
    """One segment of every episode as the device returns it: results [E],
    traces [horizon, E, ...] (steps not taken hold the device's fill values),
    beliefs [E, hw], and ``states``, the list to hand to the next segment."""
    E = len(states)
    r = {k: np.full((horizon, E) + sh, fill, dt) for k, (fill, dt, sh) in _TRACE_FILL.items()}
    r.update(steps=np.zeros(E, np.int32), status=np.zeros(E, np.uint8),
             cost=np.zeros(E, np.float32), final_cell=np.zeros(E, np.int32),
             beliefs=np.zeros((E, m_policy.H * m_policy.W), np.float32), states=[])
    for e in range(E):
        st, trace = run_segment(m_policy, m_world, control, states[e], horizon, seed, e)
        r["states"].append(st)
        r["steps"][e], r["status"][e] = st["steps"], st["status"]
        r["cost"][e], r["final_cell"][e] = st["G"], st["s"]
        r["beliefs"][e] = st["b"]
        for j, tr in enumerate(trace):
            for k, v in tr.items():
                r[k][j, e] = v
    return r


def run_batch(m_policy: Model, m_world: Model, control, b0, starts, horizon: int,
              seed: int) -> dict:
    """A run (not a resume): every episode fresh from b0 and its start cell."""
    return run_batch_segment(m_policy, m_world, control,
                             [fresh_state(b0, s) for s in starts], horizon, seed)


# ---------------------------------------------------------------- the cases
WORLD_SEED = 7
WORLD_HORIZON = 40
WORLD_GAMMA = 0.95
# name -> H, W, believed goal, world goal, world-only occupied cells (x, y),
# the cell only the believed map holds occupied
_CASES = {
    # wp = 16, three pad columns; a wall in the middle of the room
    "9x13": (9, 13, (11, 4), (11, 4), [(6, y) for y in range(2, 7)], (2, 7)),
    # wp = 12
    "7x10": (7, 10, (8, 3), (8, 3), [(5, y) for y in range(2, 5)], (1, 5)),
    # no pad column; the obstacle touches the border, the goals differ
    "8x12": (8, 12, (10, 5), (9, 2), [(11, y) for y in range(1, 5)], (2, 6)),
}


def world_case(name: str, believed_extra: bool = True) -> dict:
    """The believed and the true map of a case of tests/test_gpu_episodes_world.py
    and tests/test_episodes_world_cpu.py, and its 16 starts.  believed_extra:
    the believed map holds one cell occupied that the world has free; then the
    starts are 14 cells in columns 0..2, the world's goal and that cell, else
    16 cells in columns 0..2 over an all-free believed map."""
    H, W, goal, wgoal, wall, extra = _CASES[name]
    believed = np.zeros((H, W), np.uint8)
    world = np.zeros((H, W), np.uint8)
    for x, y in wall:
        world[y, x] = 1
    n = 16
    if believed_extra:
        believed[extra[1], extra[0]] = 1
        n = 14
    starts = [(e * 5 % H) * W + e % 3 for e in range(n)]
    if believed_extra:
        starts += [wgoal[1] * W + wgoal[0], extra[1] * W + extra[0]]
    return {"believed": believed, "world": world, "goal": goal, "world_goal": wgoal,
            "starts": np.array(starts, np.int32), "seed": WORLD_SEED, "horizon": WORLD_HORIZON,
            "gamma": WORLD_GAMMA}


def pocket_world(case: dict) -> np.ndarray:
    """The case's world with cell (0, 0) walled in: (1, 0) and (0, 1) occupied,
    so a robot there sees all four sides blocked (z = 15 with probability 0.92),
    an observation that no cell of the believed map makes likely."""
    w = case["world"].copy()
    w[0, 1] = w[1, 0] = 1
    return w


# A b0 whose first update underflows for an unlikely observation only: 2^-125 on
# every believed-free cell.  raw = L_z * pred <= 2^-125 * max L_z flushes to zero
# everywhere when no believed cell gives z a likelihood >= 1/2 -- status 2 at
# step 1 -- and is rescaled to [1, 2) otherwise.
def tiny_b0(believed: np.ndarray) -> np.ndarray:
    return np.where(believed.reshape(-1) == 0, np.float32(2.0 ** -125), np.float32(0.0))
