"""NumPy builder of uploaded ("foreign") models that the TILES routes of the
policy evaluator and of the forward occupancy admit -- or refuse by exactly
one rule -- for tests/test_gpu_foreign_model.py; tests/
test_foreign_model_cpu.py holds the builder to what it promises here.

A generated model is narrow: 9 pair classes per action out of kFactK = 16,
rows that are probability distributions and never point off the grid, no entry
near 2^-126.  The models here are not.  Every cell has a *type* and every
action's row (its T on the action's support, C and R) is a function of the
type, so the dictionary has one entry per type (plus the all-zero halo rows,
which coincide with type 0 in every class key) and an action has at most as
many (fl(gamma T) quad, C, T quad) classes as there are types.

``build(H, W, kind, seed)`` returns (T[H*W,9,9], L[H*W,16], R[H*W,9],
C[H*W,9]) as float32, pp2_model_upload's layouts.  Kept for every kind: L
constant over the cells and > 0; T bit-exactly +0 off the action's support
(SUP, kSup of csrc/pp2_internal.h); every T and C entry finite with the sign
bit clear; max C / (1 - gamma) < FLT_MAX / 2; type 0 all-zero rows with C = +0.

The types lie on a lattice, type = perm[(x + p * y + s) mod n] with p coprime
to n: n consecutive cells of any row or column hold every type, so a grid at
least n + 2 cells each way has every type in its interior, on all four borders
and in the two columns (rows) either side of every tile edge (``TILE``, which
the GPU test checks against policy_info()).

Kinds:
  classes16   16 types, 16 distinct classes in every action; rows are
              distributions (type 0 apart)
  classes17   classes16 and one more type, a copy of type 5 but for action 2's
              cost: a 17th class in action 2 alone -- not factored
  leak        sub-stochastic rows with k/64 entries, some entries of the
              support +0; type 1 all-zero rows with C > 0.  On the lattice
              every type meets every border and tile edge, so rows put weight
              off the grid and across tile edges
  bound_at    distributions and one type whose four-entry rows are a
              permutation of {0.5, 0.5, 2^-20, 0}: fp64 sum exactly 1 + 2^-20
  bound_over  bound_at and one more type, a copy of that one with 2^-19 in
              action 6's row: sum 1 + 2^-19, refused by the row-sum rule alone
  tiny        support entries from TINY_T, C from TINY_C, row sums <= 1; type 1
              holds 2^-126 and type 2 holds 2^-127 on every support entry with
              C = +0.  With ``goal=`` on the grid the two cells of
              ``tiny_cells`` take those types
  big_cost    distributions, C up to 1e30 on some types and +0 on others
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
TILE = (32, 48)  # (rows, cols) of the evaluators' tile; the GPU test checks it
SUP = ((0, 1, 3, 4), (0, 1, 2, 4), (1, 2, 4, 5), (0, 3, 4, 6), (4,), (2, 4, 5, 8), (3, 4, 6, 7),
       (4, 6, 7, 8), (4, 5, 7, 8))
KINDS = ("classes16", "classes17", "leak", "bound_at", "bound_over", "tiny", "big_cost")
ADMITTED = ("classes16", "leak", "bound_at", "tiny", "big_cost")
L_VALUE = F32(0.0625)
T126, T127, T149 = F32(2.0 ** -126), F32(2.0 ** -127), F32(2.0 ** -149)
TINY_T = (T126, F32(1.5 * 2.0 ** -126), T127, T149, F32(0.5), F32(1.0 - 2.0 ** -24))
TINY_C = (F32(0.0), T126, F32(1.0))
B20, B19 = F32(2.0 ** -20), F32(2.0 ** -19)
TINY_TO, TINY_HALF = 1, 2  # the tiny kind's types of all-2^-126 and all-2^-127 rows


def _dist_quad(rng):
    """Four positive multiples of 1/64 that sum to exactly 1."""
    cuts = np.sort(rng.choice(np.arange(1, 64), 3, replace=False))
    k = np.diff(np.concatenate(([0], cuts, [64])))
    return (k / 64.0).astype(np.float32)


def _leak_quad(rng):
    """Multiples of 1/64, some +0, summing to less than 1."""
    k = rng.integers(0, 16, 4)
    k[rng.integers(0, 4)] = 0
    if k.sum() == 0:
        k[rng.integers(0, 4)] = 7
    return (k / 64.0).astype(np.float32)


def _tiny_quad(rng):
    while True:
        q = np.array([TINY_T[i] for i in rng.integers(0, len(TINY_T), 4)], np.float32)
        if q.astype(np.float64).sum() <= 1.0:
            return q


class _Types:
    """rows[t][a]: float32 on SUP[a]; cost[t][a]; type 0 all zero."""

    def __init__(self):
        self.rows, self.cost = [], []

    def add(self, rows, cost):
        assert len(rows) == 9 and len(cost) == 9
        self.rows.append([np.asarray(r, np.float32).copy() for r in rows])
        self.cost.append([F32(c) for c in cost])
        return len(self.rows) - 1

    def copy_of(self, t):
        return self.add(self.rows[t], self.cost[t])

    def key(self, t, a):
        return self.rows[t][a].tobytes() + self.cost[t][a].tobytes()

    def n(self):
        return len(self.rows)


def _zero_rows():
    return [np.zeros(len(SUP[a]), np.float32) for a in range(9)]


def _add_distinct(ty, rng, quad, costs, one=F32(1.0), stay_costs=None):
    """A type with quad() rows, costs drawn from `costs`, distinct from every
    earlier type in every action (action 4, one entry: by its cost)."""
    t = ty.n()
    for _ in range(1000):
        rows = [quad(rng) if len(SUP[a]) == 4 else np.array([one], np.float32) for a in range(9)]
        cost = [costs[rng.integers(0, len(costs))] for _ in range(9)]
        if stay_costs is not None:
            cost[4] = stay_costs[t]
        keys = [rows[a].tobytes() + F32(cost[a]).tobytes() for a in range(9)]
        if all(keys[a] != ty.key(s, a) for s in range(t) for a in range(9)):
            return ty.add(rows, cost)
    raise AssertionError("no distinct type found")


_FAMILY = {"classes17": "classes16", "bound_over": "bound_at"}


def _type_rng(kind, seed):
    """(classes17 and bound_over draw what classes16 and bound_at draw: they
    differ from them by the one added type)"""
    return np.random.default_rng([seed, KINDS.index(_FAMILY.get(kind, kind))])


def _types(kind, rng):
    ty = _Types()
    ty.add(_zero_rows(), [0.0] * 9)
    if kind in ("classes16", "classes17"):
        stay = [F32(0.25 * t) for t in range(16)]
        for _ in range(15):
            _add_distinct(ty, rng, _dist_quad, (F32(0.0), F32(0.5), F32(1.0), F32(3.0)),
                          stay_costs=stay)
        if kind == "classes17":
            t = ty.copy_of(5)
            ty.cost[t][2] = F32(7.0)
    elif kind == "leak":
        ty.add(_zero_rows(), [1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 0.25, 1.0, 2.0])
        stay = [F32(0.125 * t) for t in range(12)]
        for t in range(2, 12):
            _add_distinct(ty, rng, _leak_quad, (F32(0.0), F32(1.0), F32(2.5)),
                          one=F32((t * 5 % 64) / 64.0), stay_costs=stay)
    elif kind in ("bound_at", "bound_over"):
        stay = [F32(0.5 * t) for t in range(10)]
        for _ in range(6):
            _add_distinct(ty, rng, _dist_quad, (F32(0.0), F32(1.0)), stay_costs=stay)
        base = np.array([0.5, 0.5, B20, 0.0], np.float32)
        t = ty.add([rng.permutation(base) if len(SUP[a]) == 4 else np.ones(1, np.float32)
                    for a in range(9)], [1.0] * 4 + [stay[7]] + [1.0] * 4)
        if kind == "bound_over":
            o = ty.copy_of(t)
            ty.rows[o][6] = np.where(ty.rows[o][6] == B20, B19, ty.rows[o][6]).astype(np.float32)
    elif kind == "tiny":
        ty.add([np.full(len(SUP[a]), T126, np.float32) for a in range(9)], [0.0] * 9)
        ty.add([np.full(len(SUP[a]), T127, np.float32) for a in range(9)], [0.0] * 9)
        assert (TINY_TO, TINY_HALF) == (1, 2)
        for t in range(3, 14):
            for _ in range(1000):
                rows = [_tiny_quad(rng) if len(SUP[a]) == 4 else
                        np.array([TINY_T[rng.integers(0, len(TINY_T))]], np.float32)
                        for a in range(9)]
                cost = [TINY_C[rng.integers(0, 3)] for _ in range(9)]
                if all(rows[a].tobytes() + F32(cost[a]).tobytes() != ty.key(s, a)
                       for s in range(t) for a in (0, 1, 2, 3, 5, 6, 7, 8)):
                    break
            ty.add(rows, cost)
    elif kind == "big_cost":
        stay = [F32(0.0), F32(1e30), F32(1e29), F32(0.5), F32(3e28), F32(2.0), F32(1e30 / 3),
                F32(7.0), F32(1e20), F32(1e-3), F32(1e25), F32(4.0)]
        for _ in range(11):
            _add_distinct(ty, rng, _dist_quad, (F32(0.0), F32(1e30), F32(1.0), F32(1e15)),
                          stay_costs=stay)
    else:
        raise ValueError(f"unknown kind {kind!r}")
    return ty


def type_map(H, W, kind, seed, goal=None):
    """[H, W] type of every cell (what ``build`` lays its rows out by)."""
    rng = np.random.default_rng([seed, KINDS.index(kind), 1])
    n = _types(kind, _type_rng(kind, seed)).n()
    p = next(q for q in (5, 7, 3, 11, 13) if np.gcd(q, n) == 1)
    perm = rng.permutation(n)
    s = int(rng.integers(0, n))
    y, x = np.mgrid[0:H, 0:W]
    types = perm[(x + p * y + s) % n]
    if kind == "tiny" and goal is not None and _on(goal, H, W):
        (x1, y1, _), (x2, y2, _) = tiny_cells(H, W, goal)
        types[y1, x1] = TINY_TO
        types[y2, x2] = TINY_HALF
    return types


def _on(goal, H, W):
    return 0 <= goal[0] < W and 0 <= goal[1] < H


def tiny_cells(H, W, goal):
    """((x, y, actions), (x, y, actions)): the cell beside the goal that carries
    2^-126 towards it and the cell above or below that carries 2^-127, each
    with the actions whose support holds the entry that points at the goal."""
    gx, gy = goal
    assert _on(goal, H, W) and W >= 2 and H >= 2
    x1, i1 = (gx - 1, 5) if gx > 0 else (gx + 1, 3)
    y2, i2 = (gy - 1, 7) if gy > 0 else (gy + 1, 1)
    acts = lambda i: tuple(a for a in range(9) if i in SUP[a])  # noqa: E731
    return (x1, gy, acts(i1)), (gx, y2, acts(i2))


def build(H, W, kind, seed, goal=None):
    ty = _types(kind, _type_rng(kind, seed))
    types = type_map(H, W, kind, seed, goal).reshape(-1)
    n = ty.n()
    Tt = np.zeros((n, 9, 9), np.float32)
    Ct = np.zeros((n, 9), np.float32)
    for t in range(n):
        for a in range(9):
            Tt[t, a, list(SUP[a])] = ty.rows[t][a]
            Ct[t, a] = ty.cost[t][a]
    Rt = (-Ct * F32(0.5)).astype(np.float32) + F32(0.0)  # a function of the type; no -0
    T = np.ascontiguousarray(Tt[types])
    C = np.ascontiguousarray(Ct[types])
    R = np.ascontiguousarray(Rt[types])
    L = np.full((H * W, 16), L_VALUE, np.float32)
    return T, L, R, C


def class_counts(T, C, gamma, halo=True):
    """Distinct classes per action, keyed as dict_props keys them: fl(gamma T)
    on the support (rounded once, subnormals kept), C, raw T on the support;
    `halo` adds the all-zero halo cell."""
    T = np.asarray(T, np.float32).reshape(-1, 9, 9)
    C = np.asarray(C, np.float32).reshape(-1, 9)
    out = []
    for a in range(9):
        r = T[:, a, list(SUP[a])]
        q = (np.float32(gamma) * r).astype(np.float32)
        key = np.concatenate([q.view(np.uint32), C[:, a:a + 1].view(np.uint32), r.view(np.uint32)],
                             axis=1)
        if halo:
            key = np.concatenate([key, np.zeros((1, key.shape[1]), np.uint32)])
        out.append(len(np.unique(key, axis=0)))
    return out


def covering_table(types, seed):
    """[H, W] uint8 actions, random, that use all nine actions at every type
    with at least nine cells (a type with fewer gets distinct actions)."""
    rng = np.random.default_rng([seed, 77])
    types = np.asarray(types)
    pi = np.zeros(types.shape, np.uint8)
    for t in np.unique(types):
        at = np.flatnonzero(types.reshape(-1) == t)
        acts = np.concatenate([rng.permutation(9) for _ in range((len(at) + 8) // 9)])[:len(at)]
        pi.reshape(-1)[rng.permutation(at)] = acts
    return pi
