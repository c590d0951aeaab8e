"""CPU: tests/foreign_model_cases.py keeps its own promises -- the uploaded
models that tests/test_gpu_foreign_model.py feeds the evaluators are what
their names say, so a mismatch on the device cannot be blamed on the inputs.
The class count is keyed exactly as dict_props (csrc/pp2_dict_props.h) keys
it; the `tiny` kind's two intended effects are asserted on the reference
restatements alone.
"""
import numpy as np
import pytest

import foreign_model_cases as FM
import occupancy_reference as OR
import policy_reference as PR
from conftest import GAMMA

TR, TC = FM.TILE
SHAPES = [(TR + 1, TC + 1), (TR, TC + 9), (5, 7)]
FLT_MAX = float(np.finfo(np.float32).max)
BOUND = 1.0 + 2.0 ** -20


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=FM.KINDS)
def kind(request):
    return request.param


@pytest.mark.parametrize("shape", SHAPES)
def test_values_support_and_bounds(kind, shape):
    H, W = shape
    T, L, R, C = FM.build(H, W, kind, 3)
    assert T.shape == (H * W, 9, 9) and L.shape == (H * W, 16)
    assert R.shape == (H * W, 9) and C.shape == (H * W, 9)
    assert all(a.dtype == np.float32 for a in (T, L, R, C))
    for a in range(9):
        off = [i for i in range(9) if i not in FM.SUP[a]]
        assert not bits(T[:, a, off]).any(), f"action {a}: off-support bits"
    for name, a in (("T", T), ("C", C), ("L", L)):
        assert (bits(a) < 0x7f800000).all(), f"{name}: sign or finiteness"
    assert (bits(L) == bits(L.reshape(-1)[:1])).all() and L[0, 0] > 0
    assert np.isfinite(R).all()
    assert float(C.max()) / (1.0 - float(GAMMA)) < FLT_MAX / 2
    cells = np.unique(np.concatenate([T.reshape(H * W, 81), L, R, C], axis=1).view(np.uint32),
                      axis=0)
    assert len(cells) + 1 <= 40 < 400
    # the same seed gives the same bits, another seed another model
    again = FM.build(H, W, kind, 3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((T, L, R, C), again))
    assert not np.array_equal(bits(T), bits(FM.build(H, W, kind, 4)[0]))


def test_classes_per_action(kind):
    H, W = SHAPES[0]
    T, _, _, C = FM.build(H, W, kind, 3)
    counts = FM.class_counts(T, C, GAMMA)
    if kind == "classes16":
        assert counts == [16] * 9
    elif kind == "classes17":
        assert counts == [16, 16, 17, 16, 16, 16, 16, 16, 16]
    else:
        assert max(counts) <= 16 and min(counts) >= 2, counts
    # the all-zero type is the halo's class: counting the halo adds none
    assert FM.class_counts(T, C, GAMMA, halo=False) == counts


def test_classes17_is_classes16_plus_one_type():
    H, W = SHAPES[0]
    a = FM.build(H, W, "classes16", 3)
    b = FM.build(H, W, "classes17", 3)

    def cell_set(m):
        return {r.tobytes() for r in np.concatenate([m[0].reshape(H * W, 81), m[3]], axis=1)}
    assert len(cell_set(a)) == 16 and len(cell_set(b)) == 17
    assert cell_set(a) < cell_set(b)
    over = FM.build(H, W, "bound_over", 3)
    at = FM.build(H, W, "bound_at", 3)
    assert cell_set(at) < cell_set(over) and len(cell_set(over)) == len(cell_set(at)) + 1
    assert FM.class_counts(over[0], over[3], GAMMA)[6] == FM.class_counts(at[0], at[3], GAMMA)[6] + 1


def test_row_sums(kind):
    H, W = SHAPES[0]
    T = FM.build(H, W, kind, 3)[0]
    s = T.astype(np.float64).sum(axis=2)  # exact: at most four terms of few bits
    quad = np.sort(T.reshape(-1, 9), axis=1)[:, -4:]

    def has(row):
        return bool((bits(quad) == bits(np.sort(np.array(row, np.float32)))).all(axis=1).any())
    if kind == "bound_over":
        assert s.max() == 1.0 + 2.0 ** -19 and has([0.5, 0.5, FM.B19, 0.0])
        assert ((s > BOUND).sum(axis=1) <= 1).all() and (s > BOUND).any(axis=1).mean() < 0.2
    else:
        assert (s <= BOUND).all()
        assert not has([0.5, 0.5, FM.B19, 0.0])
    if kind in ("bound_at", "bound_over"):
        assert has([0.5, 0.5, FM.B20, 0.0]) and (s == BOUND).any()
    if kind in ("classes16", "classes17", "big_cost"):
        zero = ~T.reshape(H * W, -1).any(axis=1)
        assert zero.any() and (s[~zero] == 1.0).all(), "distributions, the zero type apart"
    if kind == "leak":
        C = FM.build(H, W, kind, 3)[3]
        assert (s < 1.0).all()
        zero = ~T.reshape(H * W, -1).any(axis=1)
        assert (zero & (C > 0).all(axis=1)).any(), "all-zero rows with C > 0"
    if kind == "tiny":
        C = FM.build(H, W, kind, 3)[3]
        on = np.concatenate([T[:, a, list(FM.SUP[a])].reshape(-1) for a in range(9)])
        assert set(bits(on).tolist()) == {int(bits(v)[0]) for v in FM.TINY_T} | {0}
        assert set(bits(C).reshape(-1).tolist()) == {int(bits(v)[0]) for v in FM.TINY_C}
    if kind == "big_cost":
        C = FM.build(H, W, kind, 3)[3]
        assert C.max() == np.float32(1e30) and (C == 0).any()


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_every_type_at_every_edge(kind, shape):
    """Every type -- hence every class of every action -- occurs in the
    interior, on all four borders and in the two columns and rows either side
    of every tile edge; the covering table then uses every (action, class)."""
    H, W = shape
    types = FM.type_map(H, W, kind, 3)
    every = set(range(types.max() + 1))
    T, _, _, C = FM.build(H, W, kind, 3)
    assert len(every) == len({r.tobytes() for r in
                              np.concatenate([T.reshape(H * W, 81), C], axis=1)})
    places = {"interior": types[1:-1, 1:-1], "top": types[0], "bottom": types[-1],
              "left": types[:, 0], "right": types[:, -1]}
    for x in range(TC, W, TC):
        places[f"columns at {x}"] = types[:, x - 2:x]
        places[f"columns from {x}"] = types[:, x:x + 2]
    for y in range(TR, H, TR):
        places[f"rows at {y}"] = types[y - 2:y]
        places[f"rows from {y}"] = types[y:y + 2]
    for name, part in places.items():
        assert set(part.reshape(-1).tolist()) == every, name
    assert len(places) >= (7 if shape == SHAPES[1] else 9)
    pi = FM.covering_table(types, 5)
    assert pi.dtype == np.uint8 and pi.max() <= 8
    for t in every:
        assert set(pi[types == t].tolist()) == set(range(9)), f"type {t}"
    if kind == "leak":
        # weight towards neighbours off the grid, and across a tile edge
        Tu = T.reshape(H, W, 9, 9)[np.arange(H)[:, None], np.arange(W)[None, :], pi]
        assert Tu[0, :, 0:3].any() and Tu[-1, :, 6:9].any()
        assert Tu[:, 0, 0::3].any() and Tu[:, -1, 2::3].any()
        assert Tu[:, TC - 1, 2::3].any() and Tu[:, TC, 0::3].any()


def test_tiny_effects_on_the_reference():
    """P == 2^-126 with G == +0 at the cell beside the goal (fl(gamma * 2^-126)
    is subnormal and flushed; the weight itself is normal), and a 2^-127 weight
    reads as zero -- in the evaluator and, as arriving mass, in the occupancy."""
    H, W = 5, 7
    sub = np.float32(GAMMA) * FM.T126
    assert 0 < sub < FM.T126, "gamma * 2^-126 is subnormal under IEEE arithmetic"
    seen_flush = 0
    for goal in [(3, 2), (0, 0), (6, 4), (2, 4)]:
        T, _, _, C = FM.build(H, W, "tiny", 3, goal=goal)
        types = FM.type_map(H, W, "tiny", 3, goal)
        (x1, y1, a1), (x2, y2, a2) = FM.tiny_cells(H, W, goal)
        assert abs(x1 - goal[0]) + abs(y1 - goal[1]) == 1
        assert abs(x2 - goal[0]) + abs(y2 - goal[1]) == 1
        assert types[y1, x1] == FM.TINY_TO and types[y2, x2] == FM.TINY_HALF
        assert len(a1) == 3 and len(a2) == 3
        for k in range(3):
            pi = FM.covering_table(types, 5)
            pi[y1, x1], pi[y2, x2] = a1[k], a2[2 - k]
            # the other neighbours that the first cell's row reaches: their dearest action
            for i in FM.SUP[a1[k]]:
                y, x = y1 + i // 3 - 1, x1 + i % 3 - 1
                if 0 <= y < H and 0 <= x < W and (x, y) not in ((x1, y1), (x2, y2), goal):
                    pi[y, x] = np.argmax(C[y * W + x])
            i1 = (goal[1] - y1 + 1) * 3 + goal[0] - x1 + 1
            i2 = (goal[1] - y2 + 1) * 3 + goal[0] - x2 + 1
            assert bits(T[y1 * W + x1, pi[y1, x1], i1]) == bits(FM.T126)
            assert bits(T[y2 * W + x2, pi[y2, x2], i2]) == bits(FM.T127)
            G1, P, N = PR.evaluate(T, C, pi, GAMMA, goal, H, W, 1)
            assert bits(P[y1, x1]) == bits(FM.T126) and bits(G1[y1, x1]) == 0 and N[y1, x1] == 1
            assert bits(P[y2, x2]) == 0 and bits(G1[y2, x2]) == 0
            # two steps: every neighbour's G is multiplied by a flushed
            # gamma * 2^-126, so G stays +0; kept subnormal, next to a cost of 1, it
            # would not
            G2 = PR.evaluate(T, C, pi, GAMMA, goal, H, W, 2)[0]
            assert bits(G2[y1, x1]) == 0
            near = [G1[y1 + i // 3 - 1, x1 + i % 3 - 1] for i in FM.SUP[pi[y1, x1]]
                    if 0 <= y1 + i // 3 - 1 < H and 0 <= x1 + i % 3 - 1 < W]
            seen_flush += max(near) >= 1
            for (x, y), arrived in (((x1, y1), FM.T126), ((x2, y2), np.float32(0))):
                b0 = np.zeros((H, W), np.float32)
                b0[y, x] = 1.0
                D, V, curve = OR.evaluate(T, pi, goal, b0, H, W, 1)
                assert bits(curve[1]) == bits(arrived)
                assert bits(D[goal[1], goal[0]]) == bits(arrived) and V[y, x] == 1.0
    assert seen_flush >= 1, "no case where an unflushed gamma * 2^-126 would have shown in G"
