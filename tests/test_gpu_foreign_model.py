"""GPU: the policy evaluator and the forward occupancy on uploaded models that
their TILES routes admit (tests/foreign_model_cases.py): 16 pair classes per
action, sub-stochastic rows that point off the grid and across tile edges, a
row sum exactly at the 1 + 2^-20 bound, entries around 2^-126, costs up to
1e30 -- and on the two that exactly one rule refuses (a 17th class, a row sum
of 1 + 2^-19).  Every field comparison is on uint32 views against
tests/policy_reference.py and tests/occupancy_reference.py: include/pp2.h
promises that PLANES and TILES return identical bits, and the references
restate its flush-to-zero fp32 arithmetic.  The models go into fresh contexts
(halo rows all zero, which is type 0 of every kind).
"""
import ctypes as C

import numpy as np
import pytest

import foreign_model_cases as FM
import occupancy_reference as OR
import policy_reference as R
from conftest import GAMMA

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
PLANES, TILES = 1, 2
SEED = 3


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@pytest.fixture(scope="module")
def geo(pp2):
    with pp2.GridContext(np.zeros((2, 2), np.uint8), (0, 0)) as ctx:
        info = ctx.policy_info()
        occ = ctx.occupancy_info()
    assert not info["valid"] and info["launches"] == 0
    assert 1 <= info["default_block"] <= info["max_block"]
    assert not occ["valid"] and 1 <= occ["default_block"] <= occ["max_block"]
    for k in ("tile_rows", "tile_cols"):
        assert occ[k] == info[k], k
    assert (info["tile_rows"], info["tile_cols"]) == FM.TILE, "foreign_model_cases.TILE"
    info["occ_default_block"], info["occ_max_block"] = occ["default_block"], occ["max_block"]
    return info


def assert_bits(got, want, what, names="GPN"):
    for g, w, name in zip(got, want, names):
        assert g.shape == w.shape, f"{what} {name}: shape {g.shape} vs {w.shape}"
        np.testing.assert_array_equal(R.bits(g), R.bits(w), err_msg=f"{what} {name}")


OCC = ("D", "V", "curve")


def expect(status, fn, *args, **kw):
    import path_planning_2d_amd as P
    with pytest.raises(P.Pp2Error) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)


def shape_of(key, geo):
    tr, tc = geo["tile_rows"], geo["tile_cols"]
    return {"four": (tr + 1, tc + 1), "two": (tr, tc + 9), "5x7": (5, 7)}[key]


def goal_of(key, H, W, geo):
    tr, tc = geo["tile_rows"], geo["tile_cols"]
    return {"tile_end": (min(tc, W) - 1, min(tr, H) - 1), "corner": (0, 0), "off": (-1, -1)}[key]


def on_grid(goal, H, W):
    return 0 <= goal[0] < W and 0 <= goal[1] < H


def upload(ctx, m, what):
    """Into the context, and back out bit for bit."""
    ctx.model_upload(*m)
    for got, sent, name in zip(ctx.model_download(), m, "TLRC"):
        np.testing.assert_array_equal(R.bits(got), R.bits(sent), err_msg=f"{what}: download {name}")


def case(H, W, kind, goal):
    """(model, covering table) of a kind; the tiny kind's two cells by the
    goal take an action whose support points at it."""
    m = FM.build(H, W, kind, SEED, goal=goal)
    types = FM.type_map(H, W, kind, SEED, goal)
    pi = FM.covering_table(types, 5)
    if kind == "tiny" and on_grid(goal, H, W):
        (x1, y1, a1), (x2, y2, a2) = FM.tiny_cells(H, W, goal)
        pi[y1, x1], pi[y2, x2] = a1[0], a2[-1]
    if H * W >= 9 * 9 * (types.max() + 1):
        for t in range(types.max() + 1):
            used = set(pi[types == t].tolist())
            assert len(used) >= 8, f"type {t} uses {used}"
    return m, pi


def leaking_border_cell(T, pi, H, W):
    """(x, y) of a border cell whose row under pi has weight off the grid."""
    Tu = OR._rows(T, pi, H, W)
    for y in range(H):
        for x in range(W):
            if 0 < y < H - 1 and 0 < x < W - 1:
                continue
            for i in range(9):
                yy, xx = y + i // 3 - 1, x + i % 3 - 1
                if not (0 <= yy < H and 0 <= xx < W) and Tu[y, x, i] > 0:
                    return x, y
    raise AssertionError("no border cell leaks")


def random_b0(H, W, seed):
    """A random field with entries of exactly 2^-126, of +0 and of 1."""
    rng = np.random.default_rng([seed, H, W])
    b = rng.random((H, W)).astype(np.float32)
    pick = rng.random((H, W))
    b[pick < 0.15] = FM.T126
    b[pick > 0.9] = 0.0
    b.reshape(-1)[rng.integers(0, H * W)] = 1.0
    assert (R.bits(b) == R.bits(FM.T126)).any()
    return b


def starts(T, pi, H, W, seed, hot=True):
    """b0 in two forms: a one-hot on a leaking border cell, and the random field."""
    out = {"random": random_b0(H, W, seed)}
    if hot:
        x, y = leaking_border_cell(T, pi, H, W)
        out["one-hot"] = np.zeros((H, W), np.float32)
        out["one-hot"][y, x] = 1.0
    return out


def launch_horizons(B):
    """Both sides of a launch boundary of block B."""
    return sorted({1, B, B + 1, 2 * B + 1})


PARTS = ("policy", "one-hot", "random")


def check_all_routes(ctx, m, pi, table, goal, H, W, geo, what, long=True, auto=None,
                     parts=PARTS):
    """PLANES and TILES == the references, for the evaluator ("policy") and the
    occupancy from each form of b0.  long: blocks {1, default, max} and
    horizons {1, B, B + 1, 2 B + 1} of each evaluator's default block B; else
    the default block and B + 1."""
    T, _, _, Cc = m
    B, Bmax = geo["default_block"], geo["max_block"]
    for h in (launch_horizons(B) if long else [B + 1]) if "policy" in parts else []:
        want = R.evaluate(T, Cc, pi, GAMMA, goal, H, W, h)
        ctx.policy_evaluate(h, table=table, route="planes")
        info = ctx.policy_info()
        assert info["route_taken"] == PLANES and info["launches"] == 1 + h
        assert_bits(ctx.policy_get(), want, f"{what} H={h} planes")
        for b in sorted({1, B, Bmax}) if long else [B]:
            ctx.policy_evaluate(h, table=table, route="tiles", block=b)
            info = ctx.policy_info()
            assert info["valid"] and info["horizon"] == h
            assert info["route_taken"] == TILES and info["block"] == b
            assert info["launches"] == 2 + (h + b - 1) // b
            assert_bits(ctx.policy_get(), want, f"{what} H={h} tiles block {b}")
    if auto is not None and "policy" in parts:
        ctx.policy_evaluate(h, table=table, route="auto")
        assert ctx.policy_info()["route_taken"] == auto
        assert_bits(ctx.policy_get(), want, f"{what} auto")
    B, Bmax = geo["occ_default_block"], geo["occ_max_block"]
    for bname, b0 in starts(T, pi, H, W, 17, "one-hot" in parts).items():
        if bname not in parts:
            continue
        for h in launch_horizons(B) if long else [B + 1]:
            wocc = OR.evaluate(T, pi, goal, b0, H, W, h)
            ctx.occupancy_evaluate(h, b0, table=table, route="planes")
            info = ctx.occupancy_info()
            assert info["route_taken"] == PLANES and info["launches"] == 2 + h
            assert_bits(ctx.occupancy_get(), wocc, f"{what} {bname} H={h} planes", OCC)
            for b in sorted({1, B, Bmax}) if long else [B]:
                ctx.occupancy_evaluate(h, b0, table=table, route="tiles", block=b)
                info = ctx.occupancy_info()
                assert info["valid"] and info["horizon"] == h
                assert info["route_taken"] == TILES and info["block"] == b
                assert info["launches"] == 2 + (h + b - 1) // b
                assert_bits(ctx.occupancy_get(), wocc, f"{what} {bname} H={h} tiles block {b}", OCC)
        if auto is not None:
            ctx.occupancy_evaluate(h, b0, table=table, route="auto")
            assert ctx.occupancy_info()["route_taken"] == auto
            assert_bits(ctx.occupancy_get(), wocc, f"{what} {bname} auto", OCC)


# ---------------------------------------------------------------- 1. the admitted kinds
CASES = [(k, s) for k in ("classes16", "leak") for s in ("four", "two", "5x7")] + \
        [(k, "four") for k in ("bound_at", "tiny", "big_cost")]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("gkey", ["tile_end", "corner", "off"])
@pytest.mark.parametrize("kind,skey", CASES)
def test_admitted_kinds(pp2, geo, kind, skey, gkey, part):
    """The evaluator, and the occupancy from a one-hot on a leaking border cell
    and from a random field with entries of 2^-126: both routes, blocks {1,
    default, max}, horizons on both sides of a launch boundary, bit for bit;
    AUTO takes TILES.  classes16 also under the table its own coded sweep
    chooses.

    [tiny-*-random] is where the flush has to follow the rounding: b0 = 2^-126
    times T = 1 - 2^-24 is 2^-126 - 2^-150 exactly, which rounds to 2^-126 and
    stays, while a flush decided on the unrounded value gives +0 (what the
    hardware's flush mode does; the evaluators flush in code for that reason).
    Both routes did so alike, so only the reference could tell."""
    H, W = shape_of(skey, geo)
    goal = goal_of(gkey, H, W, geo)
    m, pi = case(H, W, kind, goal)
    with pp2.GridContext(np.zeros((H, W), np.uint8), goal, gamma=float(GAMMA)) as ctx:
        upload(ctx, m, kind)
        entries, active = ctx.model_dict_info()
        assert active and 2 <= entries <= 40, (entries, active)
        ctx.policy_set_table(pi)
        check_all_routes(ctx, m, pi, "user", goal, H, W, geo, f"{kind} {skey} {gkey}", auto=TILES,
                         parts=(part,))
        if kind == "classes16" and part != "one-hot":
            ctx.mdp_sweep(12)
            A = ctx.mdp_get()[1].reshape(H, W)
            check_all_routes(ctx, m, A, "mdp", goal, H, W, geo, f"{kind} {skey} {gkey} mdp",
                             long=False, auto=TILES, parts=(part,))
        if kind == "tiny" and part == "policy" and on_grid(goal, H, W):
            (x1, y1, _), (x2, y2, _) = FM.tiny_cells(H, W, goal)
            ctx.policy_evaluate(1, table="user", route="tiles")
            G, P, _ = ctx.policy_get()
            assert R.bits(P[y1, x1]) == R.bits(FM.T126) and R.bits(G[y1, x1]) == 0
            assert R.bits(P[y2, x2]) == 0


# ---------------------------------------------------------------- 2. routing edges
@pytest.mark.parametrize("kind", ["classes17", "bound_over"])
def test_refused_kinds_take_planes(pp2, geo, kind):
    """One class too many, or one row sum of 1 + 2^-19: TILES is PP2_ESTATE for
    both evaluators and leaves the earlier result and *_info() as they were;
    AUTO takes PLANES and equals the reference."""
    H, W = shape_of("four", geo)
    goal = goal_of("tile_end", H, W, geo)
    m, pi = case(H, W, kind, goal)
    T, _, _, Cc = m
    h = geo["default_block"] + 1
    b0 = random_b0(H, W, 17)
    with pp2.GridContext(np.zeros((H, W), np.uint8), goal, gamma=float(GAMMA)) as ctx:
        upload(ctx, m, kind)
        assert ctx.model_dict_info()[0] >= 2
        ctx.policy_set_table(pi)
        ctx.policy_evaluate(h, table="user", route="auto")
        ctx.occupancy_evaluate(h, b0, table="user", route="auto")
        pol, occ = ctx.policy_get(), ctx.occupancy_get()
        pinfo, oinfo = ctx.policy_info(), ctx.occupancy_info()
        assert pinfo["route_taken"] == PLANES and oinfo["route_taken"] == PLANES
        assert_bits(pol, R.evaluate(T, Cc, pi, GAMMA, goal, H, W, h), f"{kind} auto")
        assert_bits(occ, OR.evaluate(T, pi, goal, b0, H, W, h), f"{kind} auto", OCC)
        for b in (0, 1, geo["max_block"]):
            expect(ESTATE, ctx.policy_evaluate, 3, table="user", route="tiles", block=b)
            expect(ESTATE, ctx.occupancy_evaluate, 3, b0, table="user", route="tiles", block=b)
        assert ctx.policy_info() == pinfo and ctx.occupancy_info() == oinfo
        assert_bits(ctx.policy_get(), pol, f"{kind} after the refusal")
        assert_bits(ctx.occupancy_get(), occ, f"{kind} after the refusal", OCC)


# ---------------------------------------------------------------- 3. an uploaded world
def world_case(pp2, geo):
    from path_planning_2d_amd import synthetic as S
    H, W = shape_of("two", geo)
    goal, wgoal = (W - 3, H // 2), (geo["tile_cols"], H // 2 + 1)
    grid = S.synth_grid(H, W, 7)
    grid[goal[1], goal[0]] = 0
    return H, W, grid, goal, wgoal


def test_uploaded_world(pp2, geo):
    """The table is the context's (a generated model's MDP solution); the robot
    moves in a second context that holds `leak`, with another goal."""
    H, W, grid, goal, wgoal = world_case(pp2, geo)
    h = 2 * geo["default_block"] + 1
    m = FM.build(H, W, "leak", SEED)
    T, _, _, Cc = m
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(np.zeros((H, W), np.uint8), wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        ctx.mdp_solve()
        pi = ctx.mdp_get()[1].reshape(H, W)
        upload(w, m, "the world")
        assert w.model_dict_info()[1]
        b0 = random_b0(H, W, 23)
        want = R.evaluate(T, Cc, pi, GAMMA, wgoal, H, W, h)
        wocc = OR.evaluate(T, pi, wgoal, b0, H, W, h)
        for route, taken in (("auto", TILES), ("planes", PLANES), ("tiles", TILES)):
            ctx.policy_evaluate(h, table="mdp", world=w, route=route)
            assert ctx.policy_info()["route_taken"] == taken
            assert_bits(ctx.policy_get(), want, f"world, route {route}")
            ctx.occupancy_evaluate(h, b0, table="mdp", world=w, route=route)
            assert ctx.occupancy_info()["route_taken"] == taken
            assert_bits(ctx.occupancy_get(), wocc, f"world, route {route}", OCC)
        own = ctx.model_download()
        ctx.policy_evaluate(h, table="mdp")
        assert_bits(ctx.policy_get(), R.evaluate(own[0], own[3], pi, GAMMA, goal, H, W, h),
                    "world = NULL")
        assert not np.array_equal(R.bits(ctx.policy_get()[1]), R.bits(want[1]))


def test_uploaded_world_on_its_own_stream(pp2, geo):
    """The world's model replaced on the world's stream right before the
    evaluation: the evaluation sees the new one."""
    from path_planning_2d_amd import _lib
    hip = _lib.load()  # the HIP runtime's symbols, through the library that links it
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    H, W, grid, goal, wgoal = world_case(pp2, geo)
    h = 2 * geo["default_block"] + 1  # past a launch of either evaluator
    first, m = FM.build(H, W, "classes16", SEED), FM.build(H, W, "leak", SEED)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(np.zeros((H, W), np.uint8), wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        ctx.mdp_solve()
        pi = ctx.mdp_get()[1].reshape(H, W)
        b0 = random_b0(H, W, 23)
        upload(w, first, "the first world")
        ctx.policy_evaluate(h, table="mdp", world=w)
        ctx.occupancy_evaluate(h, b0, table="mdp", world=w)
        before = ctx.policy_get()
        try:
            w.set_stream(stream.value)
            w.model_upload(*m)
            ctx.policy_evaluate(h, table="mdp", world=w, route="tiles")
            ctx.occupancy_evaluate(h, b0, table="mdp", world=w, route="tiles")
            pol, occ = ctx.policy_get(), ctx.occupancy_get()
        finally:
            w.synchronize()
            w.set_stream(None)
            assert hip.hipStreamDestroy(stream) == 0
        assert_bits(pol, R.evaluate(m[0], m[3], pi, GAMMA, wgoal, H, W, h), "the second world")
        assert_bits(occ, OR.evaluate(m[0], pi, wgoal, b0, H, W, h), "the second world", OCC)
        assert not np.array_equal(R.bits(pol[0]), R.bits(before[0]))


# ---------------------------------------------------------------- 4. the model replaced
def test_model_replaced_under_the_evaluator(pp2, geo):
    """classes16, then leak uploaded over it, then a generated model: every
    evaluation is of the model in force -- no class byte, row or table of the
    one before survives."""
    from path_planning_2d_amd import synthetic as S
    H, W = shape_of("four", geo)
    goal = goal_of("tile_end", H, W, geo)
    grid = S.synth_grid(H, W, 13)
    grid[goal[1], goal[0]] = 0
    first, pi = case(H, W, "classes16", goal)
    second = FM.build(H, W, "leak", SEED)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.policy_set_table(pi)
        results = []
        for name, m in (("classes16", first), ("leak over it", second), ("generated", None)):
            if m is None:
                ctx.model_generate()
                m = ctx.model_download()
            else:
                upload(ctx, m, name)
            assert ctx.model_dict_info()[1]
            check_all_routes(ctx, m, pi, "user", goal, H, W, geo, name, long=False, auto=TILES,
                             parts=PARTS if name != "generated" else ("policy", "random"))
            results.append(ctx.policy_get())
        assert not np.array_equal(R.bits(results[0][0]), R.bits(results[1][0]))
        assert not np.array_equal(R.bits(results[1][0]), R.bits(results[2][0]))


# ---------------------------------------------------------------- 5. adjoint on a leaking model
def test_adjoint_on_leak(pp2, geo):
    """<b0, P_H> = curve[H] and <b0, N_H> = sum V on sub-stochastic rows, where
    both sides of the first fall below 1: mass that one route kept and the
    other lost would part them.  The sums in fp64 on the host; each side is H
    steps of at most ten roundings on non-negative terms: relative tolerance
    2 * H * 10 * 2^-24, as tests/test_gpu_occupancy.py has it."""
    H, W = shape_of("four", geo)
    goal = goal_of("tile_end", H, W, geo)
    h = 2 * geo["default_block"] + 1
    m, pi = case(H, W, "leak", goal)
    b0 = np.zeros((H, W), np.float32)
    b0[goal[1] - 3:goal[1] + 2, goal[0] - 3:goal[0] + 2] = 1.0  # across both tile edges
    b0[goal[1], goal[0]] = 0.0
    b0 /= b0.sum()
    tol = 2 * h * 10 * 2.0 ** -24
    with pp2.GridContext(np.zeros((H, W), np.uint8), goal, gamma=float(GAMMA)) as ctx:
        upload(ctx, m, "leak")
        ctx.policy_set_table(pi)
        for proute, oroute in (("tiles", "tiles"), ("planes", "tiles"), ("tiles", "planes")):
            ctx.policy_evaluate(h, table="user", route=proute)
            _, P, N = ctx.policy_get()
            ctx.occupancy_evaluate(h, b0, table="user", route=oroute)
            _, V, curve = ctx.occupancy_get()
            b = b0.astype(np.float64)
            bp, bn = float((b * P).sum()), float((b * N).sum())
            arrived, visits = float(curve[h]), float(V.astype(np.float64).sum())
            print(f"{proute}/{oroute}: <b0,P> {bp!r} curve[H] {arrived!r}; "
                  f"<b0,N> {bn!r} sum V {visits!r}")
            assert 0 < bp < 1 and 1 <= bn < h
            assert abs(arrived - bp) <= tol * bp
            assert abs(visits - bn) <= tol * bn
