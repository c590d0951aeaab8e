"""GPU: the policy evaluator (pp2_policy_*; kernels in csrc/pp2_policy.hip)
against the NumPy reference tests/policy_reference.py.  Every comparison is on
uint32 views: the definition is the bits, so there is no tolerance, and the
two routes (dense planes, LDS tiles of any block depth) must agree with it and
with each other.  Tile sizes and block depths come from policy_info().
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import path_reference as PR
import policy_reference as R
from conftest import GAMMA

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
PLANES, TILES = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@pytest.fixture(scope="module")
def geo(pp2):
    with pp2.GridContext(np.zeros((2, 2), np.uint8), (0, 0)) as ctx:
        info = ctx.policy_info()
    assert not info["valid"] and info["launches"] == 0
    assert 1 <= info["default_block"] <= info["max_block"]
    return info


def synth(H, W, seed, goal):
    from path_planning_2d_amd import synthetic as S
    g = S.synth_grid(H, W, seed)
    if 0 <= goal[0] < W and 0 <= goal[1] < H:
        g[goal[1], goal[0]] = 0
    return g


def model(ctx):
    T, _, _, Cc = ctx.model_download()
    return T, Cc


def assert_bits(got, want, what):
    for g, w, name in zip(got, want, "GPN"):
        np.testing.assert_array_equal(R.bits(g), R.bits(w), err_msg=f"{what} {name}")


def expect(status, fn, *args, **kw):
    import path_planning_2d_amd as P
    with pytest.raises(P.Pp2Error) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)


def random_table(H, W, seed):
    return np.random.default_rng(seed).integers(0, 9, (H, W)).astype(np.uint8)


# ---------------------------------------------------------------- 1. real maps
@pytest.mark.parametrize("name", ["map_3x3", "map_5x5", "map_10x10", "sparse_map_100x40"])
def test_golden_maps_both_tables(pp2, name):
    grid, goal = PR.golden_case(name)
    H, W = grid.shape
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        _, converged, _ = ctx.path_solve()
        assert converged
        T, Cc = model(ctx)
        pis = {"mdp": ctx.mdp_get()[1], "path": ctx.path_get()[1]}
        for table, pi in pis.items():
            for h in (1, 2, 40):
                ctx.policy_evaluate(h, table=table, route="auto")
                got = ctx.policy_get()
                info = ctx.policy_info()
                assert info["valid"] and info["horizon"] == h and info["route_taken"] == TILES
                assert_bits(got, R.evaluate(T, Cc, pi, GAMMA, goal, H, W, h), f"{name} {table} H={h}")


# ---------------------------------------------------------------- 2. tile and launch edges
SHAPES = ["tile", "tile+1", "1x7", "5x1", "33x65"]
GOALS = ["tile_end", "corner", "off"]


def shape_of(key, geo):
    tr, tc = geo["tile_rows"], geo["tile_cols"]
    return {"tile": (tr, tc), "tile+1": (tr + 1, tc + 1), "1x7": (1, 7), "5x1": (5, 1),
            "33x65": (33, 65)}[key]


@pytest.mark.parametrize("gkey", GOALS)
@pytest.mark.parametrize("skey", SHAPES)
def test_tile_and_launch_edges(pp2, geo, skey, gkey):
    """TILES at block 1, the default and the largest == PLANES == the reference,
    at horizons on both sides of a launch boundary, with the goal where a ring
    must pin it."""
    H, W = shape_of(skey, geo)
    tr, tc, B, Bmax = geo["tile_rows"], geo["tile_cols"], geo["default_block"], geo["max_block"]
    goal = {"tile_end": (min(tc, W) - 1, min(tr, H) - 1), "corner": (0, 0), "off": (-1, -1)}[gkey]
    grid = synth(H, W, 11 + H, goal)
    horizons = sorted({h for h in (1, B - 1, B, B + 1, 2 * B + 1) if h >= 1})
    pi = random_table(H, W, 5)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.policy_set_table(pi)
        T, Cc = model(ctx)
        for h in horizons:
            want = R.evaluate(T, Cc, pi, GAMMA, goal, H, W, h)
            ctx.policy_evaluate(h, table="user", route="planes")
            assert ctx.policy_info()["route_taken"] == PLANES
            assert_bits(ctx.policy_get(), want, f"{skey} {gkey} H={h} planes")
            for b in sorted({1, B, Bmax}):
                ctx.policy_evaluate(h, table="user", route="tiles", block=b)
                info = ctx.policy_info()
                assert info["route_taken"] == TILES and info["block"] == b
                assert info["launches"] == 2 + (h + b - 1) // b
                assert_bits(ctx.policy_get(), want, f"{skey} {gkey} H={h} tiles block {b}")
            if gkey == "off":
                G, P, N = want
                assert not R.bits(P).any(), "no goal: P is +0 everywhere"
                n64 = R.chain_f64(T, Cc, pi, GAMMA, goal, H, W, h)[2]
                stays = np.abs(n64 - h) < 1e-9 * h  # the chain cannot leave the grid from here
                assert stays.any()
                assert (np.abs(N[stays] - h) <= h * 10 * 2.0 ** -24 * h).all()


# ---------------------------------------------------------------- 3. dense path on a coded-off context
def test_coded_off_takes_planes(pp2, geo):
    H, W = geo["tile_rows"] + 1, geo["tile_cols"] + 1
    goal = (W - 2, H - 2)
    grid = synth(H, W, 3, goal)
    h = geo["default_block"] + 1
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.mdp_sweep(12)
        ctx.policy_evaluate(h, table="mdp", route="auto")
        assert ctx.policy_info()["route_taken"] == TILES
        coded = ctx.policy_get()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        ctx.policy_evaluate(h, table="mdp", route="auto")
        assert ctx.policy_info()["route_taken"] == PLANES
        assert_bits(ctx.policy_get(), coded, "coded off")
        expect(ESTATE, ctx.policy_evaluate, h, table="mdp", route="tiles")
        T, Cc = model(ctx)
        assert_bits(coded, R.evaluate(T, Cc, ctx.mdp_get()[1], GAMMA, goal, H, W, h), "reference")


# ---------------------------------------------------------------- 4. world
@pytest.fixture()
def world_case(geo):
    H, W = geo["tile_rows"], geo["tile_cols"] + 9  # two tiles
    goal, wgoal = (W - 3, H // 2), (W - 2, H // 2 + 1)
    grid = np.zeros((H, W), np.uint8)
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = 1
    wgrid = grid.copy()
    wgrid[4:H - 6, geo["tile_cols"] - 1] = 1  # the wall the believed map lacks, at the tile edge
    return H, W, grid, goal, wgrid, wgoal


def test_world_differs_from_the_map(pp2, geo, world_case):
    H, W, grid, goal, wgrid, wgoal = world_case
    h = 2 * geo["default_block"] + 1
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid, wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        w.model_generate()
        ctx.mdp_solve()
        pi = ctx.mdp_get()[1]
        Tw, Cw = model(w)
        want = R.evaluate(Tw, Cw, pi, GAMMA, wgoal, H, W, h)
        for route in ("auto", "planes", "tiles"):
            ctx.policy_evaluate(h, table="mdp", world=w, route=route)
            assert_bits(ctx.policy_get(), want, f"world, route {route}")
        own = R.evaluate(*model(ctx), pi, GAMMA, goal, H, W, h)
        assert not np.array_equal(R.bits(own[0]), R.bits(want[0]))
        ctx.policy_evaluate(h, table="mdp", world=None)
        a = ctx.policy_get()
        assert_bits(a, own, "world = NULL")
        ctx.policy_evaluate(h, table="mdp", world=ctx)
        assert_bits(ctx.policy_get(), a, "world = ctx")
    ulp = float(np.nextafter(np.float32(GAMMA), np.float32(1)))
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid, wgoal, gamma=ulp) as w:
        ctx.model_generate()
        w.model_generate()
        expect(EINVAL, ctx.policy_evaluate, 3, table="mdp", world=w)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid[:-1], wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        w.model_generate()
        expect(EINVAL, ctx.policy_evaluate, 3, table="mdp", world=w)


def test_world_on_its_own_stream(pp2, geo, world_case):
    """An update of the world enqueued on its stream right before the evaluation
    (no synchronise in between) is what the evaluation sees."""
    from path_planning_2d_amd import _lib
    hip = _lib.load()  # the HIP runtime's symbols, through the library that links it
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    H, W, grid, goal, wgrid, wgoal = world_case
    h = geo["default_block"] + 1
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    x = geo["tile_cols"] - 1
    opening = np.zeros((H - 10, 1), np.uint8)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid, wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        w.model_generate()
        ctx.mdp_solve()
        pi = ctx.mdp_get()[1]
        ctx.policy_evaluate(h, table="mdp", world=w)
        walled = ctx.policy_get()
        try:
            w.set_stream(stream.value)
            w.map_update(opening, x0=x, y0=4)
            ctx.policy_evaluate(h, table="mdp", world=w)
            opened = ctx.policy_get()
        finally:
            w.synchronize()
            w.set_stream(None)
            assert hip.hipStreamDestroy(stream) == 0
        Tw, Cw = model(w)
        assert_bits(opened, R.evaluate(Tw, Cw, pi, GAMMA, wgoal, H, W, h), "the opened world")
        assert not np.array_equal(R.bits(opened[0]), R.bits(walled[0]))


# ---------------------------------------------------------------- 5. USER table
def test_user_table(pp2):
    H, W = 33, 65
    goal = (40, 20)
    grid = synth(H, W, 9, goal)
    pi = random_table(H, W, 21)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        expect(ESTATE, ctx.policy_evaluate, 4, table="user")
        bad = pi.copy()
        bad[H - 1, W - 1] = 9
        expect(EINVAL, ctx.policy_set_table, bad)
        expect(ESTATE, ctx.policy_evaluate, 4, table="user")
        ctx.policy_set_table(pi)
        T, Cc = model(ctx)
        ctx.policy_evaluate(7, table="user")
        assert ctx.policy_info()["table"] == 2
        assert_bits(ctx.policy_get(), R.evaluate(T, Cc, pi, GAMMA, goal, H, W, 7), "user table")
        ctx.policy_set_table(None)
        expect(ESTATE, ctx.policy_evaluate, 4, table="user")


# ---------------------------------------------------------------- 6. refusals and state
def test_refusals_and_snapshot(pp2, geo):
    H, W = 12, 20
    goal = (15, 8)
    grid = synth(H, W, 2, goal)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        expect(ESTATE, ctx.policy_get)
        expect(ESTATE, ctx.policy_evaluate, 4, table="path")
        expect(EINVAL, ctx.policy_evaluate, 0)
        expect(EINVAL, ctx.policy_evaluate, 65537)
        expect(EINVAL, ctx.policy_evaluate, 4, block=geo["max_block"] + 1)
        expect(EINVAL, ctx.policy_evaluate, 4, block=-1)
        expect(EINVAL, ctx.policy_evaluate, 4, route=3)
        expect(EINVAL, ctx.policy_evaluate, 4, table=3)
        expect(ESTATE, ctx.policy_get)
        assert not ctx.policy_info()["valid"]
        ctx.mdp_sweep(10)
        pi = ctx.mdp_get()[1]
        T, Cc = model(ctx)
        ctx.policy_evaluate(6, table="mdp")
        first = ctx.policy_get()
        assert_bits(first, R.evaluate(T, Cc, pi, GAMMA, goal, H, W, 6), "first")
        # a snapshot: a map update does not touch it
        ctx.map_update(np.ones((3, 2), np.uint8), x0=4, y0=4)
        assert_bits(ctx.policy_get(), first, "after map_update")
        info = ctx.policy_info()
        assert info["valid"] and info["horizon"] == 6 and info["table"] == 0
        # ... and the next evaluation replaces it (the updated model, A as it stands)
        T2, C2 = model(ctx)
        ctx.policy_evaluate(3, table="mdp")
        assert ctx.policy_info()["horizon"] == 3
        assert_bits(ctx.policy_get(), R.evaluate(T2, C2, pi, GAMMA, goal, H, W, 3), "second")
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, 6)) as shard:
        shard.model_generate()
        expect(ESTATE, shard.policy_evaluate, 4)
        expect(ESTATE, shard.policy_set_table, np.zeros((6, W), np.uint8))


def test_evaluation_leaves_the_state_untouched(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = PR.golden_case("map_10x10")
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.belief_set(S.uniform_belief(grid))
        ctx.belief_update(1, 3)
        ctx.mdp_sweep(7)
        ctx.fib_reset()
        ctx.fib_sweep(3)
        ctx.path_solve()

        def state():
            b, m = ctx.belief_get_raw()
            J, A = ctx.mdp_get()
            D, Ap = ctx.path_get()
            return [R.bits(b), R.bits(np.float32(m)), R.bits(J), A, R.bits(D), Ap, R.bits(ctx.fib_get())]

        before = state()
        for table in ("mdp", "path"):
            for route in ("planes", "tiles"):
                ctx.policy_evaluate(9, table=table, route=route)
        ctx.policy_get()
        for a, b in zip(before, state()):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- 7. the example
def test_policy_eval_demo_runs(pp2):
    exe = os.path.join(ROOT, "examples", "pp2_policy_eval_demo")
    assert os.path.exists(exe), "build with make -C path_planning_2d_amd/csrc"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert "pp2_policy_eval_demo ok" in out.stdout
    assert "stale map, in the world" in out.stdout and "updated, in the world" in out.stdout
    printed = {}
    for m in re.finditer(r"^  table (mdp|path)\s+G (\S+) P (\S+) N (\S+)", out.stdout, re.M):
        printed[m.group(1)] = [np.float32(float.fromhex(m.group(k))) for k in (2, 3, 4)]
    assert sorted(printed) == ["mdp", "path"], out.stdout
    grid, goal = PR.golden_case("sparse_map_100x40")
    assert goal == (95, 34)
    with pp2.GridContext(grid, goal, gamma=0.95) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        ctx.path_solve()
        for table in ("mdp", "path"):
            ctx.policy_evaluate(200, table=table)
            got = [a[6, 11] for a in ctx.policy_get()]
            assert [int(R.bits(v)[0]) for v in got] == [int(R.bits(v)[0]) for v in printed[table]], \
                f"{table}: {got} vs {printed[table]}"
