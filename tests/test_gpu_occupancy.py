"""GPU: the forward occupancy (pp2_occupancy_*; kernels in
csrc/pp2_occupancy.hip) against the NumPy reference tests/occupancy_reference.py.
Every field comparison is on uint32 views: the definition is the bits, so there
is no tolerance, and the two routes (weight planes, LDS tiles of any block
depth) must agree with it and with each other.  Tile sizes and block depths
come from occupancy_info().  launches, as include/pp2.h documents it: the start
planes, the class bytes or the weight planes, and ceil(horizon / block) steps.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import occupancy_reference as R
import path_reference as PR
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
        info = ctx.occupancy_info()
    assert not info["valid"] and info["launches"] == 0
    assert 1 <= info["default_block"] <= info["max_block"]
    return info


def synth(H, W, seed, goal):
    from path_planning_2d_amd import synthetic as S
    g = S.synth_grid(H, W, seed)
    if 0 <= goal[0] < W and 0 <= goal[1] < H:
        g[goal[1], goal[0]] = 0
    return g


def assert_bits(got, want, what):
    for g, w, name in zip(got, want, ("D", "V", "curve")):
        assert g.shape == w.shape, f"{what} {name}: shape {g.shape} vs {w.shape}"
        np.testing.assert_array_equal(R.bits(g), R.bits(w), err_msg=f"{what} {name}")


def expect(status, fn, *args, **kw):
    import path_planning_2d_amd as P
    with pytest.raises(P.Pp2Error) as e:
        fn(*args, **kw)
    assert e.value.status == status, str(e.value)


def random_table(H, W, seed):
    return np.random.default_rng(seed).integers(0, 9, (H, W)).astype(np.uint8)


def uniform_free(grid):
    free = grid == 0
    return (free / np.float32(free.sum())).astype(np.float32)


def one_hot(H, W, x, y):
    b = np.zeros((H, W), np.float32)
    b[y, x] = 1.0
    return b


# ---------------------------------------------------------------- 1. real maps
@pytest.mark.parametrize("name", ["map_3x3", "map_5x5", "map_10x10", "sparse_map_100x40"])
def test_golden_maps_both_tables(pp2, name):
    grid, goal = PR.golden_case(name)
    H, W = grid.shape
    free = [c for c in np.flatnonzero(grid.reshape(-1) == 0) if c != goal[1] * W + goal[0]]
    hot = int(free[len(free) // 3])
    starts = {"uniform": uniform_free(grid), "one-hot": one_hot(H, W, hot % W, hot // W)}
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        _, converged, _ = ctx.path_solve()
        assert converged
        T = ctx.model_download()[0]
        pis = {"mdp": ctx.mdp_get()[1], "path": ctx.path_get()[1]}
        for table, pi in pis.items():
            for bname, b0 in starts.items():
                for h in (1, 2, 40):
                    ctx.occupancy_evaluate(h, b0, table=table, route="auto")
                    got = ctx.occupancy_get()
                    info = ctx.occupancy_info()
                    assert info["valid"] and info["horizon"] == h and info["route_taken"] == TILES
                    assert_bits(got, R.evaluate(T, pi, goal, b0, H, W, h),
                                f"{name} {table} {bname} H={h}")


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
    must hold its mass, from a dense random b0 with mass on occupied cells and
    on the goal."""
    H, W = shape_of(skey, geo)
    tr, tc, B, Bmax = geo["tile_rows"], geo["tile_cols"], geo["default_block"], geo["max_block"]
    goal = {"tile_end": (min(tc, W) - 1, min(tr, H) - 1), "corner": (0, 0), "off": (-1, -1)}[gkey]
    grid = synth(H, W, 11 + H, goal)
    horizons = sorted({h for h in (1, B - 1, B, B + 1, 2 * B + 1) if h >= 1})
    pi = random_table(H, W, 5)
    b0 = np.random.default_rng(17 + W).random((H, W)).astype(np.float32)
    assert b0.max() <= 1.0 and (H * W < 20 or b0[grid == 1].sum() > 0)
    if gkey != "off":
        assert b0[goal[1], goal[0]] > 0
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.policy_set_table(pi)
        T = ctx.model_download()[0]
        for h in horizons:
            want = R.evaluate(T, pi, goal, b0, H, W, h)
            ctx.occupancy_evaluate(h, b0, table="user", route="planes")
            info = ctx.occupancy_info()
            assert info["route_taken"] == PLANES and info["launches"] == 2 + h
            assert_bits(ctx.occupancy_get(), want, f"{skey} {gkey} H={h} planes")
            for b in sorted({1, B, Bmax}):
                ctx.occupancy_evaluate(h, b0, table="user", route="tiles", block=b)
                info = ctx.occupancy_info()
                assert info["route_taken"] == TILES and info["block"] == b
                assert info["launches"] == 2 + (h + b - 1) // b
                assert_bits(ctx.occupancy_get(), want, f"{skey} {gkey} H={h} tiles block {b}")
            if gkey == "off":
                assert not R.bits(want[2]).any(), "no goal: the curve is +0 throughout"
            else:
                assert want[2][0] == b0[goal[1], goal[0]] and (np.diff(want[2]) >= 0).all()


# ---------------------------------------------------------------- 3. transposition probe
def test_transposition_probe(pp2, geo):
    """All the mass on the cell diagonally inside the corner where four tiles
    meet: after one step it lies where that cell's own row sends it -- a gather
    that read entry 8 - i, or the destination's row, puts it elsewhere.  At
    H = B + 1 the mass crosses a launch and a tile boundary together."""
    tr, tc, B = geo["tile_rows"], geo["tile_cols"], geo["default_block"]
    H, W = tr + 1, tc + 1
    goal = (3, 2)
    grid = np.zeros((H, W), np.uint8)
    grid[tr - 2, tc - 1] = 1  # one neighbour occupied: the row is not symmetric
    pi = random_table(H, W, 29)
    pi[tr - 1, tc - 1] = 2  # a diagonal action at the probed cell
    b0 = one_hot(H, W, tc - 1, tr - 1)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.policy_set_table(pi)
        T = ctx.model_download()[0]
        row = T[(tr - 1) * W + tc - 1, 2]
        assert (row > 0).sum() >= 2 and not np.array_equal(row, row[::-1]), "the probe can tell"
        for h in (1, B + 1):
            want = R.evaluate(T, pi, goal, b0, H, W, h)
            if h == 1:
                np.testing.assert_array_equal(
                    R.bits(want[0][tr - 2:tr + 1, tc - 2:tc + 1]).reshape(-1), R.bits(row))
            for route in ("planes", "tiles"):
                ctx.occupancy_evaluate(h, b0, table="user", route=route)
                assert_bits(ctx.occupancy_get(), want, f"probe H={h} {route}")


# ---------------------------------------------------------------- 4. world
def test_world_differs_from_the_map(pp2, geo):
    H, W = geo["tile_rows"], geo["tile_cols"] + 9  # two tiles
    goal, wgoal = (W - 3, H // 2), (W - 2, H // 2 + 1)
    grid = np.zeros((H, W), np.uint8)
    grid[0, :] = grid[-1, :] = grid[:, 0] = grid[:, -1] = 1
    wgrid = grid.copy()
    wgrid[4:H - 6, geo["tile_cols"] - 1] = 1  # the wall the believed map lacks, at the tile edge
    h = 2 * geo["default_block"] + 1
    b0 = uniform_free(grid)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid, wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        w.model_generate()
        ctx.mdp_solve()
        pi = ctx.mdp_get()[1]
        Tw = w.model_download()[0]
        want = R.evaluate(Tw, pi, wgoal, b0, H, W, h)
        for route in ("auto", "planes", "tiles"):
            ctx.occupancy_evaluate(h, b0, table="mdp", world=w, route=route)
            assert_bits(ctx.occupancy_get(), want, f"world, route {route}")
        own = R.evaluate(ctx.model_download()[0], pi, goal, b0, H, W, h)
        assert not np.array_equal(R.bits(own[0]), R.bits(want[0]))
        ctx.occupancy_evaluate(h, b0, table="mdp", world=None)
        assert_bits(ctx.occupancy_get(), own, "world = NULL")
        ctx.occupancy_evaluate(h, b0, table="mdp", world=ctx)
        assert_bits(ctx.occupancy_get(), own, "world = ctx")
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx, \
            pp2.GridContext(wgrid[:-1], wgoal, gamma=float(GAMMA)) as w:
        ctx.model_generate()
        w.model_generate()
        expect(EINVAL, ctx.occupancy_evaluate, 3, b0, table="mdp", world=w)


# ---------------------------------------------------------------- 5. adjoint on the device
def test_adjoint_on_the_device(pp2):
    """<b0, P_H> = curve[H] and <b0, N_H> = sum V, P_H and N_H from
    pp2_policy_evaluate on the same context, the sums in fp64 on the host.
    Each side is H steps of at most ten roundings on non-negative terms:
    relative tolerance 2 * H * 10 * 2^-24."""
    h = 40
    grid, goal = PR.golden_case("sparse_map_100x40")
    b0 = uniform_free(grid)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        ctx.policy_evaluate(h, table="mdp")
        pol = ctx.policy_get()
        ctx.occupancy_evaluate(h, b0, table="mdp")
        _, V, curve = ctx.occupancy_get()
        b = b0.astype(np.float64)
        bp, bn = float((b * pol[1]).sum()), float((b * pol[2]).sum())
        arrived, visits = float(curve[h]), float(V.astype(np.float64).sum())
        print(f"<b0,P> {bp!r} curve[H] {arrived!r}; <b0,N> {bn!r} sum V {visits!r}")
        tol = 2 * h * 10 * 2.0 ** -24
        assert bp > 0.1 and bn > 10
        assert abs(arrived - bp) <= tol * bp
        assert abs(visits - bn) <= tol * bn
        for a, b_, name in zip(ctx.policy_get(), pol, "GPN"):
            np.testing.assert_array_equal(R.bits(a), R.bits(b_), err_msg=f"policy_get {name}")


# ---------------------------------------------------------------- 6. routes and refusals
def test_coded_off_takes_planes(pp2, geo):
    H, W = geo["tile_rows"] + 1, geo["tile_cols"] + 1
    goal = (W - 2, H - 2)
    grid = synth(H, W, 3, goal)
    h = geo["default_block"] + 1
    b0 = uniform_free(grid)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.mdp_sweep(12)
        ctx.occupancy_evaluate(h, b0, table="mdp", route="auto")
        assert ctx.occupancy_info()["route_taken"] == TILES
        coded = ctx.occupancy_get()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        ctx.occupancy_evaluate(h, b0, table="mdp", route="auto")
        assert ctx.occupancy_info()["route_taken"] == PLANES
        assert_bits(ctx.occupancy_get(), coded, "coded off")
        expect(ESTATE, ctx.occupancy_evaluate, h, b0, table="mdp", route="tiles")
        assert_bits(ctx.occupancy_get(), coded, "after the refusal")
        T = ctx.model_download()[0]
        assert_bits(coded, R.evaluate(T, ctx.mdp_get()[1], goal, b0, H, W, h), "reference")


def test_uploaded_model_without_a_dictionary(pp2):
    """More distinct cells than the dictionary holds: no coded model, so TILES
    is refused and AUTO takes PLANES -- on rows that are dense, which only this
    route's weights can hold."""
    H, W = 24, 20
    goal = (15, 8)
    grid = synth(H, W, 2, goal)
    rng = np.random.default_rng(41)
    T = rng.random((H * W, 9, 9)).astype(np.float32)
    T /= (T.sum(axis=2, keepdims=True) * np.float32(1.01))
    assert (T.astype(np.float64).sum(axis=2) <= 1).all()
    pi = random_table(H, W, 8)
    b0 = rng.random((H, W)).astype(np.float32)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        _, L, Rw, Cc = ctx.model_download()
        ctx.model_upload(T, L, Rw, Cc)
        assert not ctx.model_dict_info()[1]
        ctx.policy_set_table(pi)
        expect(ESTATE, ctx.occupancy_evaluate, 5, b0, table="user", route="tiles")
        ctx.occupancy_evaluate(5, b0, table="user", route="auto")
        assert ctx.occupancy_info()["route_taken"] == PLANES
        Tw = ctx.model_download()[0]
        np.testing.assert_array_equal(R.bits(Tw), R.bits(T))
        assert_bits(ctx.occupancy_get(), R.evaluate(Tw, pi, goal, b0, H, W, 5), "dense rows")


def test_refusals_and_snapshot(pp2, geo):
    H, W = 12, 20
    goal = (15, 8)
    grid = synth(H, W, 2, goal)
    b0 = uniform_free(grid)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        expect(ESTATE, ctx.occupancy_get)
        expect(ESTATE, ctx.occupancy_evaluate, 4, b0, table="path")
        expect(ESTATE, ctx.occupancy_evaluate, 4, b0, table="user")
        expect(EINVAL, ctx.occupancy_evaluate, 0, b0)
        expect(EINVAL, ctx.occupancy_evaluate, 65537, b0)
        expect(EINVAL, ctx.occupancy_evaluate, 4, b0, block=geo["max_block"] + 1)
        expect(EINVAL, ctx.occupancy_evaluate, 4, b0, block=-1)
        expect(EINVAL, ctx.occupancy_evaluate, 4, b0, route=3)
        expect(EINVAL, ctx.occupancy_evaluate, 4, b0, table=3)
        expect(ESTATE, ctx.occupancy_get)
        assert not ctx.occupancy_info()["valid"]
        ctx.mdp_sweep(10)
        pi = ctx.mdp_get()[1]
        T = ctx.model_download()[0]
        ctx.occupancy_evaluate(6, b0, table="mdp")
        first = ctx.occupancy_get()
        assert_bits(first, R.evaluate(T, pi, goal, b0, H, W, 6), "first")
        # a b0 outside [0, 1] is refused and the result stays
        for bad in (-1.0, np.nan, 1.5):
            b = b0.copy()
            b[H - 1, W - 1] = bad
            expect(EINVAL, ctx.occupancy_evaluate, 3, b, table="mdp")
            info = ctx.occupancy_info()
            assert info["valid"] and info["horizon"] == 6
            assert_bits(ctx.occupancy_get(), first, f"after b0 = {bad}")
        # -0 and a subnormal are +0
        b = b0.copy()
        zeros = np.flatnonzero(b.reshape(-1) == 0)[:2]
        assert zeros.size == 2
        b.reshape(-1)[zeros[0]] = -0.0
        b.reshape(-1)[zeros[1]] = np.float32(2.0 ** -130)
        assert R.bits(b).reshape(-1)[zeros[0]] == 0x80000000 and b.reshape(-1)[zeros[1]] > 0
        for route in ("planes", "tiles"):
            ctx.occupancy_evaluate(6, b, table="mdp", route=route)
            assert_bits(ctx.occupancy_get(), first, f"-0 and a subnormal, {route}")
        # b0 = None is the context's belief
        ctx.belief_set(b0)
        ctx.occupancy_evaluate(6, table="mdp")
        assert_bits(ctx.occupancy_get(), R.evaluate(T, pi, goal, ctx.belief_get(), H, W, 6),
                    "b0 = None")
        # a snapshot: a map update does not touch it, the next evaluation replaces it
        ctx.occupancy_evaluate(6, b0, table="mdp")
        ctx.map_update(np.ones((3, 2), np.uint8), x0=4, y0=4)
        assert_bits(ctx.occupancy_get(), first, "after map_update")
        T2 = ctx.model_download()[0]
        ctx.occupancy_evaluate(3, b0, table="mdp")
        assert ctx.occupancy_info()["horizon"] == 3
        assert_bits(ctx.occupancy_get(), R.evaluate(T2, pi, goal, b0, H, W, 3), "second")
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, 6)) as shard:
        shard.model_generate()
        expect(ESTATE, shard.occupancy_evaluate, 4, b0[:6])


# ---------------------------------------------------------------- 7. nothing else written
def test_evaluation_leaves_the_state_untouched(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = PR.golden_case("map_10x10")
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.belief_set(S.uniform_belief(grid))
        ctx.belief_update(1, 3)
        ctx.mdp_sweep(7)
        ctx.path_solve()
        ctx.policy_evaluate(5, table="mdp")

        def state():
            J, A = ctx.mdp_get()
            D, Ap = ctx.path_get()
            return [R.bits(ctx.belief_get()), R.bits(J), A, R.bits(D), Ap] + \
                [R.bits(a) for a in ctx.policy_get()]

        before = state()
        for table in ("mdp", "path"):
            for route in ("planes", "tiles"):
                ctx.occupancy_evaluate(9, table=table, route=route)
        ctx.occupancy_get()
        for a, b in zip(before, state()):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- 8. the example
def test_occupancy_demo_runs(pp2):
    exe = os.path.join(ROOT, "examples", "pp2_occupancy_demo")
    assert os.path.exists(exe), "build with make -C path_planning_2d_amd/csrc"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert "pp2_occupancy_demo ok" in out.stdout
    for line in ("table mdp", "table path", "stale map, in the world", "updated, in the world",
                 "largest V path - V mdp", "largest V stale - V updated"):
        assert line in out.stdout, out.stdout
    printed = {}
    for m in re.finditer(r"^  table (mdp|path)\s+arrived (\S+) .* passes 0.5 at step (-?\d+), "
                         r"0.9 at step (-?\d+);", out.stdout, re.M):
        printed[m.group(1)] = (np.float32(float.fromhex(m.group(2))), int(m.group(3)),
                               int(m.group(4)))
    assert sorted(printed) == ["mdp", "path"], out.stdout
    grid, goal = PR.golden_case("sparse_map_100x40")
    assert goal == (95, 34)
    H, W = grid.shape
    with pp2.GridContext(grid, goal, gamma=0.95) as ctx:
        ctx.model_generate()
        ctx.mdp_solve()
        ctx.path_solve()
        for table in ("mdp", "path"):
            ctx.occupancy_evaluate(200, one_hot(H, W, 11, 6), table=table)
            curve = ctx.occupancy_get()[2]

            def passes(p):
                at = np.flatnonzero(curve >= np.float32(p))
                return int(at[0]) if at.size else -1

            assert (int(R.bits(curve[200])[0]), passes(0.5), passes(0.9)) == \
                (int(R.bits(printed[table][0])[0]), printed[table][1], printed[table][2]), table
