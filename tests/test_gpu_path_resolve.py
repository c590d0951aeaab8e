"""GPU: the warm re-solve of the shortest-path field (pp2_path_resolve; the
seed and raise kernels in csrc/pp2_path.hip) against the NumPy reference.

Every comparison is of the resolved field with tests/path_reference.py's field
of the new map: D as uint32 views, A_path as bytes, ``reached`` the reference's
finite count and ``raised`` the reference's raised count
(tests/path_resolve_reference.py) -- no tolerance anywhere.  The constructions
are those of test_path_resolve_cpu.py, which shows for each one marked there
that relaxation without the raise ends on other bits: an implementation that
skips or under-marks the raise fails here.
"""
import os
import subprocess

import numpy as np
import pytest

import episodes_reference as ER
import path_reference as R
import path_resolve_reference as WR
from conftest import GAMMA

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@pytest.fixture(scope="module")
def tile(pp2):
    with pp2.GridContext(np.zeros((2, 2), np.uint8), (0, 0)) as ctx:
        info = ctx.path_info()
    return info["tile_rows"], info["tile_cols"]


def compare(ctx, grid, goal, reached, what=""):
    """The valid field == the reference's of (grid, goal); returns (D, A)."""
    D, A = ctx.path_get()
    Dr, Ar = R.field(grid, goal)
    np.testing.assert_array_equal(R.bits(D), R.bits(Dr), err_msg=f"{what} D")
    np.testing.assert_array_equal(A, Ar, err_msg=f"{what} A_path")
    assert reached == int(np.isfinite(Dr).sum()), what
    assert ctx.path_info()["valid"], what
    return D, A


def solve_update(ctx, c):
    """Cold solve on c's grid, then its updates; returns the old (D, A)."""
    _, converged, _ = ctx.path_solve()
    assert converged
    old = ctx.path_get()
    for x0, y0, p in c["updates"]:
        ctx.map_update(p, x0=x0, y0=y0)
    assert not ctx.path_info()["valid"]
    return old


def changed_boxes(c):
    """Cells of the bounding boxes of each update's occupancy changes."""
    g, n = c["grid"].copy(), 0
    for x0, y0, p in c["updates"]:
        h, w = p.shape
        ys, xs = np.nonzero((g[y0:y0 + h, x0:x0 + w] == 1) != (p == 1))
        n += int((ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1))
        g[y0:y0 + h, x0:x0 + w] = p
    return n


def resolve_case(pp2, c, what):
    """The whole sequence on a fresh context; returns resolve_info and path_info."""
    with pp2.GridContext(c["grid"], c["goal"], gamma=float(GAMMA)) as ctx:
        D0, A0 = solve_update(ctx, c)
        rounds, converged, reached, warm = ctx.path_resolve()
        assert converged and warm, what
        compare(ctx, c["grid_new"], c["goal"], reached, what)
        ri, pi = ctx.path_resolve_info(), ctx.path_info()
        print(what, ri, pi)
        assert ri["warm"]
        assert ri["raised"] == WR.raised_count(D0, A0, c["grid_new"]) == c["raised"], what
        assert rounds == ri["raise_rounds"] + ri["relax_rounds"] == pi["rounds"]
        assert ri["seed_cells"] == changed_boxes(c)
        assert pi["polls"] < pi["launches"] and pi["launches"] > rounds
        if "finite" in c:
            assert reached == c["finite"][1]
        # nothing pending now: at once, no launch
        assert ctx.path_resolve() == (0, True, reached, True)
        assert ctx.path_info()["launches"] == pi["launches"]
        return ri, pi


# ---------------------------------------------------------------- 1. constructions
def test_figures_assume_the_tile(tile):
    assert tile == (32, 64)


@pytest.mark.parametrize("free_too", [False, True])
def test_corner_handoff(pp2, free_too):
    ri, _ = resolve_case(pp2, WR.corner_handoff(free_too), f"corner {free_too}")
    assert ri["raise_rounds"] >= 2


def test_corner_handoff_through_a_raised_cell(pp2):
    """Fails if the raise round does not mark the corner tile: the seed's own
    marks do not reach it."""
    ri, _ = resolve_case(pp2, WR.corner_handoff_raised(), "corner, raised")
    assert ri["raise_rounds"] >= 3


def test_bars_next_to_the_goal(pp2):
    c = WR.bars_next_to_the_goal()
    assert len(c["updates"]) == 2
    resolve_case(pp2, c, "bars")


@pytest.mark.parametrize("k", range(3))
def test_single_tile_edge_shapes(pp2, k):
    resolve_case(pp2, WR.single_tile(k), f"single tile {k}")


def test_corridor_many_raise_rounds(pp2, tile):
    c = WR.corridor("a")
    H, W = c["grid"].shape
    ntiles = -(-H // tile[0]) * -(-W // tile[1])
    ri, _ = resolve_case(pp2, c, "corridor a")
    assert ri["raise_rounds"] > ntiles, (ri, ntiles)


def test_corridor_unconverged_then_cold(pp2):
    c = WR.corridor("a")
    with pp2.GridContext(c["grid"], c["goal"], gamma=float(GAMMA)) as ctx:
        solve_update(ctx, c)
        rounds, converged, reached, warm = ctx.path_resolve(1)
        assert (converged, reached, warm) == (False, 0, True) and rounds >= 1
        assert not ctx.path_info()["valid"]
        for fn in (ctx.path_get, ctx.path_control, lambda: ctx.path_trace(0)):
            with pytest.raises(pp2.Pp2Error) as e:
                fn()
            assert e.value.status == ESTATE
        rounds, converged, reached, warm = ctx.path_resolve()
        assert converged and not warm
        compare(ctx, c["grid_new"], c["goal"], reached, "cold after the unconverged resolve")
        ri = ctx.path_resolve_info()
        assert not ri["warm"] and ri["raised"] == 0 and ri["raise_rounds"] == 0
        assert ri["relax_rounds"] == rounds
        with pytest.raises(pp2.Pp2Error) as e:
            ctx.path_resolve(0)
        assert e.value.status == EINVAL


def test_corridor_gap_moved(pp2):
    resolve_case(pp2, WR.corridor("b"), "corridor b")


def test_freed_only(pp2):
    ri, _ = resolve_case(pp2, WR.freed_only(), "freed only")
    assert ri["raise_rounds"] == 0 and ri["raised"] == 0 and ri["relax_rounds"] >= 1


def test_mixed_update(pp2):
    c = WR.mixed_97x131()
    assert len(c["updates"]) == 1
    resolve_case(pp2, c, "mixed")


def test_resolve_after_resolve(pp2):
    """Each resolve starts from the last one's field and table."""
    c = WR.mixed_97x131()
    grid, goal = c["grid"], c["goal"]
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        assert ctx.path_solve()[1]
        g = grid.copy()
        rng = np.random.default_rng(9)
        for step in range(4):
            D0, A0 = ctx.path_get()
            for _ in range(3):
                h, w = int(rng.integers(1, 7)), int(rng.integers(1, 7))
                y0, x0 = int(rng.integers(1, 97 - h)), int(rng.integers(1, 131 - w))
                p = (rng.random((h, w)) < 0.5).astype(np.uint8)
                g[y0:y0 + h, x0:x0 + w] = p
                ctx.map_update(p, x0=x0, y0=y0)
            _, converged, reached, warm = ctx.path_resolve()
            assert converged and warm
            compare(ctx, g, goal, reached, f"step {step}")
            assert ctx.path_resolve_info()["raised"] == WR.raised_count(D0, A0, g)


# ---------------------------------------------------------------- 2. fallbacks and no-ops
def test_fallbacks(pp2):
    grid = WR.synth(33, 70, 21)
    goal = (5, 4)
    grid[goal[1], goal[0]] = 0
    one, zero = np.array([[1]], np.uint8), np.array([[0]], np.uint8)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        # before any solve
        _, converged, reached, warm = ctx.path_resolve()
        assert converged and not warm and not ctx.path_resolve_info()["warm"]
        compare(ctx, grid, goal, reached, "before any solve")
        # the goal moved
        goal2 = (40, 20)
        g = grid.copy()
        if g[goal2[1], goal2[0]] == 1:
            g[goal2[1], goal2[0]] = 0
            ctx.map_update(zero, x0=goal2[0], y0=goal2[1])
        ctx.goal_set(goal2)
        _, converged, reached, warm = ctx.path_resolve()
        assert converged and not warm
        compare(ctx, g, goal2, reached, "after goal_set")
        # the goal cell occupied, then freed
        for patch in (one, zero):
            g[goal2[1], goal2[0]] = patch[0, 0]
            ctx.map_update(patch, x0=goal2[0], y0=goal2[1])
            _, converged, reached, warm = ctx.path_resolve()
            assert converged and not warm, patch
            compare(ctx, g, goal2, reached, f"goal cell set to {patch[0, 0]}")
        # 17 one-cell updates
        free = np.flatnonzero(g.reshape(-1) != 1)
        free = free[free != goal2[1] * 70 + goal2[0]]
        for cell in np.random.default_rng(4).choice(free, 17, False):
            g[cell // 70, cell % 70] = 1
            ctx.map_update(one, x0=int(cell % 70), y0=int(cell // 70))
        _, converged, reached, warm = ctx.path_resolve()
        assert converged and not warm
        compare(ctx, g, goal2, reached, "17 updates")
        # 16 are followed warm
        for cell in np.random.default_rng(5).choice(np.flatnonzero(g.reshape(-1) == 1), 16, False):
            g[cell // 70, cell % 70] = 0
            ctx.map_update(zero, x0=int(cell % 70), y0=int(cell // 70))
        _, converged, reached, warm = ctx.path_resolve()
        assert converged and warm
        compare(ctx, g, goal2, reached, "16 updates")


def test_nothing_pending_and_occupy_then_free(pp2):
    c = WR.mixed_97x131()
    grid, goal = c["grid"], c["goal"]
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        _, converged, reached = ctx.path_solve()
        assert converged
        D0, A0 = ctx.path_get()
        launches = ctx.path_info()["launches"]
        assert ctx.path_resolve() == (0, True, reached, True)
        assert ctx.path_info()["launches"] == launches and ctx.path_info()["valid"]
        ri = ctx.path_resolve_info()
        assert ri == dict(warm=True, raised=0, raise_rounds=0, relax_rounds=0, seed_cells=0)
        # a cell on many paths occupied and freed again before one resolve
        y, x = 20, 30
        assert grid[y, x] != 1 and np.isfinite(D0[y, x])
        ctx.map_update(np.array([[1]], np.uint8), x0=x, y0=y)
        ctx.map_update(np.array([[0]], np.uint8), x0=x, y0=y)
        assert not ctx.path_info()["valid"]
        _, converged, reached2, warm = ctx.path_resolve()
        assert converged and warm and reached2 == reached
        D1, A1 = ctx.path_get()
        np.testing.assert_array_equal(R.bits(D1), R.bits(D0))
        np.testing.assert_array_equal(A1, A0)
        ri = ctx.path_resolve_info()
        assert ri["raised"] == 0 and ri["raise_rounds"] == 0 and ri["seed_cells"] == 2
        # an update that changes no occupancy keeps the field
        ctx.map_update(np.array([[0]], np.uint8), x0=x, y0=y)
        assert ctx.path_info()["valid"]


def test_shards_refuse(pp2):
    grid, goal = R.golden_case("map_10x10")
    H = grid.shape[0]
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, H // 2)) as sh:
        with pytest.raises(pp2.Pp2Error) as e:
            sh.path_resolve()
        assert e.value.status == ESTATE
    with pp2.ShardGroup(grid, goal, (0, 5, H), gamma=float(GAMMA)) as grp:
        with pytest.raises(pp2.Pp2Error) as e:
            grp.shards[0].path_resolve()
        assert e.value.status == ESTATE


# ---------------------------------------------------------------- 3. consumers
def obstacle_on_the_path(ctx, grid):
    """Occupies the middle cell of the path from (11, 6); returns the new grid."""
    W = grid.shape[1]
    cells, _ = ctx.path_trace((11, 6))
    assert len(cells) > 4
    mid = int(cells[len(cells) // 2])
    g2 = grid.copy()
    g2[mid // W, mid % W] = 1
    ctx.map_update(np.array([[1]], np.uint8), x0=mid % W, y0=mid // W)
    return g2, mid


def test_untouched_state_trace_and_control(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = R.golden_case("sparse_map_100x40")
    H, W = grid.shape
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.belief_set(S.uniform_belief(grid))
        ctx.mdp_reset()
        ctx.mdp_sweep(7)
        ctx.fib_sweep(2)
        ctx.belief_update(1, 0)
        assert ctx.path_solve()[1]
        D0, A0 = ctx.path_get()
        g2, mid = obstacle_on_the_path(ctx, grid)
        before = (ctx.mdp_get(), ctx.belief_get(), ctx.fib_get())
        _, converged, reached, warm = ctx.path_resolve()
        assert converged and warm
        after = (ctx.mdp_get(), ctx.belief_get(), ctx.fib_get())
        np.testing.assert_array_equal(R.bits(before[0][0]), R.bits(after[0][0]))
        np.testing.assert_array_equal(before[0][1], after[0][1])
        np.testing.assert_array_equal(R.bits(before[1]), R.bits(after[1]))
        np.testing.assert_array_equal(R.bits(before[2]), R.bits(after[2]))
        D, A = compare(ctx, g2, goal, reached, "obstacle on the path")
        assert ctx.path_resolve_info()["raised"] == WR.raised_count(D0, A0, g2) > 0
        assert np.isinf(D[mid // W, mid % W])
        # the trace is re-read from the planes
        start = 6 * W + 11
        cells, length = ctx.path_trace((11, 6))
        ref, _ = R.trace(A, D, start)
        np.testing.assert_array_equal(cells, ref)
        assert mid not in cells and cells[-1] == goal[1] * W + goal[0]
        assert np.float32(length).view(np.uint32) == D.reshape(-1)[start].view(np.uint32)
        # control at one-hot beliefs reads the new table
        changed = np.flatnonzero((A != A0).reshape(-1) & np.isfinite(D).reshape(-1))
        assert len(changed) > 0
        for c in [start] + [int(x) for x in changed[:8]]:
            b = np.zeros(H * W, np.float32)
            b[c] = 1
            ctx.belief_set(b)
            a, d, cell = ctx.path_control()
            assert (a, cell) == (int(A.reshape(-1)[c]), c), c
            assert np.float32(d).view(np.uint32) == D.reshape(-1)[c].view(np.uint32), c


def ep_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def snapshot(ep):
    out = dict(ep.results())
    tr = ep.trace()
    out.update({k: tr[k] for k in ("actions", "observations", "cells", "mode_cells")})
    out["beliefs"] = np.stack([ep.belief(e) for e in range(ep.episodes)])
    return {k: ep_bits(v) if v.dtype == np.float32 else v for k, v in out.items()}


def test_episodes_resume_after_resolve_equals_after_cold_solve(pp2):
    grid, goal = R.golden_case("sparse_map_100x40")
    case = ER.main_case()
    assert tuple(case["goal"]) == tuple(goal)
    E = len(case["starts"])

    def sequence(warm_wanted):
        with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
            ctx.model_generate()
            ctx.mdp_solve()
            assert ctx.path_solve()[1]
            with pp2.EpisodeBatch(ctx, E, 8, record_trace=True, placement="lds") as ep:
                ep.set_action_table("path")
                ep.run("mode", case["b0"], case["starts"], case["seed"], placed=True)
                first = snapshot(ep)
                obstacle_on_the_path(ctx, grid)
                with pytest.raises(pp2.Pp2Error) as e:
                    ep.resume("mode", case["seed"])
                assert e.value.status == ESTATE
                if warm_wanted:
                    _, converged, _, warm = ctx.path_resolve()
                    assert converged and warm
                else:
                    assert ctx.path_solve()[1]
                ep.resume("mode", case["seed"])
                return first, snapshot(ep)

    w0, w1 = sequence(True)
    c0, c1 = sequence(False)
    for got, want, what in ((w0, c0, "first segment"), (w1, c1, "resumed segment")):
        assert set(got) == set(want)
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    assert (w1["steps"] > 8).any()


# ---------------------------------------------------------------- 4. demo
def test_astar_replan_demo_runs(pp2):
    exe = os.path.join(ROOT, "examples", "pp2_astar_replan_demo")
    assert os.path.exists(exe), "build with make -C path_planning_2d_amd/csrc"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pp2_astar_replan_demo ok" in out.stdout
    assert "warm re-solve" in out.stdout and "cells raised" in out.stdout
