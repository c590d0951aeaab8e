"""GPU: the device-memory placement of the episodes' belief planes
(pp2_episodes_create_placed; the k_episodes<POLICY, true> instances and
k_episode_pad in csrc/pp2_episodes.hip) against the free-running NumPy
references tests/episodes_reference.py and tests/episodes_alpha_reference.py,
and against the LDS placement where the grid fits.  Everything is compared as
fp32 bit patterns: the placement changes no rounding.  The references are fed
the device's own Q planes / alpha planes, as in tests/test_gpu_episodes.py and
tests/test_gpu_episodes_alpha.py.
"""
import ctypes as C

import numpy as np
import pytest

import episodes_alpha_reference as AR
import episodes_global_cases as GC
import episodes_reference as R
from conftest import GAMMA, golden, golden_map

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = 5, 1
LDS, GLOBAL, AUTO = 0, 1, 2
SYNTH = {"synth_97x131": (97, 131, 3), "synth_1x7": (1, 7, 1), "synth_5x1": (5, 1, 2),
         "synth_256x256": (256, 256, 256)}
BASE = {"mode": R.MODE, "qmdp": R.QMDP}


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    assert (P.EPISODES_LDS, P.EPISODES_GLOBAL, P.EPISODES_AUTO) == (LDS, GLOBAL, AUTO)
    return P


def load_grid(name):
    from path_planning_2d_amd import synthetic as S
    if name in SYNTH:
        H, W, seed = SYNTH[name]
        grid = S.synth_grid(H, W, seed)
        grid[0, 0] = 0
        return grid, (0, 0)
    return golden_map(name), tuple(int(v) for v in golden("model", name)["goal"])


def make_ctx(pp2, grid, goal, solve=True):
    ctx = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    ctx.model_generate()
    if solve:
        ctx.mdp_solve()
    return ctx


def model_of(ctx, grid, goal):
    T, L, _, Cc = ctx.model_download()
    return R.Model(grid, goal, GAMMA, T=T, L=L, C=Cc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic_set(grid, S, seed=5, inf_at=3):
    """S alpha vectors from default_rng(seed).normal with actions k % 9; vector
    ``inf_at`` holds +inf at an occupied cell, if there is one."""
    al = np.random.default_rng(seed).normal(size=(S, grid.size)).astype(np.float32)
    occ = np.flatnonzero(grid.reshape(-1) == 1)
    if occ.size and inf_at is not None:
        al[inf_at, occ[0]] = np.inf
    return al, (np.arange(S) % 9).astype(np.uint8)


def run(ep, which, b0, starts, seed):
    """``which``: "mode", "qmdp", "fib" or "pbvi"."""
    if which in BASE:
        ep.run(which, b0, starts, seed)
    else:
        ep.run_alpha(which, b0, starts, seed)


def reference(ep, ctx, m, A, which, b0, starts, hz, seed):
    """The reference of the run ``ep`` has just made, from its own planes."""
    if which in BASE:
        return R.run_batch(m, ep.qplanes(), A, b0, starts, BASE[which], hz, seed,
                           wp=ctx.row_stride)
    al, act = ep.alphas()
    return AR.run_alpha_batch(m, al, act, b0, starts, hz, seed, wp=ctx.row_stride)


def assert_run_equal(ep, ref, which, what=""):
    """Results, traces, winners and every final belief of the last run == ref."""
    res = ep.results()
    for k in ("steps", "status", "final_cell"):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(bits(res["cost"]), bits(ref["cost"]), err_msg=f"{what} cost")
    if ep.record_trace:
        tr = ep.trace()
        for k in ("actions", "observations", "cells", "mode_cells"):
            np.testing.assert_array_equal(tr[k], ref[k], err_msg=f"{what} {k}")
        want_q = ref["qsums"] if which in ("qmdp", "fib") else np.zeros_like(ref["qsums"])
        np.testing.assert_array_equal(bits(tr["qsums"]), bits(want_q), err_msg=f"{what} qsums")
        if which not in BASE:
            ta = ep.trace_alpha()
            np.testing.assert_array_equal(ta["best_index"], ref["best_index"],
                                          err_msg=f"{what} best_index")
            np.testing.assert_array_equal(bits(ta["best_sum"]), bits(ref["best_sum"]),
                                          err_msg=f"{what} best_sum")
    for e in range(ep.episodes):
        np.testing.assert_array_equal(bits(ep.belief(e)), bits(ref["beliefs"][e]),
                                      err_msg=f"{what} belief of episode {e}")


def snapshot(ep, which, n=None, beliefs=True):
    """Everything the last run returns, as comparable arrays."""
    n = ep.episodes if n is None else n
    r = ep.results()
    out = [r[k][:n].copy() for k in ("steps", "status", "final_cell")] + [bits(r["cost"][:n]).copy()]
    if ep.record_trace:
        tr = ep.trace()
        out += [tr[k][:, :n].copy() for k in ("actions", "observations", "cells", "mode_cells")]
        out.append(bits(tr["qsums"][:, :n]).copy())
        if which not in BASE:
            ta = ep.trace_alpha()
            out += [ta["best_index"][:, :n].copy(), bits(ta["best_sum"][:, :n]).copy()]
    if beliefs:
        out += [bits(ep.belief(e)).copy() for e in range(n)]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. placement parity
@pytest.mark.parametrize("name", ["synth_1x7", "synth_5x1", "map_3x3", "map_10x10",
                                  "synth_97x131"])
def test_placement_parity_on_fitting_grids(pp2, name):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    H, W = grid.shape
    hw = H * W
    flat = grid.reshape(-1)
    occ = np.flatnonzero(flat == 1)
    free = np.flatnonzero(flat == 0)
    goal_cell = goal[1] * W + goal[0]
    b0 = S.uniform_belief(grid)
    # test_edge_geometry's starts: on the goal, both far corners, an occupied
    # cell (if any), a free cell
    starts5 = np.array([goal_cell, hw - 1, W - 1, occ[0] if occ.size else hw // 2,
                        free[len(free) // 2]], np.int32)
    al12, act12 = synthetic_set(grid, 12)  # K != 9: the chunk path, with a tail block
    with make_ctx(pp2, grid, goal) as ctx:
        if name == "synth_97x131":
            assert ctx.row_stride == 132  # a padded width
        m = model_of(ctx, grid, goal)
        _, A = ctx.mdp_get()
        ctx.fib_sweep(3)
        ctx.pbvi_set(al12, act12)
        for E, starts in ((1, starts5[1:2]), (5, starts5)):
            for hz in (1, 12):
                with pp2.EpisodeBatch(ctx, E, hz, record_trace=True, placement="global") as g, \
                        pp2.EpisodeBatch(ctx, E, hz, record_trace=True) as l:
                    assert g.placement() == {"requested": GLOBAL, "last": -1, "scratch_bytes": 0}
                    assert l.placement() == {"requested": LDS, "last": -1, "scratch_bytes": 0}
                    for which in ("mode", "qmdp", "fib", "pbvi"):
                        what = f"{name} E={E} hz={hz} {which}"
                        run(g, which, b0, starts, 77)
                        run(l, which, b0, starts, 77)
                        ref = reference(g, ctx, m, A, which, b0, starts, hz, 77)
                        assert_run_equal(g, ref, which, what)
                        assert same(snapshot(g, which), snapshot(l, which)), what
                        if which == "pbvi":
                            assert g.alphas()[0].shape[0] == 12
                        if E == 5:
                            assert ref["steps"][0] == 0 and ref["status"][0] == 1
                        gi, li = g.info(), l.info()
                        assert gi["threads"] == li["threads"] == 256
                        assert gi["workgroups"] == li["workgroups"] == E
                        assert 0 < gi["lds_bytes"] < li["lds_bytes"], what
                    pg, pl = g.placement(), l.placement()
                    assert pg["last"] == GLOBAL and pg["scratch_bytes"] > 0
                    assert pl == {"requested": LDS, "last": LDS, "scratch_bytes": 0}


# ---------------------------------------------------------------- 2. main case
@pytest.fixture(scope="module")
def main_ctx(pp2):
    case = R.main_case()
    ctx = make_ctx(pp2, case["grid"], case["goal"])
    yield case, ctx, model_of(ctx, case["grid"], case["goal"])
    ctx.close()


@pytest.mark.parametrize("policy", ["qmdp", "mode"])
def test_main_case_on_device_memory(pp2, main_ctx, policy):
    case, ctx, m = main_ctx
    _, A = ctx.mdp_get()
    E, hz = len(case["starts"]), case["horizon"]
    assert (E, hz) == (32, 32)
    with pp2.EpisodeBatch(ctx, E, hz, record_trace=True, placement="global") as ep:
        run(ep, policy, case["b0"], case["starts"], case["seed"])
        ref = reference(ep, ctx, m, A, policy, case["b0"], case["starts"], hz, case["seed"])
        assert_run_equal(ep, ref, policy, policy)
        assert ep.placement()["last"] == GLOBAL
    assert (ref["status"] == 1).any() and (ref["status"] == 0).any()


# ---------------------------------------------------------------- 3. a grid LDS refuses
def test_grid_that_lds_refuses(pp2):
    case = GC.large_case()
    grid, goal, b0, starts = case["grid"], case["goal"], case["b0"], case["starts"]
    hz, seed = case["horizon"], case["seed"]
    al12, act12 = synthetic_set(grid, 12)
    with make_ctx(pp2, grid, goal) as ctx:
        with pytest.raises(pp2.Pp2Error) as e:  # the premise: the planes do not fit LDS
            pp2.EpisodeBatch(ctx, len(starts), hz)
        assert e.value.status == EINVAL
        with pytest.raises(pp2.Pp2Error) as e:
            pp2.EpisodeBatch(ctx, len(starts), hz, placement="lds")
        assert e.value.status == EINVAL
        m = model_of(ctx, grid, goal)
        _, A = ctx.mdp_get()
        ctx.fib_sweep(3)
        ctx.pbvi_set(al12, act12)
        with pp2.EpisodeBatch(ctx, len(starts), hz, record_trace=True, placement="auto") as ep:
            assert ep.placement() == {"requested": AUTO, "last": -1, "scratch_bytes": 0}
            for which in ("mode", "qmdp", "fib", "pbvi"):
                run(ep, which, b0, starts, seed)
                ref = reference(ep, ctx, m, A, which, b0, starts, hz, seed)
                assert_run_equal(ep, ref, which, f"130x140 {which}")
                p = ep.placement()
                assert p["requested"] == AUTO and p["last"] == GLOBAL and p["scratch_bytes"] > 0
                if which == "qmdp":
                    # the paths test_episodes_global_cpu.py asserts on the oracle's solve
                    assert ref["steps"][0] == 0 and (ref["status"] == 0).any()
            info = ep.info()
            assert info["workgroups"] == len(starts) and info["threads"] == 256
            assert info["lds_bytes"] <= 160 * 1024


# ---------------------------------------------------------------- 4. 256 x 256
def test_256x256(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("synth_256x256")
    starts = GC.pick_starts(grid)
    b0 = S.uniform_belief(grid)
    hz, seed = 4, 77
    with make_ctx(pp2, grid, goal) as ctx:
        m = model_of(ctx, grid, goal)
        _, A = ctx.mdp_get()
        ctx.fib_sweep(3)
        with pp2.EpisodeBatch(ctx, len(starts), hz, record_trace=True, placement="global") as ep:
            for which in ("mode", "qmdp", "fib"):
                run(ep, which, b0, starts, seed)
                ref = reference(ep, ctx, m, A, which, b0, starts, hz, seed)
                assert_run_equal(ep, ref, which, f"256x256 {which}")
                assert ref["steps"][0] == 0 and (ref["steps"][1:] >= 1).all()
            assert ep.placement()["last"] == GLOBAL


# ---------------------------------------------------------------- 5. second and third episode
@pytest.mark.parametrize("policy", ["qmdp", "mode"])
def test_workgroups_take_further_episodes(pp2, main_ctx, policy):
    case, ctx, m = main_ctx
    _, A = ctx.mdp_get()
    E, hz, seed = 2600, 4, 11
    free = np.flatnonzero(case["grid"].reshape(-1) == 0)
    starts = free[np.arange(E) * 5 % free.size].astype(np.int32)
    b0 = case["b0"]
    with pp2.EpisodeBatch(ctx, E, hz, placement="global") as g, \
            pp2.EpisodeBatch(ctx, E, hz) as l, \
            pp2.EpisodeBatch(ctx, 5, hz, placement="global") as small:
        run(g, policy, b0, starts, seed)
        run(l, policy, b0, starts, seed)
        run(small, policy, b0, starts[:5], seed)
        wgs = g.info()["workgroups"]
        # (256 CUs x 4 workgroups: 1024, so workgroups take a second and a third episode)
        assert 1 <= wgs < E, wgs
        assert same(snapshot(g, policy, beliefs=False), snapshot(l, policy, beliefs=False))
        rg = g.results()
        Q = g.qplanes()
        for e in (0, wgs, E - 1):
            o = R.run_episode(m, Q, A, b0, int(starts[e]), BASE[policy], hz, seed, e,
                              wp=ctx.row_stride)
            assert (o["steps"], o["status"], o["final_cell"]) == (
                rg["steps"][e], rg["status"][e], rg["final_cell"][e]), e
            assert bits(o["cost"]) == bits(rg["cost"][e]), e
            assert np.array_equal(bits(o["belief"]), bits(g.belief(e))), e
            assert np.array_equal(bits(l.belief(e)), bits(g.belief(e))), e
        assert same(snapshot(g, policy, 5), snapshot(small, policy, 5))  # batch invariance


# ---------------------------------------------------------------- 6. lost belief
def test_lost_belief(pp2, main_ctx):
    case, ctx, m = main_ctx
    _, A = ctx.mdp_get()
    starts = case["starts"][:6]
    zero = np.zeros_like(case["b0"])
    for policy in ("mode", "qmdp"):
        with pp2.EpisodeBatch(ctx, 6, 5, record_trace=True, placement="global") as ep:
            run(ep, policy, zero, starts, 3)
            ref = reference(ep, ctx, m, A, policy, zero, starts, 5, 3)
            assert (ref["status"] == 2).all() and (ref["steps"] == 1).all()
            assert_run_equal(ep, ref, policy, f"lost {policy}")  # the raw update is stored
            assert ep.summary()["lost"] == 6


# ---------------------------------------------------------------- 7. AUTO decides per launch
def test_auto_decides_per_launch(pp2):
    """111 x 131: the MODE / QMDP / FIB layout fits LDS, a PBVI run's does not
    (tests/test_gpu_episodes_alpha.py::test_lds_with_alpha_scratch_must_fit)."""
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(111, 131, 3)
    grid[0, 0] = 0
    goal = (0, 0)
    b0 = S.uniform_belief(grid)
    starts = GC.pick_starts(grid)[:4]
    hz, seed = 3, 77
    al12, act12 = synthetic_set(grid, 12)
    with make_ctx(pp2, grid, goal) as ctx:
        m = model_of(ctx, grid, goal)
        _, A = ctx.mdp_get()
        ctx.pbvi_set(al12, act12)
        with pp2.EpisodeBatch(ctx, 4, hz, record_trace=True, placement="auto") as ep:
            base = ep.info()
            assert base["lds_bytes"] <= 160 * 1024 < base["lds_bytes"] + 2 * 64 * 16, base
            run(ep, "qmdp", b0, starts, seed)
            assert ep.placement() == {"requested": AUTO, "last": LDS, "scratch_bytes": 0}
            assert ep.info() == base
            first = snapshot(ep, "qmdp")
            ref = reference(ep, ctx, m, A, "qmdp", b0, starts, hz, seed)
            assert_run_equal(ep, ref, "qmdp", "auto qmdp from LDS")
            run(ep, "pbvi", b0, starts, seed)
            p = ep.placement()
            assert p["last"] == GLOBAL and p["scratch_bytes"] > 0
            assert ep.info()["lds_bytes"] < base["lds_bytes"]
            ref = reference(ep, ctx, m, A, "pbvi", b0, starts, hz, seed)
            assert_run_equal(ep, ref, "pbvi", "auto pbvi from device memory")
            run(ep, "fib", b0, starts, seed)  # K = 9: no alpha scratch, LDS again
            assert ep.placement()["last"] == LDS
            run(ep, "qmdp", b0, starts, seed)
            assert ep.placement()["last"] == LDS and ep.info() == base
            assert same(snapshot(ep, "qmdp"), first)


# ---------------------------------------------------------------- 8. errors
def test_errors(pp2):
    from path_planning_2d_amd import _lib
    from path_planning_2d_amd import synthetic as S
    assert _lib.STATUS_NAMES[ESTATE] == "PP2_ESTATE" and _lib.STATUS_NAMES[EINVAL] == "PP2_EINVAL"
    grid, goal = load_grid("map_10x10")
    H, W = grid.shape
    b0 = S.uniform_belief(grid)

    def create_fails(ctx, status, placement):
        with pytest.raises(pp2.Pp2Error) as e:
            pp2.EpisodeBatch(ctx, 4, 4, placement=placement)
        assert e.value.status == status

    for placement in ("global", "auto"):
        with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:  # no model
            create_fails(ctx, ESTATE, placement)
        with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, H // 2)) as sh:
            sh.model_generate()
            create_fails(sh, ESTATE, placement)
    with make_ctx(pp2, grid, goal) as ctx:
        h = C.c_void_p()
        for bad in (3, -1):
            with pytest.raises(pp2.Pp2Error) as e:
                _lib.call("pp2_episodes_create_placed", C.byref(h), ctx.handle, 4, 4, 0, bad)
            assert e.value.status == EINVAL and not h.value
        ctx.fib_sweep(2)
        with pp2.EpisodeBatch(ctx, 3, 4, placement="global") as ep:
            with pytest.raises(pp2.Pp2Error) as e:
                ep.run_lookahead("fib", b0, [0, 1, 2], seed=1)
            assert e.value.status == EINVAL and "LDS" in str(e.value)
            assert ep.placement() == {"requested": GLOBAL, "last": -1, "scratch_bytes": 0}
            with pytest.raises(pp2.Pp2Error) as e:  # nothing has run yet
                ep.results()
            assert e.value.status == ESTATE
            ep.run("qmdp", b0, [0, 1, 2], seed=1)  # and the batch still runs
            got = snapshot(ep, "qmdp")
            with pp2.EpisodeBatch(ctx, 3, 4) as ref:
                ref.run("qmdp", b0, [0, 1, 2], seed=1)
                assert same(got, snapshot(ref, "qmdp"))
        # an AUTO batch whose lookahead layout fits runs it, from LDS
        with pp2.EpisodeBatch(ctx, 3, 4, placement="auto") as ep, \
                pp2.EpisodeBatch(ctx, 3, 4) as ref:
            ep.run_lookahead("fib", b0, [0, 1, 2], seed=1)
            ref.run_lookahead("fib", b0, [0, 1, 2], seed=1)
            assert ep.placement()["last"] == LDS
            assert same(snapshot(ep, "fib", beliefs=True), snapshot(ref, "fib", beliefs=True))
    # ... and one whose lookahead layout does not fit refuses it, and runs on
    case = GC.large_case()
    with make_ctx(pp2, case["grid"], case["goal"], solve=False) as ctx:
        with pp2.EpisodeBatch(ctx, 2, 2, placement="auto") as ep:
            with pytest.raises(pp2.Pp2Error) as e:
                ep.run_lookahead("fib", case["b0"], [0, 1], seed=1)
            assert e.value.status == EINVAL and "LDS" in str(e.value)
            ep.run("mode", case["b0"], [0, 1], seed=1)
            assert ep.results()["steps"].shape == (2,) and ep.placement()["last"] == GLOBAL
