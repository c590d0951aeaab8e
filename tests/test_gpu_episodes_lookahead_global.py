"""GPU: the one-step lookahead on device-memory belief planes
(pp2_episodes_run_lookahead_placed; ``EpisodeBatch.run_lookahead(...,
placed=True)``; the k_episodes<3, true> instance in csrc/pp2_episodes.hip)
against the free-running NumPy reference tests/episodes_lookahead_reference.py
and against the LDS lookahead where the grid fits.  Everything is compared as
fp32 bit patterns: the placement changes no rounding.  The reference is fed the
device's own alpha planes (``alphas()``) and ``model_download``'s T, L, C, R,
as in tests/test_gpu_episodes_lookahead.py.
"""
import time

import numpy as np
import pytest

import episodes_global_cases as GC
import episodes_lookahead_reference as LR
import episodes_reference as R
from conftest import GAMMA, golden, golden_map

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = 5, 1
LDS, GLOBAL, AUTO = 0, 1, 2
SYNTH = {"synth_97x131": (97, 131, 3), "synth_1x7": (1, 7, 1), "synth_5x1": (5, 1, 2),
         "synth_256x256": (256, 256, 256)}
# the lookahead scratch that stays in LDS: two buffers of 16 x 4 sums per wave
# quad, and the 32 L classes' sixteen columns
SCRATCH = 4 * (2 * 16 * 4 * 4 + 16 * 32)


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
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
    """(model, R[hw, 9]) as the device holds them."""
    T, L, Rw, Cc = ctx.model_download()
    return R.Model(grid, goal, GAMMA, T=T, L=L, C=Cc), np.asarray(Rw, np.float32).reshape(-1, 9)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def synthetic_set(grid, S, seed=5, inf_at=3):
    """S alpha vectors from default_rng(seed).normal with actions k % 9; vector
    ``inf_at`` holds +inf at an occupied cell (none: no such vector)."""
    al = np.random.default_rng(seed).normal(size=(S, grid.size)).astype(np.float32)
    occ = np.flatnonzero(grid.reshape(-1) == 1)
    if occ.size and inf_at is not None:
        al[inf_at, occ[0]] = np.inf
    return al, (np.arange(S) % 9).astype(np.uint8)


def assert_lookahead_equal(ep, ref, what=""):
    """Results, the trace, the four lookahead arrays and every final belief of
    the last run == the reference."""
    res = ep.results()
    for k in ("steps", "status", "final_cell"):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(bits(res["cost"]), bits(ref["cost"]), err_msg=f"{what} cost")
    if ep.record_trace:
        tr = ep.trace()
        for k in ("actions", "observations", "cells", "mode_cells"):
            np.testing.assert_array_equal(tr[k], ref[k], err_msg=f"{what} {k}")
        np.testing.assert_array_equal(bits(tr["qsums"]), bits(ref["qsums"]),
                                      err_msg=f"{what} qsums")
        tl = ep.trace_lookahead()
        np.testing.assert_array_equal(tl["leaf_index"], ref["leaf_index"],
                                      err_msg=f"{what} leaf_index")
        for k in ("rewards", "leaf_max", "q"):
            np.testing.assert_array_equal(bits(tl[k]), bits(ref[k]), err_msg=f"{what} {k}")
    for e in range(ep.episodes):
        np.testing.assert_array_equal(bits(ep.belief(e)), bits(ref["beliefs"][e]),
                                      err_msg=f"{what} belief of episode {e}")


def snapshot(ep, n=None, look=True, beliefs=True):
    """Everything the last run returns (``look``: it was a lookahead run), as
    comparable arrays."""
    n = ep.episodes if n is None else n
    r = ep.results()
    out = [r[k][:n].copy() for k in ("steps", "status", "final_cell")] + [bits(r["cost"][:n]).copy()]
    if ep.record_trace:
        tr = ep.trace()
        out += [tr[k][:, :n].copy() for k in ("actions", "observations", "cells", "mode_cells")]
        out.append(bits(tr["qsums"][:, :n]).copy())
        if look:
            tl = ep.trace_lookahead()
            out.append(tl["leaf_index"][:, :n].copy())
            out += [bits(tl[k][:, :n]).copy() for k in ("rewards", "leaf_max", "q")]
    if beliefs:
        out += [bits(ep.belief(e)).copy() for e in range(n)]
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def edge_starts(grid, goal):
    """test_edge_geometry's eight starts: the goal, both far corners, an
    occupied cell (if any), free cells."""
    H, W = grid.shape
    hw = H * W
    flat = grid.reshape(-1)
    occ = np.flatnonzero(flat == 1)
    free = np.flatnonzero(flat == 0)
    goal_cell = goal[1] * W + goal[0]
    return np.array([goal_cell, hw - 1, W - 1, occ[0] if occ.size else hw // 2,
                     free[len(free) // 2], free[len(free) // 3], free[-1], free[0]], np.int32)


def fails(pp2, status, fn, *args, **kw):
    with pytest.raises(pp2.Pp2Error) as e:
        fn(*args, **kw)
    assert e.value.status == status, (fn, args, str(e.value))
    return str(e.value)


# ---------------------------------------------------------------- 1. placement parity
@pytest.mark.parametrize("name", ["synth_1x7", "synth_5x1", "map_3x3", "map_10x10"])
def test_placement_parity_on_fitting_grids(pp2, name):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    b0 = S.uniform_belief(grid)
    starts = edge_starts(grid, goal)
    E, hz = 8, 6
    al_s, act_s = synthetic_set(grid, 10)
    with make_ctx(pp2, grid, goal) as ctx:
        m, Rw = model_of(ctx, grid, goal)
        ctx.fib_sweep(9)
        ctx.pbvi_set(al_s, act_s)
        with pp2.EpisodeBatch(ctx, E, hz, record_trace=True, placement="global") as g, \
                pp2.EpisodeBatch(ctx, E, hz, record_trace=True) as l:
            for which in ("pbvi", "fib"):
                what = f"{name} {which}"
                assert g.run_lookahead(which, b0, starts, seed=77, placed=True) is g
                assert g.lookahead and g.alpha_set == (1 if which == "pbvi" else 0)
                l.run_lookahead(which, b0, starts, seed=77)
                al, act = g.alphas()
                if which == "pbvi":
                    np.testing.assert_array_equal(bits(al), bits(al_s))
                    np.testing.assert_array_equal(act, act_s)
                ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, 77, wp=ctx.row_stride)
                assert_lookahead_equal(g, ref, what)
                assert same(snapshot(g), snapshot(l)), what
                p = g.placement()
                assert p["last"] == GLOBAL and p["scratch_bytes"] > 0, what
                assert l.placement()["last"] == LDS
                # the first start is the goal: no step, b0 as given
                res = g.results()
                assert res["steps"][0] == 0 and res["status"][0] == 1
                np.testing.assert_array_equal(bits(g.belief(0)), bits(b0))
            # run("...-lookahead", placed=True) is the same call
            g.run("fib-lookahead", b0, starts, seed=77, placed=True)
            assert same(snapshot(g), snapshot(l)) and g.placement()["last"] == GLOBAL


# ---------------------------------------------------------------- 2. block tails, both buffers
@pytest.mark.parametrize("K", [70, 1, 2, 3])
def test_block_tails_and_both_sums_buffers(pp2, K):
    """map_10x10: K = 70 (eighteen blocks, a leaf winner >= 64) and the tail
    blocks of 1, 2 and 3 vectors on their own, from device-memory planes."""
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    free = np.flatnonzero(grid.reshape(-1) == 0)
    starts = free[[0, len(free) // 2, -1]].astype(np.int32)
    al_s, act_s = synthetic_set(grid, K, seed=6, inf_at=None)
    if K == 70:
        al_s[66] += np.float32(2.0)  # a vector of the last blocks that wins
    with make_ctx(pp2, grid, goal) as ctx:
        m, Rw = model_of(ctx, grid, goal)
        ctx.pbvi_set(al_s, act_s)
        with pp2.EpisodeBatch(ctx, 3, 4, record_trace=True, placement="global") as ep:
            ep.run("pbvi-lookahead", b0, starts, seed=3, placed=True)
            al, act = ep.alphas()
            np.testing.assert_array_equal(bits(al), bits(al_s))
            ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, 4, 3, wp=ctx.row_stride)
            assert_lookahead_equal(ep, ref, f"K = {K}")
            assert ep.placement()["last"] == GLOBAL
    if K == 70:
        assert ref["leaf_index"].max() >= 64
    assert (ref["steps"] > 0).any()


# ---------------------------------------------------------------- 3. W % 4 != 0
def test_padded_width(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("synth_97x131")
    b0 = S.uniform_belief(grid)
    E, hz = 4, 3
    starts = edge_starts(grid, goal)[:E]
    al_s, act_s = synthetic_set(grid, 10)
    with make_ctx(pp2, grid, goal) as ctx:
        assert ctx.row_stride == 132 and grid.shape[1] % 4 != 0
        m, Rw = model_of(ctx, grid, goal)
        ctx.pbvi_set(al_s, act_s)
        with pp2.EpisodeBatch(ctx, E, hz, record_trace=True, placement="global") as g, \
                pp2.EpisodeBatch(ctx, E, hz, record_trace=True) as l:
            g.run_lookahead("pbvi", b0, starts, seed=77, placed=True)
            l.run_lookahead("pbvi", b0, starts, seed=77)
            al, _ = g.alphas()
            np.testing.assert_array_equal(bits(al), bits(al_s))
            ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, 77, wp=ctx.row_stride)
            assert_lookahead_equal(g, ref, "97x131 pbvi")
            assert same(snapshot(g), snapshot(l))
            assert g.placement()["last"] == GLOBAL and l.placement()["last"] == LDS


# ---------------------------------------------------------------- 4. a grid LDS refuses
def test_grid_that_lds_refuses(pp2):
    case = GC.large_case()
    grid, goal, b0, starts = case["grid"], case["goal"], case["b0"], case["starts"]
    E, hz, seed = len(starts), 3, case["seed"]
    assert grid.shape == (130, 140) and E == 7 and starts[0] == 0
    with make_ctx(pp2, grid, goal) as ctx:
        m, Rw = model_of(ctx, grid, goal)
        ctx.fib_sweep(3)
        ref = None
        for placement in ("auto", "global"):
            with pp2.EpisodeBatch(ctx, E, hz, record_trace=True, placement=placement) as ep:
                # the old entry keeps its contract
                msg = fails(pp2, EINVAL, ep.run_lookahead, "fib", b0, starts, seed)
                assert "LDS" in msg
                msg = fails(pp2, EINVAL, ep.run, "fib-lookahead", b0, starts, seed)
                assert "LDS" in msg
                assert ep.placement()["last"] == -1
                ep.run_lookahead("fib", b0, starts, seed, placed=True)
                al, act = ep.alphas()
                np.testing.assert_array_equal(act, np.arange(9))
                if ref is None:  # one reference for both batches: the same alphas
                    ref_al = al
                    ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, seed,
                                                 wp=ctx.row_stride)
                np.testing.assert_array_equal(bits(al), bits(ref_al))
                assert_lookahead_equal(ep, ref, f"130x140 {placement}")
                p = ep.placement()
                assert p["last"] == GLOBAL and p["scratch_bytes"] > 0
                assert ref["steps"][0] == 0 and (ref["steps"][1:] >= 1).all()
                # pred left the planes' pads and halos zero: a QMDP run on the
                # same batch is a fresh GLOBAL batch's
                ep.run("qmdp", b0, starts, seed)
                with pp2.EpisodeBatch(ctx, E, hz, record_trace=True,
                                      placement="global") as fresh:
                    fresh.run("qmdp", b0, starts, seed)
                    assert same(snapshot(ep, look=False), snapshot(fresh, look=False))


# ---------------------------------------------------------------- 5. AUTO takes LDS where it fits
def test_auto_takes_lds_where_the_lookahead_layout_fits(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    starts = np.array([0, 1, 2, 3], np.int32)
    with make_ctx(pp2, grid, goal) as ctx:
        ctx.fib_sweep(2)
        with pp2.EpisodeBatch(ctx, 4, 3, placement="auto") as ep, \
                pp2.EpisodeBatch(ctx, 4, 3) as l:
            ep.run_lookahead("fib", b0, starts, seed=1, placed=True)
            l.run_lookahead("fib", b0, starts, seed=1)
            assert ep.placement() == {"requested": AUTO, "last": LDS, "scratch_bytes": 0}
            assert ep.info() == l.info()
            assert same(snapshot(ep), snapshot(l))
            # ... and an LDS batch's placed call is the old call
            l.run_lookahead("fib", b0, starts, seed=1, placed=True)
            assert l.placement()["last"] == LDS and ep.info() == l.info()
            assert same(snapshot(ep), snapshot(l))


# ---------------------------------------------------------------- 6. further episodes
def test_workgroups_take_further_episodes(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    E, hz, seed = 1100, 3, 11
    free = np.flatnonzero(grid.reshape(-1) == 0)
    starts = free[np.arange(E) * 5 % free.size].astype(np.int32)
    with make_ctx(pp2, grid, goal) as ctx:
        m, Rw = model_of(ctx, grid, goal)
        ctx.fib_sweep(9)
        with pp2.EpisodeBatch(ctx, E, hz, placement="global") as g, \
                pp2.EpisodeBatch(ctx, E, hz) as l, \
                pp2.EpisodeBatch(ctx, 5, hz, placement="global") as small:
            g.run("qmdp", b0, starts, seed)
            g.results()
            qmdp_wgs = g.info()["workgroups"]
            scratch = g.placement()["scratch_bytes"]
            assert scratch > 0
            g.run_lookahead("fib", b0, starts, seed, placed=True)
            l.run_lookahead("fib", b0, starts, seed)
            small.run_lookahead("fib", b0, starts[:5], seed, placed=True)
            assert same(snapshot(g), snapshot(l))  # results, costs and every belief
            assert g.placement()["scratch_bytes"] == scratch  # no reallocation
            wgs = g.info()["workgroups"]
            assert 1 <= wgs < E, wgs
            assert wgs <= qmdp_wgs, (wgs, qmdp_wgs)
            rg = g.results()
            al, _ = g.alphas()
            for e in sorted({0, wgs, E - 1}):
                o = LR.run_lookahead_episode(m, Rw, al, b0, int(starts[e]), hz, seed, e,
                                             wp=ctx.row_stride)
                assert (o["steps"], o["status"], o["final_cell"]) == (
                    rg["steps"][e], rg["status"][e], rg["final_cell"][e]), e
                assert bits(o["cost"]) == bits(rg["cost"][e]), e
                assert np.array_equal(bits(o["belief"]), bits(g.belief(e))), e
            assert same(snapshot(g, 5), snapshot(small, 5))  # batch invariance


# ---------------------------------------------------------------- 7. info
def test_info_reports_the_global_lookahead_launch(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    starts = np.array([0, 1, 2, 3], np.int32)
    with make_ctx(pp2, grid, goal) as ctx, \
            pp2.EpisodeBatch(ctx, 4, 2, placement="global") as ep:
        ep.run("qmdp", b0, starts)
        base = ep.info()
        ep.run_lookahead("fib", b0, starts, placed=True)
        info = ep.info()
        assert info["lds_bytes"] == base["lds_bytes"] + SCRATCH
        assert info["threads"] == base["threads"] == 256
        assert 1 <= info["workgroups"] <= 4
        ep.run("qmdp", b0, starts)
        assert ep.info() == base


# ---------------------------------------------------------------- 8. lost belief
def test_lost_belief(pp2):
    case = LR.look_case()
    starts = case["starts"][:6]
    zero = np.zeros_like(case["b0"])
    with make_ctx(pp2, case["grid"], case["goal"]) as ctx:
        assert case["grid"].size == 100 * 40  # the main case
        m, Rw = model_of(ctx, case["grid"], case["goal"])
        ctx.fib_sweep(3)
        with pp2.EpisodeBatch(ctx, 6, 5, record_trace=True, placement="global") as ep:
            ep.run_lookahead("fib", zero, starts, seed=3, placed=True)
            al, _ = ep.alphas()
            ref = LR.run_lookahead_batch(m, Rw, al, zero, starts, 5, 3, wp=ctx.row_stride)
            assert (ref["status"] == 2).all() and (ref["steps"] == 1).all()
            assert_lookahead_equal(ep, ref, "lost")  # the raw update is stored
            assert ep.summary()["lost"] == 6 and ep.placement()["last"] == GLOBAL


# ---------------------------------------------------------------- 9. 256 x 256
def test_256x256(pp2):
    """Two episodes, horizon 2: the goal and a free cell near the middle, so
    the reference runs two episode-steps (one to three seconds of NumPy; the
    second step is the first whose cur is a workgroup's own plane)."""
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("synth_256x256")
    H, W = grid.shape
    free = np.flatnonzero(grid.reshape(-1) == 0)
    mid = (H // 2) * W + W // 2
    starts = np.array([0, free[np.argmin(np.abs(free - mid))]], np.int32)
    b0 = S.uniform_belief(grid)
    hz, seed = 2, 77
    with make_ctx(pp2, grid, goal) as ctx:
        m, Rw = model_of(ctx, grid, goal)
        ctx.fib_sweep(3)
        with pp2.EpisodeBatch(ctx, 2, hz, record_trace=True, placement="global") as ep:
            ep.run_lookahead("fib", b0, starts, seed, placed=True)
            al, _ = ep.alphas()
            t = time.perf_counter()
            ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, seed, wp=ctx.row_stride)
            print(f"256x256 reference: {time.perf_counter() - t:.2f} s")
            assert_lookahead_equal(ep, ref, "256x256 fib")
            assert ref["steps"][0] == 0 and ref["steps"][1] == 2
            assert ep.placement()["last"] == GLOBAL


# ---------------------------------------------------------------- 10. errors
def test_errors(pp2):
    import ctypes as C

    from path_planning_2d_amd import _lib
    from path_planning_2d_amd import synthetic as S
    assert _lib.STATUS_NAMES[ESTATE] == "PP2_ESTATE" and _lib.STATUS_NAMES[EINVAL] == "PP2_EINVAL"
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    starts = np.array([0, 1, 2], np.int32)

    def run_placed(batch, which):
        _lib.call("pp2_episodes_run_lookahead_placed", batch._h, which, C.c_uint64(1),
                  b0.ctypes.data_as(C.POINTER(C.c_float)),
                  starts.ctypes.data_as(C.POINTER(C.c_int32)))

    with make_ctx(pp2, grid, goal) as ctx, \
            pp2.EpisodeBatch(ctx, 3, 4, placement="global") as ep, \
            pp2.EpisodeBatch(ctx, 3, 4, record_trace=True, placement="global") as tr, \
            pp2.EpisodeBatch(ctx, 3, 4, placement="global") as fresh:
        ctx.fib_sweep(2)
        fresh.run("qmdp", b0, starts, seed=1)
        want = snapshot(fresh, look=False)

        def still_runs():
            ep.run("qmdp", b0, starts, seed=1)
            assert same(snapshot(ep, look=False), want)

        for bad in (2, -1):  # an unknown alpha set
            fails(pp2, EINVAL, run_placed, ep, bad)
            still_runs()
        fails(pp2, ESTATE, run_placed, ep, 1)  # PBVI without alpha vectors
        still_runs()
        # a PBVI action of 9: pp2_pbvi_set refuses it itself (PP2_EINVAL, before
        # any launch), so none reaches a run and the context still has no set
        al, act = synthetic_set(grid, 5, inf_at=None)
        bad = act.copy()
        bad[3] = 9
        fails(pp2, EINVAL, ctx.pbvi_set, al, bad)
        fails(pp2, ESTATE, ep.run_lookahead, "pbvi", b0, starts, 1, True)
        assert ep.placement()["last"] == GLOBAL and not ep.lookahead
        fails(pp2, ESTATE, ep.trace_lookahead)  # the last run is still the QMDP run
        still_runs()
        ctx.pbvi_set(al, act)
        ep.run_lookahead("pbvi", b0, starts, seed=1, placed=True)
        assert ep.alphas()[0].shape[0] == 5 and ep.results()["steps"].shape == (3,)
        still_runs()
        # a placed lookahead run builds no Q planes and has no alpha trace; its
        # own trace needs record_trace
        tr.run_lookahead("fib", b0, starts, seed=1, placed=True)
        fails(pp2, ESTATE, tr.trace_alpha)
        fails(pp2, ESTATE, tr.qplanes)
        tr.trace_lookahead()
        ep.run_lookahead("fib", b0, starts, seed=1, placed=True)
        fails(pp2, ESTATE, ep.trace_lookahead)
        fails(pp2, ESTATE, ep.trace_alpha)
        fails(pp2, ESTATE, ep.qplanes)
        r_ep, r_tr = ep.results(), tr.results()
        assert all(np.array_equal(r_ep[k], r_tr[k]) for k in r_ep)
