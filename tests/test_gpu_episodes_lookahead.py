"""GPU: one-step lookahead episodes (pp2_episodes_run_lookahead; the fourth
instance of k_episodes in csrc/pp2_episodes.hip) against the free-running NumPy
reference tests/episodes_lookahead_reference.py.  Everything is compared as
fp32 bit patterns: the reference restates every rounding of include/pp2.h
"episodes" / "Lookahead runs" and is fed the device's own alpha planes
(``alphas()``) and ``model_download``'s T, L, C, R.
"""
import ctypes as C

import numpy as np
import pytest

import episodes_alpha_reference as AR
import episodes_lookahead_reference as LR
import episodes_reference as R
from conftest import GAMMA, golden, golden_map

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = 5, 1
SYNTH = {"synth_97x131": (97, 131, 3), "synth_1x7": (1, 7, 1), "synth_5x1": (5, 1, 2)}
# the lookahead scratch on top of the MODE layout: two buffers of 16 x 4 sums
# per wave quad, and the 32 L classes' sixteen columns
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
    hw = grid.size
    al = np.random.default_rng(seed).normal(size=(S, hw)).astype(np.float32)
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


@pytest.fixture(scope="module")
def main_ctx(pp2):
    case = LR.look_case()
    ctx = make_ctx(pp2, case["grid"], case["goal"])
    m, Rw = model_of(ctx, case["grid"], case["goal"])
    yield case, ctx, m, Rw
    ctx.close()


def snapshot(ep, n):
    r = ep.results()
    return ([r[k][:n].copy() for k in ("steps", "status", "final_cell")]
            + [bits(r["cost"][:n]).copy()] + [bits(ep.belief(e)).copy() for e in range(n)])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 7. existing behaviour
# (first in the file: its "before" snapshots precede every lookahead run of
# the process)
def test_existing_policies_unchanged_by_lookahead_runs(pp2, main_ctx):
    case, ctx, m, Rw = main_ctx
    b0, starts = case["b0"], case["starts"]
    ctx.fib_sweep(3)
    al, act = synthetic_set(case["grid"], 21, inf_at=None)
    ctx.pbvi_set(al, act)

    def run(policy):
        with pp2.EpisodeBatch(ctx, 8, 8) as ep:
            info0 = ep.info()
            ep.run(policy, b0, starts, seed=9)
            return info0, ep.info(), snapshot(ep, 8)

    names = ("mode", "qmdp", "fib", "pbvi")
    before = {p: run(p) for p in names}
    with pp2.EpisodeBatch(ctx, 8, 8) as other:
        other.run("fib-lookahead", b0, starts, seed=9)
        other.run("pbvi-lookahead", b0, starts, seed=9)
        other.results()
        # ... and on the batch that ran lookahead
        for p in names:
            other.run(p, b0, starts, seed=9)
            assert same(snapshot(other, 8), before[p][2]), p
            assert other.info() == before[p][1], p
    for p in names:
        info0, info1, snap = run(p)
        assert info0 == before[p][0] and info1 == before[p][1] and same(snap, before[p][2]), p


# ---------------------------------------------------------------- 1. FIB parity
def test_fib_main_parity(pp2, main_ctx):
    case, ctx, m, Rw = main_ctx
    ctx.fib_solve()
    E, hz = len(case["starts"]), case["horizon"]
    with pp2.EpisodeBatch(ctx, E, hz, record_trace=True) as ep:
        assert ep.run("fib-lookahead", case["b0"], case["starts"], case["seed"]) is ep
        assert ep.lookahead and ep.alpha_set == 0 and ep.policy is None
        al, act = ep.alphas()
        np.testing.assert_array_equal(bits(al), bits(ctx.fib_get().T))
        np.testing.assert_array_equal(act, np.arange(9))
        ref = LR.run_lookahead_batch(m, Rw, al, case["b0"], case["starts"], hz, case["seed"],
                                     wp=ctx.row_stride)
        assert_lookahead_equal(ep, ref, "fib")
        s = ep.summary()
        ok = ref["status"] == 1
        assert s["success_rate"] == ok.mean() and s["lost"] == 0
        assert s["mean_steps"] == ref["steps"][ok].mean()
        assert s["mean_cost"] == ref["cost"].astype(np.float64).mean()
        # the paths of the case (test_episodes_lookahead_cpu.py asserts them on
        # the oracle's alphas): a goal, a full horizon, a step off the greedy policy
        assert ok.any() and (ref["status"] == 0).any()
        ep.run("fib", case["b0"], case["starts"], case["seed"])
        assert not ep.lookahead
        greedy = ep.trace()["actions"]
        assert (greedy[0] != ref["actions"][0]).any() or (greedy != ref["actions"]).any()


# ---------------------------------------------------------------- 2. PBVI parity
def test_pbvi_main_parity(pp2, main_ctx):
    case, ctx, m, Rw = main_ctx
    ctx.pbvi_belief_set(case["b0"], 21, rand_seed=1)
    ctx.pbvi_backup(12)
    starts = case["starts"][:6]
    with pp2.EpisodeBatch(ctx, 6, 8, record_trace=True) as ep:
        ep.run_lookahead("pbvi", case["b0"], starts, case["seed"])
        assert ep.lookahead and ep.alpha_set == 1
        al, act = ep.alphas()
        pa, pact = ctx.pbvi_get()
        assert al.shape[0] == 21  # five blocks of four and a tail of one
        np.testing.assert_array_equal(bits(al), bits(pa))
        np.testing.assert_array_equal(act, pact)
        ref = LR.run_lookahead_batch(m, Rw, al, case["b0"], starts, 8, case["seed"],
                                     wp=ctx.row_stride)
        assert_lookahead_equal(ep, ref, "pbvi")
    print(f"PBVI lookahead: leaf winners up to {ref['leaf_index'].max()}, actions "
          f"{np.unique(ref['actions'][ref['actions'] != 255]).tolist()}")
    assert ref["leaf_index"].max() >= 4  # a winner past the first block


@pytest.mark.parametrize("K", [70, 1, 2, 3])
def test_pbvi_small_grid_parity(pp2, K):
    """map_10x10: K = 70 (a winner >= 64, eighteen blocks), and the tail
    blocks of 1, 2 and 3 vectors on their own."""
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
        with pp2.EpisodeBatch(ctx, 3, 4, record_trace=True) as ep:
            ep.run("pbvi-lookahead", b0, starts, seed=3)
            al, act = ep.alphas()
            np.testing.assert_array_equal(bits(al), bits(al_s))
            ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, 4, 3, wp=ctx.row_stride)
            assert_lookahead_equal(ep, ref, f"K = {K}")
    if K == 70:
        assert ref["leaf_index"].max() >= 64
    assert (ref["steps"] > 0).any()


# ---------------------------------------------------------------- 3. edge geometry
@pytest.mark.parametrize("name", ["synth_1x7", "synth_5x1", "map_3x3", "map_10x10",
                                  "synth_97x131"])
def test_edge_geometry(pp2, name):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    H, W = grid.shape
    hw = H * W
    flat = grid.reshape(-1)
    occ = np.flatnonzero(flat == 1)
    free = np.flatnonzero(flat == 0)
    goal_cell = goal[1] * W + goal[0]
    b0 = S.uniform_belief(grid)
    big = name == "synth_97x131"
    # on the goal, both far corners, an occupied cell (if any), free cells
    starts = np.array([goal_cell, hw - 1, W - 1, occ[0] if occ.size else hw // 2,
                       free[len(free) // 2], free[len(free) // 3], free[-1], free[0]], np.int32)
    E, hz = (4, 3) if big else (8, 6)
    starts = starts[:E]
    al_s, act_s = synthetic_set(grid, 10)
    with make_ctx(pp2, grid, goal) as ctx:
        if big:
            assert ctx.row_stride == 132 and W % 4 != 0
        m, Rw = model_of(ctx, grid, goal)
        ctx.fib_sweep(9)
        ctx.pbvi_set(al_s, act_s)
        with pp2.EpisodeBatch(ctx, E, hz, record_trace=True) as ep:
            for which in ("pbvi", "fib") if not big else ("pbvi",):
                ep.run_lookahead(which, b0, starts, seed=77)
                al, act = ep.alphas()
                if which == "pbvi":
                    np.testing.assert_array_equal(bits(al), bits(al_s))
                    np.testing.assert_array_equal(act, act_s)
                ref = LR.run_lookahead_batch(m, Rw, al, b0, starts, hz, 77, wp=ctx.row_stride)
                assert_lookahead_equal(ep, ref, f"{name} {which}")
                assert ref["steps"][0] == 0 and ref["status"][0] == 1
                if which == "pbvi" and occ.size:
                    # the vector with +inf where every update is 0 has NaN sums
                    # and never wins a leaf
                    a_pad = R.pad_plane(al, H, W, ctx.row_stride)
                    took = np.flatnonzero(ref["steps"] > 0)
                    assert took.size
                    for u in (0, 4, 8):
                        raw = np.stack([LR.O.belief_update(H, W, m.T, m.L, b0, u, z)
                                        for z in range(16)])
                        V = LR.adot_pinned_zk(R.pad_plane(raw, H, W, ctx.row_stride), a_pad)
                        assert np.isnan(V[:, 3]).all()
                    taken = ref["leaf_index"][ref["actions"] != 255]
                    assert taken.size and (taken != 3).all() and (taken >= 0).all()


# ---------------------------------------------------------------- 4. persistent workgroups, reruns
def test_batch_invariance_and_reruns(pp2, main_ctx):
    case, ctx, m, Rw = main_ctx
    free = np.flatnonzero(case["grid"].reshape(-1) == 0)
    starts = free[np.arange(700) * 5 % free.size].astype(np.int32)
    b0 = case["b0"]
    ctx.fib_solve()
    al70, act70 = synthetic_set(case["grid"], 70, seed=6, inf_at=None)
    al12, act12 = al70[:12] * np.float32(-1.0), act70[:12]
    with pp2.EpisodeBatch(ctx, 700, 4) as big, pp2.EpisodeBatch(ctx, 5, 4) as small:
        big.run("fib-lookahead", b0, starts, seed=11)
        small.run("fib-lookahead", b0, starts[:5], seed=11)
        look5 = snapshot(small, 5)
        assert same(snapshot(big, 5), look5)
        with pp2.EpisodeBatch(ctx, 1000, 4) as huge:
            s1000 = np.concatenate([starts, starts[:300]])
            huge.run("fib-lookahead", b0, s1000, seed=11)
            # workgroups take a second episode in both
            assert big.info()["workgroups"] < 700 and huge.info()["workgroups"] < 1000
            assert same(snapshot(huge, 5), look5)
            r700, r1000 = big.results(), huge.results()
            for k in ("steps", "status", "final_cell"):
                assert np.array_equal(r700[k], r1000[k][:700]), k
            assert np.array_equal(bits(r700["cost"]), bits(r1000["cost"][:700]))
            # ... and episodes that a workgroup took second are the reference's
            # (a pred plane whose halo or pads were left dirty shows here)
            al, act = huge.alphas()
            wgs = huge.info()["workgroups"]
            for e in sorted({min(wgs, 999), 999}):
                o = LR.run_lookahead_episode(m, Rw, al, b0, int(s1000[e]), 4, 11, e,
                                             wp=ctx.row_stride)
                assert (o["steps"], o["status"], o["final_cell"]) == (
                    r1000["steps"][e], r1000["status"][e], r1000["final_cell"][e]), e
                assert bits(o["cost"]) == bits(r1000["cost"][e]), e
                assert np.array_equal(bits(o["belief"]), bits(huge.belief(e))), e
        # lookahead then QMDP, and QMDP then lookahead, each equal a fresh batch
        small.run("qmdp", b0, starts[:5], seed=11)
        qmdp5 = snapshot(small, 5)
        small.run("fib-lookahead", b0, starts[:5], seed=11)
        assert same(snapshot(small, 5), look5)
        with pp2.EpisodeBatch(ctx, 5, 4) as fresh:
            fresh.run("qmdp", b0, starts[:5], seed=11)
            assert same(snapshot(fresh, 5), qmdp5)
            fresh.run("fib-lookahead", b0, starts[:5], seed=11)
            assert same(snapshot(fresh, 5), look5)
        # K from 12 to 70 and back to 12
        ctx.pbvi_set(al12, act12)
        small.run("pbvi-lookahead", b0, starts[:5], seed=11)
        assert small.alphas()[0].shape[0] == 12
        p12 = snapshot(small, 5)
        ctx.pbvi_set(al70, act70)
        small.run("pbvi-lookahead", b0, starts[:5], seed=11)
        a70, _ = small.alphas()
        np.testing.assert_array_equal(bits(a70), bits(al70))
        p70 = snapshot(small, 5)
        with pp2.EpisodeBatch(ctx, 5, 4) as fresh:
            fresh.run("pbvi-lookahead", b0, starts[:5], seed=11)
            assert same(snapshot(fresh, 5), p70)
        ctx.pbvi_set(al12, act12)
        small.run("pbvi-lookahead", b0, starts[:5], seed=11)
        assert same(snapshot(small, 5), p12)
        with pp2.EpisodeBatch(ctx, 5, 4) as fresh:
            fresh.run("pbvi-lookahead", b0, starts[:5], seed=11)
            assert same(snapshot(fresh, 5), p12)


# ---------------------------------------------------------------- 5. errors
def test_errors(pp2):
    from path_planning_2d_amd import _lib
    from path_planning_2d_amd import synthetic as S
    assert _lib.STATUS_NAMES[ESTATE] == "PP2_ESTATE" and _lib.STATUS_NAMES[EINVAL] == "PP2_EINVAL"
    grid, goal = load_grid("map_10x10")
    H, W = grid.shape
    b0 = S.uniform_belief(grid)

    def fails(status, fn, *args):
        with pytest.raises(pp2.Pp2Error) as e:
            fn(*args)
        assert e.value.status == status, (fn, args)

    with make_ctx(pp2, grid, goal) as ctx, pp2.EpisodeBatch(ctx, 3, 4) as ep, \
            pp2.EpisodeBatch(ctx, 3, 4, record_trace=True) as tr:
        m, Rw = model_of(ctx, grid, goal)

        def run_look(which, b, starts, batch=ep):
            b = np.ascontiguousarray(b, np.float32)
            st = np.ascontiguousarray(starts, np.int32)
            _lib.call("pp2_episodes_run_lookahead", batch._h, which, C.c_uint64(1),
                      b.ctypes.data_as(C.POINTER(C.c_float)),
                      st.ctypes.data_as(C.POINTER(C.c_int32)))

        # nothing has run
        fails(ESTATE, tr.trace_lookahead)
        fails(ESTATE, ep.trace_lookahead)
        # PBVI without alpha vectors; unknown sets; bad b0 / starts
        fails(ESTATE, run_look, 1, b0, [0, 1, 2])
        neg = b0.copy()
        neg[5] = -0.25
        for args in ((2, b0, [0, 1, 2]), (-1, b0, [0, 1, 2]), (0, b0, [0, 1, H * W]),
                     (0, b0, [0, -1, 2]), (0, neg, [0, 1, 2])):
            fails(EINVAL, run_look, *args)
        fails(ESTATE, tr.trace_lookahead)  # a refused run is no run
        # FIB never solved: valid, on the zero alphas the control is the argmax of rew
        tr.run_lookahead("fib", b0, [0, 1, 2], seed=1)
        al, act = tr.alphas()
        assert not al.any() and np.array_equal(act, np.arange(9))
        tl, t = tr.trace_lookahead(), tr.trace()
        taken = t["actions"] != 255
        assert taken.any() and not tl["leaf_max"].any()
        assert set(np.unique(tl["leaf_index"]).tolist()) <= {-1, 0}
        np.testing.assert_array_equal(bits(tl["q"]), bits(tl["rewards"] + np.float32(0.0)))
        np.testing.assert_array_equal(bits(t["qsums"]), bits(tl["q"]))
        want = np.array([AR.pick(r) for r in tl["rewards"][taken]])
        np.testing.assert_array_equal(t["actions"][taken], want)
        assert (t["mode_cells"] == -1).all()
        ref = LR.run_lookahead_batch(m, Rw, al, b0, [0, 1, 2], 4, 1, wp=ctx.row_stride)
        assert_lookahead_equal(tr, ref, "zero alphas")
        # a lookahead run builds no Q planes and has no alpha trace; its own
        # trace needs record_trace
        fails(ESTATE, tr.qplanes)
        fails(ESTATE, tr.trace_alpha)
        run_look(0, b0, [0, 1, 2])
        fails(ESTATE, ep.trace_lookahead)
        fails(ESTATE, ep.qplanes)
        ep.alphas()
        # after a QMDP or an alpha run the lookahead trace refuses again
        tr.run("qmdp", b0, [0, 1, 2], seed=1)
        fails(ESTATE, tr.trace_lookahead)
        tr.qplanes()
        tr.run("fib", b0, [0, 1, 2], seed=1)
        fails(ESTATE, tr.trace_lookahead)
        tr.trace_alpha()
        # the coded model switched off after create: re-checked at run
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        fails(ESTATE, run_look, 0, b0, [0, 1, 2])
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 1)
        run_look(0, b0, [0, 1, 2])
        assert ep.results()["steps"].shape == (3,)


# ---------------------------------------------------------------- 6. LDS
def test_lds_with_lookahead_scratch_must_fit(pp2):
    """111 x 131 (row stride 132): the MODE / QMDP layout fits the 160 KiB of a
    CU with less than the lookahead scratch to spare (as
    test_lds_with_alpha_scratch_must_fit derives it), so a greedy FIB run is
    admitted and a lookahead run is refused before any launch."""
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(111, 131, 3)
    grid[0, 0] = 0
    b0 = S.uniform_belief(grid)
    with make_ctx(pp2, grid, (0, 0), solve=False) as ctx, pp2.EpisodeBatch(ctx, 2, 2) as ep:
        base = ep.info()
        assert base["lds_bytes"] <= 160 * 1024 < base["lds_bytes"] + SCRATCH, base
        with pytest.raises(pp2.Pp2Error) as e:
            ep.run("fib-lookahead", b0, [0, 1])
        assert e.value.status == EINVAL
        assert ep.info() == base
        with pytest.raises(pp2.Pp2Error) as e:
            ep.results()  # nothing was launched
        assert e.value.status == ESTATE
        ep.run("fib", b0, [0, 1])
        assert ep.results()["steps"].shape == (2,) and ep.info() == base


def test_info_reports_the_lookahead_launch(pp2):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("map_10x10")
    b0 = S.uniform_belief(grid)
    with make_ctx(pp2, grid, goal) as ctx, pp2.EpisodeBatch(ctx, 4, 2) as ep:
        base = ep.info()
        ep.run("fib-lookahead", b0, [0, 1, 2, 3])
        info = ep.info()
        assert info["lds_bytes"] == base["lds_bytes"] + SCRATCH
        assert info["threads"] == base["threads"] and 1 <= info["workgroups"] <= 4
        ep.run("mode", b0, [0, 1, 2, 3])
        assert ep.info() == base
