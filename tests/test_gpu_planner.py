"""GPU parity of the QV-tree planner (C++ tree over batched gfx950 expansion
passes) against the oracle's reference-semantics tree (every node holding
its own host belief, sequential fp32 sums).

Both draw the reference's samples: glibc rand() state samples over the fp32
prefix sum of the node belief, and the cuRAND XORWOW uniforms of
curand_init(1234, i, 0).  Tree shape (children, observations, weights,
depth, expansions) must match exactly.  Bounds and rewards are sums over the
whole grid: against the oracle in fp64-accumulation mode they must agree to
rel 1e-5 at every step (and the trees stay identical).  Against the
reference-arithmetic oracle (sequential fp32 sums, whose own error is
~sqrt(hw)*eps*|value|) the fresh, shallow (<= 2 expansions) tree of the
first step must have the same shape and values within rel 1e-4: that fp32
noise alone can flip a near-tied expansion choice deeper in.  The planner's
reference_order mode runs those sums as the reference's own x-ordered fp32
chains, and is held to the reference-arithmetic oracle bit for bit at every
step (test_planner_reference_order_bit_exact)."""
import numpy as np
import pytest

from conftest import GAMMA, golden, golden_map
# (the snapshot comparisons are shared with test_gpu_planner_shapes.py)
from planner_shape_cases import compare, compare_exact, rel_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,max_depth,max_iter,steps", [
    ("map_10x10", 50, 15, 6),
    ("sparse_map_100x40", 3, 15, 8),
    ("sparse_map_100x40", 50, 15, 4),
    ("tile64_sparse_map_100x40", 5, 15, 5),
])
def test_planner_matches_oracle(oracle, name, max_depth, max_iter, steps):
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    grid = golden_map(name)
    m = golden("model", name)
    H, W = grid.shape
    with P.GridContext(grid, tuple(m["goal"]), gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        alphas = ctx.fib_get()
        a_ref, _, _ = oracle.fib_solve(H, W, GAMMA, m["T"], m["L"], m["R"])
        np.testing.assert_array_equal(alphas, a_ref)
        opl = oracle.Planner(grid, m["T"], m["L"], m["R"], alphas,
                             max_depth=max_depth, max_iter=max_iter, accurate=True)
        rpl = oracle.Planner(grid, m["T"], m["L"], m["R"], alphas,
                             max_depth=max_depth, max_iter=max_iter)
        with P.QVTreePlanner(ctx, max_search_tree_depth=max_depth,
                             max_online_iteration=max_iter, reference_order=0) as gpl:
            _, zs, _ = S.synth_trajectory(grid, steps, seed=7)
            b0 = S.uniform_belief(grid)
            a_g, v_g = gpl.step(0, 0, b0)
            a_o, v_o = opl.step(0, 0, b0)
            a_r, v_r = rpl.step(0, 0, b0)
            compare(gpl.info(), opl.info(), f"{name} step 0")
            if max_depth <= 5:  # few expansions: no room for a near-tie flip
                compare(gpl.info(), rpl.info(), f"{name} step 0 (ref)", rel=1e-4)
            assert a_g == a_o
            assert rel_close(v_g, v_o)
            for k in range(steps):
                # all planners receive the oracle's action and the same z;
                # z may or may not exist under the root (re-root vs new root)
                a_in = a_o
                a_g, v_g = gpl.step(a_in, int(zs[k]))
                a_o, v_o = opl.step(a_in, int(zs[k]))
                compare(gpl.info(), opl.info(), f"{name} step {k + 1}")
                assert a_g == a_o, f"{name} step {k + 1}: action {a_g} != {a_o}"
                assert rel_close(v_g, v_o)
            gpl.reset()
            assert gpl.info()["total_vnodes"] == 0
    opl.close()
    rpl.close()


def test_planner_256_plan_step(oracle):
    """BASELINE config 2 shape: 256x256 synthetic grid, depth 3."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(256, 256, 256)
    goal = S.synth_goal(grid)
    with P.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve(max_sweeps=40)
        alphas = ctx.fib_get()
        T, L, R = oracle.model_pomdp(grid, goal)
        opl = oracle.Planner(grid, T, L, R, alphas, max_depth=3, max_iter=15,
                             accurate=True)
        with P.QVTreePlanner(ctx, max_search_tree_depth=3, max_online_iteration=15,
                             reference_order=0) as gpl:
            b0 = S.uniform_belief(grid)
            a_g, _ = gpl.step(0, 0, b0)
            a_o, _ = opl.step(0, 0, b0)
            compare(gpl.info(), opl.info(), "256 step 0")
            assert a_g == a_o
            _, zs, _ = S.synth_trajectory(grid, 2, seed=3)
            for k in range(2):
                a_g, _ = gpl.step(a_o, int(zs[k]))
                a_o, _ = opl.step(a_o, int(zs[k]))
                compare(gpl.info(), opl.info(), f"256 step {k + 1}")
                assert a_g == a_o
        opl.close()


def test_planner_cdf_zero_block_skip_exact(oracle, monkeypatch):
    """The host cdf skips 16-cell blocks without mass (adding +0 leaves the
    fp32 running sum bit-identical): on a belief that is zero outside a band
    of rows, plans with the skip (default) and without it (PP2_CDF_SKIP=0)
    are identical, and equal the oracle's."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    name = "sparse_map_100x40"
    grid = golden_map(name)
    m = golden("model", name)
    H, W = grid.shape
    b0 = S.uniform_belief(grid).reshape(H, W).copy()
    b0[:12] = 0.0
    b0[20:] = 0.0
    b0 = (b0 / b0.sum(dtype=np.float64)).astype(np.float32).ravel()
    _, zs, _ = S.synth_trajectory(grid, 4, seed=11)
    runs = []
    with P.GridContext(grid, tuple(m["goal"]), gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        alphas = ctx.fib_get()
        for skip in ("1", "0"):
            monkeypatch.setenv("PP2_CDF_SKIP", skip)
            infos = []
            with P.QVTreePlanner(ctx, max_search_tree_depth=5, max_online_iteration=15,
                                 reference_order=0) as gpl:
                a, v = gpl.step(0, 0, b0)
                infos.append((a, v, gpl.info()))
                for k in range(4):
                    a, v = gpl.step(a, int(zs[k]))
                    infos.append((a, v, gpl.info()))
            runs.append(infos)
        opl = oracle.Planner(grid, m["T"], m["L"], m["R"], alphas, max_depth=5, max_iter=15,
                             accurate=True)
        a_o, v_o = opl.step(0, 0, b0)
        compare(runs[0][0][2], opl.info(), "skip step 0")
        assert runs[0][0][0] == a_o
        opl.close()
    for (a1, v1, i1), (a0, v0, i0) in zip(*runs):
        assert a1 == a0 and np.float32(v1) == np.float32(v0)
        for k in i1:
            assert np.array_equal(np.asarray(i1[k]), np.asarray(i0[k])), k


@pytest.mark.parametrize("name,S,max_depth,steps", [
    ("map_10x10", 64, 50, 5),
    ("sparse_map_100x40", 500, 5, 4),   # the reference node: S = 500, PBVI leaves
])
def test_planner_pbvi_lower_bound(oracle, name, S, max_depth, steps):
    """lower_bound_mode 1: every VNode's lower bound is evaluatePbviCpu over
    the context's PBVI alphas (search_tree_cuda.cu:379), and the tree's rand()
    stream continues after generateBeliefSet's draws, as in the reference node
    (PomdpPathPlanning2d::initialize runs PBVI before the first plan step)."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S_
    grid = golden_map(name)
    m = golden("model", name)
    b0 = S_.uniform_belief(grid)
    with P.GridContext(grid, tuple(m["goal"]), gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        alphas = ctx.fib_get()
        calls = ctx.pbvi_solve(b0, S)
        pal, pact = ctx.pbvi_get()
        opl = oracle.Planner(grid, m["T"], m["L"], m["R"], alphas, max_depth=max_depth,
                             max_iter=15, accurate=True)
        opl.set_pbvi(pal, pact)
        opl.skip_rand(calls)
        with P.QVTreePlanner(ctx, max_search_tree_depth=max_depth, max_online_iteration=15,
                             lower_bound_mode=1, rand_skip=calls, reference_order=0) as gpl:
            a_g, v_g = gpl.step(0, 0, b0)
            a_o, v_o = opl.step(0, 0, b0)
            gi = gpl.info()
            compare(gi, opl.info(), f"{name} pbvi step 0")
            assert a_g == a_o and rel_close(v_g, v_o)
            # PBVI is a lower bound: nowhere above the FIB upper bound
            assert gi["root_lower_bound"] <= gi["root_upper_bound"] + 1e-3
            assert gi["root_lower_bound"] > -5.0 / (1.0 - 0.95)
            _, zs, _ = S_.synth_trajectory(grid, steps, seed=11)
            for k in range(steps):
                a_g, v_g = gpl.step(a_o, int(zs[k]))
                a_o, v_o = opl.step(a_o, int(zs[k]))
                compare(gpl.info(), opl.info(), f"{name} pbvi step {k + 1}")
                assert a_g == a_o and rel_close(v_g, v_o)
    opl.close()


@pytest.mark.parametrize("name,max_depth,lb,S,steps,seq_max,walk", [
    ("map_10x10", 50, 0, 0, 8, None, None),
    ("sparse_map_100x40", 50, 0, 0, 6, None, None),
    ("sparse_map_100x40", 5, 1, 500, 5, None, None),    # the reference node: PBVI leaves, S = 500
    ("tile64_sparse_map_100x40", 8, 1, 64, 6, None, None),
    # the same small grids on the exact parallel chain sets (pp2_fchain.hip)
    # instead of the walked chains (k_chain_walk, the default up to 8192 cells)
    ("sparse_map_100x40", 50, 0, 0, 6, "0", None),
    ("sparse_map_100x40", 5, 1, 500, 3, "0", None),
    ("tile64_sparse_map_100x40", 8, 1, 64, 4, "0", None),
    # and on the walk with its terms formed beside it (k_chain_walk2)
    ("map_10x10", 50, 0, 0, 4, None, "2"),
    ("sparse_map_100x40", 5, 1, 500, 3, None, "2"),
    # and the chain sets with the FIB candidate masks (PP2_FIB_CANDS=1: the
    # kept children's dots certainly below another skipped; on these grids
    # most are)
    ("sparse_map_100x40", 50, 0, 0, 6, "0", "cands"),
    ("sparse_map_100x40", 5, 1, 500, 3, "0", "cands"),
    # and with the cdf chain enqueued before the predictions (PP2_ROW_FIRST=1)
    ("sparse_map_100x40", 5, 1, 500, 3, "0", "rowfirst"),
])
def test_planner_reference_order_bit_exact(oracle, monkeypatch, name, max_depth, lb, S, steps,
                                           seq_max, walk):
    """reference_order = 1: rewards, renormalisations and leaf bounds run as
    the reference's own x-ordered fp32 chains (inner_product / accumulate,
    search_tree_cuda.cu:168-173, :225-229; evaluateFibCpu, evaluatePbviCpu),
    so the tree equals the reference-arithmetic oracle at EVERY plan step:
    shape, observations, weights, bounds, rewards, heuristics bit for bit, and
    the chosen action and its value exactly -- deep trees included, where the
    fp64-accumulating mode may legitimately pick another near-tied node.
    Grids up to PP2_SEQ_CHAIN_MAX cells (seq_max; default 8192) run the sums
    as walked chains, larger ones as exact parallel chain sets; seq_max "0"
    forces the latter on the small grids, walk "2" the walk whose terms are
    formed beside it (PP2_CHAIN_WALK), walk "cands" the FIB candidate masks,
    "rowfirst" the cdf chain enqueued first."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S_
    if seq_max is not None:
        monkeypatch.setenv("PP2_SEQ_CHAIN_MAX", seq_max)
    if walk == "cands":
        monkeypatch.setenv("PP2_FIB_CANDS", "1")
    elif walk == "rowfirst":
        monkeypatch.setenv("PP2_ROW_FIRST", "1")
    elif walk is not None:
        monkeypatch.setenv("PP2_CHAIN_WALK", walk)
    grid = golden_map(name)
    m = golden("model", name)
    b0 = S_.uniform_belief(grid)
    with P.GridContext(grid, tuple(m["goal"]), gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        alphas = ctx.fib_get()
        calls = 0
        rpl = oracle.Planner(grid, m["T"], m["L"], m["R"], alphas, max_depth=max_depth,
                             max_iter=15)
        if lb:
            calls = ctx.pbvi_solve(b0, S)
            pal, pact = ctx.pbvi_get()
            rpl.set_pbvi(pal, pact)
            rpl.skip_rand(calls)
        with P.QVTreePlanner(ctx, max_search_tree_depth=max_depth, max_online_iteration=15,
                             lower_bound_mode=lb, rand_skip=calls, reference_order=1) as gpl:
            a_g, v_g = gpl.step(0, 0, b0)
            a_r, v_r = rpl.step(0, 0, b0)
            compare_exact(gpl.info(), rpl.info(), f"{name} ref step 0")
            assert a_g == a_r and np.float32(v_g) == np.float32(v_r)
            _, zs, _ = S_.synth_trajectory(grid, steps, seed=5)
            for k in range(steps):
                a_g, v_g = gpl.step(a_r, int(zs[k]))
                a_r, v_r = rpl.step(a_r, int(zs[k]))
                compare_exact(gpl.info(), rpl.info(), f"{name} ref step {k + 1}")
                assert a_g == a_r, f"{name} step {k + 1}: action {a_g} != {a_r}"
                assert np.float32(v_g) == np.float32(v_r)
    rpl.close()


def lockstep(gpl, rpl, where):
    """A closed-loop step function that steps the GPU planner and the
    reference-arithmetic oracle with the same message and holds them equal:
    the whole tree snapshot bit for bit, the action and its value."""
    k = [0]

    def step(a, z, b):
        a_g, v_g = gpl.step(a, z, b)
        a_r, v_r = rpl.step(a, z, b)
        compare_exact(gpl.info(), rpl.info(), f"{where} step {k[0]}")
        assert a_g == a_r, f"{where} step {k[0]}: action {a_g} != {a_r}"
        assert np.float32(v_g).view(np.uint32) == np.float32(v_r).view(np.uint32)
        k[0] += 1
        return a_g, v_g
    return step


def test_planner_reference_order_256(oracle):
    """BASELINE configs[1] exactly as bench.py times it: 256x256 synthetic
    grid, max_search_tree_depth 3, the converged FIB (fib_solve without a
    sweep cap), 24 steps of the bench's seeded closed loop
    (synthetic.closed_loop) -- bit-exact with the reference-arithmetic oracle
    at every step."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S_
    grid = S_.synth_grid(256, 256, 256)
    goal = S_.synth_goal(grid)
    with P.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        alphas = ctx.fib_get()
        T, L, R = oracle.model_pomdp(grid, goal)
        rpl = oracle.Planner(grid, T, L, R, alphas, max_depth=3, max_iter=15)
        with P.QVTreePlanner(ctx, max_search_tree_depth=3, max_online_iteration=15,
                             reference_order=1) as gpl:
            _, acts, _ = S_.closed_loop(grid, S_.uniform_belief(grid),
                                        lockstep(gpl, rpl, "256 ref"), 24)
        rpl.close()
    assert acts.size == 24


def test_planner_reference_order_pbvi_256(oracle):
    """The 256x256 PBVI-leaf plan step of bench.py (plan_step_pbvi_lb):
    lower_bound_mode 1 over the GPU's S = 500 PBVI alphas (generateBeliefSet
    + 167 backups), reference order, the tree's rand() stream continuing
    after the belief set's draws; the oracle gets the same alphas
    (set_pbvi) and is held bit-exact over 4 closed-loop steps."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S_
    grid = S_.synth_grid(256, 256, 256)
    goal = S_.synth_goal(grid)
    b0 = S_.uniform_belief(grid)
    with P.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        ctx.fib_solve()
        calls = ctx.pbvi_solve(b0, 500)
        pal, pact = ctx.pbvi_get()
        T, L, R = oracle.model_pomdp(grid, goal)
        rpl = oracle.Planner(grid, T, L, R, ctx.fib_get(), max_depth=3, max_iter=15)
        rpl.set_pbvi(pal, pact)
        rpl.skip_rand(calls)
        with P.QVTreePlanner(ctx, max_search_tree_depth=3, max_online_iteration=15,
                             lower_bound_mode=1, rand_skip=calls, reference_order=1) as gpl:
            S_.closed_loop(grid, b0, lockstep(gpl, rpl, "256 pbvi ref"), 4)
            gi = gpl.info()
        rpl.close()
    assert gi["root_lower_bound"] > -5.0 / (1.0 - 0.95)


def test_planner_pbvi_needs_alphas():
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S_
    g = S_.synth_grid(12, 12, 2)
    g[0, 0] = 0
    with P.GridContext(g, (0, 0), gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        with pytest.raises(P.Pp2Error):
            P.QVTreePlanner(ctx, lower_bound_mode=1)
        with pytest.raises(P.Pp2Error):
            P.QVTreePlanner(ctx, lower_bound_mode=2)


def test_c_client_runs(tmp_path):
    """The plain-C node sequence (examples/pp2_node_demo.c, built by the
    csrc Makefile): planner with PBVI bounds, loop steps and the reference
    text files, all through include/pp2.h."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "pp2_node_demo")
    assert os.path.exists(exe), "build with make -C path_planning_2d_amd/csrc"
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "pp2_node_demo ok" in out.stdout
    for f in ("model_data_trans_prob", "fib_alphas", "fib_actions", "pbvi_alphas",
              "pbvi_actions"):
        assert (tmp_path / f).exists(), f
