"""GPU: the tuning keys that choose a kernel instantiation (cells per lane,
PP2_TUNE_NT_STREAMS, with PP2_TUNE_CODED_MODEL deciding whether the dense
kernels run at all), each setting held to the CPU oracle at every kernel it
picks -- never to another setting of the device code.  tuning_cases.py has
the table of keys and read sites these cases are listed in, and
test_tuning_table_cpu.py what the shapes pin.

* Dense streaming kernels (k_belief_update, k_mdp_sweep, k_loop_step) at
  (cpt, nt, coded) = (4,1,0), (4,0,0), (2,.,.), (1,.,.): the raw belief of one
  update and J (as bit patterns) and A of three sweeps bit for bit; three
  loop steps as test_gpu_parity.py::test_loop_step_matches_separate_ops
  compares them (J and A bit for bit, the belief within rel 1e-5 of the
  oracle's per-step fp64-normalised one).
* The reference_order = 0 planner at 1, 2 and 4 cells per lane: the body of
  test_gpu_planner_shapes.py::test_default_order_one_expansion (one
  expansion, the fp64-accumulating oracle, rel 1e-5), then one more plan step
  onto a child the root's action sampled (materialize) and, in a second run,
  onto an observation it did not sample (a fresh root): the new root's
  belief and bounds.  The children of that second step are not compared:
  their samples are drawn from a cdf that differs between the two sides by
  rounding, so the kept sets may legitimately differ.

  launch_expand and launch_belief_dots have only <4> and <1> kernels.  When
  they sized the <1> launch by the context's 2 cells per lane, half the rows
  were never predicted, scored or reduced; every cpt2 case here then failed
  (delta_last has all its mass in the rows that were skipped)."""
import numpy as np
import pytest

import planner_shape_cases as PC
import tuning_cases as TC
from conftest import GAMMA, assert_rel_close
from planner_shape_run import context, host_models

pytestmark = pytest.mark.gpu

FTZ_FLOOR = 1e-30  # test_gpu_shards.py's: the order of the normalising sum


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@pytest.fixture(scope="module")
def host_model(oracle):
    """(T, L, R) of a planner table shape, generated once per shape."""
    return host_models(oracle)


@pytest.fixture(scope="module")
def dense_ref(oracle):
    """get(H, W, seed) -> the oracle's side of the dense cases of one shape,
    computed once: the model, the inputs, one raw belief update, three
    sweeps, three loop steps."""
    cache = {}

    def get(H, W, seed):
        if (H, W) in cache:
            return cache[(H, W)]
        from path_planning_2d_amd import synthetic as S
        grid, goal = TC.dense_grid(H, W, seed)
        T, L, _ = oracle.model_pomdp(grid, goal)
        _, Cc = oracle.model_mdp(grid, goal)
        us, zs, _ = S.synth_trajectory(grid, TC.DENSE_STEPS, seed=5)
        b0 = TC.spread_belief(grid)
        r = dict(grid=grid, goal=goal, b0=b0, us=us, zs=zs)
        r["raw"] = oracle.belief_update(H, W, T, L, b0, us[0], zs[0])
        b, J = b0, np.zeros(H * W, np.float32)
        for k in range(TC.DENSE_STEPS):
            b = oracle.belief_step(H, W, T, L, b, us[k], zs[k], mode="f64")
            J, A = oracle.mdp_sweep(H, W, GAMMA, T, Cc, J)
        r.update(b=b, J=J, A=A)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        cache[(H, W)] = r
        return r
    return get


def dense_ctx(pp2, ref, setting):
    """A context at one (cpt, nt, coded) setting, its coded model in the
    state the setting needs."""
    cpt, nt, coded = setting
    ctx = pp2.GridContext(ref["grid"], ref["goal"], gamma=float(GAMMA))
    try:
        ctx.set_cells_per_lane(cpt)
        ctx.set_tuning(ctx.TUNE_NT_STREAMS, nt)
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, coded)
        ctx.model_generate()
        entries, active = ctx.model_dict_info()
        assert entries > 0, "the generated model has a dictionary"
        assert active == TC.coded_expected(cpt, coded), (setting, active)
        assert not active, "a dense case runs the dense kernels"
    except BaseException:
        ctx.close()
        raise
    return ctx


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


DENSE = pytest.mark.parametrize("setting", TC.DENSE_SETTINGS, ids=TC.dense_id)
SHAPES = pytest.mark.parametrize("shape", TC.DENSE_SHAPES, ids=lambda s: PC.shape_id(s[:2]))


@DENSE
@SHAPES
def test_dense_belief_update(pp2, dense_ref, shape, setting):
    """k_belief_update<cpt>: the raw (unnormalised) belief bit for bit, its
    mass -- the sum of mass_partials(g, cpt) partials -- within the fp32 sum's
    error of the fp64 sum."""
    ref = dense_ref(*shape)
    with dense_ctx(pp2, ref, setting) as ctx:
        ctx.belief_set(ref["b0"])
        ctx.belief_update(int(ref["us"][0]), int(ref["zs"][0]))
        raw, mass = ctx.belief_get_raw()
    np.testing.assert_array_equal(bits(raw), bits(ref["raw"]))
    assert_rel_close(mass, ref["raw"].sum(dtype=np.float64), rel=2e-6, msg="mass")


@DENSE
@SHAPES
def test_dense_mdp_sweeps(pp2, dense_ref, shape, setting):
    """k_mdp_sweep<cpt, nt>: J as bit patterns and A after three sweeps."""
    ref = dense_ref(*shape)
    with dense_ctx(pp2, ref, setting) as ctx:
        ctx.mdp_reset()
        ctx.mdp_sweep(TC.DENSE_STEPS)
        J, A = ctx.mdp_get()
    np.testing.assert_array_equal(bits(J), bits(ref["J"]))
    np.testing.assert_array_equal(A, ref["A"])


@DENSE
@SHAPES
def test_dense_loop_steps(pp2, dense_ref, shape, setting):
    """k_loop_step<cpt, nt>, one launch per step: three steps against the
    oracle's separate update and sweep."""
    ref = dense_ref(*shape)
    with dense_ctx(pp2, ref, setting) as ctx:
        ctx.set_tuning(ctx.TUNE_RESIDENT, 0)
        ctx.set_tuning(ctx.TUNE_STEP_PAIRS, 0)
        ctx.belief_set(ref["b0"])
        ctx.mdp_reset()
        ctx.loop_run(ref["us"], ref["zs"])
        assert ctx.loop_steps_per_launch() == 1
        J, A = ctx.mdp_get()
        b = ctx.belief_get()
    np.testing.assert_array_equal(bits(J), bits(ref["J"]))
    np.testing.assert_array_equal(A, ref["A"])
    assert_rel_close(b, ref["b"], rel=1e-5, msg="loop belief")


# ------------------------------------------------- planner, default order
def planners(P, oracle, host_model, case):
    """The context, the device planner's arguments and the fp64-accumulating
    oracle planner of a case, as test_default_order_one_expansion sets them
    up."""
    H, W, kind, lb, cpt = case
    ctx, T, L, R = context(P, H, W, {"cpt": cpt}, host_model)
    try:
        alphas = ctx.fib_get()
        opl = oracle.Planner(PC.grid_of(H, W), T, L, R, alphas, max_depth=PC.MAX_DEPTH,
                             max_iter=1, accurate=True)
        if lb:
            pal, pact = PC.pbvi_of(H, W)
            ctx.pbvi_set(pal, pact)
            opl.set_pbvi(pal, pact)
    except BaseException:
        ctx.close()
        raise
    params = dict(max_search_tree_depth=PC.MAX_DEPTH, max_online_iteration=1,
                  lower_bound_mode=lb, rand_skip=0, reference_order=0)
    return ctx, (T, L), opl, params


def first_step(gpl, opl, b0, where):
    """The body of test_default_order_one_expansion; returns the oracle's
    action and tree snapshot."""
    a_g, v_g = gpl.step(0, 0, b0)
    a_o, v_o = opl.step(0, 0, b0)
    gi, oi = gpl.info(), opl.info()
    assert gi["expansions"] == 1 and gi["n_root_children"] == 9
    PC.compare(gi, oi, where, rel=1e-5)
    assert a_g == a_o, f"{where}: action {a_g} != {a_o}"
    assert PC.rel_close(v_g, v_o, rel=1e-5), f"{where}: value {v_g} != {v_o}"
    return a_o, oi


@pytest.mark.parametrize("case", TC.PLANNER_CASES, ids=TC.planner_case_id)
def test_default_order_by_cells_per_lane(pp2, oracle, host_model, case):
    """launch_expand and launch_belief_dots at the context's cells per lane:
    step 0 with one expansion against the fp64-accumulating oracle."""
    H, W, kind, _, _ = case
    ctx, _, opl, params = planners(pp2, oracle, host_model, case)
    with ctx:
        with pp2.QVTreePlanner(ctx, **params) as gpl:
            first_step(gpl, opl, PC.belief_of(H, W, kind), TC.planner_case_id(case))
    opl.close()


@pytest.mark.parametrize("sampled", [True, False], ids=["sampled_z", "fresh_root"])
@pytest.mark.parametrize("case", TC.PLANNER_CASES, ids=TC.planner_case_id)
def test_default_order_second_step(pp2, oracle, host_model, case, sampled):
    """One more plan step (launch_belief, mass_partials(g, cpt)): onto the
    child of an observation the root's action sampled (materialize), or onto
    one it did not (a fresh root) -- the likeliest of those.  The new root's
    belief against the oracle's belief update of b0 normalised in fp64, its
    bounds against the oracle planner's."""
    H, W, kind, _, _ = case
    where = f"{TC.planner_case_id(case)} {'sampled' if sampled else 'fresh'}"
    b0 = PC.belief_of(H, W, kind)
    ctx, (T, L), opl, params = planners(pp2, oracle, host_model, case)
    with ctx:
        with pp2.QVTreePlanner(ctx, **params) as gpl:
            a, oi = first_step(gpl, opl, b0, where)
            z_kept, others = TC.second_step_observations(oi, a)
            assert z_kept is not None and others, where
            if sampled:
                z, raw = z_kept, oracle.belief_update(H, W, T, L, b0, a, z_kept)
            else:
                z, raw = TC.likeliest(oracle, H, W, T, L, b0, a, others)
            assert (z in gpl.info()["q_obs"][a][:gpl.info()["q_nchildren"][a]]) == sampled
            want = oracle.normalize_f64(raw)[0]
            assert raw.sum(dtype=np.float64) > 0 and np.isfinite(want).all(), where
            before = gpl.info()["total_vnodes"]
            gpl.step(a, z)
            opl.step(a, z)
            gi, oi = gpl.info(), opl.info()
            assert gi["total_vnodes"] > 0 and before > 0
            assert_rel_close(gpl.root_belief(), want, rel=1e-5, abs_floor=FTZ_FLOOR,
                             msg=f"{where}: root belief after ({a}, {z})")
            for k in ("root_upper_bound", "root_lower_bound"):
                assert PC.rel_close(gi[k], oi[k], rel=1e-5), f"{where}: {k} {gi[k]} != {oi[k]}"
    opl.close()
