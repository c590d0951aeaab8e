"""How a reference-order case of planner_shape_cases.py is run on the device:
shared by test_gpu_planner_shapes.py, test_gpu_planner_switches.py and
planner_switch_child.py (the child process of the switches that are cached
per process), so that all three hold a case to the oracle in the same way.

The device planner and the reference-arithmetic oracle run in lockstep; the
whole tree snapshot, the action and the value are held equal bit for bit at
step 0 and at every following step."""
import ctypes as C

import numpy as np

import planner_shape_cases as PC


def host_models(oracle):
    """get(H, W) -> (T, L, R) of a table shape, generated once per shape."""
    cache = {}

    def get(H, W):
        if (H, W) not in cache:
            cache[(H, W)] = oracle.model_pomdp(PC.grid_of(H, W), PC.goal_of(H, W))
        return cache[(H, W)]
    return get


def debug_switch(name):
    """The library's pp2_debug_<name>(int) -> previous value."""
    from path_planning_2d_amd import _lib
    f = getattr(_lib.load(), "pp2_debug_" + name)
    f.argtypes = [C.c_int]
    f.restype = C.c_int
    return f


def context(P, H, W, sw, host_model):
    """A context with its model and FIB alphas in place, and the model the
    oracle gets: (ctx, T, L, R)."""
    grid = PC.grid_of(H, W)
    ctx = P.GridContext(grid, PC.goal_of(H, W), gamma=float(PC.GAMMA))
    try:
        ctx.model_generate()
        T, L, R = host_model(H, W)
        if sw.get("off_support"):
            # one T entry outside its action's support: the coded model stays,
            # its sparse dictionary does not (k_tree_pred<false>)
            T, _ = PC.off_support_model(grid, T)
            Td, Ld, Rd, Cd = ctx.model_download()
            assert np.array_equal(Ld, L) and np.array_equal(Rd, R)
            ctx.model_upload(T, Ld, Rd, Cd)
            assert np.array_equal(ctx.model_download()[0].reshape(T.shape), T)
        if "coded" in sw:
            ctx.set_tuning(ctx.TUNE_CODED_MODEL, int(sw["coded"]))
        if "cpt" in sw:
            ctx.set_cells_per_lane(int(sw["cpt"]))
        # the coded model is active at 4 cells per lane only
        assert ctx.model_dict_info()[1] == (bool(sw.get("coded", 1)) and
                                            int(sw.get("cpt", 4)) == 4)
        ctx.fib_solve(max_sweeps=40)
    except BaseException:
        ctx.close()
        raise
    return ctx, T, L, R


def run_reference_order(P, oracle, host_model, case, monkeypatch, fc_walk):
    """One reference-order case: the device planner and the oracle in
    lockstep, held equal at every step."""
    H, W, kind, lb, steps, sw = case
    for k, v in sw.items():
        if k.startswith("PP2_"):
            monkeypatch.setenv(k, v)
    if "fc_walk" in sw:
        fc_walk(sw["fc_walk"])
    where = PC.ref_case_id(case)
    grid = PC.grid_of(H, W)
    b0 = PC.belief_of(H, W, kind)
    zs = PC.zs_of(H, W, steps)
    ctx, T, L, R = context(P, H, W, sw, host_model)
    with ctx:
        alphas = ctx.fib_get()
        rpl = oracle.Planner(grid, T, L, R, alphas, max_depth=PC.MAX_DEPTH,
                             max_iter=PC.MAX_ITER)
        if lb:
            pal, pact = PC.pbvi_alphas(H, W, sw)
            ctx.pbvi_set(pal, pact)
            rpl.set_pbvi(pal, pact)
        with P.QVTreePlanner(ctx, max_search_tree_depth=PC.MAX_DEPTH,
                             max_online_iteration=PC.MAX_ITER, lower_bound_mode=lb,
                             rand_skip=0, reference_order=1) as gpl:
            a_r = 0
            for k in range(steps + 1):
                # both planners get the oracle's action and the seeded z
                msg = (0, 0, b0) if k == 0 else (a_r, zs[k - 1])
                a_g, v_g = gpl.step(*msg)
                a_r, v_r = rpl.step(*msg)
                gi = gpl.info()
                PC.compare_exact(gi, rpl.info(), f"{where} step {k}")
                assert a_g == a_r, f"{where} step {k}: action {a_g} != {a_r}"
                assert PC.f32_bits(v_g) == PC.f32_bits(v_r), f"{where} step {k}: {v_g} != {v_r}"
                assert gi["expansions"] > 0 and gi["total_vnodes"] > 0
        rpl.close()
