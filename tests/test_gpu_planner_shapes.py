"""GPU parity of the QV-tree planner with the CPU oracle at the grid sizes its
passes branch on (planner_shape_cases.SHAPES): one row, one column, the last
size on the walked chains and the first on the chain sets, a ragged last
16-cell block of the sampler's first search with every LDS slot taken, the
plain binary search above 65536 cells, and more chunks than k_fc_walk holds
(k_fc_drive by the planner's own choice).  test_gpu_planner.py runs the
bench's shapes; test_gpu_fchain.py the chain kernels on single rows.

reference_order = 1 is held to the reference-arithmetic oracle bit for bit
at step 0 and every following step: the whole tree snapshot, the action, the
value.  reference_order = 0 is held to the fp64-accumulating oracle within
rel 1e-5 after ONE expansion (test_planner_shapes_cpu.py checks the
condition that makes this a fair comparison).

FIB alphas come from the device (the FIB kernels are pinned by
test_gpu_parity.py) and are handed to the oracle; PBVI leaves use hand-made
alpha vectors on both sides."""
import ctypes as C

import numpy as np
import pytest

import planner_shape_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_model(oracle):
    """(T, L, R) of a table shape, generated once per shape."""
    cache = {}

    def get(H, W):
        if (H, W) not in cache:
            cache[(H, W)] = oracle.model_pomdp(PC.grid_of(H, W), PC.goal_of(H, W))
        return cache[(H, W)]
    return get


@pytest.fixture
def fc_walk():
    """pp2_debug_fc_walk: set the chain sets' driver, restored afterwards
    (the PP2_FC_* switches are cached per process: the environment cannot
    toggle them mid-run)."""
    from path_planning_2d_amd import _lib
    f = _lib.load().pp2_debug_fc_walk
    f.argtypes = [C.c_int]
    f.restype = C.c_int
    prev = []

    def choose(on):
        prev.append(f(int(on)))
    yield choose
    if prev:
        f(prev[0])


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
            assert ctx.model_dict_info()[1] == bool(sw["coded"])
        else:
            assert ctx.model_dict_info()[1]
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
            pal, pact = PC.pbvi_of(H, W)
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


@pytest.mark.parametrize("case", PC.REF_CASES, ids=PC.ref_case_id)
def test_reference_order_bit_exact(oracle, host_model, monkeypatch, fc_walk, case):
    import path_planning_2d_amd as P
    run_reference_order(P, oracle, host_model, case, monkeypatch, fc_walk)


@pytest.mark.parametrize("case", PC.DEFAULT_CASES, ids=PC.default_case_id)
def test_default_order_one_expansion(oracle, host_model, case):
    """reference_order = 0 (launch_expand, launch_belief_dots, the tile
    partials) against the fp64-accumulating oracle: step 0 with
    max_online_iteration = 1."""
    import path_planning_2d_amd as P
    H, W, kind, lb = case
    where = PC.default_case_id(case)
    grid = PC.grid_of(H, W)
    b0 = PC.belief_of(H, W, kind)
    ctx, T, L, R = context(P, H, W, {}, host_model)
    with ctx:
        alphas = ctx.fib_get()
        opl = oracle.Planner(grid, T, L, R, alphas, max_depth=PC.MAX_DEPTH, max_iter=1,
                             accurate=True)
        if lb:
            pal, pact = PC.pbvi_of(H, W)
            ctx.pbvi_set(pal, pact)
            opl.set_pbvi(pal, pact)
        with P.QVTreePlanner(ctx, max_search_tree_depth=PC.MAX_DEPTH, max_online_iteration=1,
                             lower_bound_mode=lb, rand_skip=0, reference_order=0) as gpl:
            a_g, v_g = gpl.step(0, 0, b0)
            a_o, v_o = opl.step(0, 0, b0)
            gi = gpl.info()
            assert gi["expansions"] == 1 and gi["n_root_children"] == 9
            PC.compare(gi, opl.info(), where, rel=1e-5)
            assert a_g == a_o, f"{where}: action {a_g} != {a_o}"
            assert PC.rel_close(v_g, v_o, rel=1e-5), f"{where}: value {v_g} != {v_o}"
        opl.close()
