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

import pytest

import planner_shape_cases as PC
from planner_shape_run import context, host_models, run_reference_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_model(oracle):
    """(T, L, R) of a table shape, generated once per shape."""
    return host_models(oracle)


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
