"""GPU: live map and goal updates (pp2_map_update, pp2_goal_set; DESIGN.md
§2.2).  Every equivalence case compares a context ``u``, updated in place, with
a context ``f`` created fresh from the final map and goal and then generated,
once per PP2_TUNE_MAP_INCREMENTAL value on ``u`` (1: the patch path, 0: the
full regenerate-and-rebuild path).

Shapes: 8 x 256 and 6 x 510 with TUNE_RESIDENT_CUS 2 -- the suite's two
smallest two-tile resident shapes (test_gpu_resident_gates.py; 510 is no
multiple of 4, so pad columns exist) -- and 5 x 7, where every cell is a border
cell and every rectangle clips.  Grids are synthetic.synth_grid's.

After each case, as bit patterns: T, L, R, C of model_download(); the coded
model active alike; the masked admission alike; map_get() round-trips.  Then,
from the same belief_set + mdp_reset on both, 7 loop steps in launches of 2 and
5, mdp_sweep(8) and mdp_control for both policies give the same raw belief,
mass, J, A and control records -- on the default (resident) path and again with
TUNE_RESIDENT 0 / TUNE_STEP_PAIRS 0.  resident_launches() advances on ``u`` as
on ``f`` and resident_status()[0] == 0 (a replayed launch would hide a stale
table).  With the knob at 1 every changing call counts as incremental and none
as a rebuild; at 0 the other way round; a patch equal to the map counts
nowhere.  Episodes (the most direct reader of the code plane and the rows) run
on ``u`` as on ``f``.

Refusals: shards, uploaded models, bad rectangles, a planner made before an
update.  pp2_mdp_resolve: J and A equal sweeps / 100 calls of mdp_sweep(100)
from the same state on a twin, and final_norm is the last block's change and
meets pp2_mdp_solve's stop rule; the cold and warm sweep counts and
max |J_warm - J_cold| are printed, not asserted (a corridor closed far from the
goal may need as many sweeps warm as cold).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import covering_trajectory as ct
import planner_shape_cases as PC
from conftest import GAMMA

pytestmark = pytest.mark.gpu

# (H, W, TUNE_RESIDENT_CUS or None, resident expected)
SHAPES = [(8, 256, 2), (6, 510, 2), (5, 7, None)]
IDS = [f"{s[0]}x{s[1]}" for s in SHAPES]
STEPS = 7
LAUNCHES = ((0, 2), (2, 7))
ESTATE, EINVAL = 5, 1


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _grid(H, W):
    """test_gpu_resident_gates.py's grid: the first seed whose model is coded."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    for seed in range(H * 7 + W, H * 7 + W + 8):
        grid = S.synth_grid(H, W, seed)
        if (grid == 0).sum() < 4:
            continue
        goal = S.synth_goal(grid)
        with P.GridContext(grid, goal, gamma=float(GAMMA)) as c:
            c.model_generate()
            if c.model_dict_info()[1]:
                grid.setflags(write=False)
                return grid, goal
    pytest.fail(f"no coded model for {H} x {W}")


# ---------------------------------------------------------------- cases
# A case: (initial grid, initial goal, ops, prepare) -- ops are ("map", x0, y0,
# patch) or ("goal", (gx, gy)); prepare: put a solve and 5 loop steps into u
# before the ops.  changing: how many ops change the model.
def _flip(grid, x0, y0, w, h):
    return (1 - grid[y0:y0 + h, x0:x0 + w]).astype(np.uint8)


def _keep_free(patch, x0, y0, cell):
    """The patch with `cell` (x, y) left free where it covers it."""
    x, y = cell
    if x0 <= x < x0 + patch.shape[1] and y0 <= y < y0 + patch.shape[0]:
        patch[y - y0, x - x0] = 0
    return patch


def _cases(H, W):
    from path_planning_2d_amd import synthetic as S
    grid, goal = _grid(H, W)
    other = S.synth_grid(H, W, 1000 + H + W)
    other[goal[1], goal[0]] = 0
    free = np.argwhere(grid == 0)
    occ = np.argwhere(grid == 1)
    rw, rh = min(5, W), min(3, H)
    far = tuple(int(v) for v in free[0][::-1])      # a free cell (x, y) near row 0
    if far == tuple(goal):
        far = tuple(int(v) for v in free[1][::-1])
    on_occ = tuple(int(v) for v in occ[len(occ) // 2][::-1])
    cx, cy = W // 2, H // 2
    if (cx, cy) == tuple(goal):
        cx -= 1
    empty = np.zeros((H, W), np.uint8)
    out = {
        "flip_interior": (grid, goal, [("map", cx, cy, _flip(grid, cx, cy, 1, 1))], False, 1),
        "rect_x0_row0": (grid, goal,
                         [("map", 0, 0, _keep_free(_flip(grid, 0, 0, rw, rh), 0, 0, goal))],
                         False, 1),
        "rect_xmax_rowmax": (grid, goal,
                             [("map", W - rw, H - rh,
                               _keep_free(_flip(grid, W - rw, H - rh, rw, rh), W - rw, H - rh, goal))],
                             False, 1),
        "whole_grid": (grid, goal, [("map", 0, 0, other)], False, 1),
        "patch_equals_map": (grid, goal, [("map", 0, 0, grid[:rh, :rw].copy()),
                                          ("map", W - rw, H - rh, grid[H - rh:, W - rw:].copy())],
                             False, 0),
        "lone_obstacle": (empty, goal, [("map", cx, cy, np.ones((1, 1), np.uint8))], False, 1),
        "three_updates_goal_between": (grid, goal, [
            ("map", cx, cy, _flip(grid, cx, cy, 1, 1)),
            ("goal", far),
            ("map", 0, 0, _keep_free(_flip(grid, 0, 0, rw, rh), 0, 0, far)),
            ("map", W - rw, H - rh,
             _keep_free(_flip(grid, W - rw, H - rh, rw, rh), W - rw, H - rh, far))], False, 4),
        "goal_onto_occupied": (grid, goal, [("goal", on_occ)], False, 1),
        "goal_off_grid": (grid, goal, [("goal", (-3, H + 5))], False, 1),
        "goal_move_with_state": (grid, goal, [("goal", far)], True, 1),
    }
    return out


CASE_NAMES = ["flip_interior", "rect_x0_row0", "rect_xmax_rowmax", "whole_grid",
              "patch_equals_map", "lone_obstacle", "three_updates_goal_between",
              "goal_onto_occupied", "goal_off_grid", "goal_move_with_state"]


def _final(grid, goal, ops):
    g = np.array(grid, np.uint8)
    for op in ops:
        if op[0] == "map":
            _, x0, y0, p = op
            g[y0:y0 + p.shape[0], x0:x0 + p.shape[1]] = p
        else:
            goal = op[1]
    return g, tuple(goal)


def _apply(c, ops):
    for op in ops:
        if op[0] == "map":
            c.map_update(op[3], op[1], op[2])
        else:
            c.goal_set(op[1])


def _traj():
    us, zs = ct.segments(1)[0]
    return us[:STEPS].copy(), zs[:STEPS].copy()


def _belief(grid):
    from path_planning_2d_amd import synthetic as S
    return S.uniform_belief(grid)


def _same_state(u, f, what):
    for c in (u, f):
        c.synchronize()
    ru, mu = u.belief_get_raw()
    rf, mf = f.belief_get_raw()
    np.testing.assert_array_equal(_bits(ru), _bits(rf), err_msg=f"raw belief, {what}")
    assert _bits(np.float32(mu)) == _bits(np.float32(mf)), (what, mu, mf)
    Ju, Au = u.mdp_get()
    Jf, Af = f.mdp_get()
    np.testing.assert_array_equal(_bits(Ju), _bits(Jf), err_msg=f"J, {what}")
    np.testing.assert_array_equal(Au, Af, err_msg=f"A, {what}")
    for c in (u, f):
        assert c.resident_status()[0] == 0, f"a resident launch timed out and was replayed: {what}"


def _same_model(u, f, fgrid, fgoal, what):
    for a, b, name in zip(u.model_download(), f.model_download(), "TLRC"):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{name}, {what}")
    assert u.model_dict_info()[1] == f.model_dict_info()[1], what
    assert u.model_dict_info()[0] >= 1 and f.model_dict_info()[0] >= 1, what
    assert u.resident_masked()[0] == f.resident_masked()[0], what
    m, g = u.map_get()
    np.testing.assert_array_equal(m, fgrid, err_msg=f"map_get, {what}")
    assert g == tuple(fgoal) == tuple(u.goal), what


def _same_loop(u, f, fgrid, resident, what):
    us, zs = _traj()
    b0 = _belief(fgrid)
    before = (u.resident_launches(), f.resident_launches())
    for c in (u, f):
        c.belief_set(b0)
        c.mdp_reset()
    for lo, hi in LAUNCHES:
        for c in (u, f):
            c.loop_run(us[lo:hi], zs[lo:hi])
        _same_state(u, f, f"{what}, loop steps [{lo}, {hi})")
    for c in (u, f):
        c.mdp_sweep(8)
    _same_state(u, f, f"{what}, mdp_sweep(8)")
    for policy in ("mode", "qmdp"):
        au, vu, cu = u.mdp_control(policy)
        af, vf, cf = f.mdp_control(policy)
        assert (au, cu) == (af, cf) and _bits(vu) == _bits(vf), (what, policy, (au, vu, cu),
                                                                 (af, vf, cf))
    du = np.subtract(u.resident_launches(), before[0])
    df = np.subtract(f.resident_launches(), before[1])
    assert tuple(du) == tuple(df), f"resident launches u {du} f {df}: {what}"
    if resident:
        assert du[0] > 0 and du[1] > 0, f"not on the resident kernels: {what}"
    elif resident is not None:
        assert tuple(du) == (0, 0), what


def _pair(pp2, H, W, cus, case, knob):
    grid, goal, ops, prepare, changing = case
    u = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    try:
        u.model_generate()
        u.set_tuning(u.TUNE_MAP_INCREMENTAL, knob)
        if cus:
            u.set_tuning(u.TUNE_RESIDENT_CUS, cus)
        if prepare:
            us, zs = _traj()
            u.belief_set(_belief(grid))
            u.mdp_solve(200)
            u.loop_run(us[:5], zs[:5])
        _apply(u, ops)
        fgrid, fgoal = _final(grid, goal, ops)
        f = pp2.GridContext(fgrid, fgoal, gamma=float(GAMMA))
    except BaseException:
        u.close()
        raise
    try:
        f.model_generate()
        if cus:
            f.set_tuning(f.TUNE_RESIDENT_CUS, cus)
    except BaseException:
        u.close()
        f.close()
        raise
    return u, f, fgrid, fgoal


@pytest.mark.parametrize("knob", [1, 0], ids=["incremental", "full"])
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_update_equals_fresh_context(pp2, shape, name, knob):
    H, W, cus = shape
    case = _cases(H, W)[name]
    changing = case[4]
    what = f"{H}x{W} {name} knob {knob}"
    u, f, fgrid, fgoal = _pair(pp2, H, W, cus, case, knob)
    with u, f:
        updates, incremental, rebuilds, added = u.map_update_info()
        print(f"{what}: updates {updates} incremental {incremental} rebuilds {rebuilds} "
              f"entries added by the last {added}; entries u {u.model_dict_info()[0]} "
              f"f {f.model_dict_info()[0]}")
        assert updates == changing, what
        assert (incremental, rebuilds) == ((changing, 0) if knob else (0, changing)), what
        if name == "lone_obstacle" and knob:
            # an all-free map has 10 tuples; one lone obstacle adds its 8
            # neighbours' and its own
            assert added > 0 and incremental == 1, what
        if not knob or changing == 0:
            assert added == 0, what
        _same_model(u, f, fgrid, fgoal, what)
        if (fgrid == 0).sum() == 0:
            pytest.fail("case leaves no free cell")
        # (resident: asserted on the two resident shapes; 5 x 7 only u == f)
        _same_loop(u, f, fgrid, True if cus else None, what + ", default path")
        for c in (u, f):
            c.set_tuning(c.TUNE_RESIDENT, 0)
            c.set_tuning(c.TUNE_STEP_PAIRS, 0)
        _same_loop(u, f, fgrid, False, what + ", per-step path")
        _same_model(u, f, fgrid, fgoal, what + ", after the runs")
        assert u.map_update_info() == (updates, incremental, rebuilds, added)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_dense_context_keeps_its_dictionary(pp2, shape):
    """TUNE_CODED_MODEL 0 on u during the updates: the dense kernels read the
    patched planes, and the dictionary behind them is kept in step, so that
    switching the coded model back on finds no stale code."""
    H, W, cus = shape
    grid, goal, ops, _, changing = _cases(H, W)["three_updates_goal_between"]
    fgrid, fgoal = _final(grid, goal, ops)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as u, \
            pp2.GridContext(fgrid, fgoal, gamma=float(GAMMA)) as f:
        for c in (u, f):
            c.model_generate()
            c.set_tuning(c.TUNE_CODED_MODEL, 0)
            if cus:
                c.set_tuning(c.TUNE_RESIDENT_CUS, cus)
        _apply(u, ops)
        assert u.map_update_info()[:3] == (changing, changing, 0)
        assert not u.model_dict_info()[1] and not f.model_dict_info()[1]
        _same_model(u, f, fgrid, fgoal, "dense")
        _same_loop(u, f, fgrid, False, f"{H}x{W} dense")
        for c in (u, f):
            c.set_tuning(c.TUNE_CODED_MODEL, 1)
        _same_model(u, f, fgrid, fgoal, "coded again")
        _same_loop(u, f, fgrid, True if cus else None, f"{H}x{W} coded again")


@pytest.mark.parametrize("knob", [1, 0], ids=["incremental", "full"])
def test_update_before_a_model_only_rewrites_the_map(pp2, knob):
    H, W = 5, 7
    grid, goal = _grid(H, W)
    case = _cases(H, W)["three_updates_goal_between"]
    fgrid, fgoal = _final(grid, goal, case[2])
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as u, \
            pp2.GridContext(fgrid, fgoal, gamma=float(GAMMA)) as f:
        u.set_tuning(u.TUNE_MAP_INCREMENTAL, knob)
        _apply(u, case[2])
        assert u.map_update_info() == (0, 0, 0, 0)
        u.model_generate()
        f.model_generate()
        _same_model(u, f, fgrid, fgoal, "updates before model_generate")


@pytest.mark.parametrize("knob", [1, 0], ids=["incremental", "full"])
def test_episodes_after_updates(pp2, knob):
    """QMDP and FIB-greedy episodes on u give f's results, traces and beliefs."""
    H, W, cus = SHAPES[0]
    case = _cases(H, W)["three_updates_goal_between"]
    u, f, fgrid, fgoal = _pair(pp2, H, W, cus, case, knob)
    E, horizon = 8, 12
    free = np.flatnonzero(fgrid.reshape(-1) == 0)
    start = free[np.linspace(0, free.size - 1, E).astype(np.int64)].astype(np.int32)
    b0 = _belief(fgrid)
    with u, f:
        for c in (u, f):
            c.mdp_solve(200)
            c.fib_reset()
            c.fib_sweep(10)
        with pp2.EpisodeBatch(u, E, horizon, record_trace=True, placement="auto") as eu, \
                pp2.EpisodeBatch(f, E, horizon, record_trace=True, placement="auto") as ef:
            for policy in ("qmdp", "fib"):
                ru = eu.run(policy, b0, start, seed=11).results()
                rf = ef.run(policy, b0, start, seed=11).results()
                for k in rf:
                    np.testing.assert_array_equal(ru[k].view(np.uint8), rf[k].view(np.uint8),
                                                  err_msg=f"{policy} results {k}")
                tu, tf = eu.trace(), ef.trace()
                for k in tf:
                    np.testing.assert_array_equal(tu[k].view(np.uint8), tf[k].view(np.uint8),
                                                  err_msg=f"{policy} trace {k}")
                for e in range(E):
                    np.testing.assert_array_equal(_bits(eu.belief(e)), _bits(ef.belief(e)),
                                                  err_msg=f"{policy} final belief {e}")
        assert u.resident_status()[0] == 0 and f.resident_status()[0] == 0


# ---------------------------------------------------------------- refusals
def _status(pp2, fn, *args):
    with pytest.raises(pp2.Pp2Error) as e:
        fn(*args)
    return e.value.status


def test_shard_context_refuses(pp2):
    H, W = 8, 256
    grid, goal = _grid(H, W)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, H // 2)) as s:
        s.model_generate()
        assert _status(pp2, s.map_update, np.ones((1, 1), np.uint8), 3, 1) == ESTATE
        assert _status(pp2, s.goal_set, (1, 1)) == ESTATE
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, H)) as s:
        assert _status(pp2, s.map_update, np.ones((1, 1), np.uint8), 3, 1) == ESTATE


def test_uploaded_model_refuses(pp2):
    H, W = 5, 7
    grid, goal = _grid(H, W)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as c:
        c.model_generate()
        T, L, R, Cc = c.model_download()
        c.model_upload(T, L, R, Cc)
        flip = _flip(grid, 3, 2, 1, 1)
        assert _status(pp2, c.map_update, flip, 3, 2) == ESTATE
        assert _status(pp2, c.goal_set, (0, 0)) == ESTATE
        assert c.map_update_info() == (0, 0, 0, 0)
        np.testing.assert_array_equal(c.map_get()[0], grid)
        c.model_generate()  # a generated model again: updates are back
        c.map_update(flip, 3, 2)
        assert c.map_update_info()[0] == 1


def test_bad_rectangles(pp2):
    from path_planning_2d_amd import _lib
    H, W = 5, 7
    grid, goal = _grid(H, W)
    one = np.zeros((H + 1, W + 1), np.uint8)
    p = one.ctypes.data_as(C.POINTER(C.c_uint8))
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as c:
        c.model_generate()
        lib = _lib.load()
        h = c.handle
        for x0, y0, w, h_ in ((0, 0, 0, 1), (0, 0, 1, 0), (W, 0, 1, 1), (0, H, 1, 1),
                              (W - 1, 0, 2, 1), (0, H - 1, 1, 2), (0, 0, W + 1, 1),
                              (2 ** 32 - 1, 0, 2, 1), (1, 1, 2 ** 32 - 1, 1)):
            assert lib.pp2_map_update(h, x0, y0, w, h_, p) == EINVAL, (x0, y0, w, h_)
        assert lib.pp2_map_update(h, 0, 0, 1, 1, None) == EINVAL
        assert c.map_update_info() == (0, 0, 0, 0)
        np.testing.assert_array_equal(c.map_get()[0], grid)
        assert c.map_get()[1] == tuple(goal)
        assert _status(pp2, c.set_tuning, c.TUNE_MAP_INCREMENTAL, 2) == EINVAL


@pytest.mark.parametrize("knob", [1, 0], ids=["incremental", "full"])
def test_planner_made_before_an_update_refuses(pp2, knob):
    H, W, _ = PC.SHAPES[0]
    grid, goal = PC.grid_of(H, W), PC.goal_of(H, W)
    occ = np.argwhere(grid == 1)
    if len(occ):
        y, x = (int(v) for v in occ[0])
    else:
        y, x = next((int(a), int(b)) for a, b in np.argwhere(grid == 0) if (b, a) != tuple(goal))
    patch = _flip(grid, x, y, 1, 1)
    fgrid, fgoal = _final(grid, goal, [("map", x, y, patch)])
    assert (fgrid == 0).sum() >= 3
    b0 = _belief(grid)
    kw = dict(max_search_tree_depth=PC.MAX_DEPTH, max_online_iteration=PC.MAX_ITER,
              lower_bound_mode=0, rand_skip=0, reference_order=1)
    zs = PC.zs_of(H, W, 2)
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as u, \
            pp2.GridContext(fgrid, fgoal, gamma=float(GAMMA)) as f:
        u.model_generate()
        u.set_tuning(u.TUNE_MAP_INCREMENTAL, knob)
        u.fib_solve(max_sweeps=40)
        with pp2.QVTreePlanner(u, **kw) as old:
            old.step(0, 0, b0)
            u.map_update(grid[y:y + 1, x:x + 1].copy(), x, y)  # equal to the map: no change
            old.step(0, zs[0])
            u.map_update(patch, x, y)
            assert _status(pp2, old.step, 0, zs[1]) == ESTATE
            old.reset()
            assert _status(pp2, old.step, 0, 0, b0) == ESTATE
        f.model_generate()
        for c in (u, f):
            c.fib_reset()
            c.fib_solve(max_sweeps=40)
        bf = _belief(fgrid)
        with pp2.QVTreePlanner(u, **kw) as pu, pp2.QVTreePlanner(f, **kw) as pf:
            a = 0
            for k in range(3):
                msg = (0, 0, bf) if k == 0 else (a, zs[k - 1])
                au, vu = pu.step(*msg)
                af, vf = pf.step(*msg)
                assert au == af and _bits(np.float32(vu)) == _bits(np.float32(vf)), (k, au, vu, af, vf)
                a = af


# ---------------------------------------------------------------- mdp_resolve
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
def test_mdp_resolve_equals_blocks_of_sweeps(pp2, shape):
    H, W, cus = shape
    grid, goal = _grid(H, W)
    case = _cases(H, W)["rect_x0_row0"]
    ops = case[2]
    fgrid, fgoal = _final(grid, goal, ops)
    thresh = 5.0 / (1.0 - float(np.float32(GAMMA))) * 1e-3
    ctxs = [pp2.GridContext(grid, goal, gamma=float(GAMMA)) for _ in range(2)]
    u, t = ctxs
    f = pp2.GridContext(fgrid, fgoal, gamma=float(GAMMA))
    with u, t, f:
        cold0 = None
        for c in (u, t):
            c.model_generate()
            if cus:
                c.set_tuning(c.TUNE_RESIDENT_CUS, cus)
            cold0 = c.mdp_solve()
            _apply(c, ops)
        J0, _ = t.mdp_get()
        before = u.resident_launches()
        sweeps, norm = u.mdp_resolve()
        assert sweeps > 0 and sweeps % 100 == 0, (sweeps, norm)
        if cus:
            assert u.resident_launches()[1] > before[1], "the warm solve left the resident path"
        Jp = J0
        for k in range(sweeps // 100):
            Jp = t.mdp_get()[0]
            t.mdp_sweep(100)
        Ju, Au = u.mdp_get()
        Jt, At = t.mdp_get()
        np.testing.assert_array_equal(_bits(Ju), _bits(Jt), err_msg="J, resolve vs sweeps")
        np.testing.assert_array_equal(Au, At, err_msg="A, resolve vs sweeps")
        last = float(np.abs(Jt - Jp).max())
        assert norm == last, (norm, last)
        assert norm <= thresh, (norm, thresh)
        f.model_generate()
        if cus:
            f.set_tuning(f.TUNE_RESIDENT_CUS, cus)
        cold = f.mdp_solve()
        Jf, _ = f.mdp_get()
        print(f"{H}x{W}: cold solve before the update {cold0}, warm re-solve ({sweeps}, {norm}), "
              f"cold solve of the new map {cold}; max |J_warm - J_cold| = "
              f"{float(np.abs(Ju - Jf).max()):.6g} (threshold {thresh:.6g})")
        assert u.resident_status()[0] == 0 and t.resident_status()[0] == 0
        # a capped warm solve stops at the cap like pp2_mdp_solve
        s2, _ = u.mdp_resolve(100)
        assert s2 == 100
