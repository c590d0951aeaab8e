"""GPU: on-device control selection (pp2_belief_mode, pp2_mdp_qvalues,
pp2_mdp_control; kernels in csrc/pp2_control.hip).

* The belief's mode is held bit for bit to the first maximum of
  pp2_belief_get (ties, zeros, padding, unnormalised stored beliefs).
* QMDP on a one-hot belief is the Bellman backup of that cell, so it is held
  bit for bit to the library's own next sweep (values and first-minimum
  actions), itself held to the oracle's sweep; with the coded model off, the
  dense k_control_q at both settings of PP2_TUNE_NT_STREAMS as well.
* On spread beliefs q is held to the fp64 reference
  (synthetic.control_reference) within the project's parity budget, rel 1e-5:
  every term b * Q is >= 0, so there is no cancellation, and an fp32 sum of n
  such terms in a tree of depth ~log2(n) + n / 1024 / 16 is far inside it.
  The action must be a minimiser of the reference up to rel 1e-4, which forces
  the exact action wherever the reference's two best differ by more.
"""
import numpy as np
import pytest

from conftest import GAMMA, assert_rel_close, golden, golden_map

pytestmark = pytest.mark.gpu

GOLDEN_MAPS = ["map_10x10", "sparse_map_100x40", "tile64_sparse_map_100x40"]
LOOP_MAPS = ["sparse_map_100x40", "tile64_sparse_map_100x40"]
SYNTH = {"synth_97x131": (97, 131, 3), "synth_1x7": (1, 7, 1), "synth_5x1": (5, 1, 2),
         "synth_256x256": (256, 256, 256)}
# more 4096-cell tiles (260) than the device has CUs: the coded Q kernel's
# workgroups take a second tile
BIG = {"synth_1040x1024": (1040, 1024, 9)}
BELIEFS = ["b0", "b1", "b2", "b4", "b8", "b16", "b32", "b64"]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def make_ctx(pp2, grid, goal, cpt=4):
    ctx = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    ctx.set_cells_per_lane(cpt)
    ctx.model_generate()
    return ctx


# which Q kernel a case runs: the coded one (the default), or with the coded
# model off the dense k_control_q<true> / k_control_q<false>
# (PP2_TUNE_NT_STREAMS 1 / 0; the sweeps then run k_mdp_sweep<4, nt>)
Q_KERNELS = ["coded", "dense_nt1", "dense_nt0"]


def choose_q_kernel(ctx, kernel):
    if kernel == "coded":
        assert ctx.model_dict_info()[1]
        return
    ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
    ctx.set_tuning(ctx.TUNE_NT_STREAMS, int(kernel[-1]))
    assert not ctx.model_dict_info()[1]


def load_grid(name):
    """(grid, goal) of a golden map or a synthetic grid."""
    from path_planning_2d_amd import synthetic as S
    if name in SYNTH or name in BIG:
        H, W, seed = (SYNTH.get(name) or BIG[name])
        grid = S.synth_grid(H, W, seed)
        grid[0, 0] = 0
        return grid, (0, 0)
    return golden_map(name), tuple(golden("model", name)["goal"])


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def first_mode(b):
    """The reference scan: first strict maximum > 0 of a float32 array."""
    best, cell = np.float32(0.0), 0
    for i, v in enumerate(np.asarray(b, np.float32)):
        if v > best:
            best, cell = v, i
    return cell, best


def check_mode(ctx, J, A, what):
    bg = ctx.belief_get()
    want_cell, want_prob = first_mode(bg)
    cell, prob = ctx.belief_mode()
    assert cell == want_cell, (what, cell, want_cell)
    assert bits(prob)[0] == bits(want_prob)[0], (what, prob, want_prob)
    a, v, c2 = ctx.mdp_control("mode")
    assert c2 == want_cell, what
    assert a == A[want_cell], (what, a, A[want_cell])
    assert bits(v)[0] == bits(J[want_cell])[0], (what, v, J[want_cell])
    return want_cell, want_prob


# ---------------------------------------------------------------- 1. mode
@pytest.mark.parametrize("name", ["map_3x3"] + GOLDEN_MAPS + list(SYNTH))
def test_mode_bit_exact(pp2, name):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    H, W = grid.shape
    n = H * W
    beliefs = {}
    if name in GOLDEN_MAPS:
        bt = golden("belief", name)
        beliefs.update({k: bt[k] for k in ("b0", "b1", "b8")})
        # the fixtures' ties at the maximum: thousands (uniform), then a few
        ties = [int((bt[k] == bt[k].max()).sum()) for k in ("b0", "b1")]
        assert ties[0] > 1 and ties[1] > 1, ties
    else:
        beliefs["uniform"] = S.uniform_belief(grid)
    beliefs["zero"] = np.zeros(n, np.float32)
    spike = np.zeros(n, np.float32)
    spike[n - 1] = 0.75
    beliefs["last_cell"] = spike
    two = np.zeros(n, np.float32)
    two[[n // 3, n - 1]] = 0.5
    beliefs["two_equal"] = two
    with make_ctx(pp2, grid, goal) as ctx:
        ctx.mdp_reset()
        ctx.mdp_sweep(7)
        J, A = ctx.mdp_get()
        for what, b in beliefs.items():
            ctx.belief_set(b)
            cell, prob = check_mode(ctx, J, A, (name, what))
            if what == "zero":
                assert cell == 0 and prob == 0
            if what == "last_cell":
                assert cell == n - 1
            if what == "two_equal":
                assert cell == n // 3
            if what in ("b0", "uniform"):
                assert cell == int(np.nonzero(grid.reshape(-1) == 0)[0][0])
        if name in LOOP_MAPS:
            # an unnormalised stored belief: the comparison is on stored / mass
            bt = golden("belief", name)
            ctx.belief_set(bt["b0"])
            for k in range(8):
                ctx.belief_update(int(bt["us"][k]), int(bt["zs"][k]))
            raw, mass = ctx.belief_get_raw()
            assert mass != 1.0
            check_mode(ctx, J, A, (name, "updated"))


# ------------------------------------------------------- 2. QMDP, one-hot
def onehot_cells(grid, rng):
    H, W = grid.shape
    occ = grid.reshape(-1)
    cells = [0, W - 1, (H - 1) * W, H * W - 1,             # corners
             W // 2, (H // 2) * W, (H // 2) * W + W - 1,  # top, left, right edges
             (H - 1) * W + W // 2,                          # bottom edge
             (H // 3) * W + W - 1]                          # last valid cell of a row
    cells.append(int(np.nonzero(occ == 1)[0][len(np.nonzero(occ == 1)[0]) // 2]))  # occupied
    # free cells beside an obstacle (4-neighbourhood)
    pad = np.pad(grid, 1, constant_values=0)
    near = (grid == 0) & ((pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]) == 1)
    beside = np.nonzero(near.reshape(-1))[0]
    cells += [int(c) for c in beside[:: max(1, beside.size // 8)][:8]]
    cells += [int(c) for c in rng.integers(0, H * W, 40 - len(cells))]
    return cells


@pytest.mark.parametrize("kernel", Q_KERNELS)
@pytest.mark.parametrize("name", LOOP_MAPS + ["synth_97x131"])
def test_qmdp_one_hot_is_the_next_sweep(pp2, oracle, name, kernel):
    grid, goal = load_grid(name)
    H, W = grid.shape
    n = H * W
    cells = onehot_cells(grid, np.random.default_rng(7))
    cells.append(goal[1] * W + goal[0])
    with make_ctx(pp2, grid, goal) as ctx:
        choose_q_kernel(ctx, kernel)
        ctx.mdp_reset()
        ctx.mdp_sweep(7)
        got = []
        for c in cells:
            b = np.zeros(n, np.float32)
            b[c] = 1.0
            ctx.belief_set(b)
            a, v, cell = ctx.mdp_control("qmdp")
            assert cell == -1
            q = ctx.mdp_qvalues()
            assert bits(q[a])[0] == bits(v)[0]
            got.append((a, v))
        ctx.mdp_sweep(1)
        J, A = ctx.mdp_get()
    for c, (a, v) in zip(cells, got):
        assert a == A[c], (name, c, a, A[c])
        assert bits(v)[0] == bits(J[c])[0], (name, c, v, J[c])
    # and that sweep is the oracle's eighth
    T, Cc = oracle.model_mdp(grid, goal)
    Jo = np.zeros(n, np.float32)
    for _ in range(8):
        Jo, Ao = oracle.mdp_sweep(H, W, GAMMA, T, Cc, Jo)
    np.testing.assert_array_equal(bits(J), bits(Jo))
    np.testing.assert_array_equal(A, Ao)


# ------------------------------------------------ 3. QMDP, spread beliefs
def check_q(ctx, q64, what):
    """q within rel 1e-5 of the reference, the action one of its minimisers
    up to rel 1e-4; returns whether the reference's gap exceeds 1e-4."""
    q = ctx.mdp_qvalues()
    a, v, _ = ctx.mdp_control("qmdp")
    assert_rel_close(q, q64, rel=1e-5, msg=str(what))
    assert bits(v)[0] == bits(q[a])[0], what
    assert a == int(np.argmin(q)), what  # first minimum of its own q
    assert q64[a] <= q64.min() * (1 + 1e-4), (what, a, q64)
    srt = np.sort(q64)
    clear = bool(srt[1] - srt[0] > 1e-4 * srt[0])
    if clear:
        assert a == int(np.argmin(q64)), what
    return clear


@pytest.mark.parametrize("kernel", Q_KERNELS)
@pytest.mark.parametrize("which", ["J7", "solved"])
def test_qmdp_spread_beliefs_against_fp64(pp2, which, kernel):
    from path_planning_2d_amd import synthetic as S
    clear = 0
    for name in GOLDEN_MAPS:
        grid, goal = load_grid(name)
        H, W = grid.shape
        m = golden("model", name)
        bt = golden("belief", name)
        with make_ctx(pp2, grid, goal) as ctx:
            choose_q_kernel(ctx, kernel)
            if which == "J7":
                ctx.mdp_reset()
                ctx.mdp_sweep(7)
            else:
                ctx.mdp_solve()
            J, _ = ctx.mdp_get()
            for k in BELIEFS:
                q64, _ = S.control_reference(m["T"], m["C"], J, bt[k], GAMMA, H, W)
                ctx.belief_set(bt[k])
                clear += check_q(ctx, q64, (name, which, k))
    print(f"{which}: {clear} of 24 cases have an fp64 top-2 gap above 1e-4")
    if which == "solved":
        assert clear >= 20, clear


# ---------------------------------------------------------- 4. invariance
@pytest.mark.parametrize("name", ["sparse_map_100x40", "synth_97x131", "synth_256x256",
                                  "synth_1040x1024"])
def test_q_bits_invariant(pp2, name):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    H, W = grid.shape
    if name in GOLDEN_MAPS:
        b = golden("belief", name)["b8"]
    else:  # a spread, uneven belief over the free cells
        rng = np.random.default_rng(11)
        b = (rng.random(H * W) * (grid.reshape(-1) == 0)).astype(np.float32)
        b /= b.sum(dtype=np.float64)
    with make_ctx(pp2, grid, goal) as ctx:
        ctx.mdp_reset()
        ctx.mdp_sweep(7)
        ctx.belief_set(b)
        entries, active = ctx.model_dict_info()
        assert entries > 0 and active  # else nothing here runs the coded kernel
        q_coded = ctx.mdp_qvalues()
        q_again = ctx.mdp_qvalues()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        assert not ctx.model_dict_info()[1]
        q_dense = ctx.mdp_qvalues()
        q_dense_again = ctx.mdp_qvalues()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 1)
        np.testing.assert_array_equal(bits(q_coded), bits(q_again))
        np.testing.assert_array_equal(bits(q_dense), bits(q_dense_again))
        np.testing.assert_array_equal(bits(q_coded), bits(q_dense))
        assert np.isfinite(q_coded).all() and (q_coded > 0).all()
        if name in BIG:
            return  # bits against the dense kernel (one block per 1024 cells) is the check here
        J, _ = ctx.mdp_get()
        T, _, _, C = ctx.model_download()
        q64, _ = S.control_reference(T, C, J, b, GAMMA, H, W)
        assert_rel_close(q_coded, q64, rel=1e-5, msg=name)
        for cpt in (1, 2):
            ctx.set_cells_per_lane(cpt)
            assert_rel_close(ctx.mdp_qvalues(), q64, rel=1e-5, msg=f"{name} cpt {cpt}")
            cell, prob = ctx.belief_mode()
            assert (cell, bits(prob)[0]) == (first_mode(b)[0], bits(ctx.belief_get()[cell])[0])


def test_q_full_dictionary_rows(pp2):
    """A T entry off its action's base-kernel support rules out the sparse LDS
    rows (tests/test_gpu_coded.py): the coded Q pass then reads full rows, and
    must still give the dense kernel's bits and the next sweep's backup."""
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(48, 60, 21)
    grid[0, 0] = 0
    H, W = grid.shape
    cell = 17 * W + 23
    rng = np.random.default_rng(5)
    b = (rng.random(H * W) * (grid.reshape(-1) == 0)).astype(np.float32)
    b /= b.sum(dtype=np.float64)
    with make_ctx(pp2, grid, (0, 0)) as ctx:
        T, L, R, C = ctx.model_download()
        T[cell, 4, 0] = np.float32(0.25)  # stay action: support is {4} only
        ctx.model_upload(T, L, R, C)
        ctx.mdp_reset()
        ctx.mdp_sweep(7)
        J, _ = ctx.mdp_get()
        ctx.belief_set(b)
        assert ctx.model_dict_info()[1]
        q_coded = ctx.mdp_qvalues()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        q_dense = ctx.mdp_qvalues()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, 1)
        np.testing.assert_array_equal(bits(q_coded), bits(q_dense))
        q64, _ = S.control_reference(T, C, J, b, GAMMA, H, W)
        assert_rel_close(q_coded, q64, rel=1e-5, msg="full rows")
        got = []
        cells = [cell, cell + 1, 0, H * W - 1, 5 * W + W - 1]
        for c in cells:
            e = np.zeros(H * W, np.float32)
            e[c] = 1.0
            ctx.belief_set(e)
            got.append(ctx.mdp_control("qmdp"))
        ctx.mdp_sweep(1)
        Jn, An = ctx.mdp_get()
    for c, (a, v, _) in zip(cells, got):
        assert a == An[c] and bits(v)[0] == bits(Jn[c])[0], (c, a, v, An[c], Jn[c])


# ------------------------------------------------------ 5. after the loop
@pytest.mark.parametrize("tuned", ["default", "per_step"])
@pytest.mark.parametrize("name", LOOP_MAPS)
def test_control_after_the_loop(pp2, name, tuned):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid(name)
    H, W = grid.shape
    bt = golden("belief", name)
    with make_ctx(pp2, grid, goal) as ctx:
        if tuned == "per_step":
            ctx.set_tuning(ctx.TUNE_RESIDENT, 0)
            ctx.set_tuning(ctx.TUNE_STEP_PAIRS, 0)
        ctx.belief_set(bt["b0"])
        ctx.mdp_reset()
        ctx.loop_run(bt["us"][:32], bt["zs"][:32])
        # the controls first: they settle whatever the loop left pending
        cell, prob = ctx.belief_mode()
        mode = ctx.mdp_control("mode")
        q = ctx.mdp_qvalues()
        qmdp = ctx.mdp_control("qmdp")
        bg = ctx.belief_get()
        J, A = ctx.mdp_get()
        T, _, _, C = ctx.model_download()
    q64, want_cell = S.control_reference(T, C, J, bg, GAMMA, H, W)
    assert cell == want_cell == first_mode(bg)[0]
    assert bits(prob)[0] == bits(bg[cell])[0]
    assert mode[0] == A[cell] and bits(mode[1])[0] == bits(J[cell])[0] and mode[2] == cell
    assert_rel_close(q, q64, rel=1e-5, msg=f"{name} {tuned}")
    a, v, c = qmdp
    assert c == -1 and bits(v)[0] == bits(q[a])[0]
    assert q64[a] <= q64.min() * (1 + 1e-4), (a, q64)


# --------------------------------------------------------------- 6. errors
def test_errors(pp2):
    from path_planning_2d_amd import _lib
    ESTATE, EINVAL = 5, 1
    assert _lib.STATUS_NAMES[ESTATE] == "PP2_ESTATE" and _lib.STATUS_NAMES[EINVAL] == "PP2_EINVAL"
    grid, goal = load_grid("map_10x10")
    H, W = grid.shape
    with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as ctx:  # no model
        for fn in (ctx.mdp_control, ctx.mdp_qvalues):
            with pytest.raises(pp2.Pp2Error) as e:
                fn()
            assert e.value.status == ESTATE
        assert ctx.belief_mode() == (0, 0)  # the mode needs no model
        ctx.model_generate()
        with pytest.raises(pp2.Pp2Error) as e:
            ctx.mdp_control(7)
        assert e.value.status == EINVAL
        with pytest.raises(ValueError):
            ctx.mdp_control("greedy")
        assert ctx.mdp_control(pp2.CONTROL_MODE)[2] == 0
    with pp2.GridContext(grid, goal, gamma=float(GAMMA), rows=(0, H // 2)) as sh:
        sh.model_generate()
        for fn in (sh.mdp_control, sh.mdp_qvalues, sh.belief_mode):
            with pytest.raises(pp2.Pp2Error) as e:
                fn()
            assert e.value.status == ESTATE
    with pp2.ShardGroup(grid, goal, (0, 5, H), gamma=float(GAMMA)) as grp:
        grp.model_generate()
        with pytest.raises(pp2.Pp2Error) as e:
            grp.shards[0].mdp_control("qmdp")
        assert e.value.status == ESTATE


# ----------------------------------------------------------- 7. controller
@pytest.mark.parametrize("policy", ["mode", "qmdp"])
def test_controller_closed_loop(pp2, policy):
    from path_planning_2d_amd import synthetic as S
    grid, goal = load_grid("sparse_map_100x40")
    b0 = S.uniform_belief(grid)
    runs = []
    with make_ctx(pp2, grid, goal) as ctx:
        ctx.mdp_solve()
        for _ in range(2):
            ctl = pp2.BeliefMdpController(ctx, policy=policy)
            _, acts, vals = S.closed_loop(grid, b0, ctl.step, 24)
            runs.append((acts, vals))
        assert len(runs[0][0]) == 24 and (runs[0][0] <= 8).all()
        np.testing.assert_array_equal(runs[0][0], runs[1][0])
        np.testing.assert_array_equal(bits(runs[0][1]), bits(runs[1][1]))
        assert (ctl.last_cell >= 0) == (policy == "mode")
        # sweeps_per_step = 1: the fused loop step, then the same control call
        ctl = pp2.BeliefMdpController(ctx, policy=policy, sweeps_per_step=1)
        _, acts, vals = S.closed_loop(grid, b0, ctl.step, 6)
        assert len(acts) == 6 and (acts <= 8).all() and np.isfinite(vals).all()
