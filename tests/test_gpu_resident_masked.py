"""GPU: the masked-support form of the resident loop's whole-row instance
(pp2_resident.hip, k_loop_resident<CAP, 1, false, false, ResidentMasked>;
admission: pp2_masked.h).  The tile's LDS
planes and the exchanged granules hold b and J with blocked cells stored as +0,
an off-centre weight is one of two constants of the kernel's head, the gather
reads the cells' centre T and L_z alone and the backup one 8-B record per
(action, cell); a blocked own cell is its centre term on the lane's own
unmasked value.

The bar is bit equality -- raw belief bits, the mass, J bits and A after every
launch -- between three contexts:
  * the masked form (the default on an admitted model; the query must say the
    launches ran it),
  * the class-table form of the same tiles (TUNE_RESIDENT_MASKED 0),
  * launch-per-step (TUNE_RESIDENT 0, TUNE_STEP_PAIRS 0).

Shapes, trajectory, launch lengths, norm blocks and the coverage condition are
those of test_gpu_resident_window.py: 16 x 1024 / 4 CUs, 8 x 256 / 2, 7 x 512 /
2, 6 x 510 / 2 and 4 x 1024 / 4; the 42-step covering segment in launches of 1,
2, 5, 25 and 9 steps; TUNE_NORM_BLOCK 8 and 1; at least 85 % of the reference's
free cells non-zero after every launch.

Edited maps (16 x 1024 and 8 x 256, a few cells of the seeded grid changed): a
free cell with all eight neighbours occupied; a free cell in a grid corner and
one on a grid edge with their in-grid neighbours occupied; occupied cells in a
tile's first and last row; at x = 255 / 256 (a wave seam) and at x = 0 / W - 1
(lanes 0 / 63); the goal next to an occupied cell; and a map with no occupied
cell.  For every edited map the launch-per-step loop is first run on the CPU
(the oracle's belief update, the blocked normalisation of the device) and must
keep 85 % of the free cells non-zero after every launch.

One case starts from a belief with mass on an occupied cell and on the
walled-in cell: it must stay there bit for bit.

Fallback: the generated model downloaded, changed and uploaded must not be
admitted, and the three contexts still agree -- one cell's off-centre weight
changed; a blocked cell whose cost differs for one action; one action's side
weight changed everywhere -- and the untouched model uploaded again is admitted
again.
"""
import numpy as np
import pytest

import covering_trajectory as ct
from conftest import GAMMA

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048
SHORT_STEPS = 24
RUNS = (1, 2, 5, SHORT_STEPS + 1)
MIN_NONZERO = 0.85

SHAPES = [
    (16, 1024, 4, (4, 4, 1)),
    (8, 256, 2, (2, 4, 1)),
    (7, 512, 2, (2, 4, 1)),
    (6, 510, 2, (2, 3, 1)),
    (4, 1024, 4, (4, 1, 1)),
]
IDS = [f"{s[0]}x{s[1]}" for s in SHAPES]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _seeded_grid(pp2, H, W):
    """test_gpu_resident_window.py's grid: the first seed whose model is coded."""
    from path_planning_2d_amd import synthetic as S
    for seed in range(H * 7 + W, H * 7 + W + 8):
        grid = S.synth_grid(H, W, seed)
        goal = S.synth_goal(grid)
        with pp2.GridContext(grid, goal, gamma=float(GAMMA)) as c:
            c.model_generate()
            if c.model_dict_info()[1]:
                return grid, goal
    pytest.fail(f"no coded model for {H} x {W}")


def _trio(pp2, grid, goal, cus, block, b0=None):
    """(masked, class-table, launch-per-step) contexts on one generated model."""
    from path_planning_2d_amd import synthetic as S
    cs = [pp2.GridContext(grid, goal, gamma=float(GAMMA)) for _ in range(3)]
    m, u, s = cs
    for c in cs:
        c.model_generate()
        assert c.model_dict_info()[1]
    for c in (m, u):
        c.set_tuning(c.TUNE_RESIDENT_CUS, cus)
    u.set_tuning(u.TUNE_RESIDENT_MASKED, 0)
    s.set_tuning(s.TUNE_RESIDENT, 0)
    s.set_tuning(s.TUNE_STEP_PAIRS, 0)
    _restart(cs, grid, block, b0)
    return cs


def _restart(cs, grid, block, b0=None):
    from path_planning_2d_amd import synthetic as S
    b0 = S.uniform_belief(grid) if b0 is None else b0
    for c in cs:
        c.set_tuning(c.TUNE_NORM_BLOCK, block)
        c.belief_set(b0)
        c.mdp_reset()


def _same(a, b, what):
    """Raw belief bits, mass bits, J bits and A; returns b's raw belief."""
    ra, ma = a.belief_get_raw()
    rb, mb = b.belief_get_raw()
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32),
                                  err_msg=f"raw belief {what}")
    assert np.float32(ma).view(np.uint32) == np.float32(mb).view(np.uint32), (what, ma, mb)
    Ja, Aa = a.mdp_get()
    Jb, Ab = b.mdp_get()
    np.testing.assert_array_equal(Ja.view(np.uint32), Jb.view(np.uint32), err_msg=f"J {what}")
    np.testing.assert_array_equal(Aa, Ab, err_msg=f"A {what}")
    return rb


def _launches(n):
    out, lo = [], 0
    for m in RUNS:
        out.append((lo, lo + m))
        lo += m
    assert n - lo >= 2, "the rest is a resident launch"
    out.append((lo, n))
    return out


def _run_and_compare(cs, grid, block, tag, masked=True, watch=()):
    """The 42-step segment in launches of 1, 2, 5, 25 and 9 steps on the three
    contexts, compared after every launch.  masked: whether the first
    context's resident launches must have run the masked form.  watch: cells
    whose raw belief is returned per launch."""
    m, u, s = cs
    free = grid.reshape(-1) == 0
    us, zs = ct.segments(block)[0]
    assert set(us[:17].tolist()) == set(range(ct.ACTIONS))
    launches = _launches(us.size)
    res0, msk0 = m.resident_launches()[0], m.resident_masked()[1]
    ures0 = u.resident_launches()[0]
    resident, low, seen = 0, 1.0, []
    for lo, hi in launches:
        for c in cs:
            c.loop_run(us[lo:hi], zs[lo:hi])
        m.synchronize()
        u.synchronize()
        resident += len(ct.resident_launches(lo, hi))
        what = f"{tag} block {block}, after steps [{lo}, {hi})"
        assert m.resident_launches()[0] == res0 + resident, what
        assert u.resident_launches()[0] == ures0 + resident, what
        assert s.resident_launches() == (0, 0), what
        assert m.resident_masked()[1] == msk0 + (resident if masked else 0), what
        assert u.resident_masked()[1] == 0, what
        assert m.resident_status()[0] == 0 and u.resident_status()[0] == 0, f"fell back: {what}"
        raw = _same(m, s, f"masked vs per-step, {what}")
        _same(u, s, f"class tables vs per-step, {what}")
        assert np.isfinite(raw).all(), what
        share = np.count_nonzero(raw[free]) / int(free.sum())
        low = min(low, share)
        print(f"{what}: {share:.3f} of the free cells non-zero")
        assert share >= MIN_NONZERO, f"{share:.3f} of the free cells non-zero {what}"
        seen.append(raw[list(watch)].copy())
    assert resident == len(launches) - 1
    print(f"{tag} block {block}: {resident} resident launches, non-zero share >= {low:.3f}")
    return seen


@pytest.mark.parametrize("block", [8, 1])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_masked_equals_class_tables_and_single_steps(pp2, H, W, cus, tiling, block):
    grid, goal = _seeded_grid(pp2, H, W)
    cs = _trio(pp2, grid, goal, cus, block)
    m, u, s = cs
    with m, u, s:
        assert m.resident_tiling() == tiling and u.resident_tiling() == tiling
        assert m.loop_steps_per_launch() == RESIDENT_STEPS == u.loop_steps_per_launch()
        assert s.loop_steps_per_launch() == 1
        assert m.resident_masked() == (True, 0), "a generated model is admitted"
        assert u.resident_masked() == (True, 0) and s.resident_masked() == (True, 0)
        _run_and_compare(cs, grid, block, f"{H} x {W}")


# ---------------------------------------------------------------- edited maps
def _edit(grid, goal):
    """The seeded grid with the cells of the module docstring changed (rt = 4
    rows per tile on both grids: rows 3 | 4 are a tile's last | first row).
    Returns (grid, goal, walled-in cell, an occupied cell)."""
    g = grid.copy()
    H, W = g.shape
    gx, gy = goal
    wy, wx = 2, W // 2 + 5  # walled in
    g[wy - 1:wy + 2, wx - 1:wx + 2] = 1
    g[wy, wx] = 0
    g[0, 0] = 0  # corner
    g[0, 1] = g[1, 0] = g[1, 1] = 1
    ex = W // 2 - 9  # bottom edge
    g[H - 2:H, ex - 1:ex + 2] = 1
    g[H - 1, ex] = 0
    for x in (17, W // 4 + 3, W - 30):  # a tile's last and first row
        g[3, x] = g[4, x + 1] = 1
    for y in (1, 3, 4, 6):  # the wave seam and lanes 0 / 63
        g[y, 255 % W] = 1
        g[y, 256 % W] = 1
        g[y, W - 1] = 1
    g[5, 0] = g[6, 0] = 1
    nx = gx + 1 if gx + 1 < W else gx - 1  # the goal next to an occupied cell
    g[gy, nx] = 1
    g[gy, gx] = 0
    return g, goal, wy * W + wx, (wy - 1) * W + wx


def _cpu_shares(grid, goal, block, b0=None):
    """The launch-per-step loop on the CPU (the oracle's belief update with the
    device's blocked normalisation: a block's first step divides by the mass
    and scales by 2^96, or by 1 for block 1): the share of free cells with a
    non-zero belief after every launch of the segment."""
    from oracle import oracle as O
    from path_planning_2d_amd import synthetic as S
    H, W = grid.shape
    T, L, _ = O.model_pomdp(grid, goal)
    b = (S.uniform_belief(grid) if b0 is None else b0).astype(np.float32)
    free = grid.reshape(-1) == 0
    us, zs = ct.segments(block)[0]
    ends = {hi for _, hi in _launches(us.size)}
    tiny = np.finfo(np.float32).tiny
    out = []
    for t in range(us.size):
        p = O.belief_update(H, W, T, L, b, us[t], zs[t])
        if t % block == 0:
            inv = np.float32(1.0) / np.float32(b.sum(dtype=np.float64))
            inv = np.float32(inv * np.float32(2.0 ** 96 if block > 1 else 1.0))
            p = p * inv
        p = np.where(np.abs(p) < tiny, np.float32(0), p).astype(np.float32)  # FTZ
        b = p
        if t + 1 in ends:
            out.append(np.count_nonzero(b[free]) / int(free.sum()))
    return out


EDIT_SHAPES = [s for s in SHAPES if (s[0], s[1]) in ((16, 1024), (8, 256))]
EDIT_IDS = [f"{s[0]}x{s[1]}" for s in EDIT_SHAPES]


@pytest.mark.parametrize("block", [8, 1])
@pytest.mark.parametrize("H,W,cus,tiling", EDIT_SHAPES, ids=EDIT_IDS)
def test_edited_maps(pp2, H, W, cus, tiling, block):
    grid, goal = _seeded_grid(pp2, H, W)
    egrid, egoal, walled, occ = _edit(grid, goal)
    assert egrid.reshape(-1)[walled] == 0 and egrid.reshape(-1)[occ] == 1
    shares = _cpu_shares(egrid, egoal, block)
    print(f"{H} x {W} edited, block {block}: CPU non-zero shares {shares}")
    assert min(shares) >= MIN_NONZERO, "the reference loses the coverage on this map"
    cs = _trio(pp2, egrid, egoal, cus, block)
    with cs[0], cs[1], cs[2]:
        assert cs[0].resident_tiling() == tiling
        assert cs[0].resident_masked() == (True, 0)
        _run_and_compare(cs, egrid, block, f"{H} x {W} edited")


@pytest.mark.parametrize("H,W,cus,tiling", EDIT_SHAPES, ids=EDIT_IDS)
def test_map_without_occupied_cells(pp2, H, W, cus, tiling):
    from path_planning_2d_amd import synthetic as S
    grid = np.zeros((H, W), np.uint8)
    goal = S.synth_goal(grid)
    shares = _cpu_shares(grid, goal, 8)
    assert min(shares) >= MIN_NONZERO, shares
    cs = _trio(pp2, grid, goal, cus, 8)
    with cs[0], cs[1], cs[2]:
        assert cs[0].resident_tiling() == tiling
        assert cs[0].resident_masked() == (True, 0)
        _run_and_compare(cs, grid, 8, f"{H} x {W} open")


def test_mass_on_blocked_and_walled_in_cells(pp2):
    """An initial belief with mass on an occupied cell and on the walled-in
    free cell: both keep it (their only term is the centre one), bit for bit
    as the launch-per-step path has it."""
    from path_planning_2d_amd import synthetic as S
    H, W, cus, tiling = SHAPES[0]
    grid, goal = _seeded_grid(pp2, H, W)
    egrid, egoal, walled, occ = _edit(grid, goal)
    b0 = S.uniform_belief(egrid).astype(np.float64)
    b0[occ] = 40.0 * b0.max()
    b0[walled] = 25.0 * b0.max()
    b0 = (b0 / b0.sum()).astype(np.float32)
    shares = _cpu_shares(egrid, egoal, 8, b0)
    assert min(shares) >= MIN_NONZERO, shares
    cs = _trio(pp2, egrid, egoal, cus, 8, b0)
    with cs[0], cs[1], cs[2]:
        assert cs[0].resident_masked() == (True, 0)
        seen = _run_and_compare(cs, egrid, 8, f"{H} x {W} mass on blocked cells",
                                watch=(occ, walled))
        print("raw belief at (occupied, walled-in) per launch:", [s.tolist() for s in seen])
        # (bit equality with the reference is _same's; the mass is really there)
        assert (seen[0] > 0).all() and (seen[1] > 0).all() and (seen[2] > 0).all()


# ---------------------------------------------------------------- fallback
def test_changed_models_are_not_admitted(pp2):
    H, W, cus, tiling = SHAPES[1]
    grid, goal = _seeded_grid(pp2, H, W)
    cs = _trio(pp2, grid, goal, cus, 8)
    m, u, s = cs
    flat = grid.reshape(-1)
    with m, u, s:
        T0, L0, R0, C0 = m.model_download()
        assert m.resident_masked() == (True, 0)

        def upload(T, Cc):
            for c in cs:
                c.model_upload(T, None, None, Cc)
                assert c.model_dict_info()[1]
            _restart(cs, grid, 8)

        # 1. one cell's off-centre weight
        T = T0.copy()
        cell, a, i = next((c, a, i) for c in np.nonzero(flat == 0)[0] for a in (0, 2, 5, 7)
                          for i in (1, 3, 5, 7) if T0[c, a, i] == np.float32(0.1))
        T[cell, a, i] = 0.125
        upload(T, C0)
        assert m.resident_masked()[0] is False, "one changed weight"
        _run_and_compare(cs, grid, 8, "one weight changed", masked=False)
        # 2. a blocked cell whose cost differs for one action
        Cc = C0.copy()
        occ = int(np.nonzero(flat == 1)[0][3])
        Cc[occ, 7] = 3.0
        upload(T0, Cc)
        assert m.resident_masked()[0] is False, "a blocked cell's cost differs by action"
        _run_and_compare(cs, grid, 8, "blocked cell's cost changed", masked=False)
        # 3. one action's side weight, everywhere
        T = T0.copy()
        side = T[:, 5, :]
        side[(side == np.float32(0.1)) & (np.arange(9) != 4)[None, :]] = 0.05
        upload(T, C0)
        assert m.resident_masked()[0] is False, "one action's side weight changed"
        _run_and_compare(cs, grid, 8, "side weight changed", masked=False)
        assert m.resident_masked()[1] == 0
        # the untouched model again
        upload(T0, C0)
        assert m.resident_masked()[0] is True, "the generated model is admitted again"
        _run_and_compare(cs, grid, 8, "generated model again", masked=True)
