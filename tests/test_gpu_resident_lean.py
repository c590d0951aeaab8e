"""GPU: the masked whole-row instances without their non-arithmetic VALU work
(pp2_resident.hip, issue_window_rows_lean and take_q of the ResidentMasked
instances of k_loop_resident): every window row is read from LDS into the
same registers whatever its source -- the tile's row, a never-written row of
zeros in front of or behind the tile buffer for a row that is off the grid, the
neighbour tile's granules OR-ed over those zeros -- and the masked J quad is
computed once for the LDS store and the publish.

The bar is test_gpu_resident_masked.py's: raw belief bits, mass bits, J bits
and A after every launch, equal between the masked form (the query must say
the launches ran it), the class-table form of the same tiles
(TUNE_RESIDENT_MASKED 0) and launch-per-step, with at least 85 % of the free
cells non-zero after every launch.  The shapes are the ones whose wave roles
the other files' shapes miss (TUNE_RESIDENT_CUS sets the tiling):
  4 x 1024 / 4 CUs   rt = 1: every wave is a tile's first and last row
  4 x 256 / 2        rt = 2: no interior wave
  6 x 510 / 2        rt = 3
  7 x 512 / 2        a partial last tile (rt = 4, 3 rows: idle waves)
  4 x 256 / 1        one tile, no neighbour: both off-grid rows are the zeros
  16 x 1024 / 4      first, interior and last tiles
Launches of 1, 2, 3, 4, 5 and 9 steps and the rest (18) run in sequence on one
context, then, from a fresh belief, 26 steps (the long trajectory instance) and
the rest: the LDS buffer parity and the trajectory word's reload (t & 3 == 3)
fall on even and odd steps, and launches end on an even t (3, 5, 9 steps) and
on an odd one (2, 4, 26).  The norm block is 8 on every shape and 1, 2 and 3
on two of them (the 18- and 26-step launches hold two blocks or more; blocks 1
and 3 start on both parities of t).

The initial belief carries extra mass on the free cells of rows 0 and H - 1,
and the first launch (one step: the single-step kernel) leaves J non-zero
there, so a window row that should be the zeros and is not shows up as a value;
every launch must leave non-zero belief and J in both rows.
"""
import functools

import numpy as np
import pytest

import covering_trajectory as ct
from conftest import GAMMA

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048
SHORT_STEPS = 24
MIN_NONZERO = 0.85
RUNS_A = (1, 2, 3, 4, 5, 9)  # then the rest of segment 0
RUNS_B = (SHORT_STEPS + 2,)  # then the rest of segment 1

# H, W, CUs, (tiles, rows per tile, tile columns)
SHAPES = {
    "4x1024-rt1": (4, 1024, 4, (4, 1, 1)),
    "4x256-rt2": (4, 256, 2, (2, 2, 1)),
    "6x510-rt3": (6, 510, 2, (2, 3, 1)),
    "7x512-partial": (7, 512, 2, (2, 4, 1)),
    "4x256-one-tile": (4, 256, 1, (1, 4, 1)),
    "16x1024": (16, 1024, 4, (4, 4, 1)),
}
CASES = [(k, 8) for k in SHAPES] + [(k, d) for k in ("4x1024-rt1", "7x512-partial")
                                    for d in (1, 2, 3)]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


@functools.lru_cache(maxsize=None)
def _seeded_grid(H, W):
    """The first seed whose generated model is coded (test_gpu_resident_window.py's)."""
    import path_planning_2d_amd as P
    from path_planning_2d_amd import synthetic as S
    for seed in range(H * 7 + W, H * 7 + W + 8):
        grid = S.synth_grid(H, W, seed)
        goal = S.synth_goal(grid)
        with P.GridContext(grid, goal, gamma=float(GAMMA)) as c:
            c.model_generate()
            if c.model_dict_info()[1]:
                grid.setflags(write=False)
                return grid, goal
    pytest.fail(f"no coded model for {H} x {W}")


def _edge_heavy_belief(grid):
    """The uniform belief with four times the mass on the free cells of the
    grid's first and last rows."""
    from path_planning_2d_amd import synthetic as S
    b = S.uniform_belief(grid).astype(np.float64).reshape(grid.shape)
    b[0] *= 4.0
    b[-1] *= 4.0
    return (b / b.sum()).astype(np.float32).reshape(-1)


def _restart(cs, b0, block):
    for c in cs:
        c.set_tuning(c.TUNE_NORM_BLOCK, block)
        c.belief_set(b0)
        c.mdp_reset()


def _same(a, b, what):
    ra, ma = a.belief_get_raw()
    rb, mb = b.belief_get_raw()
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32),
                                  err_msg=f"raw belief {what}")
    assert np.float32(ma).view(np.uint32) == np.float32(mb).view(np.uint32), (what, ma, mb)
    Ja, Aa = a.mdp_get()
    Jb, Ab = b.mdp_get()
    np.testing.assert_array_equal(Ja.view(np.uint32), Jb.view(np.uint32), err_msg=f"J {what}")
    np.testing.assert_array_equal(Aa, Ab, err_msg=f"A {what}")
    return rb, Jb


def _launches(runs, n):
    out, lo = [], 0
    for m in runs:
        out.append((lo, lo + m))
        lo += m
    assert n - lo >= 2, "the rest is a resident launch"
    out.append((lo, n))
    return out


def _run_and_compare(cs, grid, us, zs, launches, tag):
    m, u, s = cs
    H, W = grid.shape
    free = grid.reshape(-1) == 0
    res0, msk0, ures0 = m.resident_launches()[0], m.resident_masked()[1], u.resident_launches()[0]
    resident = 0
    for lo, hi in launches:
        for c in cs:
            c.loop_run(us[lo:hi], zs[lo:hi])
        m.synchronize()
        u.synchronize()
        resident += len(ct.resident_launches(lo, hi))
        what = f"{tag}, after steps [{lo}, {hi})"
        assert m.resident_launches()[0] == res0 + resident, what
        assert u.resident_launches()[0] == ures0 + resident, what
        assert s.resident_launches() == (0, 0), what
        assert m.resident_masked()[1] == msk0 + resident, f"the masked form did not run: {what}"
        assert u.resident_masked()[1] == 0, what
        assert m.resident_status()[0] == 0 and u.resident_status()[0] == 0, f"fell back: {what}"
        raw, J = _same(m, s, f"masked vs per-step, {what}")
        _same(u, s, f"class tables vs per-step, {what}")
        assert np.isfinite(raw).all(), what
        share = np.count_nonzero(raw[free]) / int(free.sum())
        print(f"{what}: {share:.3f} of the free cells non-zero")
        assert share >= MIN_NONZERO, f"{share:.3f} of the free cells non-zero {what}"
        for name, v in (("belief", raw.reshape(H, W)), ("J", J.reshape(H, W))):
            assert np.count_nonzero(v[0]) and np.count_nonzero(v[-1]), \
                f"{name} is zero in the grid's first or last row: {what}"
    return resident


@pytest.mark.parametrize("shape,block", CASES, ids=[f"{k}-block{d}" for k, d in CASES])
def test_lean_masked_equals_class_tables_and_single_steps(pp2, shape, block):
    H, W, cus, tiling = SHAPES[shape]
    grid, goal = _seeded_grid(H, W)
    b0 = _edge_heavy_belief(grid)
    assert np.count_nonzero(b0.reshape(H, W)[0]) and np.count_nonzero(b0.reshape(H, W)[-1])
    cs = [pp2.GridContext(grid, goal, gamma=float(GAMMA)) for _ in range(3)]
    m, u, s = cs
    with m, u, s:
        for c in cs:
            c.model_generate()
            assert c.model_dict_info()[1]
        for c in (m, u):
            c.set_tuning(c.TUNE_RESIDENT_CUS, cus)
        u.set_tuning(u.TUNE_RESIDENT_MASKED, 0)
        s.set_tuning(s.TUNE_RESIDENT, 0)
        s.set_tuning(s.TUNE_STEP_PAIRS, 0)
        assert m.resident_tiling() == tiling and u.resident_tiling() == tiling
        assert m.loop_steps_per_launch() == RESIDENT_STEPS == u.loop_steps_per_launch()
        assert s.loop_steps_per_launch() == 1
        assert m.resident_masked() == (True, 0), "a generated model is admitted"
        segs = ct.segments(block)
        for seg, runs in ((0, RUNS_A), (1, RUNS_B)):
            us, zs = segs[seg]
            launches = _launches(runs, us.size)
            # a launch of two blocks or more, launches that end on either parity
            assert max(hi - lo for lo, hi in launches) >= 2 * block
            assert {(hi - lo) % 2 for lo, hi in launches if hi - lo >= 2} == {0, 1} or seg == 1
            _restart(cs, b0, block)
            n = _run_and_compare(cs, grid, us, zs, launches, f"{shape} block {block} segment {seg}")
            assert n == len(launches) - (1 if runs[0] == 1 else 0)
