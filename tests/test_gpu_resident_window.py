"""GPU: the top of the resident loop's step (pp2_resident.hip,
issue_window_rows and window_row in k_loop_resident and k_sweep_resident):
the whole-row instance issues every LDS read of its window rows -- the b and J
quads of the rows that live in the tile and the edge dwords of lanes 0 / 63 --
in one burst behind the class dwords and the action-0 records, an edge wave
before it polls its neighbour's granules; k_sweep_resident does the same with
its J rows and issues its action-0 records with them.

The bar is bit equality with the launch-per-step path (TUNE_RESIDENT 0,
TUNE_STEP_PAIRS 0): raw belief bits, the mass, J bits and A after every
compared launch; for the sweeps, J and A bit for bit against launch-per-sweep,
and the solve's sweep count and norm.

Which row of a window comes from where is decided per wave by its row's place
in the tile, so the shapes walk through every kind of row:

  16 x 1024 / 4 CUs  (4, 4, 1)  the bench's tile: grid top, tile first row,
                                interior rows, tile last row, grid bottom; four
                                waves per row, so lanes 0 / 63 read a neighbour
                                wave's dword
  8 x 256 / 2 CUs    (2, 4, 1)  one wave per row: both edge dwords are the
                                zero pads
  6 x 512 / 2 CUs    (2, 3, 1)  3-row tiles, two waves per row
  7 x 512 / 2 CUs    (2, 4, 1)  a partial last tile: its third row's window
                                row below is off the grid inside the tile
  6 x 510 / 2 CUs    (2, 3, 1)  a width that is no multiple of 256, padded to
                                512 columns: the last wave's lane 63 reads the
                                zero pad behind two padded cells
  6 x 300 / 2 CUs    (0, 0, 0)  padded to 304 columns, which is no multiple of
                                256: the plan admits no resident tiling
                                (resident_plan_tc), so this grid runs the
                                launch-per-pair kernels; compared all the same,
                                so that a plan that comes to admit it is tested
                                (6 x 510 is the padded resident case)
  4 x 1024 / 4 CUs   (4, 1, 1)  one-row tiles (the plan admits them): both
                                outer rows come from polls, the LDS burst is
                                the wave's own row alone

The trajectory is the first segment of tests/covering_trajectory.py for the
normalisation block (42 steps; all nine actions within its first 17, asserted),
run as launches of 1, 2, 5 and 25 steps and the rest (9): odd and even lengths
(a launch starts in LDS buffer 0 and the step alternates the two, so both
parities end a launch), the short-trajectory instance (<= 24 steps) and the
long one, a single step between resident launches (the one-step kernel) and
consecutive resident launches.  TUNE_NORM_BLOCK 8 and 1 (every step a block
start and an arrival).  As in test_gpu_loop_coverage.py at least 85 % of the
free cells of the reference must hold a non-zero belief after every launch:
bit equality of flushed cells proves nothing.
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
    (6, 512, 2, (2, 3, 1)),
    (7, 512, 2, (2, 4, 1)),
    (6, 510, 2, (2, 3, 1)),
    (6, 300, 2, (0, 0, 0)),
    (4, 1024, 4, (4, 1, 1)),
]
IDS = [f"{s[0]}x{s[1]}" for s in SHAPES]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _coded_pair(pp2, H, W, cus, block):
    """A resident context on `cus` CUs and a launch-per-step (and
    launch-per-sweep) one on the first seeded grid whose model is
    dictionary-coded."""
    from path_planning_2d_amd import synthetic as S
    for seed in range(H * 7 + W, H * 7 + W + 8):
        grid = S.synth_grid(H, W, seed)
        goal = S.synth_goal(grid)
        a = pp2.GridContext(grid, goal, gamma=float(GAMMA))
        a.model_generate()
        if a.model_dict_info()[1]:
            break
        a.close()
    else:
        pytest.fail(f"no coded model for {H} x {W}")
    b = pp2.GridContext(grid, goal, gamma=float(GAMMA))
    b.model_generate()
    assert b.model_dict_info()[1]
    a.set_tuning(a.TUNE_RESIDENT_CUS, cus)
    b.set_tuning(b.TUNE_RESIDENT, 0)
    b.set_tuning(b.TUNE_STEP_PAIRS, 0)
    b0 = S.uniform_belief(grid)
    for c in (a, b):
        c.set_tuning(c.TUNE_NORM_BLOCK, block)
        c.belief_set(b0)
        c.mdp_reset()
    return grid, a, b


def _same_ja(a, b, what):
    Ja, Aa = a.mdp_get()
    Jb, Ab = b.mdp_get()
    np.testing.assert_array_equal(Ja.view(np.uint32), Jb.view(np.uint32), err_msg=f"J {what}")
    np.testing.assert_array_equal(Aa, Ab, err_msg=f"A {what}")


def _same(a, b, what):
    """Raw belief bits, mass bits, J bits and A; returns the reference's raw belief."""
    ra, ma = a.belief_get_raw()
    rb, mb = b.belief_get_raw()
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32),
                                  err_msg=f"raw belief {what}")
    assert np.float32(ma).view(np.uint32) == np.float32(mb).view(np.uint32), (what, ma, mb)
    _same_ja(a, b, what)
    return rb


def _launches(n):
    out, lo = [], 0
    for m in RUNS:
        out.append((lo, lo + m))
        lo += m
    assert n - lo >= 2, "the rest is a resident launch"
    out.append((lo, n))
    return out


@pytest.mark.parametrize("block", [8, 1])
@pytest.mark.parametrize("H,W,cus,tiling", SHAPES, ids=IDS)
def test_window_rows_equal_single_steps(pp2, H, W, cus, tiling, block):
    grid, a, b = _coded_pair(pp2, H, W, cus, block)
    free = grid.reshape(-1) == 0
    with a, b:
        assert a.resident_tiling() == tiling, a.resident_tiling()
        on = tiling != (0, 0, 0)
        assert (a.loop_steps_per_launch() == RESIDENT_STEPS) == on, "resident loop (not) selected"
        assert b.loop_steps_per_launch() == 1
        us, zs = ct.segments(block)[0]
        assert set(us[:17].tolist()) == set(range(ct.ACTIONS))
        launches = _launches(us.size)
        lens = [hi - lo for lo, hi in launches]
        assert {m % 2 for m in lens if m >= 2} == {0, 1}
        assert any(2 <= m <= SHORT_STEPS for m in lens) and any(m > SHORT_STEPS for m in lens)
        resident, low = 0, 1.0
        for lo, hi in launches:
            a.loop_run(us[lo:hi], zs[lo:hi])
            b.loop_run(us[lo:hi], zs[lo:hi])
            a.synchronize()
            resident += len(ct.resident_launches(lo, hi)) if on else 0
            what = f"{H} x {W} block {block}, after steps [{lo}, {hi})"
            assert a.resident_launches()[0] == resident and b.resident_launches() == (0, 0), what
            assert a.resident_status()[0] == 0, f"a resident launch fell back: {what}"
            raw = _same(a, b, what)
            assert np.isfinite(raw).all(), what
            share = np.count_nonzero(raw[free]) / int(free.sum())
            low = min(low, share)
            print(f"{what}: {share:.3f} of the free cells non-zero")
            assert share >= MIN_NONZERO, f"{share:.3f} of the free cells non-zero {what}"
        assert resident == (len(launches) - 1 if on else 0)
        print(f"{H} x {W} block {block}: {resident} resident launches, non-zero share >= {low:.3f}")


@pytest.mark.parametrize("H,W,cus,tiling", SHAPES[:4], ids=IDS[:4])
def test_sweep_window_rows_equal_per_sweep(pp2, H, W, cus, tiling):
    """k_sweep_resident on the same tiles: mdp_sweep(n) for n = 2, 7 and 100
    (consecutive launches on one J; odd and even counts end in either buffer)
    against n sweep launches, then mdp_solve capped at 150 sweeps from J = 0."""
    grid, a, b = _coded_pair(pp2, H, W, cus, 8)
    with a, b:
        assert a.resident_tiling() == tiling, a.resident_tiling()
        for k, n in enumerate((2, 7, 100)):
            a.mdp_sweep(n)
            b.mdp_sweep(n)
            assert a.resident_launches()[1] == k + 1 and b.resident_launches()[1] == 0
            assert a.resident_status()[0] == 0, "a resident launch fell back"
            _same_ja(a, b, f"{H} x {W} after mdp_sweep({n})")
        assert np.count_nonzero(b.mdp_get()[0]) > 0
        for c in (a, b):
            c.mdp_reset()
        ra, rb = a.mdp_solve(150), b.mdp_solve(150)
        assert a.resident_launches()[1] >= 4 and b.resident_launches()[1] == 0
        assert a.resident_status()[0] == 0, "a resident launch fell back"
        assert ra[0] == rb[0] and ra[0] >= 100, (ra, rb)
        assert np.float32(ra[1]) == np.float32(rb[1]), (ra, rb)
        _same_ja(a, b, f"{H} x {W} after mdp_solve(150)")
