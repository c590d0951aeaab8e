"""GPU: the resident loop's step pipeline (pp2_resident.hip: the
software-pipelined backup, mass partials only where they are read) on small
grids that still make the flagship's tile shapes.

TUNE_RESIDENT_CUS narrows the plan (rt = ceil(rows / CUs)), so a 16 x 1024
grid on 4 CUs runs the bench's tile -- 4 rows of 4 waves, 16 waves, top /
middle / bottom tiles -- in well under a second.  The bar is bit equality with
the launch-per-step path (TUNE_RESIDENT 0, TUNE_STEP_PAIRS 0): raw belief and
mass bits, J bits and A, after every chunk of a 17-step trajectory run as
(0,2) (2,5) (5,6) (6,17): odd and even lengths, block starts inside a launch
(TUNE_NORM_BLOCK 8, 3, 1) and the last step's arg-min path.
"""
import numpy as np
import pytest

from conftest import GAMMA

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048
CHUNKS = ((0, 2), (2, 5), (5, 6), (6, 17))

# (H, W, RESIDENT_CUS, tiles, rows per tile):
#   16 x 1024 / 4: the bench's tile (4 rows x 4 waves), top / middle / bottom
#   10 x 1024 / 3: 4-row tiles, the last one 2 rows (invalid waves)
#   32 x 256 / 2: 16-row tiles, one wave per row, 14 interior rows
#   6 x 512 / 2: 3-row tiles, 6 waves
SHAPES = [(16, 1024, 4, 4, 4), (10, 1024, 3, 3, 4), (32, 256, 2, 2, 16), (6, 512, 2, 2, 3)]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _coded_pair(pp2, H, W, cus, block):
    """A resident context narrowed to `cus` CUs and a launch-per-step one on
    the first seeded grid whose model is dictionary-coded."""
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


@pytest.mark.parametrize("block", [8, 3, 1])
@pytest.mark.parametrize("H,W,cus,tiles,rt", SHAPES)
def test_pipeline_equals_single_steps(pp2, H, W, cus, tiles, rt, block):
    from path_planning_2d_amd import synthetic as S
    grid, a, b = _coded_pair(pp2, H, W, cus, block)
    with a, b:
        assert a.resident_tiling() == (tiles, rt, 1), a.resident_tiling()
        assert a.loop_steps_per_launch() == RESIDENT_STEPS, "resident loop not selected"
        assert b.loop_steps_per_launch() == 1
        us, zs, _ = S.synth_trajectory(grid, 17, seed=11)
        launches = 0
        for lo, hi in CHUNKS:
            a.loop_run(us[lo:hi], zs[lo:hi])
            b.loop_run(us[lo:hi], zs[lo:hi])
            a.synchronize()
            launches += hi - lo >= 2  # a one-step run takes the single-step launch
            assert a.resident_launches()[0] == launches and b.resident_launches() == (0, 0)
            assert a.resident_status()[0] == 0, "a resident launch fell back"
            _same(a, b, f"after {hi} steps")


@pytest.mark.parametrize("n", [2, 7])
def test_pipeline_sweeps_equal_per_sweep(pp2, n):
    """k_sweep_resident on the bench's tile shape: mdp_sweep(n) as one
    resident launch equals n single sweeps, J bits and A."""
    grid, a, b = _coded_pair(pp2, 16, 1024, 4, 8)
    with a, b:
        a.mdp_sweep(n)
        for _ in range(n):
            b.mdp_sweep(1)
        assert a.resident_launches()[1] == 1 and b.resident_launches()[1] == 0
        Ja, Aa = a.mdp_get()
        Jb, Ab = b.mdp_get()
        np.testing.assert_array_equal(Ja.view(np.uint32), Jb.view(np.uint32))
        np.testing.assert_array_equal(Aa, Ab)
