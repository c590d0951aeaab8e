"""GPU: the resident loop's early arrival (pp2_resident.hip: on an arrive step
that is not itself scaled, the wave's mass partial and the tile's arrival go
out right after the gather, before the backup).

The pattern is test_gpu_resident_pipeline.py's: TUNE_RESIDENT_CUS narrows the
plan so that small grids make the flagship's tile, the reference is the
launch-per-step path (TUNE_RESIDENT 0, TUNE_STEP_PAIRS 0) and the bar is bit
equality of the raw belief and mass bits, J bits and A after every chunk.

With normalisation block d the arrive steps are the absolute steps k with
(k + 1) % d == 0 and the block starts the steps k % d == 0.  The chunks of
_chunks(d) put an arrive step
  * last in a launch (the late order: its partials go to out_partials),
  * second to last in a launch (the block start after it is the last step),
  * in the middle of a launch that starts mid-block,
  * first in a launch,
and end with two launches queued back to back with no synchronize between
them, so that the arrival base and the ring carry over a chained launch.
Block 1 (every step arrives and starts a block) takes the late order
throughout.  One 40-step launch at block 2 has 20 block starts and runs past
the mass ring's length while blocks are in flight.
"""
import numpy as np
import pytest

from conftest import GAMMA

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048

# (H, W, RESIDENT_CUS, tiles, rows per tile):
#   16 x 1024 / 4: the bench's tile (4 rows x 4 waves), top / middle / bottom
#   10 x 1024 / 3: 4-row tiles, the last one 2 rows: its invalid waves store
#                  no partial and must not be counted for the arrival
#   32 x 256 / 2: 16-row tiles, one wave per row: the reducing wave is interior
SHAPES = [(16, 1024, 4, 4, 4), (10, 1024, 3, 3, 4), (32, 256, 2, 2, 16)]


def _chunks(d):
    """((lo, hi), synchronize and compare after it) per launch."""
    m = max(d, 2)
    return (((0, m), True),                    # arrive step m - 1 is the last step
            ((m, 2 * m + 1), True),            # arrive step 2m - 1 is the second to last
            ((2 * m + 1, 4 * m - 1), True),    # starts mid-block, arrive step 3m - 1 inside
            ((4 * m - 1, 5 * m + 2), True),    # arrive step 4m - 1 is the first step
            ((5 * m + 2, 6 * m + 3), False),   # queued back to back with the next one
            ((6 * m + 3, 8 * m + 2), True))


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


@pytest.mark.parametrize("block", [8, 4, 3, 2, 1])
@pytest.mark.parametrize("H,W,cus,tiles,rt", SHAPES)
def test_early_arrival_equals_single_steps(pp2, H, W, cus, tiles, rt, block):
    from path_planning_2d_amd import synthetic as S
    grid, a, b = _coded_pair(pp2, H, W, cus, block)
    with a, b:
        assert a.resident_tiling() == (tiles, rt, 1), a.resident_tiling()
        assert a.loop_steps_per_launch() == RESIDENT_STEPS, "resident loop not selected"
        assert b.loop_steps_per_launch() == 1
        chunks = _chunks(block)
        us, zs, _ = S.synth_trajectory(grid, chunks[-1][0][1], seed=11)
        launches = 0
        for (lo, hi), sync in chunks:
            assert hi - lo >= 2  # (a one-step run takes the single-step launch)
            a.loop_run(us[lo:hi], zs[lo:hi])
            b.loop_run(us[lo:hi], zs[lo:hi])
            launches += 1
            if not sync:
                continue
            a.synchronize()
            assert a.resident_launches()[0] == launches and b.resident_launches() == (0, 0)
            assert a.resident_status()[0] == 0, "a resident launch fell back"
            _same(a, b, f"after {hi} steps")


@pytest.mark.parametrize("H,W,cus,tiles,rt", SHAPES)
def test_block2_run_past_the_ring(pp2, H, W, cus, tiles, rt):
    """40 steps at block 2 in one launch: 20 block starts, the mass ring wraps."""
    from path_planning_2d_amd import synthetic as S
    grid, a, b = _coded_pair(pp2, H, W, cus, 2)
    with a, b:
        assert a.resident_tiling() == (tiles, rt, 1), a.resident_tiling()
        us, zs, _ = S.synth_trajectory(grid, 40, seed=13)
        a.loop_run(us, zs)
        b.loop_run(us, zs)
        a.synchronize()
        assert a.resident_launches()[0] == 1 and a.resident_status()[0] == 0
        _same(a, b, "after 40 steps")
