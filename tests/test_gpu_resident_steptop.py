"""GPU: the head of the resident loop's step (pp2_resident.hip): (u, z) taken
from a trajectory word held in an SGPR (byte lane t & 3 of the launch's word
t >> 2, reloaded every fourth step), the block phase kept as a counter instead
of (kstep0 + t) % depth, and the whole-row gather's one-round-trip table reads.

The bar is bit equality with the launch-per-step path (TUNE_RESIDENT 0,
TUNE_STEP_PAIRS 0): raw belief and mass bits, J bits and A, after every run.

The trajectory is synth_trajectory(seed 13): its first 96 steps hold all nine
actions at every t mod 4 (asserted), so every case of the gather's dispatch
is taken from every byte lane.  It is run as consecutive launches of 2, 3, 4,
5, 7, 9, 23, 24 and 25 steps and the rest -- these nine come to 102 steps, so
the trajectory is drawn 152 steps long (the 96 are its prefix) and the rest is
50: the shortest multiple of 8 at which the launches' own byte lanes hold all
nine actions too (a byte's lane is its step within the launch; asserted).  The
launches start at offsets 0, 2, 5, 9, 14, 21, 30, 53, 77 and 102 (1, 2 and 0
mod 4: the same step meets different lanes than its t mod 4), use both kernel
instances (<= 24 steps, > 24), end in every lane, and reload the word at the
short instance's last word (step 20) and past it (step 24).

TUNE_NORM_BLOCK 8, 5, 3 and 1 over the same launches: at depth 8 every launch
but the first starts at a non-zero phase (kstep0 % depth), at 5 and 3 most do
(asserted: at least five), and depth 1 makes every step both a block start
and an arrival.
"""
import numpy as np
import pytest

from conftest import GAMMA

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048
SHORT_STEPS = 24  # launches of at most 24 steps run the short-trajectory instance
RUNS = (2, 3, 4, 5, 7, 9, 23, 24, 25)
STEPS = 152
TRAJ_SEED = 13

# (H, W, tunings of the resident context, (tiles, rows per tile, tile columns)):
#   16 x 1024 / 4 CUs: the bench's tile (4 rows x 4 waves), the whole-row
#                      instance; top, middle and bottom tiles
#   6 x 512 / 2 CUs: 3-row tiles, 6 waves
#   13 x 1024 / 4 CUs, two tile columns: 7 x 512 tiles, the 2-D instance
#   12 x 1024 / 8 CUs, two tile columns: 3 x 512 tiles of 384 threads, the
#                      register-rich 2-D instance (class bytes in registers)
SHAPES = [
    (16, 1024, (("TUNE_RESIDENT_CUS", 4),), (4, 4, 1)),
    (6, 512, (("TUNE_RESIDENT_CUS", 2),), (2, 3, 1)),
    (13, 1024, (("TUNE_RESIDENT_CUS", 4), ("TUNE_RESIDENT_TILE_COLS", 2)), (4, 7, 2)),
    (12, 1024, (("TUNE_RESIDENT_CUS", 8), ("TUNE_RESIDENT_TILE_COLS", 2)), (8, 3, 2)),
]


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _coded_pair(pp2, H, W, tune, block):
    """A resident context with the tunings `tune` and a launch-per-step one on
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
    for name, v in tune:
        a.set_tuning(getattr(a, name), v)
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


def _chunks(n):
    out, lo = [], 0
    for m in RUNS:
        out.append((lo, lo + m))
        lo += m
    assert lo < n
    out.append((lo, n))
    return out


def _check_trajectory(us):
    """Every action at every t mod 4 of the first 96 steps, and at every byte
    lane (step within its launch, mod 4) of the launches; the launches end in
    every lane and use both kernel instances."""
    nine = set(range(9))
    for lane in range(4):
        assert set(us[:96][lane::4].tolist()) == nine, f"t mod 4 == {lane}"
    chunks = _chunks(us.size)
    seen = [set() for _ in range(4)]
    for lo, hi in chunks:
        for t in range(lo, hi):
            seen[(t - lo) & 3].add(int(us[t]))
    assert all(s == nine for s in seen), seen
    assert {(hi - lo) % 4 for lo, hi in chunks} == {0, 1, 2, 3}
    assert any(hi - lo <= SHORT_STEPS for lo, hi in chunks)
    assert any(hi - lo > SHORT_STEPS for lo, hi in chunks)
    return chunks


@pytest.mark.parametrize("block", [8, 5, 3, 1])
@pytest.mark.parametrize("H,W,tune,tiling", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_byte_lanes_and_phase_equal_single_steps(pp2, H, W, tune, tiling, block):
    from path_planning_2d_amd import synthetic as S
    grid, a, b = _coded_pair(pp2, H, W, tune, block)
    with a, b:
        assert a.resident_tiling() == tiling, a.resident_tiling()
        assert a.loop_steps_per_launch() == RESIDENT_STEPS, "resident loop not selected"
        assert b.loop_steps_per_launch() == 1
        us, zs, _ = S.synth_trajectory(grid, STEPS, seed=TRAJ_SEED)
        chunks = _check_trajectory(us)
        if block > 1:  # launches that start inside a block (kstep0 % depth != 0)
            assert sum(lo % block != 0 for lo, _ in chunks) >= 5, (block, chunks)
        for k, (lo, hi) in enumerate(chunks):
            a.loop_run(us[lo:hi], zs[lo:hi])
            b.loop_run(us[lo:hi], zs[lo:hi])
            a.synchronize()
            assert a.resident_launches()[0] == k + 1 and b.resident_launches() == (0, 0)
            assert a.resident_status()[0] == 0, "a resident launch fell back"
            _same(a, b, f"block {block}, after steps [{lo}, {hi})")


def test_trajectory_cap(pp2):
    """One run of 2049 steps: a launch of the trajectory argument's whole 2048
    bytes (no word is read past it) and a launch of one step."""
    from path_planning_2d_amd import synthetic as S
    H, W, tune, tiling = SHAPES[0]
    grid, a, b = _coded_pair(pp2, H, W, tune, 8)
    with a, b:
        assert a.resident_tiling() == tiling, a.resident_tiling()
        assert a.loop_steps_per_launch() == RESIDENT_STEPS, "resident loop not selected"
        us, zs, _ = S.synth_trajectory(grid, RESIDENT_STEPS + 1, seed=TRAJ_SEED)
        a.loop_run(us, zs)
        b.loop_run(us, zs)
        a.synchronize()
        assert a.resident_launches()[0] == 2 and b.resident_launches() == (0, 0)
        assert a.resident_status()[0] == 0, "a resident launch fell back"
        _same(a, b, f"after {RESIDENT_STEPS + 1} steps")
