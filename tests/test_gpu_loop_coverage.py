"""GPU: every (action, observation) pair and every action transition at every
phase of a normalisation block, through every implementation of pp2_loop_run.

Inside the loop kernels u is not data: it selects one of nine specialisations
of the belief gather (pp2_resident.hip belief_any / belief_any_pre /
belief_any_regs) and the class rows issued ahead of it, z the row of the
likelihood table, and the resident loop moves those reads across step and
block-start boundaries.  The other loop tests take their trajectories from
synthetic.synth_trajectory, which reaches a fraction of that space (DESIGN.md
"Parity"); these run tests/covering_trajectory.py's segments: all 144 (u, z)
and all 81 * d (u_t, u_{t+1}, t % d).

The chain: the resident, pair and sharded paths equal the launch-per-step
path (TUNE_RESIDENT 0, TUNE_STEP_PAIRS 0) -- bit for bit where the operation
sequence is the same --, and one launch-per-step belief update equals the
oracle bit for bit, each over all 144 pairs.

What keeps a test from passing on nothing:
  * after every compared launch at least 85 % of the free cells of the
    REFERENCE context hold a non-zero raw belief (every segment starts from
    belief_set and is at most 49 steps long for this);
  * the pairs and triples are recounted from the launches that really ran --
    a transition counts only when both steps lie in one launch, a one-step
    run (the single-step launch) counts for nothing -- and all 144 pairs and
    95 % of the triples must lie inside launches of the path under test;
  * tilings, steps per launch, launch counts and the fall-back counter are
    asserted, and every context asserts a coded model.
"""
import functools

import numpy as np
import pytest

import covering_trajectory as ct
from conftest import GAMMA, assert_rel_close, golden, golden_map

pytestmark = pytest.mark.gpu

RESIDENT_STEPS = 2048
MIN_NONZERO = 0.85
MIN_TRIPLES = 0.95
FTZ_FLOOR = 1e-30  # test_gpu_shards.py's: the order of the normalising sum


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def _coded_pair(pp2, H, W, block, tune_a):
    """Context a with the tunings of the path under test and a launch-per-step
    context b on the first seeded grid whose model is dictionary-coded."""
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
    for key, value in tune_a:
        a.set_tuning(getattr(a, key), value)
    b.set_tuning(b.TUNE_RESIDENT, 0)
    b.set_tuning(b.TUNE_STEP_PAIRS, 0)
    for c in (a, b):
        c.set_tuning(c.TUNE_NORM_BLOCK, block)
    return grid, a, b


def _same(a, b, what):
    """test_gpu_resident.py's _same; returns the reference's raw belief."""
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


def _nonzero_share(raw, free, what):
    share = np.count_nonzero(raw[free]) / int(free.sum())
    assert np.isfinite(raw).all(), what
    assert share >= MIN_NONZERO, f"{share:.3f} of the free cells non-zero {what}"
    return share


def _where(d, layout, r, lo, hi, us, zs):
    return (f"block {d}, layout {layout}, segment {r}, after steps [{lo}, {hi}) "
            f"u {us[lo:hi].tolist()} z {zs[lo:hi].tolist()}")


def _drive(a, b, grid, d, layouts, launches_of, resident):
    """The protocol of every unsharded case: mdp_reset once, belief_set per
    segment, the segment's launches on both contexts, bit equality after every
    compared launch.  Returns the pairs and triples that lay inside launches
    of the path under test and the smallest non-zero share seen."""
    from path_planning_2d_amd import synthetic as S
    free = grid.reshape(-1) == 0
    b0 = S.uniform_belief(grid)
    for c in (a, b):
        c.mdp_reset()
    pairs, triples, launches, low = set(), set(), 0, 1.0
    for layout in layouts:
        for r, (us, zs) in enumerate(ct.segments(d)):
            for c in (a, b):
                c.belief_set(b0)
            for (lo, hi), sync in ct.layout_chunks(us.size, layout, d, r):
                a.loop_run(us[lo:hi], zs[lo:hi])
                b.loop_run(us[lo:hi], zs[lo:hi])
                ran = launches_of(lo, hi)
                p, t = ct.coverage(us, zs, ran, d)
                pairs |= p
                triples |= t
                launches += len(ran)
                if not sync:
                    continue  # queued back to back with the next launch
                what = _where(d, layout, r, lo, hi, us, zs)
                if resident:
                    a.synchronize()
                    assert a.resident_launches()[0] == launches, what
                    assert a.resident_status()[0] == 0, f"a resident launch fell back: {what}"
                assert b.resident_launches() == (0, 0)
                low = min(low, _nonzero_share(_same(a, b, what), free, what))
    return pairs, triples, low


# (H, W, tunings of the resident context, (tiles, rows per tile, tile columns)):
#   16 x 1024 / 4 CUs: the bench's tile (4 rows x 4 waves): whole-row pipelined
#                      (TC = 1), top / middle / bottom tiles
#   10 x 1024 / 3 CUs: the same with a partial last tile
#   32 x 256 / 2 CUs: one wave per row, the reducing wave interior
#   12 x 1024 / 8 CUs, two tile columns: 3 x 512 tiles of 384 threads, the
#                      register-rich TC = 3 instance (up to 768 threads)
#   13 x 1024 / 4 CUs, two tile columns: 7 x 512 tiles of 896 threads, the
#                      TC = 2 instance; the last tile row holds 6 rows
RESIDENT_SHAPES = [
    (16, 1024, (("TUNE_RESIDENT_CUS", 4),), (4, 4, 1)),
    (10, 1024, (("TUNE_RESIDENT_CUS", 3),), (3, 4, 1)),
    (32, 256, (("TUNE_RESIDENT_CUS", 2),), (2, 16, 1)),
    (12, 1024, (("TUNE_RESIDENT_CUS", 8), ("TUNE_RESIDENT_TILE_COLS", 2)), (8, 3, 2)),
    (13, 1024, (("TUNE_RESIDENT_CUS", 4), ("TUNE_RESIDENT_TILE_COLS", 2)), (4, 7, 2)),
]


@pytest.mark.parametrize("block", [8, 3, 1])
@pytest.mark.parametrize("H,W,tune,tiling", RESIDENT_SHAPES,
                         ids=[f"{s[0]}x{s[1]}" for s in RESIDENT_SHAPES])
def test_resident_covers_every_pair_and_transition(pp2, H, W, tune, tiling, block):
    grid, a, b = _coded_pair(pp2, H, W, block, tune)
    with a, b:
        assert a.resident_tiling() == tiling, a.resident_tiling()
        assert a.loop_steps_per_launch() == RESIDENT_STEPS, "resident loop not selected"
        assert b.loop_steps_per_launch() == 1
        pairs, triples, low = _drive(a, b, grid, block, ct.RESIDENT_LAYOUTS,
                                     ct.resident_launches, resident=True)
        print(f"{H} x {W} block {block}: {len(pairs)} pairs, {len(triples)} of {81 * block} "
              f"triples inside resident launches, non-zero share >= {low:.3f}")
        assert len(pairs) == 144
        assert len(triples) >= MIN_TRIPLES * 81 * block


@pytest.mark.parametrize("block", [8, 5, 3])
def test_step_pairs_cover_every_pair_and_transition(pp2, block):
    """k_loop_pair_coded holds two steps' (u, z) in one launch.  A pair never
    spans a block start (pp2_runtime.cpp can_pair), so of the 81 * d triples
    a pair launch can hold the 81 * (d - 1) with t % d <= d - 2; the bar is
    95 % of those, and every one of those phases."""
    H, W = 24, 512
    assert 5 * (2 * W + 8) <= 3 * 4096
    grid, a, b = _coded_pair(pp2, H, W, block,
                             (("TUNE_RESIDENT", 0), ("TUNE_STEP_PAIRS", 2)))
    with a, b:
        assert a.loop_steps_per_launch() == 2, "step pairs not selected"
        assert b.loop_steps_per_launch() == 1
        pairs, triples, low = _drive(a, b, grid, block, ct.PAIR_LAYOUTS,
                                     lambda lo, hi: ct.pair_launches(lo, hi, block),
                                     resident=False)
        assert a.resident_launches() == (0, 0)
        print(f"{H} x {W} block {block}: {len(pairs)} pairs, {len(triples)} of "
              f"{81 * (block - 1)} triples inside pair launches, non-zero share >= {low:.3f}")
        assert len(pairs) == 144
        assert len(triples) >= MIN_TRIPLES * 81 * (block - 1)
        assert {r for _, _, r in triples} == set(range(block - 1))


# (bounds, RESIDENT_HALO, SHARD_LAG, RESIDENT_TILE_COLS, steps per launch, tile columns):
#   halo 6: in-kernel power-of-two block starts, a rebase at every exchange
#   lag 1: lagged block starts (e = 64: the 312-row shard's depth)
#   tile columns 3: transposed tiles on the 512-row views of two 256-row shards
SHARD_CASES = [((0, 200, 512), 6, 0, 0, 6, None),
               ((0, 200, 512), 0, 1, 0, 64, None),
               ((0, 256, 512), 0, 0, 3, 128, 3)]


@pytest.mark.parametrize("bounds,halo,lag,tiling,e_want,cols", SHARD_CASES,
                         ids=["halo6", "lagged", "transposed"])
def test_resident_shards_cover_every_pair(pp2, bounds, halo, lag, tiling, e_want, cols):
    """test_gpu_shards.py's _resident_shard_run protocol on block 8's segments
    SHARD_SEGMENTS against the unsharded launch-per-step grid: J and A bit for
    bit, beliefs rel 1e-5 above the FTZ floor (the order of the normalising
    sum differs: per-shard sums, then a sum over shards).

    The lagged case found a range gap: a launch's first lagged block start
    (t = depth) applied no shift, so the first 2 * depth steps of a launch
    decayed on the 2^96 of its first step alone.  After the 26-step launch of
    segment 0 (P(z) ~ 1e-2 per step) 23 of the 524288 beliefs, 5e-27 to 1e-21,
    were off by up to 6.2e-2 relative and 6 more cells had flushed to zero;
    the waited scheme (lag 0, same e) had none.  k_loop_resident now shifts by
    120 - ilogb(2^96) = 24 there (pp2_resident.hip), and the case passes with
    no cell flushed that the reference keeps."""
    from path_planning_2d_amd import synthetic as S
    P = pp2
    grid = S.synth_grid(512, 1024, 7)
    goal = S.synth_goal(grid)
    free = grid.reshape(-1) == 0
    b0 = S.uniform_belief(grid)
    segs = ct.segments(8)
    with P.GridContext(grid, goal, gamma=float(GAMMA)) as ref, \
            P.ShardGroup(grid, goal, bounds, gamma=float(GAMMA)) as grp:
        ref.model_generate()
        grp.model_generate()
        assert ref.model_dict_info()[1] and all(s.model_dict_info()[1] for s in grp.shards)
        ref.set_tuning(ref.TUNE_RESIDENT, 0)
        ref.set_tuning(ref.TUNE_STEP_PAIRS, 0)
        assert ref.loop_steps_per_launch() == 1
        if halo:
            grp.set_tuning(P.GridContext.TUNE_RESIDENT_HALO, halo)
        if tiling:
            grp.set_tuning(P.GridContext.TUNE_RESIDENT_TILE_COLS, tiling)
        if lag:
            grp.set_tuning(P.GridContext.TUNE_SHARD_LAG, lag)
        e = min(grp.loop_steps_per_launch())
        assert e == e_want, grp.loop_steps_per_launch()
        if cols:
            assert [s.resident_tiling()[2] for s in grp.shards] == [cols] * len(grp.shards)
        for c in (ref, grp):
            c.mdp_reset()
        pairs, launches, low = set(), 0, 1.0
        for r in ct.SHARD_SEGMENTS:
            us, zs = segs[r]
            for c in (ref, grp):
                c.belief_set(b0)
            for (lo, hi), _ in ct.chunks(us.size, "ab"[r % 2], r):
                ref.loop_run(us[lo:hi], zs[lo:hi])
                grp.loop_run(us[lo:hi], zs[lo:hi])
                ran = ct.shard_launches(lo, hi, e)
                pairs |= ct.coverage(us, zs, ran, 8)[0]
                launches += len(ran)
                what = _where(8, "ab"[r % 2], r, lo, hi, us, zs)
                for s in grp.shards:
                    assert s.resident_launches()[0] == launches, what
                    assert s.resident_status()[0] == 0, f"a resident launch fell back: {what}"
                assert ref.resident_launches() == (0, 0)
                Jr, Ar = ref.mdp_get()
                Jg, Ag = grp.mdp_get()
                np.testing.assert_array_equal(Jg.view(np.uint32), Jr.view(np.uint32),
                                              err_msg=f"J {what}")
                np.testing.assert_array_equal(Ag, Ar, err_msg=f"A {what}")
                assert_rel_close(grp.belief_get(), ref.belief_get(), rel=1e-5,
                                 abs_floor=FTZ_FLOOR, msg=f"belief {what}")
                low = min(low, _nonzero_share(ref.belief_get_raw()[0], free, what))
        print(f"shards {bounds} e {e}: {len(pairs)} pairs inside resident launches, "
              f"non-zero share >= {low:.3f}")
        assert len(pairs) == 144


# ------------------------------------------------- one step against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_steps(name):
    """oracle.belief_update of the golden belief b8 for all 144 (u, z), once
    per map: (raw outputs [9][16], their fp64 sums)."""
    from oracle import oracle as O
    grid = golden_map(name)
    H, W = grid.shape
    m = golden("model", name)
    b8 = golden("belief", name)["b8"]
    want = [[O.belief_update(H, W, m["T"], m["L"], b8, u, z) for z in range(16)]
            for u in range(9)]
    mass = [[O.lib().orc_sum_f64(w.size, w) for w in row] for row in want]
    for row in want:
        for w in row:
            w.setflags(write=False)
    return want, mass


@pytest.mark.parametrize("coded", [1, 0])
@pytest.mark.parametrize("cpt", [1, 4])
@pytest.mark.parametrize("name", ["map_10x10", "sparse_map_100x40"])
def test_belief_kernel_bit_exact_every_pair(pp2, oracle, name, cpt, coded):
    """test_gpu_parity.py's test_belief_kernel_bit_exact_one_step over all
    144 (u, z), on the coded and the dense model: the unnormalised output of
    one belief update is bit-identical to the oracle's."""
    grid = golden_map(name)
    m = golden("model", name)
    b8 = golden("belief", name)["b8"]
    want, mass_want = _oracle_steps(name)
    with pp2.GridContext(grid, tuple(m["goal"]), gamma=float(GAMMA)) as ctx:
        ctx.set_cells_per_lane(cpt)
        ctx.model_generate()
        ctx.set_tuning(ctx.TUNE_CODED_MODEL, coded)
        ctx.belief_set(b8)
        # (the coded kernels run four cells per lane; other widths are dense)
        assert ctx.model_dict_info()[0] > 0
        assert ctx.model_dict_info()[1] == bool(coded and cpt == 4)
        for u in range(9):
            for z in range(16):
                ctx.belief_set(b8)
                ctx.belief_update(u, z)
                raw, mass = ctx.belief_get_raw()
                assert np.count_nonzero(want[u][z]) > 0
                np.testing.assert_array_equal(raw, want[u][z], err_msg=f"u {u} z {z}")
                assert_rel_close(mass, mass_want[u][z], rel=2e-6, msg=f"mass u {u} z {z}")
