"""CPU: the contract of tests/covering_trajectory.py, and that the launch
layouts of tests/test_gpu_loop_coverage.py put that coverage inside launches
(the GPU tests assert the same figures from the launches they really ran;
here they are known before any GPU run)."""
import numpy as np
import pytest

import covering_trajectory as ct

BLOCKS = (1, 2, 3, 4, 5, 8)
ALL_PAIRS = {(u, z) for u in range(9) for z in range(16)}


def _all_triples(d, phases=None):
    return {(u, v, r) for u in range(9) for v in range(9)
            for r in (range(d) if phases is None else phases)}


def _covered(d, layouts, launches_of):
    pairs, triples = set(), set()
    for layout in layouts:
        for r, (us, zs) in enumerate(ct.segments(d)):
            for (lo, hi), _ in ct.layout_chunks(us.size, layout, d, r):
                p, t = ct.coverage(us, zs, launches_of(lo, hi), d)
                pairs |= p
                triples |= t
    return pairs, triples


def test_de_bruijn_holds_every_ordered_pair_once():
    cyc = ct.de_bruijn(9, 2)
    assert len(cyc) == 81 and set(cyc) == set(range(9))
    assert len({(cyc[i], cyc[(i + 1) % 81]) for i in range(81)}) == 81


@pytest.mark.parametrize("d", BLOCKS)
def test_segments_cover_pairs_and_transitions_at_every_phase(d):
    segs = ct.segments(d)
    pairs, triples = set(), set()
    for us, zs in segs:
        assert us.dtype == np.uint8 and zs.dtype == np.uint8 and us.shape == zs.shape
        assert us.ndim == 1 and ct.CUT <= us.size <= ct.MAX_SEGMENT <= 90
        assert us.max() <= 8 and zs.max() <= 15
        p, t = ct.coverage(us, zs, [(0, us.size)], d)
        pairs |= p
        triples |= t
    assert pairs == ALL_PAIRS
    assert triples == _all_triples(d)  # 81 * d
    # the same object every time: a reference shared by the tests stays unchanged
    again = ct.segments(d)
    assert all(a[0] is b[0] and not a[0].flags.writeable and not a[1].flags.writeable
               for a, b in zip(segs, again))


def test_segment_sizes_of_the_construction():
    """164 / 249 / 684 steps of the uncut lines, plus the symbol the two
    halves of a line share and the stay actions before the second half."""
    for d, uncut in ((1, 164), (3, 249), (8, 684)):
        lines = max(d, 2)
        extra = sum(1 + (r + ct.CUT) % d for r in range(lines))
        assert sum(us.size for us, _ in ct.segments(d)) == uncut + extra
        assert len(ct.segments(d)) == 2 * lines


@pytest.mark.parametrize("layout", ["a", "b"])
@pytest.mark.parametrize("n", range(41, 50))
def test_chunks_partition_the_segment(n, layout):
    for r in range(16):
        ch = ct.chunks(n, layout, r)
        assert ch[0][0][0] == 0 and ch[-1][0][1] == n
        assert all(a[0][1] == b[0][0] for a, b in zip(ch, ch[1:]))
        assert all(hi > lo for (lo, hi), _ in ch)
        assert ch[-1][1], "the last launch of a segment is compared"
        assert ch[-1][0][1] - ch[-1][0][0] >= 2
        # only a 24-step launch is left unsynchronised, and another one follows it
        assert all(sync or hi - lo == ct.NO_SYNC for (lo, hi), sync in ch)
        lens = [hi - lo for (lo, hi), _ in ch]
        if layout == "a":  # the single-step launch and the long kernel instance
            assert 1 in lens and max(lens) > 24
        else:  # the short instance at its limit, queued back to back
            assert [sync for _, sync in ch].count(False) == 1 and max(lens) == 24
        # no launch boundary in common with the other layout
        other = ct.chunks(n, "b" if layout == "a" else "a", r)
        assert not ({lo for (lo, _), _ in ch} & {lo for (lo, _), _ in other}) - {0}


@pytest.mark.parametrize("d", BLOCKS)
def test_resident_layouts_keep_the_coverage_inside_launches(d):
    pairs, triples = _covered(d, ct.RESIDENT_LAYOUTS, ct.resident_launches)
    assert pairs == ALL_PAIRS
    assert triples == _all_triples(d)
    # launches begin and end at every block phase
    starts, ends = set(), set()
    for layout in ct.RESIDENT_LAYOUTS:
        for r, (us, _) in enumerate(ct.segments(d)):
            for (lo, hi), _ in ct.layout_chunks(us.size, layout, d, r):
                if hi - lo >= 2:
                    starts.add(lo % d)
                    ends.add(hi % d)
    assert starts == set(range(d)) and ends == set(range(d))


@pytest.mark.parametrize("d", [2, 3, 4, 5, 8])
def test_pair_layouts_keep_the_coverage_inside_launches(d):
    """A pair launch never spans a block start, so the triples it can hold
    are those with t % d <= d - 2: 81 * (d - 1)."""
    pairs, triples = _covered(d, ct.PAIR_LAYOUTS, lambda lo, hi: ct.pair_launches(lo, hi, d))
    assert pairs == ALL_PAIRS
    can = _all_triples(d, range(d - 1))
    assert triples <= can
    assert len(triples) >= 0.95 * len(can)
    assert {r for _, _, r in triples} == set(range(d - 1))


def test_pair_launches_follow_the_block():
    assert ct.pair_launches(0, 8, 8) == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert ct.pair_launches(1, 9, 8) == [(1, 3), (3, 5), (5, 7)]  # steps 7 and 8 alone
    assert ct.pair_launches(0, 7, 5) == [(0, 2), (2, 4), (5, 7)]
    assert ct.pair_launches(3, 4, 8) == []
    assert ct.shard_launches(0, 14, 6) == [(0, 6), (6, 12), (12, 14)]
    assert ct.shard_launches(5, 6, 6) == [] and ct.resident_launches(5, 6) == []


def test_shard_segments_hold_every_pair():
    """The row-shard case runs six of block 8's segments, alternating the
    layouts: all 144 pairs inside resident launches, whatever the halo block."""
    segs = ct.segments(8)
    for e in (6, 64, 128):
        pairs = set()
        for r in ct.SHARD_SEGMENTS:
            us, zs = segs[r]
            for (lo, hi), _ in ct.chunks(us.size, "ab"[r % 2], r):
                pairs |= ct.coverage(us, zs, ct.shard_launches(lo, hi, e), 8)[0]
        assert pairs == ALL_PAIRS, e
