"""A deterministic (u, z) trajectory that covers the fused loop's compile-time
paths, for tests/test_gpu_loop_coverage.py (and, for its own properties,
tests/test_covering_trajectory_cpu.py).

Inside the loop kernels the action u is not data: it selects one of nine
specialisations of the belief gather and the class rows issued ahead of it,
and z selects the row of the likelihood table.  The resident loop moves those
reads across step and block-start boundaries, so a mistake shows as a wrong
table row for one (u_t, u_{t+1}) at one position of a normalisation block.
``synthetic.synth_trajectory`` reaches a fraction of that space (DESIGN.md
"Parity"); this module reaches all of it:

``segments(d)`` -- a list of (us, zs) uint8 arrays for normalisation block d
(1..8).  Every segment is run from a fresh ``belief_set``, which restarts the
block, so step t of a segment is a block start when t % d == 0 and an arrive
step when (t + 1) % d == 0.  Over all segments
  * all 144 pairs (u, z) occur,
  * every ordered transition (u_t, u_{t+1}) occurs with t % d == r for every
    r in range(d): 81 * d triples,
  * no segment is longer than MAX_SEGMENT = 49 steps.

The construction: ``cyc`` is the de Bruijn sequence B(9, 2) (81 symbols, every
ordered pair of actions once, cyclically); line r, r in range(max(d, 2)), is
[4] * (r % d) + cyc + cyc[:1] -- the stay action shifts the cycle through the
block's phases --; and the j-th occurrence of action u, counted across the
segments, observes (7 * j + u) % 16 (7 is a unit modulo 16 and every action
occurs at least 18 times).  A line is run as two segments, cut at the cycle's
transition CUT = 41 (the second starts with the symbol the first ends with,
after as many stay actions as keep every transition at its phase).

Why two: the observations are drawn without regard to the map, P(z_t |
history) is 1e-2 on average and down to 5e-6, and the belief concentrates
until cells flush to zero.  Measured on an MI355X on the launch-per-step path
of the grids of the GPU test: with blocks 3, 5 and 8 at least 97.7 % of the
free cells stay non-zero over a whole uncut 82-to-89-step line, but with block
1 (no 2^96 block scale) a 10 x 1024 grid falls below 85 % at step 73 (66 % at
the end; 84 to 93 % on the other grids), and nowhere below 90 % before step
57.  Bit equality of flushed cells proves nothing, so the lines are cut in
half: the cut segments keep at least 93.6 % (block 1) and 99.9 % (other
blocks) everywhere.

``chunks(n, layout, r)`` -- the launches segment r of n steps is cut into,
with the bookkeeping of what a chunking puts inside one launch
(``resident_launches``, ``pair_launches``, ``shard_launches``) and
``coverage`` of a list of launches.
"""
import functools

import numpy as np

ACTIONS = 9
OBSERVATIONS = 16
CUT = 41
MAX_SEGMENT = 49
NO_SYNC = 24


def de_bruijn(k, n):
    """B(k, n) by the Lyndon-word recursion (Fredricksen, Maiorana)."""
    a = [0] * (k * n)
    out = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return out


@functools.lru_cache(maxsize=None)
def _segments(d):
    if not 1 <= d <= 8:
        raise ValueError(f"normalisation block {d} not in [1, 8]")
    cyc = de_bruijn(ACTIONS, 2)
    line = cyc + cyc[:1]  # 82 symbols, 81 transitions
    seen = [0] * ACTIONS
    out = []
    for r in range(max(d, 2)):
        for s, e in ((0, CUT), (CUT, len(line) - 1)):
            # symbol i of the line is step (r + i) % d of a block, cut or not
            us = [4] * ((r + s) % d) + line[s:e + 1]
            zs = []
            for u in us:
                zs.append((7 * seen[u] + u) % OBSERVATIONS)
                seen[u] += 1
            us, zs = np.array(us, np.uint8), np.array(zs, np.uint8)
            us.setflags(write=False)
            zs.setflags(write=False)
            out.append((us, zs))
    return tuple(out)


def segments(d):
    return list(_segments(d))


# Launch lengths inside a segment, then the rest, as ((lo, hi), synchronize
# and compare after it).
#   "a": even and odd lengths, a one-step run (the single-step launch, not the
#        resident kernel), and a rest of 25 to 33 steps: the long kernel
#        instance (more than kResidentShortSteps = 24 steps);
#   "b": 7 + r % 8 steps, so that over the segments launches begin and end at
#        every phase of a block, then the short instance at its limit of 24
#        steps, not synchronised: queued back to back with the rest.
# No launch boundary of "b" (7..14, 31..38) is one of "a" (2, 5, 6, 16): a
# transition that one layout splits over two launches lies inside a launch of
# the other.  One layout alone loses 4 of a segment's 40: more than the 5 % a
# test may miss.
def chunks(n, layout="a", r=0):
    if not CUT <= n <= MAX_SEGMENT:
        raise ValueError(f"segment of {n} steps")
    lens = {"a": [2, 3, 1, 10], "b": [7 + r % 8, NO_SYNC]}[layout]
    lens = lens + [n - sum(lens)]
    assert lens[-1] >= 2
    out, lo = [], 0
    for m in lens[:-1]:
        out.append(((lo, lo + m), m != NO_SYNC))
        lo += m
    out.append(((lo, n), True))
    return out


def phase_chunks(n, d):
    """Launches that start one step into every block: (1, d - 1) repeated.
    Step pairs never span a block start (the block's first launch carries the
    block scale), so a pair on steps (1, 2), (3, 4), ... of a block needs a
    launch that begins at phase 1."""
    out, lo = [], 0
    while lo < n:
        for m in (1, d - 1):
            m = min(m, n - lo)
            if m:
                # (compared after the launch that follows the single step)
                out.append(((lo, lo + m), m > 1 or lo + m == n))
            lo += m
    return out


# The resident tests run the segments under "a" and again under "b"; the pair
# test adds "phase".
RESIDENT_LAYOUTS = ("a", "b")
PAIR_LAYOUTS = ("a", "phase", "b")


def layout_chunks(n, layout, d, r):
    return phase_chunks(n, d) if layout == "phase" else chunks(n, layout, r)


# The row-shard test (a 512 K-cell grid) runs these segments of block 8 only:
# lines 0, 3 and 4, the cycle at the block's start and three and four steps
# into it.  The observation counter runs through the segments in between, so
# lines 0 and 3 alone hold 122 of the 144 pairs; with a neighbour, all.
SHARD_SEGMENTS = (0, 1, 6, 7, 8, 9)


def resident_launches(lo, hi):
    """The resident launches of an unsharded pp2_loop_run over steps [lo, hi):
    one, unless the run is a single step (the single-step launch)."""
    return [(lo, hi)] if hi - lo >= 2 else []


def pair_launches(lo, hi, d):
    """The two-step launches of pp2_loop_run's launch-per-pair path over steps
    [lo, hi) of a segment (pp2_runtime.cpp loop_run_launches / can_pair): a
    pair whenever the run has two steps left and so has the block."""
    out, t = [], lo
    while t < hi:
        if t + 1 < hi and t % d + 2 <= d:
            out.append((t, t + 2))
            t += 2
        else:
            t += 1
    return out


def shard_launches(lo, hi, e):
    """The resident launches of pp2_shard_group_loop_run over steps [lo, hi):
    halo blocks of up to e steps, per-step launches for a single step."""
    if hi - lo < 2:
        return []
    return [(t, min(t + e, hi)) for t in range(lo, hi, e)]


def coverage(us, zs, launches, d):
    """(pairs, triples) inside ``launches`` of one segment: the (u, z) of
    every step of a launch, and (u_t, u_{t+1}, t % d) for every two
    consecutive steps of the same launch."""
    pairs, triples = set(), set()
    for lo, hi in launches:
        for t in range(lo, hi):
            pairs.add((int(us[t]), int(zs[t])))
            if t + 1 < hi:
                triples.add((int(us[t]), int(us[t + 1]), t % d))
    return pairs, triples
