"""Grid shapes, root beliefs and case lists of the QV-tree planner's shape
tests, shared by test_planner_shapes_cpu.py, test_gpu_planner_shapes.py and
test_gpu_planner_switches.py (with planner_switch_child.py), and the table of
the library's environment switches (SWITCHES).  Everything here is a pure
function of the case.

The planner's host side (csrc/pp2_tree.cpp) and the chain sets it launches
(csrc/pp2_fchain.hip, csrc/pp2_pbvi_host.hip) pick kernels and scratch
layouts by the cell count n = H * W and the width W.  The constants below
restate the limits they branch on; test_planner_shapes_cpu.py reads the same
constants out of the sources and holds every table row to the relation it is
there for, so a changed constant fails there instead of silently moving a
shape to the other side of its limit.
"""
import functools

import numpy as np

GAMMA = np.float32(0.95)

# name: (value, source file under path_planning_2d_amd/csrc, regex whose
# group 1 is the value in that file)
LIMITS = {
    # grids up to this many cells run the reference-order sums as walked
    # chains (pp2_tree.cpp:98, p->seq at :1497)
    "kSeqChainMax": (8192, "pp2_tree.cpp",
                     r"constexpr long long kSeqChainMax = (\d+);"),
    # k_chain_walk's LDS holds walk_cap(n) terms, n <= kWalkMax
    # (pp2_pbvi_host.hip:876)
    "kWalkMax": (8192, "pp2_pbvi_host.hip", r"constexpr int kWalkMax = (\d+);"),
    # d_sub (every 16th running sum) exists up to this many cells
    # (pp2_tree.cpp:1562); above it k_tree_sample searches the whole cdf
    "kSubCellsMax": (65536, "pp2_tree.cpp",
                     r"p->n <= (\d+) && hipMalloc\(&p->d_sub"),
    # 16-cell running-sum ends k_tree_sample holds in LDS (pp2_fchain.hip:1660)
    "kSampleSub": (4096, "pp2_fchain.hip", r"constexpr int kSampleSub = (\d+);"),
    # cells per chain-set chunk (pp2_fchain.hip:46; fc_chunks,
    # pp2_pbvi_internal.h:142)
    "kFcChunk": (256, "pp2_fchain.hip", r"constexpr int kFcChunk = (\d+);"),
    # chunk entries k_fc_walk holds in LDS; longer chains go to k_fc_drive
    # (pp2_fchain.hip:1173, launch_set at :2647)
    "kWkEntries": (1024, "pp2_fchain.hip", r"constexpr int kWkEntries = (\d+);"),
    # fx_fits: n <= kFxC * kFxThreads (pp2_fchain.hip:1975, :1899, :2714)
    "kFxC": (64, "pp2_fchain.hip", r"constexpr int kFxC = (\d+);"),
    "kFxThreads": (1024, "pp2_fchain.hip", r"constexpr int kFxThreads = (\d+);"),
}
K = {k: v[0] for k, v in LIMITS.items()}


def fc_chunks(n):
    return (n + K["kFcChunk"] - 1) // K["kFcChunk"]


def nsub(n):
    return (n + 15) // 16


def fx_fits(n):
    return 0 < n <= K["kFxC"] * K["kFxThreads"]


def branches(n, W):
    """The planner branches a grid of n cells takes by the code's own
    conditions, with no environment switch set."""
    return {
        "walked_chains": n <= K["kSeqChainMax"],            # p->seq
        "d_sub": n <= K["kSubCellsMax"],                    # two-level sample search
        "fx_fits": fx_fits(n),
        "fc_walk": fc_chunks(n) <= K["kWkEntries"],         # else k_fc_drive
        "ragged_sub_block": n % 16 != 0,
        "padded_plane_rows": W % 4 != 0,
    }


# (H, W, seed of synthetic.synth_grid): what each row pins is in SHAPE_NOTES
# and asserted in test_planner_shapes_cpu.py::test_shape_table_straddles_limits.
# Any seed serves whose grid has a goal, three free cells and a free cell in
# its last 16-cell block (test_grids_are_usable) -- with one more condition
# at 257x257, where the root's two best actions under the uniform belief lie
# within rel 2e-5 .. 6e-5 of each other for seeds 1, 2 and 5 (the CPU
# oracle's two arithmetics choose different actions for seed 5); seed 4
# separates them by 3e-4, thirty times the default-order bound of 1e-5
# (test_one_expansion_tree_is_arithmetic_independent).
SHAPES = [
    (1, 7, 1),
    (5, 1, 6),
    (3, 3, 3),
    (33, 65, 4),
    (64, 128, 3),
    (63, 131, 1),
    (255, 257, 2),
    (257, 257, 4),
    (513, 515, 2),
]
SHAPE_NOTES = {
    (1, 7): "one row: n < 16 < 64, nsub 1, no y-neighbours",
    (5, 1): "one column, W 1: every x-neighbour off grid, s2 arithmetic with W 1",
    (3, 3): "smallest grid with an interior cell",
    (33, 65): "walked chains; W%4 1, n%16 1, n%64 33, n%256 97",
    (64, 128): "n == kSeqChainMax == kWalkMax: the last size on k_chain_walk",
    (63, 131): "first sizes on the chain sets; W%4 3, n%16 13 (ragged sub block), n%256 61",
    (255, 257): "nsub == kSampleSub with a ragged last block; W%4 1; fx_fits still true",
    (257, 257): "n > 65536: no d_sub, plain binary search; fx_fits false",
    (513, 515): "fc_chunks 1033 > kWkEntries: k_fc_drive by the planner's own choice",
}
_SEED = {(H, W): s for H, W, s in SHAPES}
LARGEST = (513, 515)
SECOND_LARGEST = (257, 257)


def shape_id(hw):
    return f"{hw[0]}x{hw[1]}"


@functools.lru_cache(maxsize=None)
def grid_of(H, W):
    from path_planning_2d_amd import synthetic as S
    g = S.synth_grid(H, W, _SEED[(H, W)])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def goal_of(H, W):
    from path_planning_2d_amd import synthetic as S
    return S.synth_goal(grid_of(H, W))


@functools.lru_cache(maxsize=None)
def zs_of(H, W, steps):
    """The seeded observations of the following plan steps."""
    from path_planning_2d_amd import synthetic as S
    _, zs, _ = S.synth_trajectory(grid_of(H, W), steps, seed=5)
    return tuple(int(z) for z in zs)


# ---------------------------------------------------------------- root beliefs
def last_free_cell(grid):
    return int(np.nonzero(grid.reshape(-1) == 0)[0][-1])


def uniform(grid):
    from path_planning_2d_amd import synthetic as S
    return S.uniform_belief(grid)


def delta_last(grid):
    """All mass on the last free cell: every draw lands in the last 16-cell
    block of the cdf (the ragged one where n % 16 != 0 and the grid's last
    cells are free or follow it closely)."""
    b = np.zeros(grid.size, np.float32)
    b[last_free_cell(grid)] = 1.0
    return b


SHORT_MASS_TAIL = 40


def short_mass(grid):
    """A normalised seeded belief over the free cells times exactly 0.75 (a
    power-of-two fraction: every cell's product is exact), so the fp32
    running sum ends near 0.75 and about a quarter of the draws r in [0, 1)
    run off the cdf into the sampler's clamp ("the last cell with mass",
    pp2_tree.cpp sample_observations / k_tree_sample, and forward_sampling of
    oracle/pp2_oracle_tree.c).  Both sides take the root belief as given.
    The last 40 cells hold no mass: the clamp has to walk back over more than
    two 16-cell blocks of equal running sums, to a cell that is not n - 1."""
    rng = np.random.default_rng(1000 + grid.size)
    b = rng.random(grid.size) * (grid.reshape(-1) == 0)
    b[grid.size - SHORT_MASS_TAIL:] = 0.0
    b = (b / b.sum()).astype(np.float32)
    return (b * np.float32(0.75)).astype(np.float32)


BELIEFS = {"uniform": uniform, "delta_last": delta_last, "short_mass": short_mass}


@functools.lru_cache(maxsize=None)
def belief_of(H, W, kind):
    b = BELIEFS[kind](grid_of(H, W))
    b.setflags(write=False)
    return b


def running_sum_end(b):
    """The last value of the sequential fp32 prefix sum (the sampling cdf)."""
    return np.cumsum(np.asarray(b, np.float32), dtype=np.float32)[-1]


# ---------------------------------------------------------------- PBVI leaves
PBVI_S = 37


@functools.lru_cache(maxsize=None)
def pbvi_of(H, W):
    """Hand-made PBVI-like alpha vectors [S = 37, n] and actions, so that
    lower_bound_mode 1 runs without a PBVI solve (ctx.pbvi_set on the
    device, Planner.set_pbvi on the oracle, rand_skip 0).  Every entry lies
    in [-70, -40), below every FIB alpha the tests use: rewards are >= -2, so
    after at most 40 sweeps from zero an alpha is >= -2 (1 - gamma^40) /
    (1 - gamma) > -34.9 (asserted by the CPU test) -- as a lower bound lies
    below the upper one.  Row 5 is mixed-sign: every 97th cell holds a value
    in [0, 5)."""
    n = H * W
    rng = np.random.default_rng(5 + n)
    al = rng.uniform(-70, -40, (PBVI_S, n)).astype(np.float32)
    pos = np.arange(3, n, 97)
    al[5, pos] = rng.uniform(0, 5, pos.size).astype(np.float32)
    act = rng.integers(0, 9, PBVI_S).astype(np.uint8)
    al.setflags(write=False)
    act.setflags(write=False)
    return al, act


TIES_ROWS = tuple(range(8, 20))
TIES_ULP = np.float32(2.0 ** -18)  # one ulp of an fp32 in (-64, -32]
TIES_STEPS = 3


@functools.lru_cache(maxsize=None)
def pbvi_ties_of(H, W):
    """pbvi_of with rows 8 .. 19 replaced by a near-tied best group: one base
    row with entries in [-40, -38) -- above every other row in every cell, so
    the group holds the maximum, and still below the FIB alphas (> -34.9) --
    moved in every cell by a seeded -3 .. 3 ulps of its own per row (exact:
    all stay inside one binade).  The rows' true dots with a belief differ by
    a fraction of an ulp of an entry, far less than one rounding of the fp32
    sum, while every fp32 evaluation of a row rounds along a path of its own:
    which row comes out highest is rounding noise, different noise for the
    exact sequential chains and for an approximate product (PP2_PBVI_FCHAIN's
    split-x GEMM), and the values they give differ by ulps of the sum.  (Not
    k ulps down in every cell: fp32 products and sums are monotone, so both
    evaluations would agree on the cell-wise highest row.)  A candidate bound
    that is not rigorous keeps the approximate maximum's row and loses the
    exact one (test_planner_shapes_cpu.py::test_near_tied_alphas)."""
    n = H * W
    al, act = pbvi_of(H, W)
    al = al.copy()
    rng = np.random.default_rng(77 + n)
    lo = np.float32(-40) + TIES_STEPS * TIES_ULP
    hi = np.float32(-38) - (TIES_STEPS + 1) * TIES_ULP
    base = np.clip(rng.uniform(-40, -38, n).astype(np.float32), lo, hi)
    for row in TIES_ROWS:
        k = rng.integers(-TIES_STEPS, TIES_STEPS + 1, n).astype(np.float32)
        al[row] = base + k * TIES_ULP
    al.setflags(write=False)
    return al, act


def pbvi_alphas(H, W, sw):
    """The PBVI alpha vectors of a case: pbvi_of, or with the switch
    "pbvi_ties" pbvi_ties_of."""
    return pbvi_ties_of(H, W) if sw.get("pbvi_ties") else pbvi_of(H, W)


# ---------------------------------------------------------------- models
def off_support_model(grid, T):
    """T with a single entry off its action's base-kernel support: the stay
    action (support {4}) of a free cell with a free upper-left neighbour moves
    there with 0.25, the centre weight compensated so the row still sums to
    1.  Returns (T', cell)."""
    H, W = grid.shape
    T = np.array(T, np.float32).reshape(H * W, 9, 9)
    free = grid == 0
    for y in range(H // 2, H):
        for x in range(W // 2, W):
            if free[y, x] and free[y - 1, x - 1]:
                cell = y * W + x
                assert T[cell, 4, 4] == 1.0 and T[cell, 4, 0] == 0.0
                T[cell, 4, 0] = np.float32(0.25)
                T[cell, 4, 4] = np.float32(0.75)
                return T, cell
    raise ValueError("no free cell with a free upper-left neighbour")


# ---------------------------------------------------------------- case lists
MAX_DEPTH, MAX_ITER = 3, 15
ALL = [(H, W) for H, W, _ in SHAPES]

# reference order (bit for bit): (H, W, belief, lower_bound_mode, following
# steps, switches).  switches: environment variables of the planner, plus
# "fc_walk" (pp2_debug_fc_walk's argument), "coded" (TUNE_CODED_MODEL), "cpt"
# (pp2_set_cells_per_lane), "off_support" (upload off_support_model) and
# "pbvi_ties" (pbvi_ties_of for pbvi_of).
REF_CASES = []
for _hw in ALL:
    REF_CASES.append((*_hw, "uniform", 0, 1 if _hw == LARGEST else 3, {}))
for _kind in ("delta_last", "short_mass"):
    for _hw in ((63, 131), (255, 257), (257, 257)):
        REF_CASES.append((*_hw, _kind, 0, 2, {}))
for _hw in ((5, 1), (33, 65), (63, 131), (257, 257)):
    REF_CASES.append((*_hw, "uniform", 1, 2, {}))
for _hw in ((1, 7), (5, 1), (3, 3), (33, 65), (64, 128)):
    REF_CASES.append((*_hw, "uniform", 0, 3, {"PP2_SEQ_CHAIN_MAX": "0"}))
for _hw in ((33, 65), (64, 128)):
    REF_CASES.append((*_hw, "uniform", 0, 3, {"PP2_CHAIN_WALK": "2"}))
for _hw in ((63, 131), (255, 257)):
    REF_CASES.append((*_hw, "uniform", 0, 3, {"PP2_FX": "1"}))
REF_CASES.append((33, 65, "uniform", 0, 3, {"PP2_FX": "1", "PP2_SEQ_CHAIN_MAX": "0"}))
REF_CASES.append((63, 131, "uniform", 0, 3, {"fc_walk": 0}))
for _hw in ((33, 65), (63, 131)):
    REF_CASES.append((*_hw, "uniform", 0, 3, {"coded": 0}))
# (TUNE_CODED_MODEL 0 leaves the verified-sparse dictionary in place, and with
# it k_tree_pred<true>, pp2_tree.cpp tree_sparse_t: the full 9-tap form runs
# for the off-support model only -- on the walked chains and the chain sets)
for _hw in ((33, 65), (63, 131)):
    REF_CASES.append((*_hw, "uniform", 0, 3, {"off_support": 1}))
# (below 4 cells per lane no coded model is active, whatever TUNE_CODED_MODEL
# says: tree_sparse_t and the planner's host caches on such a context --
# tuning_cases.TUNING)
REF_CASES.append((33, 65, "uniform", 0, 3, {"cpt": 1}))
REF_CASES.append((63, 131, "uniform", 0, 3, {"cpt": 2}))

# default order (rel 1e-5 against the fp64-accumulating oracle): step 0 with
# ONE expansion -- with more, the next node to expand is a comparison of
# near-tied sums that the arithmetic may move; with one there is no such
# choice, and both sides sample from the host's sequential fp32 cdf.
DEFAULT_CASES = [(*_hw, _kind, _lb) for _hw in ALL if _hw != LARGEST
                 for _kind in ("uniform", "delta_last") for _lb in (0, 1)]


# ---------------------------------------------------------------- switches
# Every environment variable the library reads (getenv("PP2_...") in
# path_planning_2d_amd/csrc; test_planner_shapes_cpu.py::
# test_switch_table_is_complete collects the names from the sources and holds
# this table to them).  Per variable:
#   default  the value that means what an unset variable means
#   flips    the first characters the source compares against to leave the
#            default, or "int" where it parses an integer
#   cached   "process" (read once into a global or a function-local static:
#            only a fresh process sees another value), "planner" (read by
#            pp2_planner_create) or "call" (read by every launch)
#   case     the id of a SWITCH_CASES entry that holds the non-default value
#            to the oracle, and / or
#   tests    existing tests that set it ("file::test", under tests/)
#   exempt   instead of both: why no case is needed
_SHAPES_TEST = "test_gpu_planner_shapes.py::test_reference_order_bit_exact"
_PLANNER_TEST = "test_gpu_planner.py::test_planner_reference_order_bit_exact"
SWITCHES = {
    # pp2_tree.cpp, pp2_planner_create
    "PP2_CDF_SKIP": dict(default="1", flips="0", cached="planner",
                         tests=["test_gpu_planner.py::test_planner_cdf_zero_block_skip_exact"]),
    "PP2_SEQ_CHAIN_MAX": dict(default=str(K["kSeqChainMax"]), flips="int", cached="planner",
                              tests=[_SHAPES_TEST]),
    "PP2_FX": dict(default="0", flips="1", cached="planner", tests=[_SHAPES_TEST]),
    "PP2_FX_STAMPS": dict(default="0", flips="1", cached="planner",
                          exempt="only allocates the fused sets' time-stamp buffer"),
    "PP2_PBVI_FCHAIN": dict(default="0", flips="1", cached="planner",
                            case="63x131-uniform-pbvi-2-pbvi_fchain1-pbvi_stats1"),
    "PP2_PBVI_STATS": dict(default="0", flips="1", cached="planner",
                           exempt="only allocates the candidate counter's host copy"),
    "PP2_PLAN_TIMING": dict(default="0", flips="1", cached="planner",
                            case="63x131-uniform-pbvi-2-plan_events1-plan_timing1"),
    "PP2_PLAN_EVENTS": dict(default="0", flips="1", cached="planner",
                            case="63x131-uniform-pbvi-2-plan_events1-plan_timing1"),
    "PP2_SPIN_WAIT": dict(default="1", flips="0", cached="planner",
                          case="63x131-uniform-pbvi-2-spin_wait0"),
    "PP2_FIB_CANDS": dict(default="0", flips="1", cached="planner", tests=[_PLANNER_TEST]),
    "PP2_FIB_UNIT": dict(default="1", flips="0", cached="planner",
                         case="63x131-uniform-pbvi-2-fib_unit0"),
    "PP2_HOST_JOIN": dict(default="1", flips="0", cached="planner",
                          case="63x131-uniform-pbvi-2-host_join0"),
    "PP2_KIDS_FIRST": dict(default="0", flips="1", cached="planner",
                           case="63x131-uniform-pbvi-2-kids_first1"),
    "PP2_ROW_FIRST": dict(default="0", flips="1", cached="planner", tests=[_PLANNER_TEST],
                          case="63x131-uniform-pbvi-2-kids_first1-row_first1"),
    # pp2_fchain.hip: globals and one function-local static
    "PP2_FC_SUMTAB": dict(default="0", flips="1", cached="process",
                          case="63x131-uniform-fib-2-fc_sumtab1"),
    "PP2_FC_K9WAVE": dict(default="0", flips="1", cached="process",
                          case="63x131-uniform-fib-2-fc_k9wave1"),
    "PP2_FC_KEPT_GY": dict(default="0", flips="int", cached="process",
                           case="63x131-uniform-fib-2-fc_kept_gy6"),
    "PP2_FC_PLAN9": dict(default="0", flips="1", cached="process",
                         case="63x131-uniform-fib-2-fc_plan91"),
    "PP2_FC_PLAN": dict(default="1", flips="0", cached="process",
                        case="63x131-uniform-fib-2-fc_plan0"),
    # (covered through pp2_debug_fc_walk, which writes the cached value:
    # REF_CASES' {"fc_walk": 0})
    "PP2_FC_WALK": dict(default="1", flips="0", cached="process", tests=[_SHAPES_TEST]),
    # pp2_pbvi_host.hip, every launch
    "PP2_PAIR_DOT": dict(default="3", flips="int", cached="call",
                         tests=["test_gpu_pbvi.py::test_evaluate_dot_shapes_bit_exact"]),
    "PP2_PAIR_SEQ": dict(default="1", flips="0", cached="call",
                         case="63x131-uniform-pbvi-2-pair_seq0"),
    # (unset and "1": k_chain_walk; "2": k_chain_walk2; "0": launch_pair_seq
    # and the sequential cdf)
    "PP2_CHAIN_WALK": dict(default="1", flips="02", cached="call", tests=[_SHAPES_TEST],
                           case="64x128-uniform-fib-2-chain_walk0"),
    # pp2_kernels.hip, pp2_rollout_dev.hip, every launch
    # (unset or empty: the kernel is chosen by the block count; "1" forces the
    # LDS kernel, any other character the dense one)
    "PP2_FIB_LDS": dict(default="", flips="1", cached="call",
                        tests=["test_gpu_parity.py::test_fib_lds_equals_dense_geometries",
                               "test_gpu_ref_pin.py::test_fib_sweeps"]),
    "PP2_BAND_DMA16": dict(default="1", flips="0", cached="call",
                           tests=["test_gpu_rollout_exact.py::test_rollout_exact_dma4_staging"]),
}
EXEMPT_ALLOWED = {"PP2_FX_STAMPS", "PP2_PBVI_STATS"}


def differs_from_default(name, value):
    """value leaves the default of SWITCHES[name] by what the source looks at:
    the first character, or the parsed integer."""
    row = SWITCHES[name]
    if row["flips"] == "int":
        return int(value) != int(row["default"])
    return value[:1] in row["flips"] and value[:1] != row["default"][:1]


# Reference-order cases of the switches no other test sets, in REF_CASES'
# format and held the same way (planner_shape_run.run_reference_order).  The
# shapes are the smallest of the table at which these paths still differ:
#   63x131                    on the chain sets by the planner's own choice; 33
#                             chunks = 9 segments with a ragged last one
#   33x65, SEQ_CHAIN_MAX=0    9 chunks, 3 segments, W%4 n%16 n%256 ragged
#   1x7, SEQ_CHAIN_MAX=0      one chunk, one segment, no predecessor
#   64x128                    the last size on the walked chains (CHAIN_WALK)
# The root expansion under the uniform belief keeps KEPT_CHILDREN of the 144
# children (the CPU oracle; test_switch_shapes_keep_enough_children): at
# 33x65 and 63x131 more than the kFcDevGroups = 64 groups dispatched for a
# device group list, so its loop wraps, and with PP2_FC_KEPT_GY 1 and 6 the
# last pass is ragged (91 % 6 = 1, 100 % 6 = 4).
KEPT_CHILDREN = {(1, 7): 48, (33, 65): 91, (63, 131): 100}
FC_DEV_GROUPS = 64  # pp2_fchain.hip kFcDevGroups
_SEQ0 = {"PP2_SEQ_CHAIN_MAX": "0"}
_CHAINS = ((63, 131, {}), (33, 65, _SEQ0))  # both on the chain sets


def _case(H, W, lb, steps, *sws):
    sw = {}
    for s in sws:
        sw.update(s)
    return (H, W, "uniform", lb, steps, sw)


SWITCH_CASES = []
# read per planner or per call: set in the test's own process.  lb 1 wherever
# the switch moves launches between the two streams or changes how they join
# (the PBVI dots are the side stream's last and longest work)
for _sw in ({"PP2_FIB_UNIT": "0"},
            {"PP2_KIDS_FIRST": "1"},
            {"PP2_KIDS_FIRST": "1", "PP2_ROW_FIRST": "1"},  # row-first wins
            {"PP2_SPIN_WAIT": "0"},
            {"PP2_PLAN_TIMING": "1", "PP2_PLAN_EVENTS": "1"}):
    for _H, _W, _s in _CHAINS:
        SWITCH_CASES.append(_case(_H, _W, 1, 2, _s, _sw))
for _lb in (0, 1):
    for _H, _W, _s in _CHAINS:
        SWITCH_CASES.append(_case(_H, _W, _lb, 2, _s, {"PP2_HOST_JOIN": "0"}))
# (PP2_PBVI_STATS=1 beside it: the candidate counter proves that a candidate
# set ran)
PBVI_FCHAIN = {"PP2_PBVI_FCHAIN": "1", "PP2_PBVI_STATS": "1"}
for _H, _W, _s in ((5, 1, {}), (33, 65, {}), (33, 65, _SEQ0), (63, 131, {})):
    SWITCH_CASES.append(_case(_H, _W, 1, 2, _s, PBVI_FCHAIN))
# and with a near-tied best group of alphas (pbvi_ties_of), which only a
# rigorous candidate bound survives -- the bound's radius c_rel is the
# planner's own (pp2_tree.cpp ref_pbvi_bounds), so no kernel-level test
# reaches it; the default leaf dots on the same alphas beside it
TIES = {"pbvi_ties": 1}
for _H, _W, _s in ((5, 1, {}), (33, 65, {}), (33, 65, _SEQ0), (63, 131, {})):
    SWITCH_CASES.append(_case(_H, _W, 1, 2, _s, PBVI_FCHAIN, TIES))
for _hw in ((33, 65), (63, 131)):
    SWITCH_CASES.append(_case(*_hw, 1, 2, TIES))
for _hw in ((33, 65), (63, 131)):  # n >= 1024: the variable decides
    SWITCH_CASES.append(_case(*_hw, 1, 2, {"PP2_PAIR_SEQ": "0"}))
for _hw in ((33, 65), (64, 128)):
    SWITCH_CASES.append(_case(*_hw, 0, 2, {"PP2_CHAIN_WALK": "0"}))
INPROCESS_SWITCH_CASES = list(SWITCH_CASES)

# cached per process: one child process per switch set, three cases each
CHILD_SETS = [
    {"PP2_FC_SUMTAB": "1"},
    {"PP2_FC_K9WAVE": "1"},
    {"PP2_FC_K9WAVE": "1", "PP2_FIB_UNIT": "0"},
    {"PP2_FC_PLAN9": "1"},
    {"PP2_FC_PLAN9": "1", "PP2_FC_K9WAVE": "1"},
    {"PP2_FC_KEPT_GY": "1"},
    {"PP2_FC_KEPT_GY": "6"},
    {"PP2_FC_PLAN": "0"},
]


def child_cases(sw):
    return [_case(1, 7, 0, 1, _SEQ0, sw), _case(33, 65, 1, 2, _SEQ0, sw),
            _case(63, 131, 0, 2, sw)]


for _sw in CHILD_SETS:
    SWITCH_CASES.extend(child_cases(_sw))


def switch_set_id(sw):
    return "-".join(f"{k.replace('PP2_', '').lower()}{v}" for k, v in sorted(sw.items()))


def ref_case_id(c):
    H, W, kind, lb, steps, sw = c
    tail = "".join(f"-{k.replace('PP2_', '').lower()}{v}" for k, v in sorted(sw.items()))
    return f"{H}x{W}-{kind}-{'pbvi' if lb else 'fib'}-{steps}{tail}"


def default_case_id(c):
    H, W, kind, lb = c
    return f"{H}x{W}-{kind}-{'pbvi' if lb else 'fib'}"


# ---------------------------------------------------------------- comparisons
def rel_close(a, b, rel=1e-5, atol=1e-6):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= np.maximum(rel * np.abs(b), atol))


SHAPE_KEYS = ("depth", "expansions", "n_root_children", "total_vnodes", "total_qnodes")


def same_tree_shape(gi, oi, where):
    """Depth, expansions, node counts, children, observations and weights of
    two tree snapshots equal."""
    for k in SHAPE_KEYS:
        assert gi[k] == oi[k], f"{where}: {k} {gi[k]} != {oi[k]}"
    n = gi["n_root_children"]
    assert np.array_equal(gi["q_nchildren"][:n], oi["q_nchildren"][:n]), where
    assert np.array_equal(gi["q_depth"][:n], oi["q_depth"][:n]), where
    for a in range(n):
        m = gi["q_nchildren"][a]
        assert np.array_equal(gi["q_obs"][a][:m], oi["q_obs"][a][:m]), where
        assert np.array_equal(gi["q_weight"][a][:m], oi["q_weight"][a][:m]), where


def compare(gi, oi, where, rel=1e-5):
    """Tree shape equal, bounds and rewards within rel (test_gpu_planner.py's
    compare)."""
    same_tree_shape(gi, oi, where)
    n = gi["n_root_children"]
    for a in range(n):
        m = gi["q_nchildren"][a]
        assert rel_close(gi["v_upper_bound"][a][:m], oi["v_upper_bound"][a][:m], rel), where
        assert rel_close(gi["v_lower_bound"][a][:m], oi["v_lower_bound"][a][:m], rel), where
    for k in ("q_upper_bound", "q_lower_bound", "q_reward", "q_heuristic"):
        assert rel_close(gi[k][:n], oi[k][:n], rel), f"{where}: {k}"
    for k in ("root_upper_bound", "root_lower_bound", "root_heuristic"):
        assert rel_close(gi[k], oi[k], rel), f"{where}: {k}"


def compare_exact(gi, oi, where):
    """Every field of the two tree snapshots equal (floats bit for bit)."""
    for k in gi:
        a, b = np.asarray(gi[k]), np.asarray(oi[k])
        if a.dtype.kind == "f":
            a32 = np.atleast_1d(a.astype(np.float32))
            b32 = np.atleast_1d(b.astype(np.float32))
            assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)), \
                f"{where}: {k} {a} != {b}"
        else:
            assert np.array_equal(a, b), f"{where}: {k} {a} != {b}"


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))
