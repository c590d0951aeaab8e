"""The tuning keys of pp2_set_tuning (TUNING), the sites of the library that
read the two keys which choose a kernel instantiation (SITES), and the shapes
and settings of test_gpu_tuning.py.  The counterpart of SWITCHES in
planner_shape_cases.py: test_tuning_table_cpu.py collects the keys and the
sites from the sources and holds these tables to them, so a new key or a new
launch site that reads c->cpt or c->nt_streams fails there until a row says
which test holds it to a reference.  Everything here is a pure function of
the case.
"""
import numpy as np

import planner_shape_cases as PC

# name: (value, source file under path_planning_2d_amd/csrc, regex whose group
# 1 is the value in that file) -- as planner_shape_cases.LIMITS
LIMITS = {
    # threads per workgroup of every streaming kernel (pp2_device.h)
    "kBlock": (256, "pp2_device.h", r"constexpr int kBlock = (\d+);"),
}
K = {k: v[0] for k, v in LIMITS.items()}


def wp_of(W):
    """Cells per plane row: the width padded to whole 4-cell lanes."""
    return (W + 3) & ~3


def threads(H, W, cpt):
    """Threads a streaming kernel's rows need at cpt cells per lane."""
    return H * (wp_of(W) // cpt)


def blocks(H, W, cpt):
    """cells_grid (pp2_kernels.hip)."""
    return (threads(H, W, cpt) + K["kBlock"] - 1) // K["kBlock"]


# ---------------------------------------------------------------- GPU cases
# (H, W, seed of synthetic.synth_grid), with the seeds of the tables the
# suite already has: test_gpu_parity.py / test_gpu_control.py (1x7, 5x1,
# 97x131) and planner_shape_cases.SHAPES (33x65).  What each pins is
# asserted in test_tuning_table_cpu.py::test_smallest_shapes.
DENSE_SHAPES = [(1, 7, 1), (5, 1, 2), (33, 65, 4), (97, 131, 3)]
DENSE_NOTES = {
    (1, 7): "one row, wp 8",
    (5, 1): "wp 4: one thread a row at 4 cells per lane, two at 2",
    (33, 65): "W%4 1, 561 threads at 4 cells per lane: a block boundary in "
              "mid-row and a ragged last block",
    (97, 131): "W%4 3, 13 blocks at 4 cells per lane, 50 full ones and a last of 4 threads at 1",
}
# (cells per lane, PP2_TUNE_NT_STREAMS, PP2_TUNE_CODED_MODEL).  nt_streams is
# looked at only at 4 cells per lane, and the coded model -- which replaces
# the dense kernels -- is active only there, so both stay at their defaults
# for 2 and 1.
DENSE_SETTINGS = [(4, 1, 0), (4, 0, 0), (2, 1, 1), (1, 1, 1)]
DENSE_STEPS = 3


def dense_id(s):
    cpt, nt, coded = s
    return f"cpt{cpt}-nt{nt}-coded{coded}"


def coded_expected(cpt, coded):
    """What model_dict_info()[1] must say on a generated model."""
    return bool(coded) and cpt == 4


def dense_grid(H, W, seed):
    """(grid, goal) as test_gpu_parity.py::test_model_generation_synthetic."""
    from path_planning_2d_amd import synthetic as S
    grid = S.synth_grid(H, W, seed)
    grid[0, 0] = 0
    return grid, (0, 0)


def spread_belief(grid):
    """A seeded, uneven, normalised belief over the free cells."""
    rng = np.random.default_rng(11 + grid.size)
    b = (rng.random(grid.size) * (grid.reshape(-1) == 0)).astype(np.float32)
    b /= b.sum(dtype=np.float64)
    return b.astype(np.float32)


# reference_order = 0 planner (launch_expand, launch_belief_dots, the tile
# partials, launch_belief / mass_partials at the second step): shapes and
# beliefs of planner_shape_cases, (H, W, belief, lower_bound_mode, cpt)
PLANNER_CPTS = (1, 2, 4)
PLANNER_SHAPES = ((5, 1), (33, 65), (63, 131))
PLANNER_CASES = [(*_hw, _kind, 0, _cpt) for _cpt in PLANNER_CPTS for _hw in PLANNER_SHAPES
                 for _kind in ("uniform", "delta_last")]
PLANNER_CASES += [(33, 65, _kind, 1, _cpt) for _cpt in PLANNER_CPTS
                  for _kind in ("uniform", "delta_last")]


def planner_case_id(c):
    H, W, kind, lb, cpt = c
    return f"{H}x{W}-{kind}-{'pbvi' if lb else 'fib'}-cpt{cpt}"


def skipped_by_half_grid(H, W, kind):
    """Whether the belief's mass lies in rows that a <1> kernel does not
    reach when it is started with the grid of 2 cells per lane (the launch
    sizing test_gpu_tuning.py's planner cases are there for): rows * wp / 2
    threads at wp threads a row cover the first rows // 2 rows."""
    b = PC.belief_of(H, W, kind).reshape(H, W)
    covered = threads(H, W, 2) // wp_of(W)
    return float(b[covered:].sum(dtype=np.float64))


def second_step_observations(info, a):
    """Of a one-expansion tree snapshot and the action a: (the observation of
    the first child that a's expansion kept, the observations it did not
    sample)."""
    m = int(info["q_nchildren"][a])
    kept = [int(z) for z in info["q_obs"][a][:m]]
    return (kept[0] if kept else None), [z for z in range(16) if z not in kept]


def likeliest(oracle, H, W, T, L, b, a, zs):
    """The observation of zs whose unnormalised belief update (the oracle's)
    has the most mass, and that update."""
    ups = [oracle.belief_update(H, W, T, L, b, a, z) for z in zs]
    k = int(np.argmax([u.sum(dtype=np.float64) for u in ups]))
    return zs[k], ups[k]


# ---------------------------------------------------------------- the keys
# One row per PP2_TUNE_* key of include/pp2.h:
#   number   the key's value in pp2.h, core.py and pp2_set_tuning's switch
#   values   the accepted values (a tuple), or for an open range its
#            description, with `range` = (lo, hi) as pp2_set_tuning checks it
#            (hi None: no upper bound, or one that depends on the context)
#   boolean  True where pp2_set_tuning takes any integer as value != 0
#   default  the context's value before any call
#   field    the pp2_ctx member that pp2_set_tuning writes
#   sets     regex of how a test file sets the key (default: the TUNE_ name)
#   held     {value or tuple of values: [(test, what it makes run)]}: for
#            every non-default value (of an open range: the values that tests
#            pass) the tests that hold it to a reference, "file::test" under
#            tests/
#   exempt   instead of held: why nothing needs holding
_T = "test_gpu_tuning.py::"
_DENSE = [_T + "test_dense_belief_update", _T + "test_dense_mdp_sweeps", _T + "test_dense_loop_steps"]
_PLANNER = [_T + "test_default_order_by_cells_per_lane", _T + "test_default_order_second_step"]
_CPT_SETS = r'set_cells_per_lane\(|TUNE_CELLS_PER_LANE|"cpt"'


def _each(tests, what):
    return [(t, what) for t in tests]


TUNING = {
    "PP2_TUNE_CELLS_PER_LANE": dict(
        number=1, values=(1, 2, 4), default=4, field="cpt", sets=_CPT_SETS,
        held={
            1: _each(_DENSE, "k_belief_update<1>, k_mdp_sweep<1,false>, k_loop_step<1,false>")
            + _each(_PLANNER, "k_expand_pred<1>, k_expand_stats<1>, k_belief_dots<1>, "
                              "k_belief_update<1> on 4 * cells_grid(g, 1) partials")
            + [("test_gpu_planner_shapes.py::test_reference_order_bit_exact",
                "tree_sparse_t and the planner's host caches without an active coded model"),
               ("test_gpu_control.py::test_q_bits_invariant", "k_control_q<true> (cpt-independent)")],
            2: _each(_DENSE, "k_belief_update<2>, k_mdp_sweep<2,false>, k_loop_step<2,false>")
            + _each(_PLANNER, "the <1> expansion kernels on their own grid (no <2> exists), "
                              "k_belief_update<2> on 4 * cells_grid(g, 2) partials")
            + [("test_gpu_planner_shapes.py::test_reference_order_bit_exact",
                "tree_sparse_t and the planner's host caches without an active coded model"),
               ("test_gpu_parity.py::test_loop_step_matches_separate_ops", "k_loop_step<2,false>"),
               ("test_gpu_parity.py::test_loop_normalisation_blocks",
                "k_loop_step<2,false> through every normalisation block phase")],
        }),
    # looked at only at 4 cells per lane (launch_mdp_sweep, launch_loop_step)
    # and by launch_control_q, all of them only while the coded model is off
    "PP2_TUNE_NT_STREAMS": dict(
        number=2, values=(0, 1), boolean=True, default=1, field="nt_streams",
        held={0: _each(_DENSE[1:], "k_mdp_sweep<4,false>, k_loop_step<4,false>")
              + [("test_gpu_control.py::test_qmdp_one_hot_is_the_next_sweep",
                  "k_control_q<false>, k_mdp_sweep<4,false>"),
                 ("test_gpu_control.py::test_qmdp_spread_beliefs_against_fp64",
                  "k_control_q<false>")]}),
    # the coded model is active only at 4 cells per lane (gate_coded_active)
    "PP2_TUNE_CODED_MODEL": dict(
        number=3, values=(0, 1), boolean=True, default=1, field="use_coded",
        held={0: _each(_DENSE, "the dense <4, true> kernels")
              + [("test_gpu_loop_coverage.py::test_belief_kernel_bit_exact_every_pair",
                  "k_belief_update<4> for every action / observation pair"),
                 ("test_gpu_planner_shapes.py::test_reference_order_bit_exact",
                  "the planner's caches on the dense model")]}),
    "PP2_TUNE_HALO_DEPTH": dict(
        number=4, values="1 .. the smallest shard's rows, at most 8", range=(1, None),
        default="the largest accepted", field="kdepth", sets=r"set_halo_depth\(|TUNE_HALO_DEPTH",
        held={(1, 3, 8): [("test_gpu_shards.py::test_shards_halo_depths",
                           "extended-domain views 1, 3 and 8 rows deep")]}),
    "PP2_TUNE_COMM_STREAM": dict(
        number=5, values=(0, 1), boolean=True, default=0, field="use_comm_stream",
        held={1: [("test_gpu_shards.py::test_rccl_single_rank_pipeline",
                   "comm_enter / comm_leave hand every RCCL call to the comm stream")]}),
    "PP2_TUNE_NORM_BLOCK": dict(
        number=6, values=tuple(range(1, 9)), range=(1, "kMaxNormBlock"), default=8,
        field="norm_block",
        held={(1, 2, 5): [("test_gpu_parity.py::test_loop_normalisation_blocks",
                           "every phase of blocks of 1, 2 and 5 steps"),
                          ("test_gpu_resident.py::test_resident_equals_single_steps",
                           "the resident loop at blocks of 1 and 5 steps")],
              (3, 4, 6, 7): [("test_gpu_parity.py::test_loop_normalisation_blocks",
                              "the same modulus arithmetic as 2 and 5 (no value is special-cased)")]}),
    "PP2_TUNE_STEP_PAIRS": dict(
        number=7, values=(0, 1, 2), range=(0, 2), default=1, field="step_pairs",
        held={0: [("test_gpu_coded.py::test_step_pairs_equal_single_steps", "single coded steps"),
                  (_DENSE[2], "one k_loop_step launch per step")],
              2: [("test_gpu_shards.py::test_shard_group_step_pairs",
                   "pairs on grids below a tile per CU")]}),
    "PP2_TUNE_RESIDENT": dict(
        number=8, values=(0, 1), range=(0, 1), default=1, field="resident",
        held={0: [("test_gpu_control.py::test_control_after_the_loop", "launch-per-step loop"),
                  (_DENSE[2], "one k_loop_step launch per step")]}),
    "PP2_TUNE_RESIDENT_HALO": dict(
        number=9, values="0 .. the halo allocation", range=(0, None), default=0,
        field="res_halo",
        held={(6,): [("test_gpu_shards.py::test_shard_group_resident_blocks",
                      "resident shard launches of 6 steps")]}),
    "PP2_TUNE_RESIDENT_CUS": dict(
        number=10, values=">= 0 (diagnostic)", range=(0, None), default=0, field="res_cus",
        held={(128,): [("test_gpu_resident.py::test_resident_not_coresident_falls_back_before_launch",
                        "a plan for fewer CUs than the tiles need falls back")]}),
    "PP2_TUNE_RESIDENT_STALL": dict(
        number=11, values=">= -1 (diagnostic)", range=(-1, None), default=-1,
        field="res_stall_tile",
        held={(100,): [("test_gpu_resident.py::test_resident_timeout_reruns_from_intact_inputs",
                        "the re-run of a resident launch that timed out")]}),
    "PP2_TUNE_RESIDENT_TILE_COLS": dict(
        number=12, values=(0, 1, 2, 3), range=(0, 3), default=0, field="res_tc_pref",
        held={1: [("test_gpu_resident.py::test_resident_tiling_switch_same_tile_count",
                   "whole-row tiles")],
              2: [("test_gpu_resident.py::test_resident_2d_tiles_equal_single_steps",
                   "two tile columns")],
              3: [("test_gpu_shards.py::test_shard_group_resident_config4", "transposed tiles")]}),
    "PP2_TUNE_SHARD_LAG": dict(
        number=13, values=(0, 1), range=(0, 1), default=0, field="shard_lag",
        held={1: [("test_gpu_shards.py::test_shard_group_resident_config4",
                   "block starts scaled from the mass one block earlier")]}),
    "PP2_TUNE_COMM_TIMING": dict(
        number=14, values=(0, 1), range=(0, 1), default=0, field="comm_timing",
        held={1: [("test_gpu_shards.py::test_comm_round_timing_single_rank",
                   "timing events around every RCCL round")]}),
    "PP2_TUNE_RESIDENT_MASKED": dict(
        number=15, values=(0, 1), range=(0, 1), default=1, field="res_masked",
        held={0: [("test_gpu_resident_masked.py::test_masked_equals_class_tables_and_single_steps",
                   "the class-table form of the resident loop")]}),
    "PP2_TUNE_MAP_INCREMENTAL": dict(
        number=16, values=(0, 1), range=(0, 1), default=1, field="map_incremental",
        held={0: [("test_gpu_map_update.py::test_update_equals_fresh_context",
                   "every update regenerates the whole model")]}),
}
# no key is exempt today; a reason alone does not admit one
EXEMPT_ALLOWED = set()


# ---------------------------------------------------------------- the sites
# Every site of csrc/*.cpp that READS c->cpt or c->nt_streams
# ("file:function:callee:field", callee = the innermost call the read is an
# argument of, or "=" + the assigned name) and every launch_* function of
# csrc/*.hip with an `int cpt` or `bool nt` parameter ("file:function").
# test_tuning_table_cpu.py::test_read_sites_have_rows collects both from the
# sources.  Per row:
#   n        reads of that key in that function (read sites only)
#   runs     {setting: (the instantiation it starts, [tests that run it])};
#            a setting is cpt, nt or (cpt, nt) as the row's fields say
#   note     what the code makes true
#   gap      instead of runs, for a known gap: why it is open
_Q_ONE = "test_gpu_control.py::test_qmdp_one_hot_is_the_next_sweep"
_Q_F64 = "test_gpu_control.py::test_qmdp_spread_beliefs_against_fp64"
_P_LOOP = "test_gpu_parity.py::test_loop_step_matches_separate_ops"
_P_BLOCKS = "test_gpu_parity.py::test_loop_normalisation_blocks"
_BELIEF_RUNS = {4: ("k_belief_update<4>", [_DENSE[0]] + _PLANNER[1:]),
                2: ("k_belief_update<2>", [_DENSE[0]] + _PLANNER[1:]),
                1: ("k_belief_update<1>", [_DENSE[0]] + _PLANNER[1:])}
_PARTIALS_RUNS = {4: ("4 * cells_grid(g, 4) partials", _PLANNER[1:]),
                  2: ("4 * cells_grid(g, 2) partials", _PLANNER[1:]),
                  1: ("4 * cells_grid(g, 1) partials", _PLANNER[1:])}
_SWEEP_RUNS = {(4, 1): ("k_mdp_sweep<4,true>", [_DENSE[1]]),
               (4, 0): ("k_mdp_sweep<4,false>", [_DENSE[1], _Q_ONE]),
               (2, None): ("k_mdp_sweep<2,false>", [_DENSE[1]]),
               (1, None): ("k_mdp_sweep<1,false>", [_DENSE[1]])}
_LOOP_RUNS = {(4, 1): ("k_loop_step<4,true>", [_DENSE[2]]),
              (4, 0): ("k_loop_step<4,false>", [_DENSE[2]]),
              (2, None): ("k_loop_step<2,false>", [_DENSE[2], _P_LOOP, _P_BLOCKS]),
              (1, None): ("k_loop_step<1,false>", [_DENSE[2], _P_LOOP, _P_BLOCKS])}
_EXPAND_RUNS = {4: ("k_expand_pred<4>, k_expand_stats<4>", _PLANNER),
                2: ("k_expand_pred<1>, k_expand_stats<1> on cells_grid(g, 1)", _PLANNER),
                1: ("k_expand_pred<1>, k_expand_stats<1>", _PLANNER)}
_DOTS_RUNS = {4: ("k_belief_dots<4>", _PLANNER),
              2: ("k_belief_dots<1> on cells_grid(g, 1)", _PLANNER),
              1: ("k_belief_dots<1>", _PLANNER)}
_CONTROL_RUNS = {1: ("k_control_q<true>", [_Q_ONE, _Q_F64]),
                 0: ("k_control_q<false>", [_Q_ONE, _Q_F64])}

SITES = {
    # ---- launch functions (csrc/*.hip)
    "pp2_kernels.hip:launch_belief_update": dict(fields=("cpt",), runs=_BELIEF_RUNS),
    "pp2_kernels.hip:launch_mdp_sweep": dict(
        fields=("cpt", "nt"), runs=_SWEEP_RUNS, note="nt is looked at only at 4 cells per lane"),
    "pp2_kernels.hip:launch_loop_step": dict(
        fields=("cpt", "nt"), runs=_LOOP_RUNS, note="nt is looked at only at 4 cells per lane"),
    "pp2_kernels.hip:launch_expand": dict(
        fields=("cpt",), runs=_EXPAND_RUNS,
        note="only <4> and <1> exist: the grid is that of the instantiation started"),
    "pp2_kernels.hip:launch_belief_dots": dict(
        fields=("cpt",), runs=_DOTS_RUNS,
        note="only <4> and <1> exist: the grid is that of the instantiation started"),
    "pp2_control.hip:launch_control_q": dict(
        fields=("nt",), runs=_CONTROL_RUNS,
        note="control_blocks is cells_grid(g, 4) whatever the context's cpt: the kernel has one "
             "cell layout.  The one-hot test holds the bits; the fp64 test bounds the sums at "
             "rel 1e-5 and does not see an ulp"),
    # ---- read sites (csrc/*.cpp)
    "pp2_runtime.cpp:gate_ctx:=x.cpt:cpt": dict(
        n=1, fields=("cpt",),
        runs={4: ("coded_active where a dictionary exists", _DENSE),
              2: ("coded_active false", _DENSE), 1: ("coded_active false", _DENSE)},
        note="every dense case asserts model_dict_info()"),
    "pp2_runtime.cpp:mdp_sweep_once:launch_mdp_sweep:cpt": dict(
        n=1, fields=("cpt", "nt"), runs=_SWEEP_RUNS),
    "pp2_runtime.cpp:mdp_sweep_once:launch_mdp_sweep:nt_streams": dict(
        n=1, fields=("cpt", "nt"), runs=_SWEEP_RUNS),
    "pp2_runtime.cpp:launch_belief:launch_belief_update:cpt": dict(
        n=1, fields=("cpt",), runs=_BELIEF_RUNS),
    "pp2_runtime.cpp:belief_update_impl:mass_partials:cpt": dict(
        n=1, fields=("cpt",),
        runs={4: ("4 * cells_grid(g, 4) partials", [_DENSE[0]]),
              2: ("4 * cells_grid(g, 2) partials", [_DENSE[0]]),
              1: ("4 * cells_grid(g, 1) partials", [_DENSE[0]])},
        note="the mass read back beside the raw belief is the sum of exactly these partials"),
    "pp2_runtime.cpp:loop_launch:launch_loop_step:cpt": dict(
        n=1, fields=("cpt", "nt"), runs=_LOOP_RUNS),
    "pp2_runtime.cpp:loop_launch:launch_loop_step:nt_streams": dict(
        n=1, fields=("cpt", "nt"), runs=_LOOP_RUNS),
    "pp2_runtime.cpp:loop_launch:mass_partials:cpt": dict(
        n=1, fields=("cpt", "nt"), runs=_LOOP_RUNS,
        note="the next step divides by the sum of these partials"),
    "pp2_control.cpp:enqueue_q:launch_control_q:nt_streams": dict(
        n=1, fields=("nt",), runs=_CONTROL_RUNS, note="only while the coded model is off"),
    "pp2_tree.cpp:materialize:mass_partials:cpt": dict(
        n=1, fields=("cpt",), runs=_PARTIALS_RUNS,
        note="the re-root onto a sampled child (second step, sampled z)"),
    "pp2_tree.cpp:tree_update:mass_partials:cpt": dict(
        n=1, fields=("cpt",), runs=_PARTIALS_RUNS,
        note="the fresh root (second step, z not sampled)"),
    "pp2_tree.cpp:make_root:launch_belief_dots:cpt": dict(
        n=1, fields=("cpt",), runs=_DOTS_RUNS),
    "pp2_tree.cpp:expand_vnode:launch_expand:cpt": dict(
        n=1, fields=("cpt",), runs=_EXPAND_RUNS),
}


def setting_keys(fields, setting):
    """The keys a setting of a SITES row leaves at a non-default value."""
    vals = dict(zip(fields, setting if isinstance(setting, tuple) else (setting,)))
    keys = []
    if vals.get("cpt") not in (None, TUNING["PP2_TUNE_CELLS_PER_LANE"]["default"]):
        keys.append("PP2_TUNE_CELLS_PER_LANE")
    if vals.get("nt") not in (None, TUNING["PP2_TUNE_NT_STREAMS"]["default"]):
        keys.append("PP2_TUNE_NT_STREAMS")
    return keys


def named_tests():
    """Every "file::test" the two tables name, with the key whose non-default
    value it is listed for (None: listed for a default setting only):
    [(test, TUNING name or None)]."""
    out = []
    for name, row in TUNING.items():
        for tests in row.get("held", {}).values():
            out += [(t, name) for t, _ in tests]
    for row in SITES.values():
        for setting, (_, tests) in row.get("runs", {}).items():
            keys = setting_keys(row["fields"], setting) or [None]
            out += [(t, k) for t in tests for k in keys]
    return sorted(set(out), key=lambda tk: (tk[0], tk[1] or ""))
