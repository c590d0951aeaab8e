"""CPU checks of tuning_cases.py against the sources: the three lists of
tuning keys agree with TUNING, every site that reads c->cpt or c->nt_streams
and every launch function that takes either has a SITES row, every test the
tables name exists in a file that sets the key, and the shapes of
test_gpu_tuning.py satisfy the relations they are there for.  No GPU."""
import collections
import functools
import os
import re

import numpy as np
import pytest

import planner_shape_cases as PC
import tuning_cases as TC
from conftest import ROOT

CSRC = os.path.join(ROOT, "path_planning_2d_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
# how a reference-order case of planner_shape_cases sets a key
REF_CASE_SWITCH = {"PP2_TUNE_CELLS_PER_LANE": "cpt", "PP2_TUNE_CODED_MODEL": "coded"}


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def set_tuning_body():
    text = strip_comments(read("path_planning_2d_amd", "csrc", "pp2_runtime.cpp"))
    m = re.search(r"^int pp2_set_tuning\(.*?^}", text, re.S | re.M)
    assert m, "pp2_set_tuning not found"
    return text, m.group(0)


def case_bodies(body):
    """{key name: the statements of its case label}"""
    parts = re.split(r"\bcase (PP2_TUNE_\w+):", body)
    out = {}
    for name, stmts in zip(parts[1::2], parts[2::2]):
        assert name not in out, f"two case labels for {name}"
        out[name] = stmts.split("default:")[0]
    return out


@pytest.mark.parametrize("name", sorted(TC.LIMITS))
def test_restated_constants_match_sources(name):
    value, fname, pattern = TC.LIMITS[name]
    found = re.findall(pattern, read("path_planning_2d_amd", "csrc", fname))
    assert len(found) == 1, f"{name}: {pattern!r} matches {len(found)} times in {fname}"
    assert int(found[0]) == value, f"{name} is {found[0]} in {fname}, restated as {value}"


# ---------------------------------------------------------------- 1. keys
def key_lists():
    header = {m.group(1): int(m.group(2)) for m in
              re.finditer(r"^#define (PP2_TUNE_\w+) (\d+)\s*$", read("include", "pp2.h"), re.M)}
    core = {"PP2_" + m.group(1): int(m.group(2)) for m in
            re.finditer(r"^    (TUNE_\w+) = (\d+)\s*$",
                        read("path_planning_2d_amd", "core.py"), re.M)}
    _, body = set_tuning_body()
    return header, core, case_bodies(body)


def test_key_lists_agree():
    """pp2.h's #defines, core.py's constants, pp2_set_tuning's case labels and
    TUNING: the same names with the same numbers."""
    header, core, cases = key_lists()
    table = {k: row["number"] for k, row in TC.TUNING.items()}
    assert header == table, (
        f"pp2.h but not TUNING: {sorted(set(header.items()) - set(table.items()))}; "
        f"TUNING but not pp2.h: {sorted(set(table.items()) - set(header.items()))}")
    assert core == table, (
        f"core.py but not TUNING: {sorted(set(core.items()) - set(table.items()))}; "
        f"TUNING but not core.py: {sorted(set(table.items()) - set(core.items()))}")
    assert set(cases) == set(table), (
        f"case labels but not TUNING: {sorted(set(cases) - set(table))}; "
        f"TUNING without a case label: {sorted(set(table) - set(cases))}")
    assert len(table) == 16 and len(set(table.values())) == 16


def test_rows_say_what_the_code_does():
    """Every row's field is what its case label writes, its range what the
    label checks, and every non-default value is held or the row exempt."""
    text, body = set_tuning_body()
    cases = case_bodies(body)
    ctx_h = read("path_planning_2d_amd", "csrc", "pp2_ctx.h")
    for name, row in TC.TUNING.items():
        stmts = cases[name]
        if name == "PP2_TUNE_CELLS_PER_LANE":  # forwards to pp2_set_cells_per_lane
            assert "pp2_set_cells_per_lane(c, value)" in stmts
            m = re.search(r"^int pp2_set_cells_per_lane\(.*?^}", text, re.S | re.M)
            stmts = m.group(0).replace("cpt", "value").replace("c->value", "c->cpt")
            assert all(f"value != {v}" in stmts for v in row["values"]), name
        assert re.search(rf"c->{row['field']} = value", stmts), f"{name} does not write {row['field']}"
        # the member exists, with the default the row states where it is a number
        m = re.search(rf"^\s*(?:int|bool)\s+{row['field']}\s*=\s*([-\w]+)[;,]", ctx_h, re.M)
        assert m, f"{name}: no member {row['field']} in pp2_ctx.h"
        if isinstance(row["default"], int):
            init = {"true": 1, "false": 0}.get(m.group(1), m.group(1))
            if str(init).lstrip("-").isdigit():
                assert int(init) == row["default"], f"{name}: default {init}"
        if row.get("boolean"):
            assert f"c->{row['field']} = value != 0" in stmts, name
            assert row["values"] == (0, 1)
        if "range" in row:
            lo, hi = row["range"]
            assert re.search(rf"value < {lo}\b", stmts), f"{name}: no lower bound {lo}"
            if hi is not None:
                assert re.search(rf"value > {hi}\b", stmts), f"{name}: no upper bound {hi}"
            if isinstance(row["values"], tuple) and isinstance(hi, int):
                assert row["values"] == tuple(range(lo, hi + 1)), name
        if "exempt" in row:
            assert name in TC.EXEMPT_ALLOWED and row["exempt"] and "held" not in row, name
            continue
        held = set()
        for k in row["held"]:
            held |= set(k if isinstance(k, tuple) else (k,))
        assert all(row["held"].values()), f"{name}: a value with no test"
        assert row["default"] not in held, f"{name}: the default needs no row"
        if isinstance(row["values"], tuple):
            want = set(row["values"]) - {row["default"]}
            assert held == want, f"{name}: held {sorted(held)}, non-default values {sorted(want)}"
        else:
            assert held, name
    assert TC.EXEMPT_ALLOWED == {k for k, r in TC.TUNING.items() if "exempt" in r}


# ---------------------------------------------------------------- 2. sites
FIELD_OF = {"cpt": "cpt", "nt_streams": "nt"}


def enclosing_function(text, pos):
    """The name of the last function definition that starts at column 0
    before pos."""
    name = None
    for m in re.finditer(r"^[A-Za-z_][^\n;{}]*?\b([A-Za-z_]\w*)\([^;{}]*\)\s*(?:const\s*)?\{",
                         text[:pos], re.M):
        name = m.group(1)
    return name


def enclosing_call(text, pos):
    """The innermost call that text[pos] is an argument of, or "=" + the
    assigned name where it is the right side of a plain assignment."""
    depth = 0
    i = pos
    while i > 0:
        i -= 1
        ch = text[i]
        if ch == ")":
            depth += 1
        elif ch == "(":
            if depth == 0:
                m = re.search(r"([A-Za-z_]\w*)\s*$", text[:i])
                return m.group(1) if m else "?"
            depth -= 1
        elif ch in ";{}" and depth == 0:
            m = re.match(r"\s*([\w.\->]+)\s*=[^=]", text[i + 1:pos])
            return "=" + m.group(1) if m else "?"
    return "?"


def collect_read_sites():
    """Counter of "file:function:callee:field" over csrc/*.cpp."""
    sites = collections.Counter()
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith(".cpp"):
            continue
        text = strip_comments(read("path_planning_2d_amd", "csrc", fname))
        for m in re.finditer(r"\bc->(cpt|nt_streams)\b(?!\s*=[^=])", text):
            sites[f"{fname}:{enclosing_function(text, m.start())}:"
                  f"{enclosing_call(text, m.start())}:{m.group(1)}"] += 1
    return sites


def collect_launch_functions():
    """{"file:function": fields} of the launch_* definitions of csrc/*.hip
    with an `int cpt` or a `bool nt` parameter."""
    out = {}
    for fname in sorted(os.listdir(CSRC)):
        if not fname.endswith(".hip"):
            continue
        text = strip_comments(read("path_planning_2d_amd", "csrc", fname))
        for m in re.finditer(r"^hipError_t (launch_\w+)\(([^)]*)\)\s*\{", text, re.M):
            fields = tuple(f for f, pat in (("cpt", r"\bint cpt\b"), ("nt", r"\bbool nt\b"))
                           if re.search(pat, m.group(2)))
            if fields:
                out[f"{fname}:{m.group(1)}"] = fields
    return out


def test_read_sites_have_rows():
    reads = collect_read_sites()
    launches = collect_launch_functions()
    assert reads and launches
    assert not [k for k in reads if "?" in k or ":None:" in k], sorted(reads)
    rows_read = {k: r["n"] for k, r in TC.SITES.items() if "n" in r}
    rows_launch = {k: r["fields"] for k, r in TC.SITES.items() if "n" not in r}
    assert dict(reads) == rows_read, (
        f"read sites without a SITES row: {sorted(set(reads.items()) - set(rows_read.items()))}; "
        f"SITES rows without a site: {sorted(set(rows_read.items()) - set(reads.items()))}")
    assert launches == rows_launch, (
        f"launch functions without a SITES row: {sorted(set(launches) - set(rows_launch))}; "
        f"SITES rows without one, or other parameters: "
        f"{sorted(k for k in rows_launch if launches.get(k) != rows_launch[k])}")
    # the key is written in exactly the places the table knows
    writes = collections.Counter()
    for fname in sorted(os.listdir(CSRC)):
        if fname.endswith((".cpp", ".hip", ".h")):
            text = strip_comments(read("path_planning_2d_amd", "csrc", fname))
            for m in re.finditer(r"\bc->(cpt|nt_streams)\s*=[^=]", text):
                writes[f"{fname}:{enclosing_function(text, m.start())}:{m.group(1)}"] += 1
    assert writes == {"pp2_runtime.cpp:pp2_set_cells_per_lane:cpt": 1,
                      "pp2_runtime.cpp:pp2_set_tuning:nt_streams": 1}, writes
    for key, row in TC.SITES.items():
        if "gap" in row:
            assert row["gap"] and "runs" not in row, key
            continue
        # every value of the fields the site reads is run by some test
        want_cpt = TC.TUNING["PP2_TUNE_CELLS_PER_LANE"]["values"]
        want_nt = TC.TUNING["PP2_TUNE_NT_STREAMS"]["values"]
        got = list(row["runs"])
        if row["fields"] == ("cpt",):
            assert sorted(got) == sorted(want_cpt), key
        elif row["fields"] == ("nt",):
            assert sorted(got) == sorted(want_nt), key
        else:  # nt is looked at only at 4 cells per lane
            assert set(got) == {(4, 1), (4, 0), (2, None), (1, None)}, key
        for setting, (what, tests) in row["runs"].items():
            assert what and tests, f"{key} {setting}: nothing runs it"


def test_expansion_launches_size_their_own_instantiation():
    """launch_expand and launch_belief_dots have no <2> kernels: they start
    <4> at 4 cells per lane and <1> otherwise, on that instantiation's grid
    (whose partials the planner's buffers hold: cells_grid(g, 1))."""
    text = strip_comments(read("path_planning_2d_amd", "csrc", "pp2_kernels.hip"))
    for fn, kernels in (("launch_expand", ("k_expand_pred", "k_expand_stats")),
                        ("launch_belief_dots", ("k_belief_dots",))):
        m = re.search(rf"^hipError_t {fn}\(.*?^}}", text, re.S | re.M)
        body = m.group(0)
        for k in kernels:
            assert set(re.findall(rf"{k}<(\d)>", body)) == {"4", "1"}, (fn, k)
        assert "cells_grid(g, cpt == 4 ? 4 : 1)" in body, fn
        assert "cells_grid(g, cpt)" not in body, fn
    tree = strip_comments(read("path_planning_2d_amd", "csrc", "pp2_tree.cpp"))
    assert re.search(r"tiles1 = pp2::cells_grid\(c->g, 1\)", tree)
    for buf in ("d_rpart", "d_spart", "d_bpart"):
        assert re.search(rf"hipMalloc\(&p->{buf}, \(size_t\)\(?tiles1", tree), buf


# ---------------------------------------------------------------- 3. tests
def test_named_tests_exist_and_set_their_key():
    named = TC.named_tests()
    assert named
    for test, key in named:
        fname, fn = test.split("::")
        path = os.path.join(TESTS, fname)
        assert os.path.exists(path), f"{test}: no such file"
        text = read("tests", fname)
        assert re.search(rf"^def {fn}\(", text, re.M), f"no {test}"
        assert re.search(r"^pytestmark = pytest\.mark\.gpu", text, re.M), fname
        if key is None:
            continue
        pattern = TC.TUNING[key].get("sets", key.replace("PP2_", ""))
        if "PC.REF_CASES" in text and not re.search(pattern, text):
            # set through the case list (planner_shape_run.context)
            sw = REF_CASE_SWITCH[key]
            default = TC.TUNING[key]["default"]
            assert any(sw in c[5] and c[5][sw] != default for c in PC.REF_CASES), \
                f"{test}: no REF_CASES entry sets {sw}"
            run = read("tests", "planner_shape_run.py")
            assert re.search(pattern, run), f"planner_shape_run.py does not set {key}"
        else:
            assert re.search(pattern, text), f"{fname} does not set {key} ({pattern})"


def test_case_lists_cover_the_issue():
    assert [s[:2] for s in TC.DENSE_SETTINGS] == [(4, 1), (4, 0), (2, 1), (1, 1)]
    assert [TC.coded_expected(c, k) for c, _, k in TC.DENSE_SETTINGS] == [False] * 4
    assert TC.coded_expected(4, 1)
    assert len(TC.PLANNER_CASES) == 3 * (3 * 2 + 2)
    assert len({TC.planner_case_id(c) for c in TC.PLANNER_CASES}) == len(TC.PLANNER_CASES)
    for cpt in TC.PLANNER_CPTS:
        mine = [c for c in TC.PLANNER_CASES if c[4] == cpt]
        assert {(c[0], c[1]) for c in mine if c[3] == 0} == set(TC.PLANNER_SHAPES)
        assert {(c[0], c[1]) for c in mine if c[3] == 1} == {(33, 65)}
        assert {c[2] for c in mine} == {"uniform", "delta_last"}
    # the shapes and beliefs are planner_shape_cases' own
    assert all((c[0], c[1]) in PC.ALL and c[2] in PC.BELIEFS for c in TC.PLANNER_CASES)
    assert (33, 65, "uniform", 0, 3, {"cpt": 1}) in PC.REF_CASES
    assert (63, 131, "uniform", 0, 3, {"cpt": 2}) in PC.REF_CASES


# ---------------------------------------------------------------- 4. shapes
def test_smallest_shapes():
    """The relations the shapes of test_gpu_tuning.py are there for, from
    wp = (W + 3) & ~3 and kBlock."""
    B = TC.K["kBlock"]
    assert B == 256
    hw = [(H, W) for H, W, _ in TC.DENSE_SHAPES]
    assert set(TC.DENSE_NOTES) == set(hw)
    # 1x7: one row, wp 8: two threads at 4 cells per lane, 8 at 1
    assert TC.wp_of(7) == 8 and [TC.threads(1, 7, c) for c in (4, 2, 1)] == [2, 4, 8]
    # 5x1: wp 4 -- one thread a row at 4 cells per lane, two at 2, four at 1;
    # the only valid cell is the first of its lane at every setting
    assert TC.wp_of(1) == 4 and [TC.threads(5, 1, c) // 5 for c in (4, 2, 1)] == [1, 2, 4]
    # 33x65: W % 4 == 1 (three pad cells end the row's last lane); 17 threads a
    # row at 4 cells per lane, 561 in all: block 0 ends inside row 15
    # (256 = 15 * 17 + 1), block 1 inside row 30, the last block holds 49
    assert 65 % 4 == 1 and TC.wp_of(65) == 68 and TC.threads(33, 65, 4) == 561
    assert B % (68 // 4) != 0 and (2 * B) % (68 // 4) != 0
    assert TC.blocks(33, 65, 4) == 3 and 561 % B == 49
    assert [TC.blocks(33, 65, c) for c in (2, 1)] == [5, 9]
    assert all(TC.threads(33, 65, c) % B and B % (68 // c) for c in (2, 1))
    # 97x131: W % 4 == 3, 13 blocks at 4 cells per lane, 50 full ones and a
    # last one of 4 threads at 1; ragged and mid-row at every setting
    assert 131 % 4 == 3 and TC.wp_of(131) == 132
    assert [TC.blocks(97, 131, c) for c in (4, 2, 1)] == [13, 26, 51]
    assert divmod(TC.threads(97, 131, 1), B) == (50, 4)
    assert all(TC.threads(97, 131, c) % B and B % (132 // c) for c in (4, 2, 1))
    # the seeds are those of the suite's own tables
    parity = read("tests", "test_gpu_parity.py")
    for H, W, seed in TC.DENSE_SHAPES:
        if (H, W) == (33, 65):
            assert (H, W, seed) in PC.SHAPES
        else:
            assert f"({H}, {W}, {seed})" in parity, (H, W, seed)
    # planner shapes: under the launch sizing this guards against (the <1>
    # kernels on the grid of 2 cells per lane, which reaches rows // 2 rows)
    # delta_last has ALL its mass out of reach and uniform a good part of it
    for H, W in TC.PLANNER_SHAPES:
        assert TC.threads(H, W, 2) // TC.wp_of(W) == H // 2
        assert TC.skipped_by_half_grid(H, W, "delta_last") == 1.0
        assert 0.3 < TC.skipped_by_half_grid(H, W, "uniform") < 0.7
        # and the two grids differ, so the sizing matters
        assert TC.blocks(H, W, 2) != TC.blocks(H, W, 1) or TC.threads(H, W, 1) <= B
    assert TC.blocks(33, 65, 1) == 9 and TC.blocks(63, 131, 1) == 33
    assert TC.blocks(63, 131, 4) == 9 and 131 % 4 == 3


@functools.lru_cache(maxsize=None)
def host_model(H, W):
    """(T, L, R, FIB alphas after at most 40 sweeps) of a table shape."""
    from oracle import oracle as O
    O.build()
    T, L, R = O.model_pomdp(PC.grid_of(H, W), PC.goal_of(H, W))
    alphas, _, _ = O.fib_solve(H, W, PC.GAMMA, T, L, R, max_sweeps=40)
    return T, L, R, alphas


@pytest.mark.parametrize("case", [c for c in TC.PLANNER_CASES if c[4] == 4],
                         ids=TC.planner_case_id)
def test_second_step_observations_exist(oracle, case):
    """test_default_order_second_step needs, for the root's chosen action,
    an observation its expansion sampled and one it did not, and a belief
    update with mass for the latter."""
    H, W, kind, lb, _ = case
    T, L, R, alphas = host_model(H, W)
    pl = oracle.Planner(PC.grid_of(H, W), T, L, R, alphas, max_depth=PC.MAX_DEPTH, max_iter=1,
                        accurate=True)
    if lb:
        pl.set_pbvi(*PC.pbvi_of(H, W))
    a, _ = pl.step(0, 0, PC.belief_of(H, W, kind))
    info = pl.info()
    pl.close()
    sampled, other = TC.second_step_observations(info, a)
    assert sampled is not None and other, (sampled, other)
    masses = [float(oracle.belief_update(H, W, T, L, PC.belief_of(H, W, kind), a, z)
                    .sum(dtype=np.float64)) for z in other]
    assert max(masses) > 0.0
