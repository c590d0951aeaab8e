"""Every environment switch of the planner's expansion path that no other test
sets, held to the reference-arithmetic oracle bit for bit
(planner_shape_cases.SWITCHES says which variable is held where, and
test_planner_shapes_cpu.py::test_switch_table_is_complete that the table names
every variable the library reads).

The cases (planner_shape_cases.SWITCH_CASES) run exactly as
test_gpu_planner_shapes.py's do: planner_shape_run.run_reference_order, the
device planner and the oracle in lockstep, the whole tree snapshot, the action
and the value equal at step 0 and at every following step.  No tolerance.

Switches read per planner or per call are set with monkeypatch.  Switches the
library caches per process (PP2_FC_SUMTAB, PP2_FC_K9WAVE, PP2_FC_PLAN9,
PP2_FC_KEPT_GY, PP2_FC_PLAN) need a fresh process: one child
(planner_switch_child.py) per switch set, started with subprocess.run, one at
a time, with the switch set added to the inherited environment.

The child's time limit is a hang stop, not a performance bound.  The default
path's cases at the child's three shapes (test_gpu_planner_shapes.py::
test_reference_order_bit_exact[1x7-uniform-fib-3-seq_chain_max0],
[33x65-uniform-pbvi-2] and [63x131-uniform-fib-3]) took 0.03 + 0.04 + 0.11 =
0.18 s (pytest --durations) on an MI355X; ten times that plus 60 s for
process start and library load is the limit: 61.8 s.  (A child took 0.7 s
there, nearly all of it start-up.)  A child that a signal ended (a fault, an
abort), that stopped at an error of the library or the device, or that ran
into the limit fails its test and ends the session: nothing further starts
on the GPU after a fault or a hang.
"""
import os
import re
import subprocess
import sys

import pytest

import planner_shape_cases as PC
from planner_shape_run import host_models, run_reference_order

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "planner_switch_child.py")
MEASURED_SUM_S = 0.18
CHILD_TIMEOUT_S = 10 * MEASURED_SUM_S + 60


@pytest.fixture(scope="module")
def host_model(oracle):
    """(T, L, R) of a table shape, generated once per shape."""
    return host_models(oracle)


def no_fc_walk(on):
    raise AssertionError("a switch case does not choose the chain sets' driver")


@pytest.mark.parametrize("case", PC.INPROCESS_SWITCH_CASES, ids=PC.ref_case_id)
def test_switch_reference_order_bit_exact(oracle, host_model, monkeypatch, capfd, case):
    """The switches pp2_planner_create or every launch reads.  With
    PP2_PBVI_FCHAIN=1 the switch can be shown to have taken effect without
    new API (neither info() nor a debug entry point exposes the counter):
    PP2_PBVI_STATS=1 makes the planner report its candidate counter on
    stderr when it is destroyed -- candidate sets ran and kept candidates.
    The two diagnostics report there too."""
    import path_planning_2d_amd as P
    capfd.readouterr()
    run_reference_order(P, oracle, host_model, case, monkeypatch, no_fc_walk)
    err = capfd.readouterr().err
    if "PP2_PLAN_TIMING" in case[5]:  # the diagnostics ran: their reports
        assert re.search(r"pp2 planner: \d+ expansions, host us per expansion", err), err
    if "PP2_PLAN_EVENTS" in case[5]:
        assert re.search(r"pp2 planner: device us from an expansion's start", err), err
    if "PP2_PBVI_FCHAIN" in case[5]:
        m = re.search(r"PBVI candidate chains (\d+) over (\d+) rows in (\d+) sets", err)
        assert m, f"no candidate counter in the planner's report: {err!r}"
        cands, rows, sets = (int(g) for g in m.groups())
        # a set per root (one a step) and per expansion, over the root rows
        # and the kept children; every row keeps at least the alpha of its
        # maximum as a candidate, at most all of them
        assert sets > case[4] + 1 and rows > sets
        assert rows <= cands <= rows * PC.PBVI_S


@pytest.fixture
def stop_after_fault():
    """After a child that a signal or its time limit ended: the session ends
    once the test has failed (nothing further starts on the GPU)."""
    why = []
    yield why
    if why:
        pytest.exit(why[0], returncode=1)


@pytest.mark.parametrize("sw", PC.CHILD_SETS, ids=PC.switch_set_id)
def test_process_switch_reference_order_bit_exact(oracle, stop_after_fault, sw):
    """The switches cached per process, in a child process of their own
    (the oracle fixture comes first: the child finds the oracle built)."""
    ids = [PC.ref_case_id(c) for c in PC.child_cases(sw)]
    name = PC.switch_set_id(sw)
    try:
        r = subprocess.run([sys.executable, CHILD, *ids], env={**os.environ, **sw},
                           timeout=CHILD_TIMEOUT_S, capture_output=True)
    except subprocess.TimeoutExpired as e:
        stop_after_fault.append(f"{name}: the child ran into its time limit")
        out = (e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace")
        pytest.fail(f"{name}: no end after {CHILD_TIMEOUT_S:.0f} s\n{out[-4000:]}")
    out = r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace")
    # (3: the child stopped at an error of the library or the device)
    if r.returncode < 0 or r.returncode in (3, 134, 139):
        stop_after_fault.append(f"{name}: the child ended with status {r.returncode}")
    assert r.returncode == 0, f"{name}: child exit status {r.returncode}\n{out[-4000:]}"
    for cid in ids:
        assert f"ok {cid}\n" in r.stdout.decode(), f"{name}: no result line of {cid}\n{out[-4000:]}"
