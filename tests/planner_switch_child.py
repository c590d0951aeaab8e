"""Child process of test_gpu_planner_switches.py: the switches that the
library caches per process (planner_shape_cases.SWITCHES, cached "process")
are read once, so only a fresh process sees another value.  The parent puts
the switch set into this process's environment and names the cases:

    python planner_switch_child.py <case id> [<case id> ...]

Every case is one of planner_shape_cases.SWITCH_CASES and runs through
planner_shape_run.run_reference_order, exactly as the in-process cases do.
One line per case ("ok <id>" or "FAILED <id>: ..."); exit status 0 only if
all held.  A mismatch goes on to the next case; any other error (the library's
or the device's) ends the process there with status 3.  (Not collected by
pytest: the file name matches no test pattern.)
"""
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import planner_shape_cases as PC  # noqa: E402
from planner_shape_run import debug_switch, host_models, run_reference_order  # noqa: E402


def no_fc_walk(on):
    raise AssertionError("a switch case does not choose the chain sets' driver")


def main(argv):
    import pytest
    from oracle import oracle as O
    import path_planning_2d_amd as P
    cases = {PC.ref_case_id(c): c for c in PC.SWITCH_CASES}
    unknown = [i for i in argv if i not in cases]
    if unknown or not argv:
        print(f"unknown case ids: {unknown}" if unknown else "no case ids given")
        return 2
    O.build()
    host_model = host_models(O)
    if os.environ.get("PP2_FC_SUMTAB", "")[:1] == "1":
        # the library read the environment: the cached value is 1 already
        prev = debug_switch("fc_sumtab")(1)
        assert prev == 1, f"PP2_FC_SUMTAB=1 in the environment, the library held {prev}"
    failed = 0
    for cid in argv:
        case = cases[cid]
        try:
            # this process has to have been started with the case's
            # process-cached switches: setting them now would be too late
            for k, v in case[5].items():
                if k in PC.SWITCHES and PC.SWITCHES[k]["cached"] == "process":
                    assert os.environ.get(k) == v, \
                        f"{k}={os.environ.get(k)!r} at start, the case sets {v!r}"
            with pytest.MonkeyPatch.context() as mp:
                run_reference_order(P, O, host_model, case, mp, no_fc_walk)
            print(f"ok {cid}", flush=True)
        except AssertionError as e:  # a mismatch: reported, counted, next case
            failed += 1
            last = traceback.format_exception_only(type(e), e)[-1].strip()
            print(f"FAILED {cid}: {last[:2000]}", flush=True)
        except BaseException as e:  # an error of the library or the device: nothing further runs
            last = traceback.format_exception_only(type(e), e)[-1].strip()
            print(f"FAILED {cid}: {last[:2000]}; stopping", flush=True)
            return 3
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
