"""The library and tools/plan_dump.cpp run the same planner with the same defaults: for every crg_gemm / crg_conv2d call of the exact
cases (tests/_exact_cases.py, no new shapes) the route the library reports afterwards equals, in all 12 fields, what the stand-alone
planner program prints for the args that call passed.  The args are captured with the recorder's ctypes-level wrapper
(tools/record_routes.py); tests/test_gemm_plan_cpu.py holds the same program against the recorded table without a device."""
import pytest

from tests import _exact_cases as E
from tests.test_gemm_plan_cpu import ROUTE_FIELDS, build_plan_dump, plan_rows

pytestmark = pytest.mark.gpu


def test_library_route_is_the_planners(tmp_path):
    from cremage_amd import ops
    from tests.test_exact_gpu import BF, run_case
    from tools.record_routes import Recorder
    exe = build_plan_dump(tmp_path, sanitize=False)  # (sanitizer builds run in the CPU test only)
    calls = []  # (case id, row), in call order
    with Recorder() as rec:
        for case in E.CASES:
            rec.last = None
            run_case(case, ops, BF)
            if case.route is not None:  # (the other cases run entry points that keep no route record)
                assert rec.last is not None and rec.last["rc"] == 0, case.id
                lib = ops.last_route()
                assert [rec.last["route"][f] for f in ROUTE_FIELDS[1:10]] == [lib[f] for f in ROUTE_FIELDS[1:10]], case.id  # the same record
                calls.append((case.id, rec.last))
    assert len(calls) == sum(c.route is not None for c in E.CASES)
    rows = [row for _, row in calls]
    for (cid, row), (rc, route, msg) in zip(calls, plan_rows(exe, rows)):
        print(f"[plan] {cid}: " + " ".join(f"{k}={v}" for k, v in route.items()))
        assert rc == row["rc"] == 0, (cid, rc, msg)
        assert route == row["route"], (cid, "library", row["route"], "planner", route)
