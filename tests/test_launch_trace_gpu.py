"""GPU: mrla_amd/functional.py asks of the C ABI exactly what the golden says (tests/golden/launch_trace.json, recorded by
scripts/record_launch_trace.py from the commit before functional.py was restructured, on the same library): per scenario and
call mode the same entry points in the same order, with the same integers and floats, the same pointers NULL, and -- with a
KernelTimer on -- the same (label, nbytes, alg, path) records, which bench.py's roofline figure is made of.  Addresses are not
compared: where a buffer is allocated is free.  tests/launch_trace_cases.py has the scenarios and what each exists for."""
import json
import os

import pytest

from tests import cases, launch_trace_cases as ltc

pytestmark = pytest.mark.gpu

_golden = {}


def golden():
    if not _golden:
        with open(os.path.join(cases.GOLDEN, "launch_trace.json")) as fh:
            _golden.update(json.load(fh))
    return _golden


def test_the_golden_has_every_scenario_and_mode():
    assert set(golden()["scenarios"]) == {f"{s.name}/{m}" for s in ltc.SCENARIOS for m in ltc.MODES}


@pytest.mark.parametrize("mode", ltc.MODES)
@pytest.mark.parametrize("name", [s.name for s in ltc.SCENARIOS])
def test_launches_are_the_recorded_ones(name, mode):
    got = ltc.trace(ltc.BY_NAME[name], mode)           # (asserts the entry points the scenario exists for)
    diff = ltc.first_difference(got, ltc.unpack(golden(), f"{name}/{mode}"))
    if diff:
        print(f"{name}/{mode}: {diff}")
    assert diff is None, diff
