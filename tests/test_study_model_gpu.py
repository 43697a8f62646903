"""The HIP engine's accepted SPR1 moves of the rare kinds held to the identity of move_steps.check_accepted_spr1: the chains of
test_study_model.py's lean stepper through EmatBackend, the same cases, seeds and wants.  What the model is and what the classes are:
tests/study_model.py, tests/test_study_model.py.  The studies of more than 64 regions take wave_local_scan to a second chunk of a level,
the one of more than 640 regions past its default block fifteen times over."""
import pytest

import delphy_amd as d
from test_study_model import C, LEAN, assert_lean_conditions, run_lean

pytestmark = pytest.mark.gpu

_done = {}


def _device(num_sites, trace):
    return d.EmatBackend(num_sites, trace_moves=trace)


@pytest.mark.parametrize("name", list(LEAN))
def test_device_accepted_spr1_of_the_rare_kinds(name, record_property):
    tally, cov, info = _done[name] = run_lean(name, _device, "device")
    record_property("classes", dict(zip(C, cov.accepted_spr1_classes)))
    record_property("run", info)
    print(name, info, dict(zip(C, cov.accepted_spr1_classes)))
    print(tally.summary())
    tally.finish(record_property)
    assert cov.unchecked == 0 and not info["unmet"], info


def test_device_lean_cases_cover_what_they_must(record_property):
    for name in LEAN:
        if name not in _done:
            _done[name] = run_lean(name, _device, "device")
    assert_lean_conditions(_done, record_property)
