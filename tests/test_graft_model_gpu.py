"""The device's own graft analysis and forced re-attachments (EmatBackend.debug_graft: dev::analyze_graft, peel_graft,
spr_move_topology, propose_new_graft, apply_graft on lane 0 of a wavefront, as inside a chain) against the exact model of one
graft.  The cases, the targets and the assertions are test_graft_model.py's, which holds the CPU oracle to the same model; the
model's results are computed once per session and shared (the tree a forced move leaves behind is the same tree on both engines,
and its model is kept by the tree's content).

What the hook runs.  k_debug_graft works on the part's slab where it lies in HBM: no part is staged in LDS by it, whatever the
handle's use_lds says (that option changes the host's slab geometry and size classes only), so there is one run per case here
and not one per staging variant.  The graft code compiled for LDS-staged parts is held to the model through the chains of
test_move_steps_gpu.py, which really are staged: every accepted subtree slide there is held to the exact log_mh built on the same
four graft numbers.

Room.  A chain stops a part BEFORE a move when its heap is short of the reserve, and redoes on a larger slab a move that
overflowed; the hook does neither.  At the product's default slack (3) a forced move at mu_proposal 1e-3, six times the
scenario's rate, overflowed a small part of the eight-part cut and ended with part status 102 (k_part_overflow: a bounds-checked
container refused the write).  The forced moves therefore get their room up front (FORCED_MOVE_SLACK), which means they never run
at the default geometry, and nothing here asserts what the default geometry ends with."""
import time

import pytest

import delphy_amd as d
import test_graft_model as G
from test_exact_model import Tally

pytestmark = pytest.mark.gpu

FORCED_MOVE_SLACK = 24.0


def _device(slab_slack=0.0):
    return lambda num_sites: d.EmatBackend(num_sites, slab_slack=slab_slack)


@pytest.mark.parametrize("name", G.CASES)
def test_device_analyses_against_the_model(name, record_property):
    """Mode 0 on every X the move code can analyse, at all three proposal rates."""
    tally = Tally("device")
    eng = G.setup(_device()(G.case(name)["sc"].num_sites), name)
    t0 = time.perf_counter()
    try:
        n = sum(G.check_analyses(tally, name, eng, mu) for mu in G.MUS)
    finally:
        eng.close()
    record_property("grafts", n)
    record_property("seconds", round(time.perf_counter() - t0, 2))
    assert n == len(G.MUS) * len(G.analysable(name))
    tally.finish(record_property)


@pytest.mark.parametrize("name", G.FORCED)
def test_device_forced_moves_against_the_model(name, record_property):
    """Mode 3 on the targets the CPU file fixed (every one asserted valid in Python before the device sees it)."""
    tally = Tally("device")
    t0 = time.perf_counter()
    results = G.forced_moves(name, _device(FORCED_MOVE_SLACK))
    record_property("engine_s", round(time.perf_counter() - t0, 2))
    untouched = G.check_forced_moves(tally, name, results)
    record_property("seconds", round(time.perf_counter() - t0, 2))
    assert untouched > 0
    tally.finish(record_property)
