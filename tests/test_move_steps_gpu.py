"""Every move of the HIP engine, one at a time, against the exact posterior: the cases of test_move_steps.py through
EmatBackend with the parts staged in LDS and resident in HBM (use_lds), large parts in the side class (k_run_moves_side),
and the parts cut by kernels from the tree resident in HBM, across two cycles.  tests/move_steps.py has the identities and
the bounds; like the oracle, the device must give back mutation times bit for bit after a rejected topology move (the
subtree pruned from under the run's root aside) and holds the lambda_i it recomputed to their exact bounds.  Every accepted
subtree slide, in every one of these runs, is held to the exact log_mh of move_steps.check_accepted_slide, and every accepted SPR1 move
to that of move_steps.check_accepted_spr1 (the candidate studies of tests/study_model.py).
What every one of these moves drew -- kind, picks, words consumed, acceptance, the bounded exponential, the Gaussian step, the slide's
pick, a reform's new times, an SPR1's time in its region -- goes through tests/draws_model.py in the same check_step, with the oracle's
counts per class as the device's minimums (Coverage.assert_conditions).

The same conditions as in test_move_steps.py keep the file honest, over all its cases."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import move_steps as M
from delphy_amd.scenarios import make_scenario
from helpers import configure, split_parts
from test_exact_model import Tally
from test_move_steps import CASES, run_case

pytestmark = pytest.mark.gpu

_done = {}
LDS_OFF_DIVISOR = 4      # the chain does not depend on use_lds: the HBM-resident variant repeats the first quarter of each case


def _device(use_lds):
    return lambda num_sites, trace: d.EmatBackend(num_sites, trace_moves=trace, use_lds=use_lds)


def _run(name, use_lds):
    key = (name, use_lds)
    if key not in _done:
        _done[key] = run_case(name, _device(use_lds), "device", 1 if use_lds else LDS_OFF_DIVISOR) + (dict(M.step_chain.cost),)
    return _done[key]


def _report(record_property, cov, cost=None):
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    if cost:
        record_property("ms_per_single_move_pass_launch_and_sync", round(1e3 * cost["advance_s"] / max(cost["passes"], 1), 4))
        record_property("ms_per_single_move_pass_read_backs", round(1e3 * cost["read_s"] / max(cost["passes"], 1), 4))


@pytest.mark.parametrize("name", ["C1/6", "fine-grid"])
@pytest.mark.parametrize("use_lds", [True, False])
def test_the_stepped_device_chain_is_the_chain(name, use_lds):
    from test_move_steps import prepare
    sc, parts, incl, ref, ev, pop, steps, setup = prepare(name)
    M.assert_stepped_chain_is_the_chain(lambda: setup(_device(use_lds)(sc.num_sites, 300)), len(parts), 300)


@pytest.mark.parametrize("use_lds", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_device_every_move_against_the_exact_posterior(name, use_lds, record_property):
    tally, cov, cost = _run(name, use_lds)
    _report(record_property, cov, cost)
    print("%s use_lds=%s: %.3f ms per single-move pass (launch + sync), %.3f ms for its read-backs, %d passes" % (
        name, use_lds, 1e3 * cost["advance_s"] / max(cost["passes"], 1), 1e3 * cost["read_s"] / max(cost["passes"], 1), cost["passes"]))
    tally.finish(record_property)
    assert cov.unchecked == 0, cov.as_dict()


def test_device_large_parts_in_the_side_class_every_move(record_property):
    """The three 2 000-node parts of test_device_large_parts_in_the_side_class_against_exact (parts_per_cu = 16), 40 moves each."""
    sc = make_scenario("C3", num_tips=3000, num_sites=3000)
    parts, incl, seeds, root_part, ref = split_parts(sc, 3, 9, 0)
    b = d.EmatBackend(sc.num_sites, trace_moves=64)
    b.set_option("parts_per_cu", 16)
    tally, cov = Tally("device"), M.Coverage()
    try:
        configure(b, sc, ref, parts, incl, seeds, root_part, None)
        M.run_stepped(tally, cov, b, sc, parts, incl, ref, X.Evo.of(sc), X.Pop(sc.pop), 40, tag="side class")
        side = np.flatnonzero(~np.asarray(b.main_class_mask(len(parts)), bool)).tolist()
    finally:
        b.close()
    _done[("side class", True)] = (tally, cov, dict(M.step_chain.cost))
    record_property("side_class_parts", side)
    _report(record_property, cov, M.step_chain.cost)
    tally.finish(record_property)
    assert [p for p in side if p != root_part], "no part other than the root part (%d) ran in a side class: %s" % (root_part, side)
    assert cov.unchecked == 0 and sum(cov.accepted) >= 30, cov.as_dict()


def test_device_tree_resident_in_hbm_every_move_across_two_cycles(record_property):
    """The run driver with the tree resident in HBM (C3, 700 tips, site rates, 24 parts cut and their tables built by kernels):
    30 single-move passes over every part in each of two cycles."""
    sc = make_scenario("C3", num_tips=700, num_sites=3000, uncertain_tips=0.2)
    nu = 0.25 + 1.5 * np.random.default_rng(3).random(sc.num_sites)
    ev, pop = X.Evo.of(sc, nu), X.Pop(sc.pop)
    b = d.EmatBackend(sc.num_sites, trace_moves=64)
    run = d.EmatRun(b, sc.tree, sc.ref, 71)
    run.set_num_parts(24); run.set_hky(sc.mu, sc.kappa, sc.pi, nu); run.set_pop_model(sc.pop)
    run.set_device_tree(True)
    tally, cov = Tally("device"), M.Coverage()
    try:
        for cyc in range(2):
            _, ref = run.tree()
            run.repartition()
            n, root_part = run.num_parts()

            def advance(e):
                run.run_moves(n); e.synchronize()
            M.run_stepped(tally, cov, b, sc, list(range(n)), [p == root_part for p in range(n)], ref, ev, pop, 30, tag="cycle %d" % cyc, advance=advance)
            run.reassemble()
    finally:
        run.close(); b.close()
    _done[("hbm tree", True)] = (tally, cov, dict(M.step_chain.cost))
    _report(record_property, cov, M.step_chain.cost)
    tally.finish(record_property)
    assert cov.unchecked == 0 and sum(cov.accepted) >= 500, cov.as_dict()


def test_device_cases_cover_what_they_must(record_property):
    total = M.Coverage()
    for name in CASES:
        for use_lds in (True, False):
            total.add(_run(name, use_lds)[1])
    for key in (("side class", True), ("hbm tree", True)):
        if key in _done:
            total.add(_done[key][1])
    _report(record_property, total)
    print("coverage:", total.as_dict())
    total.assert_conditions()
