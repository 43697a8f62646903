"""Every local move of the HIP engine under the APOBEC (mpox) rate matrices, one at a time, against the exact posterior: the cases of
tests/apobec_cases.py through EmatBackend with the parts staged in LDS and resident in HBM (use_lds), held to move_steps' identities and bounds
and to the coverage the CPU oracle reaches on the same chains (test_apobec_moves.py); and the same stepping ACROSS a change of the model, made
by the APOBEC model's own moves on the statistics of the parts while the parts are out, as the run driver makes it every cycle."""
import numpy as np
import pytest

import apobec_cases as AC
import delphy_amd as d
import exact_model as X
import move_steps as M
from oracle_ffi import OracleEngine
from test_exact_model import check_part

pytestmark = pytest.mark.gpu

_done, _oracle_done = {}, {}
# what the chain alone decides: the device runs the oracle's chains, so these are the oracle's to the last count
CHAIN_FIELDS = ("steps", "accepted", "accepted_root_displacements", "accepted_negative_log_mh", "accepted_outside_root_part", "compound", "compound_accepted",
                "rejected_topology", "unchecked", "accepted_slides_log_mh_exact", "accepted_slide_kinds", "accepted_spr1_log_mh_exact", "accepted_spr1_classes",
                "draws_held", "draws_verdicts_drawn", "draws_bexp", "draws_reforms", "draws_spr1_times", "draws_early_end", "draws_ends_at_once")


def _device(use_lds):
    return lambda num_sites, trace: d.EmatBackend(num_sites, trace_moves=trace, use_lds=use_lds)


def _oracle(name):
    if name not in _oracle_done:
        _oracle_done[name] = AC.run_case(name, lambda num_sites, trace: OracleEngine(num_sites, trace_moves=trace), "oracle")
    return _oracle_done[name]


def _run(name, use_lds):
    key = (name, use_lds)
    if key not in _done:
        _done[key] = AC.run_case(name, _device(use_lds), "device") + (dict(M.step_chain.cost),)
    return _done[key]


@pytest.mark.parametrize("use_lds", [True, False])
@pytest.mark.parametrize("name", list(AC.CASES))
def test_device_every_move_against_the_exact_posterior(name, use_lds, record_property):
    tally, cov, cost = _run(name, use_lds)
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    record_property("tied_reforms", tally.tied_reforms)
    record_property("zero_valued_reforms_with_mutations", tally.zero_valued_reforms_with_mutations)
    print("%s use_lds=%s: accepted %s, tied reforms %d, zero-valued reforms with mutations (0.0, < 0, > 0) %s, %.3f ms per single-move pass, %.3f ms for its read-backs; %s" % (
        name, use_lds, cov.accepted, tally.tied_reforms, tally.zero_valued_reforms_with_mutations, 1e3 * cost["advance_s"] / max(cost["passes"], 1),
        1e3 * cost["read_s"] / max(cost["passes"], 1), tally.summary()))
    tally.finish(record_property)
    assert cov.unchecked == 0, cov.as_dict()
    otally, ocov = _oracle(name)
    got, want = cov.as_dict(), ocov.as_dict()
    assert {f: got[f] for f in CHAIN_FIELDS} == {f: want[f] for f in CHAIN_FIELDS}
    assert tally.tied_reforms == otally.tied_reforms and tally.tied_reforms_not_zero == 0
    assert tally.zero_valued_reforms_with_mutations == otally.zero_valued_reforms_with_mutations


@pytest.mark.parametrize("use_lds", [True, False])
def test_device_cases_cover_what_they_must(use_lds, record_property):
    AC.assert_conditions({name: _run(name, use_lds) for name in AC.CASES}, record_property)


@pytest.mark.parametrize("use_lds", [True, False])
def test_stepping_across_a_change_of_the_model(use_lds, record_property):
    """apobec/3 with the parts out: 80 moves a part under the model configured, then the APOBEC model's moves on the parts' statistics install another mu and
    another q1 (ten Gibbs rounds), then 80 more moves a part.  Between the two nothing is called but reads: the first of them finds the maintained
    quantities marked as the old model's and runs the recalculation run_moves itself would run.  That recalculation is held from scratch -- log G, every
    lambda_i -- to the exact values under the NEW model, and every move after it as the moves before: a table of log(mu q_ab) staged from the old model,
    a remembered rate change across a node's missations, or a cumulative rate of the reference sequence left from the old model would show here."""
    sc, parts, incl, ref, evo, ev0, pop, _, setup = AC.prepare("apobec/3")
    tally, cov = AC.TieTally("device"), M.Coverage()
    b = setup(_device(use_lds)(sc.num_sites, 200))
    try:
        M.run_stepped(tally, cov, b, sc, parts, incl, ref, ev0, pop, 80, tag="before the change")
        before = cov.as_dict()
        r = b.parts_mpox_moves(d.MpoxSpec(mu=sc.mu, mu_star=0.5 * sc.mu, rounds=10), key=93)
        mu, pi, q = b.get_evo()
        assert mu.tolist() == [r.mu, r.mu] and r.mu != sc.mu and not np.array_equal(q[1], evo[2][1]) and np.array_equal(q[0], evo[2][0])
        assert abs(r.mu / sc.mu - 1.0) > 1e-3 and abs(r.mu_star / r.mu - 0.5) > 1e-3       # (a change the bounds below resolve many times over)
        ev1 = X.Evo(mu, pi, q, np.ones(sc.num_sites), evo[3])
        for p in range(len(parts)):
            check_part(tally, b, p, ref, ev1, pop, incl[p], "after the change", moves=80)      # (k_bar_p is the 80 moves' own: the recalculation leaves it)
        M.run_stepped(tally, cov, b, sc, parts, incl, ref, ev1, pop, 80, tag="after the change")
    finally:
        b.close()
    after = cov.as_dict()
    for k, v in after.items():
        record_property("coverage_" + k, v)
    print("use_lds=%s: accepted %s before the change, %s in all; %s" % (use_lds, before["accepted"], after["accepted"], tally.summary()))
    tally.finish(record_property)
    assert cov.unchecked == 0 and cov.steps == 2 * 80 * len(parts), after
    # (of 240 moves after the change the oracle's chains of apobec/3 accept some 40, 50 and 110 of the three simple kinds; topology moves are held when they come)
    assert all(y - x >= 10 for x, y in zip(before["accepted"][:3], after["accepted"][:3])), (before["accepted"], after["accepted"])
    assert after["accepted_spr1_log_mh_exact"] == after["accepted"][4] and after["accepted_slides_log_mh_exact"] == after["accepted"][3], after
