"""Every local move of the CPU oracle under the APOBEC (mpox) rate matrices, one at a time, against the exact posterior: the cases of
tests/apobec_cases.py through move_steps.run_stepped (its identities and bounds, no other).  test_apobec_moves_gpu.py points the same cases at
the device.  test_move_steps.py's cases are all HKY at pi = (0.31, 0.19, 0.21, 0.29); here two partitions from the sequence context, flat pi,
escape rates that are exactly equal, and so branch reforms whose log_mh is exactly 0: assert_conditions requires at least 100 accepted ones whose
exact log_mh has no differing term (S = 0), and of every one of them that the engine's log_mh IS 0.0.  As the exact model counts its terms, S = 0 says
that the branch has no mutation (470 over the cases); the ties that are this model's own, branches WITH mutations whose re-timing leaves the exact log G
where it was, have S > 0, are 76 over the cases and are counted apart (apobec_cases.TieTally): every one came out as 0.0 on the oracle."""
import numpy as np
import pytest

import apobec_cases as AC
from oracle_ffi import OracleEngine

_done = {}


def _oracle(num_sites, trace):
    return OracleEngine(num_sites, trace_moves=trace)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_the_cases_are_what_they_say(name):
    sc, parts, incl, ref, evo, ev, pop, steps, setup = AC.prepare(name)
    mu, pi, q, pfs = evo
    assert 0 < pfs.sum() < sc.num_sites
    assert np.all(np.diag(q[0]) == -1.0) and q[1][0, 0] == q[1][3, 3] == -1.0 and q[1][1, 1] == q[1][2, 2] < -1.0     # the ties: exactly equal escape rates
    if name == "apobec-gapped":
        per = [AC.missations_with_from_states_per_partition(p, pfs) for p in parts]
        assert min(sum(x[0] for x in per), sum(x[1] for x in per)) >= 1, per


@pytest.mark.parametrize("name", list(AC.CASES))
def test_oracle_every_move_against_the_exact_posterior(name, record_property):
    tally, cov = _done[name] = AC.run_case(name, _oracle, "oracle")
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    record_property("tied_reforms", tally.tied_reforms)
    print(name, "accepted", cov.accepted, "tied reforms", tally.tied_reforms, tally.summary())
    tally.finish(record_property)
    assert cov.unchecked == 0, cov.as_dict()


def test_oracle_cases_cover_what_they_must(record_property):
    for name in AC.CASES:
        if name not in _done:
            _done[name] = AC.run_case(name, _oracle, "oracle")
    AC.assert_conditions(_done, record_property)
