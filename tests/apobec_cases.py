"""The APOBEC (mpox) model as the tests of the LOCAL moves hold it: one owner for the model over a scenario's tree and for the cases that
test_apobec_moves.py (the oracle) and test_apobec_moves_gpu.py (the device) step move by move against the exact posterior.

What sets this model apart from every HKY model of the suite (DESIGN section 3 chose pi = (0.31, 0.19, 0.21, 0.29) to stay clear of it): partition 0 is
Jukes-Cantor, every escape rate exactly 1; in partition 1 A and T leave at exactly 1 and C and G at exactly 1 + 2 rho.  Re-timing a mutation
between two states of the same escape rate leaves log G as it is, so most branch reforms have a log_mh of exactly 0 -- the Metropolis tie, which
is accepted without a uniform.  The partition map comes from the sequence context and is irregular, and pi is flat."""
import numpy as np

import exact_model as X
import move_steps as M
from delphy_amd.engine import mpox_q_matrices
from delphy_amd.scenarios import make_scenario
from helpers import configure, split_parts
from test_exact_model import Tally
from test_mpox_run_host import apobec_partition, tip0_sequence


def apobec_evo(sc, rho):
    """(mu [2], pi [2][4], q [2][4][4], partition_for_site [L]): the APOBEC model at rho = mu* / mu over the scenario's tree, the site partition drawn
    from the sequence at node 0 as the run driver draws it."""
    pfs = apobec_partition(tip0_sequence(sc.tree, sc.ref)[0])
    assert 0 < pfs.sum() < sc.num_sites
    return np.array([sc.mu, sc.mu]), np.full((2, 4), 0.25), np.stack(mpox_q_matrices(rho)), pfs


def c1_40():
    return make_scenario("C1", num_tips=40, num_sites=1000, uncertain_tips=0.3, seed=77)


def gapped():
    from test_study_model import _gapped
    return _gapped()[0]


# name -> (scenario, rho, parts, the seed of the cut, single-move passes)
CASES = {
    "apobec/1": (c1_40, 20.0, 1, 3, 300),
    "apobec/3": (c1_40, 0.5, 3, 5, 250),
    "apobec-gapped": (gapped, 0.5, 2, 7, 200),
}


def missations_with_from_states_per_partition(tree, pfs):
    """How many (site, state) entries of the tree's missations-with-from-states fall in each of the two partitions."""
    sites = np.asarray(tree.mfs_site[: int(tree.mfs_offset[-1])], np.int64)
    return [int(np.sum(np.asarray(pfs)[sites] == p)) for p in (0, 1)]


def prepare(name):
    """-> (sc, parts, incl, ref, evo, Evo, Pop, steps, setup(engine)), as test_move_steps.prepare does for its cases."""
    make, rho, nparts, seed, steps = CASES[name]
    sc = make()
    evo = apobec_evo(sc, rho)
    parts, incl, seeds, root_part, ref = split_parts(sc, nparts, seed)
    assert len(parts) == nparts, (name, len(parts))

    def setup(engine):
        configure(engine, sc, ref, parts, incl, seeds, root_part, sc.default_t_step(), evo=evo)
        return engine
    return sc, parts, incl, ref, evo, X.Evo.of(sc, None, evo), X.Pop(sc.pop), steps, setup


class TieTally(Tally):
    """A Tally that also counts the accepted branch reforms whose exact log_mh has S = 0 -- no term of log G differs between the two histories, a
    Metropolis tie -- and those of them whose log_mh the engine reported as anything but 0.0 (+0.0 or -0.0)."""

    def __init__(self, who):
        super().__init__(who)
        self.tied_reforms = self.tied_reforms_not_zero = 0
        # A branch WITH mutations whose exact log_mh is 0 -- every state the re-timed mutations pass through leaves at the same rate: [reported as
        # 0.0, as a negative number, as a positive one].  Both engines form it as the difference of two sums over the branch's mutations: each
        # mutation's rate term is 0 (t - t_P) = 0 exactly, and the log(mu q_ab) terms are the same numbers added in another order, which may round
        # differently, so 0.0 is what nearly always comes out (all 76 over CASES on the oracle) but not what the algorithm promises: these are held to
        # the model's bound like any other reform, and the device's three counts to the oracle's (a tie on the other side of 0 draws, or does
        # not draw, the acceptance uniform).
        self.zero_valued_reforms_with_mutations = [0, 0, 0]

    def check(self, what, ex, got, where="", allowance=0.0):
        if what == TIE and not ex.S:
            assert ex.value == 0
            self.tied_reforms += 1
            if not float(got) == 0.0:
                self.tied_reforms_not_zero += 1
                self.fail.append("%s %s %s: log_mh %r of a tie (S = 0), exactly 0.0 wanted" % (self.who, what, where, float(got)))
        elif what == TIE and ex.value == 0:
            self.zero_valued_reforms_with_mutations[0 if float(got) == 0.0 else 1 if float(got) < 0.0 else 2] += 1
        super().check(what, ex, got, where, allowance)


TIE = "log_mh_branch_reform"


def run_case(name, make_engine, who, steps=None):
    """Step the case on make_engine(num_sites, trace) and hold every move (move_steps.run_stepped) -> (TieTally, Coverage)."""
    sc, parts, incl, ref, evo, ev, pop, case_steps, setup = prepare(name)
    steps = case_steps if steps is None else steps
    tally, cov = TieTally(who), M.Coverage()
    eng = setup(make_engine(sc.num_sites, steps + 8))
    try:
        M.run_stepped(tally, cov, eng, sc, parts, incl, ref, ev, pop, steps, tag=name)
    finally:
        eng.close()
    return tally, cov


# What the oracle reaches over CASES (test_apobec_moves.py asserts it of the oracle; the device runs the same chains and must reach the same)
MIN_ACCEPTED_PER_KIND, MIN_SPR1_HELD, MIN_SLIDES_HELD, MIN_TIED_REFORMS = 1, 10, 3, 100


def assert_conditions(done, record_property=None):
    """`done`: {case: (TieTally, Coverage)} over all of CASES.  The conditions that keep the two files honest."""
    total, ties, not_zero, worst, zv = M.Coverage(), 0, 0, 0.0, [0, 0, 0]
    for name in CASES:
        tally, cov = done[name][:2]
        total.add(cov)
        ties += tally.tied_reforms; not_zero += tally.tied_reforms_not_zero
        worst = max(worst, tally.worst_abs.get(TIE, 0.0))
        zv = [x + y for x, y in zip(zv, tally.zero_valued_reforms_with_mutations)]
    d = total.as_dict()
    d.update(tied_reforms=ties, tied_reforms_not_zero=not_zero, worst_abs_where_S_is_0_log_mh_branch_reform=worst, zero_valued_reforms_with_mutations_reported_zero_negative_positive=zv)
    if record_property is not None:
        for k, v in d.items():
            record_property("coverage_" + k, v)
    print("coverage:", d)
    assert total.unchecked == 0, d
    assert min(total.accepted) >= MIN_ACCEPTED_PER_KIND, d
    assert total.accepted_spr1_log_mh_exact == total.accepted[4] >= MIN_SPR1_HELD, d
    assert total.accepted_slides_log_mh_exact == total.accepted[3] >= MIN_SLIDES_HELD, d
    assert ties >= MIN_TIED_REFORMS and not_zero == 0 and worst == 0.0, d
    return d
