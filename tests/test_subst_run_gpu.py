"""The run driver's substitution-model moves (emat_run_set_subst_moves, emat_run_subst_moves, emat_run_get_hky) on a 200-tip tree, on the host and in
HBM: every round's key is keyed_round's, the accepted model becomes the run's and the backend's, the round comes before the site-rate round as in
the reference, nothing moves with the group off, and the refusals."""
import numpy as np
import pytest

import delphy_amd as d
import skygrid_streams as RS
from delphy_amd.scenarios import make_scenario

pytestmark = pytest.mark.gpu

SPEC = d.SubstSpec(mu_prior_alpha=1.0, mu_prior_beta=0.0, rounds=10)
KEY_TAG = 0x5355425354303031     # csrc/emat_run.cpp: "SUBST001"
SEED = 73


@pytest.fixture(scope="module")
def scenario():
    return make_scenario("C2", num_tips=200, num_sites=3000, uncertain_tips=0.2)


def _run(sc, device_tree, on, seed=SEED):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(6); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(device_tree)
    if on:
        run.set_subst_moves(True, SPEC)
    return b, run


def _round_key(k, seed=SEED):
    """keyed_round: the first 64-bit word of Philox4x32-10(counter = rounds so far, key = run seed ^ the group's tag)."""
    w = RS.philox4x32_10(np.uint64(k), np.uint64(seed ^ KEY_TAG))
    return int(w[0]) | (int(w[1]) << 32)


def _same_tree(a, b):
    (ta, ra), (tb, rb) = a, b
    return np.array_equal(ra, rb) and all(np.array_equal(getattr(ta, f), getattr(tb, f)) for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t"))


def _same_result(a, b):
    return np.array_equal(a.trace, b.trace) and a.pi.tolist() == b.pi.tolist() and all(getattr(a, f) == getattr(b, f) for f in (
        "mu", "kappa", "mu_draw", "mu_post_shape", "mu_post_rate", "delta_log_G", "delta_log_other_priors", "pi_accepted", "kappa_accepted", "pi_left_unit", "forced_rejections"))


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_the_model_moves_over_cycles_and_every_rounds_key_is_keyed_rounds(scenario, device_tree):
    """Three cycles made by hand on two runs of one seed: one through the driver's round, one through the backend's own call under the key the driver
    must have drawn, from the model the driver held.  Results, models and trees stay equal bit for bit."""
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, run = _run(sc, device_tree, True)
    b2, byhand = _run(sc, device_tree, False)
    try:
        assert run.hky()[:2] == (sc.mu, sc.kappa)
        seen = [run.hky()]
        for k in range(3):
            run.repartition(); byhand.repartition()
            mu, kappa, pi = byhand.hky()
            res = run.subst_moves(trace=True)
            want = b2.parts_subst_moves(d.SubstSpec(mu=mu, kappa=kappa, pi=tuple(pi), mu_prior_alpha=SPEC.mu_prior_alpha, mu_prior_beta=SPEC.mu_prior_beta, rounds=SPEC.rounds), key=_round_key(k), trace=True)
            assert _same_result(res, want), k
            assert len(res.trace) == 2 * SPEC.rounds
            got = run.hky()
            assert (got[0], got[1], got[2].tolist()) == (res.mu, res.kappa, res.pi.tolist())          # the accepted values are the run's ...
            for b in (b1, b2):                                                                         # ... and the backend's, on its one partition
                hm, hp, hq = b.get_evo()
                assert hm.tolist() == [res.mu] and hp[0].tolist() == res.pi.tolist()
            assert np.array_equal(b1.get_evo()[2], b2.get_evo()[2])
            byhand.set_hky(res.mu, res.kappa, res.pi)                                                  # what the driver does for itself; the next push derives the same q
            seen.append(got)
            run.run_moves(per_cycle); byhand.run_moves(per_cycle)
            run.reassemble(); byhand.reassemble()
            assert _same_tree(run.tree(), byhand.tree()), k
        assert len(set(m for m, _, _ in seen)) == 4 and len(set(kp for _, kp, _ in seen)) >= 2 and len(set(tuple(p.tolist()) for _, _, p in seen)) >= 2
        assert all(np.isfinite(m) and m > 0 and kp > 0 and np.all(p > 0) and abs(p.sum() - 1.0) < 1e-9 for m, kp, p in seen)
    finally:
        run.close(); byhand.close(); b1.close(); b2.close()


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_the_next_push_sends_the_accepted_model(scenario, device_tree):
    sc = scenario
    b, run = _run(sc, device_tree, True)
    try:
        run.repartition()
        res = run.subst_moves()
        held = [x.copy() for x in b.get_evo()]
        run.push_params()                                                      # the whole model again, from the driver's copy
        assert all(np.array_equal(x, y) for x, y in zip(held, b.get_evo()))
        assert held[0].tolist() == [res.mu]
        b.recalc_derived()
        assert all(np.isfinite(v) for v in b.totals())
        run.reassemble()
    finally:
        run.close(); b.close()


def _cycle_by_hand(run, per_cycle, order):
    run.repartition()
    for what in order:
        (run.subst_moves if what == "subst" else run.site_rate_moves)()
    run.run_moves(per_cycle)
    run.reassemble()


def test_the_round_comes_before_the_site_rate_round(scenario):
    """By result: a cycle of do_mcmc_steps with both groups on is, bit for bit, the cycle made by hand in the reference's order (run.cpp:703-732) --
    the site-rate round's Ttwiddle_l = sum_a q_a T_a is made from the NEW q -- and not the cycle made in the other order."""
    sc = scenario
    per_cycle = 10 * sc.tree.num_nodes
    made = {}
    for how in ("driver", "subst first", "site rates first"):
        b, run = _run(sc, True, True)
        try:
            run.set_site_rate_moves(True, 1.0)
            if how == "driver":
                run.do_mcmc_steps(per_cycle, per_cycle)
            else:
                _cycle_by_hand(run, per_cycle, ("subst", "rates") if how == "subst first" else ("rates", "subst"))
            made[how] = (run.hky(), run.site_rates(), run.tree())
        finally:
            run.close(); b.close()
    (h0, s0, t0), (h1, s1, t1), (h2, s2, t2) = made["driver"], made["subst first"], made["site rates first"]
    assert (h0[0], h0[1], h0[2].tolist()) == (h1[0], h1[1], h1[2].tolist()) and s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and _same_tree(t0, t1)
    assert not np.array_equal(s0[1], s2[1])                                           # the same keys, but the site-rate round read the old mu and q there


def test_the_site_rate_rounds_Ttwiddle_l_is_made_from_the_new_q(scenario):
    sc = scenario
    b, run = _run(sc, True, True)
    try:
        run.repartition()
        before = run.Ttwiddle_l()
        q_before = b.get_evo()[2][0]
        res = run.subst_moves()
        after = run.Ttwiddle_l()
        q_after = b.get_evo()[2][0]
        assert res.pi_accepted + res.kappa_accepted >= 1 and not np.array_equal(q_before, q_after)
        # a site no mutation or missation touches spends the whole tree in its reference state: Ttwiddle_l = q_ref(l) x tree length
        ratio = after / before
        want = [(-q_after[a, a]) / (-q_before[a, a]) for a in range(4)]
        near = [int(np.sum(np.abs(ratio - w) < 1e-9 * w)) for w in want]
        assert sum(near) > 0.5 * sc.num_sites, near                                   # most sites; the others mix two states' rates
        run.reassemble()
    finally:
        run.close(); b.close()


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_with_the_group_off_cycles_are_bit_for_bit_those_of_a_run_that_never_heard_of_it(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, off = _run(sc, device_tree, False)
    b2, never = _run(sc, device_tree, False)
    try:
        off.set_subst_moves(False, SPEC)                                   # the settings are kept, the group stays off
        for _ in range(4):
            off.do_mcmc_steps(per_cycle, per_cycle); never.do_mcmc_steps(per_cycle, per_cycle)
            assert _same_tree(off.tree(), never.tree())
        mu, kappa, pi = off.hky()
        assert (mu, kappa, pi.tolist()) == (sc.mu, sc.kappa, list(sc.pi))
        off.repartition(); never.repartition()
        b1.recalc_derived(); b2.recalc_derived()
        assert b1.totals() == b2.totals() and all(np.isfinite(v) for v in b1.totals())
        assert all(np.array_equal(x, y) for x, y in zip(b1.get_evo(), b2.get_evo()))
        off.reassemble(); never.reassemble()
    finally:
        off.close(); never.close(); b1.close(); b2.close()


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_an_assembled_tree_and_a_sharded_run_are_refused(scenario, device_tree):
    sc = scenario
    b, run = _run(sc, device_tree, True)
    try:
        with pytest.raises(d.EmatError, match="STATE.*repartition first"):
            run.subst_moves()                                              # nothing cut yet
        run.repartition()
        first = run.subst_moves()
        run.reassemble()
        with pytest.raises(d.EmatError, match="STATE.*repartition first"):
            run.subst_moves()                                              # assembled again
        assert run.hky()[0] == first.mu                                    # a refusal draws no key and moves nothing
        run.repartition()
        second = run.subst_moves()
        assert second.mu_draw != first.mu_draw                             # round 1's key, not round 0's again
        run.reassemble()
    finally:
        run.close(); b.close()
    b, run = _run(sc, False, True)
    try:
        run.set_shard(0, 2)
        run.repartition()
        with pytest.raises(d.EmatError, match="STATE.*sharded run"):
            run.subst_moves()
    finally:
        run.close(); b.close()
