"""The run driver's Exponential population moves (emat_run_set_exp_pop_moves, emat_run_exp_pop_moves, emat_run_get_exp_pop), tree on the host and in
HBM: a call's prior against exact_model on the downloaded tree under the returned model, the parts' coalescent tables built from the NEW model, whole
cycles with the group on, the state rule, and nothing moving when the group is off."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
from delphy_amd.scenarios import make_scenario
from test_exact_model import Tally, check_popsize_bar

pytestmark = pytest.mark.gpu

SPEC = d.ExpPopSpec(inv_n0_prior_alpha=1.0, inv_n0_prior_beta=50.0, g_min=-0.05, g_max=0.05, rounds=50)
T_STEP = 9.0


@pytest.fixture(scope="module")
def scenario():
    sc = make_scenario("C2", num_tips=100, num_sites=800, uncertain_tips=0.2)
    assert sc.pop.kind == 1 and sc.pop.p[3] > 0.0
    return sc


def _run(sc, device_tree, on, seed=71):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(5); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_coalescent_t_step(T_STEP); run.set_device_tree(device_tree)
    if on:
        run.set_exp_pop_moves(True, SPEC)
    return b, run


def _same_tree(a, b):
    (ta, ra), (tb, rb) = a, b
    return np.array_equal(ra, rb) and all(np.array_equal(getattr(ta, f), getattr(tb, f)) for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t"))


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_a_call_moves_the_model_and_the_next_repartition_builds_from_it(scenario, device_tree, record_property):
    sc = scenario
    b1, run = _run(sc, device_tree, True)
    b2, still = _run(sc, device_tree, False)
    tally = Tally("device")
    try:
        assert run.exp_pop() == (sc.pop.p[1], sc.pop.p[2])
        res = run.exp_pop_moves(trace=True)
        n0, g = run.exp_pop()
        assert (n0, g) == (res.n0, res.g) and res.n0_accepted + res.g_accepted >= 1 and (n0, g) != (sc.pop.p[1], sc.pop.p[2])
        assert len(res.trace) == 100 and np.all(res.trace["evaluated"][0::2] == 1)
        new_pm = d.PopModel.exp(sc.pop.p[0], n0, g, sc.pop.p[3])
        tree, _ = run.tree()
        t_ref = run.t_max_tip()
        tally.check("log_coalescent_prior_end", X.scalable_log_prior(tree, X.Pop(new_pm), t_ref, T_STEP), res.log_coalescent_prior_end, "after the call")
        tally.check("log_coalescent_prior_start", X.scalable_log_prior(tree, X.Pop(sc.pop), t_ref, T_STEP), res.log_coalescent_prior_start, "before the call")
        run.repartition(); still.repartition()
        with pytest.raises(d.EmatError, match="STATE"):
            run.exp_pop_moves()                                            # the parts are out
        n, _ = run.num_parts()
        for p in range(n):                                                 # the parts' tables are the NEW model's
            check_popsize_bar(tally, b1, p, X.Pop(new_pm), "after the call")
        b1.recalc_derived(); b2.recalc_derived()
        assert b1.totals()[0] == b2.totals()[0] and b1.totals()[1] != b2.totals()[1]      # the same tree of parts under another population model
        run.run_moves(20 * sc.tree.num_nodes)
        b1.check_derived()                                                 # what the moves maintained under the new model against its recomputation
        run.reassemble(); still.reassemble()
    finally:
        run.close(); still.close(); b1.close(); b2.close()
    tally.finish(record_property)


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_whole_cycles_with_the_group_on(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b, run = _run(sc, device_tree, True)
    try:
        seen = [run.exp_pop()]
        for _ in range(3):
            run.do_mcmc_steps(per_cycle, per_cycle)
            seen.append(run.exp_pop())
        assert len(set(n0 for n0, _ in seen)) == 4 and len(set(g for _, g in seen)) >= 2
        assert all(np.isfinite(v) and n0 > 0 and SPEC.g_min <= g <= SPEC.g_max for n0, g in seen for v in (n0, g))
        assert run.tree()[0].num_nodes == sc.tree.num_nodes
    finally:
        run.close(); b.close()


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_with_the_group_off_five_cycles_are_bit_for_bit_the_parents(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, off = _run(sc, device_tree, False)
    b2, never = _run(sc, device_tree, False)
    try:
        off.set_exp_pop_moves(False, SPEC)                                 # the settings are kept, the group stays off
        for _ in range(5):
            off.do_mcmc_steps(per_cycle, per_cycle); never.do_mcmc_steps(per_cycle, per_cycle)
            assert _same_tree(off.tree(), never.tree())
        assert off.exp_pop() == (sc.pop.p[1], sc.pop.p[2])
        off.repartition(); never.repartition()
        b1.recalc_derived(); b2.recalc_derived()
        assert b1.totals() == b2.totals() and all(np.isfinite(v) for v in b1.totals())
        off.reassemble(); never.reassemble()
    finally:
        off.close(); never.close(); b1.close(); b2.close()


def test_refusals_of_the_driver(scenario):
    sc = scenario
    b, run = _run(sc, True, False)
    try:
        for bad in (dict(g_prior_scale=0.0), dict(g_min=1.0, g_max=-1.0), dict(rounds=-1), dict(inv_n0_prior_beta=float("nan"))):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
                run.set_exp_pop_moves(True, d.ExpPopSpec(**bad))
        run.set_exp_pop_moves(True, d.ExpPopSpec(g_min=0.1, g_max=0.2))
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*outside"):
            run.exp_pop_moves()                                            # the run's g lies outside the bounds: the engine's own refusal
        for pm in (d.PopModel.const(100.0), d.PopModel.skygrid([sc.t_max_tip - 100.0, sc.t_max_tip], [5.0, 6.0])):
            run.set_pop_model(pm)
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*exponential"):
                run.exp_pop_moves()
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*exponential"):
                run.do_mcmc_steps(10, 10)                                  # the group is on: the cycle's round refuses
            with pytest.raises(d.EmatError, match="STATE"):
                run.exp_pop()
    finally:
        run.close(); b.close()
