"""The run driver's Skygrid round (emat_run_set_skygrid_moves, emat_run_skygrid_moves, emat_run_get_skygrid), tree on the host and in HBM: whole
cycles bit for bit the hand-driven sequence, the parts' coalescent tables built from the NEW curve, the state rule, and nothing moving when the
group is off."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
from delphy_amd.scenarios import make_scenario
from test_exact_model import Tally, check_popsize_bar

pytestmark = pytest.mark.gpu

SPEC = d.SkygridSpec(tau=2.0, low_gamma_barrier_enabled=True, low_gamma_barrier_loc=0.0)


@pytest.fixture(scope="module")
def scenario():
    sc = make_scenario("C3", num_tips=600, num_sites=2000, uncertain_tips=0.2, skygrid_log_linear=True)
    assert sc.pop.kind == 2
    return sc


def _run(sc, device_tree, on, seed=71):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(12); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(device_tree)
    if on:
        run.set_skygrid_moves(True, SPEC)
    return b, run


def _same_tree(a, b):
    (ta, ra), (tb, rb) = a, b
    return np.array_equal(ra, rb) and all(np.array_equal(getattr(ta, f), getattr(tb, f)) for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t"))


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_three_cycles_are_the_hand_driven_sequence_bit_for_bit(scenario, device_tree, record_property):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, auto = _run(sc, device_tree, True)
    b2, hand = _run(sc, device_tree, True)
    tally = Tally("device")
    try:
        assert np.array_equal(auto.skygrid()[0], sc.pop.skygrid_gamma) and auto.skygrid()[1] == SPEC.tau
        auto.do_mcmc_steps(3 * per_cycle, per_cycle)
        curves = []
        for cycle in range(3):
            res = hand.skygrid_moves(trace=True)                               # moves, repartition, local moves, reassemble
            g, tau = hand.skygrid()
            assert np.array_equal(g, res.gamma) and tau == res.tau and res.hmc_steps_done >= 1
            curves.append(g.copy())
            hand.repartition()
            with pytest.raises(d.EmatError, match="STATE"):
                hand.skygrid_moves()                                           # the parts are out
            if cycle == 0:                                                     # the parts' tables are the NEW curve's
                pop = X.Pop(d.PopModel.skygrid(sc.pop.skygrid_x, g, True))
                n, _ = hand.num_parts()
                for p in range(n):
                    check_popsize_bar(tally, b2, p, pop, "after the round")
            hand.run_moves(per_cycle)
            hand.reassemble()
        assert not np.array_equal(curves[0], sc.pop.skygrid_gamma) and not np.array_equal(curves[0], curves[1])
        hand.do_mcmc_steps(0, per_cycle)                                       # (no cycle: what do_mcmc_steps does at its end, the host tree's root normalised)
        ga, ta = auto.skygrid(); gh, th = hand.skygrid()
        assert np.array_equal(ga, gh) and ta == th
        assert _same_tree(auto.tree(), hand.tree())
    finally:
        auto.close(); hand.close(); b1.close(); b2.close()
    tally.finish(record_property)


@pytest.mark.parametrize("device_tree", [False, True], ids=["host tree", "tree in HBM"])
def test_with_the_group_off_nothing_new_happens(scenario, device_tree):
    sc = scenario
    per_cycle = 20 * sc.tree.num_nodes
    b1, off = _run(sc, device_tree, False)
    b2, never = _run(sc, device_tree, False)
    try:
        off.set_skygrid_moves(False, SPEC)                                     # the settings are kept, the group stays off
        off.do_mcmc_steps(2 * per_cycle, per_cycle); never.do_mcmc_steps(2 * per_cycle, per_cycle)
        g, tau = off.skygrid()
        assert np.array_equal(g, sc.pop.skygrid_gamma) and tau == SPEC.tau
        assert _same_tree(off.tree(), never.tree())
    finally:
        off.close(); never.close(); b1.close(); b2.close()


def test_refusals_of_the_driver(scenario):
    sc = scenario
    b, run = _run(sc, True, False)
    try:
        for bad in (dict(tau=0.0), dict(tau=float("nan")), dict(hmc_steps=-1), dict(hmc_mean_dt=0.0), dict(low_gamma_barrier_enabled=True, low_gamma_barrier_scale=0.0)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
                run.set_skygrid_moves(True, d.SkygridSpec(**bad))
        run.set_pop_model(d.PopModel.const(100.0))
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*Skygrid"):
            run.skygrid_moves()
        with pytest.raises(d.EmatError, match="STATE"):
            run.skygrid()
    finally:
        run.close(); b.close()
