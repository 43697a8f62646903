"""What the three groups of global moves (site rates, Skygrid, Exponential population) share: the resident tree's refusals against the table recorded
from the library BEFORE the groups' rules got one owner each (tests/golden/make_global_moves_refusals.py tree), the scratch a handle keeps from
call to call, whichever group or source of statistics used it last, and the run driver's round keys."""
import dataclasses
import json
import os

import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario
from test_tree_stages_gpu import _status

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_moves_refusals.json")
TIPS, SITES = 33, 300
SKY_SPEC = d.SkygridSpec(tau=2.0, low_gamma_barrier_enabled=True, hmc_steps=5)
XP_SPEC = d.ExpPopSpec(inv_n0_prior_alpha=1.0, inv_n0_prior_beta=50.0, rounds=4)


@pytest.fixture(scope="module")
def scenario():
    return make_scenario("C1", num_tips=TIPS, num_sites=SITES)


def _grid(sc, cells=7):
    """(t_ref, t_step) that lay `cells` cells over the tree, the last one ending after the latest tip."""
    t = np.asarray(sc.tree.t)
    t_ref = float(t.max())
    return t_ref, (t_ref - float(t.min())) / (cells - 1.5)


def _models(sc):
    t = np.asarray(sc.tree.t)
    curve = d.PopModel.skygrid(np.linspace(t.min() - 1.0, t.max(), 9), 4.0 + 0.5 * np.sin(np.arange(9.0)), True)
    return curve, d.PopModel.exp(float(t.max()), 3.0, 2.0 / float(t.max() - t.min()), 0.5)


# ---- refusals by tree state and by grid ----------------------------------------------------------------------------------------------------
def _tree_calls(b, sc, t_ref, t_step):
    curve, growth = _models(sc)
    return {"emat_tree_coalescent_stats": lambda: b.tree_coalescent_stats(t_ref, t_step),
            "emat_tree_skygrid_moves": lambda: b.tree_skygrid_moves(curve, SKY_SPEC, t_ref, t_step, key=3),
            "emat_tree_exp_pop_moves": lambda: b.tree_exp_pop_moves(growth, XP_SPEC, t_ref, t_step, key=3)}


def record_tree_refusals():
    """{state or grid: {entry point: [status, last_error or ""]}} of the three calls on the resident tree's statistics."""
    sc = make_scenario("C1", num_tips=TIPS, num_sites=SITES)
    t_ref, t_step = _grid(sc)
    span = t_ref - float(np.asarray(sc.tree.t).min())
    grids = {"no tree": (t_ref, t_step), "tree home": (t_ref, t_step), "parts out": (t_ref, t_step),
             "more than 2^22 cells": (t_ref, span / ((1 << 22) + 10)), "cell numbers beyond 2^30": (t_ref + ((1 << 30) + 100) * t_step, t_step)}
    table = {}
    for state, grid in grids.items():
        b = d.EmatBackend(sc.num_sites)
        run = None
        try:
            if state == "parts out":
                run = d.EmatRun(b, sc.tree, sc.ref, 3)
                run.set_num_parts(3); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
                run.repartition()
            elif state != "no tree":
                b.tree_upload(sc.tree)
            for name, call in _tree_calls(b, sc, *grid).items():
                st = int(_status(b, call))
                table.setdefault(state, {})[name] = [st, b.last_error() if st != 0 else ""]
        finally:
            if run is not None:
                run.close()
            b.close()
    return table


def test_the_resident_trees_refusals_are_as_recorded():
    want = json.load(open(GOLDEN))["tree"]
    got = record_tree_refusals()
    assert got == want
    assert all(st == 0 for st, _ in want["tree home"].values()) and sum(1 for s in want.values() for st, _ in s.values() if st != 0) == 12


# ---- one handle, every group and both sources of statistics in turn ------------------------------------------------------------------------
def _bits(res):
    """Everything a call returned, as bytes (NaNs and signed zeros included)."""
    if isinstance(res, tuple):
        return [np.asarray(v).tobytes() for v in res]
    fields = dataclasses.asdict(res) if dataclasses.is_dataclass(res) else vars(res)
    return {k: None if v is None else np.asarray(v).tobytes() for k, v in fields.items()}


def _answer(call):
    try:
        return _bits(call())
    except d.EmatError as e:
        return str(e)


def test_one_handle_in_mixed_order_answers_as_fresh_handles_do(scenario):
    sc = scenario
    t_ref, t_step = _grid(sc)
    curve, growth = _models(sc)
    k400 = 1.0 + (np.arange(400) % 7); in400 = -np.linspace(0.005, 3.995, 64)                # 400 cells of 0.01 before t = 0
    wide = d.PopModel.skygrid(np.linspace(-4.5, 0.0, 6), 1.0 + 0.3 * np.cos(np.arange(6.0)), True)
    steps = [
        ("Skygrid on host statistics of 400 cells", lambda b: b.skygrid_moves(wide, SKY_SPEC, 0.0, 0.01, -400, k400, in400, key=11, trace=True)),
        ("Exponential on the tree", lambda b: b.tree_exp_pop_moves(growth, XP_SPEC, t_ref, t_step, key=12, trace=True)),
        ("tree_coalescent_stats", lambda b: b.tree_coalescent_stats(t_ref, t_step)),
        ("Skygrid on the tree", lambda b: b.tree_skygrid_moves(curve, SKY_SPEC, t_ref, t_step, key=13, trace=True)),
        ("Exponential on host statistics of 1 cell and 1 inner node", lambda b: b.exp_pop_moves(growth, XP_SPEC, t_ref, t_step, -3, [2.5], [t_ref - 2.5 * t_step], key=14, trace=True)),
        ("Skygrid with 1 knot", lambda b: b.tree_skygrid_moves(d.PopModel.skygrid([t_ref], [1.0], True), SKY_SPEC, t_ref, t_step, key=15, trace=True)),
        ("Exponential with rounds 0", lambda b: b.tree_exp_pop_moves(growth, dataclasses.replace(XP_SPEC, rounds=0), t_ref, t_step, key=16, trace=True)),
    ]
    one = d.EmatBackend(sc.num_sites)
    try:
        one.tree_upload(sc.tree)
        assert len(one.tree_coalescent_stats(t_ref, t_step)[1]) == 7
        for name, call in steps:
            fresh = d.EmatBackend(sc.num_sites)
            try:
                fresh.tree_upload(sc.tree)
                want = _answer(lambda: call(fresh))
            finally:
                fresh.close()
            assert _answer(lambda: call(one)) == want, name
            assert isinstance(want, str) == (name == "Skygrid with 1 knot"), (name, want)
    finally:
        one.close()


# ---- the site-rate moves' scratch outlives the call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [255, 256, 257])
def test_the_site_rate_scratch_of_an_earlier_call_changes_nothing(L):
    rng = np.random.default_rng(L)
    T = rng.uniform(0.5, 40.0, L); M = rng.poisson(1.5, L).astype(np.int32); pi = [0.3, 0.2, 0.2, 0.3]

    def handle(nu):
        b = d.EmatBackend(L)
        b.set_ref_sequence(np.zeros(L, np.uint8)); b.set_hky(1e-3, 2.0, pi, nu)
        return b
    one = handle(np.ones(L))
    try:
        first = one.site_rate_moves(T, M, 0.8, 10, key=101, trace=True)
        nu1 = one.nu_l()
        assert len(first.trace) == 10 and not np.array_equal(nu1, np.ones(L))
        second = one.site_rate_moves(T, M, first.alpha, 10, key=202, trace=False)
        nu2 = one.nu_l()
    finally:
        one.close()
    fresh = handle(nu1)
    try:
        want = fresh.site_rate_moves(T, M, first.alpha, 10, key=202, trace=False)
        assert _bits(second) == _bits(want) and second.trace is None
        assert nu2.tobytes() == fresh.nu_l().tobytes() and not np.array_equal(nu2, nu1)
    finally:
        fresh.close()


# ---- the run driver's round keys -----------------------------------------------------------------------------------------------------------
GROUPS = {
    "site rates": ("C1", lambda run: run.set_site_rate_moves(True, 1.0), lambda run: (np.float64(run.site_rates()[0]).tobytes(), run.site_rates()[1].tobytes())),
    "Skygrid": ("C3", lambda run: run.set_skygrid_moves(True, SKY_SPEC), lambda run: (run.skygrid()[0].tobytes(), np.float64(run.skygrid()[1]).tobytes())),
    "Exponential": ("C2", lambda run: run.set_exp_pop_moves(True, XP_SPEC), lambda run: np.asarray(run.exp_pop()).tobytes()),
}


def _group_run(sc, switch_on, seed=5):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(2); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
    switch_on(run)
    return b, run


@pytest.mark.parametrize("group", list(GROUPS))
def test_three_cycles_from_one_seed_draw_the_same_parameters_twice(group):
    kind, switch_on, params = GROUPS[group]
    sc = make_scenario(kind, num_tips=TIPS, num_sites=SITES, **(dict(skygrid_log_linear=True) if kind == "C3" else {}))
    per_cycle = 10 * sc.tree.num_nodes
    seen = []
    for _ in range(2):
        b, run = _group_run(sc, switch_on)
        try:
            start = params(run); after = []
            for _cycle in range(3):
                run.do_mcmc_steps(per_cycle, per_cycle)
                after.append(params(run))
            seen.append(after)
            assert after[0] != start and after[1] != after[0] and after[2] != after[1]
        finally:
            run.close(); b.close()
    assert seen[0] == seen[1]


def test_a_refused_round_draws_its_key_again():
    """Three cycles by hand with a round refused in between, because the tree is cut: the curve after each round is the one of three cycles of do_mcmc_steps."""
    _, switch_on, params = GROUPS["Skygrid"]
    sc = make_scenario("C3", num_tips=TIPS, num_sites=SITES, skygrid_log_linear=True)
    per_cycle = 10 * sc.tree.num_nodes
    b1, auto = _group_run(sc, switch_on)
    b2, hand = _group_run(sc, lambda run: run.set_skygrid_moves(False, SKY_SPEC))
    try:
        want, got = [], []
        for cycle in range(3):
            auto.do_mcmc_steps(per_cycle, per_cycle)
            want.append(params(auto))
            hand.skygrid_moves()
            hand.repartition()
            if cycle == 1:
                with pytest.raises(d.EmatError, match="STATE.*reassemble first"):
                    hand.skygrid_moves()
            hand.run_moves(per_cycle); hand.reassemble()
            got.append(params(hand))
        assert got == want and want[2] != want[1]
    finally:
        auto.close(); hand.close(); b1.close(); b2.close()
