"""What the two groups that read the parts' substitution statistics (the substitution-model moves, the APOBEC model's moves) share: the refusals of the three calls on
the parts' statistics by the handle's state, against the table recorded from the library BEFORE the two groups got one frame (tests/golden/make_global_moves_refusals.py
parts); the statistics record and the scratch a handle keeps from call to call, whichever group or source of statistics used them last; the run driver's round keys."""
import dataclasses
import json
import os

import numpy as np
import pytest

import delphy_amd as d
from apobec_cases import apobec_evo
from delphy_amd.scenarios import make_scenario
from helpers import configure, split_parts
from test_global_moves_frame_gpu import _answer, _bits
from test_tree_stages_gpu import _status

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_moves_refusals.json")
TIPS, SITES, PARTS = 33, 300, 3


@pytest.fixture(scope="module")
def scenario():
    return make_scenario("C1", num_tips=TIPS, num_sites=SITES)


@pytest.fixture(scope="module")
def cut(scenario):
    return split_parts(scenario, PARTS, 9)


def _apobec_evo(sc, mu=None, pi=None, q=None):
    """(mu [2], pi [2][4], q [2][4][4], partition_for_site): the APOBEC model at rho = 0.5 over the scenario's tree, or the model given over the same two site partitions."""
    model = apobec_evo(sc, 0.5)
    return model if mu is None else (mu, pi, q, model[3])


def _with_parts(sc, cut, evo=None):
    parts, incl, seeds, root_part, ref = cut
    b = d.EmatBackend(sc.num_sites)
    configure(b, sc, ref, parts, incl, seeds, root_part, evo=evo)
    return b


def _specs(sc, **kw):
    return d.SubstSpec(mu=sc.mu, kappa=sc.kappa, pi=tuple(sc.pi), rounds=2, **kw), d.MpoxSpec(mu=sc.mu, mu_star=0.5 * sc.mu, rounds=2, **kw)


# ---- refusals by the handle's state ---------------------------------------------------------------------------------------------------------
def record_parts_refusals():
    """{state: {entry point: [status, last_error or ""]}} of the three calls on the parts' statistics, in this order on one handle per state."""
    sc = make_scenario("C1", num_tips=TIPS, num_sites=SITES)
    cut = split_parts(sc, PARTS, 9)
    sb, mx = _specs(sc)
    table = {}
    for state in ("no parts", "parts out, 1 partition", "parts out, the APOBEC model", "after reassembly"):
        run = None
        if state == "no parts":
            b = d.EmatBackend(sc.num_sites); b.set_ref_sequence(sc.ref); b.set_hky(sc.mu, sc.kappa, sc.pi)
        elif state == "after reassembly":
            b = d.EmatBackend(sc.num_sites)
            run = d.EmatRun(b, sc.tree, sc.ref, 3)
            run.set_num_parts(PARTS); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(True)
            run.repartition(); run.reassemble()
        else:
            b = _with_parts(sc, cut, _apobec_evo(sc) if "APOBEC" in state else None)
        try:
            calls = {"emat_parts_subst_stats": lambda: b.parts_subst_stats(), "emat_parts_subst_moves": lambda: b.parts_subst_moves(sb, key=3), "emat_parts_mpox_moves": lambda: b.parts_mpox_moves(mx, key=3)}
            for name, call in calls.items():
                st = int(_status(b, call))
                table.setdefault(state, {})[name] = [st, b.last_error() if st != 0 else ""]
        finally:
            if run is not None:
                run.close()
            b.close()
    return table


def test_the_refusals_by_state_are_as_recorded():
    want = json.load(open(GOLDEN))["parts"]
    got = record_parts_refusals()
    assert got == want
    assert all(st != 0 for st, _ in want["no parts"].values())
    assert [want["parts out, 1 partition"][c][0] != 0 for c in ("emat_parts_subst_stats", "emat_parts_subst_moves", "emat_parts_mpox_moves")] == [False, False, True]
    assert all(st == 0 for st, _ in want["parts out, the APOBEC model"].values())


# ---- one handle, both groups and both sources of statistics in turn --------------------------------------------------------------------------
def test_one_handle_in_mixed_order_answers_as_fresh_handles_do(scenario, cut):
    sc = scenario
    sb, mx = _specs(sc)
    ref_handle = _with_parts(sc, cut, _apobec_evo(sc))
    try:
        T, M, Cn = ref_handle.parts_subst_stats(2)
    finally:
        ref_handle.close()
    num_muts = int(M.sum() - np.trace(M, axis1=1, axis2=2).sum())
    assert num_muts > 0 and M[1, 1, 3] + M[1, 2, 0] >= 1
    undrawable = dict(mu_prior_alpha=-(num_muts + 10.0))                                      # shape = num_muts + alpha (- 1) < 0: known only where the parts' statistics are
    sb_bad, mx_bad = _specs(sc, **undrawable)
    steps = [
        ("1 subst on host statistics", lambda b: b.subst_moves(sb, T, M, Cn, key=21, trace=True)),
        ("2 mpox on the parts", lambda b: b.parts_mpox_moves(mx, key=22, trace=True)),
        ("3 parts_subst_stats", lambda b: b.parts_subst_stats(2)),
        ("4 subst on the parts", lambda b: b.parts_subst_moves(sb, key=24, trace=True)),
        ("5 mpox on host statistics", lambda b: b.mpox_moves(mx, 2.0 * T, 3 * M, key=25, trace=True)),
        ("6 mpox with 0 rounds and a trace buffer", lambda b: b.parts_mpox_moves(dataclasses.replace(mx, rounds=0), key=26, trace=True)),
        ("7 subst with 0 rounds", lambda b: b.parts_subst_moves(dataclasses.replace(sb, rounds=0), key=27, trace=True)),
        ("8 mpox with 1 round", lambda b: b.parts_mpox_moves(dataclasses.replace(mx, rounds=1), key=28, trace=True)),
        ("8 mpox with 3 rounds", lambda b: b.parts_mpox_moves(dataclasses.replace(mx, rounds=3), key=28, trace=True)),
        ("9 subst on the parts, the first mu draw refused on the device", lambda b: b.parts_subst_moves(sb_bad, key=29, trace=True)),
        ("9 a good subst call after it", lambda b: b.parts_subst_moves(sb, key=29, trace=True)),
        ("9 mpox on the parts, the first mu draw refused on the device", lambda b: b.parts_mpox_moves(mx_bad, key=30, trace=True)),
        ("9 a good mpox call after it", lambda b: b.parts_mpox_moves(mx, key=30, trace=True)),
    ]
    one = _with_parts(sc, cut, _apobec_evo(sc))
    try:
        for name, call in steps:
            before = one.get_evo()
            fresh = _with_parts(sc, cut, _apobec_evo(sc, *before))                           # the model the handle holds now, the same parts
            try:
                want = _answer(lambda: call(fresh)); want_evo = _bits(fresh.get_evo())
            finally:
                fresh.close()
            assert _answer(lambda: call(one)) == want, name
            assert _bits(one.get_evo()) == want_evo, name
            refused = "refused on the device" in name
            assert isinstance(want, str) == refused, (name, want)
            if refused:
                assert "INVALID_ARGUMENT" in want and "positive shape" in want and _bits(one.get_evo()) == _bits(before), (name, want)
            elif "0 rounds" not in name and name != "3 parts_subst_stats":
                assert _bits(one.get_evo()) != _bits(before), name                            # a call that draws installs a model
    finally:
        one.close()


# ---- the run driver's round keys -------------------------------------------------------------------------------------------------------------
SB_RUN_SPEC, MX_RUN_SPEC = d.SubstSpec(rounds=4), d.MpoxSpec(rounds=4)
GROUPS = {
    "substitution model": (lambda run: run.set_subst_moves(True, SB_RUN_SPEC), lambda run: run.subst_moves(trace=True), lambda run: (np.float64(run.hky()[:2]).tobytes(), run.hky()[2].tobytes())),
    "APOBEC model": (lambda run: run.set_mpox(True, MX_RUN_SPEC), lambda run: run.mpox_moves(trace=True), lambda run: np.float64(run.mpox()).tobytes()),
}


def _group_run(sc, switch_on, seed=5, device_tree=True):
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    run.set_num_parts(2); run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(device_tree)
    switch_on(run)
    return b, run


def _tree_bits(run):
    tree, ref = run.tree()
    return [np.asarray(getattr(tree, f)).tobytes() for f in ("parent", "child0", "child1", "t", "mut_offset", "mut_site", "mut_t")] + [np.asarray(ref).tobytes()]


@pytest.mark.parametrize("group", list(GROUPS))
def test_three_cycles_from_one_seed_draw_the_same_parameters_and_tree_twice(scenario, group):
    sc = scenario
    switch_on, _, params = GROUPS[group]
    per_cycle = 10 * sc.tree.num_nodes
    seen = []
    for _ in range(2):
        b, run = _group_run(sc, switch_on)
        try:
            start = params(run); after = []
            for _cycle in range(3):
                run.do_mcmc_steps(per_cycle, per_cycle)
                after.append(params(run))
            seen.append((after, _tree_bits(run)))
            assert after[0] != start and after[1] != after[0] and after[2] != after[1]
        finally:
            run.close(); b.close()
    assert seen[0] == seen[1]


@pytest.mark.parametrize("group", list(GROUPS))
def test_a_round_refused_on_the_assembled_tree_draws_its_key_again(scenario, group):
    sc = scenario
    switch_on, moves, params = GROUPS[group]
    b1, refused = _group_run(sc, switch_on, device_tree=False)                              # (a host tree's parts stay uploaded after the reassemble: the tree's state alone refuses)
    b2, never = _group_run(sc, switch_on, device_tree=False)
    try:
        with pytest.raises(d.EmatError, match="STATE.*repartition first"):
            moves(refused)                                                                    # nothing cut yet: refused, and no key is drawn
        refused.repartition(); never.repartition()
        refused.reassemble(); never.reassemble()
        with pytest.raises(d.EmatError, match="STATE.*read the parts: repartition first"):
            moves(refused)                                                                    # parts there were, but the tree is assembled again: likewise
        refused.repartition(); never.repartition()
        got, want = moves(refused), moves(never)
        assert _bits(got) == _bits(want) and len(got.trace) > 0
        assert params(refused) == params(never)
        second = moves(never)                                                                 # (the round after it draws another key)
        assert not np.array_equal(second.trace, want.trace)
    finally:
        refused.close(); never.close(); b1.close(); b2.close()
