"""Every move of the CPU oracle, one at a time, against the exact posterior (tests/move_steps.py has the identities and the
bounds).  The oracle is the engine under test here, so the identities are proved without a GPU; test_move_steps_gpu.py points
the same cases at the device.

An accepted subtree slide's whole log_mh is one of the identities (move_steps.check_accepted_slide: the four graft numbers of
tests/graft_model.py, the slide's Hastings factor and the exact prior difference).  Over CASES the oracle accepts 60 slides: 54
along the same branch, 4 up past an ancestor and 2 down past the sibling with two or more branches to choose from, 4 of a child
of the run's root, 25 in parts without the run's root; Coverage.assert_conditions requires at least one of each kind.

An accepted SPR1 move's whole log_mh is another (move_steps.check_accepted_spr1: the same graft numbers, the exact prior difference and
log_alpha_n2o - log_alpha_o2n of the two candidate studies of tests/study_model.py, at the scan limit read from the part's random stream).
Over CASES the oracle proposes 297 SPR1 moves and accepts 178, every one of which goes through it (asserted); the rare kinds -- unlimited
scans, root changes, large studies -- are test_study_model.py's.

What a rejected topology move gives back, as this file establishes on the oracle (check_step asserts it of every rejected
subtree slide and SPR1 move of these cases; Coverage counts them): mutation times BIT FOR BIT, except on the sibling branch of a
subtree pruned from under the run's root (reflected about the root's time and back: held to four roundings); lambda_i bit for
bit in most of them, and within its Exact bound where the hops or the rooty graft recomputed it.  test_move_steps_gpu.py asserts
the same of the device.

Every move's draws are held to tests/draws_model.py in the same check_step; Coverage.assert_conditions names the classes and the counts
the oracle reaches over CASES.  DRAW_CASES are the two cases that reach what CASES do not (test_draws_model.py runs them)."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
import move_steps as M
from delphy_amd.scenarios import make_scenario, random_scenario
from helpers import configure, split_parts
from oracle_ffi import OracleEngine
from test_exact_model import CONFIGS, Tally


def high_mutation_scenario():
    """The scenario of test_site_rates_mostly_one_on_branches_of_more_than_32_mutations (test_parity_gpu.py): 14 tips whose
    branches hold more than 32 mutations, the same site more than once on a branch, site rates 1 but for a few sites."""
    import delphy_amd.engine as e
    par = e.SynthParams(num_tips=14, num_sites=6000, tip_span=200.0, pop_n0=2000.0, mu=6e-6, gaps_per_tip=1, mean_gap_len=40, seed=4242)
    par.pi, par.kappa = (0.31, 0.19, 0.21, 0.29), 5.0
    tree, ref, tmax = e.make_synthetic_emat(par)
    sc = make_scenario("C1", num_tips=14, num_sites=6000)
    sc.tree, sc.ref, sc.t_max_tip, sc.mu = tree, ref, tmax, par.mu
    sc.pop = d.PopModel.exp(tmax, 2000.0, 0.0, 0.0)
    nu = np.ones(6000)
    shaped = 0
    for n in range(tree.num_nodes):
        sites = tree.mut_site[tree.mut_offset[n]:tree.mut_offset[n + 1]]
        if sites.shape[0] > 32 and n != tree.root and sites[0] not in sites[32:] and np.all(nu[sites[32:]] == 1.0):
            nu[sites[0]] = 1.7; shaped += 1
    assert shaped >= 2
    return sc, nu


def steep_scenario():
    """21 nodes by hand, 64 sites under Jukes-Cantor at mu = 2^-7 (lambda = 1/2 everywhere).  Two cherries whose nodes have 200 to 400
    days between their parents and their tips (the exact ltr = lambda (b - a) of their displacement is 100 to 200) and whose tips may lie
    anywhere in the 300 days after them (theirs about -150), under a node S that the partition's rule can cut at (a part needs ten nodes
    on either side), so that the steep windows lie in a part WITHOUT the run's root: the copy of the simple moves that is the hot path.
    Above S a ladder of day-long branches with exact-date tips (ltr in between).  Long windows need long branches, and a history sampled
    along one holds lambda T mutations: the branches next to the run's root, which a branch reform re-samples, are a day long, and the
    topology moves are off."""
    from delphy_amd.scenarios import Scenario
    L = ZERO_SLOPE_SITES
    big = 3.4028234663852886e38
    # (name, time, children or None for an exact-date tip, or the (t_min, t_max) of an uncertain one)
    wide = (-400.0, 300.0)
    sub = ("S", -400.0, [("C", -200.0, [("A", 0.0, wide), ("B", 0.0, wide)]),
                         ("M", -399.5, [("M2", -399.3, [("C2", -200.0, [("A2", 0.0, wide), ("B2", 0.0, wide)]), ("T2", -399.1, None)]), ("T", -399.0, None)])])
    top = sub
    for k in range(4, -1, -1):          # the ladder: N4 .. N1 and the root, each with an exact-date tip half a day later
        top = ("N%d" % k, -405.0 + k, [top, ("Q%d" % k, -404.5 + k, None)])
    rows = []

    def walk(node, parent):
        i = len(rows)
        rows.append([parent, -1, -1, node[1], -big, big])
        if isinstance(node[2], list):
            rows[i][1], rows[i][2] = walk(node[2][0], i), walk(node[2][1], i)
        else:
            rows[i][4], rows[i][5] = node[2] if node[2] else (node[1], node[1])
        return i
    walk(top, -1)
    t = d.FlatTree.empty(len(rows), 0, 0, 0)
    t.root = 0
    for i, (par, c0, c1, time, lo, hi) in enumerate(rows):
        t.parent[i], t.child0[i], t.child1[i], t.t[i], t.t_min[i], t.t_max[i] = par, c0, c1, time, lo, hi
    ref = np.random.default_rng(2).integers(0, 4, L).astype(np.uint8)
    return Scenario("two cherries on long stalks", t, ref, 300.0, 2.0 ** -7, 1.0, (0.25, 0.25, 0.25, 0.25), d.PopModel.const(200.0), L)


def on_a_bound_scenario():
    """Two tips by hand whose parent, the run's root, lies one double before them: tip A's date may be anywhere in the ten days before 100,
    so its window is (t_root, 100], two doubles wide, and every time its bounded exponential draws rounds to one end of it: the move ends
    un-noted after the pick and one word.  A population of 2^-40 makes the prior refuse every step of the root further back (the two
    lineages would coexist longer: -1e12 in log per day), so the window stays what it is."""
    from delphy_amd.scenarios import Scenario
    L = ZERO_SLOPE_SITES
    t = d.FlatTree.empty(3, 0, 0, 0)
    t.root = 0
    t.child0[0], t.child1[0] = 1, 2
    t.parent[1] = t.parent[2] = 0
    t.t[:] = (np.nextafter(100.0, -np.inf), 100.0, 100.0)
    big = 3.4028234663852886e38
    t.t_min[:] = (-big, 90.0, 100.0); t.t_max[:] = (big, 100.0, 100.0)
    ref = np.random.default_rng(3).integers(0, 4, L).astype(np.uint8)
    return Scenario("a tip one double below its parent", t, ref, 101.0, 2.0 ** -7, 1.0, (0.25, 0.25, 0.25, 0.25), d.PopModel.const(2.0 ** -40), L)


ZERO_SLOPE_SITES = 64


def zero_slope_scenario():
    """Three tips by hand: the two tips of a cherry miss complementary halves of the sites, the third is an outgroup.  Just below the
    cherry node every site is missing under one child or the other, so d log G / dt of its time is lambda - lambda: the Fraction 0 exactly,
    and with a mutation rate of 2^-10 under Jukes-Cantor the engines' maintained doubles cancel to 0.0 too (the uniform branch)."""
    from delphy_amd.scenarios import Scenario
    L = ZERO_SLOPE_SITES
    t = d.FlatTree.empty(5, 0, 2, 0)
    t.root = 0
    t.child0[0], t.child1[0] = 1, 2
    t.child0[1], t.child1[1] = 3, 4
    t.parent[1] = t.parent[2] = 0; t.parent[3] = t.parent[4] = 1
    t.t[:] = (-100.0, -50.0, 0.0, 0.0, 0.0)
    big = 3.4028234663852886e38
    t.t_min[:] = (-big, -big, 0.0, 0.0, 0.0); t.t_max[:] = (big, big, 0.0, 0.0, 0.0)
    t.miss_offset[:] = (0, 0, 0, 0, 1, 2)
    t.miss_start[:] = (0, L // 2); t.miss_end[:] = (L // 2, L)
    ref = np.random.default_rng(1).integers(0, 4, L).astype(np.uint8)
    return Scenario("cherry of complementary halves", t, ref, 0.0, 2.0 ** -10, 1.0, (0.25, 0.25, 0.25, 0.25), d.PopModel.const(50.0), L)


def _case(name):
    """name -> (scenario, nu_l, evo, num_parts, seed, t_step factor, steps).  Step counts and seeds are chosen so that the
    conditions of Coverage.assert_conditions hold over the file on the oracle."""
    if name.startswith("C"):
        cfg, nparts = name.split("/")
        return CONFIGS[cfg](), None, None, int(nparts), 3 if nparts == "1" else 5, 1.0, STEPS[name]
    if name.startswith("random"):
        case = int(name[6:])
        rng = np.random.default_rng(7100 + case)
        sc, nu_l, evo, _ = random_scenario(rng, case, max_tips=160)
        nparts = int(rng.integers(1, 6))
        return sc, nu_l, evo, nparts, 11 + case, float(rng.choice([0.5, 1.0, 3.0])), STEPS["random"]
    if name.startswith("high-mutation/"):      # (14 tips: one part; two chains from two seeds)
        sc, nu = high_mutation_scenario()
        return sc, nu, None, 1, {"a": 11, "b": 12}[name[-1]], 1.0, STEPS[name]
    if name == "fine-grid":
        return make_scenario("C1", num_tips=40, num_sites=1000, uncertain_tips=0.3, seed=77), None, None, 2, 13, 1.0 / 8, STEPS[name]
    if name == "steep":
        return steep_scenario(), None, None, 2, 2, None, STEPS[name]      # (seed 2: the partition cuts at S)
    if name == "on-a-bound":
        return on_a_bound_scenario(), None, None, 1, 7, None, STEPS[name]
    if name == "zero-slope":
        return zero_slope_scenario(), None, None, 1, 3, None, STEPS[name]
    raise KeyError(name)


STEPS = {"C1/1": 500, "C1/6": 250, "C2/1": 120, "C2/6": 100, "C3/1": 30, "C3/6": 40, "random": 150,
         "high-mutation/a": 350, "high-mutation/b": 300, "fine-grid": 500, "steep": 300, "zero-slope": 200, "on-a-bound": 150}
CASES = ["C1/1", "C1/6", "C2/1", "C2/6", "C3/1", "C3/6"] + ["random%d" % k for k in range(12)] + ["high-mutation/a", "high-mutation/b", "fine-grid"]
# what CASES do not reach of the draws (tests/draws_model.py): test_draws_model.py runs these on the oracle, test_draws_model_gpu.py on the device
DRAW_CASES = ["steep", "zero-slope", "on-a-bound"]
TOPOLOGY_OFF = ("steep", "on-a-bound")      # (the draw that picks the move spans 30 there)
_done = {}


def prepare(name):
    sc, nu_l, evo, nparts, seed, tf, steps = _case(name)
    parts, incl, seeds, root_part, ref = split_parts(sc, nparts, seed)
    t_step = sc.default_t_step() * tf if tf is not None else 1.0

    def setup(engine):
        configure(engine, sc, ref, parts, incl, seeds, root_part, t_step, topology=name not in TOPOLOGY_OFF, nu_l=nu_l, evo=evo)
        return engine
    return sc, parts, incl, ref, X.Evo.of(sc, nu_l, evo), X.Pop(sc.pop), steps, setup


def run_case(name, make_engine, who, steps_divisor=1):
    sc, parts, incl, ref, ev, pop, steps, setup = prepare(name)
    steps = max(steps // steps_divisor, 1)
    tally, cov = Tally(who), M.Coverage()
    eng = setup(make_engine(sc.num_sites, steps + 8))
    try:
        M.run_stepped(tally, cov, eng, sc, parts, incl, ref, ev, pop, steps, tag=name, topology=name not in TOPOLOGY_OFF)
    finally:
        eng.close()
    return tally, cov


def _oracle(num_sites, trace):
    return OracleEngine(num_sites, trace_moves=trace)


@pytest.mark.parametrize("name", ["C1/6", "random3", "fine-grid"])
def test_the_stepped_chain_is_the_chain(name):
    """300 passes of one move against one pass of 300 moves: traces, trees, totals bit for bit and the same number of draws."""
    sc, parts, incl, ref, ev, pop, steps, setup = prepare(name)
    M.assert_stepped_chain_is_the_chain(lambda: setup(_oracle(sc.num_sites, 300)), len(parts), 300)


@pytest.mark.parametrize("name", ["C1/6", "random1", "random4", "random8", "high-mutation/b", "fine-grid"])
def test_exact_deltas_equal_the_difference_of_the_exact_totals(name):
    """partial_log_prior_delta and part_log_G_delta on pairs of states 1, 3, 20 and 150 moves apart (topology moves and grid growth
    among them): the delta IS full(after) - full(before), as Fractions, and its S is no larger than the two totals' together."""
    sc, parts, incl, ref, ev, pop, steps, setup = prepare(name)
    eng = setup(_oracle(sc.num_sites, 0))
    pairs = 0
    try:
        for gap in (1, 1, 1, 3, 3, 20, 150):
            before = [eng.part_download(p) for p in range(len(parts))]
            eng.run_moves_per_part(gap, threads=1)
            for p in range(len(parts)):
                after, tab = eng.part_download(p), eng.part_coalescent(p)
                if M.trees_identical(before[p], after):
                    continue
                dP = X.partial_log_prior_delta(before[p], after, pop, incl[p], tab)
                fB, fA = X.partial_log_prior(before[p], pop, incl[p], tab), X.partial_log_prior(after, pop, incl[p], tab)
                assert dP.value == fA.value - fB.value, (name, gap, p, float(dP.value), float(fA.value - fB.value))
                assert dP.S <= fA.S + fB.S
                dG = X.part_log_G_delta(before[p], after, ref, ev, incl[p])
                gB, gA = X.Derived(before[p], ref, ev).part_log_G(incl[p]), X.Derived(after, ref, ev).part_log_G(incl[p])
                assert dG.value == gA.value - gB.value, (name, gap, p, float(dG.value), float(gA.value - gB.value))
                assert dG.S <= gA.S + gB.S
                pairs += 1
    finally:
        eng.close()
    assert pairs >= 3, pairs


def test_assert_valid_part_refuses_broken_trees():
    sc = make_scenario("C1", num_tips=30, num_sites=600, uncertain_tips=0.3, seed=5)
    M.assert_valid_part(sc.tree, sc.ref)
    import copy
    tips = np.flatnonzero(sc.tree.child0 < 0)
    inner = [x for x in np.flatnonzero(sc.tree.child0 >= 0) if x != sc.tree.root]
    branch = next(x for x in range(sc.tree.num_nodes) if x != sc.tree.root and sc.tree.mut_offset[x + 1] > sc.tree.mut_offset[x])
    k = int(sc.tree.mut_offset[branch])

    def broken(edit):
        t = copy.deepcopy(sc.tree)
        edit(t)
        with pytest.raises(AssertionError):
            M.assert_valid_part(t, sc.ref)
    broken(lambda t: t.parent.__setitem__(inner[0], tips[0]))
    broken(lambda t: t.t.__setitem__(inner[0], t.t[t.parent[inner[0]]]))
    broken(lambda t: t.mut_t.__setitem__(k, t.t[t.parent[branch]]))
    broken(lambda t: t.mut_t.__setitem__(k, np.nextafter(t.t[branch], np.inf)))
    broken(lambda t: t.mut_from.__setitem__(k, (t.mut_from[k] + 1) % 4 if (t.mut_from[k] + 1) % 4 != t.mut_to[k] else (t.mut_from[k] + 2) % 4))
    broken(lambda t: t.t.__setitem__(tips[0], float(t.t_max[tips[0]]) + 1.0))
    if sc.tree.miss_start.shape[0] > 0 and sc.tree.miss_offset[-1] > 0:
        broken(lambda t: t.miss_end.__setitem__(0, t.miss_start[0]))


@pytest.mark.parametrize("name", CASES)
def test_oracle_every_move_against_the_exact_posterior(name, record_property):
    tally, cov = _done[name] = run_case(name, _oracle, "oracle")
    for k, v in cov.as_dict().items():
        record_property("coverage_" + k, v)
    tally.finish(record_property)
    assert cov.unchecked == 0, cov.as_dict()


def test_oracle_cases_cover_what_they_must(record_property):
    """The conditions that keep this file honest, over all its cases (a case not run in this session is run here)."""
    total = M.Coverage()
    for name in CASES:
        if name not in _done:
            _done[name] = run_case(name, _oracle, "oracle")
        total.add(_done[name][1])
    for k, v in total.as_dict().items():
        record_property("coverage_" + k, v)
    print("coverage:", total.as_dict())
    total.assert_conditions()
    assert total.rejected_topology >= 50, total.as_dict()
