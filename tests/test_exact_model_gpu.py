"""The HIP engine against the exact values of tests/exact_model.py: the comparisons of test_exact_model.py with the device in
place of the oracle, plus the device's population-model code on inputs the reference's fixtures do not reach and the
coalescent tables the kernels build for the tree resident in HBM.  Each quantity is held to (n + 8) u S of its exact value
(exact_model's docstring); a device and an oracle that made the same mistake would both fail here."""
import numpy as np
import pytest

import delphy_amd as d
import exact_model as X
from delphy_amd.scenarios import make_scenario, random_scenario
from helpers import split_parts
from test_exact_model import CONFIGS, Tally, check_part, check_popsize_bar, check_stats, oracle_against_exact

pytestmark = pytest.mark.gpu


def test_device_population_models_on_adversarial_inputs(record_property):
    """k_debug_pop (emat_debug_pop): pop_at_time and pop_integral against the exact values."""
    b = d.EmatBackend(100)
    tally = Tally("device")
    try:
        for name, pm, a, bb in X.adversarial_pop_cases():
            pop = X.Pop(pm)
            integ = b.debug_pop(pm, 1, a, bb)
            at = b.debug_pop(pm, 0, a, a)
            for i in range(a.shape[0]):
                tally.check("pop_integral", pop.pop_integral(float(a[i]), float(bb[i])), integ[i], "%s [%r, %r]" % (name, a[i], bb[i]))
                tally.check("pop_at_time", pop.pop_at_time(float(a[i])), at[i], "%s t=%r" % (name, a[i]))
    finally:
        b.close()
    tally.finish(record_property)


@pytest.mark.parametrize("name,use_lds", [(n, True) for n in sorted(CONFIGS)] + [("C3", False)])
def test_device_derived_quantities_and_maintained_totals_against_exact(name, use_lds, record_property):
    """k_recalc_derived (part_derived from scratch and after recalc_derived), what k_run_moves maintained in a pass, the part grids,
    k_global_stats and k_num_muts_l: whole tree (with k_scalable_prior) and parts."""
    tally = Tally("device")
    sc = CONFIGS[name]()
    oracle_against_exact(tally, sc, 1, 1500, 3, grid_prior=True, engine=d.EmatBackend(sc.num_sites, use_lds=use_lds))
    oracle_against_exact(tally, sc, 6, 1500, 5, engine=d.EmatBackend(sc.num_sites, use_lds=use_lds))
    tally.finish(record_property)


def test_device_large_parts_in_the_side_class_against_exact(record_property):
    """C3 cut by the reference's rule (max_part_nodes = 0) into three parts of about 2 000 nodes each, with the main launch's LDS
    area sized for 16 parts per CU as a large partition's is (the parts_per_cu option): these parts' fixed-size prefixes do not
    fit it, so they run as giants in k_run_moves_side.  The test asserts that they do."""
    tally = Tally("device")
    sc = make_scenario("C3", num_tips=3000, num_sites=3000)
    b = d.EmatBackend(sc.num_sites)
    b.set_option("parts_per_cu", 16)
    side, root = [], []

    def classes(e, n):
        side.extend(np.flatnonzero(~np.asarray(e.main_class_mask(n), bool)).tolist())
    n = oracle_against_exact(tally, sc, 3, 1000, 9, engine=b, max_part_nodes=0, after_pass=classes)
    _, _, _, root_part, _ = split_parts(sc, 3, 9, 0)
    record_property("side_class_parts", side)
    tally.finish(record_property)
    assert [p for p in side if p != root_part], "no part other than the root part (%d) of %d ran in a side class: %s" % (root_part, n, side)


def test_device_random_scenarios_against_exact(record_property):
    """random_scenario's cases 0-11 (every population kind, site rates, two partitions, tip-date uncertainty), LDS and HBM-resident."""
    tally = Tally("device")
    for case in range(12):
        rng = np.random.default_rng(7300 + case)
        sc, nu_l, evo, what = random_scenario(rng, case, max_tips=160)
        nparts = int(rng.integers(1, 6))
        t_step = sc.default_t_step() * float(rng.choice([0.5, 1.0, 3.0]))
        before = len(tally.fail)
        oracle_against_exact(tally, sc, nparts, 600, 11 + case, nu_l=nu_l, evo=evo, t_step=t_step, grid_prior=(nparts == 1),
                             engine=d.EmatBackend(sc.num_sites, use_lds=bool(case % 2)))
        if len(tally.fail) > before:
            tally.fail.insert(before, "-- " + what)
    tally.finish(record_property)


def _whole_tree_checks(tally, b, run, sc, ev, pop, ref, tag):
    """What the device computes for the WHOLE tree from its parts -- EmatRun.Ttwiddle_l, global_stats, num_muts_l, the grid prior
    directly and staged -- against the exact values of the parts it holds (the statistics do not depend on the cut)."""
    n, root_part = run.num_parts()
    trees = [b.part_download(p) for p in range(n)]
    tot = check_stats(tally, b, trees, ref, ev, tag)
    got = run.Ttwiddle_l()
    for l in range(got.shape[0]):
        tally.check("Ttwiddle_l", tot["Ttwiddle_l"][l], got[l], "%s site %d" % (tag, l))
    run.reassemble()
    whole, ref = run.tree()
    t_ref = float(np.max(whole.t[whole.child0 == -1]))
    t_step = sc.default_t_step()
    ex = X.scalable_log_prior(whole, pop, t_ref, t_step)
    tally.check("scalable_prior", ex, b.scalable_coalescent_log_prior(t_ref, t_step), tag)
    _, _, first = b.scalable_coalescent_partial(t_ref, t_step, 0, 0)
    kb, logs, _ = b.scalable_coalescent_partial(t_ref, t_step, first - 3, 3 - first)
    tally.check("scalable_prior_staged", ex, b.scalable_coalescent_log_prior_from_grid(t_ref, t_step, first - 3, kb, logs), tag)


@pytest.mark.parametrize("device_tree", [False, True])
def test_device_whole_tree_statistics_and_resident_tree_tables_against_exact(device_tree, record_property):
    """Two cycles of the run driver (C3, site rates, 24 parts).  With the tree resident in HBM the parts and their coalescent
    tables are cut and built by kernels (k_gt_coal_*): every part's k_bar_p must be the exact time-integral of its lineage
    count per cell and popsize_bar the exact pop_integral / t_step of every cell it is active in."""
    tally = Tally("device")
    sc = make_scenario("C3", num_tips=700, num_sites=3000, uncertain_tips=0.2)
    nu = 0.25 + 1.5 * np.random.default_rng(3).random(sc.num_sites)
    ev, pop = X.Evo.of(sc, nu), X.Pop(sc.pop)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, 71)
    run.set_num_parts(24); run.set_hky(sc.mu, sc.kappa, sc.pi, nu); run.set_pop_model(sc.pop)
    run.set_device_tree(device_tree)
    try:
        for cyc in range(2):
            _, ref = run.tree()                   # the sequence the parts are written against (repartition keeps it)
            run.repartition()
            n, root_part = run.num_parts()
            for p in range(n):
                check_part(tally, b, p, ref, ev, pop, p == root_part, "cycle %d from scratch" % cyc)
                check_popsize_bar(tally, b, p, pop, "cycle %d" % cyc)
            if cyc > 0:
                run.run_moves(n * 800); b.synchronize()
            _whole_tree_checks(tally, b, run, sc, ev, pop, ref, "cycle %d" % cyc)
    finally:
        run.close(); b.close()
    tally.finish(record_property)


def _full_size_against_exact(tally, sc, num_parts, seed, max_part_nodes, moves, sample_every, device_tree):
    """A full-size configuration cut by the run driver (max_part_nodes as bench.py's --max-part-nodes): every `sample_every`-th
    part and the root part -- lambda_i, log G, partial prior, k_bar_p and popsize_bar of every active cell -- from scratch, as
    the pass maintained them, and recomputed after it."""
    ev, pop = X.Evo.of(sc), X.Pop(sc.pop)
    b = d.EmatBackend(sc.num_sites)
    run = d.EmatRun(b, sc.tree, sc.ref, seed)
    try:
        run.set_num_parts(num_parts); run.set_max_part_nodes(max_part_nodes)
        run.set_hky(sc.mu, sc.kappa, sc.pi); run.set_pop_model(sc.pop); run.set_device_tree(device_tree)
        _, ref = run.tree()
        run.repartition()
        n, root_part = run.num_parts()
        sample = sorted(set(range(0, n, sample_every)) | {root_part})
        scales = {}
        for p in sample:
            exG, exA, _ = check_part(tally, b, p, ref, ev, pop, p == root_part, "from scratch")
            scales[p] = (abs(exG.f), abs(exA.f))
            check_popsize_bar(tally, b, p, pop, "from scratch")
        run.run_moves(n * moves); b.synchronize()
        for p in sample:
            assert b.part_stats(p)["status"] == 0 and b.part_stats(p)["moves_done"] == moves
            check_part(tally, b, p, ref, ev, pop, p == root_part, "maintained", scales[p], moves)
        b.recalc_derived()
        for p in sample:
            check_part(tally, b, p, ref, ev, pop, p == root_part, "after a pass", moves=moves)
        return n
    finally:
        run.close(); b.close()


@pytest.mark.parametrize("max_part_nodes", [0, -1])
def test_device_c3_full_size_every_part_against_exact(max_part_nodes, record_property):
    """Config C3 whole (10 000 tips, 29 903 sites, skygrid), 400 parts requested, the tree in HBM: every part, under the
    reference's cut (0) and bench.py's default cut (-1, whose large parts get further cut nodes)."""
    tally = Tally("device")
    n = _full_size_against_exact(tally, make_scenario("C3"), 400, 101, max_part_nodes, 1000, 1, True)
    record_property("parts", n)
    tally.finish(record_property)


@pytest.mark.parametrize("max_part_nodes", [0, -1])
def test_device_c4_sampled_parts_against_exact(max_part_nodes, record_property):
    """Config C4 (100 000 tips) with the benchmark's 8 192 parts requested and seed, under the reference's cut (0, 7 955 parts) and
    bench.py's own (-1, 8 092 parts): every 97th part plus the root part, the sample test_c4_incremental_totals_match_recomputation_and_oracle
    takes, 300 moves per part."""
    tally = Tally("device")
    n = _full_size_against_exact(tally, make_scenario("C4"), 8192, 20261001, max_part_nodes, 300, 97, False)
    record_property("parts", n)
    tally.finish(record_property)
