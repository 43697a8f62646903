"""tests/samples_site_states_model.py held to the reference's own site-state fixtures, and its generator to the condition the
reference asserts of a tree's mutations.  No GPU."""
import random

import numpy as np
import pytest

import mcc_model
import prober_model as M
import samples_site_states_model as SS
from prober_golden import G, check_prober_case, flat_tree, pop_model


@pytest.mark.parametrize("case", G["site_states_tree_prober"], ids=lambda c: c["test"])
def test_the_reference_fixtures_as_three_identical_samples(case):
    tree, ref = flat_tree(case["tree"])
    s = SS.MutSample(tree, tree.mut_offset, tree.mut_site, tree.mut_from, tree.mut_to, tree.mut_t, ref)
    SS.check_state_chain(s, times=False)
    pop = pop_model(case["pop"])
    args = (case["t_start"], case["t_end"], case["num_t_cells"])
    p, mean, stats, skip, tol = SS.model_batched([s, s, s], [pop], [case["site"], case["site"]], *args, ranks=[0, 2])
    assert p.shape == (3, 2, 4, case["num_t_cells"]) and mean.shape == p.shape[1:] and stats.shape == (2,) + p.shape[1:]
    want = M.probe_site_states_on_tree(tree, ref, M.OraclePop(pop), case["site"], *args)
    for k in range(3):
        for i in range(2):
            check_prober_case(case, p[k, i], "%s, sample %d, entry %d" % (case["test"], k, i))
            assert p[k, i].tobytes() == want.tobytes()
    assert stats[0].tobytes() == p[0].tobytes() and stats[1].tobytes() == p[0].tobytes()      # three equal values: every rank is that value
    assert np.max(np.abs(mean - p[0])) <= 2.0 ** -52                                         # (a + a + a) / 3 is a to the last bit or so
    assert len(set(skip.tolist())) == 1 and np.all(tol >= 1e-12)


def test_the_generators_sets_satisfy_the_state_chain_the_reference_asserts():
    kinds = set()
    for case, (tips, pushed, first, stride, cells, spec, split) in enumerate(SS.gpu_cases()):
        ss, special = SS.sample_set(case + 1, tips, pushed)
        assert len(ss) == pushed and len(set(special.values())) == 3
        for s in ss:
            assert s.n == 2 * tips - 1 and s.ref.shape == (SS.NUM_SITES,)
            SS.check_state_chain(s)
            mcc_model.check_times(s.topology())
            r = s.root
            on_root = s.mut_site[s.mut_offset[r]:s.mut_offset[r + 1]]
            assert on_root.size >= 1 and np.all(on_root == special["root"])                    # the root's own list changes that site and no other
            assert not np.any(s.mut_site == special["never"])
            tip_hit = [v for v in range(s.n) if s.child0[v] < 0 and v != r and special["tip"] in s.mut_site[s.mut_offset[v]:s.mut_offset[v + 1]]]
            assert tip_hit or s.n == 1
            twice = any(np.unique(s.mut_site[s.mut_offset[v]:s.mut_offset[v + 1]]).size < s.mut_offset[v + 1] - s.mut_offset[v] for v in range(s.n))
            kinds.add(("twice on a list", twice)); kinds.add(("two on the root", on_root.size == 2))
        sites = SS.sites_of(spec, special)
        assert 1 <= len(sites) <= 5 and all(0 <= x < SS.NUM_SITES for x in sites)
    assert kinds == {("twice on a list", True), ("twice on a list", False), ("two on the root", True), ("two on the root", False)}
    specs = "".join(c[5] for c in SS.gpu_cases())
    assert {"n", "r", "t"} <= set(specs) and any(len(set(c[5])) < len(c[5]) for c in SS.gpu_cases())      # the special sites and a repeated one
    nodes = {2 * c[0] - 1 for c in SS.gpu_cases()}
    assert {3, 255, 257, 511, 513} <= nodes and {1, 100} <= {c[1] for c in SS.gpu_cases()} and {1, 1000} <= {c[4] for c in SS.gpu_cases()}


def test_the_model_accepts_the_generators_sets():
    """The reference side stays within every precondition by itself: no branch ends before it starts, every site is in range."""
    import delphy_amd as d
    split_seen = 0
    for case, (tips, pushed, first, stride, cells, spec, split) in enumerate(SS.gpu_cases()):
        if tips > 12 or pushed > 9 or cells > 65: continue                                     # (the large ones run on the GPU test's machine)
        ss, special = SS.sample_set(case + 1, tips, pushed)
        chosen = ss[first::stride]
        t_start, t_end = SS.window(chosen, random.Random(1000 + case), split)
        sites = SS.sites_of(spec, special)
        p, mean, stats, skip, tol = SS.model_batched(chosen, [d.PopModel.const(1.5)], sites, t_start, t_end, cells, ranks=[0, len(chosen) - 1])
        assert np.all(p >= 0.0) and np.all(p <= 1.0 + 1e-12) and np.all(np.abs(p.sum(axis=2) - 1.0) <= 1e-12)
        assert np.all(stats[0] <= mean + 1e-15) and np.all(mean <= stats[1] + 1e-15)
        split_seen += len(set(skip.tolist())) > 1
    assert split_seen >= 3
