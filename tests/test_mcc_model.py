"""tests/mcc_model.py: derive_mcc_tree to the letter (a) against the definitions (b), and both against cases worked by hand.

The reference has no unit test of core/mcc_tree.cpp; these two restatements, written from different ends (fingerprints, counts and a
walk by node times; sets of tips and inclusion), are the yardstick tests/test_mcc_gpu.py holds the device against."""
import collections
import math
import os
import random

import numpy as np

import mcc_model as M

NO = -1


def tree_from_newick_like(spec, times):
    """spec: nested pairs of tip indices, e.g. ((0, 1), (2, 3)); inner nodes are numbered after the tips in post order; times: {node: t}."""
    parent, c0, c1 = {}, {}, {}
    num_tips = [0]

    def count(s):
        if isinstance(s, int): num_tips[0] = max(num_tips[0], s + 1)
        else: count(s[0]); count(s[1])
    count(spec)
    nxt = [num_tips[0]]

    def build(s):
        if isinstance(s, int):
            c0[s] = c1[s] = NO
            return s
        a, b = build(s[0]), build(s[1])
        v = nxt[0]; nxt[0] += 1
        c0[v], c1[v] = a, b; parent[a] = parent[b] = v
        return v
    root = build(spec); parent[root] = NO
    n = nxt[0]
    arr = lambda dct: np.array([dct[v] for v in range(n)], np.int32)
    return M.Sample(arr(parent), arr(c0), arr(c1), np.array([times[v] for v in range(n)], float), root)


# tips A, B, C, D = 0, 1, 2, 3 at time 0; inner nodes 4, 5 (the cherries, in the order written) and 6 (the root)
def four_tip_samples():
    s0 = tree_from_newick_like(((0, 1), (2, 3)), {0: 0, 1: 0, 2: 0, 3: 0, 4: -1.0, 5: -2.0, 6: -5.0})
    s1 = tree_from_newick_like(((0, 1), (2, 3)), {0: 0, 1: 0, 2: 0, 3: 0, 4: -3.0, 5: -1.0, 6: -6.0})
    s2 = tree_from_newick_like(((0, 2), (1, 3)), {0: 0, 1: 0, 2: 0, 3: 0, 4: -1.5, 5: -2.5, 6: -4.0})
    return [s0, s1, s2]


def check_four_tips(r: M.Mcc):
    """((A,B),(C,D)) twice and ((A,C),(B,D)) once."""
    assert r.master == 0
    assert list(r.num_exact) == [3, 3, 3, 3, 2, 2, 3]
    assert list(r.support) == [1.0, 1.0, 1.0, 1.0, 2.0 / 3.0, 2.0 / 3.0, 1.0]
    # a cherry's t: the mean of the two samples that have it; its t_mrca: the mean over three, the third sample's ROOT standing in
    assert r.t[4] == (-1.0 + -3.0) / 2 and r.t[5] == (-2.0 + -1.0) / 2 and r.t[6] == (-5.0 + -6.0 + -4.0) / 3
    assert r.t_mrca[4] == (-1.0 + -3.0 + -4.0) / 3 and r.t_mrca[5] == (-2.0 + -1.0 + -4.0) / 3 and r.t_mrca[6] == r.t[6]
    assert list(r.corr[2]) == [0, 1, 2, 3, 6, 6, 6] and list(r.exact[2]) == [True] * 4 + [False, False, True]
    assert list(r.corr[1]) == list(range(7)) and r.exact[1].all()
    # log cc: samples 0 and 1 have two clades of count 2 and the root (3); sample 2 two clades of count 1 and the root
    want01 = 2 * (math.log(2) - math.log(3)); want2 = 2 * (math.log(1) - math.log(3))
    assert abs(r.log_cc[0] - want01) < 1e-15 and r.log_cc[0] == r.log_cc[1] and abs(r.log_cc[2] - want2) < 1e-15
    assert all(tt == 0 for tt in r.t[:4]) and all(tt == 0 for tt in r.t_mrca[:4])


def test_three_samples_of_four_tips_worked_by_hand():
    check_four_tips(M.derive_letter(four_tip_samples(), 1))
    check_four_tips(M.derive_sets(four_tip_samples()))


def test_one_sample():
    s = four_tip_samples()[2]
    for r in (M.derive_letter([s], 3), M.derive_sets([s])):
        assert r.master == 0 and r.log_cc == [0.0] and list(r.num_exact) == [1] * 7 and list(r.support) == [1.0] * 7
        assert np.array_equal(r.t, s.t) and np.array_equal(r.t_mrca, s.t) and list(r.corr[0]) == list(range(7)) and r.exact.all()


def test_identical_samples():
    s = four_tip_samples()
    ss = [s[0], s[1], s[0].copy(), s[1].copy()]
    for r in (M.derive_letter(ss, 5), M.derive_sets(ss)):
        assert r.master == 0 and r.log_cc == [0.0] * 4 and list(r.support) == [1.0] * 7 and r.exact.all()
        assert r.t[4] == (-1.0 + -3.0 + -1.0 + -3.0) / 4 and np.array_equal(r.t, r.t_mrca)


def test_two_tips():
    a = tree_from_newick_like((0, 1), {0: 0.5, 1: 0.25, 2: -1.0})
    b = tree_from_newick_like((1, 0), {0: 0.5, 1: 0.25, 2: -2.0})
    for r in (M.derive_letter([a, b], 9), M.derive_sets([a, b])):
        assert r.master == 0 and r.log_cc == [0.0, 0.0] and list(r.support) == [1.0] * 3 and list(r.t) == [0.5, 0.25, -1.5] and list(r.t_mrca) == [0.5, 0.25, -1.5]


def test_the_walk_by_times_finds_the_mrca_when_times_are_equal():
    # all inner nodes at one time: find_MRCA_of's last branch (phylo_tree.cpp:228-265)
    s = tree_from_newick_like((((0, 1), (2, 3)), (4, 5)), {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: -1, 7: -1, 8: -1, 9: -1, 10: -1})
    assert M.find_mrca_by_times(s, 6, 7) == 8 and M.find_mrca_by_times(s, 6, 9) == 10 and M.find_mrca_by_times(s, 0, 3) == 8 and M.find_mrca_by_times(s, 6, 8) == 8


def sweep_case(seed, max_tips, max_samples):
    rng = random.Random(seed)
    ss = M.random_sample_set(rng, max_tips, max_samples)
    for s in ss: M.check_times(s)
    return ss


def test_to_the_letter_against_the_definitions_on_random_sample_sets():
    """A few hundred seeded sets (2-60 tips, 1-40 samples, SPR-perturbed, a quarter with integer node times).  Everything but log_cc must be
    EQUAL, the sums in sample order bit for bit; log_cc within the bound of mcc_model.log_cc_bound; the master as expected_master says."""
    base = int(os.environ.get("EMAT_FUZZ_SEED", "1000"))
    kinds = collections.Counter(); below_one = 0; equal_time_sets = 0
    for case in range(int(os.environ.get("EMAT_FUZZ_CASES", "300"))):
        ss = sweep_case(base + case, 60, 40)
        n_inner = len(ss[0].inner_nodes())
        b = M.derive_sets(ss)
        a_free = M.derive_letter(ss, case)
        want, by_bound = M.expected_master(a_free, n_inner)
        kinds[M.tie_kind(ss, a_free, n_inner)] += 1
        assert b.master == want, (case, b.master, want, a_free.master)
        if not by_bound: assert a_free.master == want
        a = M.derive_letter(ss, case, master=b.master)
        assert a.inner_counts == b.inner_counts, case
        assert np.array_equal(a.corr, b.corr) and np.array_equal(a.exact, b.exact), case
        assert np.array_equal(a.num_exact, b.num_exact) and np.array_equal(a.support, b.support), case
        assert np.array_equal(a.t, b.t) and np.array_equal(a.t_mrca, b.t_mrca), case
        for k in range(len(ss)):
            assert abs(a.log_cc[k] - b.log_cc[k]) <= M.log_cc_bound(n_inner, a.log_cc_terms_abs[k]), (case, k)
        below_one += bool((b.support < 1).any())
        equal_time_sets += any(len(set(s.t[s.inner_nodes()])) < n_inner for s in ss)
    print("master decided by:", dict(kinds), "; sets with a support < 1:", below_one, "; sets with equal inner-node times:", equal_time_sets)
    assert kinds["rounding"] == 0 and kinds["gap"] > 0 and kinds["same topology"] > 0
    if "EMAT_FUZZ_SEED" not in os.environ: assert below_one > 200 and equal_time_sets > 30


GPU_SWEEP_SEED = 6202       # tests/test_mcc_gpu.py: case k of the device sweep is sweep_case(GPU_SWEEP_SEED * 1000 + k, 400, 64)
GPU_SWEEP_CASES = 200


def test_no_master_of_the_device_sweep_is_decided_by_rounding():
    """tests/test_mcc_gpu.py names the master by expected_master.  Of the committed device sweep no case may be decided by rounding: where
    the best log_cc is not alone within the bound, everything within the bound is an EXACT tie -- the same histogram of clade counts, which
    the same topology implies and which every pair of different trees at M = 2 has too -- so that the first index is the answer in any
    arithmetic that sums the same terms."""
    kinds = collections.Counter()
    for case in range(GPU_SWEEP_CASES):
        ss = sweep_case(GPU_SWEEP_SEED * 1000 + case, 400, 64)
        kinds[M.tie_kind(ss, M.derive_letter(ss, case), len(ss[0].inner_nodes()))] += 1
    print("device sweep, master decided by:", dict(kinds))
    assert kinds["rounding"] == 0
